"""CPU: the NumPy statement of the shapelet rule (tests/shapelet_cases.py) against what the reference
computed on the same seeded cases (tests/golden/shapelet_ref.npz, scripts/gen_shapelet_golden.py)."""
import os

import numpy as np
import pytest

import shapelet_cases as sc
from conftest import GOLDEN, report


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "shapelet_ref.npz"))


@pytest.fixture(scope="module")
def trained():
    """The statement's train() on every golden set, once."""
    out = []
    for args in sc.GOLDEN_SETS:
        seqs, labels = sc.make_set(*args)
        out.append((seqs, labels, args[3], sc.train(seqs, labels, args[3])))
    return out


def test_features_equal_the_reference_bit_for_bit(ref):
    for n, (seed, lengths, joints) in enumerate(sc.GOLDEN_MOTION):
        mot = sc.make_motion(seed, lengths, joints)
        for mode in (0, 1, 2):
            ours = sc.motion_features(mot, lengths, mode)
            want = ref["motion%d_mode%d" % (n, mode)]
            assert ours.dtype == want.dtype == np.float32 and ours.shape == want.shape
            assert np.array_equal(ours.view(np.uint32), want.view(np.uint32)), (n, mode)


def test_features_do_not_cross_a_clip_boundary():
    mot = sc.make_motion(5, [6, 6], 18, zero_frac=0.0)
    mot[4:8, 3, 0] = 0  # a run of zeros across the boundary: rows 4, 5 fill from row 3, rows 6, 7 stay
    both = sc.motion_features(mot, [6, 6], 0)
    assert np.array_equal(both[:6], sc.motion_features(mot[:6], None, 0))
    assert np.array_equal(both[6:], sc.motion_features(mot[6:], None, 0))
    assert not np.array_equal(both, sc.motion_features(mot, None, 0))


def test_winner_locs_and_score_equal_the_reference(ref, trained):
    for n, (seqs, labels, m, ours) in enumerate(trained):
        assert ours["shapeindex"] == int(ref["set%d_shapeindex" % n]), n
        assert ours["cand"] == int(ref["set%d_cand" % n]), n
        assert np.array_equal(ours["locs"], ref["set%d_locs" % n]), n
        assert ours["score"] == float(ref["set%d_score" % n]), n


def test_distances_are_no_further_from_float64_than_the_reference(ref, trained):
    """Maximum absolute error against float64 over the whole fixture, ours <= the reference's, for
    the sliding distances and for the winner's dis.  No margin."""
    err = {"sd_ours": 0.0, "sd_ref": 0.0, "dis_ours": 0.0, "dis_ref": 0.0}
    for n, (seqs, labels, m, ours) in enumerate(trained):
        sd64, dis64 = ref["set%d_sd64" % n], ref["set%d_dis64" % n]
        sd = sc.sliding_distance(seqs[0][:m], seqs)
        err["sd_ours"] = max(err["sd_ours"], float(np.abs(sd - sd64).max()))
        err["sd_ref"] = max(err["sd_ref"], float(np.abs(ref["set%d_sd" % n] - sd64).max()))
        err["dis_ours"] = max(err["dis_ours"], float(np.abs(ours["dis"] - dis64).max()))
        err["dis_ref"] = max(err["dis_ref"], float(np.abs(ref["set%d_dis" % n] - dis64).max()))
    line = "shapelet statement vs float64, max abs error: " + ", ".join("%s %.3g" % kv for kv in err.items())
    print(line)
    report(line)
    assert err["sd_ours"] <= err["sd_ref"]
    assert err["dis_ours"] <= err["dis_ref"]


def test_two_positives_tie_goes_to_the_first_candidate():
    """With exactly two positive clips the two windows that are each other's nearest have the same
    distances to each other, bit for bit (e is symmetric), so they tie whenever the other clips
    rank alike: built here with integers, shown as a tie, and resolved to the first."""
    rng = np.random.default_rng(11)
    m, D = 3, 2
    pat = rng.integers(-4, 5, (m, D)).astype(np.float32)
    seqs = [rng.integers(20, 30, (7, D)).astype(np.float32) for _ in range(5)]
    labels = np.array([0, 1, 0, 1, 0], np.uint8)
    seqs[1][2:5] = pat
    seqs[3][1:4] = pat
    res = sc.find(seqs, labels, m)
    P1 = len(seqs[1]) - m + 1
    a, b = 2, P1 + 1  # the planted windows' candidate rows
    assert res["nums"][a] == res["nums"][b] == res["nums"].max()
    assert res["losses"][a] == res["losses"][b] == res["losses"][res["nums"] == res["nums"].max()].min()
    assert (res["shapeindex"], res["cand"]) == (1, 2)
    # the symmetry behind it: s(r, c) of (x, y) is s(c, r) of (y, x), bit for bit
    s = sc.s_matrix(seqs[1], seqs[3], m)
    assert np.array_equal(s.view(np.uint32), sc.s_matrix(seqs[3], seqs[1], m).T.view(np.uint32))


@pytest.mark.parametrize("mode", ["x-mirror", "y-mirror"])
def test_mirror_call_is_a_normal_call_over_the_doubled_set_then_the_pair_minimum(mode):
    seqs, labels = sc.make_set(21, 8, 4, 5, 3, max_extra=10)
    n, m = len(seqs), 5
    got = sc.train(seqs, labels, m, mirror=mode)
    doubled = seqs + sc.mirror_copies(seqs, mode)
    min2, loc = sc.mindist(doubled, [i for i in range(n) if labels[i]], m)
    # the pair minimum first, then the plain (unmirrored) scoring of n samples; the loss is over the
    # originals' own distances
    take = min2[:, n:].view(np.uint32) < min2[:, :n].view(np.uint32)
    pm = np.where(take, min2[:, n:], min2[:, :n])
    nums = np.array([sc.candidate_score(row, labels)[0] for row in pm])
    losses = np.array([sc.candidate_score(row, labels)[1] for row in min2[:, :n]])
    w = sc.select(nums, losses)
    rows = [(i, r) for i in range(n) if labels[i] for r in range(len(seqs[i]) - m + 1)]
    assert (got["shapeindex"], got["cand"]) == rows[w]
    assert got["num"] == nums[w] and got["loss"] == losses[w]
    assert np.array_equal(got["mirrored"], take[w])
    assert np.array_equal(got["dis"], np.sqrt(pm[w]))
    assert np.array_equal(got["locs"], np.where(take[w], loc[w, n:], loc[w, :n]))
    assert got["mirrored"].any() and not got["mirrored"].all()
