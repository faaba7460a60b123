"""CPU: the cases of tests/shapelet_scan_cases.py have the geometry they claim (which hits fall on
which tile, word or step boundary, which path's LDS condition holds, how many occurrences), the
statement's walk gives the hand-derived occurrences of the dictated profiles, and the host helpers
of src/augment.py reproduce the reference goldens of tests/golden/shapelet_scan_ref.npz with
shapelet_scan replaced by the statement."""
import json
import os

import numpy as np
import pytest

import shapelet_cases as sc
import shapelet_scan_cases as cs
from conftest import GOLDEN

F32 = np.float32


# ---------------------------------------------------------------- the pick profiles
@pytest.mark.parametrize("name", cs.PICK_CASES)
def test_walk_gives_the_hand_derived_occurrences(name):
    for dist, off, m, sigma, want in cs.pick_calls(name):
        occ, pos, d = cs.pick(dist, off, m, sigma)
        assert occ[0] == 0 and len(occ) == len(off) and occ[-1] == len(pos) == len(d)
        if want is None:
            continue
        for j, entries in enumerate(want):
            assert pos[occ[j]:occ[j + 1]].tolist() == [c for c, _ in entries], (name, j)
            assert d[occ[j]:occ[j + 1]].tolist() == [F32(v) for _, v in entries], (name, j)


def test_pick_profiles_sit_where_they_claim():
    dist, off, m, sigma, _ = cs.pick_case("word_boundary")
    hits = np.nonzero(dist < sigma)[0]
    assert hits.min() < 64 <= hits.max()                        # two mask words
    dist, off, m, sigma, _ = cs.pick_case("step_boundary")
    assert off[-1] == 64 * 64 + 70
    hits = np.nonzero(dist < sigma)[0]
    run = hits[(hits > 100) & (hits < cs.STEP_ROWS + 30)]
    assert run.min() < cs.STEP_ROWS <= run.max() and np.all(np.diff(run) == 1)   # one run over the 64-word step
    dist, off, m, sigma, _ = cs.pick_case("all_hits")
    assert np.all(dist < sigma)
    dist, off, m, sigma, _ = cs.pick_case("no_hits")
    assert not np.any(dist < sigma)
    dist, off, m, sigma, _ = cs.pick_case("mid_word")
    assert off[1] % 64 != 0 and off[1] < 64                      # stream 1 starts inside the first word
    assert np.all(dist[off[1] - (m - 1):off[1]] < sigma)         # the predecessor's tail rows are below sigma
    dist, off, m, sigma, _ = cs.pick_case("two_in_word")
    assert off[-1] <= 64
    dist, off, m, sigma, _ = cs.pick_case("at_sigma")
    assert np.count_nonzero(dist == sigma) == 2 and np.count_nonzero(dist < sigma) == 1
    dist, off, m, sigma, _ = cs.pick_case("empty_and_short")
    assert sorted(set(np.diff(off).tolist()) & {0, m - 1, m}) == [0, m - 1, m]


def test_runs_are_longer_than_two_windows():
    for name in ("falling_run", "rising_run", "equal_run"):
        for dist, off, m, sigma, want in cs.pick_calls(name):
            hits = np.nonzero(dist < sigma)[0]
            assert len(hits) > 2 * m and np.all(np.diff(hits) == 1)
            d = dist[hits]
            if name == "falling_run":
                assert np.all(np.diff(d) < 0) and len(want[0]) == 1 and want[0][0][0] == hits[-1]
            else:
                assert np.all(np.diff(d) > 0) if name == "rising_run" else np.all(d == d[0])
                assert np.all(np.diff([c for c, _ in want[0]]) == m // 2 + 1) and want[0][0][0] == hits[0]


# ---------------------------------------------------------------- the distance cases
def test_constants_name_a_consistent_kernel():
    assert cs.TC % 64 == 0 and cs.THREADS % cs.TC == 0 and cs.PG % (cs.THREADS // cs.TC) == 0
    assert 2 * cs.LDS_BYTES <= 160 * 1024                        # two workgroups per CU
    assert cs.lds_bytes(39, 92) <= cs.LDS_BYTES                  # the reference's lengths at D = 92 stay in LDS


def test_distance_cases_have_their_geometry():
    pats, sig, seqs = cs.dist_case("tile_edges")
    lens = [len(y) for y in seqs]
    m = len(pats[0])
    assert {cs.TC - 1, cs.TC, cs.TC + 1, 2 * cs.TC + 1, m - 1, m, 0} <= set(lens)
    assert [len(cs.dist_case(n)[0]) for n in ("one_pattern", "full_group", "group_plus_one")] == [1, cs.PG, cs.PG + 1]
    pats, sig, seqs = cs.dist_case("mixed_lengths")
    assert sorted(len(p) for p in pats) == [1, 2, 37, cs.MAXM] and len(pats) <= cs.PG
    assert any(len(y) < 37 for y in seqs) and any(len(y) > cs.TC for y in seqs)
    for D in (1, 4, 7, 92):
        assert cs.dist_case("D%d" % D)[2][0].shape[1] == D
    assert cs.takes_lds_path(cs.dist_case("lds_fits")[0]) and not cs.takes_lds_path(cs.dist_case("lds_over")[0])
    assert max(len(p) for p in cs.dist_case("lds_over")[0]) == max(len(p) for p in cs.dist_case("lds_fits")[0]) + 1
    pats, sig, seqs = cs.dist_case("global_max")
    assert not cs.takes_lds_path(pats) and pats[0].shape == (cs.MAXM, cs.MAXD) and len(seqs[0]) < 2 * cs.TC
    for n in cs.DIST_CASES:
        if n not in ("lds_over", "global_max"):
            assert cs.takes_lds_path(cs.dist_case(n)[0]), n
    assert len(cs.dist_case("long_stream")[2][0]) == 64 * 64 + 70
    assert max(len(y) for n in cs.DIST_CASES for y in cs.dist_case(n)[2]) == 64 * 64 + 70
    assert len(cs.dist_case("chunks")[0]) > 2


@pytest.mark.parametrize("name", [n for n in cs.DIST_CASES if n != "global_max"])
def test_distance_cases_have_occurrences_and_thinned_runs(name):
    pats, sig, seqs = cs.dist_case(name)
    occ, pos, dist = cs.dist_expected(name)
    assert len(occ) == len(pats) * len(seqs) + 1 and occ[-1] == len(pos) > 0
    hits = sum(int(np.count_nonzero(cs.distances(p, y) < s)) for p, s in zip(pats, sig) for y in seqs)
    assert hits >= len(pos)
    if name not in ("integer_planted", "one_pattern"):
        assert hits > len(pos), "no run of neighbouring hits was thinned"
    for q, p in enumerate(pats):  # streams without a position have no occurrence
        for j, y in enumerate(seqs):
            if len(y) < len(p):
                assert occ[q * len(seqs) + j] == occ[q * len(seqs) + j + 1]


def test_integer_case_hits_exact_values():
    pats, sig, seqs = cs.dist_case("integer_planted")
    occ, pos, dist = cs.dist_expected("integer_planted")
    n = len(seqs)
    first = dist[occ[0]:occ[n]]
    assert len(first) == 3 and np.all(first == 0)                # the three copies, and nothing else below 0.5
    assert (pos[occ[0]:occ[1]] == [30, cs.TC - 3]).all()         # one of them across the tile edge
    all_d = np.concatenate([cs.distances(pats[1], y) for y in seqs])
    assert np.any(all_d == 3)                                    # dist == sigma exists and is no hit
    assert sorted(dist[occ[n]:occ[2 * n]].tolist()) == [0, 0, 0, 2]
    assert pos[occ[n + 1]:occ[n + 2]].tolist() == [10, 38]
    assert occ[2 * n] == occ[3 * n]                              # sigma 0: nothing


def test_long_stream_has_hits_on_both_sides_of_the_step():
    occ, pos, dist = cs.dist_expected("long_stream")
    first = pos[occ[0]:occ[1]]
    assert first.min() < cs.STEP_ROWS <= first.max()


# ---------------------------------------------------------------- src/augment.py against the reference
@pytest.fixture(scope="module")
def golden():
    path = os.path.join(GOLDEN, "shapelet_scan_ref.npz")
    return np.load(path), json.load(open(path[:-4] + ".json"))


@pytest.fixture()
def augment(monkeypatch):
    """src.augment with the device calls replaced by the NumPy statements."""
    from src import augment as aug

    def scan(patterns, sigmas, seq, off, **kw):
        occ, pos, dist = cs.scan(patterns, sigmas, [seq[a:b] for a, b in zip(off[:-1], off[1:])])
        return {"off": occ, "pos": pos, "dist": dist}

    def features(motion, datamode=None, featuremode=0, lengths=None, handle=None):
        return sc.motion_features(motion, lengths, featuremode)

    monkeypatch.setattr(aug._shapelet, "shapelet_scan", scan)
    monkeypatch.setattr(aug._shapelet, "MotionJointFeatures", features)
    return aug


def check_against_golden(golden, name, got, videos):
    data, meta = golden
    assert 0 < meta["dist_rtol"] < 2e-6
    assert list(got) == list(videos)
    for vk in videos:
        pairs = got[vk]
        assert [p for p, _ in pairs] == data["%s_%s_pos" % (name, vk)].tolist(), (name, vk)
        np.testing.assert_allclose([d for _, d in pairs], data["%s_%s_dist" % (name, vk)], rtol=meta["dist_rtol"], atol=0)


@pytest.mark.parametrize("seed,m,fm,seg", cs.AUG_CASES)
def test_augmentate_one_shapelet_gives_the_reference_occurrences(augment, golden, seed, m, fm, seg):
    pattern, sigma = cs.aug_case(seed, m, fm)
    name = cs.aug_name(seed, m, fm, seg)
    assert golden[0]["%s_sigma" % name] == sigma
    videos = cs.aug_videos(seed)
    got = augment.AugmentateOneShapelet(pattern, sigma, videos, "posehand", fm, MaxSegLength=seg)
    check_against_golden(golden, name, got, videos)


def test_segments_are_the_reference_segments():
    from src import augment as aug
    assert aug.segments(150, 15, None) == [(0, 150)]
    assert aug.segments(150, 15, 64) == [(0, 64), (49, 128), (113, 150)]
    assert aug.segments(128, 15, 64) == [(0, 64), (49, 128)]
    assert aug.segments(0, 15, 64) == []


def test_a_segment_shorter_than_the_pattern_contributes_nothing(augment):
    """(A later segment starts m rows early, so only a video shorter than the pattern makes one.)"""
    full = cs.aug_videos(0)["v1"]
    pattern, sigma = cs.aug_case(0, 24, 2)
    for seg in (None, 64):
        videos = {"short": full[:23], "long": full[:66], "none": full[:0]}
        got = augment.AugmentateOneShapelet(pattern, F32(1e9), videos, "posehand", 2, MaxSegLength=seg)
        assert got["short"] == [] and got["none"] == [] and len(got["long"]) > 0
        assert all(p <= 66 - 24 for p, _ in got["long"])


@pytest.mark.parametrize("seed", cs.PATTERN_RECORD_SEEDS)
@pytest.mark.parametrize("mode", [0, 1])
def test_get_shapelet_pattern_gives_the_reference_list(golden, seed, mode):
    from src import augment as aug
    rec = cs.pattern_record(seed)
    got = aug.GetShapeletPattern(rec, mode=mode, scale=0.3)
    assert [int(k) for k, _, _ in got] == golden[0]["pattern%d_mode%d_keys" % (seed, mode)].tolist()
    assert [F32(s) for _, _, s in got] == golden[0]["pattern%d_mode%d_sigmas" % (seed, mode)].tolist()
    assert all(isinstance(k, str) for k, _, _ in got)
    assert len(got) == (len(rec) if mode == 0 else 1)
    for k, shapelet, _ in got:
        assert np.array_equal(shapelet, rec[int(k)]["shapelet"])


def test_data_augmentate_cuts_the_window_and_stores_the_reference_arrays(augment, golden):
    """One word whose record holds the found window's clip index: the result per level key equals
    AugmentateOneShapelet on the window cut by hand, as arrays float64 [n, 2] or shape (0,)."""
    seed, fm = 0, 1
    videos = cs.aug_videos(seed)
    key, a, b = cs.AUG_CLIP
    clips = {"word": (["v1", key], np.array([[0, 30], [a, b]]))}
    dists = np.linspace(1, 30, 10).astype(F32)
    records = {"word": {m: {"locs": np.array([3, cs.AUG_LOC], np.int16), "dists": dists,
                            "shapelet": np.array([1], np.int16), "score": np.array([0.8], F32)} for m in (9, 15)}}
    got = augment.DataAugmentate(records, videos, clips, "posehand", fm, mode=0, scale=0.3)
    assert list(got) == ["word/15", "word/9"]                    # the reference's key order: as strings
    for m in (9, 15):
        pattern, _ = cs.aug_case(seed, m, fm)
        want = augment.AugmentateOneShapelet(pattern, dists[3], videos, "posehand", fm)
        for vk in videos:
            arr = got["word/%d" % m][vk]
            assert arr.dtype == np.float64 and arr.shape == ((len(want[vk]), 2) if want[vk] else (0,))
            assert np.array_equal(arr, np.array(want[vk]))
        assert sum(len(v) for v in want.values()) > 0
    empty = augment.DataAugmentate({"word": {9: dict(records["word"][9], dists=np.full(10, 1e-9, F32))}}, videos, clips,
                                   "posehand", fm)
    assert all(v.shape == (0,) for k, v in empty["word/9"].items() if k != key)
