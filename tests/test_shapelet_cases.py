"""CPU: the NumPy statement of the shapelet rule (tests/shapelet_cases.py) against what the reference
computed on the same seeded cases (tests/golden/shapelet_ref.npz, scripts/gen_shapelet_golden.py), and
the edge cases of shapelet_cases.py: that each has the sizes, block counts and ties its comment claims."""
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


# ------------------------------------------------------------------ the edge cases of shapelet_cases.py:
# each does what its comment claims (tests/test_gpu_shapelet.py runs them on the device)
T, TR, TC, DC = sc.T, sc.TR, sc.TC, sc.DC


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_edge_case_digests():
    got = sc.edge_digests()
    assert got == sc.EDGE_DIGESTS, {k: v for k, v in got.items() if sc.EDGE_DIGESTS.get(k) != v}


def test_sliding_cases_cross_the_workgroup_where_said():
    m = sc.SLIDING_M
    for name, total in sc.SLIDING_TOTALS.items():
        lens = sc.sliding_lengths(name)
        assert sum(lens) == total and min(lens) >= m and len(set(lens)) > 3, name
    off = np.cumsum([0] + sc.sliding_lengths("ends_at_T"))
    assert T in off[1:-1] and off[-1] > T + m            # a sequence begins at row T
    off = np.cumsum([0] + sc.sliding_lengths("straddles_T"))
    j = int(np.searchsorted(off, T, side="right")) - 1   # the sequence of row T
    assert off[j] < T - 1 and off[j + 1] - m == T - 1    # its last window starts at T - 1 ...
    assert m > 1 and off[j + 1] > T                      # ... and rows T .. off[j + 1] - 1 have none
    lens = sc.sliding_lengths("300_short")
    assert len(lens) == 300 and set(lens) == {m, m + 1, m + 2} and sum(lens) > 4 * T
    for name in sc.SLIDING_CASES:
        pat, seqs = sc.sliding_case(name)
        assert pat.shape == (m, sc.SLIDING_D) and [len(y) for y in seqs] == sc.sliding_lengths(name)
        assert len(sc.sliding_distance(pat, seqs)) == sum(len(y) for y in seqs) - len(seqs) * (m - 1)


def _num_with_later_sample_first(s_row, labels):
    """candidate_score's num with the tie among equal keys turned round (k descending)."""
    n = len(labels)
    key, _ = sc.pair_keys(s_row, n)
    order = np.lexsort((-np.arange(n), key))
    negs = int(n - np.count_nonzero(labels))
    correct = num = negs
    for k in order:
        correct += 1 if labels[k] else -1
        num = max(num, correct)
    return num


def test_score_label_cases_have_the_ties_they_claim():
    assert sc.SCORE_LABEL_SIZES == [T - 1, T, T + 1, 2 * T + 3, sc.MAXSEQ]
    for n in sc.SCORE_LABEL_SIZES:
        rows, labels = sc.score_case("labels_%d" % n)
        nums, losses, w = sc.score_expected("labels_%d" % n)
        assert rows.shape == (6, n) and labels.shape == (n,) and 0 < labels.sum() < n
        assert len(np.unique(rows)) <= 56 and (rows[1] == rows[1, 0]).all()
        pairs = sc.score_pairs(n)
        assert (len(pairs) == 0) == (n <= T) and (n < 2 * T or len(pairs) == 16)
        for a, b, v in pairs:
            assert b - a in (T, T + 1) and labels[a] != labels[b]
            for q in (0, 2, 3, 4, 5):  # the pair's value is the pair's alone
                assert np.array_equal(np.nonzero(rows[q] == np.float32(v))[0], [a, b])
        if n >= 2 * T:
            assert {b - a for a, b, _ in pairs} == {T, T + 1}
        # the order inside the ties decides num: turned round, some row scores differently
        turned = [_num_with_later_sample_first(row, labels) for row in rows]
        assert any(t != v for t, v in zip(turned, nums)), n
        assert len(set(nums.tolist())) > 1


def test_score_label_edge_cases():
    rows, labels = sc.score_case("all_positive")
    assert labels.all() and len(labels) == T + 1
    assert (sc.score_expected("all_positive")[0] == T + 1).all()
    rows, labels = sc.score_case("one_positive")
    assert labels.sum() == 1 and labels[T] == 1 and len(labels) == T + 1
    nums, losses, _ = sc.score_expected("one_positive")
    assert np.array_equal(losses, np.sqrt(rows[:, T]).astype(np.float64))
    # row 1's keys are all equal and the positive is the last sample: num is negs, not negs + 1
    assert (rows[1] == rows[1, 0]).all() and nums[1] == T
    assert _num_with_later_sample_first(rows[1], labels) == T + 1
    rows, labels = sc.score_case("all_keys_equal")
    assert rows.shape[1] == 2 * T + 3 and (rows == rows[0, 0]).all() and 0 < labels.sum() < len(labels)
    nums = sc.score_expected("all_keys_equal")[0]
    assert nums[0] != _num_with_later_sample_first(rows[0], labels)  # only k orders the samples


def test_score_mirror_cases_have_smaller_equal_and_larger_copies_past_T():
    assert sc.SCORE_MIRROR_SIZES == [T + 5, sc.MAXSEQ // 2]
    for n in sc.SCORE_MIRROR_SIZES:
        rows, labels = sc.score_case("mirror_%d" % n)
        assert rows.shape == (6, 2 * n) and len(labels) == n
        nums, losses, _ = sc.score_expected("mirror_%d" % n)
        assert any(sc.candidate_score(row[:n], labels)[0] != v for row, v in zip(rows, nums))  # num reads the minimum
        for q, row in enumerate(rows):
            a, b = u32(row[:n])[T:], u32(row[n:])[T:]
            assert (b < a).any() and (b == a).any() and (b > a).any()
            key, mirrored = sc.pair_keys(row, n)
            assert not mirrored[T:][b == a].any() and mirrored[T:][b < a].all()  # the original on a tie
            pm = np.where(mirrored, row[n:], row[:n])
            num_pm, loss_pm = sc.candidate_score(pm, labels)
            assert num_pm == nums[q] and loss_pm != losses[q]       # the loss reads the unmirrored values
            assert losses[q] == sc.candidate_score(row[:n], labels)[1]


def test_select_cases_tie_as_they_claim():
    assert sc.SELECT_SIZES == [T - 1, T, T + 1, 2 * T + 7]
    assert sorted(v[0] for v in sc.SELECT_TIES.values()) == sorted(sc.SELECT_SIZES + [2 * T + 7] * 2)
    for n_cand in sc.SELECT_SIZES:
        rows, labels = sc.score_case("select_last_%d" % n_cand)
        nums, losses, w = sc.score_expected("select_last_%d" % n_cand)
        assert len(rows) == n_cand and w == n_cand - 1 and (nums[:w] < nums[w]).all()
    for name, (n_cand, members) in sc.SELECT_TIES.items():
        rows, labels = sc.score_case(name)
        nums, losses, w = sc.score_expected(name)
        assert len(rows) == n_cand and w == members[0] == min(members), name
        for q in members[1:]:
            assert np.array_equal(u32(rows[q]), u32(rows[w]))  # identical rows, not merely equal sums
            assert nums[q] == nums[w] and losses[q:q + 1].view(np.uint64) == losses[w:w + 1].view(np.uint64)
        others = np.setdiff1d(np.arange(n_cand), members)
        assert (nums[others] < nums[w]).all(), name           # the tie is for the first place
    q, a, b = sc.SELECT_TIES["select_tie_%d" % (2 * T + 7)][1]
    assert q < T and (a, b) == (q + T, q + T + 1)
    first, other = sc.SELECT_TIES["select_tie_first_past_T"][1]
    assert T <= first < other and first % T > other % T        # the later member sits in the lower thread
    first, other = sc.SELECT_TIES["select_tie_lower_thread_later"][1]
    assert first < T <= other and first % T > other % T
    first, other = sc.SELECT_TIES["select_tie_%d" % (T + 1)][1]
    assert other == T and first % T > other % T
    n_cand, planted = sc.SELECT_NUM_TIE
    nums, losses, w = sc.score_expected("select_num_tie")
    rows_ = [q for q, _ in planted]
    assert w == rows_[-1] and len(set(nums[rows_].tolist())) == 1 and (np.diff(losses[rows_]) < 0).all()
    assert (nums[np.setdiff1d(np.arange(n_cand), rows_)] < nums[w]).all()
    assert rows_[0] % T == rows_[1] % T and rows_[1] % T != rows_[2] % T  # one thread's two trips, and another's


def _blocks(n, edge):
    return -(-n // edge)


def test_mindist_cases_meet_the_blocks_they_claim():
    assert sc.MINDIST_LONG_M == [TC + 1, 2 * TC + 3, sc.MAXM]
    assert [(_blocks(P, TR), _blocks(P, TC)) for P in sc.MINDIST_LONG_P] == [(1, 1), (1, 1), (1, 1), (2, 2), (3, 3)]
    assert TR - 1 in sc.MINDIST_LONG_P and TR in sc.MINDIST_LONG_P
    for m in sc.MINDIST_LONG_M:
        seqs, mm, cands = sc.mindist_case("long_m%d" % m)
        assert mm == m > TC and seqs[0].shape[1] == DC + 1 and cands == list(range(len(seqs)))
        assert [len(y) - m + 1 for y in seqs] == sc.MINDIST_LONG_P
    assert [D % DC for D in sc.MINDIST_CHUNK_D] == [0, 0, DC - 1] and sc.MINDIST_CHUNK_D[:2] == [DC, 2 * DC]
    for D in sc.MINDIST_CHUNK_D:
        seqs, m, cands = sc.mindist_case("chunks_D%d" % D)
        assert seqs[0].shape[1] == D and m == 3 and len(seqs[0]) == m and len(seqs[2]) - m + 1 > TC
    seqs, m, cands = sc.mindist_case("max_D")
    assert seqs[0].shape[1] == sc.MAXD and m == 2 and len(seqs) == 3
    seqs, m, cands = sc.mindist_case("workload")
    assert (m, seqs[0].shape[1], len(seqs)) == (25, 92, 6) and all(60 <= len(y) <= 90 for y in seqs)
    assert cands == list(range(6))
    seqs, m, cands = sc.mindist_case("300_seqs")
    assert len(seqs) == 300 and {len(y) for y in seqs} == {m, m + 1, m + 2, m + 3} and len(cands) == 3
    seqs, m, cands = sc.mindist_case("max_seq")
    assert len(seqs) == sc.MAXSEQ and {len(y) for y in seqs} == {1, 2} and (m, seqs[0].shape[1]) == (1, 1)
    assert len(cands) == 3
    # the long tie: the planted window's s is 0 at one place in each of three position blocks
    seqs, m, cands = sc.mindist_case("long_tie")
    assert m == TC + 5 and [p // TC for p in sc.LONG_TIE_PLACES] == [0, 1, 2]
    s = sc.s_matrix(seqs[0], seqs[1], m)
    assert np.array_equal(np.nonzero(s[1] == 0)[0], sc.LONG_TIE_PLACES)
    min2, loc = sc.mindist_expected("long_tie")
    assert min2[1, 1] == 0 and loc[1, 1] == sc.LONG_TIE_PLACES[0]


def _dis64(seqs, cands, m):
    """sqrt of the minimum over c of s(r, c), every term and sum in float64: [n_cand, n_seq]."""
    out = []
    for i in cands:
        x = np.asarray(seqs[i], np.float64)
        R = len(x) - m + 1
        rows = np.empty((R, len(seqs)))
        for j, y in enumerate(seqs):
            y = np.asarray(y, np.float64)
            P = len(y) - m + 1
            e = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
            s = np.zeros((R, P))
            for k in range(m):
                s += e[k:k + R, k:k + P]
            rows[:, j] = s.min(1)
        out.append(rows)
    return np.sqrt(np.concatenate(out))


def test_real_valued_mindist_cases_are_no_further_from_float64_than_the_reference(ref):
    """The bar of test_distances_are_no_further_from_float64_than_the_reference: the reference's own
    maximum absolute error of dis against float64 over the fixture.  The statement's sqrt(min2) of
    every real-valued edge case stays within it."""
    bound = max(float(np.abs(ref["set%d_dis" % n] - ref["set%d_dis64" % n]).max()) for n in range(len(sc.GOLDEN_SETS)))
    worst = 0.0
    for name in sc.MINDIST_REAL:
        seqs, m, cands = sc.mindist_case(name)
        min2, _ = sc.mindist_expected(name)
        err = float(np.abs(np.sqrt(min2) - _dis64(seqs, cands, m)).max())
        print("%s: max abs error of dis against float64 %.3g (bar %.3g)" % (name, err, bound))
        worst = max(worst, err)
        assert err <= bound, name
    report("shapelet edge cases vs float64, max abs error of dis: %.3g (the reference's over the fixture: %.3g)"
           % (worst, bound))


def test_find_cases_cut_and_tie_where_said():
    # more candidates than one default chunk; the winner is not row 0 and ties fully with a later chunk's row
    seqs, labels, m = sc.find_case("default_chunks")
    want = sc.find_expected("default_chunks")
    lens = [len(y) for y in seqs]
    chunks = sc.chunk_table(lens, labels, m, sc.DEFAULT_CANDS)
    assert want["n_cand"] > sc.DEFAULT_CANDS and len(chunks) == 2
    assert sum(e[2] for e in chunks[0]) == sc.DEFAULT_CANDS
    w = sc.select(want["nums"], want["losses"])
    full = (want["nums"] == want["nums"][w]) & (want["losses"] == want["losses"][w])
    assert 0 < w < sc.DEFAULT_CANDS and full[sc.DEFAULT_CANDS:].any() and not full[:w].any()
    # the planted full tie, in one chunk and in two
    seqs, labels, m = sc.find_case("tie")
    want = sc.find_expected("tie")
    a, b = sc.TIE_FIND_ROWS
    assert want["nums"][a] == want["nums"][b] == want["nums"].max()
    assert want["losses"][a:a + 1].view(np.uint64) == want["losses"][b:b + 1].view(np.uint64)
    rest = np.setdiff1d(np.arange(want["n_cand"]), [a, b])
    assert ((want["nums"][rest] < want["nums"][a]) | (want["losses"][rest] > want["losses"][a])).all()
    assert sc.select(want["nums"], want["losses"]) == a and (want["shapeindex"], want["cand"]) == (1, a)
    lens = [len(y) for y in seqs]
    assert len(sc.chunk_table(lens, labels, m, sc.DEFAULT_CANDS)) == 1
    chunks = sc.chunk_table(lens, labels, m, sc.TIE_FIND_SPLIT)
    assert a < sc.TIE_FIND_SPLIT <= b < 2 * sc.TIE_FIND_SPLIT and sc.TIE_FIND_SPLIT % TR
    assert chunks[0][-1][:2] == (1, TR) and chunks[1][0][:2] == (1, sc.TIE_FIND_SPLIT)  # a block of clip 1 is cut
    # the cut cases: a unique winner in a chosen entry of the table
    assert sc.CUT_CANDS % TR
    entries = {"cut_second_block": (0, 1), "cut_after_cut": (1, 0), "cut_next_clip": (1, 1)}  # (chunk, entry)
    for name, (clip, start) in sc.CUT_WINNERS.items():
        seqs, labels, m = sc.find_case(name)
        want = sc.find_expected(name)
        assert (want["shapeindex"], want["cand"]) == (clip, start), name
        w = sc.select(want["nums"], want["losses"])
        rest = np.delete(np.arange(want["n_cand"]), w)
        assert ((want["nums"][rest] < want["nums"][w]) | (want["losses"][rest] > want["losses"][w])).all()
        chunks = sc.chunk_table([len(y) for y in seqs], labels, m, sc.CUT_CANDS)
        assert len(chunks) == 3
        ci, ei = entries[name]
        i, r0, n, out0 = chunks[ci][ei]
        assert i == clip and r0 <= start < r0 + n, name
        assert w == sum(sum(e[2] for e in c) for c in chunks[:ci]) + out0 + start - r0
    assert chunks[0][1][1:3] == (TR, sc.CUT_CANDS - TR) and chunks[1][0][1] == sc.CUT_CANDS  # the cut block
    assert chunks[1][1][3] > 0


def test_feature_cases_have_the_edges_they_claim():
    R = sc.FEAT_ROWS
    assert sc.FEATURE_LENGTHS["empty"][0] == 0 and sc.FEATURE_LENGTHS["empty"][-1] == 0
    assert sc.FEATURE_LENGTHS["empty"][2:4] == [0, 0]
    assert sum(sc.FEATURE_LENGTHS["L_rows"]) == R and sum(sc.FEATURE_LENGTHS["L_rows+1"]) == R + 1
    assert sc.FEATURE_LENGTHS["300_rows"] == [1] * 300
    for joints in (18, 60):
        # an empty sequence contributes nothing: the statement equals itself without the empty ones
        mot, lengths = sc.feature_case("empty", joints)
        for mode in (0, 1, 2):
            a = sc.motion_features(mot, lengths, mode)
            b = sc.motion_features(mot, [n for n in lengths if n], mode)
            assert len(a) == len(mot) and np.array_equal(u32(a), u32(b))
        mot, lengths = sc.feature_case("carry", joints)
        off = np.cumsum([0] + lengths)
        assert off[1] < R < off[2] and off[3] == 2 * R
        xy = mot[:, :, :2].astype(np.float32).reshape(len(mot), -1)
        s1 = sc.fill_forward(xy[off[1]:off[2]])
        assert (s1[:, 4] == 0).all()                           # joint 2, x: the refused carry, the zeros stay
        assert sc.fill_forward(xy[:off[2]])[R, 4] == np.float32(123.5)    # (it would have filled them)
        assert (xy[R:off[2], 6] == 0).all() and (s1[R - off[1]:, 6] == np.float32(234.5)).all()  # joint 3: accepted
        s3 = sc.fill_forward(xy[off[3]:])
        assert (s3[:3, 8] == 0).all() and sc.fill_forward(xy)[off[3], 8] == np.float32(345.5)    # joint 4: refused
        n3 = sc.fill_nearby(xy[off[3]:])
        assert xy[off[3], 10] == 0 and n3[0, 10] == np.float32(56.5)      # joint 5: r + 1, not the row before
        assert sc.fill_nearby(xy)[off[3], 10] == np.float32(456.5)
        n2 = sc.fill_nearby(xy[off[2]:off[3]])
        assert (n2[-2:, 12] == np.float32(67.5)).all()                    # joint 6: r - 1 / r - 2, not the rows after
        assert sc.fill_nearby(xy)[off[3] - 1, 12] == np.float32(567.5)
        for mode in (0, 1, 2):
            assert not np.array_equal(sc.motion_features(mot, lengths, mode), sc.motion_features(mot, None, mode))
