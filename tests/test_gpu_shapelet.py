"""GPU: the shapelet search (csrc/shapelet.hip, src/shapelet.py) against the NumPy statement of
tests/shapelet_cases.py.  Every comparison is bit equality.  The edge lengths come from the tile
constants of csrc/shapelet.h, so they follow the code."""
import os
import re

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

import shapelet_cases as sc
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu


def _constants():
    src = open(os.path.join(REPO, "pytorch-openpose_amd", "csrc", "shapelet.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}


K = _constants()
TR, TC, DC, MAXM, MAXD, MAXSEQ, FEAT_ROWS = (K[k] for k in ("kShpTR", "kShpTC", "kShpDC", "kShpMaxM", "kShpMaxD",
                                                              "kShpMaxSeq", "kFeatRows"))
SUB = K["kShpThreads"] // TR  # threads that share one candidate start's positions
T, DEFAULT_CANDS = K["kShpThreads"], K["kShpDefaultCands"]
assert K == sc.K  # the edge cases of shapelet_cases.py are cut to the same constants


@pytest.fixture(scope="module")
def sh():
    from src import shapelet
    return shapelet


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ragged(seqs):
    return (np.ascontiguousarray(np.concatenate(seqs), np.float32),
            np.cumsum([0] + [len(y) for y in seqs]).astype(np.int64))


def random_seqs(seed, lengths, D, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        return [rng.integers(-4, 5, (n, D)).astype(np.float32) for n in lengths]
    return [rng.standard_normal((n, D)).astype(np.float32) for n in lengths]


def check_mindist(sh, seqs, m, cands=None, want=None):
    cands = list(range(len(seqs))) if cands is None else cands
    seq, off = ragged(seqs)
    min2, loc = sh.shapelet_mindist(seq, off, m, cands)
    want2, wantloc = want or sc.mindist(seqs, cands, m)
    assert min2.shape == want2.shape
    assert np.array_equal(bits(min2), bits(want2))
    assert np.array_equal(loc, wantloc)
    return min2, loc


def check_find(sh, seqs, labels, m, max_cands=0, want=None):
    seq, off = ragged(seqs)
    got = sh.shapelet_find(seq, off, labels, m, max_cands, every=True)
    want = want or sc.find(seqs, labels, m)
    assert got["best"].tolist() == [want["shapeindex"], want["cand"], want["num"], want["n_cand"]]
    assert got["loss"][0] == want["loss"]
    assert np.array_equal(got["nums"], want["nums"])
    assert np.array_equal(got["losses"].view(np.uint64), want["losses"].view(np.uint64))
    assert np.array_equal(bits(got["dis"]), bits(want["dis"]))
    assert np.array_equal(got["locs"], want["locs"])
    return got, want


# ---------------------------------------------------------------- 1. the distance stage
@pytest.mark.parametrize("m,D,n_seq", [(1, 1, 1), (2, 3, 2), (15, 92, 2), (MAXM, DC + 1, 2), (1, DC + 1, 9), (2, 92, 9),
                                       (15, 1, 9), (MAXM, 3, 1)])
def test_mindist_sizes(sh, m, D, n_seq):
    rng = np.random.default_rng(m * 1000 + D)
    lengths = [m] + [int(v) for v in rng.integers(m, m + 12, n_seq - 1)]
    check_mindist(sh, random_seqs(m + D, lengths, D), m)


def test_mindist_block_edges(sh):
    """A sequence of exactly m rows; candidate blocks and position blocks at extent - 1, extent and
    extent + 1; a target that spans three position blocks."""
    m = 3
    P = sorted({1, TR - 1, TR, TR + 1, TC - 1, TC, TC + 1, 2 * TC + 3})
    check_mindist(sh, random_seqs(7, [p + m - 1 for p in P], 5), m)


def test_mindist_lower_location_wins_a_tie_across_blocks(sh):
    m, D = 4, 3
    seqs = random_seqs(9, [m + 2, 2 * TC + 20], D, integer=True)
    seqs[1][:] += 50  # nothing else comes near the planted window
    # the same window in three position blocks; positions 2, 2 + SUB and TC + 2 fall to one thread
    # (within a block and across blocks), the others to other threads of the same start
    places = (2, 2 + max(SUB, m), TC + 2, TC + 2 + m + 3, 2 * TC + 7)
    assert all(b - a >= m for a, b in zip(places, places[1:]))
    for p in places:
        seqs[1][p:p + m] = seqs[0][1:1 + m]
    min2, loc = check_mindist(sh, seqs, m, cands=[0])
    assert min2[1, 1] == 0 and loc[1, 1] == 2


def test_profile_mode_agrees_with_mindist_mode(sh):
    m = 5
    seqs = random_seqs(13, [m, TC + 9, 2 * TC + 1], 7)
    seq, off = ragged(seqs)
    min2, loc = check_mindist(sh, seqs, m)
    handle = sh.default_handle()
    from src._native import lib
    row = 0
    for i, x in enumerate(seqs):
        for r in (0, len(x) - m):
            pat = np.ascontiguousarray(x[r:r + m])
            dist = np.empty(len(seq) - len(seqs) * (m - 1), np.float32)
            handle.check(lib.opose_sliding_distance(handle.h, pat.ctypes.data, m, seq.ctypes.data, off.ctypes.data,
                                                    len(seqs), seq.shape[1], dist.ctypes.data, 0))
            assert np.array_equal(bits(dist), bits(sc.sliding_distance(pat, seqs)))
            q = row + r
            for j in range(len(seqs)):
                prof = dist[off[j] - j * (m - 1):off[j + 1] - (j + 1) * (m - 1)]
                assert prof.min() == np.sqrt(min2[q, j]) and prof[loc[q, j]] == prof.min()
        row += len(x) - m + 1
    one = sh.SlidingDistance(seqs[1][3:3 + m], seqs[2])
    assert np.array_equal(bits(one), bits(sc.sliding_distance(seqs[1][3:3 + m], [seqs[2]])))


# ---------------------------------------------------------------- 2. score, selection, the whole search
def test_find_equals_mindist_then_debug_score(sh):
    seqs, labels = sc.make_set(31, 9, 3, 4, 4, integer=True, max_extra=8)
    seq, off = ragged(seqs)
    got, want = check_find(sh, seqs, labels, 4)
    cands = [i for i in range(len(seqs)) if labels[i]]
    min2, loc = sh.shapelet_mindist(seq, off, 4, cands)
    from src._native import lib
    handle = sh.default_handle()
    n_cand = len(min2)
    nums, losses = np.empty(n_cand, np.int32), np.empty(n_cand, np.float64)
    winner, wloss = np.empty(4, np.int32), np.empty(1, np.float64)
    handle.check(lib.opose_debug_shapelet_score(handle.h, min2.ctypes.data, n_cand, len(seqs), labels.ctypes.data,
                                                len(labels), nums.ctypes.data, losses.ctypes.data,
                                                winner.ctypes.data, wloss.ctypes.data))
    assert np.array_equal(nums, got["nums"]) and np.array_equal(losses, got["losses"])
    w = int(winner[1])
    assert winner.tolist() == [0, w, int(got["best"][2]), n_cand] and wloss[0] == got["loss"][0]
    assert w == sc.select(want["nums"], want["losses"])
    assert np.array_equal(bits(np.sqrt(min2[w])), bits(got["dis"])) and np.array_equal(loc[w], got["locs"])


@pytest.mark.parametrize("seed", [41, 42])
def test_find_in_three_chunks_equals_one_chunk(sh, seed):
    seqs, labels = sc.make_set(seed, 7, 3, 3, 3, max_extra=TR + 6)
    one, want = check_find(sh, seqs, labels, 3)
    third = -(-want["n_cand"] // 3)
    assert third < want["n_cand"] and -(-want["n_cand"] // third) == 3
    three, _ = check_find(sh, seqs, labels, 3, max_cands=third)
    for k in one:
        assert np.array_equal(one[k], three[k]), k


def test_identical_clips_with_different_labels_tie_on_the_index(sh):
    seqs, labels = sc.make_set(51, 6, 2, 3, 2, integer=True, max_extra=5)
    pos, neg = int(np.nonzero(labels)[0][0]), int(np.nonzero(labels == 0)[0][0])
    seqs[neg] = seqs[pos].copy()  # equal distances to every candidate: k breaks the tie in the order
    got, want = check_find(sh, seqs, labels, 3)
    row = want["min2"][sc.select(want["nums"], want["losses"])]
    assert bits(row)[pos] == bits(row)[neg]
    # and with the pair's labels exchanged, so both orders of (positive, negative) are met
    swapped = labels.copy()
    swapped[[pos, neg]] = swapped[[neg, pos]]
    check_find(sh, seqs, swapped, 3)


@pytest.mark.parametrize("n_pos", [1, 6])
def test_one_positive_and_all_positive(sh, n_pos):
    seqs, labels = sc.make_set(60 + n_pos, 6, 3, 2, n_pos, integer=True, max_extra=6)
    got, want = check_find(sh, seqs, labels, 2)
    assert want["num"] == 6 if n_pos == 6 else want["num"] >= 5


def test_two_positives_tie_goes_to_the_first_candidate(sh):
    rng = np.random.default_rng(11)
    m, D = 3, 2
    pat = rng.integers(-4, 5, (m, D)).astype(np.float32)
    seqs = [rng.integers(20, 30, (7, D)).astype(np.float32) for _ in range(5)]
    labels = np.array([0, 1, 0, 1, 0], np.uint8)
    seqs[1][2:5] = pat
    seqs[3][1:4] = pat
    got, want = check_find(sh, seqs, labels, m)
    assert got["best"][:2].tolist() == [1, 2]


# ---------------------------------------------------------------- 3. features
def feature_motion(joints):
    lengths = [1, 5, 2 * FEAT_ROWS + 12, 4, FEAT_ROWS - 14]
    mot = sc.make_motion(70 + joints, lengths, joints)
    off = np.cumsum([0] + lengths)
    mot[0, 2, 0] = 0            # a zero in row 0 (the one-row sequence)
    mot[off[2], 4, :2] = 0      # a leading zero of a sequence
    mot[off[1] + 3:off[2] + 3, 5, 1] = 0   # a run of zeros across a sequence boundary
    mot[off[2] + 11:off[3], 6, 0] = 0      # a column empty for two fill blocks: the carry crosses them
    mot[off[3] - 1, 7, :2] = 0  # mode 2 at the end of a sequence ...
    mot[off[3], 7, :2] = 0      # ... and at the start of the next
    mot[off[3] + 1, 7, :2] = 0
    mot[off[2] + 20:off[2] + 24, :2, 1] = 300.25  # nose.y == neck.y: the scale is 1e-5
    mot[off[2] + 30, 0, :2] = 0  # a missing nose
    mot[off[2] + 30:off[2] + 33, 0, 1] = 0
    return mot, lengths


@pytest.mark.parametrize("joints", [18, 60])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_features_equal_the_statement(sh, joints, mode):
    mot, lengths = feature_motion(joints)
    got = sh.MotionJointFeatures(mot.copy(), featuremode=mode, lengths=lengths)
    want = sc.motion_features(mot, lengths, mode)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(sc.motion_features(mot, None, mode)))  # the boundaries matter
    dev = sh.MotionJointFeatures(torch.from_numpy(mot).cuda(), featuremode=mode, lengths=lengths)
    assert dev.is_cuda and np.array_equal(bits(dev.cpu().numpy()), bits(want))


def test_features_of_the_fixture_equal_the_reference(sh):
    ref = np.load(os.path.join(GOLDEN, "shapelet_ref.npz"))
    for n, (seed, lengths, joints) in enumerate(sc.GOLDEN_MOTION):
        mot = sc.make_motion(seed, lengths, joints)
        for mode in (0, 1, 2):
            got = sh.MotionJointFeatures(mot.copy(), featuremode=mode, lengths=lengths)
            assert np.array_equal(bits(got), bits(ref["motion%d_mode%d" % (n, mode)])), (n, mode)


# ---------------------------------------------------------------- 4. the model, devices, errors
def test_fixture_sets_end_to_end(sh):
    ref = np.load(os.path.join(GOLDEN, "shapelet_ref.npz"))
    for n, args in enumerate(sc.GOLDEN_SETS):
        seqs, labels = sc.make_set(*args)
        model = sh.ShapeletMatrixModel().train(seqs, torch.from_numpy(labels.astype(np.int64)), args[3])
        assert (model.shapeindex, model.cand) == (int(ref["set%d_shapeindex" % n]), int(ref["set%d_cand" % n])), n
        assert model.locs.dtype == np.int16 and np.array_equal(model.locs, ref["set%d_locs" % n]), n
        assert model.score == float(ref["set%d_score" % n]), n
        want = sc.train(seqs, labels, args[3])
        assert np.array_equal(model.dis, want["dis"].astype(np.float64)) and model.loss == want["loss"], n


def test_device_resident_equals_host(sh):
    seqs, labels = sc.make_set(81, 8, 6, 4, 3, max_extra=TC + 4)
    seq, off = ragged(seqs)
    host = sh.shapelet_find(seq, off, labels, 4, every=True)
    dev = sh.shapelet_find(torch.from_numpy(seq).cuda(), off, labels, 4, every=True)
    for k, v in host.items():
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), v), k
    m2, lc = sh.shapelet_mindist(seq, off, 4, [0, 2])
    dm2, dlc = sh.shapelet_mindist(torch.from_numpy(seq).cuda(), off, 4, [0, 2])
    assert np.array_equal(bits(dm2.cpu().numpy()), bits(m2)) and np.array_equal(dlc.cpu().numpy(), lc)
    d = sh.SlidingDistance(torch.from_numpy(seqs[0][:4]).cuda(), torch.from_numpy(seqs[1]).cuda())
    assert d.is_cuda and np.array_equal(bits(d.cpu().numpy()), bits(sh.SlidingDistance(seqs[0][:4], seqs[1])))
    # the [N, D, T] tensor form of the reference, on the device
    X = torch.from_numpy(np.stack([y[:4].T for y in seqs])).cuda()
    a = sh.ShapeletMatrixModel().train(X, labels, 2)
    b = sh.ShapeletMatrixModel().train([y[:4] for y in seqs], labels, 2)
    assert (a.shapeindex, a.cand, a.score) == (b.shapeindex, b.cand, b.score) and np.array_equal(a.locs, b.locs)


@pytest.mark.parametrize("mode", ["x-mirror", "y-mirror"])
def test_mirror_modes_equal_the_statement(sh, mode):
    seqs, labels = sc.make_set(21, 8, 4, 5, 3, max_extra=10)
    model = sh.ShapeletMatrixModel().train(seqs, labels, 5, mirror=mode)
    want = sc.train(seqs, labels, 5, mirror=mode)
    assert (model.shapeindex, model.cand, model.score) == (want["shapeindex"], want["cand"], want["score"])
    assert np.array_equal(model.mirrored, want["mirrored"]) and np.array_equal(model.locs, want["locs"])
    assert np.array_equal(model.dis, want["dis"].astype(np.float64)) and model.loss == want["loss"]


def test_shape_and_argument_errors(sh):
    from src import _native
    lib, handle = _native.lib, sh.default_handle()
    seq = np.zeros((MAXSEQ + 1, 1), np.float32)

    def mindist(off, D, m, n_seq=None):
        off = np.asarray(off, np.int64)
        n_seq = len(off) - 1 if n_seq is None else n_seq
        cs = np.zeros(1, np.int32)
        out = np.zeros((64, max(n_seq, 1)), np.float32)
        loc = np.zeros((64, max(n_seq, 1)), np.int32)
        return lib.opose_shapelet_mindist(handle.h, seq.ctypes.data, off.ctypes.data, n_seq, D, m, cs.ctypes.data, 1,
                                          out.ctypes.data, loc.ctypes.data, 0)

    assert mindist([0, 4, 8], 1, 3) == _native.OPOSE_OK
    assert mindist([0, 4, 6], 1, 3) == _native.OPOSE_E_SHAPE       # a sequence shorter than m
    assert mindist([1, 4, 8], 1, 3) == _native.OPOSE_E_ARG         # off[0] != 0
    assert mindist([0, 5, 4, 8], 1, 1) == _native.OPOSE_E_ARG      # off decreases
    assert mindist([0, 4, 8], 0, 3) == _native.OPOSE_E_ARG
    assert mindist([0, 4, 8], 1, 0) == _native.OPOSE_E_ARG
    assert mindist([0, 2], MAXD + 1, 1) == _native.OPOSE_E_SHAPE   # the limits
    assert mindist([0, MAXM + 2], 1, MAXM + 1) == _native.OPOSE_E_SHAPE
    assert mindist(np.arange(MAXSEQ + 2), 1, 1) == _native.OPOSE_E_SHAPE
    labels = np.array([1, 0], np.uint8)
    with pytest.raises(_native.OposeError) as e:
        sh.shapelet_find(seq[:8], np.array([0, 4, 6], np.int64), labels, 3)
    assert e.value.code == _native.OPOSE_E_SHAPE
    with pytest.raises(_native.OposeError) as e:
        sh.shapelet_find(seq[:12], np.array([0, 4, 8, 12], np.int64), labels, 3)  # 3 sequences, 2 labels
    assert e.value.code == _native.OPOSE_E_ARG
    with pytest.raises(_native.OposeError) as e:
        sh.shapelet_find(seq[:8], np.array([0, 4, 8], np.int64), np.zeros(2, np.uint8), 3)  # no candidate
    assert e.value.code == _native.OPOSE_E_ARG
    with pytest.raises(_native.OposeError) as e:
        sh.MotionJointFeatures(np.zeros((4, 18, 3)), lengths=[4], featuremode=3)
    assert e.value.code == _native.OPOSE_E_ARG


# ---------------------------------------------------------------- 5. past one workgroup, at the limits
# The cases of shapelet_cases.py (tests/test_shapelet_cases.py shows that each has the geometry and
# the ties it claims); T = kShpThreads.
@pytest.mark.parametrize("name", sc.SLIDING_CASES)
def test_sliding_distance_over_several_workgroups(sh, name):
    """sliding_distance's row blockIdx.x * T + threadIdx.x: batches of T - 1, T, T + 1 and 2 T + 5 rows,
    a sequence that ends at row T, one that straddles it (its tail rows, which have no window, in
    the second workgroup), and seq_of_row's search over 300 sequences.  The output is prefilled, so
    a value not written, or written past the end, shows."""
    from src import _native
    pat, seqs = sc.sliding_case(name)
    seq, off = ragged(seqs)
    m, n_seq = len(pat), len(seqs)
    want = sc.sliding_distance(pat, seqs)
    assert len(want) == len(seq) - n_seq * (m - 1)
    handle = sh.default_handle()
    patd, seqd = torch.from_numpy(pat).cuda(), torch.from_numpy(seq).cuda()
    dist = torch.full((len(want) + T,), -1.0, dtype=torch.float32, device="cuda")
    handle.torch_call(_native.lib.opose_sliding_distance, patd.data_ptr(), m, seqd.data_ptr(), off.ctypes.data, n_seq,
                      seq.shape[1], dist.data_ptr(), _native.DEVICE_IO)
    got = dist.cpu().numpy()
    assert np.array_equal(bits(got[:len(want)]), bits(want))
    assert (got[len(want):] == -1.0).all()
    host = np.full(len(want), -1.0, np.float32)
    handle.check(_native.lib.opose_sliding_distance(handle.h, pat.ctypes.data, m, seq.ctypes.data, off.ctypes.data,
                                                    n_seq, seq.shape[1], host.ctypes.data, 0))
    assert np.array_equal(bits(host), bits(want))


@pytest.mark.parametrize("name", sc.SCORE_CASES)
def test_score_and_select_past_their_first_trip(sh, name):
    """shapelet_score's key fill, rank count and label scatter (loops that step by T over n_labels:
    n_labels of T - 1, T, T + 1, 2 T + 3 and kShpMaxSeq, equal keys at k and k + T -- one thread, two
    trips -- and at k and k + T + 1, every key equal, all / one positive, the pair minimum at
    k + n_labels for k >= T), and shapelet_select's candidate walk and reduction (n_cand of T - 1, T,
    T + 1, 2 T + 7; the last candidate the winner; identical rows tying fully across trips and across
    threads, the later member in the lower thread; equal num with the smaller loss later)."""
    from src._native import lib
    rows, labels = sc.score_case(name)
    want_nums, want_losses, w = sc.score_expected(name)
    rows = np.ascontiguousarray(rows, np.float32)
    n_cand, n_seq = rows.shape
    handle = sh.default_handle()
    nums, losses = np.full(n_cand, -7, np.int32), np.full(n_cand, -1.0, np.float64)
    winner, wloss = np.full(4, -7, np.int32), np.full(1, -1.0, np.float64)
    handle.check(lib.opose_debug_shapelet_score(handle.h, rows.ctypes.data, n_cand, n_seq, labels.ctypes.data,
                                                len(labels), nums.ctypes.data, losses.ctypes.data,
                                                winner.ctypes.data, wloss.ctypes.data))
    assert np.array_equal(nums, want_nums)
    assert np.array_equal(losses.view(np.uint64), want_losses.view(np.uint64))
    assert winner.tolist() == [0, w, int(want_nums[w]), n_cand]
    assert wloss.view(np.uint64)[0] == want_losses.view(np.uint64)[w]


@pytest.mark.parametrize("name", sc.MINDIST_CASES)
def test_mindist_long_windows_chunks_and_limits(sh, name):
    """shapelet_mindist where m > kShpTC meets several candidate and position blocks (the band E, the
    row counts na / nb, the c0 + b >= ylen tail), D a whole number of kShpDC chunks and one short of
    it, D = kShpMaxD, the workload's shape (m 25, D 92), 300 and kShpMaxSeq sequences (grid y), and
    a window of m = kShpTC + 5 planted in three position blocks: the lowest location wins."""
    seqs, m, cands = sc.mindist_case(name)
    check_mindist(sh, seqs, m, cands, want=sc.mindist_expected(name))


def test_find_on_the_workload_shape(sh):
    """The shape scripts/shapelet_timing.py times (m 25, D 92), made small, through the whole search."""
    seqs, m, _ = sc.mindist_case("workload")
    got, want = check_find(sh, seqs, np.array([1, 0, 1, 0, 1, 0], np.uint8), m)
    assert want["n_cand"] == sum(len(seqs[i]) - m + 1 for i in (0, 2, 4))


def test_find_cuts_a_chunk_at_its_default_size(sh):
    """max_cands = 0 with more than kShpDefaultCands candidates: the default path cuts a chunk, the
    per-candidate nums / losses of the second chunk land behind the first's (in the caller's device
    memory too), and the winner's full tie with a candidate of the second chunk stays with the winner."""
    seqs, labels, m = sc.find_case("default_chunks")
    want = sc.find_expected("default_chunks")
    host, _ = check_find(sh, seqs, labels, m, want=want)
    assert host["best"][3] == want["n_cand"] and want["n_cand"] > DEFAULT_CANDS
    seq, off = ragged(seqs)
    dev = sh.shapelet_find(torch.from_numpy(seq).cuda(), off, labels, m, every=True)
    for k, v in host.items():
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), v), k


def test_find_full_tie_across_chunks_stays_with_the_earlier_candidate(sh):
    """shapelet_select's take: the running winner is replaced only by a strictly better candidate.
    The two planted windows tie fully; in one chunk the reduction decides, in two the strict <."""
    seqs, labels, m = sc.find_case("tie")
    want = sc.find_expected("tie")
    one, _ = check_find(sh, seqs, labels, m, want=want)
    two, _ = check_find(sh, seqs, labels, m, max_cands=sc.TIE_FIND_SPLIT, want=want)
    assert one["best"][:2].tolist() == [1, sc.TIE_FIND_ROWS[0]]
    for k in one:
        assert np.array_equal(one[k], two[k]), k


@pytest.mark.parametrize("name", list(sc.CUT_WINNERS))
def test_find_chunk_cut_inside_a_candidate_block(sh, name):
    """max_cands not a multiple of kShpTR cuts a sequence's block of starts: the winner in the cut
    block's two parts and in the entry after them (shapelet_select's table walk from out0)."""
    seqs, labels, m = sc.find_case(name)
    want = sc.find_expected(name)
    cut, _ = check_find(sh, seqs, labels, m, max_cands=sc.CUT_CANDS, want=want)
    assert cut["best"][:2].tolist() == list(sc.CUT_WINNERS[name])
    one, _ = check_find(sh, seqs, labels, m, want=want)
    for k in one:
        assert np.array_equal(one[k], cut[k]), k


def test_single_length_rows_are_written_in_place_and_nothing_past_them(sh):
    """opose_shapelet_mindist / opose_shapelet_find run the several-lengths kernel with one length, so
    a start's output row comes from the per-(entry, length) row table, not from the block table's out0.
    m = 5, D = kShpDC + 3, clips of one start, exactly one table entry, an entry with a single start
    behind a full one, and one with two; every clip a candidate; max_cands = 8, so chunks end inside
    table entries.  The device outputs are prefilled and kShpThreads elements too long: every row
    equals the statement bit for bit and nothing past the end is written."""
    from src import _native
    lib, handle = _native.lib, sh.default_handle()
    m, D = 5, DC + 3
    seqs = random_seqs(97, [m, m + TR - 1, m + TR, m + TR + 1], D)
    labels = np.ones(len(seqs), np.uint8)
    want = sc.find(seqs, labels, m)  # its min2 / loc: sc.mindist with every clip a candidate
    seq, off = ragged(seqs)
    n_seq, n_cand = len(seqs), 1 + TR + (TR + 1) + (TR + 2)
    assert want["min2"].shape == (n_cand, n_seq) and 1 < 8 < 1 + TR  # the first chunk ends inside clip 1's entry
    seqd = torch.from_numpy(seq).cuda()

    def prefilled(n, dtype, fill):
        return torch.full((n + T,), fill, dtype=dtype, device="cuda")

    def written(buf, n, fill):
        got = buf.cpu().numpy()
        assert (got[n:] == fill).all()
        return got[:n]

    cs = np.arange(n_seq, dtype=np.int32)
    min2, loc = prefilled(n_cand * n_seq, torch.float32, -1.0), prefilled(n_cand * n_seq, torch.int32, -7)
    handle.torch_call(lib.opose_shapelet_mindist, seqd.data_ptr(), off.ctypes.data, n_seq, D, m, cs.ctypes.data, n_seq,
                      min2.data_ptr(), loc.data_ptr(), _native.DEVICE_IO)
    assert np.array_equal(bits(written(min2, n_cand * n_seq, -1.0)), bits(want["min2"]).reshape(-1))
    assert np.array_equal(written(loc, n_cand * n_seq, -7), want["loc"].reshape(-1))

    best, loss = prefilled(4, torch.int32, -7), prefilled(1, torch.float64, -1.0)
    dis, locs = prefilled(n_seq, torch.float32, -1.0), prefilled(n_seq, torch.int32, -7)
    nums, losses = prefilled(n_cand, torch.int32, -7), prefilled(n_cand, torch.float64, -1.0)
    handle.torch_call(lib.opose_shapelet_find, seqd.data_ptr(), off.ctypes.data, n_seq, D, m, labels.ctypes.data, n_seq,
                      8, best.data_ptr(), loss.data_ptr(), dis.data_ptr(), locs.data_ptr(), nums.data_ptr(),
                      losses.data_ptr(), _native.DEVICE_IO)
    assert np.array_equal(written(nums, n_cand, -7), want["nums"])
    assert np.array_equal(written(losses, n_cand, -1.0).view(np.uint64), want["losses"].view(np.uint64))
    assert written(best, 4, -7).tolist() == [want["shapeindex"], want["cand"], want["num"], n_cand]
    assert written(loss, 1, -1.0)[0] == want["loss"]
    assert np.array_equal(bits(written(dis, n_seq, -1.0)), bits(want["dis"]))
    assert np.array_equal(written(locs, n_seq, -7), want["locs"])


@pytest.mark.parametrize("joints", [18, 60])
@pytest.mark.parametrize("name", sc.FEATURE_CASES)
def test_feature_edges_equal_the_statement(sh, name, joints):
    """feat_compute / seq_of_row with empty sequences (first, two in the middle, last), L of kFeatRows
    and kFeatRows + 1, 300 one-row sequences (the search), and the fills at the fill block's edges:
    a carry from the previous sequence in the previous block refused beside one accepted, a sequence
    that starts / ends on a block boundary with zeros there (modes 0 / 1 and the nearby fill of mode 2)."""
    mot, lengths = sc.feature_case(name, joints)
    for mode in (0, 1, 2):
        got = sh.MotionJointFeatures(mot, featuremode=mode, lengths=lengths)
        want = sc.motion_features(mot, lengths, mode)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), mode
    dev = sh.MotionJointFeatures(torch.from_numpy(mot).cuda(), featuremode=2, lengths=lengths)
    assert dev.is_cuda and np.array_equal(bits(dev.cpu().numpy()), bits(sc.motion_features(mot, lengths, 2)))
