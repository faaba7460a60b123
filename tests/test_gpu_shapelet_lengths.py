"""GPU: the search over several window lengths in one pass (shapelet_mindist in csrc/shapelet.hip
with more than one length, opose_shapelet_mindist_lengths / opose_shapelet_find_lengths, and their
Python forms in src/shapelet.py) against the NumPy statement of tests/shapelet_lengths_cases.py and
against the single-length entry points, which launch the same kernel once per length: a snapshot
taken at the wrong term, or a row of one length landing in another's, differs from both.  Every
comparison is bit equality.  The cases are those of shapelet_lengths_cases.py, cut to the constants
of csrc/shapelet.h; tests/test_shapelet_lengths_cases.py shows on the CPU that each has the
geometry it claims."""
import os
import re

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

import shapelet_cases as sc
import shapelet_lengths_cases as lc
from conftest import REPO

pytestmark = pytest.mark.gpu


def _constants():
    src = open(os.path.join(REPO, "pytorch-openpose_amd", "csrc", "shapelet.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}


K = _constants()
TR, TC, DC, MAXM, MAXLENS = (K[k] for k in ("kShpTR", "kShpTC", "kShpDC", "kShpMaxM", "kShpMaxLens"))
assert K == sc.K


@pytest.fixture(scope="module")
def sh():
    from src import shapelet
    return shapelet


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ragged(seqs):
    return (np.ascontiguousarray(np.concatenate(seqs), np.float32),
            np.cumsum([0] + [len(y) for y in seqs]).astype(np.int64))


def check_mindist_lengths(sh, seqs, m_lens, cands, want=None, single=True):
    """The several-lengths call against the statement (when given) and, per length, against the
    single-length call on the device (the same kernel, launched with that length alone)."""
    seq, off = ragged(seqs)
    got = sh.shapelet_mindist_lengths(seq, off, m_lens, cands)
    assert len(got) == len(m_lens)
    for l, (m, (min2, loc)) in enumerate(zip(m_lens, got)):
        assert min2.shape == loc.shape == (sum(len(seqs[i]) - m + 1 for i in cands), len(seqs))
        if want is not None:
            assert np.array_equal(bits(min2), bits(want[l][0])) and np.array_equal(loc, want[l][1]), m
        if single:
            one2, oneloc = sh.shapelet_mindist(seq, off, m, cands)
            assert np.array_equal(bits(min2), bits(one2)) and np.array_equal(loc, oneloc), m
    return got


def same_result(got, want):
    """A dict of shapelet_find_lengths against the dict shapelet_find returns."""
    for k in ("best", "locs", "nums"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["dis"]), bits(want["dis"]))
    for k in ("loss", "losses"):
        assert np.array_equal(np.asarray(got[k]).view(np.uint64), np.asarray(want[k]).view(np.uint64)), k


def same_statement(got, want):
    """A dict of shapelet_find_lengths against the statement's dict."""
    assert got["best"].tolist() == [want["shapeindex"], want["cand"], want["num"], want["n_cand"]]
    assert got["loss"][0] == want["loss"]
    assert np.array_equal(got["nums"], want["nums"])
    assert np.array_equal(got["losses"].view(np.uint64), want["losses"].view(np.uint64))
    assert np.array_equal(bits(got["dis"]), bits(want["dis"])) and np.array_equal(got["locs"], want["locs"])


# ---------------------------------------------------------------- 1 - 6. the distance stage
@pytest.mark.parametrize("m", lc.ONE_LENGTHS)
def test_one_length_equals_the_single_length_call(sh, m):
    """n_lens = 1 at m = 1, 15 and kShpMaxM: the dynamic LDS at its smallest and its largest size."""
    name = "one_m%d" % m
    seqs, m_lens, cands = lc.mindist_case(name)
    check_mindist_lengths(sh, seqs, m_lens, cands, want=lc.mindist_expected(name))


@pytest.mark.parametrize("key", list(lc.EDGE_LENGTHS))
def test_block_edges_that_move_with_the_length(sh, key):
    """Clips of mx, mx + 1, mx + TR - 1, mx + TR, mx + TR + 1 and mx + 2 TC + 3 rows (mx the longest
    length), D = kShpDC + 3, every clip a candidate: a clip with one start at the longest length, and
    candidate and position blocks whose edges differ from length to length."""
    seqs, m_lens, cands = lc.mindist_case("edges_" + key)
    check_mindist_lengths(sh, seqs, m_lens, cands, want=lc.mindist_expected("edges_" + key))


@pytest.mark.parametrize("which", list(lc.FULL_LENGTHS))
def test_full_register_set(sh, which):
    """kShpMaxLens lengths, 1 .. 16 and kShpMaxM - 15 .. kShpMaxM: every running pair, the largest LDS."""
    seqs, m_lens, cands = lc.mindist_case("full_" + which)
    assert len(m_lens) == MAXLENS
    check_mindist_lengths(sh, seqs, m_lens, cands, want=lc.mindist_expected("full_" + which))


def test_the_reference_lengths(sh):
    """range(15, 40, 2) at D = 92 on four clips of 39 to 80 rows."""
    seqs, m_lens, cands = lc.mindist_case("reference")
    check_mindist_lengths(sh, seqs, m_lens, cands, want=lc.mindist_expected("reference"))


def test_exact_ties_go_to_the_first_position_at_every_length(sh):
    seqs, m_lens, cands = lc.mindist_case("ties")
    got = check_mindist_lengths(sh, seqs, m_lens, cands, want=lc.mindist_expected("ties"))
    for min2, loc in got:
        assert min2[1, 1] == 0 and loc[1, 1] == lc.TIE_PLACES[0]


@pytest.mark.parametrize("name", ["tail_position", "clip_boundary"])
def test_position_validity_per_length(sh, name):
    """The short length finds its minimum at P_0 - 1, where the long length has no position; and
    the long length does not find the window that would run on into the next clip."""
    seqs, m_lens, cands = lc.mindist_case(name)
    (short2, shortloc), (long2, longloc) = check_mindist_lengths(sh, seqs, m_lens, cands,
                                                                 want=lc.mindist_expected(name))
    assert shortloc[0, 1] == len(seqs[1]) - m_lens[0]
    assert longloc[0, 1] <= len(seqs[1]) - m_lens[1]


# ---------------------------------------------------------------- 7, 8. the whole search
@pytest.mark.parametrize("mirror", [None, "x-mirror"])
@pytest.mark.parametrize("max_cands", lc.FIND_CANDS)
@pytest.mark.parametrize("seed", lc.FIND_SEEDS)
def test_find_lengths_equals_find_per_length(sh, seed, max_cands, mirror):
    seqs, labels = lc.find_set(seed, mirror)
    seq, off = ragged(seqs)
    got = sh.shapelet_find_lengths(seq, off, labels, lc.FIND_LENGTHS, max_cands, every=True)
    want = lc.find_expected(seed, mirror)
    assert len(got) == len(lc.FIND_LENGTHS)
    for m, g, w in zip(lc.FIND_LENGTHS, got, want):
        same_result(g, sh.shapelet_find(seq, off, labels, m, max_cands, every=True))
        same_statement(g, w)
    if seed == 0 and mirror is None:
        assert [tuple(g["best"][:2]) for g in got] == lc.FIND_WINNERS_SEED0


@pytest.mark.parametrize("name", list(lc.CHUNK_CASES))
def test_chunk_traps(sh, name):
    """max_cands = 8: a chunk without a candidate at the long length (the length keeps its winner and
    its count), and a table entry that is empty at the long length in front of the winner's entry
    (the selection reads the long length's own table).  The second also in one chunk, where the
    empty entry is the clip's second."""
    seqs, labels, m_lens = lc.chunk_case(name)
    seq, off = ragged(seqs)
    want = lc.chunk_expected(name)
    for cap in (lc.CHUNK_CANDS, 0):
        got = sh.shapelet_find_lengths(seq, off, labels, m_lens, cap, every=True)
        for m, g, w in zip(m_lens, got, want):
            same_statement(g, w)
            same_result(g, sh.shapelet_find(seq, off, labels, m, cap, every=True))


# ---------------------------------------------------------------- 9, 10. devices and the facade
def test_device_path_equals_host_path(sh):
    seqs, labels = lc.find_set(1)
    seq, off = ragged(seqs)
    seqd = torch.from_numpy(seq).cuda()
    host = sh.shapelet_find_lengths(seq, off, labels, lc.FIND_LENGTHS, 40, every=True)
    dev = sh.shapelet_find_lengths(seqd, off, labels, lc.FIND_LENGTHS, 40, every=True)
    for h, d in zip(host, dev):
        for k, v in h.items():
            assert d[k].is_cuda and np.array_equal(d[k].cpu().numpy(), v), k
    cands = [int(i) for i in np.nonzero(labels)[0]]
    hm = sh.shapelet_mindist_lengths(seq, off, lc.FIND_LENGTHS, cands)
    dm = sh.shapelet_mindist_lengths(seqd, off, lc.FIND_LENGTHS, cands)
    for (h2, hl), (d2, dl) in zip(hm, dm):
        assert d2.is_cuda and dl.is_cuda
        assert np.array_equal(bits(d2.cpu().numpy()), bits(h2)) and np.array_equal(dl.cpu().numpy(), hl)


ATTRS = ("shapeindex", "cand", "score", "loss", "mirrored", "dis", "locs")


@pytest.mark.parametrize("mirror", [None, "x-mirror"])
def test_train_lengths_equals_train(sh, mirror):
    seqs, labels = lc.find_set(0)
    models = sh.ShapeletMatrixModel().train_lengths(seqs, labels, lc.FIND_LENGTHS, mirror=mirror, max_cands=40)
    assert [m.m_len for m in models] == list(lc.FIND_LENGTHS)
    for m, model in zip(lc.FIND_LENGTHS, models):
        one = sh.ShapeletMatrixModel().train(seqs, labels, m, mirror=mirror, max_cands=40)
        for a in ATTRS:
            got, want = getattr(model, a), getattr(one, a)
            assert type(got) is type(want) and np.array_equal(got, want), (m, a)
            if isinstance(want, np.ndarray):
                assert got.dtype == want.dtype and got.shape == want.shape, (m, a)


def test_brute_force_records_equal_the_arrays_built_from_train(sh):
    seqs, labels = lc.find_set(1)
    m_lens = [15, 17, 20]
    rec = sh.brute_force_records(seqs, torch.from_numpy(labels.astype(np.int64)), m_lens)
    assert list(rec) == m_lens
    pos = labels != 0
    for m in m_lens:
        model = sh.ShapeletMatrixModel().train(seqs, labels, m, mirror="x-mirror")
        # srcmx/shapeletlearning.py:190-200
        want = {"locs": np.array([model.locs[i] for i in range(len(labels)) if pos[i]]).astype(np.int16),
                "dists": np.array([model.dis[i] for i in range(len(labels)) if pos[i]]).astype(np.float32),
                "shapelet": np.array([model.shapeindex]).astype(np.int16),
                "score": np.array([model.score]).astype(np.float32)}
        assert sorted(rec[m]) == sorted(want)
        for k, v in want.items():
            assert rec[m][k].dtype == v.dtype and rec[m][k].shape == v.shape and np.array_equal(rec[m][k], v), (m, k)
    assert rec[15]["locs"].shape == (int(pos.sum()),)


# ---------------------------------------------------------------- 11. errors
def test_refusals_leave_the_outputs_untouched(sh):
    from src import _native
    lib, handle = _native.lib, sh.default_handle()
    seq = np.zeros((64, 1), np.float32)
    labels = np.array([1, 0], np.uint8)

    def mindist(off, lens, n_lens=None):
        off, ml = np.asarray(off, np.int64), np.asarray(lens, np.int32)
        cs = np.zeros(1, np.int32)
        out, loc = np.full((256, 2), -3.0, np.float32), np.full((256, 2), -3, np.int32)
        rc = lib.opose_shapelet_mindist_lengths(handle.h, seq.ctypes.data, off.ctypes.data, len(off) - 1, 1,
                                                ml.ctypes.data, len(ml) if n_lens is None else n_lens,
                                                cs.ctypes.data, 1, out.ctypes.data, loc.ctypes.data, 0)
        touched = not ((out == -3.0).all() and (loc == -3).all())
        return rc, touched

    def find(off, lens, n_lens=None):
        off, ml = np.asarray(off, np.int64), np.asarray(lens, np.int32)
        n = len(ml)
        best, loss = np.full((n, 4), -3, np.int32), np.full(n, -3.0, np.float64)
        dis, locs = np.full((n, 2), -3.0, np.float32), np.full((n, 2), -3, np.int32)
        rc = lib.opose_shapelet_find_lengths(handle.h, seq.ctypes.data, off.ctypes.data, len(off) - 1, 1,
                                             ml.ctypes.data, n if n_lens is None else n_lens, labels.ctypes.data, 2, 0,
                                             best.ctypes.data, loss.ctypes.data, dis.ctypes.data, locs.ctypes.data,
                                             None, None, 0)
        touched = not ((best == -3).all() and (loss == -3.0).all() and (dis == -3.0).all() and (locs == -3).all())
        return rc, touched

    off = [0, 20, 40]
    for call in (mindist, find):
        assert call(off, [3, 5]) == (_native.OPOSE_OK, True)
        assert call(off, [3, 5], n_lens=0) == (_native.OPOSE_E_ARG, False)        # n_lens < 1
        assert call(off, [0, 5]) == (_native.OPOSE_E_ARG, False)                  # a length below 1
        assert call(off, [3, 3]) == (_native.OPOSE_E_ARG, False)                  # not strictly ascending
        assert call(off, [5, 3]) == (_native.OPOSE_E_ARG, False)
        assert call(off, list(range(1, MAXLENS + 2))) == (_native.OPOSE_E_SHAPE, False)   # n_lens > kShpMaxLens
        assert call(off, list(range(1, MAXLENS + 1))) == (_native.OPOSE_OK, True)
        assert call([0, MAXM + 2, 2 * MAXM + 4], [3, MAXM + 1]) == (_native.OPOSE_E_SHAPE, False)  # last > kShpMaxM
        assert call([0, 20, 24], [3, 5]) == (_native.OPOSE_E_SHAPE, False)        # shorter than the last length
        assert call([0, 20, 25], [3, 5]) == (_native.OPOSE_OK, True)              # ... and exactly that long
        assert call([1, 20, 40], [3, 5]) == (_native.OPOSE_E_ARG, False)          # the existing batch checks
    # the Python forms raise what the single-length calls raise
    off = np.array([0, 20, 24], np.int64)
    with pytest.raises(_native.OposeError) as single:
        sh.shapelet_find(seq[:24], off, labels, 5)
    for lens in ([3, 5], list(range(1, MAXLENS + 2))):
        with pytest.raises(_native.OposeError) as e:
            sh.shapelet_find_lengths(seq[:24], off, labels, lens)
        assert e.value.code == single.value.code == _native.OPOSE_E_SHAPE
        with pytest.raises(_native.OposeError) as e:
            sh.shapelet_mindist_lengths(seq[:24], off, lens, [0])
        assert e.value.code == _native.OPOSE_E_SHAPE
    with pytest.raises(_native.OposeError) as single:
        sh.shapelet_mindist(seq[:24], off, 0, [0])
    for lens in ([0, 3], [3, 3], []):
        with pytest.raises(_native.OposeError) as e:
            sh.shapelet_mindist_lengths(seq[:24], off, lens, [0])
        assert e.value.code == single.value.code == _native.OPOSE_E_ARG
        with pytest.raises(_native.OposeError) as e:
            sh.shapelet_find_lengths(seq[:24], off, labels, lens)
        assert e.value.code == _native.OPOSE_E_ARG
    with pytest.raises(_native.OposeError) as e:  # no positive clip, as the single-length call
        sh.shapelet_find_lengths(seq[:40], np.array([0, 20, 40], np.int64), np.zeros(2, np.uint8), [3, 5])
    assert e.value.code == _native.OPOSE_E_ARG
