"""GPU: every occurrence of found shapelets across whole streams (shapelet_scan_dist /
shapelet_scan_pick in csrc/shapelet.hip, opose_shapelet_scan / opose_debug_shapelet_pick, and their
Python forms in src/shapelet.py and src/augment.py) against the NumPy statement of
tests/shapelet_scan_cases.py.  Every comparison with the statement is bit equality on off, pos and
the bits of dist; the reference goldens are held to the tolerance their generator measured.
tests/test_shapelet_scan_cases.py shows on the CPU that each case has the geometry it claims."""
import json
import os

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

import shapelet_scan_cases as cs
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def sh():
    from src import shapelet
    return shapelet


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ragged(seqs):
    D = seqs[0].shape[1]
    return (np.ascontiguousarray(np.concatenate([np.asarray(y, F32).reshape(-1, D) for y in seqs]), F32),
            np.cumsum([0] + [len(y) for y in seqs]).astype(np.int64))


def same(got, want):
    occ, pos, dist = want
    assert np.array_equal(np.asarray(got["off"]), occ)
    assert np.array_equal(np.asarray(got["pos"]), pos)
    assert np.array_equal(bits(got["dist"]), bits(dist))


# ---------------------------------------------------------------- the pick rule, dictated profiles
def debug_pick(native, sh, dist, off, m, sigma, cap=None):
    n_seq = len(off) - 1
    cap = len(dist) + 1 if cap is None else cap
    occ = np.full(n_seq + 1, -7, np.int64)
    pos, d = np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7, F32)
    dist, off = np.ascontiguousarray(dist, F32), np.ascontiguousarray(off, np.int64)
    rc = native.lib.opose_debug_shapelet_pick(sh.default_handle().h, dist.ctypes.data, off.ctypes.data, n_seq, int(m),
                                              float(sigma), occ.ctypes.data, pos.ctypes.data, d.ctypes.data, cap)
    return rc, occ, pos, d


@pytest.mark.parametrize("name", cs.PICK_CASES)
def test_pick_rule(native, sh, name):
    for dist, off, m, sigma, want in cs.pick_calls(name):
        rc, occ, pos, d = debug_pick(native, sh, dist, off, m, sigma)
        assert rc == native.OPOSE_OK
        wocc, wpos, wd = cs.pick(dist, off, m, sigma)
        n = int(wocc[-1])
        assert np.array_equal(occ, wocc) and np.array_equal(pos[:n], wpos) and np.array_equal(bits(d[:n]), bits(wd))
        assert np.all(pos[n:] == -7)  # nothing past the total is written
        if want is not None:  # the hand-derived lists, independent of the statement's walk
            for j, entries in enumerate(want):
                assert pos[occ[j]:occ[j + 1]].tolist() == [c for c, _ in entries]
                assert d[occ[j]:occ[j + 1]].tolist() == [F32(v) for _, v in entries]


def test_pick_capacity(native, sh):
    dist, off, m, sigma, _ = cs.pick_case("all_hits")
    wocc, wpos, wd = cs.pick(dist, off, m, sigma)
    total = int(wocc[-1])
    assert total > 3
    rc, occ, pos, d = debug_pick(native, sh, dist, off, m, sigma, cap=total)
    assert rc == native.OPOSE_OK and np.array_equal(pos[:total], wpos)
    rc, occ, pos, d = debug_pick(native, sh, dist, off, m, sigma, cap=total - 1)
    assert rc == native.OPOSE_E_CAPACITY and np.array_equal(occ, wocc)
    assert np.array_equal(pos[:total - 1], wpos[:-1]) and np.array_equal(bits(d[:total - 1]), bits(wd[:-1]))


# ---------------------------------------------------------------- the distance stage
@pytest.mark.parametrize("name", cs.DIST_CASES)
def test_scan_equals_the_statement(sh, name):
    pats, sig, seqs = cs.dist_case(name)
    seq, off = ragged(seqs)
    got = sh.shapelet_scan(pats, sig, seq, off)
    same(got, cs.dist_expected(name))
    # the distance at every reported position is SlidingDistance's for that pattern and stream
    occ, n = got["off"], len(seqs)
    for q, p in enumerate(pats):
        for j, y in enumerate(seqs):
            a, b = occ[q * n + j], occ[q * n + j + 1]
            if a == b:
                continue
            sd = sh.SlidingDistance(p, y)
            assert np.array_equal(bits(sd[got["pos"][a:b]]), bits(got["dist"][a:b])), (q, j)


def test_nan_and_non_positive_sigma_give_no_hits(sh):
    pats, sig, seqs = cs.dist_case("one_pattern")
    seq, off = ragged(seqs)
    for s in (np.nan, 0.0, -1.0, -np.inf):
        got = sh.shapelet_scan(pats, [s], seq, off)
        assert not got["off"].any() and len(got["pos"]) == 0
    got = sh.shapelet_scan(pats, [np.inf], seq, off)
    assert got["off"][-1] > 0


# ---------------------------------------------------------------- chunking, capacity, devices
def test_chunking_does_not_change_the_result(sh):
    pats, sig, seqs = cs.dist_case("chunks")
    seq, off = ragged(seqs)
    want = cs.dist_expected("chunks")
    for max_pats in (1, 2, 0, len(pats), len(pats) + 3):
        same(sh.shapelet_scan(pats, sig, seq, off, max_pats=max_pats), want)


def test_capacity(sh, native):
    pats, sig, seqs = cs.dist_case("chunks")
    seq, off = ragged(seqs)
    wocc, wpos, wd = cs.dist_expected("chunks")
    total = int(wocc[-1])
    same(sh.shapelet_scan(pats, sig, seq, off, cap=total, max_pats=2), (wocc, wpos, wd))
    # one short: the error, occ_off complete, the first cap entries right
    pat, pat_off = ragged(pats)
    sig = np.ascontiguousarray(sig, F32)
    occ = np.full(len(wocc), -7, np.int64)
    pos, d = np.full(total, -7, np.int32), np.full(total, -7, F32)
    rc = native.lib.opose_shapelet_scan(sh.default_handle().h, pat.ctypes.data, pat_off.ctypes.data, len(pats),
                                        sig.ctypes.data, seq.ctypes.data, off.ctypes.data, len(seqs), seq.shape[1], 2,
                                        occ.ctypes.data, pos.ctypes.data, d.ctypes.data, total - 1, 0)
    assert rc == native.OPOSE_E_CAPACITY
    assert np.array_equal(occ, wocc) and np.array_equal(pos[:-1], wpos[:-1]) and np.array_equal(bits(d[:-1]), bits(wd[:-1]))
    assert pos[-1] == -7
    with pytest.raises(native.OposeError) as e:
        sh.shapelet_scan(pats, sig, seq, off, cap=total - 1)
    assert e.value.code == native.OPOSE_E_CAPACITY


def test_the_wrapper_retries_with_the_exact_total(sh, monkeypatch):
    pats, sig, seqs = cs.dist_case("chunks")
    seq, off = ragged(seqs)
    want = cs.dist_expected("chunks")
    assert want[0][-1] > 2
    monkeypatch.setattr(sh, "SCAN_FIRST_CAP", 2)
    same(sh.shapelet_scan(pats, sig, seq, off), want)
    got = sh.shapelet_scan([torch.from_numpy(p).cuda() for p in pats], sig, torch.from_numpy(seq).cuda(), off)
    same({k: v.cpu().numpy() for k, v in got.items()}, want)


@pytest.mark.parametrize("name", ["tile_edges", "group_plus_one", "lds_over"])
def test_device_path_equals_host_path(sh, name):
    pats, sig, seqs = cs.dist_case(name)
    seq, off = ragged(seqs)
    got = sh.shapelet_scan([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pats], sig,
                           torch.from_numpy(seq).cuda(), off)
    assert all(v.is_cuda for v in got.values())
    assert got["off"].dtype == torch.int64 and got["pos"].dtype == torch.int32 and got["dist"].dtype == torch.float32
    same({k: v.cpu().numpy() for k, v in got.items()}, cs.dist_expected(name))
    # a cap below the total on the device path: no error, the total in off, the first cap entries
    total = int(cs.dist_expected(name)[0][-1])
    short = sh.shapelet_scan(pats, sig, torch.from_numpy(seq).cuda(), off, cap=total - 1)
    assert int(short["off"][-1]) == total and len(short["pos"]) == total - 1
    assert np.array_equal(short["pos"].cpu().numpy(), cs.dist_expected(name)[1][:-1])


# ---------------------------------------------------------------- arguments
def test_refusals_leave_the_outputs_untouched(sh, native):
    lib, handle = native.lib, sh.default_handle()
    E_ARG, E_SHAPE, OK = native.OPOSE_E_ARG, native.OPOSE_E_SHAPE, native.OPOSE_OK

    def call(pat_off=(0, 3), off=(0, 20, 40), D=1, n_pat=None, n_seq=None, cap=64, max_pats=0, h=handle.h, seq_rows=None):
        pat_off, off = np.asarray(pat_off, np.int64), np.asarray(off, np.int64)
        n_pat = len(pat_off) - 1 if n_pat is None else n_pat
        n_seq = len(off) - 1 if n_seq is None else n_seq
        pat = np.zeros((max(int(pat_off.max()), 1), max(D, 1)), F32)
        seq = np.ones((max(int(off.max()), 1) if seq_rows is None else seq_rows, max(D, 1)), F32)
        sig = np.ones(max(len(pat_off) - 1, 1), F32)
        occ = np.full(max(len(pat_off) - 1, 1) * max(len(off) - 1, 1) + 1, -3, np.int64)
        pos, d = np.full(64, -3, np.int32), np.full(64, -3.0, F32)
        rc = lib.opose_shapelet_scan(h, pat.ctypes.data, pat_off.ctypes.data, n_pat, sig.ctypes.data, seq.ctypes.data,
                                     off.ctypes.data, n_seq, D, max_pats, occ.ctypes.data, pos.ctypes.data,
                                     d.ctypes.data, cap, 0)
        touched = not ((occ == -3).all() and (pos == -3).all() and (d == -3.0).all())
        return rc, touched

    assert call() == (OK, True)
    assert call(h=None) == (E_ARG, False)
    assert call(n_pat=0) == (E_ARG, False)
    assert call(n_seq=0) == (E_ARG, False)
    assert call(D=0) == (E_ARG, False)
    assert call(pat_off=(1, 3)) == (E_ARG, False)          # offsets that do not start at 0
    assert call(off=(1, 20, 40)) == (E_ARG, False)
    assert call(pat_off=(0, 3, 2)) == (E_ARG, False)       # ... or that decrease
    assert call(off=(0, 20, 10)) == (E_ARG, False)
    assert call(pat_off=(0, 3, 3, 5)) == (E_ARG, False)    # a pattern of 0 rows
    assert call(cap=-1) == (E_ARG, False)
    assert call(max_pats=-1) == (E_ARG, False)
    assert call(off=(0, 0, 0)) == (OK, True)               # empty streams are no error
    assert call(off=(0, 2, 2, 40)) == (OK, True)           # nor streams shorter than the pattern
    assert call(pat_off=(0, cs.MAXM)) == (OK, True)
    assert call(pat_off=(0, cs.MAXM + 1)) == (E_SHAPE, False)
    assert call(D=cs.MAXD + 1) == (E_SHAPE, False)
    assert call(off=[0] * (cs.MAXSEQ + 2)) == (E_SHAPE, False)
    assert call(pat_off=list(range(cs.MAXPAT + 2))) == (E_SHAPE, False)
    # pairs: kScanMaxPat patterns against more streams than kScanMaxPairs allows
    n_seq = cs.MAXPAIRS // cs.MAXPAT + 1
    assert n_seq <= cs.MAXSEQ
    assert call(pat_off=list(range(cs.MAXPAT + 1)), off=[0] * (n_seq + 1)) == (E_SHAPE, False)
    assert call(off=(0, 2 ** 31), seq_rows=1) == (E_SHAPE, False)   # L beyond kShpMaxRows

    def pick(off=(0, 20), m=3, cap=32, h=handle.h, n_seq=None):
        off = np.asarray(off, np.int64)
        dist = np.zeros(max(int(off.max()), 1), F32)
        occ, pos, d = np.full(len(off), -3, np.int64), np.full(32, -3, np.int32), np.full(32, -3.0, F32)
        rc = lib.opose_debug_shapelet_pick(h, dist.ctypes.data, off.ctypes.data, len(off) - 1 if n_seq is None else n_seq,
                                           m, 1.0, occ.ctypes.data, pos.ctypes.data, d.ctypes.data, cap)
        return rc, not ((occ == -3).all() and (pos == -3).all())

    assert pick() == (OK, True)
    assert pick(h=None) == (E_ARG, False) and pick(n_seq=0) == (E_ARG, False) and pick(m=0) == (E_ARG, False)
    assert pick(off=(1, 20)) == (E_ARG, False) and pick(off=(0, 20, 10)) == (E_ARG, False) and pick(cap=-1) == (E_ARG, False)
    assert pick(m=cs.MAXM + 1) == (E_SHAPE, False)


# ---------------------------------------------------------------- src/augment.py, the real path
@pytest.fixture(scope="module")
def golden():
    path = os.path.join(GOLDEN, "shapelet_scan_ref.npz")
    return np.load(path), json.load(open(path[:-4] + ".json"))


@pytest.mark.parametrize("seed,m,fm,seg", cs.AUG_CASES)
def test_augmentate_one_shapelet_against_the_reference(golden, seed, m, fm, seg):
    from src import augment
    data, meta = golden
    pattern, sigma = cs.aug_case(seed, m, fm)
    name = cs.aug_name(seed, m, fm, seg)
    videos = cs.aug_videos(seed)
    got = augment.AugmentateOneShapelet(pattern, sigma, videos, "posehand", fm, MaxSegLength=seg)
    want = cs.aug_statement(seed, m, fm, seg)
    for vk in videos:
        assert [p for p, _ in got[vk]] == data["%s_%s_pos" % (name, vk)].tolist(), (name, vk)
        np.testing.assert_allclose([d for _, d in got[vk]], data["%s_%s_dist" % (name, vk)], rtol=meta["dist_rtol"], atol=0)
        assert got[vk] == [(p, float(d)) for p, d in want[vk]]  # and the statement, exactly


def test_data_augmentate_runs_every_pattern_through_one_scan(sh, monkeypatch):
    from src import augment
    seed, fm = 1, 1
    videos = cs.aug_videos(seed)
    key, a, b = cs.AUG_CLIP
    clips = {w: (["v1", key], np.array([[0, 60], [a, b]])) for w in ("one", "two")}
    rec = {m: {"locs": np.array([3 + m % 5, cs.AUG_LOC], np.int16), "dists": np.linspace(1, 30, 10).astype(F32),
               "shapelet": np.array([m % 2], np.int16), "score": np.array([0.8], F32)} for m in (9, 15, 24)}
    calls = []
    real = sh.shapelet_scan
    monkeypatch.setattr(sh, "shapelet_scan", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    got = augment.DataAugmentate({"one": rec, "two": {15: rec[15]}}, videos, clips, "posehand", fm)
    assert calls == [4] and list(got) == ["one/15", "one/24", "one/9", "two/15"]
    for name, res in got.items():
        word, m = name.split("/")
        pattern = augment.shapelet_window(rec, m, rec[int(m)]["shapelet"], videos, clips[word], "posehand", fm)
        assert pattern.shape == (int(m), 92)
        one = augment.AugmentateOneShapelet(pattern, np.sort(rec[int(m)]["dists"])[3], videos, "posehand", fm)
        for vk in videos:
            assert np.array_equal(res[vk], np.array(one[vk])) and res[vk].dtype == np.float64
    assert sum(len(v) for res in got.values() for v in res.values()) > 0
