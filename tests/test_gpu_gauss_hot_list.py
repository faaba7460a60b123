"""GPU: gauss_nms_resize's two launches through opose_debug_gauss_hot_tiles -- the screen that lists
the tiles whose sources can reach the threshold, and the NMS whose fixed grid strides over that list.

The hot list against tests/peak_stage_cases.py's restatement of the cold criterion
(resize_cold_tiles: every tile is in exactly one of the two), the peaks against its float64 SciPy
reference (ref_peaks) as in tests/test_gpu_peak_stages.py: sorted indices equal, scores equal as
bit patterns.  Then what the list adds to go wrong: maps with no hot tile, only hot tiles or only
NaN, a grid of fewer workgroups than hot tiles (each loops), a handle reused for another geometry,
and many maps appending to the one list."""
import numpy as np
import pytest

import peak_stage_cases as pc
from oracle.cv_resize import resize_cubic

pytestmark = pytest.mark.gpu
F32, F64 = pc.F32, pc.F64


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def handle(native):
    return native.Handle(0)


def _grid(H, W):
    return (W + pc.WTW - 1) // pc.WTW, (H + pc.WTH - 1) // pc.WTH


def _run(native, handle, mid, geom, max_grid=0):
    """(cnt, list, score, hot): hot = per map the sorted (x0, y0) of the listed tiles, after the
    list's own invariants: *hot_cnt entries, each a valid id, none twice, the rest left at -1."""
    N, Cm, coff, P, Hs, Ws, H, W, thre, cap = geom
    NP = N * P
    ntx, nty = _grid(H, W)
    tiles = NP * ntx * nty
    cnt, lst = np.full(NP, -7, np.int32), np.full((NP, cap), -7, np.int32)
    score = np.full((NP, cap), np.nan, F64)
    hot_cnt, hot = np.full(1, -7, np.int32), np.full(tiles, -7, np.int32)
    mid = np.ascontiguousarray(mid, F32)
    handle.check(native.lib.opose_debug_gauss_hot_tiles(
        handle.h, mid.ctypes.data, N, Cm, coff, P, Hs, Ws, H, W, thre, cap, max_grid, cnt.ctypes.data, lst.ctypes.data,
        score.ctypes.data, hot_cnt.ctypes.data, hot.ctypes.data))
    n = int(hot_cnt[0])
    assert 0 <= n <= tiles and (hot[n:] == -1).all()
    ids = np.sort(hot[:n].astype(np.int64))
    assert len(np.unique(ids)) == n, "a tile listed twice"
    assert n == 0 or (ids[0] >= 0 and ids[-1] < tiles)
    per_map = [[] for _ in range(NP)]
    for i in ids:
        per_map[i // ntx // nty].append((int(i % ntx) * pc.WTW, int(i // ntx % nty) * pc.WTH))
    return cnt, lst, score, [sorted(m) for m in per_map]


def _check_hot(mid, geom, hot):
    """Every tile is listed or cold by the restated bound, never both."""
    N, Cm, coff, P, Hs, Ws, H, W, thre, cap = geom
    every = set(pc.tiles(H, W))
    for k in range(N * P):
        cold = set(pc.resize_cold_tiles(mid[k // P, coff + k % P], H, W, thre))
        assert every - set(hot[k]) == cold, (k, sorted(every - set(hot[k])), sorted(cold))


def _check_peaks(ref, NP, cap, cnt, lst, score):
    """ref(k) -> (row-major indices, scores); counts, sorted lists and score bit patterns equal
    (every case here keeps cap at or above the count)."""
    total = 0
    for k in range(NP):
        ref_idx, ref_sc = ref(k)
        assert cnt[k] == len(ref_idx) <= cap, (k, int(cnt[k]), len(ref_idx))
        n = len(ref_idx)
        assert (lst[k, n:] == -1).all() and not pc.bits(score[k, n:]).any()  # unused slots keep the preset
        order = np.argsort(lst[k, :n])
        assert np.array_equal(lst[k, :n][order], ref_idx), k
        assert np.array_equal(pc.bits(score[k, :n][order]), pc.bits(ref_sc)), k
        total += n
    return total


def _case(name):
    N, Cm, coff, P, Hs, Ws, H, W, thre, cap, fits = pc.RESIZE[name]
    assert fits
    return pc.resize_mid(name), (N, Cm, coff, P, Hs, Ws, H, W, thre, cap or H * W)


def _case_ref(name, thre):
    return lambda k: pc.ref_peaks(("resize", name), k, thre)[:2]


# ------------------------------------------------------------------------------------ hot set
@pytest.mark.parametrize("name", ["cold_bound", "cold_bound_negated", "planes_2x5_off1_3",
                                  "workload_184x328_to_368x656"])
def test_hot_set_and_peaks(native, handle, name):
    mid, geom = _case(name)
    cnt, lst, score, hot = _run(native, handle, mid, geom)
    _check_hot(mid, geom, hot)
    assert _check_peaks(_case_ref(name, geom[8]), geom[0] * geom[3], geom[9], cnt, lst, score) > 0


# ---------------------------------------------------------------------------- degenerate maps
DEGENERATE_GEOM = (1, 1, 0, 1, 20, 30, 61, 205, pc.THRE, 61 * 205)  # 3 x 3 tiles, ragged both ways


def _direct_ref(mid, geom):
    """The reference of a map that is no named case: resize, smooth, peak test."""
    N, Cm, coff, P, Hs, Ws, H, W, thre, cap = geom

    def ref(k):
        m = 0.0 + resize_cubic(np.ascontiguousarray(mid[k // P, coff + k % P]), (W, H)).astype(F64)
        idx = np.flatnonzero(pc.peak_mask(pc.smooth(m), thre))
        return idx, m.ravel()[idx]
    return ref


@pytest.mark.parametrize("fill", [0.0, 0.5, np.nan], ids=["zero", "const_0.5", "nan"])
def test_degenerate_maps(native, handle, fill):
    geom = DEGENERATE_GEOM
    mid = np.full((1, 1, geom[4], geom[5]), fill, F32)
    cnt, lst, score, hot = _run(native, handle, mid, geom)
    _check_hot(mid, geom, hot)
    every = sorted(pc.tiles(geom[6], geom[7]))
    assert hot[0] == (every if fill == 0.5 else [])
    total = _check_peaks(_direct_ref(mid, geom), 1, geom[9], cnt, lst, score)
    assert (total > 0) == (fill == 0.5)


# ------------------------------------------------------------------------------------ looping
@pytest.mark.parametrize("max_grid", [3, 1])
def test_few_workgroups_loop_over_the_list(native, handle, max_grid):
    name = "max_step_68_to_110"  # 2 maps x 8 tiles, every one hot
    mid, geom = _case(name)
    cnt, lst, score, hot = _run(native, handle, mid, geom, max_grid)
    assert sum(len(m) for m in hot) == 16
    _check_hot(mid, geom, hot)
    assert _check_peaks(_case_ref(name, geom[8]), 2, geom[9], cnt, lst, score) > 0


# ------------------------------------------------------------------- no state between calls
def test_second_call_on_a_handle_equals_a_fresh_one(native, handle):
    big, big_geom = _case("workload_184x328_to_368x656")
    mid, geom = _case("cold_bound")
    _run(native, handle, big, big_geom)
    cnt, lst, score, hot = _run(native, handle, mid, geom)
    fresh = native.Handle(0)
    cnt2, lst2, score2, hot2 = _run(native, fresh, mid, geom)
    assert hot == hot2 and np.array_equal(cnt, cnt2)
    n = int(cnt[0])
    o, o2 = np.argsort(lst[0, :n]), np.argsort(lst2[0, :n])
    assert np.array_equal(lst[0, :n][o], lst2[0, :n][o2])
    assert np.array_equal(pc.bits(score[0, :n][o]), pc.bits(score2[0, :n][o2]))
    _check_hot(mid, geom, hot)
    assert _check_peaks(_case_ref("cold_bound", geom[8]), 1, geom[9], cnt, lst, score) > 0


# --------------------------------------------------------------------------- aggregated append
def test_many_maps_append_each_hot_tile_once(native, handle):
    """planes_2x5_off1_3's geometry with 40 frames: 120 maps of 9 tiles, one append per map.  Maps
    scaled to 1, 1/4 (cold: 1.9 x 0.05 < 0.1) and 0, and every third map zero outside its top left
    2 x 2 sources, so that maps contribute nine, some or no tiles."""
    _, Cm, coff, P, Hs, Ws, H, W, thre, _, _ = pc.RESIZE["planes_2x5_off1_3"]
    N = 40
    rng = np.random.default_rng(120)
    mid = rng.random((N, Cm, Hs, Ws), dtype=F32) * F32(0.2)
    mid *= rng.choice(np.array([1.0, 0.25, 0.0], F32), size=(N, Cm, 1, 1))
    corner = mid.reshape(N * Cm, Hs, Ws)[::3]
    corner[:, 2:, :] = 0
    corner[:, :, 2:] = 0
    geom = (N, Cm, coff, P, Hs, Ws, H, W, thre, H * W)
    _, _, _, hot = _run(native, handle, mid, geom)  # (_run: no id twice)
    _check_hot(mid, geom, hot)
    sizes = {len(m) for m in hot}
    assert 0 in sizes and 9 in sizes and len(sizes) > 2
