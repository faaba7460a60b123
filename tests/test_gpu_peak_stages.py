"""GPU: the exact mode's peak finder and heat average one launch at a time -- gauss_nms_wide<float>
and <double>, gauss_nms_resize, heat_full_scales and the per-scale heat_full, and the hand threshold
gauss_threshold -- each against plain SciPy / NumPy float64 of the same operation, at the sizes
where the kernels change path: the three load modes' boundaries, exact ties across a tile corner,
the threshold at equality, cold tiles on their bound, NaN, ragged XCD-ordered tile counts, the
largest source steps the staged rows hold, identity scales, a division by the number of scales
that is not exact.

Every comparison is equality (tests/peak_stage_cases.py says why): counts, sorted peak lists,
scores and averages as bit patterns.  tests/test_peak_stage_cases.py asserts on the CPU that every
case reaches the path it is named for."""
import ctypes

import numpy as np
import pytest

import peak_stage_cases as pc

pytestmark = pytest.mark.gpu
F32, F64 = pc.F32, pc.F64
IDS = {F32: "f32", F64: "f64"}.get


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def handle(native):
    return native.Handle(0)


def _outputs(NP, cap):
    return np.full(NP, -7, np.int32), np.full((NP, cap), -7, np.int32), np.full((NP, cap), np.nan, F64)


def _check_peaks(key, NP, thre, cap, cnt, lst, score):
    """cnt, the sorted list and the scores' bit patterns of every map against the reference; above
    cap: the true count, and cap distinct members of the reference set with their scores."""
    total = 0
    for k in range(NP):
        ref_idx, ref_sc, _ = pc.ref_peaks(key, k, thre)
        assert cnt[k] == len(ref_idx), (key, k, int(cnt[k]), len(ref_idx))
        n = min(len(ref_idx), cap)
        got = lst[k, :n].astype(np.int64)
        assert (lst[k, n:] == -1).all() and not pc.bits(score[k, n:]).any()  # unused slots keep the preset
        order = np.argsort(got)
        got, got_sc = got[order], score[k, :n][order]
        assert len(np.unique(got)) == n
        if len(ref_idx) <= cap:
            assert np.array_equal(got, ref_idx), (key, k, np.setxor1d(got, ref_idx)[:8])
            assert np.array_equal(pc.bits(got_sc), pc.bits(ref_sc)), (key, k)
        else:
            pos = np.searchsorted(ref_idx, got)
            assert (pos < len(ref_idx)).all() and np.array_equal(ref_idx[np.minimum(pos, len(ref_idx) - 1)], got)
            assert np.array_equal(pc.bits(got_sc), pc.bits(ref_sc[pos])), (key, k)
        total += len(ref_idx)
    return total


# --------------------------------------------------------------------------- gauss_nms_wide
@pytest.mark.parametrize("dtype", [F32, F64], ids=IDS)
@pytest.mark.parametrize("name", list(pc.WIDE))
def test_gauss_nms_wide(native, handle, name, dtype):
    maps, thre, cap = pc.wide_case(name, dtype)
    NP, H, W = maps.shape
    cnt, lst, score = _outputs(NP, cap)
    handle.check(native.lib.opose_debug_gauss_nms(handle.h, maps.ctypes.data, int(dtype == F32), NP, H, W, thre, cap,
                                                  cnt.ctypes.data, lst.ctypes.data, score.ctypes.data))
    total = _check_peaks(("wide", name, dtype), NP, thre, cap, cnt, lst, score)
    assert (total == 0) == pc.WIDE[name]


# -------------------------------------------------------------------------- gauss_nms_resize
@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_gauss_nms_resize(native, handle, name):
    N, Cm, coff, P, Hs, Ws, H, W, thre, cap, fits = pc.RESIZE[name]
    cap = cap or H * W
    mid = pc.resize_mid(name)
    cnt, lst, score = _outputs(N * P, cap)
    rc = native.lib.opose_debug_gauss_nms_resize(handle.h, mid.ctypes.data, N, Cm, coff, P, Hs, Ws, H, W, thre, cap,
                                                 cnt.ctypes.data, lst.ctypes.data, score.ctypes.data)
    if not fits:  # refused before any launch: nothing written
        assert rc == pc.OPOSE_E_ARG and (cnt == -7).all() and (lst == -7).all()
        return
    handle.check(rc)
    assert _check_peaks(("resize", name), N * P, thre, cap, cnt, lst, score) > 0


# -------------------------------------------------------------------------- heat_full_scales
def _heat(native, handle, name, one_launch):
    sizes, N, Cm, coff, C, H, W, _ = pc.HEAT[name]
    mids = pc.heat_mids(name)
    n = len(sizes)
    ptrs = (ctypes.c_void_p * n)(*[m.ctypes.data for m in mids])
    hs = np.array([s[0] for s in sizes], np.int32)
    ws = np.array([s[1] for s in sizes], np.int32)
    avg = np.full((N * C, H, W), np.nan, F64)
    rc = native.lib.opose_debug_heat_scales(handle.h, n, ctypes.cast(ptrs, ctypes.c_void_p), hs.ctypes.data,
                                            ws.ctypes.data, N, Cm, coff, C, H, W, one_launch, avg.ctypes.data)
    return rc, avg


@pytest.mark.parametrize("name", list(pc.HEAT))
def test_heat_average(native, handle, name):
    """Both forms against the reference and against each other, as bit patterns (the sign of a
    zero included)."""
    ref = pc.bits(pc.heat_reference(name))
    rc, per_scale = _heat(native, handle, name, 0)
    handle.check(rc)
    assert np.array_equal(pc.bits(per_scale), ref), name + ": a launch per scale"
    rc, one = _heat(native, handle, name, 1)
    if name in pc.HEAT_REFUSED:  # refused before any launch: nothing written
        assert rc == pc.OPOSE_E_ARG and np.isnan(one).all()
        return
    handle.check(rc)
    assert np.array_equal(pc.bits(one), ref), name + ": one launch"
    assert np.array_equal(pc.bits(one), pc.bits(per_scale))


# ------------------------------------------------------------------------------ hand threshold
@pytest.mark.parametrize("name", list(pc.HAND))
def test_hand_threshold(native, handle, name):
    """gauss_threshold's cold tiles (-1 written, early return) beside a hot one, one component over
    every tile, and a constant map at the threshold: labels equal scipy.ndimage.label's, component
    sums within 1e-12 (the bar of test_hand_labels_match_scipy: the sums' order is the kernel's)."""
    H, W, thre = pc.HAND[name]
    maps = pc.hand_map(name)
    NP = len(maps)
    labels = np.full((NP, H, W), -7, np.int32)
    sums = np.full((NP, H, W), np.nan, F64)
    handle.check(native.lib.opose_debug_hand_label(handle.h, maps.ctypes.data, NP, H, W, thre, labels.ctypes.data,
                                                   sums.ctypes.data))
    for k, (expect, first, ref_sums) in enumerate(pc.hand_reference(name)):
        assert np.array_equal(labels[k], expect), (name, k)
        assert len(first) >= 1
        np.testing.assert_allclose(sums[k].ravel()[first], ref_sums, rtol=1e-12, atol=1e-12)
