"""GPU: the fast mode's kernels (`Batch_body`, `Batch_hand`: torch conventions) one stage at a
time -- preprocess_torch_u8, the two torch-tap resizes on every staged-row bucket and on the
thread-per-pixel fallback, blur5_nms, blur5_seed + cc_union -- each against the float64 oracle
of the same operation, at the sizes where such kernels go wrong: map borders (reflection, zero
neighbours), 32-pixel tile edges, exact ties, ragged tiles, 64-pixel run segments, row groups
and column blocks that end short.  Then the public post paths at sizes no golden covers.

The cases, the float bar (within 4 e_ref of the float64 oracle, mean error within twice the
float32 oracle's) and the conditions of the exact comparisons are in tests/fast_stage_cases.py;
tests/test_fast_stage_cases.py asserts the conditions from the oracle alone.  Every float case
reports its error in units of e_ref."""
import numpy as np
import pytest

import fast_stage_cases as fc
from conftest import report
from oracle import batch_post

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def handle(native):
    return native.Handle(0)


def _bar(name, got, ref32, ref64):
    worst, mean, bad = fc.float_bar(got, ref32, ref64)
    line = "fast stage %-44s max err %.2f e_ref (e_ref %.3g), mean err %.2f x the float32 oracle's" % (
        name, worst, fc.e_ref(ref32, ref64), mean)
    print(line)
    report(line)
    assert bad is None, name + ": " + bad


# ------------------------------------------------------------------------------ preprocess
@pytest.mark.parametrize("name", [c[0] for c in fc.PREPROCESS])
def test_preprocess(native, handle, name):
    """ToTensor, torch bicubic at float(1 / scale_factor), - 0.5, zero pad (preprocess_torch_u8)."""
    frames, x32, x64, (H, W, nh, nw) = fc.preprocess_case(name)
    v, ptr, N, h, w, rs, fs, _ = native.frames_view(frames)
    assert (h, w) == (H, W) and (rs != 3 * W) == name.startswith("roi")
    hw = np.zeros(2, np.int32)
    handle.check(native.lib.opose_debug_batch_preprocess(handle.h, ptr, N, H, W, rs, fs, 368.0, 0.5, None,
                                                         hw.ctypes.data))
    assert (N, 3) + tuple(hw) == x64.shape
    out = np.full(x64.shape, np.nan, np.float32)
    handle.check(native.lib.opose_debug_batch_preprocess(handle.h, ptr, N, H, W, rs, fs, 368.0, 0.5, out.ctypes.data,
                                                         hw.ctypes.data))
    pad_rows, pad_cols = out[:, :, nh:], out[:, :, :, nw:]  # empty where nh, nw are multiples of 8
    assert np.array_equal(pad_rows, np.zeros_like(pad_rows)) and np.array_equal(pad_cols, np.zeros_like(pad_cols))
    _bar("preprocess " + name, out[:, :, :nh, :nw], x32[:, :, :nh, :nw], x64[:, :, :nh, :nw])


# ---------------------------------------------------------------------------- resize chain
@pytest.mark.parametrize("case", fc.RESIZE, ids=lambda c: "%dx%d_box%d" % c)
def test_resize_chain(native, handle, case):
    """launch_upsample8_torch (mid) and launch_resize_torch_f32 (heat): the 8-, 16- and 44-row
    staged buckets, the last size the staged rows hold, and the thread-per-pixel resize beyond."""
    H, W, _ = case
    maps, (_, _, nh, nw), (m32, h32), (m64, h64) = fc.resize_case(*case)
    N, _, hl, wl = maps.shape
    heat = np.full(h64.shape, np.nan, np.float32)
    mid = np.full(m64.shape, np.nan, np.float32)
    handle.check(native.lib.opose_debug_batch_heat(handle.h, maps.ctypes.data, N, hl, wl, nh, nw, H, W,
                                                   heat.ctypes.data, mid.ctypes.data))
    name = "%dx%d box %d" % case
    _bar("resize mid " + name, mid, m32, m64)
    _bar("resize heat " + name, heat, h32, h64)
    if (nh, nw) == (H, W):  # torch's coefficients at lambda 0 are exactly (0, 1, 0, 0)
        assert np.array_equal(heat.view(np.uint32), np.ascontiguousarray(mid[:, 38:56]).view(np.uint32))
    only_heat = np.full(h64.shape, np.nan, np.float32)  # mid is optional
    handle.check(native.lib.opose_debug_batch_heat(handle.h, maps.ctypes.data, N, hl, wl, nh, nw, H, W,
                                                   only_heat.ctypes.data, None))
    assert np.array_equal(only_heat, heat)


# ------------------------------------------------------------------------------ blur + NMS
def _blur5_nms(native, handle, heat, thre, cap):
    heat = np.ascontiguousarray(heat, np.float32)
    NP, H, W = heat.shape
    cnt = np.full(NP, -7, np.int32)
    lst = np.full((NP, cap), -7, np.int32)
    score = np.full((NP, cap), np.nan, np.float64)
    handle.check(native.lib.opose_debug_blur5_nms(handle.h, heat.ctypes.data, NP, H, W, float(thre), cap,
                                                  cnt.ctypes.data, lst.ctypes.data, score.ctypes.data))
    return cnt, lst, score


def _sorted_peaks(cnt, lst, score, k):
    n = int(cnt[k])
    assert 0 <= n <= lst.shape[1] and (lst[k, n:] == -1).all()
    order = np.argsort(lst[k, :n])
    return lst[k, :n][order], score[k, :n][order]


@pytest.mark.parametrize("case", fc.BLUR_NMS, ids=lambda c: "%dx%d_thre%g_seed%d" % c)
def test_blur5_nms_random(native, handle, case):
    """White noise: a peak every few pixels, on the border, on both sides of every tile edge.  The
    peak set is the float64 oracle's (every decision is 8 e_ref clear there); the scores meet the
    float bar."""
    H, W, thre, _ = case
    heat, b32, b64, margin = fc.blur_nms_case(*case)
    cnt, lst, score = _blur5_nms(native, handle, heat, thre, H * W)
    got, s32, s64 = [], [], []
    for k, ref in enumerate(fc.peak_sets(margin)):
        idx, sc = _sorted_peaks(cnt, lst, score, k)
        assert np.array_equal(idx, ref), (k, np.setxor1d(idx, ref)[:8])
        got.append(sc)
        s32.append(b32[k].ravel()[ref])
        s64.append(b64[k].ravel()[ref])
    got, s32, s64 = np.concatenate(got), np.concatenate(s32), np.concatenate(s64)
    e = fc.e_ref(b32, b64)  # of the blurred maps, as for every other stage; the means over the peaks
    worst = float(np.abs(got - s64).max()) / e
    mean = float(np.abs(got - s64).mean() / np.abs(s32 - s64).mean())
    line = "fast stage %-44s max err %.2f e_ref (e_ref %.3g), mean err %.2f x the float32 oracle's" % (
        "blur5_nms scores %dx%d thre %g" % (H, W, thre), worst, e, mean)
    print(line)
    report(line)
    assert worst <= fc.BAR and mean <= 2, line
    assert np.array_equal(got, got.astype(np.float32))  # float32 values


def test_blur5_nms_constant_map_is_all_peaks(native, handle):
    """'>=' against the neighbours: on a constant map every blurred value is the same sum in the
    same order, so every pixel is a peak."""
    H, W = 33, 65
    cnt, lst, score = _blur5_nms(native, handle, np.full((2, H, W), 0.5, np.float32), 0.1, H * W)
    for k in range(2):
        idx, sc = _sorted_peaks(cnt, lst, score, k)
        assert np.array_equal(idx, np.arange(H * W))
        assert (sc == sc[0]).all() and abs(sc[0] - 0.5 * np.float32(batch_post.GAUSS5).sum(dtype=np.float64)) < 1e-6


def test_blur5_nms_border_spikes(native, handle):
    """A single 1.0 at each corner and at the middle of each edge: exactly that pixel is a peak (a
    neighbour outside the map counts as zero, not as its reflection), and its score is the centre
    weight exactly: the reflection must not show the spike twice."""
    H, W = 33, 65
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 32), (H - 1, 32), (16, 0), (16, W - 1)]
    heat = np.zeros((len(spots), H, W), np.float32)
    for k, (y, x) in enumerate(spots):
        heat[k, y, x] = 1.0
    cnt, lst, score = _blur5_nms(native, handle, heat, 0.1, H * W)
    for k, (y, x) in enumerate(spots):
        idx, sc = _sorted_peaks(cnt, lst, score, k)
        assert idx.tolist() == [y * W + x], (k, idx)
        assert sc[0] == float(np.float32(0.22508352))


def test_blur5_nms_ties_across_tile_edges(native, handle):
    """Two equal adjacent 1.0 pixels across x = 31|32 and across y = 31|32: both are peaks.  Each
    blurred value is a two-term sum with symmetric weights, an exact tie in any order."""
    H, W = 40, 70
    heat = np.zeros((2, H, W), np.float32)
    heat[0, 10, 31] = heat[0, 10, 32] = 1.0
    heat[1, 31, 10] = heat[1, 32, 10] = 1.0
    cnt, lst, score = _blur5_nms(native, handle, heat, 0.1, H * W)
    expect = [[10 * W + 31, 10 * W + 32], [31 * W + 10, 32 * W + 10]]
    for k in range(2):
        idx, sc = _sorted_peaks(cnt, lst, score, k)
        assert idx.tolist() == expect[k], (k, idx)
        assert sc[0] == sc[1] == float(np.float32(0.22508352) + np.float32(0.11098164))


def test_blur5_nms_cap_below_the_peak_count(native, handle):
    """cnt is the true count; the list holds cap distinct members of the true set."""
    case = fc.BLUR_NMS[4]
    H, W, thre, _ = case
    heat, b32, b64, margin = fc.blur_nms_case(*case)
    cap = 5
    cnt, lst, score = _blur5_nms(native, handle, heat, thre, cap)
    for k, ref in enumerate(fc.peak_sets(margin)):
        assert len(ref) > cap and cnt[k] == len(ref)
        assert len(set(lst[k].tolist())) == cap and np.isin(lst[k], ref).all()
        assert np.abs(score[k] - b64[k].ravel()[lst[k]]).max() <= fc.BAR * fc.e_ref(b32, b64)


# --------------------------------------------------------------------------- hand labelling
@pytest.mark.parametrize("shape", fc.HAND_LABEL, ids=lambda s: "%dx%d" % s)
def test_batch_hand_labels_match_scipy(native, handle, shape):
    """blur5_seed's blurred map and run seeds, cc_union and cc_compress_sum, label for label against
    scipy.ndimage.label (8-connectivity) of the float64 blurred map at a threshold that sits in the
    widest gap of its values: ragged 64 x 16 tiles, runs across 64-pixel segments."""
    H, W = shape
    heat, b32, b64, thre, gap = fc.hand_label_case(H, W)
    NP = heat.shape[0]
    blurred = np.full((NP, H, W), np.nan, np.float64)
    labels = np.full((NP, H, W), -7, np.int32)
    sums = np.full((NP, H, W), np.nan, np.float64)
    handle.check(native.lib.opose_debug_batch_hand_label(handle.h, heat.ctypes.data, NP, H, W, thre,
                                                         blurred.ctypes.data, labels.ctypes.data, sums.ctypes.data))
    _bar("hand blurred %dx%d" % shape, blurred, b32, b64)
    assert np.array_equal(blurred, blurred.astype(np.float32))  # float32 values
    ncomp = 0
    for k in range(NP):
        expect, first, lab = fc.label_first_pixel(b64[k] > thre)
        ncomp += len(first)
        assert np.array_equal(labels[k], expect), (k, np.argwhere(labels[k] != expect)[:8])
        got = sums[k].ravel()[first]
        np.testing.assert_allclose(got, np.bincount(lab.ravel(), weights=b64[k].ravel())[1:], rtol=1e-6)
        # the summation itself: the float64 sum of the kernel's own float32 summands
        np.testing.assert_allclose(got, np.bincount(lab.ravel(), weights=blurred[k].ravel())[1:], rtol=1e-12)
    assert ncomp > 10


# ------------------------------------------------------------------------- public hand post
@pytest.fixture(scope="module")
def bh():
    from src.batch_model import Batch_hand
    from src.weights import seeded_state_dict
    return Batch_hand(seeded_state_dict("hand", 0))


@pytest.mark.parametrize("case", fc.HAND_POST, ids=lambda c: "%dx%d_seed%d" % c)
def test_batch_hand_post_hovering_maps(native, bh, case):
    """Batch_hand.post on maps that hover around the threshold (many components per part) against
    the oracle: x and y equal, score at rtol 1e-5, except the parts fast_stage_cases excludes."""
    heat, thre, gap, e, ref32, ref64, excluded = fc.hand_post_case(*case)
    params = bh.params
    bh.params = native.default_params(native.NET_HAND, scale_search=(1.0,), thre_hand=float(thre))  # Batch_hand(thre=)
    try:
        got = bh.post(heat)
    finally:
        bh.params = params
    keep = ~excluded
    assert excluded.mean() <= fc.HAND_EXCLUDED_SHARE
    assert got.dtype == ref32.dtype and got.shape == ref32.shape
    assert np.array_equal(got[keep][:, :2], ref32[keep][:, :2])
    np.testing.assert_allclose(got[keep][:, 2], ref32[keep][:, 2], rtol=1e-5)


# ------------------------------------------------------------------------- public body post
@pytest.fixture(scope="module")
def bodies():
    from src.batch_model import Batch_body
    from src.weights import seeded_state_dict
    made = {}

    def get(boxsize):
        if boxsize not in made:
            made[boxsize] = Batch_body(seeded_state_dict("body", 0), boxsize=boxsize)
        return made[boxsize]
    return get


@pytest.mark.parametrize("case", fc.BODY_POST, ids=lambda c: "%dx%d_box%d_seed%d_p%d" % c)
def test_batch_body_post_planted_scenes(bodies, case):
    """Batch_body.post on planted people at sizes no golden covers -- frames too short for the
    staged resize, the last that fits, both small buckets -- against the oracle at the bar of
    test_gpu_batch_model: pixels, ids and subsets identical, scores at rtol 1e-5."""
    from test_gpu_batch_model import _same
    H, W, boxsize = case[:3]
    maps, ref, margin, e, _ = fc.body_post_case(*case)
    assert margin >= fc.DECIDE * e
    res = bodies(boxsize).post(maps, H, W)
    assert len(res) == len(ref) == 2
    for got, (cand, subset) in zip(res, ref):
        assert len(subset) >= 1
        _same(got, np.asarray(cand, np.float64), np.asarray(subset, np.float64), rtol=1e-5)
