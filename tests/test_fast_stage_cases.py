"""CPU: the inputs of tests/test_gpu_fast_stages.py meet the conditions its exact comparisons
rest on, from the float64 oracle alone -- peak margins, threshold gaps, the share of excluded
parts, component counts -- so that a badly seeded case fails here and not on the GPU.  Also the
float32 oracle (the reference's arithmetic) against the float64 one: their difference e_ref, the
unit of every float bar, must be what float32 rounding explains, and the two must decide every
exact comparison alike."""
import numpy as np
import pytest

import fast_stage_cases as fc

EPS = float(np.finfo(np.float32).eps)


def _coordinate_bound(extent, vmax):
    """What float32 can cost a bicubic resize against float64.  The source coordinate
    scale * (d + 0.5) - 0.5 is a float32 product: off by up to eps * extent pixels, at a slope of
    at most 2 vmax per pixel (a cubic through values in [-vmax, vmax] overshoots by 1/8 at most);
    the two four-term sums add a few eps vmax."""
    return 2 * vmax * EPS * extent + 32 * EPS * vmax


def _sum_bound(vmax):
    """25 float32 products and sums of values up to vmax with weights that sum to 1."""
    return 32 * EPS * vmax


@pytest.mark.parametrize("name", [c[0] for c in fc.PREPROCESS])
def test_preprocess_cases(name):
    frames, x32, x64, (h, w, nh, nw) = fc.preprocess_case(name)
    assert frames.shape == (2, h, w, 3) and x32.shape == x64.shape
    assert x32.shape[2] % 8 == 0 and x32.shape[3] % 8 == 0 and x32.shape[2] - nh < 8 and x32.shape[3] - nw < 8
    assert (frames.strides[1] != 3 * w) == name.startswith("roi")
    assert not x64[:, :, nh:].any() and not x64[:, :, :, nw:].any()
    e = fc.e_ref(x32, x64)
    assert 0 < e <= _coordinate_bound(max(h, w), 1.0), e


@pytest.mark.parametrize("case", fc.RESIZE, ids=lambda c: "%dx%d_box%d" % c)
def test_resize_cases(case):
    H, W, boxsize = case
    maps, (h, w, nh, nw), (m32, h32), (m64, h64) = fc.resize_case(*case)
    assert m64.shape == (2, 56, nh, nw) and h64.shape == (2, 18, H, W)
    vmax = float(np.abs(maps).max()) * 1.25
    assert 0 < fc.e_ref(m32, m64) <= _coordinate_bound(max(maps.shape[2:]), vmax)
    assert 0 < fc.e_ref(h32, h64) <= _coordinate_bound(max(nh, nw), vmax) + fc.e_ref(m32, m64)
    # the staged rows hold a workgroup's 16 output rows up to nh / H = 2.4375
    assert (nh / H <= 2.4375) == (case not in [(75, 120, 368), (53, 97, 368), (9, 24, 368)])
    if (nh, nw) == (H, W):  # torch's coefficients at lambda 0 are exactly (0, 1, 0, 0)
        assert np.array_equal(h32, m32[:, 38:56])


@pytest.mark.parametrize("case", fc.BLUR_NMS, ids=lambda c: "%dx%d_thre%g_seed%d" % c)
def test_blur_nms_cases(case):
    H, W, thre, _ = case
    heat, b32, b64, margin = fc.blur_nms_case(*case)
    e = fc.e_ref(b32, b64)
    assert 0 < e <= _sum_bound(1.0)
    assert np.abs(margin).min() >= fc.DECIDE * e, (np.abs(margin).min(), e)
    peaks = fc.peak_sets(margin)
    assert all(len(p) for p in peaks)
    for got, ref in zip(fc.peak_sets(fc.peak_margin(b32.astype(np.float64), thre)), peaks):
        assert np.array_equal(got, ref)
    # what a planted person rarely does: peaks on the border, and next to a 32-pixel tile edge
    ys, xs = np.concatenate(peaks) // W, np.concatenate(peaks) % W
    assert ((ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)).any()
    if W > 32:
        assert ((xs == 31) | (xs == 32)).sum() >= 2
    if H > 32:
        assert ((ys == 31) | (ys == 32)).sum() >= 2


@pytest.mark.parametrize("shape", fc.HAND_LABEL, ids=lambda s: "%dx%d" % s)
def test_hand_label_cases(shape):
    H, W = shape
    heat, b32, b64, thre, gap = fc.hand_label_case(H, W)
    e = fc.e_ref(b32, b64)
    assert 0 < e <= _sum_bound(float(np.abs(heat).max()))
    assert 0.03 <= thre <= 0.04 and gap >= fc.DECIDE * e, (gap, e)
    ncomp, crossing = 0, 0
    for k in range(3):
        lab64, first, lab = fc.label_first_pixel(b64[k] > thre)
        assert np.array_equal(fc.label_first_pixel(b32[k] > thre)[0], lab64)
        ncomp += len(first)
        s64 = np.bincount(lab.ravel(), weights=b64[k].ravel())[1:]
        s32 = np.bincount(lab.ravel(), weights=b32[k].astype(np.float64).ravel())[1:]
        np.testing.assert_allclose(s32, s64, rtol=1e-6)
        if W > 64:
            crossing += int(((lab64[:, 63] >= 0) & (lab64[:, 64] >= 0)).sum())
    assert ncomp > 10
    assert crossing > 0 or W <= 64  # runs that cross a 64-pixel segment boundary


@pytest.mark.parametrize("case", fc.HAND_POST, ids=lambda c: "%dx%d_seed%d" % c)
def test_hand_post_cases(case):
    heat, thre, gap, e, ref32, ref64, excluded = fc.hand_post_case(*case)
    assert 0.03 <= thre <= 0.04 and gap >= fc.DECIDE * e > 0, (gap, e)
    assert excluded.mean() <= fc.HAND_EXCLUDED_SHARE, excluded.sum()
    keep = ~excluded
    assert ref32.dtype == ref64.dtype == np.float64 and (ref64[:, :, 2] > thre).all()  # every part found
    assert np.array_equal(ref32[keep][:, :2], ref64[keep][:, :2])
    np.testing.assert_allclose(ref32[keep][:, 2], ref64[keep][:, 2], rtol=1e-5)


@pytest.mark.parametrize("case", fc.BODY_POST, ids=lambda c: "%dx%d_box%d_seed%d_p%d" % c)
def test_body_post_cases(case):
    maps, ref, margin, e, same = fc.body_post_case(*case)
    assert maps.shape[:2] == (2, 57)
    assert margin >= fc.DECIDE * e > 0, (margin, e)
    assert same
    assert all(len(subset) >= 1 for _, subset in ref)
