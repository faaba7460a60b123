"""GPU: every conv kernel family of the networks, one layer at a time, against float64.

The hooks (opose_debug_conv_segs / _chain / _conv1, csrc/engine_debug.cpp) run the forward's own
launch paths -- run_conv_x6_segs with its planner, the fused 1x1 chain, conv1_1's direct kernel
and conv1_2's window kernel -- on the cases of tests/conv_layer_cases.py.  For every case: the
planner reports the intended kernel family and k slabs, no 16-byte unit outside the written slice
of any output allocation changes (X6P pads, neighbouring groups of a concat buffer, fp32 channels
outside the slice), the X6 and the fp32 epilogue agree bit for bit, and so does a duplicate
destination.  Dense cases are held to the layer bar of tests/test_gpu_x6.py, one-hot cases to
2^-21 of the single product (conv_layer_cases.py derives both).

Each test also reports its mean error as a ratio to the float32 CPU oracle's (torch float32 conv2d
against float64); it is printed, not asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_layer_cases as cc
from conftest import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def handle(native):
    return native.Handle(0)


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def conv_segs(native, handle, xs, ws, bs, slabs, offs, *, family, out_kind, out_total, relu=True, pool=False,
              in_padded=True, dup=False, net=0, lvl=3, pair=False):
    """opose_debug_conv_segs: segment i on weight set i % len(ws).  -> outs, dups, ran, clobbered"""
    cout, cin, ks, _ = ws[0].shape
    geom = np.array([[x.shape[0], x.shape[2], x.shape[3], s, i % len(ws), o]
                     for i, (x, s, o) in enumerate(zip(xs, slabs, offs))], np.int32)
    shapes = [(x.shape[0], cout) + tuple(d // 2 if pool else d for d in x.shape[2:]) for x in xs]
    outs = [np.full(s, np.nan, np.float32) for s in shapes]
    dups = [np.full(s, np.nan, np.float32) for s in shapes]
    ran = np.full((len(xs), 2), -9, np.int32)
    clobbered = np.full(1, -1, np.int64)
    handle.check(native.lib.opose_debug_conv_segs(
        handle.h, len(xs), geom.ctypes.data, _ptrs(xs), len(ws), _ptrs(ws), _ptrs(bs), cin, cout, ks, int(relu), family,
        int(pool), int(in_padded), out_kind, out_total, int(dup), net, lvl, int(pair), _ptrs(outs),
        _ptrs(dups) if dup else None, ran.ctypes.data, clobbered.ctypes.data))
    return outs, dups if dup else None, ran, int(clobbered[0])


def mfma32(native, handle, x, w, b, relu, whole=False):
    """The fp32 MFMA kernel (opose_debug_conv) on one layer.  whole: a data-parallel grid of
    128 x 128 (Cout <= 64: 64 x 128) tiles, every output summed in one run over k like a one-slab
    run of the kernels under test (as tests/test_gpu_x6.py gives both kernels one tile and split);
    else the kernel's own plan, which splits k over stream-K workgroups on small layers."""
    n, cin, h, wd = x.shape
    cout, _, ks, _ = w.shape
    out = np.empty((n, cout, h, wd), np.float32)
    mt, pt = ((64 if cout <= 64 else 128), 128) if whole else (0, 0)
    handle.check(native.lib.opose_debug_conv(handle.h, x.ctypes.data, w.ctypes.data, b.ctypes.data, n, cin, h, wd, cout,
                                             ks, ks // 2, int(relu), mt, pt, 0, out.ctypes.data))
    return out


def pool2(y):
    return F.max_pool2d(torch.from_numpy(y), 2, 2).numpy()


def dense_bar(what, y, y32, ref, bound, o32, y32_plan=None):
    """The layer bar: elementwise |y - ref| <= bound, and the mean error relative to mag within 3x
    the fp32 MFMA kernel's on the same inputs.  Reports (worst |err| / bound, mean ratio to the
    MFMA kernel, mean ratio to the float32 CPU oracle) and, given y32_plan (the MFMA kernel on its
    own stream-K plan), the mean ratio to that as well."""
    assert y.shape == ref.shape and np.isfinite(y).all(), what
    mag = np.maximum((bound - cc.ABS) / cc.REL, 1e-30)
    e = np.abs(y - ref)
    worst = float((e / bound).max())
    m, m32, mo = (float((np.abs(a - ref) / mag).mean()) for a in (y, y32, o32))
    print("%s: max |err| / bound %.4f, mean error %.3g = %.3f x MFMA fp32 = %.3f x float32 CPU oracle"
          % (what, worst, m, m / m32, m / mo))
    report("conv layers %-42s |err|/bound %.4f  mean/MFMA %.3f  mean/oracle %.3f" % (what, worst, m / m32, m / mo))
    if y32_plan is not None:
        mp = float((np.abs(y32_plan - ref) / mag).mean())
        print("%s: mean error %.3f x MFMA fp32 on its own plan" % (what, m / mp))
        report("conv layers %-42s mean/MFMA own plan %.3f" % (what, m / mp))
    assert worst <= 1, (what, worst)
    assert m <= 3 * m32 + 1e-9, (what, m, m32)


def check_ran(ran, reports, slabs, clobbered, what):
    assert (ran[:, 0] == reports).all(), (what, ran.tolist())
    for got, want in zip(ran[:, 1], slabs):
        assert got == want if want else got >= 1, (what, ran.tolist())
    assert clobbered == 0, (what, clobbered)


# ---------------------------------------------------------------------------------- dense cases
DENSE_RUNS = [(name, i) for name, c in cc.DENSE.items() for i in range(len(c["runs"]))]
_mfma_cache = {}


@pytest.mark.parametrize("name,ri", DENSE_RUNS, ids=["%s-run%d" % r for r in DENSE_RUNS])
def test_dense_layer(native, handle, name, ri):
    """One conv layer on the family and slab count of the run, written once as an X6P group slice
    with a duplicate and once as fp32 channels (pooled: as dense X6).  The fp32 MFMA kernel of the
    mean check sums each output in one run over k (mfma32 whole=True), like a one-slab run under
    test; the ratio to the same kernel on its own plan, which splits k over stream-K workgroups on
    layers this small, is printed beside it and listed here, so that a growth of the summation
    error shows against either.

    Measured on an MI355X -- worst |err| / bound, then the mean error as a ratio to the MFMA
    kernel's in one run over k (asserted <= 3), to the MFMA kernel's on its own plan, and to the
    float32 CPU oracle's (both printed, not asserted):
      win7_bench_2x23x41   slabs 1: 0.069 1.16 3.82 2.84   3: 0.031 0.76 2.49 1.85
                           slabs 7: 0.017 0.52 1.72 1.28   conv_x6, 4 slabs: 0.027 0.67 2.19 1.62
      win7_two_frames_3x17x19       0.074 1.19 4.91 3.49
      win7_19groups_2x9x13          0.070 1.19 4.99 3.19
      win7_one_tile_5x6x7  slabs 1: 0.075 1.21 2.37 1.19   5: 0.033 0.71 1.38 0.69
      win7_3groups_2x11x11          0.068 1.18 2.80 1.52
      win7_large_2x20x61            0.075 1.17 2.88 1.51
      win7_large_1x40x100           0.078 1.16 2.50 1.78
      win3_large_2x12x120           0.078 1.17 2.76 2.69
      wino3_2x23x41        window:  0.085 1.17 2.80 2.79   Winograd: 0.047 0.90 2.15 2.14
      win7_per_frame_2x46x82        0.037 0.66 0.66 0.86   (the same under the hand policy's 4 slabs)
      win7_two_segments    seg 0:   0.101 1.18 3.88 2.88   seg 1 (4 slabs): 0.018 0.64 2.64 1.61
      two_segments_cout19  seg 0:   0.062 1.16 4.58 2.75   seg 1 (4 slabs): 0.017 0.62 2.78 1.57
      pooled_x6_2x19x23    slabs 1: 0.061 1.19 2.45 2.34   3: 0.030 0.72 1.48 1.41"""
    c, r = cc.DENSE[name], cc.DENSE[name]["runs"][ri]
    xs, ws, bs, refs = cc.dense_case(name)
    cout, og, pool = c["cout"], (c["cout"] + 7) // 8, r["pool"]
    nseg = len(xs)
    kw = dict(family=r["family"], pool=pool, in_padded=r["in_padded"], net=r["net"], lvl=r["lvl"], pair=r["pair"])
    want = r["planned"] or r["slabs"]  # the slab counts the segments must report
    if nseg == 2:
        xkind, xtotal, xoffs = cc.TWO_SEG_X6P
        fkind, ftotal, foffs = cc.TWO_SEG_F32 if cout == 19 else (cc.OUT_F32, 38 + cout + 3, (38, 38))
    else:
        xkind, xtotal, xoffs = cc.OUT_X6P, og + 3, (1,)
        fkind, ftotal, foffs = cc.OUT_F32, cout + 7, (3,)
    what = "%s%s family %d slabs %s" % (name, " hand" if r["net"] else "", r["family"], "/".join(map(str, r["slabs"])))
    y6, d6, ran, clob = conv_segs(native, handle, xs, ws, bs, r["slabs"], xoffs, out_kind=xkind, out_total=xtotal,
                                  dup=not pool, **kw)
    check_ran(ran, r["reports"], want, clob, what + " (X6P out)")
    if pool:  # the pooled epilogue writes X6 only: padded against dense
        yf, _, ran, clob = conv_segs(native, handle, xs, ws, bs, r["slabs"], (2,) * nseg, out_kind=cc.OUT_X6,
                                     out_total=og + 3, **kw)
    else:
        yf, _, ran, clob = conv_segs(native, handle, xs, ws, bs, r["slabs"], foffs, out_kind=fkind, out_total=ftotal, **kw)
    check_ran(ran, r["reports"], want, clob, what + " (second output kind)")
    for i in range(nseg):
        assert np.array_equal(y6[i], yf[i]), what          # the split epilogue is lossless
        if d6:
            assert np.array_equal(d6[i], y6[i]), what      # the duplicate destination
        k = i % c["nw"]
        if (name, i, pool) not in _mfma_cache:
            y32 = [mfma32(native, handle, xs[i], ws[k], bs[k], True, whole=wh) for wh in (True, False)]
            _mfma_cache[name, i, pool] = [pool2(y) if pool else y for y in y32]
        ref, bound, o32 = refs[i, pool]
        y32, y32_plan = _mfma_cache[name, i, pool]
        dense_bar("%s seg %d" % (what, i), y6[i], y32, ref, bound, o32, y32_plan)


# ---------------------------------------------------------------------------------------- chain
def chain(native, handle, xs, wts, m1, cout2, relu2, in_padded, out_x6):
    nseg = len(xs)
    geom = np.array([[x.shape[0], x.shape[2], x.shape[3], i] for i, x in enumerate(xs)], np.int32)
    outs = [np.full((x.shape[0], cout2) + x.shape[2:], np.nan, np.float32) for x in xs]
    cols = [_ptrs([t[j] for t in wts]) for j in range(4)]
    handle.check(native.lib.opose_debug_chain(handle.h, nseg, geom.ctypes.data, _ptrs(xs), len(wts), *cols, m1, cout2,
                                              int(relu2), int(in_padded), int(out_x6), _ptrs(outs)))
    return outs


CHAIN_RUNS = [(name, relu2) for name, c in cc.CHAIN.items() for relu2 in c["relu2"]]


@pytest.mark.parametrize("name,relu2", CHAIN_RUNS, ids=["%s-relu%d" % r for r in CHAIN_RUNS])
def test_chain(native, handle, name, relu2):
    """conv1x1_chain_x6 against the float64 composition; the mean check against the fp32 MFMA
    kernel applied twice.  fp32 output from an X6P input and an X6P output from a dense input
    agree bit for bit.  Measured (worst |err| / bound, mean / MFMA, mean / float32 CPU oracle):
    chain_128_38 0.006 1.24 1.59; chain_128_19_two_segments 0.005 1.25 1.62 and 0.005 1.25 1.67;
    chain_512_22 0.004 1.80 1.18 (relu2: 0.004 1.77 1.16); chain_65_pixels 0.005 1.20 1.21."""
    c = cc.CHAIN[name]
    xs, wts, refs = cc.chain_case(name)
    yf = chain(native, handle, xs, wts, c["m1"], c["cout2"], relu2, True, False)
    y6 = chain(native, handle, xs, wts, c["m1"], c["cout2"], relu2, False, True)
    for i, (x, (w1, b1, w2, b2), (ref, bound, o32)) in enumerate(zip(xs, wts, refs)):
        assert np.array_equal(yf[i], y6[i]), name
        y32 = mfma32(native, handle, mfma32(native, handle, x, w1, b1, True), w2, b2, relu2)
        if relu2:
            ref, o32 = np.maximum(ref, 0), np.maximum(o32, 0)
        dense_bar("%s relu2 %d seg %d" % (name, relu2, i), yf[i], y32, ref, bound, o32)


# ---------------------------------------------------------------------------- conv1_1, conv1_2
def conv1(native, handle, stage, xs, w, b, f32):
    geom = np.array([[x.shape[0], x.shape[2], x.shape[3]] for x in xs], np.int32)
    d = 1 if stage == 1 else 2
    outs = [np.full((x.shape[0], 64, x.shape[2] // d, x.shape[3] // d), np.nan, np.float32) for x in xs]
    handle.check(native.lib.opose_debug_conv1(handle.h, stage, len(xs), geom.ctypes.data, _ptrs(xs), w.ctypes.data,
                                              b.ctypes.data, int(f32), _ptrs(outs)))
    return outs


@pytest.mark.parametrize("launch", cc.CONV1_LAUNCHES, ids=lambda l: "frames" + "".join(map(str, l)))
@pytest.mark.parametrize("stage", [1, 2])
def test_conv1(native, handle, stage, launch):
    """conv1_1 (conv_first_x6) and conv1_2 + pool (conv3_pool_win_x6) on whole, ragged and odd 8 x 16
    tiles, each frame alone and three in one launch, in both forms of the fp32 hand-off.  Measured
    (worst |err| / bound, mean / MFMA, mean / float32 CPU oracle): conv1_1 0.035-0.048, 1.00, 1.00
    (the same fp32 FMA chain); conv1_2 0.045-0.079, 2.27-2.36, 1.97-2.32."""
    xs_all, w, b, refs = cc.conv1_case(stage)
    xs = [xs_all[i] for i in launch]
    y_f32 = conv1(native, handle, stage, xs, w, b, True)
    y_x6 = conv1(native, handle, stage, xs, w, b, False)
    for k, i in enumerate(launch):
        assert np.array_equal(y_f32[k], y_x6[k]), (stage, launch, i)
        y32 = mfma32(native, handle, xs[k], w, b, True)
        ref, bound, o32 = refs[i]
        dense_bar("conv1_%d launch %s frame %d" % (stage, "".join(map(str, launch)), i), y_f32[k],
                  pool2(y32) if stage == 2 else y32, ref, bound, o32)


# -------------------------------------------------------------------------------------- one-hot
def one_hot_bar(what, y, exp, bound, mag, single):
    e = np.abs(y - exp)
    bad = e > bound
    units = float((e[mag > 0] / (2.0 ** -24 * mag[mag > 0])).max())
    assert not bad.any(), (what, "worst |err| = %.2f x 2^-24 |ab|" % units, np.argwhere(bad)[:4].tolist())
    assert (y[mag == 0] == 0).all(), what  # taps outside the frame
    return units if single else 0.0


@pytest.mark.parametrize("name", ["win7_small", "win7_large", "x6_3x3"])
def test_one_hot_gemm(native, handle, name):
    """Every output of the window kernel (small and large window) and of conv_x6 is one product
    x[c, y + dy, x + dx] * w (a last weight set: three), each k of the layer hit by some set, as one
    run over all chunks and as three slabs through conv_x6_fixup: within 2^-21 |a b| (multi-term:
    of the sum of |a_i b_i|, plus 2^-23 per extra addition), exact zeros outside the frame.
    Measured worst single-product error, in units of 2^-24 |a b| (the bar is 8): 5.04 (small
    window), 4.91 (large window), 4.79 (conv_x6)."""
    c = cc.ONE_HOT_CASES[name]
    x, sets = cc.one_hot_case(name)
    b = np.zeros(c["cout"], np.float32)
    worst = 0.0
    for slabs in c["slabs"]:
        for si, terms in enumerate(sets):
            w = cc.one_hot_weights(terms, c["cin"], c["ks"])
            exp, mag, nterms = cc.one_hot_expected(x, terms, c["ks"])
            what = "%s set %d slabs %d" % (name, si, slabs)
            (y,), _, ran, clob = conv_segs(native, handle, [x], [w], [b], (slabs,), (1,), family=c["family"],
                                           out_kind=cc.OUT_X6P, out_total=c["cout"] // 8 + 2, relu=False)
            check_ran(ran, c["family"], (slabs,), clob, what)
            worst = max(worst, one_hot_bar(what, y, exp, cc.one_hot_bound(mag, nterms), mag, nterms == 1))
    print("%s: worst single-product error %.2f x 2^-24 |ab| (bar: 8)" % (name, worst))
    report("conv layers one-hot %-12s worst %.2f x 2^-24 |ab|" % (name, worst))


def test_one_hot_chain_first(native, handle):
    """The chain's first conv: W1 one-hot, W2 selects 64 of the 128 intermediate channels with weight
    1: its pieces are (1, 0, 0), so the second GEMM only adds the three bf16 pieces of the fp32
    intermediate t, and every partial sum of them is exact in fp32 -- y is the first GEMM's result.
    Both signs of W1, so that the ReLU between the convs passes every product once: within
    2^-21 |a b|.  Measured worst: 4.54 x 2^-24 |a b|."""
    c = cc.ONE_HOT_CASES["chain_first"]
    x, (terms,) = cc.one_hot_case("chain_first")
    w1 = cc.one_hot_weights(terms, 128, 1)
    exp, mag, _ = cc.one_hot_expected(x, terms, 1)
    z1, z2 = np.zeros(128, np.float32), np.zeros(64, np.float32)
    worst = 0.0
    for half in (0, 1):
        w2 = np.zeros((64, 128, 1, 1), np.float32)
        w2[np.arange(64), np.arange(64) + 64 * half] = 1
        for sign in (1, -1):
            (y,) = chain(native, handle, [x], [(w1 * np.float32(sign), z1, w2, z2)], 128, 64, False, True, False)
            sl = slice(64 * half, 64 * half + 64)
            worst = max(worst, one_hot_bar("chain half %d sign %d" % (half, sign), y, np.maximum(sign * exp[:, sl], 0),
                                           cc.one_hot_bound(mag[:, sl], 1) * (sign * exp[:, sl] > 0), mag[:, sl], True))
    print("chain_first: worst error %.2f x 2^-24 |ab| (bar: 8)" % worst)
    report("conv layers one-hot chain_first  worst %.2f x 2^-24 |ab|" % worst)
    assert c["cin"] == 128


def test_one_hot_chain_second(native, handle):
    """The chain's second conv: W1 = +-identity, so the intermediate is relu(+-x) exactly (a product
    with 1 is the exact sum of x's three pieces), W2 one-hot with full mantissas over every k of the
    128 intermediate channels: within 2^-21 |a b|.  Measured worst: 4.13 x 2^-24 |a b|."""
    c = cc.ONE_HOT_CASES["chain_second"]
    x, sets = cc.one_hot_case("chain_second")
    eye = np.eye(128, dtype=np.float32).reshape(128, 128, 1, 1)
    z1, z2 = np.zeros(128, np.float32), np.zeros(64, np.float32)
    worst = 0.0
    for si, terms in enumerate(sets):
        w2 = cc.one_hot_weights(terms, 128, 1)
        for sign in (1, -1):
            exp, mag, _ = cc.one_hot_expected(np.maximum(sign * x, 0), terms, 1)
            (y,) = chain(native, handle, [x], [(eye * np.float32(sign), z1, w2, z2)], 128, 64, False, False, True)
            worst = max(worst, one_hot_bar("chain second set %d sign %d" % (si, sign), y, exp, cc.one_hot_bound(mag, 1),
                                           mag, True))
    print("chain_second: worst error %.2f x 2^-24 |ab| (bar: 8)" % worst)
    report("conv layers one-hot chain_second worst %.2f x 2^-24 |ab|" % worst)
    assert c["cout"] == 64


@pytest.mark.parametrize("stage", [1, 2])
def test_one_hot_conv1(native, handle, stage):
    """conv1_1 (fp32 FMA, no split): the product within 2^-23 |a b|; conv1_2 + pool: the 2x2 maximum
    of four products, each within 2^-21 |a b| (max is 1-Lipschitz: the 2x2 maximum of the bounds).
    Both kernels apply ReLU: each weight set runs with both signs.  Measured worst through conv1_1:
    0.99 x 2^-24 |a b|."""
    name = "conv1_%d" % stage
    c = cc.ONE_HOT_CASES[name]
    x, sets = cc.one_hot_case(name)
    b = np.zeros(64, np.float32)
    rel = cc.ONE_HOT_FMA if stage == 1 else cc.ONE_HOT
    worst = 0.0
    for si, terms in enumerate(sets):
        w = cc.one_hot_weights(terms, c["cin"], 3)
        exp, mag, _ = cc.one_hot_expected(x, terms, 3)
        for sign in (1, -1):
            e, bound, m = sign * exp, rel * mag, mag
            if stage == 2:
                e, bound, m = (F.max_pool2d(torch.from_numpy(a), 2, 2).numpy() for a in (e, bound, m))
            for f32 in (True, False):
                (y,) = conv1(native, handle, stage, [x], w * np.float32(sign), b, f32)
                worst = max(worst, one_hot_bar("%s set %d sign %d f32 %d" % (name, si, sign, f32), y, np.maximum(e, 0),
                                               bound, m, stage == 1))
    if stage == 1:
        print("conv1_1: worst error %.2f x 2^-24 |ab| (bar: 2)" % worst)
        report("conv layers one-hot conv1_1      worst %.2f x 2^-24 |ab|" % worst)
