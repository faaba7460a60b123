"""Case tables of the conv layer tests (tests/test_gpu_conv_layers.py on the GPU,
tests/test_conv_layer_cases.py for the inputs and bars alone): plain NumPy / torch on the CPU,
seeded, every input pinned by a digest.

Two kinds of case:

* dense random layers (post-ReLU normal x, He-scaled w, 0.1-scaled b, as tests/test_gpu_x6.py)
  against float64 F.conv2d, held to the project's layer bar |y - ref| <= 4e-6 * mag + 1e-6 with
  mag = conv(|x|, |w|) + |b|.  That bar is ~20-60x wider than fp32 summation noise, so it sees a
  wrong tap, a wrong k order or a dropped slab, but not a lost piece product (at most 2^-18 of a
  product, of random sign);
* one-hot layers: every output channel has one (a few sets: three) non-zero weights, x and w random
  fp32 with full mantissas in [0.5, 2) of both signs, so every output is a single product a * b (or
  a sum of three) and the bar is 2^-21 |a b|: the three dropped piece terms are below 2^-23 |a b|
  and six fp32 accumulator additions round by at most 6 * 2^-24 |a b| -- 1.75 * 2^-22 in all -- while
  a lost (1,1), (2,0) or (0,2) piece product costs up to 2^-18 |a b| (a piece is at most 2^-9 of
  the piece before it), 8x the bar, and more than the bar at a large share of the outputs
  (test_conv_layer_cases.py).  Over a case's weight sets every k = (channel, tap) of the layer is
  hit.
"""
import functools
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

# kernel families (csrc/engine.h)
PLANNER, X6, WIN, WIN_FRAMES, WINO = -1, 0, 1, 2, 3
# output kinds of opose_debug_conv_segs
OUT_F32, OUT_X6, OUT_X6P = 0, 1, 2

REL, ABS = 4e-6, 1e-6            # the layer bar
ONE_HOT = 2.0 ** -21             # single-term outputs, relative to |a b|
ONE_HOT_ADD = 2.0 ** -23         # per extra addition of a multi-term output, relative to sum |a_i b_i|
ONE_HOT_FMA = 2.0 ** -23         # conv1_1 (fp32 FMA, no split)


# ---------------------------------------------------------------------------------- split3
def bf16_rne(v):
    """float32 -> the nearest bf16 (ties to even) as float32."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def split3(v):
    """The three bf16 pieces of float32 values (x0 + x1 + x2 == x), as float32 arrays."""
    v = np.ascontiguousarray(v, np.float32)
    h0 = bf16_rne(v)
    r = v - h0
    h1 = bf16_rne(r)
    return h0, h1, bf16_rne(r - h1)


def third_piece_share(v):
    return float((split3(v)[2] != 0).mean())


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


# ------------------------------------------------------------------------------ dense cases
# name -> frames [(N, H, W)], Cin, Cout, ks, nw weight sets, and the runs: (family forced, the
# family the segments must report, slabs per segment (0: the planner's), pool, X6P input)
def _case(frames, cin, cout, ks, runs, nw=1):
    return dict(frames=frames, cin=cin, cout=cout, ks=ks, nw=nw, runs=runs)


def _run(family, reports, slabs, pool=False, in_padded=True, net=0, lvl=3, pair=False, planned=None):
    """net, lvl, pair: the layer as the slab policy sees it (0: body); planned: the slab counts the
    policy must arrive at where `slabs` leaves them to it"""
    return dict(family=family, reports=reports, slabs=slabs, pool=pool, in_padded=in_padded, net=net, lvl=lvl,
                pair=pair, planned=planned)


DENSE = {
    # the 7x7 window kernel, windows of at most 832 units (three weight stages)
    "win7_bench_2x23x41": _case([(2, 23, 41)], 128, 128, 7,        # 707 units; forced slabs: 196 chunks,
                                [_run(WIN, WIN, (1,)),             # the cuts inside channel groups
                                 _run(WIN, WIN, (3,)), _run(WIN, WIN, (7,)),
                                 _run(X6, X6, (4,))]),             # the im2col path on the X6P input
    "win7_two_frames_3x17x19": _case([(3, 17, 19)], 185, 128, 7, [_run(WIN, WIN, (1,))]),  # ragged last group
    "win7_one_tile_5x6x7": _case([(5, 6, 7)], 16, 128, 7,          # cin_g = 2: no group g + 2 prefetch
                                 [_run(WIN, WIN, (1,)), _run(WIN, WIN, (5,))]),
    "win7_19groups_2x9x13": _case([(2, 9, 13)], 150, 128, 7, [_run(WIN, WIN, (1,))]),  # last chunk padded
    "win7_3groups_2x11x11": _case([(2, 11, 11)], 24, 256, 7, [_run(WIN, WIN, (1,))]),  # nM = 2
    # windows of 833 .. 1088 units (two weight stages)
    "win7_large_2x20x61": _case([(2, 20, 61)], 24, 128, 7, [_run(WIN, WIN, (1,))]),     # 899 units
    "win7_large_1x40x100": _case([(1, 40, 100)], 40, 128, 7, [_run(WIN, WIN, (1,))]),   # 1033 units
    "win3_large_2x12x120": _case([(2, 12, 120)], 128, 128, 3, [_run(WIN, WIN, (1,))]),  # 985 units
    # the opt-in Winograd kernel through the same hook, beside the window kernel (the bench's H/8 3x3)
    "wino3_2x23x41": _case([(2, 23, 41)], 128, 256, 3, [_run(WIN, WIN, (1,)), _run(WINO, WINO, (1,))]),
    # the batch's window needs 1108 units, one frame's 938: one segment per frame
    # (as a hand layer: slab_count's hand table gives a segment of 30 window tiles 4 slabs)
    "win7_per_frame_2x46x82": _case([(2, 46, 82)], 24, 128, 7,
                                    [_run(PLANNER, WIN_FRAMES, (0,)),
                                     _run(PLANNER, WIN_FRAMES, (0,), net=1, planned=(4,))]),
    # two segments of different geometry and weights in one launch
    "win7_two_segments": _case([(2, 23, 41), (1, 9, 13)], 128, 128, 7, [_run(WIN, WIN, (1, 4))], nw=2),
    # Cout 19 has no window-kernel weights (Mpad 64): the planner's family, conv_x6
    "two_segments_cout19": _case([(2, 23, 41), (1, 9, 13)], 128, 19, 7, [_run(PLANNER, X6, (1, 4))], nw=2),
    # conv + 2x2 max-pool in conv_x6's epilogue; odd sizes: floor mode drops a row and a column;
    # three slabs: the pooled fold of conv_x6_fixup
    "pooled_x6_2x19x23": _case([(2, 19, 23)], 64, 128, 3,
                               [_run(X6, X6, (1,), pool=True, in_padded=False),
                                _run(X6, X6, (3,), pool=True, in_padded=False),
                                _run(X6, X6, (3,), pool=True, in_padded=True)]),
}
# where the two-segment cases write: (kind, allocation size, per-segment offset)
TWO_SEG_X6P = (OUT_X6P, 24, (5, 8))     # groups 5.. and 8.. of 24-group buffers, with a duplicate
TWO_SEG_F32 = (OUT_F32, 57, (38, 38))   # channels 38.. of 57-channel buffers


def _relu_inputs(rng, frames, cin, cout, ks, nw):
    xs = [np.maximum(rng.standard_normal((n, cin, h, w), dtype=np.float32), 0) for n, h, w in frames]
    ws = [rng.standard_normal((cout, cin, ks, ks), dtype=np.float32) * np.float32(np.sqrt(2 / (cin * ks * ks)))
          for _ in range(nw)]
    bs = [rng.standard_normal(cout, dtype=np.float32) * np.float32(0.1) for _ in range(nw)]
    return xs, ws, bs


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def conv_refs(x, w, b, pad, relu=True, pool=False):
    """(float64 reference, elementwise bound, float32 CPU oracle) of one conv (+ ReLU, + pool): the
    bound is the layer bar, through a pool its 2x2 maximum (max is 1-Lipschitz)."""
    xd, wd, bd = (torch.from_numpy(a).double() for a in (x, w, b))
    ref = F.conv2d(xd, wd, bd, padding=pad)
    bound = REL * F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=pad) + ABS
    o32 = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), padding=pad)
    if relu:
        ref, o32 = ref.clamp_min(0), o32.clamp_min(0)
    if pool:
        ref, bound, o32 = (F.max_pool2d(t, 2, 2) for t in (ref, bound, o32))
    return ref.numpy(), bound.numpy(), o32.numpy()


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """xs, ws, bs (segment i uses weight set i % nw) and, per (segment, pool), the references of
    conv_refs; shared by every run of the case, never modified."""
    c = DENSE[name]
    xs, ws, bs = _relu_inputs(np.random.default_rng(_seed(name)), c["frames"], c["cin"], c["cout"], c["ks"], c["nw"])
    refs = {}
    for pool in sorted({r["pool"] for r in c["runs"]}):
        for i, x in enumerate(xs):
            k = i % c["nw"]
            refs[i, pool] = conv_refs(x, ws[k], bs[k], c["ks"] // 2, True, pool)
    return xs, ws, bs, refs


# ------------------------------------------------------------------------------ chain cases
# name -> frames, m1, cout2, relu2 variants
CHAIN = {
    "chain_128_38": dict(frames=[(2, 17, 19)], m1=128, cout2=38, relu2=(False,)),
    "chain_128_19_two_segments": dict(frames=[(2, 17, 19), (2, 17, 19)], m1=128, cout2=19, relu2=(False,)),
    "chain_512_22": dict(frames=[(1, 9, 13)], m1=512, cout2=22, relu2=(False, True)),
    "chain_65_pixels": dict(frames=[(1, 5, 13)], m1=128, cout2=38, relu2=(False,)),  # the 2nd tile: one pixel
}


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """xs, (w1, b1, w2, b2) per segment, and per segment the float64 composition before the last
    ReLU, its bound and the float32 CPU oracle.  Bound: the layer bar of the second conv on the
    float64 intermediate plus the first conv's bar carried through |W2| (triangle inequality; ReLU
    is 1-Lipschitz)."""
    c = CHAIN[name]
    rng = np.random.default_rng(_seed(name))
    nseg = len(c["frames"])
    xs = [np.maximum(rng.standard_normal((n, 128, h, w), dtype=np.float32), 0) for n, h, w in c["frames"]]
    wts, refs = [], []
    for i in range(nseg):
        w1 = rng.standard_normal((c["m1"], 128, 1, 1), dtype=np.float32) * np.float32(np.sqrt(2 / 128))
        b1 = rng.standard_normal(c["m1"], dtype=np.float32) * np.float32(0.1)
        w2 = rng.standard_normal((c["cout2"], c["m1"], 1, 1), dtype=np.float32) * np.float32(np.sqrt(2 / c["m1"]))
        b2 = rng.standard_normal(c["cout2"], dtype=np.float32) * np.float32(0.1)
        wts.append((w1, b1, w2, b2))
        xd, w1d, b1d, w2d, b2d = (torch.from_numpy(a).double() for a in (xs[i], w1, b1, w2, b2))
        mid = F.conv2d(xd, w1d, b1d).clamp_min(0)
        bound1 = REL * F.conv2d(xd.abs(), w1d.abs(), b1d.abs()) + ABS
        ref = F.conv2d(mid, w2d, b2d)
        bound = REL * F.conv2d(mid.abs(), w2d.abs(), b2d.abs()) + ABS + F.conv2d(bound1, w2d.abs())
        t = [torch.from_numpy(a) for a in (xs[i], w1, b1, w2, b2)]
        o32 = F.conv2d(F.conv2d(t[0], t[1], t[2]).clamp_min(0), t[3], t[4])
        refs.append((ref.numpy(), bound.numpy(), o32.numpy()))
    return xs, wts, refs


# ------------------------------------------------------------------- conv1_1 / conv1_2 cases
CONV1_FRAMES = [(1, 8, 16), (2, 9, 17), (1, 24, 40), (1, 13, 50)]
# launches: each frame alone, and the first three as one launch of three segments
CONV1_LAUNCHES = [(0,), (1,), (2,), (3,), (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def conv1_case(stage):
    """stage 1: conv1_1 on network-input-like x [N,3,H,W]; stage 2: conv1_2 + pool on post-ReLU
    x [N,64,H,W].  xs per frame of CONV1_FRAMES, w, b and per frame the references of conv_refs."""
    rng = np.random.default_rng(_seed("conv1_%d" % stage))
    cin = 3 if stage == 1 else 64
    if stage == 1:
        xs = [rng.random((n, 3, h, w), dtype=np.float32) - np.float32(0.5) for n, h, w in CONV1_FRAMES]
    else:
        xs = [np.maximum(rng.standard_normal((n, 64, h, w), dtype=np.float32), 0) for n, h, w in CONV1_FRAMES]
    w = rng.standard_normal((64, cin, 3, 3), dtype=np.float32) * np.float32(np.sqrt(2 / (cin * 9)))
    b = rng.standard_normal(64, dtype=np.float32) * np.float32(0.1)
    return xs, w, b, [conv_refs(x, w, b, 1, True, stage == 2) for x in xs]


# ---------------------------------------------------------------------------- one-hot cases
def _full_mantissa(rng, shape):
    """random fp32 with full mantissas, magnitudes in [0.5, 2), both signs"""
    m = rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    e = rng.integers(126, 128, shape, dtype=np.uint32)   # 2^-1, 2^0
    s = rng.integers(0, 2, shape, dtype=np.uint32)
    return ((s << 31) | (e << 23) | m).view(np.float32)


def k_position(pos, order, cin, ks):
    """position `pos` of a family's k order -> (channel, tap).  "oihw": the reference layout;
    "win": conv_win_x6's pair order (pair q = (group, tap), 8 channels each); "x6": conv_x6's chunks
    of (4 groups, 1 tap) for cin a multiple of 32."""
    taps = ks * ks
    if order == "oihw":
        return pos // taps, pos % taps
    if order == "win":
        q, ci = divmod(pos, 8)
        return (q // taps) * 8 + ci, q % taps
    chunk, within = divmod(pos, 32)
    return (chunk // taps) * 32 + within, chunk % taps


# name -> geometry, the hook that runs it, the family's k order and the forced slab counts
ONE_HOT_CASES = {
    "win7_small": dict(frames=(3, 17, 19), cin=16, cout=128, ks=7, order="win", family=WIN, slabs=(1, 3)),
    "win7_large": dict(frames=(2, 20, 61), cin=16, cout=128, ks=7, order="win", family=WIN, slabs=(1, 3)),
    "x6_3x3": dict(frames=(2, 9, 13), cin=32, cout=128, ks=3, order="x6", family=X6, slabs=(1, 3)),
    "chain_first": dict(frames=(2, 9, 13), cin=128, cout=128, ks=1, order="oihw"),
    "chain_second": dict(frames=(2, 9, 13), cin=128, cout=64, ks=1, order="oihw"),
    "conv1_1": dict(frames=(2, 9, 17), cin=3, cout=64, ks=3, order="oihw"),
    "conv1_2": dict(frames=(2, 9, 17), cin=64, cout=64, ks=3, order="oihw"),
}
_STRIDE = 55  # coprime to every K here: consecutive j -> (j * 55) % K visits every k


@functools.lru_cache(maxsize=None)
def one_hot_case(name):
    """x [N,cin,H,W] and the weight sets: each a list over output channels of its terms
    [(channel, tap, weight), ...].  The single-term sets step through K with a stride coprime to
    it, so together they hit every k; for the GEMM families one more set gives every channel three
    terms, one in each third of the family's own k order (for most channels three different slabs of
    a 3-slab run)."""
    c = ONE_HOT_CASES[name]
    n, h, w = c["frames"]
    cin, cout, ks = c["cin"], c["cout"], c["ks"]
    K = cin * ks * ks
    assert np.gcd(_STRIDE, K) == 1
    rng = np.random.default_rng(_seed("one_hot_" + name))
    x = _full_mantissa(rng, (n, cin, h, w))
    sets = []
    for s in range(-(-K // cout)):
        wv = _full_mantissa(rng, cout)
        sets.append([[k_position(((s * cout + m) * _STRIDE) % K, "oihw", cin, ks) + (wv[m],)] for m in range(cout)])
    if c["order"] != "oihw":
        wv = _full_mantissa(rng, (cout, 3))
        third = K // 3
        sets.append([[k_position(j * third + (m * _STRIDE) % third, c["order"], cin, ks) + (wv[m, j],) for j in range(3)]
                     for m in range(cout)])
    return x, sets


def one_hot_weights(terms, cin, ks):
    w = np.zeros((len(terms), cin, ks, ks), np.float32)
    for m, ts in enumerate(terms):
        for ch, tap, v in ts:
            assert w[m, ch, tap // ks, tap % ks] == 0
            w[m, ch, tap // ks, tap % ks] = v
    return w


def one_hot_covered(name):
    """per k of the layer, how many of the case's weight sets hit it"""
    c = ONE_HOT_CASES[name]
    hits = np.zeros((c["cin"], c["ks"] * c["ks"]), int)
    for terms in one_hot_case(name)[1]:
        for ts in terms:
            for ch, tap, _ in ts:
                hits[ch, tap] += 1
    return hits


def one_hot_expected(x, terms, ks):
    """(expected sum of products, sum of |products|, number of terms) per output, float64 [N,M,H,W]:
    x[c, y + dy, x + dx] * w, 0 where the tap falls outside the frame."""
    n, _, h, w = x.shape
    pad = ks // 2
    xp = np.zeros((n, x.shape[1], h + 2 * pad, w + 2 * pad), np.float64)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    exp = np.zeros((n, len(terms), h, w), np.float64)
    mag = np.zeros_like(exp)
    for m, ts in enumerate(terms):
        for ch, tap, v in ts:
            dy, dx = divmod(tap, ks)
            p = xp[:, ch, dy:dy + h, dx:dx + w] * np.float64(v)
            exp[:, m] += p
            mag[:, m] += np.abs(p)
    return exp, mag, max(len(ts) for ts in terms)


def one_hot_bound(mag, nterms, rel=ONE_HOT):
    return (rel + (nterms - 1) * ONE_HOT_ADD) * mag


# ------------------------------------------------------------------------------ input digests
# sha256 (first 16 hex digits) over the case's seeded inputs: a change of a seed or of the recipe
# shows up here, not as a silently different test
INPUT_DIGESTS = {
    "win7_bench_2x23x41": "f96f28a1201adb6f",
    "win7_two_frames_3x17x19": "047f3531d8f4c7e7",
    "win7_one_tile_5x6x7": "bc8901abf997d4fc",
    "win7_19groups_2x9x13": "1c24f91fcfd1d027",
    "win7_3groups_2x11x11": "41cc3c727ca6831c",
    "win7_large_2x20x61": "0a74c01aaa66ac59",
    "win7_large_1x40x100": "bc1df6e717ffdf47",
    "win3_large_2x12x120": "6699ea830864cdb7",
    "wino3_2x23x41": "2ad04b914603078a",
    "win7_per_frame_2x46x82": "733abb730b9d9bfb",
    "win7_two_segments": "ca1015170ab11209",
    "two_segments_cout19": "0793f64d28b1f866",
    "pooled_x6_2x19x23": "99264a717452dce0",
    "chain_128_38": "c81e985faba9d29a",
    "chain_128_19_two_segments": "4408a0f98afffa93",
    "chain_512_22": "349bb470aab94a10",
    "chain_65_pixels": "4fd4f7fa8ce08aa5",
    "win7_small": "49ebfba3bcefee6f",
    "win7_large": "f7ec5dd1535f6595",
    "x6_3x3": "62aa0e7523125b77",
    "chain_first": "38814585996e168d",
    "chain_second": "01ad1b121a8c291b",
    "conv1_1": "7303015b34aa2ec6",
    "conv1_2": "95d1dc998558bf69",
    "conv1_stage1": "cd45ab1fd14881f1",
    "conv1_stage2": "5b5ce469a85542ff",
}


def case_digest(name):
    if name in DENSE:
        xs, ws, bs, _ = dense_case(name)
        return digest(*xs, *ws, *bs)
    if name in CHAIN:
        xs, wts, _ = chain_case(name)
        return digest(*xs, *[a for t in wts for a in t])
    if name in ONE_HOT_CASES:
        c = ONE_HOT_CASES[name]
        x, sets = one_hot_case(name)
        return digest(x, *[one_hot_weights(t, c["cin"], c["ks"]) for t in sets])
    xs, w, b, _ = conv1_case(int(name[-1]))
    return digest(*xs, w, b)


ALL_CASES = list(DENSE) + list(CHAIN) + list(ONE_HOT_CASES) + ["conv1_stage1", "conv1_stage2"]
