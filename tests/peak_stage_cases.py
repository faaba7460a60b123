"""Case tables of the exact mode's peak and heat-average stage tests (tests/test_gpu_peak_stages.py
on the GPU, tests/test_peak_stage_cases.py for the inputs and what they reach alone):
gauss_nms_wide<float / double>, gauss_nms_resize and heat_full_scales / heat_full, each through its
debug hook (opose_debug_gauss_nms, opose_debug_gauss_nms_resize, opose_debug_heat_scales), and the
hand threshold gauss_threshold through opose_debug_hand_label.

The reference is plain NumPy / SciPy in float64: scipy.ndimage.gaussian_filter(map, sigma=3), the
four `>=` comparisons against neighbours that are zero outside the map, then `> thre`
(oracle/body_post.py find_peaks); oracle.cv_resize.resize_cubic for the resize; and
0.0 + float64(float32(resized) / float32(ns)) added in scale order for the average.  The kernels
evaluate the same expressions in the same order, so every comparison is equality: counts, sorted
peak lists, scores and averages as bit patterns.

The second half of the file restates in Python the conditions by which the kernels pick a path (load
mode of a tile, staged rows, cold tiles, fits, the XCD-ordered tile decode), so that the CPU test
can assert that every case reaches what it is named for.
"""
import functools
import math

import numpy as np
from scipy.ndimage import gaussian_filter, label

from oracle.cv_resize import resize_cubic

F32, F64 = np.float32, np.float64
THRE = 0.1                       # src/body.py thre1
WTW, WTH = 102, 30               # gauss_nms_wide / gauss_nms_resize: outputs per tile
HALO = 13                        # 12 filter taps + the NMS ring
FOOT_W, FOOT_H = WTW + 2 * HALO, WTH + 2 * HALO  # 128 x 56 footprint
GR_MAXR = 40                     # gauss_nms_resize: staged source rows
RS_RT, RS_MAXR, HEAT_SCALES = 16, 44, 8  # heat_full_scales: rows per workgroup, staged rows, scales
HTW, HTH = 64, 32                # gauss_threshold: tile
OPOSE_E_ARG = -1


# ------------------------------------------------------------------------------ reference
def smooth(m):
    with np.errstate(invalid="ignore"):
        return gaussian_filter(np.asarray(m, F64), sigma=3)


def peak_mask(g, thre):
    """oracle/body_post.py find_peaks on a smoothed map (NaN: every comparison false)."""
    nb = np.zeros((4,) + g.shape)
    nb[0, 1:, :] = g[:-1, :]
    nb[1, :-1, :] = g[1:, :]
    nb[2, :, 1:] = g[:, :-1]
    nb[3, :, :-1] = g[:, 1:]
    with np.errstate(invalid="ignore"):
        return (g >= nb[0]) & (g >= nb[1]) & (g >= nb[2]) & (g >= nb[3]) & (g > thre)


@functools.lru_cache(maxsize=None)
def _ref_cached(key, k, thre):
    m = np.asarray(_MAPS[key]()[k], F64)
    g = smooth(m)
    idx = np.flatnonzero(peak_mask(g, thre))
    for a in (g, idx):
        a.setflags(write=False)
    return idx, m.ravel()[idx], g


_MAPS = {}


def ref_peaks(key, k, thre):
    """(row-major peak indices, the float64 map at them, the smoothed map) of map k of the case
    `key` (a name registered in _MAPS), computed once."""
    return _ref_cached(key, k, float(thre))


def bits(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


# --------------------------------------------------------------------------- gauss_nms_wide
def _noise(seed, shape, dtype, scale=0.2, offset=0.0):
    """Dense uniform noise of mean offset + scale / 2.  float64: thirds of random float32 values,
    which no float32 holds, so a narrowing cast of the map shows in the scores."""
    base = np.random.default_rng(seed).random(shape, dtype=F32)
    if dtype == F32:
        return base * F32(scale) + F32(offset)
    return base.astype(F64) / 3.0 * (3.0 * scale) + offset


MODE_W = [12, 13, 57, 58, 108, 109, 216, 217]  # at H = 73
MODE_H = [12, 13, 21, 22, 36, 37, 72]          # at W = 217 (73 x 217 is in MODE_W)
# ((H, W), tile (x0, y0), its load mode): each inequality of gauss_nms_wide from both sides
MODE_CLAIMS = [((73, 216), (102, 30), 1), ((73, 217), (102, 30), 0), ((72, 217), (102, 30), 1),
               ((73, 57), (0, 0), 2), ((73, 58), (0, 0), 1), ((73, 108), (102, 0), 2), ((73, 109), (102, 0), 1),
               ((21, 217), (0, 0), 2), ((22, 217), (0, 0), 1), ((36, 217), (0, 30), 2), ((37, 217), (0, 30), 1),
               ((73, 12), (0, 0), 2), ((73, 13), (0, 0), 2), ((12, 217), (0, 0), 2), ((13, 217), (0, 0), 2)]
CORNER = (30, 102)  # the pixel whose upper-left corner four tiles share

# name -> (empty: the reference has no peak, on purpose)
WIDE = {}
for _w in MODE_W:
    WIDE["mode_73x%d" % _w] = False
for _h in MODE_H:
    WIDE["mode_%dx217" % _h] = False
WIDE.update({
    "tie_unit4": False, "tie_flat12": False,
    "const_thre_37x109": True, "const_next_37x109": False, "const_0.3_37x109": False,
    "const_thre_5x3": True, "const_next_5x3": False, "const_0.3_5x3": False,
    "thre_equal": False, "thre_just_below": False, "thre_zero": False, "thre_minus1": False,
    "cold_beside_hot_61x307": False, "nan_hot": False, "nan_cold": True,
    "ragged_3x61x205": False, "ragged_5x29x97": False})
CONST_THRE = float(F32(0.1))  # a threshold both map types hold exactly


def _pick_threshold(dtype):
    """The smoothed value at the median-height peak (of those above 0.1) of the dense 73 x 217 map."""
    key = ("wide", "mode_73x217", dtype)
    idx, _, g = ref_peaks(key, 0, THRE)
    p = idx[np.argsort(g.ravel()[idx])[len(idx) // 2]]
    return int(p), float(g.ravel()[p])


@functools.lru_cache(maxsize=None)
def wide_case(name, dtype):
    """(maps [NP, H, W] of dtype, thre, cap) of a gauss_nms_wide case."""
    cap = None
    thre = THRE
    if name.startswith("mode_"):
        H, W = (int(v) for v in name[5:].split("x"))
        maps = _noise(H * 1000 + W, (2, H, W), dtype)
    elif name.startswith("tie_"):
        v = F32(1.0) if dtype == F32 else 1.0 / 3.0
        maps = np.zeros((1, 73, 217), dtype)
        y, x = CORNER
        if name == "tie_unit4":
            maps[0, y - 1:y + 1, x - 1:x + 1] = v
            thre = 0.05 * float(v)
        else:
            maps[0, y - 6:y + 6, x - 6:x + 6] = v
            thre = 0.1 * float(v)
    elif name.startswith("const_"):
        _, level, shape = name.split("_")
        H, W = (int(v) for v in shape.split("x"))
        thre = CONST_THRE
        c = {"thre": dtype(thre), "next": np.nextafter(dtype(thre), dtype(1)), "0.3": dtype(0.3)}[level]
        maps = np.full((1, H, W), c, dtype)
        cap = 64 if H * W > 64 else H * W
    elif name in ("thre_equal", "thre_just_below"):
        maps = wide_case("mode_73x217", dtype)[0]
        thre = _pick_threshold(dtype)[1]
        if name == "thre_just_below":
            thre = float(np.nextafter(thre, -np.inf))
    elif name in ("thre_zero", "thre_minus1"):
        maps = _noise(77, (2, 37, 109), dtype, 0.2, -0.105)  # smoothed maxima on both sides of zero
        thre = 0.0 if name == "thre_zero" else -1.0
    elif name == "cold_beside_hot_61x307":
        maps = _noise(61307, (1, 61, 307), dtype, 0.02)
        maps[0, 4:7, 152:155] = 0.9  # rows that only the first tile row's footprints reach
    elif name == "nan_hot":
        maps = wide_case("mode_73x217", dtype)[0].copy()
        for k in range(2):  # on a peak of the clean map: the middle one of its list, then the last
            idx = ref_peaks(("wide", "mode_73x217", dtype), k, THRE)[0]
            maps[k].ravel()[idx[-1] if k else idx[len(idx) // 2]] = np.nan
    elif name == "nan_cold":
        maps = _noise(5, (1, 73, 217), dtype, 0.02)
        maps[0, 31, 100] = np.nan
    elif name == "ragged_3x61x205":
        maps = _noise(3, (3, 61, 205), dtype)
    elif name == "ragged_5x29x97":
        maps = _noise(4, (5, 29, 97), dtype)
    else:
        raise KeyError(name)
    maps = np.ascontiguousarray(maps, dtype)
    maps.setflags(write=False)
    return maps, float(thre), int(cap or maps.shape[1] * maps.shape[2])


for _name in WIDE:
    for _dt in (F32, F64):
        _MAPS[("wide", _name, _dt)] = functools.partial(lambda n, d: wide_case(n, d)[0], _name, _dt)


# -------------------------------------------------------------------------- gauss_nms_resize
# name -> (N, Cm, coff, P, Hs, Ws, H, W, thre, cap (None: H * W), fits)
RESIZE = {
    "cold_bound": (1, 1, 0, 1, 12, 16, 240, 320, THRE, None, True),
    "cold_bound_negated": (1, 1, 0, 1, 12, 16, 240, 320, THRE, None, True),
    "max_step_68_to_110": (1, 2, 0, 2, 68, 50, 110, 130, THRE, None, True),
    "max_step_102_to_165": (1, 1, 0, 1, 102, 60, 165, 103, THRE, None, True),
    "too_steep_68_to_109": (1, 1, 0, 1, 68, 50, 109, 130, THRE, None, False),
    "wrap_34_to_55": (1, 2, 0, 2, 34, 20, 55, 50, THRE, None, True),
    "wrap_12_to_40": (1, 2, 0, 2, 12, 9, 40, 47, THRE, None, True),
    "cropped_181x323_to_331x587": (1, 1, 0, 1, 181, 323, 331, 587, THRE, None, True),
    "planes_2x5_off1_3": (2, 5, 1, 3, 10, 14, 61, 205, THRE, None, True),
    "cap_below_count": (1, 2, 0, 2, 68, 50, 110, 130, THRE, 3, True),
    "workload_184x328_to_368x656": (1, 2, 0, 2, 184, 328, 368, 656, THRE, None, True),
}
COLD_PATCH = 0.085  # 1.9 x this passes the threshold; it alone does not


@functools.lru_cache(maxsize=None)
def resize_mid(name):
    """mid float32 [N, Cm, Hs, Ws] of a gauss_nms_resize case."""
    N, Cm, coff, P, Hs, Ws, H, W, _, _, _ = RESIZE[name]
    if name.startswith("cold_bound"):
        mid = np.zeros((N, Cm, Hs, Ws), F32)
        mid[0, 0, 3:8, 4:10] = F32(COLD_PATCH)
        if name == "cold_bound_negated":
            mid = -mid
            mid[0, 0, 10, 14] = F32(0.3)
    elif name.startswith("cropped") or name.startswith("workload"):  # sparse blobs, as a network's maps
        rng = np.random.default_rng(Hs * 7 + Ws)
        low = np.zeros((N * Cm, (Hs + 7) // 8 + 1, (Ws + 7) // 8 + 1), F32)
        for k in range(N * Cm):
            ys, xs = rng.integers(0, low.shape[1], 12), rng.integers(0, low.shape[2], 12)
            low[k, ys, xs] = rng.random(12, dtype=F32) * F32(0.85) + F32(0.05)
        mid = np.stack([resize_cubic(p, (8 * p.shape[1], 8 * p.shape[0]))[:Hs, :Ws] for p in low])
        mid = mid.reshape(N, Cm, Hs, Ws)
    else:
        seed = sum(ord(c) for c in name.replace("cap_below_count", "max_step_68_to_110"))
        mid = _noise(seed, (N, Cm, Hs, Ws), F32)
    mid = np.ascontiguousarray(mid, F32)
    mid.setflags(write=False)
    return mid


@functools.lru_cache(maxsize=None)
def resize_maps(name):
    """The float64 maps [N * P, H, W] the fused kernel's window holds: 0.0 + the float32 resize."""
    N, Cm, coff, P, Hs, Ws, H, W, _, _, _ = RESIZE[name]
    mid = resize_mid(name)
    out = np.stack([0.0 + resize_cubic(mid[n, coff + p], (W, H)).astype(F64) for n in range(N) for p in range(P)])
    out.setflags(write=False)
    return out


for _name in RESIZE:
    _MAPS[("resize", _name)] = functools.partial(resize_maps, _name)


# -------------------------------------------------------------------------- heat_full_scales
# name -> (sizes [(Hs, Ws)] per scale, N, Cm, coff, C, H, W, kind); kind "noise" or "negzero".
# (H, W) itself is an identity scale; (H, W + 13) has the rows of one and is none.
def _pool(H, W):
    return [(max(2, round(H * 0.58)), max(2, round(W * 0.7))), (H, W), (round(H * 1.6), round(W * 1.3)),
            (max(2, round(H * 0.185)), max(2, round(W * 0.3))), (H, W + 13), (H + 5, W), (2 * H, 2 * W),
            (max(2, H // 3), W), (H, W)]


HEAT = {}
for _ns in (1, 2, 3, 5, 8, 9):
    HEAT["ns%d_40x40" % _ns] = (_pool(40, 40)[:_ns], 1, 2, 0, 2, 40, 40, "noise")
_a, _b = (23, 31), (64, 52)
HEAT["identity_first"] = ([(40, 40), _a, _b], 1, 2, 0, 2, 40, 40, "noise")
HEAT["identity_middle"] = ([_a, (40, 40), _b], 1, 2, 0, 2, 40, 40, "noise")
HEAT["identity_last"] = ([_a, _b, (40, 40)], 1, 2, 0, 2, 40, 40, "noise")
for _h in (7, 16, 17, 40):
    for _w in (257, 40):
        HEAT["rows_%dx%d" % (_h, _w)] = ([(max(2, round(_h * 0.58)), round(_w * 0.7)), (_h, _w), (_h + 3, _w // 2)],
                                         1, 1, 0, 1, _h, _w, "noise")
HEAT["steps_0.185_0.58_1.6"] = ([(37, 17), (116, 23), (320, 64)], 1, 1, 0, 1, 200, 40, "noise")
HEAT["step_2.4375_39_to_16"] = ([(39, 30), (16, 40), (9, 21)], 1, 2, 0, 2, 16, 40, "noise")
HEAT["step_2.4375_78_to_32"] = ([(78, 30), (32, 40), (19, 21)], 1, 2, 0, 2, 32, 40, "noise")
HEAT["step_2.46875_79_to_32"] = ([(79, 30), (32, 40), (19, 21)], 1, 2, 0, 2, 32, 40, "noise")
HEAT["negzero_ns1"] = ([(23, 31)], 1, 1, 0, 1, 40, 40, "negzero")
HEAT["negzero_ns3"] = ([(23, 31), (40, 40), (64, 52)], 1, 1, 0, 1, 40, 40, "negzero")
HEAT["planes_2x5_off1_3"] = ([(23, 31), (40, 40), (64, 52)], 2, 5, 1, 3, 40, 40, "noise")
# cases the one-launch form refuses (the per-scale form takes every case)
HEAT_REFUSED = {"ns9_40x40", "step_2.46875_79_to_32"}


@functools.lru_cache(maxsize=None)
def heat_mids(name):
    sizes, N, Cm, _, _, _, _, kind = HEAT[name]
    rng = np.random.default_rng(sum(ord(c) for c in name))
    out = []
    for (hs, ws) in sizes:
        m = np.full((N, Cm, hs, ws), F32(-0.0)) if kind == "negzero" else \
            (rng.standard_normal((N, Cm, hs, ws)) * 0.3).astype(F32)
        m.setflags(write=False)
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def heat_reference(name):
    """avg float64 [N * C, H, W]: src/body.py:51-67."""
    sizes, N, Cm, coff, C, H, W, _ = HEAT[name]
    ns = F32(len(sizes))
    avg = np.zeros((N * C, H, W), F64)
    for m in heat_mids(name):
        for n in range(N):
            for c in range(C):
                r = resize_cubic(np.ascontiguousarray(m[n, coff + c]), (W, H))
                avg[n * C + c] = avg[n * C + c] + (r / ns).astype(F32).astype(F64)
    avg.setflags(write=False)
    return avg


# ------------------------------------------------------------------------------ hand threshold
# name -> (H, W, thre)
HAND = {"one_hot_tile_100x200": (100, 200, 0.05), "thre_minus1_33x130": (33, 130, -1.0),
        "const_next_70x100": (70, 100, 0.05), "const_above_70x100": (70, 100, 0.05)}


@functools.lru_cache(maxsize=None)
def hand_map(name):
    H, W, thre = HAND[name]
    if name.startswith("one_hot_tile"):
        m = np.zeros((1, H, W), F64)
        m[0, 2:7, 3:12] = 0.5
        m[0, 9:16, 20:24] = 0.4 / 3
        m[0, 4:6, 30:46] = 0.7
        m[0, 12:15, 8:10] = 1.0 / 3
    elif name.startswith("thre_minus1"):
        m = np.random.default_rng(33130).random((1, H, W)) / 3.0
    elif name.startswith("const_next"):
        m = np.full((1, H, W), np.nextafter(thre, 1.0))
    else:
        m = np.full((1, H, W), thre * (1 + 1e-9))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def hand_reference(name):
    """Per map: (labels int32 [H, W]: -1 or the component's first pixel in raster order, the first
    pixels, the components' sums), as tests/test_gpu_hand.py test_hand_labels_match_scipy."""
    H, W, thre = HAND[name]
    out = []
    for m in hand_map(name):
        binary = gaussian_filter(m, sigma=3) > thre
        lab, n = label(binary, structure=np.ones((3, 3), int))
        flat = lab.ravel()
        first = np.zeros(n + 1, np.int64)
        idx = np.flatnonzero(flat)
        first[1:] = np.full(n, flat.size)
        np.minimum.at(first, flat[idx], idx)
        expect = np.where(flat > 0, first[flat], -1).reshape(H, W).astype(np.int32)
        sums = np.bincount(flat, weights=m.ravel(), minlength=n + 1)[1:]
        out.append((expect, first[1:], sums))
    return out


# ------------------------------------------------------- the kernels' conditions, restated
def reflect_idx(i, n):
    i = np.asarray(i) % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def tiles(H, W, tw=WTW, th=WTH):
    return [(x0, y0) for y0 in range(0, H, th) for x0 in range(0, W, tw)]


def wide_mode(H, W, x0, y0):
    """gauss_nms_wide's choice of gauss_wide_load<MODE>."""
    if x0 >= 13 and x0 + WTW + 13 <= W and y0 >= 13 and y0 + WTH + 13 <= H:
        return 0
    if x0 - 13 >= -W and x0 + WTW + 13 <= 2 * W and y0 - 13 >= -H and y0 + WTH + 13 <= 2 * H:
        return 1
    return 2


def footprint(m, x0, y0, tw=WTW, th=WTH):
    """The reflected inputs a tile's vertical pass loads."""
    H, W = m.shape
    ys = reflect_idx(np.arange(y0 - HALO, y0 - HALO + th + 2 * HALO), H)
    xs = reflect_idx(np.arange(x0 - HALO, x0 - HALO + tw + 2 * HALO), W)
    return m[np.ix_(ys, xs)]


def skip_below(thre):
    return thre * (1.0 - 1e-9) if thre > 0.0 else -math.inf


def hot_tiles(m, thre, tw=WTW, th=WTH):
    """Tiles gauss_wide_tail / gauss_tile do not drop (a NaN counts as below)."""
    with np.errstate(invalid="ignore"):
        return [t for t in tiles(*m.shape, tw, th) if (footprint(np.asarray(m, F64), *t, tw, th) >= skip_below(thre)).any()]


def source_step(dst, src):
    return 1.0 / (float(dst) / src)  # geom_from_pads


def cubic_rows(d, step, ssize):
    """(first, last) clamped tap row of destination rows d (cubic_tap)."""
    f = ((np.asarray(d, F64) + 0.5) * step - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    return np.clip(s - 1, 0, ssize - 1), np.clip(s + 2, 0, ssize - 1)


def staged_rows(Hs, H, y0):
    """hi - lo + 1 of gauss_nms_resize's tile at y0."""
    lo, hi = cubic_rows(reflect_idx(np.arange(y0 - HALO, y0 - HALO + FOOT_H), H), source_step(H, Hs), Hs)
    return int(hi.max() - lo.min() + 1)


def resize_fits(Hs, Ws, H, W):
    return not (Hs == H and Ws == W) and 55.0 * source_step(H, Hs) + 6.0 <= float(GR_MAXR)


def resize_cold_tiles(mid_plane, H, W, thre):
    """Tiles gauss_nms_resize drops on the bound of their sources: 1.9 max|q| < skip_below."""
    Hs, Ws = mid_plane.shape
    out = []
    for (x0, y0) in tiles(H, W):
        lo, hi = cubic_rows(reflect_idx(np.arange(y0 - HALO, y0 - HALO + FOOT_H), H), source_step(H, Hs), Hs)
        cl, ch = cubic_rows(reflect_idx(np.arange(x0 - HALO, x0 - HALO + FOOT_W), W), source_step(W, Ws), Ws)
        cols = np.unique(np.concatenate([np.arange(a, b + 1) for a, b in zip(cl, ch)]))
        q = np.abs(mid_plane[lo.min():hi.max() + 1][:, cols])
        mx = F32(np.fmax.reduce(q, axis=None, initial=F32(0)))  # fmaxf: a NaN is skipped
        if not 1.9 * float(mx) >= skip_below(thre):
            out.append((x0, y0))
    return out


def heat_rows_fit(step):
    return RS_RT * step + 5.0 <= float(RS_MAXR)


def heat_fits(sizes, H, W):
    return all((hs == H and ws == W) or heat_rows_fit(source_step(H, hs)) for hs, ws in sizes) and \
        1 <= len(sizes) <= HEAT_SCALES


def xcd_contiguous_id(total, b):
    q, rr, xcd = total >> 3, total & 7, b & 7
    return xcd * q + min(xcd, rr) + (b >> 3)
