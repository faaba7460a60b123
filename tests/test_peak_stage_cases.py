"""CPU: every case of tests/peak_stage_cases.py reaches what it is named for, from the reference and
the kernels' conditions restated in Python alone -- the load mode of each tile, staged-row counts,
cold and hot tiles, exact ties, ragged tile counts, what fits -- so that a case that stops reaching
its path fails here and not silently on the GPU."""
import numpy as np
import pytest

import peak_stage_cases as pc

F32, F64 = pc.F32, pc.F64
DTYPES = [F32, F64]
IDS = {F32: "f32", F64: "f64"}.get


def _counts(key, maps, thre):
    return [len(pc.ref_peaks(key, k, thre)[0]) for k in range(len(maps))]


# --------------------------------------------------------------------------- gauss_nms_wide
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(pc.WIDE))
def test_wide_cases_have_peaks(name, dtype):
    maps, thre, cap = pc.wide_case(name, dtype)
    assert maps.dtype == dtype and maps.flags.c_contiguous
    counts = _counts(("wide", name, dtype), maps, thre)
    if pc.WIDE[name]:
        assert counts == [0] * len(maps), counts
    else:
        assert min(counts) >= 1, counts
    if dtype == F64 and not name.startswith("const_thre"):  # a narrowing cast would change the map
        finite = maps[np.isfinite(maps) & (maps != 0)]
        assert (finite != finite.astype(F32)).mean() > 0.5
        for k in range(len(maps)):
            sc = pc.ref_peaks(("wide", name, dtype), k, thre)[1]
            assert not len(sc) or (sc != sc.astype(F32)).any()  # ... and show in that map's scores


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wide_mode_maps_are_dense(dtype):
    """Tens of peaks per map at the larger sizes, and the threshold decides among the maxima."""
    maps, thre, _ = pc.wide_case("mode_73x217", dtype)
    for k in range(len(maps)):
        above = len(pc.ref_peaks(("wide", "mode_73x217", dtype), k, thre)[0])
        every = len(pc.ref_peaks(("wide", "mode_73x217", dtype), k, -1.0)[0])
        assert 20 <= above < every, (above, every)


@pytest.mark.parametrize("claim", pc.MODE_CLAIMS, ids=lambda c: "%dx%d_tile%d_%d_mode%d" % (c[0] + c[1] + (c[2],)))
def test_wide_mode_boundaries(claim):
    (H, W), (x0, y0), mode = claim
    assert ("mode_%dx%d" % (H, W)) in pc.WIDE and (x0, y0) in pc.tiles(H, W)
    assert pc.wide_mode(H, W, x0, y0) == mode
    # mode 1 promises reflect_near's range, mode 0 promises no reflection at all
    xs = np.arange(x0 - 13, x0 - 13 + pc.FOOT_W)
    ys = np.arange(y0 - 13, y0 - 13 + pc.FOOT_H)
    if mode == 0:
        assert xs[0] >= 0 and xs[-1] < W and ys[0] >= 0 and ys[-1] < H
    if mode == 1:
        assert xs[0] >= -W and xs[-1] < 2 * W and ys[0] >= -H and ys[-1] < 2 * H
    if mode == 2:
        assert xs[0] < -W or xs[-1] >= 2 * W or ys[0] < -H or ys[-1] >= 2 * H


def test_every_mode_is_reached_and_each_boundary_from_both_sides():
    seen = {pc.wide_mode(H, W, *t) for H, W in [(73, w) for w in pc.MODE_W] + [(h, 217) for h in pc.MODE_H]
            for t in pc.tiles(H, W)}
    assert seen == {0, 1, 2}
    modes = {c[0] + c[1]: c[2] for c in pc.MODE_CLAIMS}
    for (a, b, tile) in [((73, 216), (73, 217), (102, 30)), ((72, 217), (73, 217), (102, 30)),
                         ((73, 57), (73, 58), (0, 0)), ((73, 108), (73, 109), (102, 0)),
                         ((21, 217), (22, 217), (0, 0)), ((36, 217), (37, 217), (0, 30))]:
        assert modes[a + tile] == modes[b + tile] + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["tie_unit4", "tie_flat12"])
def test_tie_cases_tie_exactly_across_the_tile_corner(name, dtype):
    maps, thre, _ = pc.wide_case(name, dtype)
    idx, _, g = pc.ref_peaks(("wide", name, dtype), 0, thre)
    y, x = pc.CORNER
    four = [(y - 1, x - 1), (y - 1, x), (y, x - 1), (y, x)]
    assert {(yy // pc.WTH, xx // pc.WTW) for yy, xx in four} == {(0, 0), (0, 1), (1, 0), (1, 1)}  # four tiles
    vals = pc.bits(np.array([g[p] for p in four]))
    assert (vals == vals[0]).all() and g[four[0]] > thre
    assert sorted(idx) == sorted(yy * 217 + xx for yy, xx in four)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_maps(dtype):
    for shape, n in (("37x109", 4033), ("5x3", 15)):
        counts = {}
        for level in ("thre", "next", "0.3"):
            name = "const_%s_%s" % (level, shape)
            maps, thre, cap = pc.wide_case(name, dtype)
            assert thre == pc.CONST_THRE and float(maps[0, 0, 0]) >= thre
            counts[level] = len(pc.ref_peaks(("wide", name, dtype), 0, thre)[0])
            assert counts[level] in (0, n)  # one value everywhere: all pixels or none
        assert counts["0.3"] == n and counts["next"] == n and counts["thre"] == 0
    assert pc.wide_case("const_0.3_37x109", dtype)[2] == 64 < 4033  # the list overflows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_threshold_at_equality(dtype):
    p, v = pc._pick_threshold(dtype)
    _, t_eq, _ = pc.wide_case("thre_equal", dtype)
    _, t_lo, _ = pc.wide_case("thre_just_below", dtype)
    assert t_eq == v and t_lo < t_eq and np.nextafter(t_lo, np.inf) == t_eq
    eq = pc.ref_peaks(("wide", "thre_equal", dtype), 0, t_eq)[0]
    lo = pc.ref_peaks(("wide", "thre_just_below", dtype), 0, t_lo)[0]
    assert p not in eq and p in lo and len(lo) == len(eq) + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nonpositive_thresholds_see_negative_values(dtype):
    for name in ("thre_zero", "thre_minus1"):
        maps, thre, _ = pc.wide_case(name, dtype)
        assert thre <= 0 and pc.skip_below(thre) == -np.inf and (maps < 0).any()
    g = pc.ref_peaks(("wide", "thre_minus1", dtype), 0, -1.0)[2]
    idx = pc.ref_peaks(("wide", "thre_minus1", dtype), 0, -1.0)[0]
    assert (g.ravel()[idx] < 0).any()  # peaks below zero: kept at -1, gone at 0
    assert len(pc.ref_peaks(("wide", "thre_zero", dtype), 0, 0.0)[0]) < len(idx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cold_tiles_beside_a_hot_one(dtype):
    maps, thre, _ = pc.wide_case("cold_beside_hot_61x307", dtype)
    assert len(pc.tiles(61, 307)) == 12
    assert pc.hot_tiles(maps[0], thre) == [(102, 0)]
    idx = pc.ref_peaks(("wide", "cold_beside_hot_61x307", dtype), 0, thre)[0]
    assert len(idx) >= 1 and all(i // 307 < 30 and 102 <= i % 307 < 204 for i in idx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_cases(dtype):
    hot, thre, _ = pc.wide_case("nan_hot", dtype)
    clean = pc.wide_case("mode_73x217", dtype)[0]
    assert np.isnan(hot).sum() == 2 and np.isnan(hot[0]).sum() == 1
    for k in range(2):
        with_nan = pc.ref_peaks(("wide", "nan_hot", dtype), k, thre)[0]
        without = pc.ref_peaks(("wide", "mode_73x217", dtype), k, thre)[0]
        assert 1 <= len(with_nan) < len(without) and set(with_nan) < set(without)  # a NaN only removes peaks
    cold, thre, _ = pc.wide_case("nan_cold", dtype)
    assert np.isnan(cold).sum() == 1 and pc.hot_tiles(cold[0], thre) == []
    assert not np.isnan(clean).any()


@pytest.mark.parametrize("name", ["ragged_3x61x205", "ragged_5x29x97"])
def test_ragged_tile_counts(name):
    maps, thre, _ = pc.wide_case(name, F32)
    NP, H, W = maps.shape
    total = len(pc.tiles(H, W)) * NP
    assert total == {"ragged_3x61x205": 27, "ragged_5x29x97": 5}[name] and total % 8
    ids = sorted(pc.xcd_contiguous_id(total, b) for b in range(total))
    assert ids == list(range(total))  # the decode is a permutation ...
    assert sorted(xcd * (total >> 3) + (b >> 3) for b in range(total) for xcd in [b & 7]) != ids  # ... through min(xcd, rr)
    for dtype in DTYPES:
        maps = pc.wide_case(name, dtype)[0]
        sets = [tuple(pc.ref_peaks(("wide", name, dtype), k, thre)[0]) for k in range(NP)]
        assert len(set(sets)) == NP  # every map differs: a misplaced tile shows


# -------------------------------------------------------------------------- gauss_nms_resize
@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_resize_cases(name):
    N, Cm, coff, P, Hs, Ws, H, W, thre, cap, fits = pc.RESIZE[name]
    assert pc.resize_fits(Hs, Ws, H, W) == fits
    assert pc.resize_mid(name).shape == (N, Cm, Hs, Ws) and coff + P <= Cm
    if not fits:
        return
    rows = [pc.staged_rows(Hs, H, y0) for y0 in range(0, H, pc.WTH)]
    assert max(rows) <= pc.GR_MAXR, rows
    counts = _counts(("resize", name), pc.resize_maps(name), thre)
    assert min(counts) >= 1, counts
    if cap is not None:
        assert min(counts) > cap


def test_resize_cold_bound_case():
    """Every source at or below 0.085 < thre, yet the reference has peaks above it: the cubic
    overshoot survives the smoothing, and only the factor 1.9 keeps the tiles."""
    mid = pc.resize_mid("cold_bound")
    assert float(np.abs(mid).max()) == float(F32(pc.COLD_PATCH)) < pc.THRE < 1.9 * pc.COLD_PATCH
    idx, sc, g = pc.ref_peaks(("resize", "cold_bound"), 0, pc.THRE)
    assert [(i // 320, i % 320) for i in idx] == [(77, 97), (77, 182), (142, 97), (142, 182)]
    assert pc.resize_maps("cold_bound").max() > 0.104 and (g.ravel()[idx] > 0.1019).all()
    cold = pc.resize_cold_tiles(mid[0, 0], 240, 320, pc.THRE)
    assert 0 < len(cold) < len(pc.tiles(240, 320))
    peak_tiles = {(i % 320 // pc.WTW * pc.WTW, i // 320 // pc.WTH * pc.WTH) for i in idx}
    assert not peak_tiles & set(cold)
    # the negated patch: only the lone positive pixel makes peaks, the patch's tiles stay hot
    neg = pc.resize_mid("cold_bound_negated")
    assert float(neg.min()) == -float(F32(pc.COLD_PATCH))
    idx = pc.ref_peaks(("resize", "cold_bound_negated"), 0, pc.THRE)[0]
    assert len(idx) >= 1 and all(i // 320 > 180 and i % 320 > 260 for i in idx)


@pytest.mark.parametrize("name,y0", [("max_step_68_to_110", 30), ("max_step_102_to_165", 30)])
def test_resize_largest_step_stages_nearly_every_row(name, y0):
    _, _, _, _, Hs, _, H, _, _, _, _ = pc.RESIZE[name]
    assert pc.source_step(H, Hs) == pc.source_step(110, 68)
    assert 38 <= pc.staged_rows(Hs, H, y0) <= pc.GR_MAXR
    assert not pc.resize_fits(Hs, 50, H - 1, 130)


@pytest.mark.parametrize("name", ["wrap_34_to_55", "wrap_12_to_40"])
def test_resize_wrap_cases_wrap(name):
    H = pc.RESIZE[name][6]
    assert H < pc.FOOT_H


def test_resize_plane_case_is_ragged_and_distinct():
    N, Cm, coff, P, Hs, Ws, H, W, thre, _, _ = pc.RESIZE["planes_2x5_off1_3"]
    assert (len(pc.tiles(H, W)) * N * P) % 8
    mid = pc.resize_mid("planes_2x5_off1_3")
    flat = mid.reshape(N * Cm, -1)
    assert len({p.tobytes() for p in flat}) == N * Cm
    sets = [tuple(pc.ref_peaks(("resize", "planes_2x5_off1_3"), k, thre)[0]) for k in range(N * P)]
    assert len(set(sets)) == N * P


# -------------------------------------------------------------------------- heat_full_scales
@pytest.mark.parametrize("name", list(pc.HEAT))
def test_heat_cases(name):
    sizes, N, Cm, coff, C, H, W, kind = pc.HEAT[name]
    assert pc.heat_fits(sizes, H, W) == (name not in pc.HEAT_REFUSED)
    assert coff + C <= Cm and len(sizes) <= 16
    ref = pc.heat_reference(name)
    assert ref.shape == (N * C, H, W)
    if kind == "negzero":  # 0.0 + -0.0: the average of a map of -0.0f is +0.0
        assert not pc.bits(ref).any()
    else:
        assert np.isfinite(ref).all() and ref.std() > 0.01


def test_heat_cases_cover_the_named_paths():
    assert [len(pc.HEAT["ns%d_40x40" % n][0]) for n in (1, 2, 3, 5, 8, 9)] == [1, 2, 3, 5, 8, 9]
    for name, pos in (("identity_first", 0), ("identity_middle", 1), ("identity_last", 2)):
        sizes, _, _, _, _, H, W, _ = pc.HEAT[name]
        assert [s == (H, W) for s in sizes] == [i == pos for i in range(3)]
    assert any(hs == 40 and ws != 40 for hs, ws in pc.HEAT["ns5_40x40"][0])  # an identity's rows, not its columns
    assert [pc.source_step(200, hs) for hs, _ in pc.HEAT["steps_0.185_0.58_1.6"][0]] == pytest.approx([0.185, 0.58, 1.6], rel=1e-15)
    assert pc.source_step(16, 39) == pc.source_step(32, 78) == 2.4375 and pc.heat_rows_fit(2.4375)
    assert pc.source_step(32, 79) == 2.46875 and not pc.heat_rows_fit(2.46875)
    # a division by the number of scales that float32 and float64 round differently
    for name in ("ns3_40x40", "ns5_40x40"):
        sizes = pc.HEAT[name][0]
        m = pc.heat_mids(name)[1][0, 0]  # the identity scale
        ns = len(sizes)
        assert ((m / F32(ns)).astype(F64) != m.astype(F64) / ns).any()


# ------------------------------------------------------------------------------ hand threshold
@pytest.mark.parametrize("name", list(pc.HAND))
def test_hand_cases(name):
    H, W, thre = pc.HAND[name]
    m = pc.hand_map(name)[0]
    expect, first, sums = pc.hand_reference(name)[0]
    hot = pc.hot_tiles(m, thre, pc.HTW, pc.HTH)
    if name.startswith("one_hot_tile"):
        assert hot == [(0, 0)] and len(pc.tiles(H, W, pc.HTW, pc.HTH)) == 16
        assert len(first) >= 2 and (expect[:pc.HTH, :pc.HTW] >= 0).any()
        assert (expect[pc.HTH:] == -1).all() and (expect[:, pc.HTW:] == -1).all()
    else:
        assert len(hot) == len(pc.tiles(H, W, pc.HTW, pc.HTH)) > 1
        assert list(first) == [0] and (expect == 0).all()  # one component over every tile, named by pixel 0
