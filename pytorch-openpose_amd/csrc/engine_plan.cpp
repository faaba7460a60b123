// engine_plan.cpp — conv launch planning of libopose: tile shape, grid, k slabs, kernel family.
#include "engine.h"

namespace opose {

// --------------------------------------------------------------- conv launch planning
// choose_tile: the fp32 MFMA path (OPOSE_CONV=f32, conv.hip stream-K) and the whole-tile choice of
// the split-bf16 debug entry points; the split-bf16 network plans with slab_count / pick_tile
//
// Cost model in units of one 32-deep k-chunk of a 64x64 output tile on one CU.  A CU that
// holds k >= 2 co-resident workgroups finishes them in k * work; a lone workgroup (one wave per
// SIMD) runs at ~60 %.  Stream-K (grid = all resident slots) balances the chip exactly and
// pays for the partial slabs of tiles it splits plus one fixup launch.
TileChoice choose_tile(int Mpad, const std::vector<int>& gpix, int nK, bool x6, bool dp_only, double* cost_out) {
    long npix_all = 0;
    for (int n : gpix) npix_all += n;
    static const int cfg[6][3] = {{128, 128, 2}, {128, 256, 1}, {256, 128, 1},
                                  {128, 64, 3},  {64, 128, 3},  {64, 64, 4}};  // mt, pt, WG/CU
    // split-bf16 kernel: 2.5x the MFMA rate per chunk, more LDS per workgroup
    static const int occ6[6] = {1, 1, 1, 2, 2, 3};
    // (256x128 measured 0-2.5 % faster than 128x256 where both fit: half the im2col DMA per MFMA;
    // a 64x256 tile (four 64x64 waves) for the M = 64 layers measured 91 vs 109 TF/s with 64x128
    // on conv1_2 -- an M = 64 tile loads the same im2col bytes per MFMA whatever its width -- and
    // was deleted)
    static const double ovh6_big[6] = {1.5, 1.0, 0.96, 1.1, 1.1, 1.2};
    // layers of one or two small frames (C2 / C3 / single-frame C5, stream-K over the whole chip):
    // 128x128 priced like the 8-wave tiles and 64x64 higher -- measured, C2 1.91 -> 1.72 ms and
    // Hand() 10.0 -> 9.9 ms, C5 and the bench unchanged; the same weights on the bench's
    // 32-frame layers cost 6 % (a round-4 A/B, kept in git history)
    static const double ovh6_small[6] = {1.0, 1.0, 0.96, 1.1, 1.1, 1.6};
    const double* ovh6 = npix_all <= 16384 ? ovh6_small : ovh6_big;
    const double rate = x6 ? 0.4 : 1.0;
    // relative cost per MFMA of the smaller tiles of the fp32 kernel (more load/issue work per
    // MFMA), measured with scripts/conv_timing.py
    static const double ovh[6] = {1.0, 0.95, 0.93, 1.02, 1.02, 1.06};
    TileChoice best{64, 64, 1};
    double best_cost = 1e300;
    for (int c = 0; c < 6; ++c) {
        const int mt = cfg[c][0], pt = cfg[c][1], occ = x6 ? occ6[c] : cfg[c][2];
        if (Mpad % mt) continue;
        long tiles = 0;
        for (int n : gpix) tiles += (long)(Mpad / mt) * ((n + pt - 1) / pt);
        const double unit = (mt / 64.0) * (pt / 64.0) * (x6 ? ovh6[c] : ovh[c]) * rate;
        // data parallel
        const long per_cu = (tiles + 255) / 256;
        // one resident workgroup of a 2-per-CU config runs at ~60 % (floor 1.6); the 8-wave
        // 128x256 config fills the CU on its own
        const double floor1 = occ >= 2 ? 1.6 : 1.0;
        const double dp = std::max<double>(per_cu, floor1) * nK * unit;
        if (dp < best_cost * 0.97) {
            best_cost = dp;
            best = {mt, pt, (int)tiles};
        }
        // stream-K over every resident slot (each workgroup >= 4 chunks)
        const long iters = tiles * nK;
        long grid = std::min<long>(256L * occ, iters / 4);
        if (!dp_only && grid >= 1 && grid != tiles) {
            const double per_wg = (double)iters / grid;
            const double cu_load = std::max(floor1, std::ceil(grid / 256.0)) * per_wg * unit;
            // partial slabs: every workgroup segment that is not a whole tile writes one, the
            // fixup re-reads them all (grid > tiles: ~grid + tiles segments, each tile cut in
            // grid / tiles parts -- the dominant cost of tiny single-frame layers)
            // (measured: with grid <= 2 x tiles the slabs stay cache resident and the old
            // tiles-with-partials estimate ranks configurations better)
            const long segs = grid > 2 * tiles ? grid + tiles : std::min<long>(tiles, 2 * grid);
            const double slab_bytes = grid > 2 * tiles
                                          ? (double)segs * mt * pt * 4.0 * 2.0 + (double)tiles * mt * pt * 4.0
                                          : (double)segs * mt * pt * 4.0 * 3.0;
            const double sk = cu_load + slab_bytes / 5e12 / 0.42e-6 + 8.0;      // + fixup launch
            if (sk < best_cost * 0.97) {
                best_cost = sk;
                best = {mt, pt, (int)grid};
            }
        }
    }
    if (cost_out) *cost_out = best_cost;
    return best;
}

// ---------------------------------------------------------------- fixed k slabs (split-bf16 path)
// A tile of a group with S slabs sums chunks [s nK / S, (s + 1) nK / S) from zero for each s and
// the slabs are folded in slab order (common.h X6Group::slabs).  S is a function of the layer and
// the segment (slab_count), so the work units (tile, slab) of a launch are fixed before its grid
// is chosen; the grid only decides which workgroup runs which unit.

struct SlabGroup {
    long tiles;
    int S;
};

// per-unit fixed cost in chunks (prologue: weight stages / window DMA; epilogue stores)
constexpr double kUnitOvh = 1.5;

// Longest-first assignment of the units of `gs` (numbered group, tile, slab) to G workgroups:
// each unit costs its chunks + kUnitOvh and goes to the least loaded workgroup (ties: the lowest
// index).  Returns the largest load in chunks; `lists`: per workgroup its units, ascending.
static double lpt_units(const std::vector<SlabGroup>& gs, int nK, int G, std::vector<std::vector<int>>* lists) {
    struct Un {
        double c;
        int id;
    };
    std::vector<Un> us;
    int u = 0;
    double total = 0, big = 0;
    for (const SlabGroup& g : gs)
        for (long t = 0; t < g.tiles; ++t)
            for (int s = 0; s < g.S; ++s, ++u) {
                const double c = (double)((s + 1) * nK / g.S - s * nK / g.S) + kUnitOvh;
                us.push_back({c, u});
                total += c;
                big = std::max(big, c);
            }
    if (!lists && us.size() > 8192) return std::max(total / G, big);  // planning estimate of a large launch
    std::stable_sort(us.begin(), us.end(), [](const Un& a, const Un& b) { return a.c > b.c; });
    std::priority_queue<std::pair<double, int>, std::vector<std::pair<double, int>>, std::greater<>> pq;
    for (int w = 0; w < G; ++w) pq.push({0.0, w});
    if (lists) lists->assign(G, {});
    double mk = 0;
    for (const Un& x : us) {
        auto top = pq.top();
        pq.pop();
        top.first += x.c;
        mk = std::max(mk, top.first);
        if (lists) (*lists)[top.second].push_back(x.id);
        pq.push(top);
    }
    if (lists)
        for (auto& L : *lists) std::sort(L.begin(), L.end());
    return mk;
}

// conv_x6 tile configurations: mt, pt, co-resident workgroups per CU, cost per chunk relative to
// a 64 x 64 tile's (measured, scripts/conv_timing.py; rounds 1-2)
static const int kX6Cfg[6][3] = {{128, 128, 1}, {128, 256, 1}, {256, 128, 1}, {128, 64, 2}, {64, 128, 2}, {64, 64, 3}};
static const double kX6Ovh[6] = {1.5, 1.0, 0.96, 1.1, 1.1, 1.2};
// launches of at most 16,384 columns (one small frame, C2's layers): 128x128 priced like the
// 8-wave tiles and 64x64 higher (round 3, choose_tile: C2 1.91 -> 1.72 ms)
static const double kX6OvhSmall[6] = {1.0, 1.0, 0.96, 1.1, 1.1, 1.6};

// GEMM columns and slab count of one group of a launch
struct ColGroup {
    long cols;
    int S;
};

static std::vector<SlabGroup> slab_groups(const std::vector<ColGroup>& cg, int Mpad, int mt, int pt) {
    std::vector<SlabGroup> gs;
    for (const ColGroup& c : cg) gs.push_back({(long)(Mpad / mt) * ((c.cols + pt - 1) / pt), c.S});
    return gs;
}

// Tile shape and grid of one launch (window kernel: 128 x 256 only) priced in choose_tile's units
// (a 32-deep chunk of a 64 x 64 tile = 0.4): the largest workgroup load (one-slab launches: rounds
// of whole tiles over the hardware dispatcher; else the longest-first unit schedule) times the
// tile's chunk cost, plus the slab partials' HBM round trip and the fixup launch.
struct TilePick {
    int mt = 0, pt = 0, grid = 0;
    double cost = 1e300;
};
static TilePick pick_tile(const std::vector<ColGroup>& cg, bool win, int nK, int Mpad, bool pool = false,
                          bool small_tiles = true) {
    bool multi = false;
    long cols_all = 0;
    for (const ColGroup& c : cg) {
        multi = multi || c.S > 1;
        cols_all += c.cols;
    }
    const double* ovh = cols_all <= 16384 ? kX6OvhSmall : kX6Ovh;
    // multi-slab launches of one small frame's layers (C2; slab_count's small-frame rule): 128 x 64 tiles,
    // one work unit per workgroup slot (slab_count) -- the measured best of 128 x 64 / 128 x 128 /
    // 64 x 128 / 64 x 64 / 128 x 256 at 6-32 slabs on C2's 7x7 layers (round 4 sweep)
    const bool small1 =
        small_tiles && !win && cols_all <= (pool ? 16384L : 4096L) * (long)cg.size() && Mpad % 128 == 0 && multi;
    TilePick best;
    for (int ci = 0; ci < 6; ++ci) {
        const int mt = win ? 128 : kX6Cfg[ci][0], pt = win ? 256 : kX6Cfg[ci][1], occ = win ? 1 : kX6Cfg[ci][2];
        if (win && ci > 0) break;
        if (Mpad % mt) continue;
        if (small1 && (mt != 128 || pt != 64)) continue;
        const std::vector<SlabGroup> gs = slab_groups(cg, Mpad, mt, pt);
        long units = 0, tiles = 0;
        for (const SlabGroup& g : gs) {
            units += g.tiles * g.S;
            tiles += g.tiles;
        }
        // one-slab launches: one workgroup per tile, the hardware dispatcher balancing them
        const long G = multi ? std::min<long>(units, 256L * occ) : tiles;
        const double mk = multi ? lpt_units(gs, nK, (int)G, nullptr) : (double)((tiles + 256L * occ - 1) / (256L * occ)) * nK;
        const double unit = (mt / 64.0) * (pt / 64.0) * (win ? 0.8 : ovh[ci]) * 0.4;
        // co-resident workgroups share a CU; a lone one of a 2-3 per CU tile runs at ~60 %
        const double share = G <= 256 ? (occ >= 2 ? 1.6 : 1.0) : (multi ? std::min<double>(occ, (double)G / 256.0) : occ);
        double cost = mk * unit * share;
        if (multi) cost += (double)units * mt * pt * 4.0 * 2.0 / 5e12 / 0.42e-6 + 8.0;  // slab partials + fixup
        if (cost < best.cost * 0.97) {
            best.cost = cost;
            best.mt = mt;
            best.pt = pt;
            best.grid = (int)G;
        }
    }
    return best;
}

// k slabs of a segment (common.h X6Group::slabs): a function of the layer, its kernel family and
// the segment's logical geometry (N frames of H x W) -- never of the launch that runs it, its
// grid, its other groups or a row band's rows.  Large layers keep one slab (one run over all
// chunks, the data-parallel grids of the bench's 32-frame batch); smaller ones are cut so that
// their work units fill the chip, counting tiles of the kernel's smallest tile (window: 128 x 256,
// conv_x6: 128 x 64) and both branches of a CPM pair.  The hand's layers run as one launch per
// layer for a 4-scale pyramid (lockstep): its 3x3 layers fill the chip with whole tiles (254 /
// 502 tiles over the pyramid), and the 7x7 counts are set per scale size so that the pyramid's
// units pack evenly over 256 workgroups (longest-first, lpt_units).
int slab_count(opose_ctx* h, const DevConv* c, bool win, int N, int H, int W, bool pool) {
    const int nK = win ? c->nK6p : c->nK6;
    if (c->ks == 1 || nK < 8) return 1;  // 1x1: the closing pairs' unfused form sums like the fused chain
    const int smax = nK / 4;
    const long npix = (long)N * H * W;
    const double mr = c->Mpad / 128.0;
    auto clampS = [&](long s) { return (int)std::max<long>(1, std::min<long>(s, smax)); };
    if (c->net == OPOSE_NET_HAND) {
        if (pool) return 1;
        // the 7x7 stages, and conv5_3_CPM (3x3 at H/8, 128 outputs: 65 whole tiles for a 368 crop);
        // conv2_1 (128 outputs at H/2: 994 tiles) runs whole tiles
        if (!(c->ks == 7 && win) && !(c->ks == 3 && c->Mpad <= 128 && c->lvl == 3)) return 1;
        // A 368 crop's scales have 3 / 9 / 19 / 34 tiles: 4 / 7 / 8 / 4 slabs make 363 units whose
        // longest-first packing over 256 workgroups is within a chunk of the best of every table of
        // 1-16 slabs per scale (a makespan model with a per-unit overhead of 4 chunks), with the
        // fewest units of those (fewer partials, a shorter fixup).  Measured, same box: one crop
        // 7.39-7.53 -> 7.09 ms, a 368 + 256 crop batch 13.85-13.97 -> 13.50 ms (round 4's
        // 16 / 12 / 8 / 7; profiles/r5_hand_slabs.log).
        const double T = std::ceil(npix / 256.0) * mr;
        return clampS(T < 6 ? 4 : T < 12 ? 7 : T < 30 ? 8 : T < 60 ? 4 : T < 120 ? 4 : T < 240 ? 2 : 1);
    }
    const int mult = c->pair ? 2 : 1;
    if (std::ceil(npix / 256.0) * mr * mult >= 160) return 1;  // the bench's batches: whole tiles fill the chip
    if (!win && npix <= (pool ? 16384 : 4096) && c->Mpad % 128 == 0) {
        // one small frame (C2 and the pyramid's small scales on conv_x6): 128 x 64 tiles (pick_tile),
        // as many slabs as keep (tiles x slabs) within the 512 workgroup slots (two per CU) -- one
        // unit per workgroup.  C2's 7x7 layers: 10 slabs (300 units) 35.4 us, 16 (480) 33.6 us,
        // 20-32 (several units per workgroup) 40-43 us
        // (pooled convs: conv_x6_fixup pools the folded quads)
        const long tiles = (long)(c->Mpad / 128) * ((npix + 63) / 64) * mult;
        return clampS(std::max<long>(1, 512 / tiles));
    }
    if (pool) return 1;
    // otherwise the count that prices lowest for the segment run alone (with its CPM sibling), as
    // Body(frame) runs a scale -- plus, for one frame whose H/8 map has >= 40 rows (a scale the
    // balanced C5 split may cut into row bands, src/dist.py split_plan), the same layer on a fifth
    // of the rows (+ the band trunk's margin), as a band rank runs it.  A band's smaller launch
    // may take smaller tiles: the tile does not change a pixel's sum, the slab count does.
    const int h8 = H >> (3 - std::min(3, c->lvl));
    const long bpix = N == 1 && h8 >= 40
                          ? (long)std::min(H, H / 5 + (c->lvl < 3 ? 20 << (3 - c->lvl) : 0)) * W
                          : 0;
    const std::string key = std::to_string(win) + "/" + std::to_string(nK) + "/" + std::to_string(c->Mpad) + "/" +
                            std::to_string(npix) + "/" + std::to_string(mult) + "/" + std::to_string(bpix);
    auto it = h->slab_cache.find(key);
    if (it != h->slab_cache.end()) return it->second;
    static const int cand[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 64};
    int best = 1;
    double best_cost = 1e300;
    for (int S : cand) {
        if (S > std::max(1, smax)) break;
        double cost = pick_tile(std::vector<ColGroup>(mult, ColGroup{npix, S}), win, nK, c->Mpad).cost;
        // (the band proxy is a slice of a large scale: any tile, not the small-frame rule's)
        if (bpix) cost += pick_tile(std::vector<ColGroup>(mult, ColGroup{bpix, S}), win, nK, c->Mpad, false, false).cost;
        if (cost < best_cost * 0.97) {
            best_cost = cost;
            best = S;
        }
    }
    h->slab_cache[key] = best;
    return best;
}

// The kernel family of a segment -- conv_x6's (4 groups, 1 tap) chunks or conv_win_x6's pair
// order -- is part of each pixel's summation order, so like the slab count it is a function of
// the layer and the segment only:
//  * the window kernel for 3x3 / 7x7 layers on padded inputs whose window fits the LDS: one frame
//    of any height (conv_win_fits_rows: a 256-pixel run at W columns, so a row band and its whole
//    frame agree), or a batch whose tiles straddle frames;
//  * a 7x7 batch whose straddling windows do not fit but one frame's do: the window kernel on
//    one segment per frame (frame views of the same buffers; a crop batch's 92 x 92 scale);
//  * body layers of fewer than 4096 pixels (C2's single frame, a pyramid's 0.5 scale): conv_x6,
//    whose 128 x 64 tiles spread a small layer over the chip;
//  * the hand's 512-channel 3x3 layers at H/8 (conv4_x, conv5_1/5_2; not conv5_3_CPM's 128 outputs,
//    which take the 7x7 layers' slab layout on the window kernel): conv_x6, whose 256 x 128 tiles
//    cover a 368 crop's 4-scale pyramid in one data-parallel round (254 tiles; the window
//    kernel's 128 x 256 tiles make 260: 225 vs 270 TF/s);
//  * everything else (dense inputs, pooled convs, 1x1): conv_x6.
static int seg_kernel_direct(const opose_ctx* h, const ConvSeg& sg, bool pool) {
    const DevConv* c = sg.c;
    if (!h->win7 || pool || !c->wx6p || !sg.in.padded || (c->ks != 3 && c->ks != 7)) return kKernelX6;
    const long lpix = (long)sg.N * (sg.Hl ? sg.Hl : sg.H) * sg.W;
    if (c->net == OPOSE_NET_BODY && lpix < 4096) return kKernelX6;
    if (c->net == OPOSE_NET_HAND && c->ks == 3 && c->lvl == 3 && c->Mpad > 128) return kKernelX6;
    if (sg.N == 1) return conv_win_fits_rows(sg.W, c->ks) ? kKernelWin : kKernelX6;
    if (conv_win_fits(sg.N, sg.H, sg.W, c->ks)) return kKernelWin;
    if (c->ks == 7 && h->split_frames && conv_win_fits_rows(sg.W, c->ks)) return kKernelWinFrames;
    return kKernelX6;
}

//  * Winograd (conv_wino_x6): a 3x3 segment the window kernel would run as whole tiles (one k
//    slab) whose Winograd window fits (wino_tpf, a function of N, H, W; one frame: of W only);
//    the output pairs sit at even x of the frame, so a row band and its frame still agree.
int seg_kernel(opose_ctx* h, const ConvSeg& sg, bool pool) {
    if (h->force_kernel >= 0) return h->force_kernel;
    const int k = seg_kernel_direct(h, sg, pool);
    const DevConv* c = sg.c;
    if (k == kKernelWin && h->wino && c->ks == 3 && c->wwino &&
        slab_count(h, c, true, sg.N, sg.Hl ? sg.Hl : sg.H, sg.W, pool) == 1 &&
        wino_tpf(sg.N, sg.Hl ? sg.Hl : sg.H, sg.W) >= 0)
        return kKernelWino;
    return k;
}

// Launch plan of one kernel family over segments whose slab counts are set: tile shape, grid,
// and (multi-slab launches) the longest-first unit schedule.  Cached per signature.
ConvPlan plan_launch(opose_ctx* h, const std::vector<ConvSeg>& segs, bool win, bool pool, int nK, int Mpad) {
    std::string key = (win ? "w" : "x") + std::to_string(pool) + "/" + std::to_string(nK) + "/" + std::to_string(Mpad);
    for (const ConvSeg& s : segs)
        key += "/" + std::to_string((long)s.N * s.H * s.W) + ":" + std::to_string(s.slabs) + ":" +
               std::to_string(pool ? s.W : 0);
    auto it = h->plans.find(key);
    if (it != h->plans.end()) return it->second;
    std::vector<ColGroup> cg;
    bool multi = false;
    for (const ConvSeg& s : segs) {
        cg.push_back({pool ? (long)s.N * (s.H / 2) * (s.W / 2) * 4 : (long)s.N * s.H * s.W, s.slabs});
        multi = multi || s.slabs > 1;
    }
    const TilePick tp = pick_tile(cg, win, nK, Mpad, pool);
    ConvPlan best;
    best.mt = tp.mt;
    best.pt = tp.pt;
    best.grid = tp.grid;
    best.sched = nullptr;
    if (multi) {
        std::vector<std::vector<int>> lists;
        lpt_units(slab_groups(cg, Mpad, best.mt, best.pt), nK, best.grid, &lists);
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        OPOSE_HIP_CHECK(hipStreamIsCapturing(h->stream, &cs));
        if (cs != hipStreamCaptureStatusNone) return best;  // (captured: contiguous unit ranges, same sums)
        std::vector<int> flat(best.grid + 1, 0);
        for (int w = 0; w < best.grid; ++w) flat[w + 1] = flat[w] + (int)lists[w].size();
        for (const auto& L : lists) flat.insert(flat.end(), L.begin(), L.end());
        int* d = nullptr;
        OPOSE_HIP_CHECK(hipMalloc(&d, flat.size() * sizeof(int)));
        h->sched_host.push_back(std::move(flat));
        const std::vector<int>& src = h->sched_host.back();
        OPOSE_HIP_CHECK(hipMemcpyAsync(d, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // (once per launch signature)
        h->sched_mem.push_back(d);
        best.sched = d;
    }
    h->plans[key] = best;
    return best;
}

}  // namespace opose