// engine_post.cpp — post-network drivers of libopose: scale geometry, the x8 mid maps, the body
// and hand paths from maps to records / peaks, and the copy of the results to the caller.
#include "engine.h"

namespace opose {

// ---------------------------------------------------------------- geometry (src/body.py:32-41)
static int cv_round(double v) { return (int)std::nearbyint(v); }

ScaleGeom geom(double s, const opose_params& p, int H, int W) {
    ScaleGeom g;
    g.mult = s * p.boxsize / H;
    g.Hs = cv_round(H * g.mult);
    g.Ws = cv_round(W * g.mult);
    if (g.Hs <= 0 || g.Ws <= 0) throw std::invalid_argument("scale produces an empty image");
    g.Hp = round_up(g.Hs, p.stride);
    g.Wp = round_up(g.Ws, p.stride);
    g.hl = g.Hp / 8;
    g.wl = g.Wp / 8;
    g.up_sy = 1.0 / ((double)H / g.Hs);
    g.up_sx = 1.0 / ((double)W / g.Ws);
    return g;
}

// geometry of a scale whose network ran elsewhere: its maps are hl x wl, its padding pad_down /
// pad_right pixels of the 8 hl x 8 wl input (the caller checks the pads: Hs, Ws may be <= 0 here)
ScaleGeom geom_from_pads(int hl, int wl, int pad_down, int pad_right, int H, int W) {
    ScaleGeom g;
    g.mult = 0;
    g.hl = hl;
    g.wl = wl;
    g.Hp = 8 * hl;
    g.Wp = 8 * wl;
    g.Hs = g.Hp - pad_down;
    g.Ws = g.Wp - pad_right;
    g.up_sy = 1.0 / ((double)H / g.Hs);
    g.up_sx = 1.0 / ((double)W / g.Ws);
    return g;
}

// Body mid set of one scale: the x8 heat channels [N][18][Hs][Ws] (read whole by the heat resize),
// then the network's low-res PAF channels [N][38][hl][wl], whose x8 values paf_score evaluates at
// its sample points only (the x8 PAF maps are never written: PafScales::low)
static size_t body_mid_heat(int N, const ScaleGeom& g) { return (size_t)N * 18 * g.Hs * g.Ws; }

// The heat average of a pyramid (src/body.py:57-67, src/hand.py:53-56) into avg [N * C][H][W]:
// scale s's x8 maps are frames [frame0, frame0 + N) of mid set s ([.][C][Hs][Ws]).  Every scale in
// one launch with the average written once (heat_full_scales) where the handle allows it and the
// scales fit, else a launch per scale; f32: one scale, whose average is exactly its float32
// resize -> avg holds a float map.  mid_per_scale: the per-scale profile entries also book the
// mid bytes they read (the body path's do, the hand path's do not).  slot0: the mid set of scale 0.
static void heat_average(opose_ctx* h, int N, int C, int frame0, int H, int W, const std::vector<ScaleGeom>& gs,
                         bool f32, bool mid_per_scale, double* avg, int slot0 = 0) {
    const int ns = (int)gs.size();
    auto mid = [&](int s) {
        return h->mid(slot0 + s).ensure<float>(0, h->stream) + (size_t)frame0 * C * gs[s].Hs * gs[s].Ws;
    };
    ProfEntry pe;
    HeatScales hsc{};
    hsc.n = ns;
    hsc.ns = (float)ns;
    double mid_bytes = 0;
    for (int s = 0; s < ns && s < kHeatScales; ++s) {
        hsc.s[s] = HeatScale{mid(s), C, 0, gs[s].Hs, gs[s].Ws, gs[s].up_sy, gs[s].up_sx};
        mid_bytes += (double)N * C * 4.0 * gs[s].Hs * gs[s].Ws;
    }
    if (!f32 && h->heat_scales && heat_full_scales_fits(hsc, H, W)) {
        h->prof_begin(pe, "heat_full", 0, (double)N * C * H * W * 8.0 + mid_bytes);
        launch_heat_full_scales(hsc, N, C, H, W, avg, h->stream);
        h->prof_end(pe);
        return;
    }
    for (int s = 0; s < ns; ++s) {
        h->prof_begin(pe, "heat_full", 0,
                      (double)N * C * (H * W * (f32 ? 4.0 : 8.0) * (s ? 2 : 1) +
                                       (mid_per_scale ? 4.0 * gs[s].Hs * gs[s].Ws : 0.0)));
        if (f32)
            launch_heat_full_f32(mid(s), C, 0, C, N, gs[s].Hs, gs[s].Ws, H, W, gs[s].up_sy, gs[s].up_sx,
                                 reinterpret_cast<float*>(avg), h->stream);
        else
            launch_heat_full(mid(s), C, 0, C, N, gs[s].Hs, gs[s].Ws, H, W, gs[s].up_sy, gs[s].up_sx, ns, s > 0, avg,
                             h->stream);
        h->prof_end(pe);
    }
}

// the peak-list and matching workspace of N frames at the handle's capacity
struct PeakWS {
    int *cnt, *list;
    double* lscore;
    int *pos, *pcnt;
    double* score;
    Conn* conn;
    int* ccnt;
};
static PeakWS peak_ws(opose_ctx* h, int N) {
    const int cap = h->ppp;
    PeakWS w;
    w.cnt = h->cnt.ensure<int>((size_t)N * 18 + 1, h->stream);  // + gauss_nms_resize's hot-tile count
    w.list = h->list.ensure<int>((size_t)N * 18 * cap, h->stream);
    w.lscore = h->list_score.ensure<double>((size_t)N * 18 * cap, h->stream);
    w.pos = h->peak_pos.ensure<int>((size_t)N * 18 * cap, h->stream);
    w.pcnt = h->part_cnt.ensure<int>((size_t)N * 18, h->stream);
    w.score = h->score.ensure<double>((size_t)N * 19 * cap * cap, h->stream);
    w.conn = h->conn.ensure<Conn>((size_t)N * 19 * cap, h->stream);
    w.ccnt = h->conn_cnt.ensure<int>((size_t)N * 19, h->stream);
    return w;
}

// Second half of the body post path, shared by Body (body_post_common) and Batch_body
// (batch_post_common): the peak-list and matching workspace, then find_peaks(cap, cnt, list, lscore)
// (the caller's NMS over its part maps), then peaks_finalize .. assemble into the records.
// paf_bytes: what the caller's profile books for paf_score.
template <class F>
static void peaks_to_records(opose_ctx* h, int N, int H, int W, const PafScales& S, const opose_params& p,
                             double paf_bytes, uint8_t* rec_dev, F&& find_peaks) {
    const RecordLayout L = make_record_layout(h->ppp, h->maxp);
    const int cap = h->ppp;
    const PeakWS w = peak_ws(h, N);
    int *cnt = w.cnt, *list = w.list, *pos = w.pos, *pcnt = w.pcnt, *ccnt = w.ccnt;
    double *lscore = w.lscore, *score = w.score;
    Conn* conn = w.conn;
    OPOSE_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * ((size_t)N * 18 + 1), h->stream));  // and the hot-tile count
    find_peaks(cap, cnt, list, lscore);
    ProfEntry pe;
    h->prof_begin(pe, "peaks_finalize", 0, 0);
    launch_peaks_finalize(cnt, list, lscore, N, H, W, L, rec_dev, pos, pcnt, h->stream);
    h->prof_end(pe);
    h->prof_begin(pe, "paf_score", 0, paf_bytes);
    launch_paf_score(S, pos, pcnt, N, cap, p.thre2, score, h->stream);
    h->prof_end(pe);
    h->prof_begin(pe, "limb_greedy", 0, 0);
    launch_limb_greedy(score, pcnt, N, cap, conn, ccnt, h->stream);
    h->prof_end(pe);
    h->prof_begin(pe, "assemble", 0, 0);
    launch_assemble(conn, ccnt, pcnt, N, L, rec_dev, h->stream);
    h->prof_end(pe);
}

// what paf_score reads of the per-scale mid sets (body_to_mid) slot0 .. : the low-res PAF channels
PafScales body_paf_scales(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, int slot0) {
    const int ns = (int)gs.size();
    PafScales S{};
    for (int s = 0; s < ns; ++s) {
        S.mid[s] = h->mid(slot0 + s).ensure<float>(0, h->stream);
        S.low[s] = S.mid[s] + body_mid_heat(N, gs[s]);
        S.hs[s] = gs[s].Hs;
        S.ws[s] = gs[s].Ws;
        S.hl[s] = gs[s].hl;
        S.wl[s] = gs[s].wl;
        S.sy[s] = gs[s].up_sy;
        S.sx[s] = gs[s].up_sx;
    }
    S.n = ns;
    S.cm = 18;
    S.lcm = 38;
    S.H = H;
    S.W = W;
    return S;
}

// body_post_common's single-scale form with the heat resize inside the NMS tiles: no average map
static bool body_post_resizes_in_nms(int H, int W, const std::vector<ScaleGeom>& gs) {
    return gs.size() == 1 && gauss_nms_resize_fits(gs[0].Hs, gs[0].Ws, H, W, gs[0].up_sy);
}

// Every buffer body_to_mid (into mid sets slot0 ..) and body_post_common need for N frames of
// H x W, allocated now: a call that runs several groups of frames (opose_body_infer_groups) sizes
// them for every group before it enqueues anything, since a buffer that grows synchronises the
// device and loses its contents.
void body_post_reserve(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, int slot0) {
    for (size_t s = 0; s < gs.size(); ++s)
        h->mid(slot0 + (int)s).ensure<float>(body_mid_heat(N, gs[s]) + (size_t)N * 38 * gs[s].hl * gs[s].wl, h->stream);
    peak_ws(h, N);
    if (body_post_resizes_in_nms(H, W, gs))
        h->hot_tiles.ensure<int>((size_t)gauss_nms_resize_tiles(N, 18, H, W), h->stream);
    else
        h->avg.ensure<double>((size_t)N * 18 * H * W, h->stream);
}

// post-network body path from per-scale mid sets (body_to_mid; scale s in set slot0 + s) to records
void body_post_common(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, const opose_params& p,
                      uint8_t* rec_dev, int slot0) {
    const int ns = (int)gs.size();
    const PafScales S = body_paf_scales(h, N, H, W, gs, slot0);
    // bytes: the low-res PAF channels, read once from HBM (every sample after the first hits L2)
    double paf_bytes = 0;
    for (int s = 0; s < ns; ++s) paf_bytes += (double)N * 38 * 4 * gs[s].hl * gs[s].wl;
    peaks_to_records(h, N, H, W, S, p, paf_bytes, rec_dev, [&](int cap, int* cnt, int* list, double* lscore) {
        ProfEntry pe;
        // single scale: the float64 average equals the float32 resize output exactly -> f32 map
        const bool f32 = ns == 1;
        if (body_post_resizes_in_nms(H, W, gs)) {
            // one scale, a true upsampling resize (the reference's 368-row frames at scale 0.5): the
            // resize runs inside the NMS tiles (post.hip gauss_nms_resize) and tiles whose sources
            // cannot produce a peak are dropped by a screen launch before it (both booked as
            // gauss_nms_resize), so no full-resolution map is written or read.
            // float64-VALU bound: flops = the reference filter's 2 x 37 float64 operations per
            // full-resolution part-map pixel (bench.py GAUSS_OPS_PER_PIXEL); bytes: the x8 heat
            // channels the tiles read
            h->prof_begin(pe, "gauss_nms_resize", 74.0 * N * 18 * (double)H * W,
                          (double)N * 18 * 4.0 * gs[0].Hs * gs[0].Ws);
            int* hot = h->hot_tiles.ensure<int>((size_t)gauss_nms_resize_tiles(N, 18, H, W), h->stream);
            launch_gauss_nms_resize(S.mid[0], 18, 0, 18, N, gs[0].Hs, gs[0].Ws, H, W, gs[0].up_sy, gs[0].up_sx,
                                    p.thre1, cap, cnt, list, lscore, cnt + (size_t)N * 18, hot, 0, h->stream);
            h->prof_end(pe);
            return;
        }
        double* avg = h->avg.ensure<double>((size_t)N * 18 * H * W, h->stream);
        heat_average(h, N, 18, 0, H, W, gs, f32, true, avg, slot0);
        h->prof_begin(pe, "gauss_nms", 0, (double)N * 18 * H * W * (f32 ? 4 : 8));
        launch_gauss_nms(avg, f32, N * 18, H, W, p.thre1, cap, cnt, list, lscore, h->stream);
        h->prof_end(pe);
    });
}

void upsample_to_mid(opose_ctx* h, int s, const float* maps, int cstride, int N, const ScaleGeom& g, int C) {
    float* mid = h->mid(s).ensure<float>((size_t)N * C * g.Hs * g.Ws, h->stream);
    ProfEntry pe;
    h->prof_begin(pe, "upsample8", 0, (double)N * C * g.Hs * g.Ws * 4);
    launch_upsample8(maps, cstride, 0, C, N, g.hl, g.wl, g.Hs, g.Ws, mid, h->stream);
    h->prof_end(pe);
}

// body maps (PAF channels 0..37, heat 38..55 of [N][cstride][hl][wl]) -> mid set s (body_mid_heat)
void body_to_mid(opose_ctx* h, int s, const float* maps, int cstride, int N, const ScaleGeom& g) {
    const size_t heat = body_mid_heat(N, g), lp = (size_t)g.hl * g.wl;
    float* mid = h->mid(s).ensure<float>(heat + (size_t)N * 38 * lp, h->stream);
    ProfEntry pe;
    h->prof_begin(pe, "upsample8", 0, (double)heat * 4 + (double)N * 56 * lp * 4 + (double)N * 38 * lp * 4);
    launch_upsample8(maps, cstride, 38, 18, N, g.hl, g.wl, g.Hs, g.Ws, mid, h->stream);
    OPOSE_HIP_CHECK(hipMemcpy2DAsync(mid + heat, 38 * lp * 4, maps, (size_t)cstride * lp * 4, 38 * lp * 4, N,
                                     hipMemcpyDeviceToDevice, h->stream));
    h->prof_end(pe);
}

// Batch_body fast mode after the network (srcmx/Batch_model.py:159-204): torch bicubic x8
// cropped to nh x nw, torch bicubic to H x W, 5x5 blur + peaks on the blurred map, then the
// shared limb scoring / greedy matching / assembly.  maps: [N][cstride][hl][wl] with PAF
// channels 0..37 and heat 38..56.
// batch_resize_chain: the two resizes, into mid [N][56][nh][nw] (PAF and heat x8, cropped) and
// heat [N][18][H][W].
void batch_resize_chain(opose_ctx* h, int N, int H, int W, const float* maps, int cstride, int hl, int wl, int nh,
                        int nw, float* mid, float* heat) {
    ProfEntry pe;
    h->prof_begin(pe, "upsample8", 0, (double)N * 56 * nh * nw * 4);
    launch_upsample8_torch(maps, cstride, 0, 56, N, hl, wl, nh, nw, mid, h->stream);
    h->prof_end(pe);
    h->prof_begin(pe, "heat_full", 0, (double)N * 18 * (4.0 * H * W + 4.0 * nh * nw));
    launch_resize_torch_f32(mid, 56, 38, 18, N, nh, nw, H, W, heat, h->stream);
    h->prof_end(pe);
}

// what paf_score reads of batch_resize_chain's mid [N][56][nh][nw]: its PAF channels, resampled to
// H x W with torch's taps
PafScales batch_paf_scales(const float* mid, int nh, int nw, int H, int W) {
    PafScales S{};
    S.mid[0] = mid;
    S.hs[0] = nh;
    S.ws[0] = nw;
    S.sy[0] = (double)((float)nh / (float)H);
    S.sx[0] = (double)((float)nw / (float)W);
    S.n = 1;
    S.cm = 56;
    S.H = H;
    S.W = W;
    S.torch = 1;
    return S;
}

void batch_post_common(opose_ctx* h, int N, int H, int W, const float* maps, int cstride, int hl, int wl, int nh,
                       int nw, const opose_params& p, uint8_t* rec_dev) {
    ProfEntry pe;
    float* mid = h->mid(0).ensure<float>((size_t)N * 56 * nh * nw, h->stream);
    float* heat = reinterpret_cast<float*>(h->avg.ensure<double>((size_t)N * 18 * H * W, h->stream));
    batch_resize_chain(h, N, H, W, maps, cstride, hl, wl, nh, nw, mid, heat);
    const PafScales S = batch_paf_scales(mid, nh, nw, H, W);
    peaks_to_records(h, N, H, W, S, p, 0, rec_dev, [&](int cap, int* cnt, int* list, double* lscore) {
        h->prof_begin(pe, "gauss_nms", 0, (double)N * 18 * H * W * 4);
        launch_blur5_nms(heat, N * 18, H, W, p.thre1, cap, cnt, list, lscore, h->stream);
        h->prof_end(pe);
    });
}

// where a hand call writes its NP peaks and found flags on the device, from crop slot out_crop on:
// the caller's buffers (OPOSE_OUT_DEVICE) or the handle's, which hand_finish copies to the host
struct HandDest {
    double* peaks;
    int* found;
};
static HandDest hand_dest(opose_ctx* h, int NP, double* peaks_out, int32_t* found_out, int flags, int out_crop) {
    const bool od = flags & OPOSE_OUT_DEVICE;
    const size_t first = (size_t)out_crop * 21;
    return {(od ? peaks_out : h->hpeaks.ensure<double>((first + NP) * 3, h->stream)) + first * 3,
            (od ? found_out : h->hfound.ensure<int>(first + NP, h->stream)) + first};
}

// Hand post path from per-scale x8 maps (mids[s] = [N][21][Hs][Ws]) to peaks / found.
// mid_crop: first crop of this call inside mids[s] (crop-batched hand path); out_crop: first
// crop's slot in the peaks / found outputs
void hand_post_common(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, const opose_params& p,
                      double* peaks_out, int32_t* found_out, int flags, int mid_crop, int out_crop) {
    const int NP = N * 21;
    double* avg = h->avg.ensure<double>((size_t)NP * H * W, h->stream);
    ProfEntry pe;
    heat_average(h, N, 21, mid_crop, H, W, gs, false, false, avg);
    int* lab = h->hlab.ensure<int>((size_t)NP * H * W, h->stream);
    double* sums = h->hsums.ensure<double>((size_t)NP * H * W, h->stream);
    int* cnt = h->cnt.ensure<int>((size_t)NP, h->stream);
    const HandDest d = hand_dest(h, NP, peaks_out, found_out, flags, out_crop);
    OPOSE_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * NP, h->stream));
    h->prof_begin(pe, "gauss_threshold", 0, (double)NP * H * W * 12);
    launch_gauss_threshold(avg, NP, H, W, p.thre_hand, lab, cnt, sums, h->stream);
    h->prof_end(pe);
    h->prof_begin(pe, "hand_cc", 0, 0);
    void* ws = h->hsel.ensure<uint8_t>(hand_cc_workspace_bytes(NP), h->stream);
    launch_hand_cc(avg, NP, H, W, lab, sums, cnt, d.peaks, d.found, ws, true, h->stream);
    h->prof_end(pe);
}

// copy the hand results to the host (unless they were written to device buffers)
void hand_finish(opose_ctx* h, int N, double* peaks_out, int32_t* found_out, int flags) {
    const int NP = N * 21;
    if (!(flags & OPOSE_OUT_DEVICE)) {
        double* st = h->hand_out.ensure<double>((size_t)NP * 4);  // NP * 3 peaks, then NP found
        int32_t* sf = reinterpret_cast<int32_t*>(st + (size_t)NP * 3);
        OPOSE_HIP_CHECK(hipMemcpyAsync(st, h->hpeaks.ensure<double>((size_t)NP * 3, h->stream), sizeof(double) * NP * 3,
                                       hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(sf, h->hfound.ensure<int>((size_t)NP, h->stream), sizeof(int) * NP,
                                       hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        std::memcpy(peaks_out, st, sizeof(double) * NP * 3);
        std::memcpy(found_out, sf, sizeof(int32_t) * NP);
    }
    h->prof_drain();
}

// Batch_hand after the network (srcmx/Batch_model.py:334-354): maps [N][cstride][H/8][W/8]
// with the 22 heat channels first
void batch_hand_post_common(opose_ctx* h, int N, int H, int W, const float* maps, int cstride, const opose_params& p,
                            double* peaks, int32_t* found, int flags) {
    const int NP = N * 21;
    ProfEntry pe;
    float* mid = h->mid(0).ensure<float>((size_t)NP * H * W, h->stream);
    h->prof_begin(pe, "upsample8", 0, (double)NP * H * W * 4);
    launch_upsample8_torch(maps, cstride, 0, 21, N, H / 8, W / 8, H, W, mid, h->stream);
    h->prof_end(pe);
    double* avg = h->avg.ensure<double>((size_t)NP * H * W, h->stream);
    int* lab = h->hlab.ensure<int>((size_t)NP * H * W, h->stream);
    double* sums = h->hsums.ensure<double>((size_t)NP * H * W, h->stream);
    int* cnt = h->cnt.ensure<int>((size_t)NP, h->stream);
    const HandDest d = hand_dest(h, NP, peaks, found, flags, 0);
    OPOSE_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * NP, h->stream));
    h->prof_begin(pe, "gauss_threshold", 0, (double)NP * H * W * 16);
    launch_blur5_seed(mid, NP, H, W, p.thre_hand, avg, lab, cnt, h->stream);
    h->prof_end(pe);
    h->prof_begin(pe, "hand_cc", 0, 0);
    void* ws = h->hsel.ensure<uint8_t>(hand_cc_workspace_bytes(NP), h->stream);
    launch_hand_cc(avg, NP, H, W, lab, sums, cnt, d.peaks, d.found, ws, false, h->stream);
    h->prof_end(pe);
    hand_finish(h, N, peaks, found, flags & OPOSE_OUT_DEVICE);
}

static int worst_status(const uint8_t* rec, int N, size_t bytes) {
    int w = 0;
    for (int n = 0; n < N; ++n) {
        int s = reinterpret_cast<const int32_t*>(rec + (size_t)n * bytes)[0];
        if (s < w) w = s;
    }
    return w;
}

// where a call's records are written on the device: the caller's buffer (OPOSE_OUT_DEVICE) or the
// handle's, which finish_records copies to the host
uint8_t* records_dest(opose_ctx* h, int N, void* records, int flags) {
    if (flags & OPOSE_OUT_DEVICE) return static_cast<uint8_t*>(records);
    return h->records.ensure<uint8_t>(make_record_layout(h->ppp, h->maxp).bytes * N, h->stream);
}

// finish_records for the n groups of one call (group g: N[g] records at rec_dev[g] for records[g]):
// every copy, then one wait; the worst status of all
int finish_records_groups(opose_ctx* h, int n, const int* N, void* const* records, uint8_t* const* rec_dev,
                          int flags) {
    const RecordLayout L = make_record_layout(h->ppp, h->maxp);
    const bool od = flags & OPOSE_OUT_DEVICE;
    for (int g = 0; g < n; ++g)
        if (rec_dev[g] != records[g])
            OPOSE_HIP_CHECK(hipMemcpyAsync(records[g], rec_dev[g], L.bytes * N[g],
                                           od ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (!od) OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->prof_drain();
    int worst = OPOSE_OK;
    if (!od)
        for (int g = 0; g < n; ++g) worst = std::min(worst, worst_status(static_cast<const uint8_t*>(records[g]), N[g], L.bytes));
    return worst;
}

int finish_records(opose_ctx* h, int N, void* records, uint8_t* rec_dev, int flags) {
    const RecordLayout L = make_record_layout(h->ppp, h->maxp);
    if (flags & OPOSE_OUT_DEVICE) {
        if (rec_dev != records)
            OPOSE_HIP_CHECK(hipMemcpyAsync(records, rec_dev, L.bytes * N, hipMemcpyDeviceToDevice, h->stream));
        h->prof_drain();
        return OPOSE_OK;
    }
    OPOSE_HIP_CHECK(hipMemcpyAsync(records, rec_dev, L.bytes * N, hipMemcpyDeviceToHost, h->stream));
    OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->prof_drain();
    return worst_status(static_cast<const uint8_t*>(records), N, L.bytes);
}

}  // namespace opose
