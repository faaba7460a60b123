// engine_net.cpp — network drivers of libopose: the fp32 and the split-bf16 (X6) forward of the body
// and hand networks, one conv launch per layer over every segment.
#include "engine.h"

namespace opose {

// OPOSE_PIPELINE_DEFER gate: the layer before which the next network records it ("stageN": before
// CPM stage N).  Swept on the bench, same box: conv4_1 2,101, stage2 2,100, stage3 2,105, stage4
// 2,107 frames/s against 2,110 with no gate (a round-4 A/B, kept in git history)
static const std::string& gate_layer() {
    static const std::string g = "conv3_1";
    return g;
}

static const char* conv_class(int ks) { return ks == 7 ? "conv7x7" : (ks == 3 ? "conv3x3" : "conv1x1"); }

// run one (possibly 2-group) conv: out = act(conv(in))
static void run_conv(opose_ctx* h, DevConv* c0, DevConv* c1, int N, int H, int W, Act in0, Act out0, Act in1,
                     Act out1, bool relu0, bool relu1, Act dup = {nullptr, 0, 0}) {
    ConvArgs a{};
    const int ng = c1 ? 2 : 1;
    a.N = N;
    a.H = H;
    a.W = W;
    a.Cin = c0->cin;
    a.ks = c0->ks;
    a.pad = c0->pad;
    a.K = c0->K;
    a.Kpad = c0->Kpad;
    a.Mpad = c0->Mpad;
    a.npix = N * H * W;
    a.tap_major = c0->tap_major ? 1 : 0;
    DevConv* cs[2] = {c0, c1};
    Act ins[2] = {in0, in1}, outs[2] = {out0, out1};
    bool relus[2] = {relu0, relu1};
    for (int g = 0; g < ng; ++g) {
        ConvGroup& G = a.g[g];
        G.in = ins[g].p;
        G.in_cstride = ins[g].cstride;
        G.in_coff = ins[g].coff;
        G.wt = cs[g]->wt;
        G.bias = cs[g]->bias;
        G.out = outs[g].p;
        G.out_cstride = outs[g].cstride;
        G.out_coff = outs[g].coff;
        G.out2 = nullptr;
        G.cout = cs[g]->cout;
        G.relu = relus[g] ? 1 : 0;
    }
    if (dup.p) {
        a.g[0].out2 = dup.p;
        a.g[0].out2_cstride = dup.cstride;
        a.g[0].out2_coff = dup.coff;
    }
    if (ng == 1) a.g[1] = a.g[0];
    for (int g = 0; g < ng; ++g)  // the im2col gather addresses the input with 32-bit byte offsets
        if ((double)N * ins[g].cstride * H * W * 4.0 >= 2147483648.0)
            throw std::invalid_argument("activation slab >= 2 GiB: split the batch");
    const TileChoice t = choose_tile(a.Mpad, std::vector<int>(ng, a.npix), a.Kpad / 32);
    a.ngroups = ng;
    a.sk_grid = t.grid;
    a.partial = h->w().partial.ensure<float>((size_t)2 * t.grid * t.mt * t.pt, h->stream);
    double flops = 0;
    for (int g = 0; g < ng; ++g) flops += 2.0 * cs[g]->cout * (double)a.K * a.npix;
    ProfEntry pe;
    h->prof_begin(pe, conv_class(c0->ks), flops, 0);
    if (h->detail)
        pe.detail = "layer/" + c0->name + "/" + std::to_string(t.mt) + "x" + std::to_string(t.pt) + "s" +
                    std::to_string(t.grid) + "/n" + std::to_string(a.npix);
    launch_conv(a, c0->ktab, t.mt, t.pt, h->stream);
    h->prof_end(pe);
}

static void run_pool(opose_ctx* h, const float* in, float* out, int NC, int H, int W) {
    ProfEntry pe;
    h->prof_begin(pe, "maxpool", 0, (double)NC * H * W * 4 * 1.25);
    launch_maxpool(in, out, NC, H, W, h->stream);
    h->prof_end(pe);
}

// VGG trunk: x [N,3,H,W] -> final trunk conv written via `last` (+ optional duplicate)
static void run_trunk(opose_ctx* h, int net, const float* x, int N, int H, int W, Act last, Act dup) {
    const std::vector<Spec> vgg = net == OPOSE_NET_BODY ? vgg_body() : vgg_hand();
    size_t act = (size_t)N * 64 * H * W;
    float* A = h->w().bufA.ensure<float>(act, h->stream);
    float* B = h->w().bufB.ensure<float>(act, h->stream);
    const float* cur = x;
    int cc = 3, hh = H, ww = W;
    for (size_t i = 0; i < vgg.size(); ++i) {
        const Spec& s = vgg[i];
        DevConv* c = find_conv(h, net, s.name);
        const bool final_layer = i + 1 == vgg.size();
        float* dst = (cur == A) ? B : A;
        Act out = final_layer ? last : Act{dst, s.cout, 0};
        run_conv(h, c, nullptr, N, hh, ww, Act{const_cast<float*>(cur), cc, 0}, out, Act{}, Act{}, true, false,
                 final_layer ? dup : Act{nullptr, 0, 0});
        cur = dst;
        cc = s.cout;
        // pools follow conv1_2, conv2_2, conv3_4 (src/model.py:37,40,45 / :147,150,155)
        if (s.name == "conv1_2" || s.name == "conv2_2" || s.name == "conv3_4") {
            float* pd = (cur == A) ? B : A;
            run_pool(h, cur, pd, N * cc, hh, ww);
            hh /= 2;
            ww /= 2;
            cur = pd;
        }
    }
}

// ---------------------------------------------------------------- split-bf16 network path
static XAct f32act(float* p, int c, int off) {
    XAct a;
    a.p = p;
    a.c = c;
    a.off = off;
    a.f32 = true;
    return a;
}

static uint32_t checked_ps(size_t ps) {
    if (ps * 3 >= 2147483648.0) throw std::invalid_argument("X6 activation >= 2 GiB: split the batch");
    return (uint32_t)ps;
}

// dense X6 [N][cg][H*W], groups [goff, ...)
XAct x6act(uint8_t* p, int cg, int goff, int N, int H, int W) {
    const size_t hw = (size_t)H * W;
    XAct a;
    a.p = p;
    a.ps = checked_ps((size_t)N * cg * hw * 16);
    a.l = X6Layout{(uint32_t)(cg * hw), (uint32_t)hw, (uint32_t)W, (uint32_t)(goff * hw)};
    return a;
}

// padded X6P (common.h): units per (piece, group) plane
size_t x6p_plane(int N, int H, int W) { return (size_t)(N * (H + 3) + 4) * x6p_pitch(W); }

XAct x6pact(uint8_t* p, int cg, int goff, int N, int H, int W) {
    const size_t P = (size_t)x6p_pitch(W), plane = x6p_plane(N, H, W);
    XAct a;
    a.p = p;
    a.ps = checked_ps((size_t)cg * plane * 16);
    a.l = X6Layout{(uint32_t)((H + 3) * P), (uint32_t)plane, (uint32_t)P, (uint32_t)(goff * plane + 3 * P + 3)};
    a.padded = true;
    return a;
}

// frame n of an activation (N frames of H x W) as a one-frame activation of the same buffer
static XAct frame_view(const XAct& a, int n, int H, int W) {
    XAct v = a;
    if (!a.p) return v;
    if (a.f32) v.p = static_cast<float*>(a.p) + (size_t)n * a.c * H * W;
    else v.l.o0 = a.l.o0 + (uint32_t)n * a.l.fs;
    return v;
}

// One launch: segments of one kernel family, at most kX6Groups of them, slab counts set.
static void launch_segs(opose_ctx* h, const std::vector<ConvSeg>& segs, int family, bool pool) {
    const bool win = family == kKernelWin, wino = family == kKernelWino;
    DevConv* c0 = segs[0].c;
    X6Args a{};
    const int ng = (int)segs.size();
    a.ks = c0->ks;
    a.pad = c0->pad;
    a.cin_g = c0->cin_g;
    a.small = c0->small6 ? 1 : 0;
    a.nK = wino ? c0->nKw : win ? c0->nK6p : c0->nK6;
    a.Mpad = c0->Mpad;
    a.pool = pool ? 1 : 0;
    a.ngroups = ng;
    double flops = 0;
    long npix_all = 0;
    for (int g = 0; g < ng; ++g) {
        const ConvSeg& sg = segs[g];
        DevConv* c = sg.c;
        if (c->ks != c0->ks || c->cin_g != c0->cin_g || c->Mpad != c0->Mpad || c->nK6 != c0->nK6 || c->nK6p != c0->nK6p)
            throw std::invalid_argument("conv segments of different shapes");
        if (pool && (sg.dup.p || sg.out.f32)) throw std::invalid_argument("pooled conv: single X6 output only");
        X6Group& G = a.g[g];
        G.in = static_cast<const uint8_t*>(sg.in.p);
        G.in_ps = sg.in.ps;
        G.in_l = sg.in.l;
        G.wt = wino ? c->wwino : win ? c->wx6p : c->wx6;
        G.bias = c->bias;
        G.out = sg.out.p;
        G.out_ps = sg.out.ps;
        G.out_l = sg.out.l;
        G.out_c = sg.out.c;
        G.out_off = sg.out.off;
        G.out_f32 = sg.out.f32 ? 1 : 0;
        G.out2 = sg.dup.p;
        G.out2_ps = sg.dup.ps;
        G.out2_l = sg.dup.l;
        G.cout = c->cout;
        G.relu = sg.relu ? 1 : 0;
        G.N = sg.N;
        G.H = sg.H;
        G.W = sg.W;
        G.npix = pool ? sg.N * (sg.H / 2) * (sg.W / 2) * 4 : sg.N * sg.H * sg.W;
        G.ylo = sg.in.ylo;
        G.yhi = sg.in.yhi;
        G.slabs = sg.slabs;
        G.tpf = wino ? wino_tpf(sg.N, sg.Hl ? sg.Hl : sg.H, sg.W) : 0;
        if (G.yhi && (sg.N != 1 || pool)) throw std::invalid_argument("row band views: one frame, no pooling");
        npix_all += G.npix;
        flops += 2.0 * c->cout * (double)c->K * (pool ? 4.0 * sg.N * (sg.H / 2) * (sg.W / 2) : (double)G.npix);
    }
    if (wino) {
        ProfEntry pe;
        h->prof_begin(pe, conv_class(c0->ks), flops, 0);
        if (h->detail) {
            std::string nm = c0->name;
            for (int g = 1; g < ng; ++g)
                if (segs[g].c != c0 && nm.find(segs[g].c->name) == std::string::npos) nm += "|" + segs[g].c->name;
            pe.detail = "layer/" + nm + "/wino/g" + std::to_string(ng) + "/n" + std::to_string(npix_all);
        }
        launch_conv_wino_x6(a, h->stream);
        h->prof_end(pe);
        return;
    }
    const ConvPlan p = plan_launch(h, segs, win, pool, a.nK, a.Mpad);
    a.sk_grid = p.grid;
    a.sched = p.sched;
    const X6Args num = x6_number_tiles(a, p.mt, p.pt);
    a.partial = num.units != num.tiles ? h->w().partial.ensure<float>((size_t)num.units * p.mt * p.pt, h->stream) : nullptr;
    ProfEntry pe;
    h->prof_begin(pe, conv_class(c0->ks), flops, 0);
    if (h->detail) {
        std::string nm = c0->name;
        for (int g = 1; g < ng; ++g)
            if (segs[g].c != c0 && nm.find(segs[g].c->name) == std::string::npos) nm += "|" + segs[g].c->name;
        pe.detail = "layer/" + nm + "/" + (win ? "win" : "x6") + "/" + std::to_string(p.mt) + "x" + std::to_string(p.pt) +
                    "g" + std::to_string(p.grid) + "u" + std::to_string(num.units) + "/g" + std::to_string(ng) + "/n" +
                    std::to_string(npix_all);
    }
    if (win) launch_conv_win_x6(a, h->stream);
    else launch_conv_x6(a, p.mt, p.pt, h->stream);
    h->prof_end(pe);
}

// Run convs of one shape (ks, Cin, Mpad) over up to kX6Groups segments per launch: the CPM
// branch pair of a stage and the scales of a pyramid share one grid (X6Args groups).
// pool: MaxPool2d(2, 2) (src/model.py:10-13, floor mode) fused into the epilogue; out is then the
// pooled [N][(H/2)(W/2)] X6 tensor (conv outputs the floor mode drops are never computed)
void run_conv_x6_segs(opose_ctx* h, const std::vector<ConvSeg>& segs, bool pool) {
    if (segs.empty()) return;
    // kernel family and slab count per segment, frames of kKernelWinFrames segments as segments
    std::vector<ConvSeg> parts[3];  // conv_x6, conv_win_x6, conv_wino_x6
    for (const ConvSeg& s0 : segs) {
        ConvSeg sg = s0;
        const int kind = seg_kernel(h, sg, pool);
        const bool win = kind != kKernelX6;
        if (kind == kKernelWino) {
            sg.slabs = 1;
            parts[2].push_back(sg);
            continue;
        }
        if (!sg.slabs) sg.slabs = slab_count(h, sg.c, win, sg.N, sg.Hl ? sg.Hl : sg.H, sg.W, pool);
        if (kind == kKernelWinFrames) {
            for (int n = 0; n < sg.N; ++n) {
                ConvSeg f = sg;
                f.N = 1;
                f.in = frame_view(sg.in, n, sg.H, sg.W);
                f.out = frame_view(sg.out, n, sg.H, sg.W);
                f.dup = frame_view(sg.dup, n, sg.H, sg.W);
                parts[1].push_back(f);
            }
        } else {
            parts[win ? 1 : 0].push_back(sg);
        }
    }
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < parts[k].size(); i += kX6Groups)
            launch_segs(h,
                        std::vector<ConvSeg>(parts[k].begin() + i,
                                             parts[k].begin() + std::min(parts[k].size(), i + (size_t)kX6Groups)),
                        k == 0 ? kKernelX6 : k == 1 ? kKernelWin : kKernelWino, pool);
}

// One launch of conv1x1_chain_x6 for every segment (the intermediate never leaves the CU), or,
// with OPOSE_FUSE_1X1=0 or a shape the kernel does not take, the two convs as separate launches
// through `mid`.
static void run_chain_x6(opose_ctx* h, const std::vector<ChainSeg>& segs) {
    // a small frame's 512-wide stage-1 pair (C2: 943 pixels, 15 workgroups of 64 pixels per
    // branch in the fused kernel, 42 us) runs as two launches over 128 x 64 tiles: the same sums
    // (1x1 convs never split k, the fused kernel rounds the intermediate like conv_x6's epilogue).
    // Not a hand pyramid's small scales: they share the fused launch of the large ones.
    auto small_pair = [&](const ChainSeg& sg) {
        return (long)sg.N * (sg.Hl ? sg.Hl : sg.H) * sg.W <= 4096 && sg.c1->cout >= 256 && sg.c1->net == OPOSE_NET_BODY;
    };
    {
        std::vector<ChainSeg> small, rest;
        for (const ChainSeg& sg : segs) (small_pair(sg) ? small : rest).push_back(sg);
        if (!small.empty() && !rest.empty()) {
            run_chain_x6(h, small);
            run_chain_x6(h, rest);
            return;
        }
    }
    bool fuse = h->fuse1x1 && !segs.empty() && segs.size() <= (size_t)kX6Groups && !small_pair(segs[0]);
    for (const ChainSeg& sg : segs) {
        const DevConv *c1 = sg.c1, *c2 = sg.c2;
        fuse = fuse && c1->ks == 1 && c2->ks == 1 && c1->cin_g == 16 && c1->cout == c1->Mpad && c1->Mpad % 128 == 0 &&
               c2->cin == c1->cout && c2->Mpad == 64 && c2->nK6 == c1->cout / 32 && !c1->small6 &&
               c1->cin_g == segs[0].c1->cin_g && c1->cout == segs[0].c1->cout;
    }
    if (!fuse) {
        std::vector<ConvSeg> first, second;
        for (const ChainSeg& sg : segs) {
            first.push_back(ConvSeg{sg.c1, sg.N, sg.H, sg.W, sg.in, sg.mid, XAct{}, true, sg.Hl});
            second.push_back(ConvSeg{sg.c2, sg.N, sg.H, sg.W, sg.mid, sg.out, XAct{}, sg.relu2, sg.Hl});
        }
        run_conv_x6_segs(h, first);
        run_conv_x6_segs(h, second);
        return;
    }
    X6ChainArgs a{};
    a.cin_g = segs[0].c1->cin_g;
    a.m1 = segs[0].c1->cout;
    a.ngroups = (int)segs.size();
    double flops = 0;
    long npix_all = 0;
    for (size_t g = 0; g < segs.size(); ++g) {
        const ChainSeg& sg = segs[g];
        X6ChainGroup& G = a.g[g];
        G.in = static_cast<const uint8_t*>(sg.in.p);
        G.in_ps = sg.in.ps;
        G.in_l = sg.in.l;
        G.w1 = sg.c1->wx6;
        G.b1 = sg.c1->bias;
        G.w2 = sg.c2->wx6;
        G.b2 = sg.c2->bias;
        G.out = sg.out.p;
        G.out_ps = sg.out.ps;
        G.out_l = sg.out.l;
        G.out_c = sg.out.c;
        G.out_off = sg.out.off;
        G.out_f32 = sg.out.f32 ? 1 : 0;
        G.cout2 = sg.c2->cout;
        G.relu2 = sg.relu2 ? 1 : 0;
        G.N = sg.N;
        G.H = sg.H;
        G.W = sg.W;
        G.npix = sg.N * sg.H * sg.W;
        npix_all += G.npix;
        flops += 2.0 * G.npix * ((double)sg.c1->cout * sg.c1->K + (double)sg.c2->cout * sg.c2->K);
    }
    ProfEntry pe;
    h->prof_begin(pe, "conv1x1", flops, 0);
    if (h->detail)
        pe.detail = "layer/" + segs[0].c1->name + ">" + segs[0].c2->name + "/chain/g" + std::to_string(a.ngroups) + "/n" +
                    std::to_string(npix_all);
    launch_conv1x1_chain_x6(a, h->stream);
    h->prof_end(pe);
}

// Zero the padding units of X6P buffers (cg groups each) for an N x H x W geometry.  The convs
// never write them, so a buffer stays valid for its geometry until a forward of another geometry
// writes pixels where this one has pads: clear only on a geometry change (or a reallocation),
// and then invalidate the captured graphs, whose replays assume their own geometry's pads are
// zero.  Inside a stream capture the clear becomes part of the graph (replayed every time) and
// the keys stay unset.
static void clear_x6p_pads(opose_ctx* h, std::initializer_list<std::pair<DevBuf*, int>> bufs, int N, int H, int W) {
    uint8_t* p[8];
    int planes[8];
    DevBuf* owner[8];
    int n = 0;
    for (const auto& b : bufs) {
        const uint64_t key = ((uint64_t)N << 40) ^ ((uint64_t)H << 20) ^ (uint64_t)W ^ ((uint64_t)b.second << 58) ^ 1u;
        if (b.first->pad_key == key) continue;
        p[n] = static_cast<uint8_t*>(b.first->p);
        planes[n] = 3 * b.second;
        owner[n] = b.first;
        ++n;
    }
    if (!n) return;
    ProfEntry pe;
    h->prof_begin(pe, "x6p_pads", 0, 0);
    launch_x6p_clear_pads(p, planes, n, N, H, W, h->stream);
    h->prof_end(pe);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    OPOSE_HIP_CHECK(hipStreamIsCapturing(h->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) return;
    int i = 0;
    for (const auto& b : bufs) {
        const uint64_t key = ((uint64_t)N << 40) ^ ((uint64_t)H << 20) ^ (uint64_t)W ^ ((uint64_t)b.second << 58) ^ 1u;
        if (i < n && owner[i] == b.first) {
            b.first->pad_key = key;
            ++i;
        }
    }
    g_alloc_epoch.fetch_add(1);
}

// VGG trunk on X6 activations: every segment's x -> its final trunk conv written via last[i]
// (+ dup[i]).  Full and half resolution run on dense X6 buffers (A / B); from the second pool on
// (H/4: conv3_x, H/8: conv4_x, conv5_x of the hand) the activations are padded X6P (P0 / P1,
// Q0 / Q1), which the windowed conv_win_x6 reads (conv_x6 reads either layout).
static void run_trunk_x6(opose_ctx* h, int net, const std::vector<NetSeg>& segs, const std::vector<XAct>& last,
                         const std::vector<XAct>& dup) {
    const std::vector<Spec> vgg = net == OPOSE_NET_BODY ? vgg_body() : vgg_hand();
    const size_t ns = segs.size();
    // padded levels (fused pooling only: the separate maxpool_x6 reads and writes dense X6)
    const bool padded = h->fused_pool;
    int maxg4 = 0, maxg8 = 0;  // widest activation (groups) at H/4 and H/8
    {
        int lvl = 0;
        for (const Spec& s : vgg) {
            const int og = (s.cout + 7) / 8;
            const bool pooled = s.name == "conv1_2" || s.name == "conv2_2" || s.name == "conv3_4";
            const int out_lvl = lvl + (pooled ? 1 : 0);
            if (out_lvl == 2) maxg4 = std::max(maxg4, og);
            if (out_lvl == 3) maxg8 = std::max(maxg8, og);
            lvl = out_lvl;
        }
    }
    struct Bufs {
        uint8_t *A, *B, *P0, *P1, *Q0, *Q1;
        XAct cur;
    };
    std::vector<Bufs> bs(ns);
    for (size_t i = 0; i < ns; ++i) {
        const NetSeg& sg = segs[i];
        auto& w = h->ws[sg.slot];
        const int N = sg.N, H = sg.Hp, W = sg.Wp;
        const size_t act = (size_t)N * H * W * 8 * 16 * 3;  // 64 channels at full resolution: the largest dense tensor
        Bufs& b = bs[i];
        b.A = w.x6A.ensure<uint8_t>(act, h->stream);
        b.B = w.x6B.ensure<uint8_t>(act, h->stream);
        b.P0 = b.P1 = b.Q0 = b.Q1 = nullptr;
        if (padded) {
            const int H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
            b.P0 = w.x6P0.ensure<uint8_t>(x6p_plane(N, H4, W4) * maxg4 * 48, h->stream);
            b.P1 = w.x6P1.ensure<uint8_t>(x6p_plane(N, H4, W4) * maxg4 * 48, h->stream);
            b.Q0 = w.x6Q0.ensure<uint8_t>(x6p_plane(N, H8, W8) * maxg8 * 48, h->stream);
            b.Q1 = w.x6Q1.ensure<uint8_t>(x6p_plane(N, H8, W8) * maxg8 * 48, h->stream);
            clear_x6p_pads(h, {{&w.x6P0, maxg4}, {&w.x6P1, maxg4}}, N, H4, W4);
            clear_x6p_pads(h, {{&w.x6Q0, maxg8}, {&w.x6Q1, maxg8}}, N, H8, W8);
        }
    }
    // output buffer of segment i for a layer at resolution level `lvl` (0: H, 1: H/2, 2: H/4,
    // 3: H/8), not the one its input is in
    auto out_buf = [&](size_t i, int lvl, int og) -> XAct {
        const Bufs& b = bs[i];
        const void* avoid = b.cur.p;
        const int N = segs[i].N, hh = segs[i].Hp >> lvl, ww = segs[i].Wp >> lvl;
        if (!padded || lvl < 2) return x6act(avoid == b.A ? b.B : b.A, og, 0, N, hh, ww);
        uint8_t* p = lvl == 2 ? (avoid == b.P0 ? b.P1 : b.P0) : (avoid == b.Q0 ? b.Q1 : b.Q0);
        return x6pact(p, og, 0, N, hh, ww);
    };
    // conv1_1 straight from the fp32 input (conv_first_x6, no input split) of segment i; f32: its
    // output as fp32 units for the windowed conv1_2, which splits them itself
    auto conv11_direct = [&](size_t i, const Spec& s, DevConv* c, bool f32) {
        const NetSeg& sg = segs[i];
        const size_t npix = (size_t)sg.N * sg.Hp * sg.Wp;
        ProfEntry pe;
        h->prof_begin(pe, "conv3x3", 2.0 * 64 * 27 * (double)npix, 0);
        if (h->detail) pe.detail = "layer/" + s.name + "/first_direct/n" + std::to_string(npix);
        launch_conv_first_x6(sg.x, sg.N, 3, sg.Hp, sg.Wp, c->wt, c->Mpad, c->bias, bs[i].A, (uint32_t)(npix * 8 * 16),
                             f32, h->stream);
        h->prof_end(pe);
        bs[i].cur = x6act(bs[i].A, 8, 0, sg.N, sg.Hp, sg.Wp);
        bs[i].cur.f32 = f32;  // (fp32 units at the X6 unit addresses x 2)
    };
    // conv1_2 + pool with the input window in LDS instead of the 9-tap im2col stream (segment i,
    // input at resolution level lvl)
    auto conv12_win_ok = [&](const Spec& s, const DevConv* c) {
        return h->fused_pool && h->win12 && s.name == "conv1_2" && c->cin == 64 && c->cout == 64 && c->ks == 3 &&
               c->pad == 1 && c->Mpad == 64 && c->nK6 == 18 && !c->small6;
    };
    auto conv12_win = [&](size_t i, const Spec& s, DevConv* c, int lvl) {
        const NetSeg& sg = segs[i];
        const int og = (s.cout + 7) / 8;
        const int hh = sg.Hp >> lvl, ww = sg.Wp >> lvl;
        if (bs[i].cur.padded || bs[i].cur.l.fs != 8u * hh * ww) throw std::logic_error("conv1_2 input layout");
        const size_t np = (size_t)sg.N * hh * ww, npo = (size_t)sg.N * (hh / 2) * (ww / 2);
        const XAct out = out_buf(i, lvl + 1, og);
        ProfEntry pe;
        h->prof_begin(pe, "conv3x3", 2.0 * 64 * 576 * (double)(npo * 4), 0);
        if (h->detail) pe.detail = "layer/" + s.name + "/x6win/n" + std::to_string(npo * 4);
        launch_conv3_pool_win_x6(static_cast<const uint8_t*>(bs[i].cur.p), (uint32_t)(np * 8 * 16), sg.N, hh, ww,
                                 c->wx6, c->bias, static_cast<uint8_t*>(out.p), (uint32_t)(npo * 8 * 16),
                                 bs[i].cur.f32, h->stream);
        h->prof_end(pe);
        bs[i].cur = out;
    };
    int lvl = 0;
    for (size_t li = 0; li < vgg.size(); ++li) {
        const Spec& s = vgg[li];
        DevConv* c = find_conv(h, net, s.name);
        if (h->gate_ev && s.name == gate_layer()) {  // OPOSE_PIPELINE_DEFER: the previous post may start
            OPOSE_HIP_CHECK(hipEventRecord(h->gate_ev, h->stream));
            h->gate_done = true;
        }
        if (li == 0 && s.cin == 3 && s.cout == 64 && s.ks == 3 && s.pad == 1 && vgg.size() > 1 && h->first_direct) {
            DevConv* c2 = find_conv(h, net, vgg[1].name);
            const bool pair12 = conv12_win_ok(vgg[1], c2);
            const bool f32 = pair12 && h->c11_f32;
            if (ns > 1 && ns <= (size_t)kConv1Segs && pair12) {
                // a pyramid's conv1_1 and conv1_2 as one launch each over every segment: the
                // small scales' tiles fill the large scale's tail (round 3 ran the per-scale
                // chains on concurrent streams, which a captured graph may not fork any more)
                Conv1Segs S1{}, S2{};
                S1.n = S2.n = (int)ns;
                double f1 = 0, f2 = 0;
                long px1 = 0, px2 = 0;
                for (size_t i = 0; i < ns; ++i) {
                    const NetSeg& sg = segs[i];
                    const size_t npix = (size_t)sg.N * sg.Hp * sg.Wp;
                    const size_t npo = (size_t)sg.N * (sg.Hp / 2) * (sg.Wp / 2);
                    bs[i].cur = x6act(bs[i].A, 8, 0, sg.N, sg.Hp, sg.Wp);  // conv1_1's output
                    const XAct o2 = out_buf(i, 1, 8);                        // (not A)
                    if (o2.p == bs[i].A) throw std::logic_error("conv1_2 output aliases its input");
                    S1.s[i] = Conv1Seg{sg.x, bs[i].A, 0u, (uint32_t)(npix * 8 * 16), sg.N, sg.Hp, sg.Wp, 0};
                    S2.s[i] = Conv1Seg{bs[i].A, static_cast<uint8_t*>(o2.p), (uint32_t)(npix * 8 * 16),
                                       (uint32_t)(npo * 8 * 16), sg.N, sg.Hp, sg.Wp, 0};
                    f1 += 2.0 * 64 * 27 * (double)npix;
                    f2 += 2.0 * 64 * 576 * (double)(npo * 4);
                    px1 += (long)npix;
                    px2 += (long)npo * 4;
                    bs[i].cur = o2;
                }
                ProfEntry pe;
                h->prof_begin(pe, "conv3x3", f1, 0);
                if (h->detail) pe.detail = "layer/" + s.name + "/first_direct/g" + std::to_string(ns) + "/n" + std::to_string(px1);
                launch_conv_first_x6_segs(S1, c->wt, c->Mpad, c->bias, f32, h->stream);
                h->prof_end(pe);
                h->prof_begin(pe, "conv3x3", f2, 0);
                if (h->detail) pe.detail = "layer/" + vgg[1].name + "/x6win/g" + std::to_string(ns) + "/n" + std::to_string(px2);
                launch_conv3_pool_win_x6_segs(S2, c2->wx6, c2->bias, f32, h->stream);
                h->prof_end(pe);
                ++li;
                ++lvl;
                continue;
            }
            for (size_t i = 0; i < ns; ++i) conv11_direct(i, s, c, f32);
            continue;
        }
        if (li == 0) {
            for (size_t i = 0; i < ns; ++i) {
                const NetSeg& sg = segs[i];
                const size_t npix = (size_t)sg.N * sg.Hp * sg.Wp;
                uint8_t* X = h->ws[sg.slot].x6in.ensure<uint8_t>(npix * 16 * 3, h->stream);
                ProfEntry pe;
                h->prof_begin(pe, "to_x6", 0, (double)npix * (12 + 48));
                launch_to_x6(sg.x, 3, 0, 3, sg.N, sg.Hp * sg.Wp, X, 1, 0, (uint32_t)(npix * 16), h->stream);
                h->prof_end(pe);
                bs[i].cur = x6act(X, 1, 0, sg.N, sg.Hp, sg.Wp);
            }
        }
        const bool final_layer = li + 1 == vgg.size();
        const int og = (s.cout + 7) / 8;
        const bool pooled = s.name == "conv1_2" || s.name == "conv2_2" || s.name == "conv3_4";
        if (pooled && conv12_win_ok(s, c)) {
            for (size_t i = 0; i < ns; ++i) conv12_win(i, s, c, lvl);
            ++lvl;
            continue;
        }
        std::vector<ConvSeg> cs;
        std::vector<XAct> outs;
        const bool fuse = pooled && h->fused_pool;  // conv + MaxPool2d(2, 2) in one launch
        for (size_t i = 0; i < ns; ++i) {
            const NetSeg& sg = segs[i];
            const XAct out = fuse ? out_buf(i, lvl + 1, og) : final_layer ? last[i] : out_buf(i, lvl, og);
            outs.push_back(out);
            cs.push_back(ConvSeg{c, sg.N, sg.Hp >> lvl, sg.Wp >> lvl, bs[i].cur, out,
                                 final_layer && !fuse ? dup[i] : XAct{}, true, sg.Hl >> lvl});
        }
        run_conv_x6_segs(h, cs, fuse);
        for (size_t i = 0; i < ns; ++i) bs[i].cur = outs[i];
        if (fuse) {
            ++lvl;
            continue;
        }
        if (pooled) {  // separate MaxPool2d(2, 2) (fused_pool off: dense buffers throughout)
            for (size_t i = 0; i < ns; ++i) {
                const NetSeg& sg = segs[i];
                const int hh = sg.Hp >> lvl, ww = sg.Wp >> lvl;
                const size_t np = (size_t)sg.N * hh * ww;
                Bufs& b = bs[i];
                const XAct pd = x6act(b.cur.p == b.A ? b.B : b.A, og, 0, sg.N, hh / 2, ww / 2);
                ProfEntry pe;
                h->prof_begin(pe, "maxpool", 0, (double)np * og * 48 * 1.25);
                launch_maxpool_x6(static_cast<const uint8_t*>(b.cur.p), (uint32_t)(np * og * 16),
                                  static_cast<uint8_t*>(pd.p), (uint32_t)((size_t)sg.N * (hh / 2) * (ww / 2) * og * 16),
                                  sg.N * og, hh, ww, h->stream);
                h->prof_end(pe);
                b.cur = pd;
            }
            ++lvl;
        }
    }
}

// output rows of a band's trunk past each cut edge (engine body_net_x6; src/dist.py BAND_MARGIN)
constexpr int kBandTrunkMargin = 10;

// bodypose_model.forward on X6 activations, every segment in lockstep; per segment the fp32
// output in its slot's S0 with the fp32 path's layout (channel stride 185: paf [0,38), heat [38,57)).
// band: one segment of one frame, stages on rows [band->r0, band->r1) only, output in band->maps.
std::vector<float*> body_net_x6(opose_ctx* h, const std::vector<NetSeg>& segs, const Band* band) {
    const int SG = 24, TG = 32, UG = 128;  // [L1 | L2 | trunk] = 5 + 3 + 16 groups; 256 / 1024 channels
    const int net = OPOSE_NET_BODY;
    const size_t ns = segs.size();
    // per segment: S (stage inputs) and T (branch activations): padded X6P, read by the 7x7 / 3x3
    // convs; U (conv5_4 output, read by the 1x1 conv5_5): dense
    struct Bufs {
        uint8_t *S[2], *T[2], *U;
        float* O;
        int N, hl, wl;
    };
    std::vector<Bufs> bs(ns);
    std::vector<XAct> last, dup;
    for (size_t i = 0; i < ns; ++i) {
        auto& w = h->ws[segs[i].slot];
        Bufs& b = bs[i];
        b.N = segs[i].N;
        b.hl = segs[i].Hp / 8;
        b.wl = segs[i].Wp / 8;
        const size_t px = (size_t)b.N * b.hl * b.wl, plane = x6p_plane(b.N, b.hl, b.wl);
        b.S[0] = w.x6S0.ensure<uint8_t>(plane * SG * 48, h->stream);
        b.S[1] = w.x6S1.ensure<uint8_t>(plane * SG * 48, h->stream);
        b.T[0] = w.x6T0.ensure<uint8_t>(plane * TG * 48, h->stream);
        b.T[1] = w.x6T1.ensure<uint8_t>(plane * TG * 48, h->stream);
        b.U = w.x6U.ensure<uint8_t>(px * UG * 48, h->stream);
        b.O = w.S0.ensure<float>(px * 185, h->stream);
        clear_x6p_pads(h, {{&w.x6S0, SG}, {&w.x6S1, SG}, {&w.x6T0, TG}, {&w.x6T1, TG}}, b.N, b.hl, b.wl);
        last.push_back(x6pact(b.S[0], SG, 8, b.N, b.hl, b.wl));
        dup.push_back(x6pact(b.S[1], SG, 8, b.N, b.hl, b.wl));
    }
    if (band && (ns != 1 || bs[0].N != 1 || band->r0 < 0 || band->r1 > bs[0].hl || band->r1 - band->r0 < 3))
        throw std::invalid_argument("row band: one frame, 3 <= r1 - r0 rows inside the map");
    // rows a stage layer computes, and the band view of a full-height X6P activation
    const int hb = band ? band->r1 - band->r0 : 0;
    auto rows = [&](size_t i) { return band ? hb : bs[i].hl; };
    auto bview = [&](XAct a) {
        if (band) {
            a.l.o0 += (uint32_t)band->r0 * a.l.rs;
            a.l.fs = (uint32_t)(hb + 3) * a.l.rs;
            a.ylo = band->r0 > 0 ? -3 : 0;
            a.yhi = band->r1 < bs[0].hl ? hb + 3 : hb;
        }
        return a;
    };
    auto s_ = [&](size_t i, int k, int goff) { return bview(x6pact(bs[i].S[k], SG, goff, bs[i].N, bs[i].hl, bs[i].wl)); };
    auto t_ = [&](size_t i, int k, int goff) { return bview(x6pact(bs[i].T[k], TG, goff, bs[i].N, bs[i].hl, bs[i].wl)); };
    auto u_ = [&](size_t i, int goff) { return x6act(bs[i].U, UG, goff, bs[i].N, rows(i), bs[i].wl); };
    // band edges: send the band's first / last 3 rows of groups [g0, g0 + ng) of X6P buffer buf
    // (cg groups) up / down, receive the neighbours' rows into the rows above / below the band
    auto band_halo = [&](uint8_t* buf, int cg, int g0, int ng) {
        if (!band) return;
        const int hl = bs[0].hl, P = x6p_pitch(bs[0].wl);
        const size_t plane = x6p_plane(1, hl, bs[0].wl), bytes = (size_t)9 * ng * P * 16;
        const int mask = (band->r0 > 0 ? 1 : 0) | (band->r1 < hl ? 2 : 0);
        if (!mask) return;
        if (bytes > band->cap) throw std::invalid_argument("row band: halo buffer too small");
        const uint32_t ps = checked_ps((size_t)cg * plane * 16);
        uint8_t* x = band->xbuf;
        const size_t c = band->cap;
        ProfEntry pe;
        h->prof_begin(pe, "band_halo", 0, 4.0 * (double)bytes);
        launch_x6p_halo(buf, ps, (uint32_t)plane, g0, ng, P, 3 + band->r0, band->r1, x, x + c, mask, false, h->stream);
        if (!band->fn) {  // the library's own exchange: RCCL P2P on the handle's stream
            const Rccl& R = rccl();
            rccl_check(R.group_start());
            if (mask & 1) {
                rccl_check(R.send(x, bytes, ncclUint8, h->band_up, h->comm, h->stream));
                rccl_check(R.recv(x + 2 * c, bytes, ncclUint8, h->band_up, h->comm, h->stream));
            }
            if (mask & 2) {
                rccl_check(R.send(x + c, bytes, ncclUint8, h->band_dn, h->comm, h->stream));
                rccl_check(R.recv(x + 3 * c, bytes, ncclUint8, h->band_dn, h->comm, h->stream));
            }
            rccl_check(R.group_end());
        } else if (band->fn(band->user, bytes, h->stream) != 0) {
            throw std::runtime_error("row band: halo exchange failed");
        }
        launch_x6p_halo(buf, ps, (uint32_t)plane, g0, ng, P, band->r0, 3 + band->r1, x + 2 * c, x + 3 * c, mask, true,
                        h->stream);
        h->prof_end(pe);
    };
    // one layer over every segment: branch L1 (conv c1) and, when c2, branch L2
    auto layer = [&](const std::string& n1, const std::string& n2, const std::function<XAct(size_t)>& in1,
                     const std::function<XAct(size_t)>& out1, const std::function<XAct(size_t)>& in2,
                     const std::function<XAct(size_t)>& out2, bool relu1, bool relu2) {
        DevConv* c1 = find_conv(h, net, n1);
        DevConv* c2 = n2.empty() ? nullptr : find_conv(h, net, n2);
        std::vector<ConvSeg> cs;
        for (size_t i = 0; i < ns; ++i) {
            cs.push_back(ConvSeg{c1, bs[i].N, rows(i), bs[i].wl, in1(i), out1(i), XAct{}, relu1, bs[i].hl});
            if (c2) cs.push_back(ConvSeg{c2, bs[i].N, rows(i), bs[i].wl, in2(i), out2(i), XAct{}, relu2, bs[i].hl});
        }
        run_conv_x6_segs(h, cs);
    };
    auto none = [](size_t) { return XAct{}; };
    if (band) {
        // the band's trunk on the input rows its stages need: out1 rows [r0 - 3, r1 + 3) (the 7x7
        // Mconv1 halo) plus kBandTrunkMargin - 3 rows that a cut edge's zero padding corrupts
        // (1 + 1 rows at H, 2 at H/2, 4 at H/4, 4 at H/8: 6.75 rows at H/8); rows a multiple of 8
        // so the three pools see the whole frame's 2x2 windows
        const int hl = bs[0].hl, Wp = segs[0].Wp, Hp = segs[0].Hp;
        const int a = std::max(0, band->r0 - kBandTrunkMargin), b = std::min(hl, band->r1 + kBandTrunkMargin);
        const int Hs = 8 * (b - a);
        float* xs = h->ws[segs[0].slot].xband.ensure<float>((size_t)3 * Hs * Wp, h->stream);
        OPOSE_HIP_CHECK(hipMemcpy2DAsync(xs, (size_t)Hs * Wp * 4, segs[0].x + (size_t)8 * a * Wp, (size_t)Hp * Wp * 4,
                                         (size_t)Hs * Wp * 4, 3, hipMemcpyDeviceToDevice, h->stream));
        auto sub = [&](XAct v) {
            v.l.o0 += (uint32_t)a * v.l.rs;
            v.l.fs = (uint32_t)(b - a + 3) * v.l.rs;
            return v;
        };
        run_trunk_x6(h, net, {NetSeg{xs, 1, Hs, Wp, segs[0].slot, Hp}}, {sub(last[0])}, {sub(dup[0])});
    } else {
        run_trunk_x6(h, net, segs, last, dup);
    }
    layer("conv5_1_CPM_L1+L2", "", [&](size_t i) { return s_(i, 0, 8); }, [&](size_t i) { return t_(i, 0, 0); }, none,
          none, true, false);
    band_halo(bs[0].T[0], TG, 0, TG);
    layer("conv5_2_CPM_L1", "conv5_2_CPM_L2", [&](size_t i) { return t_(i, 0, 0); },
          [&](size_t i) { return t_(i, 1, 0); }, [&](size_t i) { return t_(i, 0, 16); },
          [&](size_t i) { return t_(i, 1, 16); }, true, true);
    band_halo(bs[0].T[1], TG, 0, TG);
    layer("conv5_3_CPM_L1", "conv5_3_CPM_L2", [&](size_t i) { return t_(i, 1, 0); },
          [&](size_t i) { return t_(i, 0, 0); }, [&](size_t i) { return t_(i, 1, 16); },
          [&](size_t i) { return t_(i, 0, 16); }, true, true);
    // 1x1 pairs of both branches and every segment: L1 then L2 of each segment
    auto chain = [&](const std::string& a1, const std::string& a2, const std::string& b1, const std::string& b2,
                     const std::function<ChainSeg(size_t, int, DevConv*, DevConv*)>& mk) {
        DevConv *ca1 = find_conv(h, net, a1), *ca2 = find_conv(h, net, a2);
        DevConv *cb1 = find_conv(h, net, b1), *cb2 = find_conv(h, net, b2);
        std::vector<ChainSeg> cs;
        for (size_t i = 0; i < ns; ++i) {
            cs.push_back(mk(i, 0, ca1, ca2));
            cs.push_back(mk(i, 1, cb1, cb2));
        }
        run_chain_x6(h, cs);
    };
    chain("conv5_4_CPM_L1", "conv5_5_CPM_L1", "conv5_4_CPM_L2", "conv5_5_CPM_L2",
          [&](size_t i, int br, DevConv* c1, DevConv* c2) {
              return ChainSeg{c1, c2, bs[i].N, rows(i), bs[i].wl, t_(i, 0, br ? 16 : 0), u_(i, br ? 64 : 0),
                              s_(i, 1, br ? 5 : 0), false, bs[i].hl};
          });
    band_halo(bs[0].S[1], SG, 0, 8);
    int cur = 1;
    for (int st = 2; st <= 6; ++st) {
        const std::string sf = "_stage" + std::to_string(st);
        if (h->gate_ev && gate_layer() == "stage" + std::to_string(st)) {
            OPOSE_HIP_CHECK(hipEventRecord(h->gate_ev, h->stream));
            h->gate_done = true;
        }
        layer("Mconv1" + sf + "_L1+L2", "", [&](size_t i) { return s_(i, cur, 0); },
              [&](size_t i) { return t_(i, 0, 0); }, none, none, true, false);
        int t = 0;
        for (int k = 2; k <= 5; ++k) {
            band_halo(bs[0].T[t], TG, 0, TG);  // Mconv2..5 read 3 rows past the band
            const std::string nm = "Mconv" + std::to_string(k) + sf;
            layer(nm + "_L1", nm + "_L2", [&](size_t i) { return t_(i, t, 0); },
                  [&](size_t i) { return t_(i, t ^ 1, 0); }, [&](size_t i) { return t_(i, t, 16); },
                  [&](size_t i) { return t_(i, t ^ 1, 16); }, true, true);
            t ^= 1;
        }
        // Mconv6 -> Mconv7; Mconv7: no ReLU, except Mconv7_stage6_L2 (no_relu list quirk,
        // src/model.py:30-33)
        chain("Mconv6" + sf + "_L1", "Mconv7" + sf + "_L1", "Mconv6" + sf + "_L2", "Mconv7" + sf + "_L2",
              [&](size_t i, int br, DevConv* c1, DevConv* c2) {
                  const XAct o = st < 6 ? s_(i, cur ^ 1, br ? 5 : 0)
                                 : band ? f32act(band->maps, 57, br ? 38 : 0) : f32act(bs[i].O, 185, br ? 38 : 0);
                  return ChainSeg{c1, c2, bs[i].N, rows(i), bs[i].wl, t_(i, t, br ? 16 : 0), t_(i, t ^ 1, br ? 16 : 0), o,
                                  br == 1 && st == 6, bs[i].hl};
              });
        if (st < 6) band_halo(bs[0].S[cur ^ 1], SG, 0, 8);  // the next Mconv1 (7x7) reads them
        cur ^= 1;
    }
    std::vector<float*> outs;
    for (const Bufs& b : bs) outs.push_back(b.O);
    return outs;
}

// handpose_model.forward on X6 activations, every segment in lockstep; per segment the fp32
// output in its slot's S0, channel stride 150 (heat [0,22))
std::vector<float*> hand_net_x6(opose_ctx* h, const std::vector<NetSeg>& segs) {
    const int SG = 19, TG = 16, UG = 64;  // [L 22 + 2 | trunk 128] = 3 + 16 groups; 128 / 512 channels
    const int net = OPOSE_NET_HAND;
    const size_t ns = segs.size();
    struct Bufs {
        uint8_t *S[2], *T[2], *U;
        float* O;
        int N, hl, wl;
    };
    std::vector<Bufs> bs(ns);
    std::vector<XAct> last, dup;
    for (size_t i = 0; i < ns; ++i) {
        auto& w = h->ws[segs[i].slot];
        Bufs& b = bs[i];
        b.N = segs[i].N;
        b.hl = segs[i].Hp / 8;
        b.wl = segs[i].Wp / 8;
        const size_t px = (size_t)b.N * b.hl * b.wl, plane = x6p_plane(b.N, b.hl, b.wl);
        b.S[0] = w.x6S0.ensure<uint8_t>(plane * SG * 48, h->stream);
        b.S[1] = w.x6S1.ensure<uint8_t>(plane * SG * 48, h->stream);
        b.T[0] = w.x6T0.ensure<uint8_t>(plane * TG * 48, h->stream);
        b.T[1] = w.x6T1.ensure<uint8_t>(plane * TG * 48, h->stream);
        b.U = w.x6U.ensure<uint8_t>(px * UG * 48, h->stream);
        b.O = w.S0.ensure<float>(px * 150, h->stream);
        clear_x6p_pads(h, {{&w.x6S0, SG}, {&w.x6S1, SG}, {&w.x6T0, TG}, {&w.x6T1, TG}}, b.N, b.hl, b.wl);
        last.push_back(x6pact(b.S[0], SG, 3, b.N, b.hl, b.wl));
        dup.push_back(x6pact(b.S[1], SG, 3, b.N, b.hl, b.wl));
    }
    auto s_ = [&](size_t i, int k, int goff) { return x6pact(bs[i].S[k], SG, goff, bs[i].N, bs[i].hl, bs[i].wl); };
    auto t_ = [&](size_t i, int k) { return x6pact(bs[i].T[k], TG, 0, bs[i].N, bs[i].hl, bs[i].wl); };
    auto u_ = [&](size_t i) { return x6act(bs[i].U, UG, 0, bs[i].N, bs[i].hl, bs[i].wl); };
    auto layer = [&](const std::string& name, const std::function<XAct(size_t)>& in,
                     const std::function<XAct(size_t)>& out, bool relu) {
        DevConv* c = find_conv(h, net, name);
        std::vector<ConvSeg> cs;
        for (size_t i = 0; i < ns; ++i) cs.push_back(ConvSeg{c, bs[i].N, bs[i].hl, bs[i].wl, in(i), out(i), XAct{}, relu});
        run_conv_x6_segs(h, cs);
    };
    auto chain = [&](const std::string& n1, const std::string& n2, const std::function<ChainSeg(size_t, DevConv*, DevConv*)>& mk) {
        DevConv *c1 = find_conv(h, net, n1), *c2 = find_conv(h, net, n2);
        std::vector<ChainSeg> cs;
        for (size_t i = 0; i < ns; ++i) cs.push_back(mk(i, c1, c2));
        run_chain_x6(h, cs);
    };
    run_trunk_x6(h, net, segs, last, dup);
    chain("conv6_1_CPM", "conv6_2_CPM", [&](size_t i, DevConv* c1, DevConv* c2) {
        return ChainSeg{c1, c2, bs[i].N, bs[i].hl, bs[i].wl, s_(i, 0, 3), u_(i), s_(i, 1, 0), false};
    });
    int cur = 1;
    for (int st = 2; st <= 6; ++st) {
        const std::string sf = "_stage" + std::to_string(st);
        layer("Mconv1" + sf, [&](size_t i) { return s_(i, cur, 0); }, [&](size_t i) { return t_(i, 0); }, true);
        int t = 0;
        for (int k = 2; k <= 5; ++k) {
            layer("Mconv" + std::to_string(k) + sf, [&](size_t i) { return t_(i, t); },
                  [&](size_t i) { return t_(i, t ^ 1); }, true);
            t ^= 1;
        }
        chain("Mconv6" + sf, "Mconv7" + sf, [&](size_t i, DevConv* c1, DevConv* c2) {
            const XAct o = st == 6 ? f32act(bs[i].O, 150, 0) : s_(i, cur ^ 1, 0);
            return ChainSeg{c1, c2, bs[i].N, bs[i].hl, bs[i].wl, t_(i, t), t_(i, t ^ 1), o, false};
        });
        cur ^= 1;
    }
    std::vector<float*> outs;
    for (const Bufs& b : bs) outs.push_back(b.O);
    return outs;
}

// bodypose_model.forward (src/model.py:106-133). Output: S-buffer with paf [0,38), heat [38,57)
float* body_net(opose_ctx* h, const float* x, int N, int Hp, int Wp) {
    if (!h->loaded[OPOSE_NET_BODY]) throw std::runtime_error("body weights not loaded");
    if (h->x6) return body_net_x6(h, {NetSeg{x, N, Hp, Wp, h->slot}})[0];
    const int hl = Hp / 8, wl = Wp / 8;
    const size_t px = (size_t)N * hl * wl;
    float* S[2] = {h->w().S0.ensure<float>(px * 185, h->stream), h->w().S1.ensure<float>(px * 185, h->stream)};
    float* T[2] = {h->w().T0.ensure<float>(px * 256, h->stream), h->w().T1.ensure<float>(px * 256, h->stream)};
    float* U = h->w().U.ensure<float>(px * 1024, h->stream);
    const int net = OPOSE_NET_BODY;
    run_trunk(h, net, x, N, Hp, Wp, Act{S[0], 185, 57}, Act{S[1], 185, 57});
    // stage 1 (src/model.py:52-62): input = trunk slice of S0
    run_conv(h, find_conv(h, net, "conv5_1_CPM_L1+L2"), nullptr, N, hl, wl, Act{S[0], 185, 57}, Act{T[0], 256, 0},
             Act{}, Act{}, true, false);
    run_conv(h, find_conv(h, net, "conv5_2_CPM_L1"), find_conv(h, net, "conv5_2_CPM_L2"), N, hl, wl,
             Act{T[0], 256, 0}, Act{T[1], 256, 0}, Act{T[0], 256, 128}, Act{T[1], 256, 128}, true, true);
    run_conv(h, find_conv(h, net, "conv5_3_CPM_L1"), find_conv(h, net, "conv5_3_CPM_L2"), N, hl, wl,
             Act{T[1], 256, 0}, Act{T[0], 256, 0}, Act{T[1], 256, 128}, Act{T[0], 256, 128}, true, true);
    run_conv(h, find_conv(h, net, "conv5_4_CPM_L1"), find_conv(h, net, "conv5_4_CPM_L2"), N, hl, wl,
             Act{T[0], 256, 0}, Act{U, 1024, 0}, Act{T[0], 256, 128}, Act{U, 1024, 512}, true, true);
    run_conv(h, find_conv(h, net, "conv5_5_CPM_L1"), find_conv(h, net, "conv5_5_CPM_L2"), N, hl, wl,
             Act{U, 1024, 0}, Act{S[1], 185, 0}, Act{U, 1024, 512}, Act{S[1], 185, 38}, false, false);
    int cur = 1;
    for (int st = 2; st <= 6; ++st) {
        const std::string s = "_stage" + std::to_string(st);
        float* in = S[cur];
        float* out = S[cur ^ 1];
        run_conv(h, find_conv(h, net, "Mconv1" + s + "_L1+L2"), nullptr, N, hl, wl, Act{in, 185, 0},
                 Act{T[0], 256, 0}, Act{}, Act{}, true, false);
        int t = 0;
        for (int i = 2; i <= 6; ++i) {
            const std::string nm = "Mconv" + std::to_string(i) + s;
            run_conv(h, find_conv(h, net, nm + "_L1"), find_conv(h, net, nm + "_L2"), N, hl, wl, Act{T[t], 256, 0},
                     Act{T[t ^ 1], 256, 0}, Act{T[t], 256, 128}, Act{T[t ^ 1], 256, 128}, true, true);
            t ^= 1;
        }
        // Mconv7: no ReLU, except Mconv7_stage6_L2 (no_relu list quirk, src/model.py:30-33)
        run_conv(h, find_conv(h, net, "Mconv7" + s + "_L1"), find_conv(h, net, "Mconv7" + s + "_L2"), N, hl, wl,
                 Act{T[t], 256, 0}, Act{out, 185, 0}, Act{T[t], 256, 128}, Act{out, 185, 38}, false, st == 6);
        cur ^= 1;
    }
    return S[cur];
}

// handpose_model.forward (src/model.py:197-214). Output: S-buffer with heat [0,22)
float* hand_net(opose_ctx* h, const float* x, int N, int Hp, int Wp) {
    if (!h->loaded[OPOSE_NET_HAND]) throw std::runtime_error("hand weights not loaded");
    if (h->x6) return hand_net_x6(h, {NetSeg{x, N, Hp, Wp, h->slot}})[0];
    const int hl = Hp / 8, wl = Wp / 8;
    const size_t px = (size_t)N * hl * wl;
    float* S[2] = {h->w().S0.ensure<float>(px * 150, h->stream), h->w().S1.ensure<float>(px * 150, h->stream)};
    float* T[2] = {h->w().T0.ensure<float>(px * 128, h->stream), h->w().T1.ensure<float>(px * 128, h->stream)};
    float* U = h->w().U.ensure<float>(px * 512, h->stream);
    const int net = OPOSE_NET_HAND;
    run_trunk(h, net, x, N, Hp, Wp, Act{S[0], 150, 22}, Act{S[1], 150, 22});
    run_conv(h, find_conv(h, net, "conv6_1_CPM"), nullptr, N, hl, wl, Act{S[0], 150, 22}, Act{U, 512, 0}, Act{},
             Act{}, true, false);
    run_conv(h, find_conv(h, net, "conv6_2_CPM"), nullptr, N, hl, wl, Act{U, 512, 0}, Act{S[1], 150, 0}, Act{},
             Act{}, false, false);
    int cur = 1;
    for (int st = 2; st <= 6; ++st) {
        const std::string s = "_stage" + std::to_string(st);
        float* in = S[cur];
        float* out = S[cur ^ 1];
        run_conv(h, find_conv(h, net, "Mconv1" + s), nullptr, N, hl, wl, Act{in, 150, 0}, Act{T[0], 128, 0}, Act{},
                 Act{}, true, false);
        int t = 0;
        for (int i = 2; i <= 6; ++i) {
            run_conv(h, find_conv(h, net, "Mconv" + std::to_string(i) + s), nullptr, N, hl, wl, Act{T[t], 128, 0},
                     Act{T[t ^ 1], 128, 0}, Act{}, Act{}, true, false);
            t ^= 1;
        }
        run_conv(h, find_conv(h, net, "Mconv7" + s), nullptr, N, hl, wl, Act{T[t], 128, 0}, Act{out, 150, 0}, Act{},
                 Act{}, false, false);
        cur ^= 1;
    }
    return S[cur];
}

}  // namespace opose
