// engine_net.cpp — network drivers of libopose: one walk over a network's description (topology.h)
// and its two executors, the fp32 and the split-bf16 (X6) forward, one conv launch per layer over
// every segment.
#include "engine.h"

namespace opose {

// the network's layers as opose_load_weights resolved them
static const NetTable& net_table(opose_ctx* h, int net) {
    if (!h->loaded[net]) throw std::runtime_error(std::string(net_desc(net).what) + " weights not loaded");
    return h->table[net];
}

// OPOSE_PIPELINE_DEFER (NetDesc::gate): the previous call's post-network part may start
static void record_gate(opose_ctx* h) {
    if (!h->gate_ev) return;
    OPOSE_HIP_CHECK(hipEventRecord(h->gate_ev, h->stream));
    h->gate_done = true;
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
static void run_trunk(opose_ctx* h, const NetDesc& d, const NetTable& t, const float* x, int N, int H, int W, Act last,
                      Act dup) {
    const std::vector<Layer>& vgg = d.trunk;
    size_t act = (size_t)N * 64 * H * W;
    float* A = h->w().bufA.ensure<float>(act, h->stream);
    float* B = h->w().bufB.ensure<float>(act, h->stream);
    const float* cur = x;
    int cc = 3, hh = H, ww = W;
    for (size_t i = 0; i < vgg.size(); ++i) {
        const Spec& s = vgg[i].s;
        DevConv* c = t.trunk[i];
        const bool final_layer = i + 1 == vgg.size();
        float* dst = (cur == A) ? B : A;
        Act out = final_layer ? last : Act{dst, s.cout, 0};
        run_conv(h, c, nullptr, N, hh, ww, Act{const_cast<float*>(cur), cc, 0}, out, Act{}, Act{}, true, false,
                 final_layer ? dup : Act{nullptr, 0, 0});
        cur = dst;
        cc = s.cout;
        if (vgg[i].pool) {  // (src/model.py:37,40,45 / :147,150,155)
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

// "layer/<names>" of a launch's profiler detail: the first segment's layer and every other one
static std::string layer_names(const std::vector<ConvSeg>& segs) {
    std::string nm = segs[0].c->name;
    for (size_t g = 1; g < segs.size(); ++g)
        if (segs[g].c != segs[0].c && nm.find(segs[g].c->name) == std::string::npos) nm += "|" + segs[g].c->name;
    return "layer/" + nm;
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
        if (h->detail) pe.detail = layer_names(segs) + "/wino/g" + std::to_string(ng) + "/n" + std::to_string(npix_all);
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
    if (h->detail)
        pe.detail = layer_names(segs) + "/" + (win ? "win" : "x6") + "/" + std::to_string(p.mt) + "x" + std::to_string(p.pt) +
                    "g" + std::to_string(p.grid) + "u" + std::to_string(num.units) + "/g" + std::to_string(ng) + "/n" +
                    std::to_string(npix_all);
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
    if (segs.size() > (size_t)kX6Groups) {  // more pairs than a launch has groups (five or more body segments)
        for (size_t i = 0; i < segs.size(); i += kX6Groups)
            run_chain_x6(h, std::vector<ChainSeg>(segs.begin() + i, segs.begin() + std::min(segs.size(), i + (size_t)kX6Groups)));
        return;
    }
    bool fuse = h->fuse1x1 && !segs.empty() && !small_pair(segs[0]);
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
    launch_chain_segs(h, segs);
}

// The fused form: one conv1x1_chain_x6 launch over segments whose pairs run_chain_x6 found to fit it
void launch_chain_segs(opose_ctx* h, const std::vector<ChainSeg>& segs) {
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
static void run_trunk_x6(opose_ctx* h, const NetDesc& d, const NetTable& t, const std::vector<NetSeg>& segs,
                         const std::vector<XAct>& last, const std::vector<XAct>& dup) {
    const std::vector<Layer>& vgg = d.trunk;
    const size_t ns = segs.size();
    // padded levels (fused pooling only: the separate maxpool_x6 reads and writes dense X6)
    const bool padded = h->fused_pool;
    int maxg4 = 0, maxg8 = 0;  // widest activation (groups) at H/4 and H/8
    for (const Layer& L : vgg) {
        const int og = (L.s.cout + 7) / 8, out_lvl = L.lvl + (L.pool ? 1 : 0);
        if (out_lvl == 2) maxg4 = std::max(maxg4, og);
        if (out_lvl == 3) maxg8 = std::max(maxg8, og);
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
    auto conv12_win_ok = [&](size_t li, const DevConv* c) {
        return h->fused_pool && h->win12 && li == 1 && vgg[li].pool && c->cin == 64 && c->cout == 64 && c->ks == 3 &&
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
    for (size_t li = 0; li < vgg.size(); ++li) {
        const Spec& s = vgg[li].s;
        const int lvl = vgg[li].lvl;
        const bool pooled = vgg[li].pool;
        DevConv* c = t.trunk[li];
        if ((int)li == d.gate_trunk) record_gate(h);
        if (li == 0 && s.cin == 3 && s.cout == 64 && s.ks == 3 && s.pad == 1 && vgg.size() > 1 && h->first_direct) {
            DevConv* c2 = t.trunk[1];
            const bool pair12 = conv12_win_ok(1, c2);
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
                if (h->detail) pe.detail = "layer/" + vgg[1].s.name + "/x6win/g" + std::to_string(ns) + "/n" + std::to_string(px2);
                launch_conv3_pool_win_x6_segs(S2, c2->wx6, c2->bias, f32, h->stream);
                h->prof_end(pe);
                ++li;
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
        if (conv12_win_ok(li, c)) {
            for (size_t i = 0; i < ns; ++i) conv12_win(i, s, c, lvl);
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
        if (pooled && !fuse) {  // separate MaxPool2d(2, 2) (fused_pool off: dense buffers throughout)
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
        }
    }
}

// ---------------------------------------------------------------- the CPM stages, both paths
// Where a stage's step reads or writes: the stage-input concat S[k] (whole, its trunk slice, or a
// branch's output slice), the branches' activations T[k], or stage 1's hidden 1x1 outputs U.
struct Place {
    enum Buf { S, T, U } buf;
    int k;  // which of S[2] / T[2]
    enum Part { Whole, Trunk, Branch } part;
};

// The stages of a forward in launch order, once the trunk has written the trunk slice of S[0] and
// S[1] (src/model.py:106-133, :197-214).  conv(st, c0, c1, in, out): one layer with ReLU; c1 null:
// c0 on `in` and `out` as they are (a stage's opening layer, every branch's outputs in one conv),
// else c0 / c1 on branch 0's / 1's slices.  close(st, c, in, mid, out, relu2): per branch b the
// 1x1 pair c[b][0] -> c[b][1] from in through mid to out, the second with ReLU where relu2[b].
// Returns k of the S buffer the last stage wrote.
template <class Conv, class Close>
static int walk_stages(const NetDesc& d, const NetTable& t, Conv&& conv, Close&& close) {
    int cur = 0;
    for (int st = 1; st <= kStages; ++st, cur ^= 1) {
        const NetTable::Stage& ts = t.stages[st - 1];
        const Place sin{Place::S, cur, st == 1 ? Place::Trunk : Place::Whole};
        if (ts.open) conv(st, ts.open, nullptr, sin, Place{Place::T, 0, Place::Whole});
        int tb = 0;
        for (size_t m = 0; m < ts.mid[0].size(); ++m, tb ^= 1)
            conv(st, ts.mid[0][m], d.branches == 2 ? ts.mid[1][m] : nullptr, Place{Place::T, tb, Place::Branch},
                 Place{Place::T, tb ^ 1, Place::Branch});
        // stage 1's pair is wider than T: through U
        close(st, ts.close, ts.open ? Place{Place::T, tb, Place::Branch} : sin,
              st == 1 ? Place{Place::U, 0, Place::Branch} : Place{Place::T, tb ^ 1, Place::Branch},
              Place{Place::S, cur ^ 1, Place::Branch}, d.stages[st - 1].relu2);
    }
    return cur;
}

// output rows of a band's trunk past each cut edge (net_forward_x6; src/dist.py BAND_MARGIN)
constexpr int kBandTrunkMargin = 10;

// A network's forward on X6 activations, every segment in lockstep; per segment the fp32 output in
// its slot's S0 with the fp32 path's layout (channel stride NetDesc::Sc, branch b at s_off[b]).
// band (body only): one segment of one frame, stages on rows [band->r0, band->r1) only, output in
// band->maps.
std::vector<float*> net_forward_x6(opose_ctx* h, int net, const std::vector<NetSeg>& segs, const Band* band) {
    const NetDesc& d = net_desc(net);
    const NetTable& t = net_table(h, net);
    const size_t ns = segs.size();
    // per segment: S (stage inputs) and T (branch activations): padded X6P, read by the 7x7 / 3x3
    // convs; U (stage 1's hidden 1x1 outputs, read by its second 1x1): dense
    struct Bufs {
        uint8_t *S[2], *T[2], *U;
        int N, hl, wl;
    };
    std::vector<Bufs> bs(ns);
    std::vector<XAct> last, dup;
    std::vector<float*> outs;
    for (size_t i = 0; i < ns; ++i) {
        auto& w = h->ws[segs[i].slot];
        Bufs& b = bs[i];
        b.N = segs[i].N;
        b.hl = segs[i].Hp / 8;
        b.wl = segs[i].Wp / 8;
        const size_t px = (size_t)b.N * b.hl * b.wl, plane = x6p_plane(b.N, b.hl, b.wl);
        b.S[0] = w.x6S0.ensure<uint8_t>(plane * d.SG * 48, h->stream);
        b.S[1] = w.x6S1.ensure<uint8_t>(plane * d.SG * 48, h->stream);
        b.T[0] = w.x6T0.ensure<uint8_t>(plane * d.TG * 48, h->stream);
        b.T[1] = w.x6T1.ensure<uint8_t>(plane * d.TG * 48, h->stream);
        b.U = w.x6U.ensure<uint8_t>(px * d.UG * 48, h->stream);
        outs.push_back(w.S0.ensure<float>(px * d.Sc, h->stream));
        clear_x6p_pads(h, {{&w.x6S0, d.SG}, {&w.x6S1, d.SG}, {&w.x6T0, d.TG}, {&w.x6T1, d.TG}}, b.N, b.hl, b.wl);
        last.push_back(x6pact(b.S[0], d.SG, d.trunk_goff, b.N, b.hl, b.wl));
        dup.push_back(x6pact(b.S[1], d.SG, d.trunk_goff, b.N, b.hl, b.wl));
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
    // segment i's activation at p, branch b's slice where p names the branches'
    auto at = [&](size_t i, Place p, int b) {
        const Bufs& B = bs[i];
        if (p.buf == Place::S)
            return bview(x6pact(B.S[p.k], d.SG, p.part == Place::Trunk ? d.trunk_goff : p.part == Place::Branch ? d.s_goff[b] : 0,
                                B.N, B.hl, B.wl));
        if (p.buf == Place::T) return bview(x6pact(B.T[p.k], d.TG, p.part == Place::Branch ? b * kMid / 8 : 0, B.N, B.hl, B.wl));
        return x6act(B.U, d.UG, b * kHidden / 8, B.N, rows(i), B.wl);
    };
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
        run_trunk_x6(h, d, t, {NetSeg{xs, 1, Hs, Wp, segs[0].slot, Hp}}, {sub(last[0])}, {sub(dup[0])});
    } else {
        run_trunk_x6(h, d, t, segs, last, dup);
    }
    walk_stages(
        d, t,
        [&](int st, DevConv* c0, DevConv* c1, Place in, Place out) {
            if (in.buf == Place::S && st == d.gate_stage) record_gate(h);
            // a 3x3 / 7x7 layer reads 3 rows of T past the band
            if (in.buf == Place::T && c0->ks > 1) band_halo(bs[0].T[in.k], d.TG, 0, d.TG);
            std::vector<ConvSeg> cs;
            for (size_t i = 0; i < ns; ++i) {
                cs.push_back(ConvSeg{c0, bs[i].N, rows(i), bs[i].wl, at(i, in, 0), at(i, out, 0), XAct{}, true, bs[i].hl});
                if (c1) cs.push_back(ConvSeg{c1, bs[i].N, rows(i), bs[i].wl, at(i, in, 1), at(i, out, 1), XAct{}, true, bs[i].hl});
            }
            run_conv_x6_segs(h, cs);
        },
        [&](int st, DevConv* const(*c)[2], Place in, Place mid, Place out, const bool* relu2) {
            // every segment's branches in one launch; the last stage writes the fp32 output
            std::vector<ChainSeg> cs;
            for (size_t i = 0; i < ns; ++i)
                for (int b = 0; b < d.branches; ++b) {
                    const XAct o = st < kStages ? at(i, out, b)
                                   : band       ? f32act(band->maps, d.trunk_off, d.s_off[b])
                                                : f32act(outs[i], d.Sc, d.s_off[b]);
                    cs.push_back(ChainSeg{c[b][0], c[b][1], bs[i].N, rows(i), bs[i].wl, at(i, in, b), at(i, mid, b), o,
                                          relu2[b], bs[i].hl});
                }
            run_chain_x6(h, cs);
            if (st < kStages) band_halo(bs[0].S[out.k], d.SG, 0, d.trunk_goff);  // the next opening 7x7 reads them
        });
    return outs;
}

// A network's forward (src/model.py:106-133, :197-214).  Output: S buffer, channel stride
// NetDesc::Sc, branch b's maps at s_off[b] (body: paf [0,38), heat [38,57); hand: heat [0,22))
float* net_forward(opose_ctx* h, int net, const float* x, int N, int Hp, int Wp) {
    const NetDesc& d = net_desc(net);
    const NetTable& t = net_table(h, net);
    if (h->x6) return net_forward_x6(h, net, {NetSeg{x, N, Hp, Wp, h->slot}})[0];
    const int hl = Hp / 8, wl = Wp / 8;
    const size_t px = (size_t)N * hl * wl;
    float* S[2] = {h->w().S0.ensure<float>(px * d.Sc, h->stream), h->w().S1.ensure<float>(px * d.Sc, h->stream)};
    float* T[2] = {h->w().T0.ensure<float>(px * d.Tc, h->stream), h->w().T1.ensure<float>(px * d.Tc, h->stream)};
    float* U = h->w().U.ensure<float>(px * d.Uc, h->stream);
    auto at = [&](Place p, int b) {
        if (p.buf == Place::S)
            return Act{S[p.k], d.Sc, p.part == Place::Trunk ? d.trunk_off : p.part == Place::Branch ? d.s_off[b] : 0};
        if (p.buf == Place::T) return Act{T[p.k], d.Tc, p.part == Place::Branch ? b * kMid : 0};
        return Act{U, d.Uc, b * kHidden};
    };
    // a layer's conv, or both branches' convs in one launch (c1 null: one conv)
    auto pair = [&](DevConv* c0, DevConv* c1, Place in, Place out, bool relu0, bool relu1) {
        run_conv(h, c0, c1, N, hl, wl, at(in, 0), at(out, 0), c1 ? at(in, 1) : Act{}, c1 ? at(out, 1) : Act{}, relu0, relu1);
    };
    run_trunk(h, d, t, x, N, Hp, Wp, at(Place{Place::S, 0, Place::Trunk}, 0), at(Place{Place::S, 1, Place::Trunk}, 0));
    const int k = walk_stages(
        d, t, [&](int, DevConv* c0, DevConv* c1, Place in, Place out) { pair(c0, c1, in, out, true, true); },
        [&](int, DevConv* const(*c)[2], Place in, Place mid, Place out, const bool* relu2) {
            pair(c[0][0], c[1][0], in, mid, true, true);  // (one branch: c[1] is null)
            pair(c[0][1], c[1][1], mid, out, relu2[0], relu2[1]);
        });
    return S[k];
}

}  // namespace opose
