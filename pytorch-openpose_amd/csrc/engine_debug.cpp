// engine_debug.cpp — libopose's test hooks: single launches and stages behind the C ABI.
#include "engine.h"

using namespace opose;

// ------------------------------------------------------------------ test hooks
int opose_debug_conv(opose_t* h, const float* x, const float* w, const float* b, int N, int Cin, int H, int W,
                     int Cout, int ks, int pad, int relu, int mt, int pt, int splits, float* out) {
    if (!h || !x || !w || !b || !out || ks > 15 || pad > 7) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        Spec s{"debug", Cin, Cout, ks, pad};
        upload_conv(h, 0, "__debug__", {&s}, {w}, {b}, 3, false);
        DevConv* c = h->convs[0]["__debug__"].get();
        DevBuf xin, yout;
        const size_t nx = (size_t)N * Cin * H * W, ny = (size_t)N * Cout * H * W;
        float* xd = xin.ensure<float>(nx, h->stream);
        float* yd = yout.ensure<float>(ny, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(xd, x, nx * 4, hipMemcpyHostToDevice, h->stream));
        ConvArgs a{};
        a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ks = ks; a.pad = pad;
        a.K = c->K; a.Kpad = c->Kpad; a.Mpad = c->Mpad; a.npix = N * H * W;
        a.tap_major = c->tap_major ? 1 : 0;
        ConvGroup& G = a.g[0];
        G.in = xd; G.in_cstride = Cin; G.in_coff = 0; G.wt = c->wt; G.bias = c->bias;
        G.out = yd; G.out_cstride = Cout; G.out_coff = 0; G.out2 = nullptr; G.cout = Cout; G.relu = relu;
        a.g[1] = a.g[0];
        TileChoice t = choose_tile(a.Mpad, {a.npix}, a.Kpad / 32);
        if (mt > 0) { t.mt = mt; t.pt = pt; t.grid = (a.Mpad / mt) * ((a.npix + pt - 1) / pt); }
        if (splits > 0) t.grid = splits;
        if (a.Mpad % t.mt) throw std::invalid_argument("tile M does not divide Mpad");
        a.ngroups = 1;
        a.sk_grid = t.grid;
        a.partial = h->w().partial.ensure<float>((size_t)2 * t.grid * t.mt * t.pt, h->stream);
        launch_conv(a, c->ktab, t.mt, t.pt, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(out, yd, ny * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->convs[0].erase("__debug__");
    });
    return OPOSE_OK;
}

// Test-hook plan of a conv_x6 launch (groups filled): tile mt x pt (0: choose_tile's data-parallel
// pick), `slabs` k slabs per tile (<= 1: one; clamped to nK), one workgroup per whole tile or,
// with slabs, min(units, 256) workgroups over contiguous unit ranges; sets grid, units, partials.
static TileChoice debug_x6_plan(opose_ctx* h, X6Args& a, int mt, int pt, int slabs) {
    std::vector<int> gpix;
    for (int g = 0; g < a.ngroups; ++g) gpix.push_back(a.g[g].npix);
    TileChoice t = choose_tile(a.Mpad, gpix, a.nK, true, true);
    if (mt > 0) {
        t.mt = mt;
        t.pt = pt;
    }
    if (a.Mpad % t.mt) throw std::invalid_argument("tile M does not divide Mpad");
    for (int g = 0; g < a.ngroups; ++g) a.g[g].slabs = std::max(1, std::min(slabs, a.nK));
    const X6Args num = x6_number_tiles(a, t.mt, t.pt);
    t.grid = num.units == num.tiles ? num.tiles : std::min(num.units, 256);
    a.sk_grid = t.grid;
    a.sched = nullptr;
    a.partial = h->w().partial.ensure<float>((size_t)num.units * t.mt * t.pt, h->stream);
    return t;
}

// ---- the host's X6 split and join (the kernels' split3: each piece the round-to-nearest-even bf16
// of what the pieces before it left), for activations of any X6Layout (dense or X6P, a group slice)
static uint16_t bf16_rne(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_f32(uint16_t hb) {
    const uint32_t u = (uint32_t)hb << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
static size_t host_unit(const XAct& a, int n, int g, int y, int x) {
    return (size_t)a.l.o0 + (size_t)n * a.l.fs + (size_t)g * a.l.gs + (size_t)y * a.l.rs + x;
}
// x fp32 [N][C][H][W] -> the pixels' units of activation `a` in hx (three piece planes of a.ps bytes)
static void host_split_x6(const float* x, int N, int C, int H, int W, const XAct& a, uint16_t* hx) {
    const size_t pl = a.ps / 2;  // bf16 per piece
    for (int n = 0; n < N; ++n)
        for (int ch = 0; ch < C; ++ch)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) {
                    const float v = x[(((size_t)n * C + ch) * H + y) * W + xx];
                    const size_t e = host_unit(a, n, ch / 8, y, xx) * 8 + ch % 8;
                    const uint16_t h0 = bf16_rne(v);
                    const float r = v - bf16_f32(h0);
                    const uint16_t h1 = bf16_rne(r);
                    hx[e] = h0;
                    hx[pl + e] = h1;
                    hx[2 * pl + e] = bf16_rne(r - bf16_f32(h1));
                }
}
// the piece planes hy of activation `a` -> out fp32 [N][C][H][W] ((x0 + x1) + x2, as from_x6 sums)
static void host_join_x6(const uint16_t* hy, const XAct& a, int N, int C, int H, int W, float* out) {
    const size_t pl = a.ps / 2;
    for (int n = 0; n < N; ++n)
        for (int ch = 0; ch < C; ++ch)
            for (int y = 0; y < H; ++y)
                for (int xx = 0; xx < W; ++xx) {
                    const size_t e = host_unit(a, n, ch / 8, y, xx) * 8 + ch % 8;
                    out[(((size_t)n * C + ch) * H + y) * W + xx] =
                        (bf16_f32(hy[e]) + bf16_f32(hy[pl + e])) + bf16_f32(hy[2 * pl + e]);
                }
}

// split-bf16 conv of one layer: x fp32 NCHW -> X6 -> conv_x6 -> fp32 (out_x6: through an X6
// output buffer and back, exercising the split epilogue)
int opose_debug_conv_x6(opose_t* h, const float* x, const float* w, const float* b, int N, int Cin, int H, int W,
                        int Cout, int ks, int pad, int relu, int mt, int pt, int splits, int out_x6, float* out) {
    if (!h || !x || !w || !b || !out || ks > 15 || pad > 7) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        Spec s{"debug", Cin, Cout, ks, pad};
        upload_conv(h, 0, "__debug__", {&s}, {w}, {b}, 3, false);
        DevConv* c = h->convs[0]["__debug__"].get();
        const int HW = H * W;
        const int cg = c->cin_g, og = (Cout + 7) / 8;
        if (mt <= -2) {
            // padded (X6P) input and output through run_conv_x6_segs with the family under test
            // forced: -2 the window kernel, -3 Winograd (conv_wino_x6); the host splits and joins
            XAct ia = x6pact(nullptr, cg, 0, N, H, W), oa = x6pact(nullptr, og, 0, N, H, W);
            std::vector<uint16_t> hx((size_t)3 * (ia.ps / 2), 0), hy((size_t)3 * (oa.ps / 2));
            host_split_x6(x, N, Cin, H, W, ia, hx.data());
            DevBuf bi, bo;
            ia.p = bi.ensure<uint8_t>(hx.size() * 2, h->stream);
            oa.p = bo.ensure<uint8_t>(hy.size() * 2, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(ia.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, h->stream));
            OPOSE_HIP_CHECK(hipMemsetAsync(oa.p, 0, hy.size() * 2, h->stream));
            ConvSeg sg{c, N, H, W, ia, oa, XAct{}, relu != 0};
            if (mt == -3) sg.slabs = 1;
            {
                Redirect<int> family(h->force_kernel, mt == -3 ? kKernelWino : kKernelWin);
                run_conv_x6_segs(h, {sg});
            }
            OPOSE_HIP_CHECK(hipMemcpyAsync(hy.data(), oa.p, hy.size() * 2, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            host_join_x6(hy.data(), oa, N, Cout, H, W, out);
            h->convs[0].erase("__debug__");
            return OPOSE_OK;
        }
        DevBuf xin, xx, yx, yout;
        const size_t nx = (size_t)N * Cin * HW, ny = (size_t)N * Cout * HW;
        const uint32_t ips = (uint32_t)((size_t)N * cg * HW * 16), ops = (uint32_t)((size_t)N * og * HW * 16);
        float* xd = xin.ensure<float>(nx, h->stream);
        uint8_t* x6 = xx.ensure<uint8_t>((size_t)ips * 3, h->stream);
        uint8_t* y6 = yx.ensure<uint8_t>((size_t)ops * 3, h->stream);
        float* yd = yout.ensure<float>(ny, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(xd, x, nx * 4, hipMemcpyHostToDevice, h->stream));
        launch_to_x6(xd, Cin, 0, Cin, N, HW, x6, cg, 0, ips, h->stream);
        X6Args a{};
        a.ks = ks; a.pad = pad;
        a.cin_g = cg; a.small = c->small6 ? 1 : 0; a.nK = c->nK6; a.Mpad = c->Mpad;
        X6Group& G = a.g[0];
        G.N = N; G.H = H; G.W = W; G.npix = N * HW;
        G.in = x6; G.in_ps = ips; G.in_l = x6act(x6, cg, 0, N, H, W).l;
        G.wt = c->wx6; G.bias = c->bias; G.cout = Cout; G.relu = relu; G.out2 = nullptr;
        if (out_x6) { G.out = y6; G.out_ps = ops; G.out_l = x6act(y6, og, 0, N, H, W).l; G.out_f32 = 0; }
        else { G.out = yd; G.out_c = Cout; G.out_off = 0; G.out_f32 = 1; }
        a.ngroups = 1;
        const TileChoice t = debug_x6_plan(h, a, mt, pt, splits);
        launch_conv_x6(a, t.mt, t.pt, h->stream);
        if (out_x6) launch_from_x6(y6, og, 0, ops, Cout, N, HW, yd, Cout, 0, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(out, yd, ny * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->convs[0].erase("__debug__");
    });
    return OPOSE_OK;
}

// the hooks' layers, gone from the handle when the hook returns or throws
struct DebugConvs {
    opose_ctx* h;
    int net;
    std::vector<std::string> keys;
    DevConv* add(const std::string& key, const Spec& s, const float* w, const float* b, int lvl, bool pair) {
        upload_conv(h, net, key, {&s}, {w}, {b}, lvl, pair);
        keys.push_back(key);
        return h->convs[net][key].get();
    }
    ~DebugConvs() {
        for (const std::string& k : keys) h->convs[net].erase(k);
    }
};

constexpr int kDebugFill = 0xa5;  // every byte of an output allocation before the launch under test

// 16-byte units of the piece planes hy of an X6 activation `a` (all_groups groups allocated, og of
// them written from a's first) that no longer hold the fill pattern although no pixel of the
// N x H x W frames' slice lives there: pads, other groups
static int64_t clobbered_units(const uint16_t* hy, const XAct& a, int og, int N, int H, int W) {
    const size_t units = a.ps / 16;
    std::vector<uint8_t> written(units, 0);
    for (int n = 0; n < N; ++n)
        for (int g = 0; g < og; ++g)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) written[host_unit(a, n, g, y, x)] = 1;
    uint8_t fill[16];
    std::memset(fill, kDebugFill, 16);
    int64_t bad = 0;
    for (int pc = 0; pc < 3; ++pc)
        for (size_t u = 0; u < units; ++u)
            if (!written[u] && std::memcmp(hy + ((size_t)pc * units + u) * 8, fill, 16) != 0) ++bad;
    return bad;
}

// One run_conv_x6_segs call on 1 .. kX6Groups segments of one conv shape, each with its own frames
// (geom [nseg][6]: N, H, W, forced k slabs (0: the planner's), weight set, and where its output
// goes: the first channel of an fp32 buffer or the first group of an X6 buffer).
int opose_debug_conv_segs(opose_t* h, int nseg, const int* geom, const float* const* x, int nw, const float* const* w,
                          const float* const* b, int Cin, int Cout, int ks, int relu, int family, int pool,
                          int in_padded, int out_kind, int out_total, int dup, int net, int lvl, int pair,
                          float* const* out, float* const* out_dup, int* ran, int64_t* clobbered) {
    if (!h || !geom || !x || !w || !b || !out || !ran || !clobbered) return OPOSE_E_ARG;
    if (nseg < 1 || nseg > kX6Groups || nw < 1 || nw > 2 || Cin < 1 || Cout < 1) return OPOSE_E_ARG;
    if ((ks != 1 && ks != 3 && ks != 7) || family < -1 || family > kKernelWino || out_kind < 0 || out_kind > 2)
        return OPOSE_E_ARG;
    if ((net != OPOSE_NET_BODY && net != OPOSE_NET_HAND) || lvl < 0 || lvl > 3) return OPOSE_E_ARG;
    if (dup && (out_kind == 0 || pool || !out_dup)) return OPOSE_E_ARG;  // (the fp32 epilogue writes no duplicate)
    if (pool && out_kind == 0) return OPOSE_E_ARG;
    const int og = (Cout + 7) / 8;
    for (int i = 0; i < nseg; ++i) {
        const int* g = geom + 6 * i;
        if (!x[i] || !out[i] || (dup && !out_dup[i]) || g[0] < 1 || g[1] < 1 || g[2] < 1 || g[3] < 0) return OPOSE_E_ARG;
        if (g[4] < 0 || g[4] >= nw || !w[g[4]] || !b[g[4]]) return OPOSE_E_ARG;
        if (g[5] < 0 || g[5] + (out_kind == 0 ? Cout : og) > out_total) return OPOSE_E_ARG;
        if (pool && (g[1] < 2 || g[2] < 2)) return OPOSE_E_ARG;
    }
    OPOSE_TRY(h, {
        enter_main(h);
        Spec s{"debug", Cin, Cout, ks, ks / 2};
        DebugConvs convs{h, net, {}};
        DevConv* cs[2] = {nullptr, nullptr};
        for (int k = 0; k < nw; ++k) cs[k] = convs.add("__debug" + std::to_string(k) + "__", s, w[k], b[k], lvl, pair != 0);
        const int cg = cs[0]->cin_g;
        // a forced family runs only shapes its launcher takes
        for (int i = 0; i < nseg; ++i) {
            const int* g = geom + 6 * i;
            const bool win = family == kKernelWin || family == kKernelWinFrames;
            if (win && (!cs[0]->wx6p || !in_padded || pool || !conv_win_fits(family == kKernelWin ? g[0] : 1, g[1], g[2], ks)))
                return OPOSE_E_ARG;
            if (family == kKernelWino && (!cs[0]->wwino || !in_padded || pool || g[3] > 1 || wino_tpf(g[0], g[1], g[2]) < 0))
                return OPOSE_E_ARG;
        }
        struct SegBufs {
            DevBuf in, out, dup;
            XAct oa, da;
            size_t obytes = 0;
            int Ho = 0, Wo = 0;
        };
        std::vector<SegBufs> bs(nseg);
        std::vector<ConvSeg> segs;
        std::vector<uint16_t> hx;
        for (int i = 0; i < nseg; ++i) {
            const int* g = geom + 6 * i;
            const int N = g[0], H = g[1], W = g[2];
            SegBufs& B = bs[i];
            B.Ho = pool ? H / 2 : H;
            B.Wo = pool ? W / 2 : W;
            XAct ia = in_padded ? x6pact(nullptr, cg, 0, N, H, W) : x6act(nullptr, cg, 0, N, H, W);
            hx.assign((size_t)3 * (ia.ps / 2), 0);  // input pads are zero, as in the product
            host_split_x6(x[i], N, Cin, H, W, ia, hx.data());
            ia.p = B.in.ensure<uint8_t>(hx.size() * 2, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(ia.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // (hx is reused)
            auto xout = [&](DevBuf& buf) {
                XAct a = out_kind == 2 ? x6pact(nullptr, out_total, g[5], N, B.Ho, B.Wo)
                                       : x6act(nullptr, out_total, g[5], N, B.Ho, B.Wo);
                a.p = buf.ensure<uint8_t>((size_t)3 * a.ps, h->stream);
                OPOSE_HIP_CHECK(hipMemsetAsync(a.p, kDebugFill, (size_t)3 * a.ps, h->stream));
                return a;
            };
            if (out_kind == 0) {
                B.obytes = (size_t)N * out_total * H * W * 4;
                B.oa = XAct{};
                B.oa.p = B.out.ensure<uint8_t>(B.obytes, h->stream);
                B.oa.c = out_total;
                B.oa.off = g[5];
                B.oa.f32 = true;
                OPOSE_HIP_CHECK(hipMemsetAsync(B.oa.p, kDebugFill, B.obytes, h->stream));
            } else {
                B.oa = xout(B.out);
                B.obytes = (size_t)3 * B.oa.ps;
            }
            if (dup) B.da = xout(B.dup);
            ConvSeg sg{cs[g[4]], N, H, W, ia, B.oa, dup ? B.da : XAct{}, relu != 0};
            sg.slabs = g[3];
            segs.push_back(sg);
        }
        {
            Redirect<int> forced(h->force_kernel, family);  // (-1: the planner's choice)
            // What run_conv_x6_segs makes of each segment.  The launch leaves no record of it, so this
            // repeats the first lines of that function's loop (seg_kernel, then a forced count or
            // slab_count on the segment's N, H, W; the hook's segments carry no Hl): keep the two alike.
            // A forced count comes back as given -- that it ran shows in the sums (one-hot sets with
            // a term in each slab, the fixup mutation), not here.
            for (int i = 0; i < nseg; ++i) {
                const ConvSeg& sg = segs[i];
                const int kind = seg_kernel(h, sg, pool != 0);
                ran[2 * i] = kind;
                ran[2 * i + 1] = kind == kKernelWino ? 1
                                 : sg.slabs        ? sg.slabs
                                                   : slab_count(h, sg.c, kind != kKernelX6, sg.N, sg.H, sg.W, pool != 0);
            }
            run_conv_x6_segs(h, segs, pool != 0);
        }
        int64_t bad = 0;
        std::vector<uint8_t> hy;
        for (int i = 0; i < nseg; ++i) {
            const int* g = geom + 6 * i;
            const int N = g[0];
            SegBufs& B = bs[i];
            hy.resize(B.obytes);
            OPOSE_HIP_CHECK(hipMemcpyAsync(hy.data(), B.oa.p, B.obytes, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            if (out_kind == 0) {
                const size_t HW = (size_t)B.Ho * B.Wo;
                const float* y = reinterpret_cast<const float*>(hy.data());
                float fill;
                std::memset(&fill, kDebugFill, 4);
                for (int n = 0; n < N; ++n)
                    for (int ch = 0; ch < out_total; ++ch) {
                        const float* src = y + ((size_t)n * out_total + ch) * HW;
                        if (ch >= g[5] && ch < g[5] + Cout)
                            std::memcpy(out[i] + ((size_t)n * Cout + ch - g[5]) * HW, src, HW * 4);
                        else
                            for (size_t p = 0; p < HW; ++p) bad += std::memcmp(src + p, &fill, 4) != 0;
                    }
                continue;
            }
            const uint16_t* y = reinterpret_cast<const uint16_t*>(hy.data());
            host_join_x6(y, B.oa, N, Cout, B.Ho, B.Wo, out[i]);
            bad += clobbered_units(y, B.oa, og, N, B.Ho, B.Wo);
            if (dup) {
                OPOSE_HIP_CHECK(hipMemcpyAsync(hy.data(), B.da.p, B.obytes, hipMemcpyDeviceToHost, h->stream));
                OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
                host_join_x6(y, B.da, N, Cout, B.Ho, B.Wo, out_dup[i]);
                bad += clobbered_units(y, B.da, og, N, B.Ho, B.Wo);
            }
        }
        *clobbered = bad;
    });
    return OPOSE_OK;
}

// conv1x1_chain_x6 on one or two segments (geom [nseg][4]: N, H, W, weight set) of 128-channel
// inputs: Y = W2 relu(W1 X + b1) + b2, W1 [m1][128], W2 [cout2][m1]
int opose_debug_chain(opose_t* h, int nseg, const int* geom, const float* const* x, int nw, const float* const* w1,
                      const float* const* b1, const float* const* w2, const float* const* b2, int m1, int cout2,
                      int relu2, int in_padded, int out_x6, float* const* out) {
    if (!h || !geom || !x || !w1 || !b1 || !w2 || !b2 || !out) return OPOSE_E_ARG;
    if (nseg < 1 || nseg > 2 || nw < 1 || nw > 2 || (m1 != 128 && m1 != 512) || cout2 < 1 || cout2 > 64) return OPOSE_E_ARG;
    for (int i = 0; i < nseg; ++i) {
        const int* g = geom + 4 * i;
        if (!x[i] || !out[i] || g[0] < 1 || g[1] < 1 || g[2] < 1 || g[3] < 0 || g[3] >= nw) return OPOSE_E_ARG;
        if (!w1[g[3]] || !b1[g[3]] || !w2[g[3]] || !b2[g[3]]) return OPOSE_E_ARG;
    }
    OPOSE_TRY(h, {
        enter_main(h);
        constexpr int Cin = 128;
        Spec s1{"debug1", Cin, m1, 1, 0}, s2{"debug2", m1, cout2, 1, 0};
        DebugConvs convs{h, 0, {}};
        DevConv *c1[2] = {}, *c2[2] = {};
        for (int k = 0; k < nw; ++k) {
            c1[k] = convs.add("__debug1_" + std::to_string(k) + "__", s1, w1[k], b1[k], 3, nseg == 2);
            c2[k] = convs.add("__debug2_" + std::to_string(k) + "__", s2, w2[k], b2[k], 3, nseg == 2);
            // (what run_chain_x6 asks of a pair before it fuses it)
            if (c1[k]->cin_g != 16 || c1[k]->cout != c1[k]->Mpad || c2[k]->Mpad != 64 || c2[k]->nK6 != m1 / 32 || c1[k]->small6)
                return OPOSE_E_ARG;
        }
        const int og = (cout2 + 7) / 8;
        struct SegBufs {
            DevBuf in, out;
            XAct oa;
            size_t obytes = 0;
        };
        std::vector<SegBufs> bs(nseg);
        std::vector<ChainSeg> segs;
        std::vector<uint16_t> hx;
        for (int i = 0; i < nseg; ++i) {
            const int* g = geom + 4 * i;
            const int N = g[0], H = g[1], W = g[2];
            SegBufs& B = bs[i];
            XAct ia = in_padded ? x6pact(nullptr, 16, 0, N, H, W) : x6act(nullptr, 16, 0, N, H, W);
            hx.assign((size_t)3 * (ia.ps / 2), 0);
            host_split_x6(x[i], N, Cin, H, W, ia, hx.data());
            ia.p = B.in.ensure<uint8_t>(hx.size() * 2, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(ia.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            if (out_x6) {
                B.oa = x6pact(nullptr, og, 0, N, H, W);
                B.obytes = (size_t)3 * B.oa.ps;
            } else {
                B.oa = XAct{};
                B.oa.c = cout2;
                B.oa.f32 = true;
                B.obytes = (size_t)N * cout2 * H * W * 4;
            }
            B.oa.p = B.out.ensure<uint8_t>(B.obytes, h->stream);
            OPOSE_HIP_CHECK(hipMemsetAsync(B.oa.p, 0, B.obytes, h->stream));
            segs.push_back(ChainSeg{c1[g[3]], c2[g[3]], N, H, W, ia, XAct{}, B.oa, relu2 != 0});
        }
        launch_chain_segs(h, segs);
        std::vector<uint8_t> hy;
        for (int i = 0; i < nseg; ++i) {
            const int* g = geom + 4 * i;
            SegBufs& B = bs[i];
            hy.resize(B.obytes);
            void* dst = out_x6 ? static_cast<void*>(hy.data()) : static_cast<void*>(out[i]);
            OPOSE_HIP_CHECK(hipMemcpyAsync(dst, B.oa.p, B.obytes, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            if (out_x6) host_join_x6(reinterpret_cast<const uint16_t*>(hy.data()), B.oa, g[0], cout2, g[1], g[2], out[i]);
        }
    });
    return OPOSE_OK;
}

// The first two layers' own kernels on 1 .. kConv1Segs segments (geom [nseg][3]: N, H, W) in one
// launch.  stage 1: conv1_1 (conv_first_x6; x [N,3,H,W], w [64,3,3,3]) -> out [N,64,H,W], f32: its
// output as fp32 units, else X6.  stage 2: conv1_2 + pool (conv3_pool_win_x6; x [N,64,H,W],
// w [64,64,3,3]) -> out [N,64,H/2,W/2], f32: its input as fp32 units, else X6.  Both add the bias
// and apply ReLU, as in the networks.
int opose_debug_conv1(opose_t* h, int stage, int nseg, const int* geom, const float* const* x, const float* w,
                      const float* b, int f32, float* const* out) {
    if (!h || !geom || !x || !w || !b || !out || (stage != 1 && stage != 2) || nseg < 1 || nseg > kConv1Segs)
        return OPOSE_E_ARG;
    for (int i = 0; i < nseg; ++i) {
        const int* g = geom + 3 * i;
        if (!x[i] || !out[i] || g[0] < 1 || g[1] < stage || g[2] < stage) return OPOSE_E_ARG;
    }
    OPOSE_TRY(h, {
        enter_main(h);
        const int Cin = stage == 1 ? 3 : 64;
        Spec s{"debug", Cin, 64, 3, 1};
        DebugConvs convs{h, 0, {}};
        DevConv* c = convs.add("__debug__", s, w, b, 0, false);
        // (what run_trunk_x6 asks of conv1_2 before it runs the window kernel)
        if (stage == 2 && (c->Mpad != 64 || c->nK6 != 18 || c->small6)) return OPOSE_E_ARG;
        struct SegBufs {
            DevBuf in, out;
            XAct oa;
            size_t obytes = 0;
        };
        std::vector<SegBufs> bs(nseg);
        Conv1Segs S{};
        S.n = nseg;
        std::vector<uint16_t> hx;
        std::vector<float> hf;
        for (int i = 0; i < nseg; ++i) {
            const int* g = geom + 3 * i;
            const int N = g[0], H = g[1], W = g[2], HW = H * W;
            const int Ho = stage == 1 ? H : H / 2, Wo = stage == 1 ? W : W / 2;
            SegBufs& B = bs[i];
            const void* in;
            uint32_t ips = 0;
            if (stage == 1) {
                float* xd = B.in.ensure<float>((size_t)N * 3 * HW, h->stream);
                OPOSE_HIP_CHECK(hipMemcpyAsync(xd, x[i], (size_t)N * 3 * HW * 4, hipMemcpyHostToDevice, h->stream));
                in = xd;
            } else if (f32) {  // fp32 units [N][8][H*W] of 8 channels
                hf.resize((size_t)N * 64 * HW);
                for (int n = 0; n < N; ++n)
                    for (int ch = 0; ch < 64; ++ch)
                        for (int p = 0; p < HW; ++p)
                            hf[(((size_t)n * 8 + ch / 8) * HW + p) * 8 + ch % 8] = x[i][((size_t)n * 64 + ch) * HW + p];
                float* xd = B.in.ensure<float>(hf.size(), h->stream);
                OPOSE_HIP_CHECK(hipMemcpyAsync(xd, hf.data(), hf.size() * 4, hipMemcpyHostToDevice, h->stream));
                in = xd;
            } else {
                XAct ia = x6act(nullptr, 8, 0, N, H, W);
                hx.assign((size_t)3 * (ia.ps / 2), 0);
                host_split_x6(x[i], N, 64, H, W, ia, hx.data());
                uint8_t* xd = B.in.ensure<uint8_t>(hx.size() * 2, h->stream);
                OPOSE_HIP_CHECK(hipMemcpyAsync(xd, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, h->stream));
                in = xd;
                ips = ia.ps;
            }
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // (hx / hf are reused)
            B.oa = x6act(nullptr, 8, 0, N, Ho, Wo);
            B.obytes = stage == 1 && f32 ? (size_t)N * 64 * HW * 4 : (size_t)3 * B.oa.ps;
            B.oa.p = B.out.ensure<uint8_t>(B.obytes, h->stream);
            OPOSE_HIP_CHECK(hipMemsetAsync(B.oa.p, 0, B.obytes, h->stream));
            S.s[i] = Conv1Seg{in, static_cast<uint8_t*>(B.oa.p), ips, B.oa.ps, N, H, W, 0};
        }
        if (stage == 1) launch_conv_first_x6_segs(S, c->wt, c->Mpad, c->bias, f32 != 0, h->stream);
        else launch_conv3_pool_win_x6_segs(S, c->wx6, c->bias, f32 != 0, h->stream);
        std::vector<uint8_t> hy;
        for (int i = 0; i < nseg; ++i) {
            const int* g = geom + 3 * i;
            const int N = g[0], Ho = stage == 1 ? g[1] : g[1] / 2, Wo = stage == 1 ? g[2] : g[2] / 2, HWo = Ho * Wo;
            SegBufs& B = bs[i];
            hy.resize(B.obytes);
            OPOSE_HIP_CHECK(hipMemcpyAsync(hy.data(), B.oa.p, B.obytes, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            if (stage == 1 && f32) {
                const float* y = reinterpret_cast<const float*>(hy.data());
                for (int n = 0; n < N; ++n)
                    for (int ch = 0; ch < 64; ++ch)
                        for (int p = 0; p < HWo; ++p)
                            out[i][((size_t)n * 64 + ch) * HWo + p] = y[(((size_t)n * 8 + ch / 8) * HWo + p) * 8 + ch % 8];
            } else {
                host_join_x6(reinterpret_cast<const uint16_t*>(hy.data()), B.oa, N, 64, Ho, Wo, out[i]);
            }
        }
    });
    return OPOSE_OK;
}

// timing of one split-bf16 conv launch configuration on hashed data
int opose_debug_conv_x6_time(opose_t* h, int N, int Cin, int H, int W, int Cout, int ks, int ngroups, int mt, int pt,
                             int splits, int reps, float* ms) {
    if (!h || !ms || reps < 1 || ngroups < 1 || ngroups > 2) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        Spec s{"timing", Cin, Cout, ks, ks / 2};
        std::vector<float> w((size_t)Cout * Cin * ks * ks), b(Cout, 0.f);
        for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((i * 2654435761u) % 2001) / 1000.f - 1.f;
        upload_conv(h, 0, "__timing__", {&s}, {w.data()}, {b.data()}, 3, false);
        DevConv* c = h->convs[0]["__timing__"].get();
        const int HW = H * W;
        const int cg = c->cin_g, og = (Cout + 7) / 8;
        const uint32_t ips = (uint32_t)((size_t)ngroups * N * cg * HW * 16);
        const uint32_t ops = (uint32_t)((size_t)ngroups * N * og * HW * 16);
        DevBuf xin, xx, yx;
        float* xd = xin.ensure<float>((size_t)ngroups * N * cg * 8 * HW, h->stream);
        launch_fill_hash(xd, (size_t)ngroups * N * cg * 8 * HW, 0x80000003u, h->stream);
        uint8_t* x6 = xx.ensure<uint8_t>((size_t)ips * 3, h->stream);
        uint8_t* y6 = yx.ensure<uint8_t>((size_t)ops * 3, h->stream);
        launch_to_x6(xd, cg * 8, 0, cg * 8, ngroups * N, HW, x6, cg, 0, ips, h->stream);
        X6Args a{};
        a.ks = ks; a.pad = ks / 2;
        a.cin_g = cg; a.small = c->small6 ? 1 : 0; a.nK = c->nK6; a.Mpad = c->Mpad;
        for (int g = 0; g < ngroups; ++g) {
            X6Group& G = a.g[g];
            const int gg = g;
            G.N = N; G.H = H; G.W = W; G.npix = N * HW;
            G.in = x6 + (size_t)gg * N * cg * HW * 16; G.in_ps = ips; G.in_l = x6act(x6, cg, 0, N, H, W).l;
            G.wt = c->wx6; G.bias = c->bias; G.cout = Cout; G.relu = 1; G.out2 = nullptr;
            G.out = y6 + (size_t)gg * N * og * HW * 16; G.out_ps = ops; G.out_l = x6act(y6, og, 0, N, H, W).l;
            G.out_f32 = 0;
        }
        a.ngroups = ngroups;
        const TileChoice t = debug_x6_plan(h, a, mt, pt, splits);
        launch_conv_x6(a, t.mt, t.pt, h->stream);  // warm-up
        hipEvent_t e0, e1;
        OPOSE_HIP_CHECK(hipEventCreate(&e0));
        OPOSE_HIP_CHECK(hipEventCreate(&e1));
        OPOSE_HIP_CHECK(hipEventRecord(e0, h->stream));
        for (int r = 0; r < reps; ++r) launch_conv_x6(a, t.mt, t.pt, h->stream);
        OPOSE_HIP_CHECK(hipEventRecord(e1, h->stream));
        OPOSE_HIP_CHECK(hipEventSynchronize(e1));
        OPOSE_HIP_CHECK(hipEventElapsedTime(ms, e0, e1));
        *ms /= reps;
        OPOSE_HIP_CHECK(hipEventDestroy(e0));
        OPOSE_HIP_CHECK(hipEventDestroy(e1));
        h->convs[0].erase("__timing__");
    });
    return OPOSE_OK;
}

// timing of one conv launch configuration on hashed data (ablate: see ConvArgs::ablate)
int opose_debug_conv_time(opose_t* h, int N, int Cin, int H, int W, int Cout, int ks, int ngroups, int mt, int pt,
                          int splits, int ablate, int reps, float* ms) {
    if (!h || !ms || reps < 1 || ngroups < 1 || ngroups > 2) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        Spec s{"timing", Cin, Cout, ks, ks / 2};
        std::vector<float> w((size_t)Cout * Cin * ks * ks, 0.01f), b(Cout, 0.f);
        upload_conv(h, 0, "__timing__", {&s}, {w.data()}, {b.data()}, 3, false);
        DevConv* c = h->convs[0]["__timing__"].get();
        launch_fill_hash(c->wt, (size_t)c->Kpad * c->Mpad, 7, h->stream);
        DevBuf xin, yout;
        const size_t nx = (size_t)ngroups * N * Cin * H * W, ny = (size_t)ngroups * N * Cout * H * W;
        float* xd = xin.ensure<float>(nx, h->stream);
        float* yd = yout.ensure<float>(ny, h->stream);
        launch_fill_hash(xd, nx, 3u, h->stream);
        ConvArgs a{};
        a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ks = ks; a.pad = ks / 2;
        a.K = c->K; a.Kpad = c->Kpad; a.Mpad = c->Mpad; a.npix = N * H * W;
        a.tap_major = c->tap_major ? 1 : 0;
        for (int g = 0; g < 2; ++g) {
            ConvGroup& G = a.g[g];
            const int gg = g < ngroups ? g : 0;
            G.in = xd + (size_t)gg * N * Cin * H * W; G.in_cstride = Cin; G.in_coff = 0; G.wt = c->wt; G.bias = c->bias;
            G.out = yd + (size_t)gg * N * Cout * H * W; G.out_cstride = Cout; G.out_coff = 0; G.out2 = nullptr;
            G.cout = Cout; G.relu = 1;
        }
        TileChoice t = choose_tile(a.Mpad, std::vector<int>(ngroups, a.npix), a.Kpad / 32);
        if (mt > 0) { t.mt = mt; t.pt = pt; t.grid = (a.Mpad / mt) * ((a.npix + pt - 1) / pt) * ngroups; }
        if (splits > 0) t.grid = splits;
        if (a.Mpad % t.mt) throw std::invalid_argument("tile M does not divide Mpad");
        a.ngroups = ngroups;
        a.sk_grid = t.grid;
        a.partial = h->w().partial.ensure<float>((size_t)2 * t.grid * t.mt * t.pt, h->stream);
        if (ablate) throw std::invalid_argument("timing ablations were removed");
        auto go = [&]() { launch_conv(a, c->ktab, t.mt, t.pt, h->stream); };
        go();  // warm-up
        hipEvent_t e0, e1;
        OPOSE_HIP_CHECK(hipEventCreate(&e0));
        OPOSE_HIP_CHECK(hipEventCreate(&e1));
        OPOSE_HIP_CHECK(hipEventRecord(e0, h->stream));
        for (int r = 0; r < reps; ++r) go();
        OPOSE_HIP_CHECK(hipEventRecord(e1, h->stream));
        OPOSE_HIP_CHECK(hipEventSynchronize(e1));
        OPOSE_HIP_CHECK(hipEventElapsedTime(ms, e0, e1));
        *ms /= reps;
        OPOSE_HIP_CHECK(hipEventDestroy(e0));
        OPOSE_HIP_CHECK(hipEventDestroy(e1));
        h->convs[0].erase("__timing__");
    });
    return OPOSE_OK;
}

int opose_debug_preprocess(opose_t* h, const uint8_t* bgr, int H, int W, double scale, int pad_value, float* out,
                           int* HpWp) {
    if (!h || !bgr || !HpWp) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        opose_params p;
        opose_default_params(OPOSE_NET_BODY, &p);
        p.pad_value = pad_value;
        const ScaleGeom g = geom(scale, p, H, W);
        HpWp[0] = g.Hp;
        HpWp[1] = g.Wp;
        if (!out) return OPOSE_OK;
        DevBuf fin, xo;
        uint8_t* fd = fin.ensure<uint8_t>((size_t)H * W * 3, h->stream);
        float* xd = xo.ensure<float>((size_t)3 * g.Hp * g.Wp, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(fd, bgr, (size_t)H * W * 3, hipMemcpyHostToDevice, h->stream));
        preprocess_scale(fd, (int64_t)H * W * 3, (int64_t)W * 3, 1, H, W, g, p, xd, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(out, xd, (size_t)3 * g.Hp * g.Wp * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

int opose_debug_preprocess_groups(opose_t* h, int n_groups, const uint8_t* const* bgr, const int* N, const int* H,
                                  const int* W, double scale, int pad_value, float* const* out, int* HpWp) {
    if (!h || !bgr || !N || !H || !W || !HpWp || n_groups < 1 || n_groups > OPOSE_MAX_SCALES) return OPOSE_E_ARG;
    for (int g = 0; g < n_groups; ++g)
        if (!bgr[g] || N[g] <= 0 || H[g] <= 0 || W[g] <= 0) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        opose_params p;
        opose_default_params(OPOSE_NET_BODY, &p);
        p.pad_value = pad_value;
        std::vector<ScaleGeom> gs;
        bool run = out != nullptr;
        for (int g = 0; g < n_groups; ++g) {
            gs.push_back(geom(scale, p, H[g], W[g]));
            HpWp[2 * g] = gs[g].Hp;
            HpWp[2 * g + 1] = gs[g].Wp;
            run = run && out[g];
        }
        if (!run) return OPOSE_OK;
        std::vector<DevBuf> fin(n_groups), xo(n_groups);
        PrepTable table{};
        for (int g = 0; g < n_groups; ++g) {
            const size_t fb = (size_t)H[g] * W[g] * 3;
            uint8_t* fd = fin[g].ensure<uint8_t>(fb * N[g], h->stream);
            float* xd = xo[g].ensure<float>((size_t)N[g] * 3 * gs[g].Hp * gs[g].Wp, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(fd, bgr[g], fb * N[g], hipMemcpyHostToDevice, h->stream));
            table.s[g] = prep_seg(fd, (int64_t)fb, (int64_t)W[g] * 3, N[g], H[g], W[g], gs[g], xd);
        }
        preprocess_segs(h, table, n_groups, p);
        for (int g = 0; g < n_groups; ++g)
            OPOSE_HIP_CHECK(hipMemcpyAsync(out[g], table.s[g].out, (size_t)N[g] * 3 * gs[g].Hp * gs[g].Wp * 4,
                                           hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}

// maps [57][hl][wl] -> heat_avg [18][H][W] (float64) and PAF x8 map [38][Hs][Ws] (float32)
int opose_debug_heat(opose_t* h, const float* maps, int hl, int wl, int pad_down, int pad_right, int H, int W,
                     double* heat_avg, float* paf_mid) {
    if (!h || !maps || !heat_avg) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf min_;
        float* md = min_.ensure<float>((size_t)57 * hl * wl, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(md, maps, (size_t)57 * hl * wl * 4, hipMemcpyHostToDevice, h->stream));
        const ScaleGeom g = geom_from_pads(hl, wl, pad_down, pad_right, H, W);
        upsample_to_mid(h, 0, md, 57, 1, g, 56);
        double* avg = h->avg.ensure<double>((size_t)18 * H * W, h->stream);
        launch_heat_full(h->mid(0).ensure<float>(0, h->stream), 56, 38, 18, 1, g.Hs, g.Ws, H, W, g.up_sy, g.up_sx, 1, 0,
                         avg, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(heat_avg, avg, (size_t)18 * H * W * 8, hipMemcpyDeviceToHost, h->stream));
        if (paf_mid)
            OPOSE_HIP_CHECK(hipMemcpyAsync(paf_mid, h->mid(0).ensure<float>(0, h->stream),
                                           (size_t)38 * g.Hs * g.Ws * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

int opose_debug_hand_label(opose_t* h, const double* maps, int NP, int H, int W, double thre, int32_t* labels,
                           double* sums) {
    if (!h || !maps || !labels || !sums || NP <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const size_t n = (size_t)NP * H * W;
        DevBuf mb, lb, sb, cb, pk, fd, ws;
        double* md = mb.ensure<double>(n, h->stream);
        int* lab = lb.ensure<int>(n, h->stream);
        double* sd = sb.ensure<double>(n, h->stream);
        int* cnt = cb.ensure<int>((size_t)NP, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(md, maps, n * 8, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * NP, h->stream));
        launch_gauss_threshold(md, NP, H, W, thre, lab, cnt, sd, h->stream);
        launch_hand_cc(md, NP, H, W, lab, sd, cnt, pk.ensure<double>((size_t)NP * 3, h->stream),
                       fd.ensure<int>((size_t)NP, h->stream), ws.ensure<uint8_t>(hand_cc_workspace_bytes(NP), h->stream),
                       true, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(labels, lab, n * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(sums, sd, n * 8, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

int opose_debug_batch_preprocess(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                                 int64_t frame_stride, double boxsize, double scale, float* out, int* HpWp) {
    if (!h || !bgr || !HpWp || N <= 0 || H <= 0 || W <= 0 || boxsize <= 0 || scale <= 0) return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        opose_params p;
        opose_default_params(OPOSE_NET_BODY, &p);
        p.boxsize = boxsize;
        p.n_scales = 1;
        p.scales[0] = scale;
        const BatchGeom g = batch_geom(p, H, W);
        HpWp[0] = g.Hp;
        HpWp[1] = g.Wp;
        if (!out) return OPOSE_OK;
        DevBuf xo;
        const size_t nx = (size_t)N * 3 * g.Hp * g.Wp;
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, 0);
        float* xd = xo.ensure<float>(nx, h->stream);
        batch_preprocess(fd, frame_stride, row_stride, N, H, W, g, xd, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(out, xd, nx * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

int opose_debug_batch_heat(opose_t* h, const float* maps, int N, int hl, int wl, int nh, int nw, int H, int W,
                           float* heat, float* mid) {
    if (!h || !maps || !heat || N <= 0 || hl <= 0 || wl <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    if (nh <= 0 || nw <= 0 || nh > 8 * hl || nw > 8 * wl) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf min_, mb, hb;
        const size_t nm = (size_t)N * 57 * hl * wl, nmid = (size_t)N * 56 * nh * nw, nheat = (size_t)N * 18 * H * W;
        float* md = min_.ensure<float>(nm, h->stream);
        float* midd = mb.ensure<float>(nmid, h->stream);
        float* hd = hb.ensure<float>(nheat, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(md, maps, nm * 4, hipMemcpyHostToDevice, h->stream));
        batch_resize_chain(h, N, H, W, md, 57, hl, wl, nh, nw, midd, hd);
        OPOSE_HIP_CHECK(hipMemcpyAsync(heat, hd, nheat * 4, hipMemcpyDeviceToHost, h->stream));
        if (mid) OPOSE_HIP_CHECK(hipMemcpyAsync(mid, midd, nmid * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_debug_blur5_nms(opose_t* h, const float* heat, int NP, int H, int W, double thre, int cap, int32_t* cnt,
                          int32_t* list, double* score) {
    if (!h || !heat || !cnt || !list || !score || NP <= 0 || H <= 0 || W <= 0 || cap <= 0) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf hb, cb, lb, sb;
        const size_t n = (size_t)NP * H * W, nl = (size_t)NP * cap;
        float* hd = hb.ensure<float>(n, h->stream);
        int* cd = cb.ensure<int>((size_t)NP, h->stream);
        int* ld = lb.ensure<int>(nl, h->stream);
        double* sd = sb.ensure<double>(nl, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(hd, heat, n * 4, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(cd, 0, sizeof(int) * NP, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(ld, 0xff, sizeof(int) * nl, h->stream));  // unused slots: -1
        OPOSE_HIP_CHECK(hipMemsetAsync(sd, 0, sizeof(double) * nl, h->stream));
        launch_blur5_nms(hd, NP, H, W, thre, cap, cd, ld, sd, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(cnt, cd, sizeof(int) * NP, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(list, ld, sizeof(int) * nl, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(score, sd, sizeof(double) * nl, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

int opose_debug_batch_hand_label(opose_t* h, const float* heat, int NP, int H, int W, double thre, double* blurred,
                                 int32_t* labels, double* sums) {
    if (!h || !heat || !blurred || !labels || !sums || NP <= 0 || H <= 0 || W <= 0) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const size_t n = (size_t)NP * H * W;
        DevBuf hb, bb, lb, sb, cb, pk, fd, ws;
        float* hd = hb.ensure<float>(n, h->stream);
        double* bd = bb.ensure<double>(n, h->stream);
        int* lab = lb.ensure<int>(n, h->stream);
        double* sd = sb.ensure<double>(n, h->stream);
        int* cnt = cb.ensure<int>((size_t)NP, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(hd, heat, n * 4, hipMemcpyHostToDevice, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * NP, h->stream));
        launch_blur5_seed(hd, NP, H, W, thre, bd, lab, cnt, h->stream);
        launch_hand_cc(bd, NP, H, W, lab, sd, cnt, pk.ensure<double>((size_t)NP * 3, h->stream),
                       fd.ensure<int>((size_t)NP, h->stream), ws.ensure<uint8_t>(hand_cc_workspace_bytes(NP), h->stream),
                       false, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(blurred, bd, n * 8, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(labels, lab, n * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipMemcpyAsync(sums, sd, n * 8, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

// ---- the body matching kernels one at a time (tests/test_gpu_match_stages.py): each hook calls the
// launcher peaks_to_records calls, with its arguments, at the handle's capacity
static bool counts_ok(const int32_t* c, size_t n, int lo, int hi) {
    for (size_t i = 0; i < n; ++i)
        if (c[i] < lo || c[i] > hi) return false;
    return true;
}
// the first part_cnt positions of every part lie on the H x W map
static bool positions_ok(const int32_t* pos, const int32_t* pcnt, int N, int cap, int64_t HW) {
    for (int np = 0; np < N * 18; ++np)
        for (int i = 0; i < pcnt[np]; ++i) {
            const int32_t v = pos[(size_t)np * cap + i];
            if (v < 0 || v >= HW) return false;
        }
    return true;
}
template <class T>
static T* to_device(opose_ctx* h, DevBuf& b, const T* src, size_t n) {
    T* d = b.ensure<T>(n, h->stream);
    OPOSE_HIP_CHECK(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return d;
}
template <class T>
static void to_host(opose_ctx* h, T* dst, const T* src, size_t n) {
    OPOSE_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
}

int opose_debug_peaks_finalize(opose_t* h, const int32_t* cnt, const int32_t* list, const double* score, int N, int H,
                               int W, void* records, int32_t* peak_pos, int32_t* part_cnt) {
    if (!h || !cnt || !list || !score || !records || !peak_pos || !part_cnt || N <= 0 || H <= 0 || W <= 0)
        return OPOSE_E_ARG;
    const int cap = h->ppp;
    const int64_t HW = (int64_t)H * W;
    if (HW > 0x7fffffff) return OPOSE_E_ARG;
    for (int np = 0; np < N * 18; ++np) {  // the raw count may pass the capacity: the list holds cap entries
        if (cnt[np] < 0) return OPOSE_E_ARG;
        for (int i = 0; i < std::min(cnt[np], cap); ++i)
            if (list[(size_t)np * cap + i] < 0 || list[(size_t)np * cap + i] >= HW) return OPOSE_E_ARG;
    }
    OPOSE_TRY(h, {
        enter_main(h);
        const RecordLayout L = make_record_layout(h->ppp, h->maxp);
        const size_t nl = (size_t)N * 18 * cap;
        DevBuf cb, lb, sb, rb, pb, qb;
        const int* cd = to_device(h, cb, cnt, (size_t)N * 18);
        const int* ld = to_device(h, lb, list, nl);
        const double* sd = to_device(h, sb, score, nl);
        uint8_t* rec = rb.ensure<uint8_t>(L.bytes * N, h->stream);
        int* pos = pb.ensure<int>(nl, h->stream);
        int* pcnt = qb.ensure<int>((size_t)N * 18, h->stream);
        OPOSE_HIP_CHECK(hipMemsetAsync(rec, 0, L.bytes * N, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(pos, 0xff, sizeof(int) * nl, h->stream));  // unused slots: -1
        launch_peaks_finalize(cd, ld, sd, N, H, W, L, rec, pos, pcnt, h->stream);
        to_host(h, static_cast<uint8_t*>(records), rec, L.bytes * N);
        to_host(h, peak_pos, pos, nl);
        to_host(h, part_cnt, pcnt, (size_t)N * 18);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

int opose_debug_paf_score(opose_t* h, int fast, int n_scales, const float* const* maps, const int* hl, const int* wl,
                          const int* ga, const int* gb, const int32_t* peak_pos, const int32_t* part_cnt, int N, int H,
                          int W, double thre2, double* score) {
    if (!h || !maps || !hl || !wl || !ga || !gb || !peak_pos || !part_cnt || !score || N <= 0 || H <= 0 || W <= 0)
        return OPOSE_E_ARG;
    if (n_scales < 1 || n_scales > (fast ? 1 : kMaxScales) || (int64_t)H * W > 0x7fffffff) return OPOSE_E_ARG;
    for (int s = 0; s < n_scales; ++s) {
        if (!maps[s] || hl[s] <= 0 || wl[s] <= 0) return OPOSE_E_ARG;
        if (fast ? (ga[s] <= 0 || gb[s] <= 0 || ga[s] > 8 * hl[s] || gb[s] > 8 * wl[s])
                 : (ga[s] < 0 || gb[s] < 0 || ga[s] >= 8 * hl[s] || gb[s] >= 8 * wl[s]))
            return OPOSE_E_ARG;
    }
    const int cap = h->ppp;
    if (!counts_ok(part_cnt, (size_t)N * 18, 0, cap) || !positions_ok(peak_pos, part_cnt, N, cap, (int64_t)H * W))
        return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf mb[kMaxScales], midb, heatb, pb, qb, sb;
        PafScales S{};
        if (fast) {
            const int nh = ga[0], nw = gb[0];
            const float* md = to_device(h, mb[0], maps[0], (size_t)N * 57 * hl[0] * wl[0]);
            float* mid = midb.ensure<float>((size_t)N * 56 * nh * nw, h->stream);
            float* heat = heatb.ensure<float>((size_t)N * 18 * H * W, h->stream);
            batch_resize_chain(h, N, H, W, md, 57, hl[0], wl[0], nh, nw, mid, heat);
            S = batch_paf_scales(mid, nh, nw, H, W);
        } else {
            std::vector<ScaleGeom> gs;
            for (int s = 0; s < n_scales; ++s) {
                const ScaleGeom g = geom_from_pads(hl[s], wl[s], ga[s], gb[s], H, W);
                body_to_mid(h, s, to_device(h, mb[s], maps[s], (size_t)N * 57 * hl[s] * wl[s]), 57, N, g);
                gs.push_back(g);
            }
            S = body_paf_scales(h, N, H, W, gs);
        }
        const size_t ns = (size_t)N * 19 * cap * cap;
        const int* pos = to_device(h, pb, peak_pos, (size_t)N * 18 * cap);
        const int* pcnt = to_device(h, qb, part_cnt, (size_t)N * 18);
        double* sc = sb.ensure<double>(ns, h->stream);
        OPOSE_HIP_CHECK(hipMemsetAsync(sc, 0xff, sizeof(double) * ns, h->stream));  // a NaN in every unwritten entry
        launch_paf_score(S, pos, pcnt, N, cap, thre2, sc, h->stream);
        to_host(h, score, sc, ns);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_debug_limb_greedy(opose_t* h, const double* score, const int32_t* part_cnt, int N, int32_t* conn_i,
                            int32_t* conn_j, double* conn_s, int32_t* conn_cnt) {
    if (!h || !score || !part_cnt || !conn_i || !conn_j || !conn_s || !conn_cnt || N <= 0) return OPOSE_E_ARG;
    const int cap = h->ppp;
    if (!counts_ok(part_cnt, (size_t)N * 18, 0, cap)) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const size_t nc = (size_t)N * 19 * cap;
        DevBuf sb, qb, cb, nb;
        const double* sc = to_device(h, sb, score, nc * cap);
        const int* pcnt = to_device(h, qb, part_cnt, (size_t)N * 18);
        Conn* conn = cb.ensure<Conn>(nc, h->stream);
        int* ccnt = nb.ensure<int>((size_t)N * 19, h->stream);
        OPOSE_HIP_CHECK(hipMemsetAsync(conn, 0xff, sizeof(Conn) * nc, h->stream));  // unused slots: -1, -1, NaN
        launch_limb_greedy(sc, pcnt, N, cap, conn, ccnt, h->stream);
        std::vector<Conn> hc(nc);
        to_host(h, hc.data(), conn, nc);
        to_host(h, conn_cnt, ccnt, (size_t)N * 19);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        for (size_t e = 0; e < nc; ++e) {
            conn_i[e] = hc[e].i;
            conn_j[e] = hc[e].j;
            conn_s[e] = hc[e].s;
        }
    });
    return OPOSE_OK;
}

int opose_debug_assemble(opose_t* h, void* records, const int32_t* part_cnt, const int32_t* conn_i,
                         const int32_t* conn_j, const double* conn_s, const int32_t* conn_cnt, int N, int* stage) {
    if (!h || !records || !part_cnt || !conn_i || !conn_j || !conn_s || !conn_cnt || !stage || N <= 0) return OPOSE_E_ARG;
    const int cap = h->ppp;
    if (!counts_ok(part_cnt, (size_t)N * 18, 0, cap) || !counts_ok(conn_cnt, (size_t)N * 19, -1, cap)) return OPOSE_E_ARG;
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < 19; ++k) {
            const int nA = part_cnt[n * 18 + kHostLimbA[k]], nB = part_cnt[n * 18 + kHostLimbB[k]];
            for (int c = 0; c < conn_cnt[n * 19 + k]; ++c) {  // (need not be a matching)
                const size_t e = ((size_t)n * 19 + k) * cap + c;
                if (conn_i[e] < 0 || conn_i[e] >= nA || conn_j[e] < 0 || conn_j[e] >= nB) return OPOSE_E_ARG;
            }
        }
    OPOSE_TRY(h, {
        enter_main(h);
        const RecordLayout L = make_record_layout(h->ppp, h->maxp);
        *stage = assemble_stage(L);
        const size_t nc = (size_t)N * 19 * cap;
        std::vector<Conn> hc(nc);
        for (size_t e = 0; e < nc; ++e) hc[e] = Conn{conn_i[e], conn_j[e], conn_s[e]};
        DevBuf rb, qb, cb, nb;
        uint8_t* rec = to_device(h, rb, static_cast<const uint8_t*>(records), L.bytes * N);
        const int* pcnt = to_device(h, qb, part_cnt, (size_t)N * 18);
        const Conn* conn = to_device(h, cb, hc.data(), nc);
        const int* ccnt = to_device(h, nb, conn_cnt, (size_t)N * 19);
        launch_assemble(conn, ccnt, pcnt, N, L, rec, h->stream);
        to_host(h, static_cast<uint8_t*>(records), rec, L.bytes * N);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

// ---- the exact mode's peak finder and heat average one launch at a time
// (tests/test_gpu_peak_stages.py), modelled on opose_debug_blur5_nms: own buffers, cnt zeroed,
// list preset to -1 and score to 0, one launch, copied back and synchronised
struct DebugPeaks {
    DevBuf cb, lb, sb;
    int NP;
    size_t nl;
    int *cnt, *list;
    double* score;
    DebugPeaks(opose_ctx* h, int NP_, int cap) : NP(NP_), nl((size_t)NP_ * cap) {
        cnt = cb.ensure<int>((size_t)NP + 1, h->stream);  // + gauss_nms_resize's hot-tile count
        list = lb.ensure<int>(nl, h->stream);
        score = sb.ensure<double>(nl, h->stream);
        OPOSE_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * ((size_t)NP + 1), h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(list, 0xff, sizeof(int) * nl, h->stream));  // unused slots: -1
        OPOSE_HIP_CHECK(hipMemsetAsync(score, 0, sizeof(double) * nl, h->stream));
    }
    void fetch(opose_ctx* h, int32_t* c, int32_t* l, double* s) {
        to_host(h, c, cnt, (size_t)NP);
        to_host(h, l, list, nl);
        to_host(h, s, score, nl);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
};

int opose_debug_gauss_nms(opose_t* h, const void* maps, int is_f32, int NP, int H, int W, double thre, int cap,
                          int32_t* cnt, int32_t* list, double* score) {
    if (!h || !maps || !cnt || !list || !score || NP <= 0 || H <= 0 || W <= 0 || cap <= 0) return OPOSE_E_ARG;
    if ((int64_t)H * W > 0x7fffffff) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf mb;
        const size_t bytes = (size_t)NP * H * W * (is_f32 ? 4 : 8);
        const uint8_t* md = to_device(h, mb, static_cast<const uint8_t*>(maps), bytes);
        DebugPeaks out(h, NP, cap);
        launch_gauss_nms(md, is_f32 != 0, NP, H, W, thre, cap, out.cnt, out.list, out.score, h->stream);
        out.fetch(h, cnt, list, score);
    });
    return OPOSE_OK;
}

// opose_debug_gauss_nms_resize / opose_debug_gauss_hot_tiles: the production launch pair on the
// handle's own hot-tile buffer; the hot count is the word after the peak counts, as in peak_ws
static int debug_gauss_resize(opose_t* h, const float* mid, int N, int Cm, int coff, int P, int Hs, int Ws, int H, int W,
                              double thre, int cap, int max_grid, int32_t* cnt, int32_t* list, double* score,
                              int32_t* hot_cnt, int32_t* hot_tiles) {
    if (!h || !mid || !cnt || !list || !score || N <= 0 || P <= 0 || coff < 0 || coff + P > Cm) return OPOSE_E_ARG;
    if (Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || cap <= 0 || (int64_t)H * W > 0x7fffffff) return OPOSE_E_ARG;
    const double sy = 1.0 / ((double)H / Hs), sx = 1.0 / ((double)W / Ws);  // as geom_from_pads
    if (!gauss_nms_resize_fits(Hs, Ws, H, W, sy)) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf mb;
        const float* md = to_device(h, mb, mid, (size_t)N * Cm * Hs * Ws);
        DebugPeaks out(h, N * P, cap);
        const size_t nt = (size_t)gauss_nms_resize_tiles(N, P, H, W);
        int* hot = h->hot_tiles.ensure<int>(nt, h->stream);
        if (hot_tiles) OPOSE_HIP_CHECK(hipMemsetAsync(hot, 0xff, sizeof(int) * nt, h->stream));  // unused slots: -1
        launch_gauss_nms_resize(md, Cm, coff, P, N, Hs, Ws, H, W, sy, sx, thre, cap, out.cnt, out.list, out.score,
                                out.cnt + out.NP, hot, max_grid, h->stream);
        if (hot_cnt) to_host(h, hot_cnt, out.cnt + out.NP, 1);
        if (hot_tiles) to_host(h, hot_tiles, hot, nt);
        out.fetch(h, cnt, list, score);
    });
    return OPOSE_OK;
}

int opose_debug_gauss_nms_resize(opose_t* h, const float* mid, int N, int Cm, int coff, int P, int Hs, int Ws, int H,
                                 int W, double thre, int cap, int32_t* cnt, int32_t* list, double* score) {
    return debug_gauss_resize(h, mid, N, Cm, coff, P, Hs, Ws, H, W, thre, cap, 0, cnt, list, score, nullptr, nullptr);
}

int opose_debug_gauss_hot_tiles(opose_t* h, const float* mid, int N, int Cm, int coff, int P, int Hs, int Ws, int H,
                                int W, double thre, int cap, int max_grid, int32_t* cnt, int32_t* list, double* score,
                                int32_t* hot_cnt, int32_t* hot_tiles) {
    if (!hot_cnt || !hot_tiles || max_grid < 0) return OPOSE_E_ARG;
    return debug_gauss_resize(h, mid, N, Cm, coff, P, Hs, Ws, H, W, thre, cap, max_grid, cnt, list, score, hot_cnt,
                              hot_tiles);
}

int opose_debug_heat_scales(opose_t* h, int n, const float* const* mids, const int* Hs, const int* Ws, int N, int Cm,
                            int coff, int C, int H, int W, int one_launch, double* avg) {
    constexpr int kMost = 16;  // scales of the per-scale form (the one-launch form: kHeatScales)
    if (!h || !mids || !Hs || !Ws || !avg || n < 1 || n > kMost || N <= 0 || C <= 0 || coff < 0 || coff + C > Cm)
        return OPOSE_E_ARG;
    if (H <= 0 || W <= 0) return OPOSE_E_ARG;
    for (int s = 0; s < n; ++s)
        if (!mids[s] || Hs[s] <= 0 || Ws[s] <= 0) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        DevBuf mb[kMost], ab;
        HeatScales S{};
        S.n = n;
        S.ns = (float)n;
        double sy[kMost], sx[kMost];
        for (int s = 0; s < n; ++s) {
            sy[s] = 1.0 / ((double)H / Hs[s]);  // as geom_from_pads
            sx[s] = 1.0 / ((double)W / Ws[s]);
            if (s < kHeatScales) S.s[s] = HeatScale{nullptr, Cm, coff, Hs[s], Ws[s], sy[s], sx[s]};
        }
        if (one_launch && !heat_full_scales_fits(S, H, W)) return OPOSE_E_ARG;
        const float* md[kMost];
        for (int s = 0; s < n; ++s) md[s] = to_device(h, mb[s], mids[s], (size_t)N * Cm * Hs[s] * Ws[s]);
        const size_t na = (size_t)N * C * H * W;
        double* ad = ab.ensure<double>(na, h->stream);
        OPOSE_HIP_CHECK(hipMemsetAsync(ad, kDebugFill, na * 8, h->stream));
        if (one_launch) {
            for (int s = 0; s < n; ++s) S.s[s].mid = md[s];
            launch_heat_full_scales(S, N, C, H, W, ad, h->stream);
        } else {
            for (int s = 0; s < n; ++s)
                launch_heat_full(md[s], Cm, coff, C, N, Hs[s], Ws[s], H, W, sy[s], sx[s], n, s > 0, ad, h->stream);
        }
        to_host(h, avg, ad, na);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

// ---- the hand extraction kernels one at a time (tests/test_gpu_hand_stages.py): the calls
// opose_batch_hand_extract makes, on host arrays.  (hand_boxes: opose_batch_hand_boxes.)
int opose_debug_hand_crops(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const int32_t* boxes, int boxsize, float* x, uint8_t* crops,
                           int32_t* status) {
    if (!h || !bgr || !boxes || !status || (!x && !crops) || H <= 0 || W <= 0 || !extract_batch_ok(N, boxsize))
        return OPOSE_E_ARG;
    if (row_stride < (int64_t)W * 3 || frame_stride < row_stride * H) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const size_t slots = (size_t)2 * N, nx = slots * 3 * boxsize * boxsize;
        DevBuf bb, xb, cb, sb;
        const uint8_t* fd = stage_frames(h, bgr, N, H, W, row_stride, frame_stride, 0);
        const int32_t* bd = to_device(h, bb, boxes, slots * 4);
        float* xd = x ? xb.ensure<float>(nx, h->stream) : nullptr;
        uint8_t* cd = crops ? cb.ensure<uint8_t>(nx, h->stream) : nullptr;
        int32_t* sd = sb.ensure<int32_t>(slots, h->stream);
        if (xd) OPOSE_HIP_CHECK(hipMemsetAsync(xd, kDebugFill, nx * 4, h->stream));
        if (cd) OPOSE_HIP_CHECK(hipMemsetAsync(cd, kDebugFill, nx, h->stream));
        OPOSE_HIP_CHECK(hipMemsetAsync(sd, kDebugFill, slots * 4, h->stream));
        run_hand_crops(h, fd, frame_stride, row_stride, N, H, W, bd, boxsize, xd, cd, sd);
        if (xd) to_host(h, x, xd, nx);
        if (cd) to_host(h, crops, cd, nx);
        to_host(h, status, sd, slots);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_debug_hand_backmap(opose_t* h, const double* peaks, const int32_t* found, const int32_t* boxes, int N,
                             int boxsize, double* handmat) {
    if (!h || !peaks || !found || !boxes || !handmat || !extract_batch_ok(N, boxsize)) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const size_t slots = (size_t)2 * N;
        DevBuf pb, fb, bb, hb;
        const double* pd = to_device(h, pb, peaks, slots * 63);
        const int32_t* fd = to_device(h, fb, found, slots * 21);
        const int32_t* bd = to_device(h, bb, boxes, slots * 4);
        double* hm = hb.ensure<double>((size_t)N * 126, h->stream);
        OPOSE_HIP_CHECK(hipMemsetAsync(hm, kDebugFill, (size_t)N * 126 * 8, h->stream));
        launch_hand_backmap(pd, fd, bd, N, boxsize, hm, h->stream);
        to_host(h, handmat, hm, (size_t)N * 126);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}

// ---- the drawing setup kernel alone (tests/test_gpu_draw.py), through the call the draw entry
// points make
int opose_debug_draw_prims(opose_t* h, const void* src, int N, int joints, int H, int W, int32_t* prims,
                           int32_t* counts, int32_t* status) {
    if (!h || !src || !prims || !counts || !status || !draw_dims_ok(N, H, W)) return OPOSE_E_ARG;
    if (joints != 0 && joints != 18 && joints != 60) return OPOSE_E_ARG;
    if (joints == 0 && reinterpret_cast<uintptr_t>(src) % 8) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        enter_main(h);
        const size_t slots = (size_t)N * draw_cap(h, joints) * kDrawPrimInts;
        DevBuf sb, pb, cb, tb;
        const uint8_t* rd = nullptr;
        const double* md = nullptr;
        if (joints == 0)
            rd = to_device(h, sb, static_cast<const uint8_t*>(src), make_record_layout(h->ppp, h->maxp).bytes * N);
        else
            md = to_device(h, sb, static_cast<const double*>(src), (size_t)N * joints * 3);
        int32_t* pd = pb.ensure<int32_t>(slots, h->stream);
        int32_t* cd = cb.ensure<int32_t>((size_t)N, h->stream);
        int32_t* td = tb.ensure<int32_t>((size_t)N, h->stream);
        OPOSE_HIP_CHECK(hipMemsetAsync(pd, 0, slots * 4, h->stream));  // slots past a frame's count stay zero
        run_draw_setup(h, rd, md, joints, N, H, W, pd, cd, td);
        to_host(h, prims, pd, slots);
        to_host(h, counts, cd, (size_t)N);
        to_host(h, status, td, (size_t)N);
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof_drain();
    });
    return OPOSE_OK;
}
