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
            const size_t plane = x6p_plane(N, H, W), P = (size_t)x6p_pitch(W);
            auto rne = [](float v) -> uint16_t {
                uint32_t u;
                std::memcpy(&u, &v, 4);
                u += 0x7fffu + ((u >> 16) & 1u);
                return (uint16_t)(u >> 16);
            };
            auto f16 = [](uint16_t hb) {
                const uint32_t u = (uint32_t)hb << 16;
                float v;
                std::memcpy(&v, &u, 4);
                return v;
            };
            std::vector<uint16_t> hx((size_t)3 * cg * plane * 8, 0);
            const size_t ipl = (size_t)cg * plane * 8;  // bf16 per piece
            for (int n = 0; n < N; ++n)
                for (int ch = 0; ch < Cin; ++ch)
                    for (int y = 0; y < H; ++y)
                        for (int xx0 = 0; xx0 < W; ++xx0) {
                            const float v = x[(((size_t)n * Cin + ch) * H + y) * W + xx0];
                            const size_t u = (size_t)(ch / 8) * plane + (3 + (size_t)n * (H + 3) + y) * P + 3 + xx0;
                            const uint16_t h0 = rne(v);
                            const float r = v - f16(h0);
                            const uint16_t h1 = rne(r);
                            const uint16_t h2 = rne(r - f16(h1));
                            hx[u * 8 + ch % 8] = h0;
                            hx[ipl + u * 8 + ch % 8] = h1;
                            hx[2 * ipl + u * 8 + ch % 8] = h2;
                        }
            DevBuf bi, bo;
            uint8_t* xi = bi.ensure<uint8_t>(hx.size() * 2, h->stream);
            const size_t opl = (size_t)og * plane * 8;
            uint8_t* yo = bo.ensure<uint8_t>(3 * opl * 2, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(xi, hx.data(), hx.size() * 2, hipMemcpyHostToDevice, h->stream));
            OPOSE_HIP_CHECK(hipMemsetAsync(yo, 0, 3 * opl * 2, h->stream));
            ConvSeg sg{c, N, H, W, x6pact(xi, cg, 0, N, H, W), x6pact(yo, og, 0, N, H, W), XAct{}, relu != 0};
            if (mt == -3) sg.slabs = 1;
            {
                Redirect<int> family(h->force_kernel, mt == -3 ? kKernelWino : kKernelWin);
                run_conv_x6_segs(h, {sg});
            }
            std::vector<uint16_t> hy(3 * opl);
            OPOSE_HIP_CHECK(hipMemcpyAsync(hy.data(), yo, hy.size() * 2, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            for (int n = 0; n < N; ++n)
                for (int ch = 0; ch < Cout; ++ch)
                    for (int y = 0; y < H; ++y)
                        for (int xx0 = 0; xx0 < W; ++xx0) {
                            const size_t u = (size_t)(ch / 8) * plane + (3 + (size_t)n * (H + 3) + y) * P + 3 + xx0;
                            out[(((size_t)n * Cout + ch) * H + y) * W + xx0] =
                                (f16(hy[u * 8 + ch % 8]) + f16(hy[opl + u * 8 + ch % 8])) + f16(hy[2 * opl + u * 8 + ch % 8]);
                        }
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
