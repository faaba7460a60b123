// engine_tgcn.cpp — the TGCN sign classifier's entry points: a model's checks, the batch-norm fold
// and the packing of its weights for tgcn.hip, and the forward pass's staging, chunks and launches.
#include "engine.h"

// One loaded model: everything the kernels read, in one device allocation.
struct opose_tgcn {
    int V = 0, F = 0, H = 0, C = 0, S = 0, resi = 0;
    std::vector<opose::TgcnLayer> layers;  // 1 + 2 S
    const float *fcT = nullptr, *fcb = nullptr;  // [H][C] (fc_out.weight transposed), [C]
    void* mem = nullptr;
};

namespace opose {

static int64_t tgcn_layer_params(int V, int F, int H) { return (int64_t)F * H + (int64_t)V * V + H + 4 * (int64_t)V * H; }

// W [F][H] -> [H tiles][F chunks][piece][k-group][column] units of 8 bf16 (k = 32 chunk + 8 group + e),
// zero past F and H
static void tgcn_pack_w(const float* W, int F, int H, uint16_t* out) {
    const int tiles = (H + kTgcnTN - 1) / kTgcnTN, nK = (F + 31) / 32;
    std::fill(out, out + tgcn_w_units(F, H) * 8, (uint16_t)0);
    for (int t = 0; t < tiles; ++t)
        for (int c = 0; c < nK; ++c)
            for (int g = 0; g < 4; ++g)
                for (int col = 0; col < kTgcnTN; ++col)
                    for (int e = 0; e < 8; ++e) {
                        const int k = 32 * c + 8 * g + e, h = t * kTgcnTN + col;
                        if (k >= F || h >= H) continue;
                        uint16_t p[3];
                        split3_host(W[(size_t)k * H + h], p);
                        for (int pc = 0; pc < 3; ++pc)
                            out[(((((size_t)t * nK + c) * 3 + pc) * 4 + g) * kTgcnTN + col) * 8 + e] = p[pc];
                    }
}

// att [V][V] -> [k-step][piece][k-group][row] units (k = 32 step + 8 group + e the node summed over),
// zero past V in both directions
static void tgcn_pack_att(const float* att, int V, uint16_t* out) {
    std::fill(out, out + kTgcnAttUnits * 8, (uint16_t)0);
    for (int ks = 0; ks < 2; ++ks)
        for (int g = 0; g < 4; ++g)
            for (int row = 0; row < V; ++row)
                for (int e = 0; e < 8; ++e) {
                    const int k = 32 * ks + 8 * g + e;
                    if (k >= V) continue;
                    uint16_t p[3];
                    split3_host(att[(size_t)row * V + k], p);
                    for (int pc = 0; pc < 3; ++pc)
                        out[((((size_t)ks * 3 + pc) * 4 + g) * kTgcnV + row) * 8 + e] = p[pc];
                }
}

static int tgcn_geometry_check(opose_ctx* h, int V, int F, int H, int C, int S) {
    if (V < 1 || F < 1 || H < 1 || C < 1 || S < 0) {
        h->err = "tgcn: V, F_in, H and C must be positive and n_stage not negative";
        return OPOSE_E_ARG;
    }
    if (V > kTgcnV || F > kTgcnMaxF || H > kTgcnMaxF || C > kTgcnMaxC || S > kTgcnMaxStage) {
        h->err = "tgcn: V, F_in, H, C or n_stage beyond the supported limit";
        return OPOSE_E_SHAPE;
    }
    return OPOSE_OK;
}

// The layers of the chunk's samples [n0, n1): the stem from the caller's x (copies in place), the
// blocks between the three activation buffers, the head.  1 + 2 S + 1 launches.
static void tgcn_run_chunk(opose_ctx* h, const opose_tgcn* m, const float* x, int copies, int64_t n0, int64_t n1,
                           float* act[3], float* copy_logits, float* logits) {
    const int n = (int)(n1 - n0);
    launch_tgcn_gc(m->layers[0], m->V, x, (int64_t)copies * m->F, copies, n0, n, nullptr, act[0], h->stream);
    int cur = 0;
    for (int s = 0; s < m->S; ++s) {
        const int mid = (cur + 1) % 3, nxt = (cur + 2) % 3;
        launch_tgcn_gc(m->layers[1 + 2 * s], m->V, act[cur], m->H, 1, 0, n, nullptr, act[mid], h->stream);
        launch_tgcn_gc(m->layers[2 + 2 * s], m->V, act[mid], m->H, 1, 0, n, m->resi ? act[cur] : nullptr, act[nxt],
                       h->stream);
        cur = nxt;
    }
    launch_tgcn_head(act[cur], n0, n1, copies, m->V, m->H, m->C, m->fcT, m->fcb, copy_logits, logits, h->stream);
}

}  // namespace opose

using namespace opose;

int opose_tgcn_create(opose_t* h, int V, int F_in, int H, int C, int n_stage, int is_resi, double bn_eps,
                      const float* params, int64_t n_params, opose_tgcn_t** model) {
    if (!h || !params || !model) return OPOSE_E_ARG;
    if (const int rc = tgcn_geometry_check(h, V, F_in, H, C, n_stage)) return rc;
    if (!(bn_eps > 0.0)) {
        h->err = "tgcn: bn_eps must be positive";
        return OPOSE_E_ARG;
    }
    const int nl = 1 + 2 * n_stage;
    const int64_t expect = tgcn_layer_params(V, F_in, H) + 2 * (int64_t)n_stage * tgcn_layer_params(V, H, H) +
                           (int64_t)C * H + C;
    if (n_params != expect) {
        h->err = "tgcn: n_params is " + std::to_string(n_params) + ", the model takes " + std::to_string(expect);
        return OPOSE_E_ARG;
    }
    const size_t VH = (size_t)V * H;
    {
        const float* p = params;
        for (int l = 0; l < nl; ++l) {
            const int F = l ? H : F_in;
            const float* var = p + (size_t)F * H + (size_t)V * V + H + 3 * VH;
            for (size_t e = 0; e < VH; ++e)
                if (!((double)var[e] + bn_eps > 0.0)) {
                    h->err = "tgcn: a running_var + bn_eps is not positive";
                    return OPOSE_E_ARG;
                }
            p += tgcn_layer_params(V, F, H);
        }
    }
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        // the device block: per layer packed W, packed att, a, c; then fcT, fcb (every part a
        // multiple of 16 bytes)
        auto pad4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
        size_t bytes = 0;
        for (int l = 0; l < nl; ++l) bytes += (tgcn_w_units(l ? H : F_in, H) + kTgcnAttUnits) * 16 + 2 * pad4(VH) * 4;
        bytes += (pad4((size_t)H * C) + pad4(C)) * 4;
        std::vector<uint8_t> host(bytes);
        auto mdl = std::make_unique<opose_tgcn>();
        mdl->V = V, mdl->F = F_in, mdl->H = H, mdl->C = C, mdl->S = n_stage, mdl->resi = is_resi ? 1 : 0;
        OPOSE_HIP_CHECK(hipMalloc(&mdl->mem, bytes));
        uint8_t* dev = static_cast<uint8_t*>(mdl->mem);
        size_t o = 0;
        const float* p = params;
        for (int l = 0; l < nl; ++l) {
            const int F = l ? H : F_in;
            const float *W = p, *att = W + (size_t)F * H, *bias = att + (size_t)V * V, *gamma = bias + H,
                        *beta = gamma + VH, *mean = beta + VH, *var = mean + VH;
            TgcnLayer L{};
            L.F = F, L.H = H;
            L.w = dev + o;
            tgcn_pack_w(W, F, H, reinterpret_cast<uint16_t*>(host.data() + o));
            o += tgcn_w_units(F, H) * 16;
            L.att = dev + o;
            tgcn_pack_att(att, V, reinterpret_cast<uint16_t*>(host.data() + o));
            o += kTgcnAttUnits * 16;
            // the batch-norm on running statistics and the layer's bias as one scale and shift,
            // formed in float64 and rounded once
            float* a = reinterpret_cast<float*>(host.data() + o);
            L.a = reinterpret_cast<const float*>(dev + o);
            o += pad4(VH) * 4;
            float* c = reinterpret_cast<float*>(host.data() + o);
            L.c = reinterpret_cast<const float*>(dev + o);
            o += pad4(VH) * 4;
            for (size_t e = 0; e < VH; ++e) {
                const double ad = (double)gamma[e] / std::sqrt((double)var[e] + bn_eps);
                a[e] = (float)ad;
                c[e] = (float)((double)beta[e] + ((double)bias[e % H] - (double)mean[e]) * ad);
            }
            mdl->layers.push_back(L);
            p += tgcn_layer_params(V, F, H);
        }
        float* fcT = reinterpret_cast<float*>(host.data() + o);
        mdl->fcT = reinterpret_cast<const float*>(dev + o);
        o += pad4((size_t)H * C) * 4;
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < H; ++k) fcT[(size_t)k * C + c] = p[(size_t)c * H + k];
        std::memcpy(host.data() + o, p + (size_t)C * H, (size_t)C * 4);
        mdl->fcb = reinterpret_cast<const float*>(dev + o);
        const hipError_t e = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(mdl->mem);
            OPOSE_HIP_CHECK(e);
        }
        *model = mdl.release();
    });
    return OPOSE_OK;
}

int opose_tgcn_destroy(opose_t* h, opose_tgcn_t* model) {
    if (!h || !model) return OPOSE_E_ARG;
    OPOSE_TRY(h, {
        OPOSE_HIP_CHECK(hipSetDevice(h->device));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // no launch still reads the model
        OPOSE_HIP_CHECK(hipFree(model->mem));
        delete model;
    });
    return OPOSE_OK;
}

int opose_tgcn_forward(opose_t* h, const opose_tgcn_t* m, const float* x, int B, int copies, int max_samples,
                       float* logits, float* copy_logits, int flags) {
    if (!h || !m || !x || !logits) return OPOSE_E_ARG;
    if (B < 1 || copies < 1 || max_samples < 0) {
        h->err = "tgcn: B and copies must be positive and max_samples not negative";
        return OPOSE_E_ARG;
    }
    const int64_t ns = (int64_t)B * copies;
    if (ns >= ((int64_t)1 << 24)) {
        h->err = "tgcn: copies * B beyond the supported limit";
        return OPOSE_E_SHAPE;
    }
    OPOSE_TRY(h, {
        enter_main(h);
        const bool id = flags & OPOSE_IN_DEVICE, od = flags & OPOSE_OUT_DEVICE;
        const size_t VH = (size_t)m->V * m->H, nx = (size_t)ns * m->V * m->F, nl = (size_t)B * m->C,
                     ncl = (size_t)ns * m->C;
        // a chunk: max_samples, or as many samples as keep an activation buffer at 64 MB
        const int64_t chunk =
            std::min<int64_t>(ns, max_samples ? max_samples : std::max<int64_t>(kTgcnG, ((int64_t)1 << 24) / (int64_t)VH));
        const float* xd = x;
        if (!id) {
            float* p = h->tg_x.ensure<float>(nx, h->stream);
            OPOSE_HIP_CHECK(hipMemcpyAsync(p, x, nx * 4, hipMemcpyHostToDevice, h->stream));
            xd = p;
        }
        // logits [B][C] | copy_logits [B copies][C]: the caller's device arrays, or staged
        float* ld = logits;
        float* cd = copy_logits;
        if (!od) {
            ld = h->tg_out.ensure<float>(nl + ncl, h->stream);
            cd = ld + nl;
        } else if (!cd) {
            cd = h->tg_out.ensure<float>(ncl, h->stream);
        }
        float* act[3];
        for (int i = 0; i < 3; ++i) act[i] = h->tg_act[i].ensure<float>((size_t)chunk * VH, h->stream);
        ProfEntry pe;
        h->prof_begin(pe, "tgcn_forward", 0, 0);
        for (int64_t n0 = 0; n0 < ns; n0 += chunk) tgcn_run_chunk(h, m, xd, copies, n0, std::min(ns, n0 + chunk), act, cd, ld);
        h->prof_end(pe);
        if (!od) {
            OPOSE_HIP_CHECK(hipMemcpyAsync(logits, ld, nl * 4, hipMemcpyDeviceToHost, h->stream));
            if (copy_logits) OPOSE_HIP_CHECK(hipMemcpyAsync(copy_logits, cd, ncl * 4, hipMemcpyDeviceToHost, h->stream));
            OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        h->prof_drain();
    });
    return OPOSE_OK;
}

int opose_debug_tgcn_layer(opose_t* h, const opose_tgcn_t* m, int layer, const float* x_in, int B, const float* residual,
                           float* out) {
    if (!h || !m || !x_in || !out) return OPOSE_E_ARG;
    if (layer < 0 || layer >= (int)m->layers.size() || B < 1) {
        h->err = "tgcn: no such layer, or B is not positive";
        return OPOSE_E_ARG;
    }
    if (B >= (1 << 24)) {
        h->err = "tgcn: B beyond the supported limit";
        return OPOSE_E_SHAPE;
    }
    OPOSE_TRY(h, {
        enter_main(h);
        const TgcnLayer& L = m->layers[layer];
        const size_t nx = (size_t)B * m->V * L.F, no = (size_t)B * m->V * L.H;
        DevBuf xb, rb, ob;
        float* xd = xb.ensure<float>(nx, h->stream);
        float* od = ob.ensure<float>(no, h->stream);
        float* rd = residual ? rb.ensure<float>(no, h->stream) : nullptr;
        OPOSE_HIP_CHECK(hipMemcpyAsync(xd, x_in, nx * 4, hipMemcpyHostToDevice, h->stream));
        if (rd) OPOSE_HIP_CHECK(hipMemcpyAsync(rd, residual, no * 4, hipMemcpyHostToDevice, h->stream));
        launch_tgcn_gc(L, m->V, xd, L.F, 1, 0, B, rd, od, h->stream);
        OPOSE_HIP_CHECK(hipMemcpyAsync(out, od, no * 4, hipMemcpyDeviceToHost, h->stream));
        OPOSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    });
    return OPOSE_OK;
}
