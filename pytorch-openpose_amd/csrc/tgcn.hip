// tgcn.hip — the TGCN sign classifier's forward pass in evaluation mode: the reference's
// GCN_muti_att (cls/TGCN/tgcn_model.py) driven as cls/TGCN/test_tgcn.py drives it.
//
// Reference steps replaced (hitmaxiang/pytorch-openpose):
//  * cls/TGCN/tgcn_model.py:38-45    GraphConvolution_att.forward, att (x W) + bias,
//  * cls/TGCN/tgcn_model.py:70-85,   the BatchNorm1d on running statistics, Tanh, the identity
//    116-123                         Dropout and a block's residual                  => tgcn_gc
//  * cls/TGCN/tgcn_model.py:126-127  the node mean and fc_out,
//  * cls/TGCN/test_tgcn.py:38-39     the mean over the copies                        => tgcn_head
//
// include/opose.h states the rule and tests/tgcn_cases.py restates it in NumPy float64.
//
// tgcn_gc, one launch per graph-convolution layer.  A workgroup of 4 waves takes kTgcnG samples and
// kTgcnTN output columns; wave w owns the node rows 16 w .. 16 w + 15 of the kTgcnV = 64 padded
// rows.  Both products run on v_mfma_f32_16x16x32_bf16 with each fp32 operand as three exact bf16
// pieces and the six piece products of x6.h, in x6.h's order:
//   1. P = x W.  k runs in chunks of 32, ascending; per chunk the six products, one MFMA each, all
//      into one fp32 accumulator that starts at +0.  The wave reads its rows of x straight from
//      global memory (row v >= V and column k >= F read as +0: no padded copy of x exists) and
//      splits them in registers; W comes packed by the host (zero past F and H), a chunk at a time
//      through LDS, the next chunk's global loads of W in flight while this one multiplies.
//   2. P goes from the accumulators to LDS, split again: all 64 rows by 64 columns of the three
//      piece planes are written for every sample, so nothing a previous sample or launch left is
//      ever read.  Rows >= V of P are the products of the +0 rows of x.
//   3. Y = att P.  k = the 64 padded nodes, two k-steps (nodes 0..31, then 32..63), six products
//      each, one accumulator from +0.  att comes packed by the host, zero past V in both
//      directions, and stays in registers for the workgroup's samples.
//   4. rows < V and columns < H only: y = tanhf(Y * a + c) (one multiply, one add: this file is
//      built without FMA contraction), then + the residual when the layer closes a block.
// A sample's accumulators, fragments and LDS image are its own: its result does not depend on the
// samples that share its workgroup or its launch.
//
// tgcn_head, one launch: a workgroup per batch element b.  Per copy i of b in the launch, thread h
// takes m[h] = (sum over v ascending of y[v][h]) / V, then thread c takes
// (sum over h ascending of fcT[h][c] * m[h]) + fc_b[c], all fp32 from +0; the workgroup that holds
// b's last copy folds logits[b][c] = (sum over i ascending of copy_logits[b][i][c]) / copies.
// No atomics and no barrier beyond the workgroup's.
//
// Every address derives from the validated integers of the call; a thread writes out[n][v][h] only
// for n < the launch's samples, v < V and h < H.
#include "common.h"
#include "kernels.h"
#include "x6.h"

namespace opose {

// 8 consecutive floats of a row of x from column k (a multiple of 8): vec when the row is 16-byte
// aligned and wholly inside [0, F); else element by element, +0 at and past F.  row == nullptr: +0.
__device__ __forceinline__ void tgcn_load8(const float* row, int k, int F, bool vec, float (&v)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = 0.0f;
    if (!row || k >= F) return;
    if (vec) {
        const float4 lo = *reinterpret_cast<const float4*>(row + k);
        const float4 hi = *reinterpret_cast<const float4*>(row + k + 4);
        v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w;
        v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (k + t < F) v[t] = row[k + t];
    }
}

// a 16-byte unit as an MFMA operand fragment
__device__ __forceinline__ i32x4 tgcn_frag(const uint4& u) { return i32x4{(int)u.x, (int)u.y, (int)u.z, (int)u.w}; }

__global__ __launch_bounds__(kTgcnThreads) void tgcn_gc(TgcnLayer L, int V, const float* __restrict__ x, int64_t ld,
                                                        int copies, int64_t n_in0, int n_samples, int tiles,
                                                        const float* __restrict__ res, float* __restrict__ out) {
    constexpr int G = kTgcnG, TN = kTgcnTN, NJ = TN / 16;
    __shared__ i32x4 s_w[3 * 4 * TN];  // a chunk of W: [piece][k-group][column]
    __shared__ i32x4 s_p[3 * 8 * TN];  // a sample's P: [piece][node group of 8][column]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g4 = lane >> 4;
    const int tile = blockIdx.x % tiles, grp = blockIdx.x / tiles;
    const int F = L.F, H = L.H, nK = (F + 31) >> 5;
    const int ns0 = grp * G;  // first sample of the group
    const int v_in = wave * 16 + l15;  // the row of x this lane feeds

    const float* rows[G];
#pragma unroll
    for (int s = 0; s < G; ++s) {
        const int64_t n = n_in0 + ns0 + s;
        rows[s] = (ns0 + s < n_samples && v_in < V) ? x + ((n / copies) * V + v_in) * ld + (n % copies) * (int64_t)F
                                                    : nullptr;
    }
    const bool vec = (F & 7) == 0 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const i32x4* wg = reinterpret_cast<const i32x4*>(L.w) + (size_t)tile * nK * (3 * 4 * TN);

    f32x4 acc[G][NJ];
#pragma unroll
    for (int s = 0; s < G; ++s)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[s][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    i32x4 wr[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) wr[q] = wg[tid + kTgcnThreads * q];

    for (int c = 0; c < nK; ++c) {
        // this chunk's x, in flight across the two barriers
        float xc[G][8];
#pragma unroll
        for (int s = 0; s < G; ++s) tgcn_load8(rows[s], 32 * c + 8 * g4, F, vec, xc[s]);
        __syncthreads();  // the previous chunk's reads of s_w are over
#pragma unroll
        for (int q = 0; q < 3; ++q) s_w[tid + kTgcnThreads * q] = wr[q];
        __syncthreads();
        if (c + 1 < nK) {
#pragma unroll
            for (int q = 0; q < 3; ++q) wr[q] = wg[(size_t)(c + 1) * (3 * 4 * TN) + tid + kTgcnThreads * q];
        }
        i32x4 fb[3][NJ];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                fb[pc][j] = s_w[(pc * 4 + g4) * TN + 16 * j + l15];
#pragma unroll
        for (int s = 0; s < G; ++s) {
            uint4 pw[3];
            pack_pieces8(xc[s], pw);
            i32x4 fa[3];
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) fa[pc] = tgcn_frag(pw[pc]);
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[s][j] = mfma_x6(fa[kPieceA[t]], fb[kPieceB[t]][j], acc[s][j]);
        }
    }

    // att fragments of the wave's rows: [k-step][piece], kept for every sample of the group
    i32x4 fatt[2][3];
    {
        const i32x4* ag = reinterpret_cast<const i32x4*>(L.att);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc)
                fatt[ks][pc] = ag[((ks * 3 + pc) * 4 + g4) * kTgcnV + wave * 16 + l15];
    }

    uint2* s_p2 = reinterpret_cast<uint2*>(s_p);
    const int n0col = tile * TN;
#pragma unroll
    for (int s = 0; s < G; ++s) {
        if (ns0 + s >= n_samples) continue;  // the whole workgroup: the group's tail
        __syncthreads();  // the previous sample's reads of s_p are over
        // the lane's accumulator block (s, j): nodes 16 wave + 4 g4 .. + 3 of column 16 j + l15 -- half
        // (g4 & 1) of unit (node group 2 wave + (g4 >> 1), column)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float v4[4] = {acc[s][j][0], acc[s][j][1], acc[s][j][2], acc[s][j][3]};
            uint2 w[3];
            pack_pieces4(v4, w);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc)
                s_p2[((pc * 8 + 2 * wave + (g4 >> 1)) * TN + 16 * j + l15) * 2 + (g4 & 1)] = w[pc];
        }
        __syncthreads();
        f32x4 y[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) y[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            i32x4 fb[3][NJ];
#pragma unroll
            for (int pc = 0; pc < 3; ++pc)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    fb[pc][j] = s_p[(pc * 8 + 4 * ks + g4) * TN + 16 * j + l15];
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int j = 0; j < NJ; ++j) y[j] = mfma_x6(fatt[ks][kPieceA[t]], fb[kPieceB[t]][j], y[j]);
        }
        // epilogue: rows < V, columns < H
        const size_t ob = (size_t)(ns0 + s) * V * H;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int h = n0col + 16 * j + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = wave * 16 + 4 * g4 + r;
                if (v < V && h < H) {
                    const size_t e = (size_t)v * H + h;
                    float t = y[j][r] * L.a[e];
                    t = t + L.c[e];
                    t = tanhf(t);
                    if (res) t = t + res[ob + e];
                    out[ob + e] = t;
                }
            }
        }
    }
}

void launch_tgcn_gc(const TgcnLayer& L, int V, const float* x, int64_t ld, int copies, int64_t n_in0, int n,
                    const float* res, float* out, hipStream_t st) {
    const int tiles = (L.H + kTgcnTN - 1) / kTgcnTN, groups = (n + kTgcnG - 1) / kTgcnG;
    hipLaunchKernelGGL(tgcn_gc, dim3((unsigned)(tiles * groups)), dim3(kTgcnThreads), 0, st, L, V, x, ld, copies, n_in0,
                       n, tiles, res, out);
}

__global__ __launch_bounds__(kTgcnThreads) void tgcn_head(const float* __restrict__ y, int64_t n0, int64_t n1,
                                                          int copies, int V, int H, int C,
                                                          const float* __restrict__ fcT, const float* __restrict__ fcb,
                                                          float* copy_logits, float* __restrict__ logits) {
    __shared__ float m[kTgcnMaxF];
    const int tid = threadIdx.x;
    const int64_t b = n0 / copies + blockIdx.x;
    for (int i = 0; i < copies; ++i) {
        const int64_t n = b * copies + i;
        if (n < n0 || n >= n1) continue;  // the whole workgroup
        const float* yn = y + (size_t)(n - n0) * V * H;
        __syncthreads();  // the previous copy's reads of m are over
        for (int h = tid; h < H; h += kTgcnThreads) {
            float s = 0.0f;
            for (int v = 0; v < V; ++v) s = s + yn[(size_t)v * H + h];
            m[h] = s / (float)V;
        }
        __syncthreads();
        for (int c = tid; c < C; c += kTgcnThreads) {
            float s = 0.0f;
            for (int h = 0; h < H; ++h) s = s + fcT[(size_t)h * C + c] * m[h];
            copy_logits[(size_t)n * C + c] = s + fcb[c];
        }
    }
    if ((b + 1) * copies <= n1) {
        // every copy_logits[b][i][c] read here was written by this thread, above or in an earlier launch
        for (int c = tid; c < C; c += kTgcnThreads) {
            float s = 0.0f;
            for (int i = 0; i < copies; ++i) s = s + copy_logits[(size_t)(b * copies + i) * C + c];
            logits[(size_t)b * C + c] = s / (float)copies;
        }
    }
}

void launch_tgcn_head(const float* y, int64_t n0, int64_t n1, int copies, int V, int H, int C, const float* fcT,
                      const float* fcb, float* copy_logits, float* logits, hipStream_t st) {
    const int64_t nb = (n1 - 1) / copies - n0 / copies + 1;
    hipLaunchKernelGGL(tgcn_head, dim3((unsigned)nb), dim3(kTgcnThreads), 0, st, y, n0, n1, copies, V, H, C, fcT, fcb,
                       copy_logits, logits);
}

}  // namespace opose
