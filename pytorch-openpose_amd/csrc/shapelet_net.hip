// shapelet_net.hip — learning a shapelet by gradient descent: the reference's ShapeletNetModel
// (srcmx/shapeletmodel.py:11-90) for several independent models over the same clips.
//
// Reference steps replaced (hitmaxiang/pytorch-openpose):
//  * srcmx/shapeletmodel.py:82-90   slidingdistance (conv1d, QQ + XX - 2 QX) and the torch.min of
//    forward / __call__ / localizeshape                                   => shapelet_net_forward
//  * srcmx/shapeletmodel.py:36-62   the Linear(1, 2) head, CrossEntropyLoss, its backward and the
//    head's share of Adam.step                                            => shapelet_net_head
//  * the backward of the minimum into the query and the query's share of Adam.step
//                                                                         => shapelet_net_step
//
// One epoch is these three launches in stream order; include/opose.h states the rule they follow
// and tests/shapelet_net_cases.py restates it in NumPy.  The distance is the direct squared form of
// shapelet.hip (fp32, e over d ascending, s over k ascending, no FMA contraction in this file), not
// the reference's expansion, which cancels.  No floating-point atomics: every sum has one order.
//
// Every address below derives from the validated integers of the call (off, q_off, t_pad, D) or
// from a location the forward kernel wrote, which is a position 0 .. P - 1 of its clip by
// construction; a row at or past its clip's end is never read (it is +0).
#include "common.h"
#include "kernels.h"
#include "shapelet.h"

namespace opose {

// positions of a clip of len rows for a query of m rows
__device__ inline int net_positions(int len, int m, int t_pad) { return (t_pad ? t_pad : len) - m + 1; }

// ------------------------------------------------------------------------------------ forward
// Workgroup (position tile, clip i, model k): thread t takes position c = tile * kNetTC + t,
//   s = sum over k of ( sum over d of (q[k][d] - x_i[c + k][d])^2 ),
// and the tile's minimum of (bits of s) << 32 | c goes into best[k][i] by one 64-bit integer
// atomicMin per wave: s >= +0, so the key orders like (s, c) and the first minimum wins whatever
// the order of arrival.  best holds all ones before the launch.  kQLds: the query is staged into
// LDS; kXLds: so are the clip's rows c0 .. c0 + kNetTC + m - 2 (row stride D | 1: lanes read
// distinct banks), rows at or past the clip's end as +0.
template <bool kQLds, bool kXLds>
__global__ __launch_bounds__(kNetTC) void shapelet_net_forward(const float* __restrict__ seq,
                                                               const int64_t* __restrict__ off, int D, int t_pad,
                                                               const NetModel* __restrict__ models,
                                                               const float* __restrict__ query, int n_seq,
                                                               unsigned long long* __restrict__ best) {
    extern __shared__ float net_lds[];
    const int t = threadIdx.x, i = blockIdx.y, k = blockIdx.z;
    const NetModel md = models[k];
    const int m = md.m;
    const int64_t x0 = off[i];
    const int len = (int)(off[i + 1] - x0);
    const int P = net_positions(len, m, t_pad);
    const int c0 = blockIdx.x * kNetTC;
    if (c0 >= P) return;  // the whole workgroup: a shorter clip or a longer query has fewer tiles
    const float* qg = query + md.row0 * D;
    const int ld = D | 1;
    float* ql = net_lds;
    float* xl = net_lds + (kQLds ? m * D : 0);
    if (kQLds)
        for (int e = t; e < m * D; e += kNetTC) ql[e] = qg[e];
    if (kXLds) {
        const int rows = kNetTC + m - 1;
        for (int e = t; e < rows * D; e += kNetTC) {
            const int r = e / D, d = e - r * D;
            xl[r * ld + d] = c0 + r < len ? seq[(x0 + c0 + r) * D + d] : 0.0f;
        }
    }
    if (kQLds || kXLds) __syncthreads();
    const int c = c0 + t;
    float s = 0.0f;
    for (int kk = 0; kk < m; ++kk) {
        const float* q = (kQLds ? ql : qg) + kk * D;
        // a row at or past the clip's end reads as +0: without the tile no such row is addressed
        const bool in = c + kk < len;
        const float* x = kXLds ? xl + (t + kk) * ld : seq + (x0 + (in ? c + kk : 0)) * D;
        float e = 0.0f;
        int d = 0;
        if (kXLds || in) {
            for (; d + kNetDU <= D; d += kNetDU) {
#pragma unroll
                for (int u = 0; u < kNetDU; ++u) {
                    const float v = q[d + u] - x[d + u];
                    e = e + v * v;
                }
            }
            for (; d < D; ++d) {
                const float v = q[d] - x[d];
                e = e + v * v;
            }
        } else {
            for (; d < D; ++d) {
                const float v = q[d] - 0.0f;
                e = e + v * v;
            }
        }
        s = s + e;
    }
    unsigned long long key = c < P ? ((unsigned long long)__float_as_uint(s) << 32) | (unsigned)c : ~0ull;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, sh);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), sh);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        if (o < key) key = o;
    }
    if ((t & 63) == 0) atomicMin(best + (size_t)k * n_seq + i, key);
}

size_t shapelet_net_q_bytes(int m, int D) { return sizeof(float) * (size_t)m * D; }
size_t shapelet_net_x_bytes(int m, int D) { return sizeof(float) * (size_t)(kNetTC + m - 1) * (D | 1); }
static_assert(kNetQLdsBytes + kNetXLdsBytes <= 65536, "dynamic LDS within what a launch gets without an attribute call");
static_assert(kNetTC == 64, "one wave per workgroup: the tile's minimum is one wave reduction");

void launch_shapelet_net_forward(const float* seq, const int64_t* off, int n_seq, int D, int t_pad,
                                 const NetModel* models, int n_models, int m_max, int tiles, const float* query,
                                 uint64_t* best, hipStream_t st) {
    // one choice per launch, by the longest query: every model of the launch takes the same path
    const bool ql = shapelet_net_q_bytes(m_max, D) <= (size_t)kNetQLdsBytes;
    const bool xl = shapelet_net_x_bytes(m_max, D) <= (size_t)kNetXLdsBytes;
    const size_t shm = (ql ? shapelet_net_q_bytes(m_max, D) : 0) + (xl ? shapelet_net_x_bytes(m_max, D) : 0);
    const dim3 grid(tiles, n_seq, n_models), block(kNetTC);
    unsigned long long* b = reinterpret_cast<unsigned long long*>(best);
    if (ql && xl)
        hipLaunchKernelGGL((shapelet_net_forward<true, true>), grid, block, shm, st, seq, off, D, t_pad, models, query,
                           n_seq, b);
    else if (ql)
        hipLaunchKernelGGL((shapelet_net_forward<true, false>), grid, block, shm, st, seq, off, D, t_pad, models, query,
                           n_seq, b);
    else if (xl)
        hipLaunchKernelGGL((shapelet_net_forward<false, true>), grid, block, shm, st, seq, off, D, t_pad, models, query,
                           n_seq, b);
    else
        hipLaunchKernelGGL((shapelet_net_forward<false, false>), grid, block, shm, st, seq, off, D, t_pad, models, query,
                           n_seq, b);
}

// ------------------------------------------------------------------------------------ Adam
// torch.optim.Adam's step on one fp32 element (defaults: betas 0.9 / 0.999, eps 1e-8, no weight
// decay): step = lr / (1 - beta1^t) and bc2s = sqrt(1 - beta2^t) come from the host, formed in
// float64 and rounded once.
__device__ inline float net_adam(float p, float g, float* m, float* v, float step, float bc2s) {
    const float w1 = (float)(1.0 - 0.9), b2 = (float)0.999, w2 = (float)(1.0 - 0.999);
    const float mn = *m + (g - *m) * w1;
    const float vn = *v * b2 + (w2 * g) * g;
    *m = mn;
    *v = vn;
    const float denom = sqrtf(vn) / bc2s + 1e-8f;
    return p - step * (mn / denom);
}

// ------------------------------------------------------------------------------------ head
// One workgroup per model k.  Per clip i, in float64 from the fp32 d_i = the value half of
// best[k][i] and the head (w0, w1, b0, b1): z_j = w_j d + b_j, the log-softmax through the larger
// z, dz_j = (p_j - [y = j]) / N and g_i = dz_0 w_0 + dz_1 w_1, stored as float32.  The five sums
// over the clips (log p_i[y_i], dz_0 d, dz_1 d, dz_0, dz_1) are taken i ascending, each by one
// thread, from the terms the workgroup left in ws [n_models][5][n_seq]; correct counts
// argmax_j z_ij == y_i with index 0 on a tie (an integer count: its order does not matter).
//   loss_out  (or null) the model's loss goes to loss_out[k * loss_stride]
//   dis, locs, correct (or null) the halves of best and the count, [n_models][n_seq] / [n_models]
//   dhead     (or null) the four sums dw0, dw1, db0, db1 as float64
//   update    the head's Adam step, in place, from the sums rounded to float32
//   next      (or null) the other buffer of best, set to all ones for the next forward launch
__global__ __launch_bounds__(kNetThreads) void shapelet_net_head(
    const unsigned long long* __restrict__ best, unsigned long long* __restrict__ next,
    const uint8_t* __restrict__ labels, int n_seq, float* __restrict__ head, float* __restrict__ head_m,
    float* __restrict__ head_v, float step, float bc2s, int update, float* __restrict__ g, double* __restrict__ ws,
    double* __restrict__ loss_out, int64_t loss_stride, float* __restrict__ dis, int32_t* __restrict__ locs,
    int32_t* __restrict__ correct, double* __restrict__ dhead) {
    __shared__ double sums[5];
    __shared__ int right;
    const int t = threadIdx.x, k = blockIdx.x;
    const double w0 = head[4 * k], w1 = head[4 * k + 1], b0 = head[4 * k + 2], b1 = head[4 * k + 3];
    const double N = (double)n_seq;
    double* wk = ws + (size_t)k * 5 * n_seq;
    if (t == 0) right = 0;
    __syncthreads();
    int mine = 0;
    for (int i = t; i < n_seq; i += kNetThreads) {
        const size_t o = (size_t)k * n_seq + i;
        const unsigned long long key = best[o];
        const float df = __uint_as_float((unsigned)(key >> 32));
        const int y = labels[i];
        const double d = (double)df;
        const double z0 = w0 * d + b0, z1 = w1 * d + b1;
        const double mx = z0 > z1 ? z0 : z1;
        const double lse = mx + log(exp(z0 - mx) + exp(z1 - mx));
        const double lp0 = z0 - lse, lp1 = z1 - lse;
        const double dz0 = (exp(lp0) - (y == 0 ? 1.0 : 0.0)) / N;
        const double dz1 = (exp(lp1) - (y == 1 ? 1.0 : 0.0)) / N;
        if (g) g[o] = (float)(dz0 * w0 + dz1 * w1);
        wk[i] = y ? lp1 : lp0;
        wk[(size_t)n_seq + i] = dz0 * d;
        wk[(size_t)2 * n_seq + i] = dz1 * d;
        wk[(size_t)3 * n_seq + i] = dz0;
        wk[(size_t)4 * n_seq + i] = dz1;
        mine += ((z1 > z0) ? 1 : 0) == y;
        if (dis) {
            dis[o] = df;
            locs[o] = (int32_t)(unsigned)key;
        }
        if (next) next[o] = ~0ull;
    }
    if (mine) atomicAdd(&right, mine);
    __syncthreads();  // the terms in ws are visible to the workgroup
    if (t < 5) {
        const double* col = wk + (size_t)t * n_seq;
        double acc = 0.0;
        for (int i = 0; i < n_seq; ++i) acc = acc + col[i];
        sums[t] = acc;
    }
    __syncthreads();
    if (t == 0) {
        if (loss_out) loss_out[(int64_t)k * loss_stride] = -(sums[0] / N);
        if (correct) correct[k] = right;
    }
    if (t < 4) {
        if (dhead) dhead[4 * k + t] = sums[1 + t];
        if (update)
            head[4 * k + t] = net_adam(head[4 * k + t], (float)sums[1 + t], head_m + 4 * k + t, head_v + 4 * k + t, step, bc2s);
    }
}

void launch_shapelet_net_head(const uint64_t* best, uint64_t* next, const uint8_t* labels, int n_seq, int n_models,
                              float* head, float* head_m, float* head_v, float step, float bc2s, bool update, float* g,
                              double* ws, double* loss_out, int64_t loss_stride, float* dis, int32_t* locs,
                              int32_t* correct, double* dhead, hipStream_t st) {
    hipLaunchKernelGGL(shapelet_net_head, dim3(n_models), dim3(kNetThreads), 0, st,
                       reinterpret_cast<const unsigned long long*>(best), reinterpret_cast<unsigned long long*>(next),
                       labels, n_seq, head, head_m, head_v, step, bc2s, update ? 1 : 0, g, ws, loss_out, loss_stride, dis,
                       locs, correct, dhead);
}

// ------------------------------------------------------------------------------------ query step
// Workgroup (block of kNetThreads query elements, model k): the thread of element (kk, d) walks
// the clips i ascending,
//   dq = sum over i of g_i * (2 * (q[kk][d] - x_i[loc_i + kk][d])),  fp32 from +0,
// loc_i the location half of best[k][i], a row at or past the clip's end as +0; then the element's
// Adam step in place, or, with dq_out, the gradient alone.
__global__ __launch_bounds__(kNetThreads) void shapelet_net_step(
    const float* __restrict__ seq, const int64_t* __restrict__ off, int n_seq, int D,
    const NetModel* __restrict__ models, const unsigned long long* __restrict__ best, const float* __restrict__ g,
    float* __restrict__ query, float* __restrict__ q_m, float* __restrict__ q_v, float step, float bc2s,
    float* __restrict__ dq_out) {
    const int k = blockIdx.y;
    const NetModel md = models[k];
    const int e = blockIdx.x * kNetThreads + threadIdx.x;
    if (e >= md.m * D) return;
    const int kk = e / D, d = e - kk * D;
    const size_t qe = (size_t)md.row0 * D + e;
    const float qv = query[qe];
    float acc = 0.0f;
    for (int i = 0; i < n_seq; ++i) {
        const size_t o = (size_t)k * n_seq + i;
        const int row = (int)(unsigned)best[o] + kk;
        const int64_t x0 = off[i];
        const int len = (int)(off[i + 1] - x0);
        const float xv = row >= 0 && row < len ? seq[(x0 + row) * D + d] : 0.0f;
        const float t2 = 2.0f * (qv - xv);
        acc = acc + g[o] * t2;
    }
    if (dq_out) {
        dq_out[qe] = acc;
        return;
    }
    query[qe] = net_adam(qv, acc, q_m + qe, q_v + qe, step, bc2s);
}

void launch_shapelet_net_step(const float* seq, const int64_t* off, int n_seq, int D, const NetModel* models,
                              int n_models, int m_max, const uint64_t* best, const float* g, float* query, float* q_m,
                              float* q_v, float step, float bc2s, float* dq_out, hipStream_t st) {
    const dim3 grid((m_max * D + kNetThreads - 1) / kNetThreads, n_models);
    hipLaunchKernelGGL(shapelet_net_step, grid, dim3(kNetThreads), 0, st, seq, off, n_seq, D, models,
                       reinterpret_cast<const unsigned long long*>(best), g, query, q_m, q_v, step, bc2s, dq_out);
}

}  // namespace opose
