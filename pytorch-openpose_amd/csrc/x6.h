// x6.h — the device core shared by the split-bf16 ("X6") convolution kernels (conv_x6.hip,
// conv_win.hip, conv_wino.hip, conv1x1_chain.hip): the exact three-way bf16 split and its packed
// stores, the piece-product order and MFMA wrapper, the XCD-contiguous workgroup id, the bias
// table, the weight LDS-DMA, the output epilogue (fp32 NCHW or X6 slices), and the work-unit
// decoding of a launch.  The six-block chunk loop of conv_x6 / conv_win_x6 is in x6_loop.h.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace opose {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) uint4* lds_units_t;  // 16-byte units in LDS

namespace x6 {

constexpr int x6_waves(int mt, int pt) { return mt * pt >= 32768 ? 8 : 4; }

__device__ __forceinline__ uint32_t bf16_rne(float x) {
    uint32_t u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// x -> three bf16 pieces, x0 + x1 + x2 == x exactly (each remainder is exact by Sterbenz)
__device__ __forceinline__ void split3(float x, uint32_t& h0, uint32_t& h1, uint32_t& h2) {
    h0 = bf16_rne(x);
    const float r = x - __uint_as_float(h0 << 16);
    h1 = bf16_rne(r);
    const float r2 = r - __uint_as_float(h1 << 16);
    h2 = bf16_rne(r2);
}

__device__ __forceinline__ float join3(uint32_t h0, uint32_t h1, uint32_t h2) {
    return (__uint_as_float(h0 << 16) + __uint_as_float(h1 << 16)) + __uint_as_float(h2 << 16);
}

// 4 (half a unit) or 8 (a unit) consecutive channels of one pixel, split: w[pc] = piece pc of all
// of them, two bf16 per word
__device__ __forceinline__ void pack_pieces4(const float (&v)[4], uint2 (&w)[3]) {
    uint32_t h[3][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) split3(v[t], h[0][t], h[1][t], h[2][t]);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        w[pc].x = h[pc][0] | (h[pc][1] << 16);
        w[pc].y = h[pc][2] | (h[pc][3] << 16);
    }
}
__device__ __forceinline__ void pack_pieces8(const float (&v)[8], uint4 (&w)[3]) {
    uint32_t h[3][8];
#pragma unroll
    for (int t = 0; t < 8; ++t) split3(v[t], h[0][t], h[1][t], h[2][t]);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        w[pc].x = h[pc][0] | (h[pc][1] << 16);
        w[pc].y = h[pc][2] | (h[pc][3] << 16);
        w[pc].z = h[pc][4] | (h[pc][5] << 16);
        w[pc].w = h[pc][6] | (h[pc][7] << 16);
    }
}
// ... written into the 3 piece planes (ps bytes apart): half a unit / a whole unit at `unit`
__device__ __forceinline__ void store4_x6(uint8_t* unit, uint32_t ps, const float (&v)[4]) {
    uint2 w[3];
    pack_pieces4(v, w);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<uint2*>(unit + (size_t)pc * ps) = w[pc];
}
__device__ __forceinline__ void store8_x6(uint8_t* unit, uint32_t ps, const float (&v)[8]) {
    uint4 w[3];
    pack_pieces8(v, w);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<uint4*>(unit + (size_t)pc * ps) = w[pc];
}

// The six piece products of a chunk, in issue order: A piece kPieceA[t] x B piece kPieceB[t],
// (0,2) (0,0) (0,1) (1,0) (2,0) (1,1) -- every kernel sums them in this order (x6_loop.h)
constexpr int kPieceA[6] = {0, 0, 0, 1, 2, 1};
constexpr int kPieceB[6] = {2, 0, 1, 0, 0, 1};
__device__ __forceinline__ f32x4 mfma_x6(const i32x4& a, const i32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
}

// this workgroup's XCD-contiguous id (common.h)
__device__ __forceinline__ int x6_xcd_id() { return xcd_contiguous_id(gridDim.x, blockIdx.x); }

// bias of the tile's MT rows (first row m0) into LDS, 0 past cout
__device__ __forceinline__ void x6_load_bias(float* s_bias, const X6Group& G, int m0, int MT) {
    const int tid = threadIdx.x;
    if (tid < MT) s_bias[tid] = (m0 + tid < G.cout) ? G.bias[m0 + tid] : 0.f;
}

// Weight (A operand) LDS-DMA of one 64-unit run: LDS units [unit0, unit0 + 64) of the stage at
// `stage` from the resource's bytes soffset + lane16 (= lane * 16, kept by the caller) ...
__device__ __forceinline__ void x6_dma_weights_unit(__amdgpu_buffer_rsrc_t rsrc, lds_units_t stage, int unit0,
                                                    uint32_t lane16, uint32_t soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(stage + unit0), 16, lane16, (int)soffset, 0, 0);
}
// the buffer resource of chunk c of packed weights wt ([chunk][piece][4][Mpad] units)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x6_weights_rsrc(const uint8_t* wt, int Mpad, int c) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(wt + (size_t)c * 12 * Mpad * 16), (short)0, (int)0x7fffffff,
                                             0x00020000);
}

// Slab partials (X6Args::partial): per work unit of a multi-slab group an fp32 [MT/4][PT] array
// of channel quads -- quad q (channels 4q .. 4q+3 of the tile), pixel pl at float index
// (q * PT + pl) * 4.  A lane's accumulator block holds 4 consecutive channels of one pixel, so
// it leaves the kernel as one 16-byte write-through (sc1) store; conv_x6_fixup reads two quads
// per X6 unit.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slab_rsrc(float* partial) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)partial, (short)0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void store_slab_quad(__amdgpu_buffer_rsrc_t r, uint32_t byte_off, f32x4 v) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)byte_off, 0, 16);  // aux 16: sc1
}

// unit index of (frame n, group g of the slice, y, x) in an X6 plane (common.h X6Layout)
__device__ __forceinline__ uint32_t x6_unit(const X6Layout& l, int n, int g, int y, int x) {
    return l.o0 + (uint32_t)n * l.fs + (uint32_t)g * l.gs + (uint32_t)y * l.rs + (uint32_t)x;
}

// Where a group's results go: fp32 NCHW channels [out_off, out_off + cout) of out_c, or X6
// slices (out, and a duplicate out2 when set)
struct X6Out {
    void *out, *out2;
    uint32_t out_ps, out2_ps;
    X6Layout out_l, out2_l;
    int out_c, out_off, cout, cout8, out_f32;  // cout8: cout rounded up to whole units
};
__device__ __forceinline__ X6Out x6_out(const X6Group& G) {
    return X6Out{G.out,   G.out2,    G.out_ps, G.out2_ps,        G.out_l, G.out2_l,
                 G.out_c, G.out_off, G.cout,   (G.cout + 7) & ~7, G.out_f32};
}
__device__ __forceinline__ X6Out x6_out(const X6ChainGroup& G) {
    return X6Out{G.out,   nullptr,   G.out_ps, 0u,                 G.out_l, G.out_l,
                 G.out_c, G.out_off, G.cout2,  (G.cout2 + 7) & ~7, G.out_f32};
}
// NCH = 4 or 8 consecutive channels from mq (a multiple of NCH) of pixel (n, y, x) into an X6 slice
template <int NCH>
__device__ __forceinline__ void x6_store_slice(void* out, const X6Layout& l, uint32_t ps, int n, int y, int x, int mq,
                                               const float (&v)[NCH]) {
    uint8_t* unit = static_cast<uint8_t*>(out) + (size_t)x6_unit(l, n, mq >> 3, y, x) * 16;
    if constexpr (NCH == 8) store8_x6(unit, ps, v);
    else store4_x6(unit + ((mq >> 2) & 1) * 8, ps, v);
}
// The output epilogue: finished values v (bias and ReLU applied) of channels mq .. mq + NCH - 1 of
// pixel (n, y, x), rem = y W + x of a frame of HW pixels
template <int NCH>
__device__ __forceinline__ void x6_store_quad(const X6Out& o, int n, int y, int x, int rem, int HW, int mq,
                                              const float (&v)[NCH]) {
    if (o.out_f32) {
        float* ob = static_cast<float*>(o.out) + ((size_t)n * o.out_c + o.out_off) * HW + rem;
#pragma unroll
        for (int t = 0; t < NCH; ++t)
            if (mq + t < o.cout) ob[(size_t)(mq + t) * HW] = v[t];
    } else if (mq < o.cout8) {
        x6_store_slice(o.out, o.out_l, o.out_ps, n, y, x, mq, v);
        if (o.out2) x6_store_slice(o.out2, o.out2_l, o.out2_ps, n, y, x, mq, v);
    }
}

// group of a tile (groups are numbered in tile order, X6Group::t0)
__device__ __forceinline__ int x6_group_of(const X6Args& a, int tile) {
    int g = 0;
    for (int i = 1; i < a.ngroups; ++i) g = tile >= a.g[i].t0 ? i : g;
    return g;
}

// A work unit: chunks [c0, c1) of one tile, slab s of the group's `slabs` (common.h X6Group)
struct X6Unit {
    int g, tile, c0, c1;
    bool whole;  // the tile's only slab: the conv writes the output itself
};
__device__ __forceinline__ X6Unit x6_unit_of(const X6Args& a, int u) {
    int g = 0;
    for (int i = 1; i < a.ngroups; ++i) g = u >= a.g[i].u0 ? i : g;
    const int S = a.g[g].slabs, ul = u - a.g[g].u0, tl = ul / S, s = ul - tl * S;
    return X6Unit{g, a.g[g].t0 + tl, s * a.nK / S, (s + 1) * a.nK / S, S == 1};
}

// the unit list of workgroup w of gridDim.x: positions [k0, k1) of `list` (nullptr: the units
// themselves, a contiguous range)
struct X6Work {
    int k0, k1;
    const int* list;
};
__device__ __forceinline__ X6Work x6_work_of(const X6Args& a, int w) {
    const int G = gridDim.x;
    if (a.sched) return X6Work{a.sched[w], a.sched[w + 1], a.sched + G + 1};
    return X6Work{(int)((long long)w * a.units / G), (int)((long long)(w + 1) * a.units / G), nullptr};
}

}  // namespace x6
using namespace x6;

}  // namespace opose
