// x6_loop.h — the six-block chunk loop of conv_x6 and conv_win_x6: the fragment registers, their
// refill order and the waits that make it correct.  This is the description both kernels follow;
// conv_win_x6 runs the code below, conv_x6 still spells the same schedule out (conv_x6.hip says
// why), so a change here is repeated there.
//
// A chunk (32 k) is one v_mfma_f32_16x16x32_bf16 k-step.  Lane l holds row / pixel (l & 15) and
// k-group (l >> 4) of its 16-row blocks; a wave owns TM x TN accumulator blocks and one fragment
// set: fa[piece][i], fb[piece][j], each a ds_read_b128 from an LDS tile of [piece][group][row]
// units (16-lane phases hit 4 rows of each of 4 groups: conflict free).  The six piece products
// (x6.h kPieceA / kPieceB) run as blocks of TM * TN MFMAs,
//     (0,2) (0,0) (0,1) | barrier | (1,0) (2,0) (1,1)
// and each piece's registers are refilled with the next chunk's fragments right after their last
// use in this one -- refill group R0 = A0, B2 (after block 2, read during block 3), R1 = B0, A2
// (after block 4, during block 5), R2 = B1, A1 (in the next chunk's block 0) -- one read per MFMA
// gap, the order pinned by sched_barrier.  The barrier sits after block 2: by then every wave has
// read this chunk's stage (R2 is waited for before block 2), and the caller's VMCNT says how many
// of the wave's newest LDS-DMA instructions may still be in flight once the next stage has
// landed.  After the barrier the stage just read is free: blocks 3-5 interleave the next chunk's
// R0 (block 3) and R1 (block 5) reads with the kernel's own filler operations, the LDS-DMA that
// refills the stage.
//
// Here: the fragment set (rd / mf / fence_all), blocks 0-2 with every lgkmcnt wait (head) and
// the barrier with its vmcnt.  Blocks 3-5 stay in the kernel, a dozen lines on top of rd and mf:
// with the fillers handed to a shared function as callables, the generated code swapped the last
// MFMA of blocks 3 and 5 with the LDS-DMA next to it.
#pragma once
#include "x6.h"

namespace opose {
namespace x6 {

// B fragment addressing: addr(j) is the LDS byte address for block j, off(pc, j) the immediate
// added for piece pc.  conv_win_x6: a pixel unit per block in a window of WMAX units a piece
template <int TN, int WMAX>
struct X6BWin {
    uint32_t a[TN];
    __device__ __forceinline__ uint32_t addr(int j) const { return a[j]; }
    static constexpr int off(int pc, int) { return pc * WMAX * 16; }
};

// The fragment set and accumulators of a wave's TM x TN blocks of an MT-row tile
template <int MT, int TM, int TN>
struct X6Frags {
    static constexpr int NB = TM * TN;   // MFMAs per block
    static constexpr int TMN = TM + TN;  // reads per refill group
    i32x4 fa[3][TM], fb[3][TN];
    f32x4 acc[TM][TN];

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // refill group g (0: A0 B2, 1: B0 A2, 2: B1 A1), read r of TMN; A from the stage at abase
    template <class B>
    __device__ __forceinline__ void rd(int g, int r, uint32_t abase, const B& b) {
        const bool isA = g == 0 ? r < TM : r >= TN;
        const int k = g == 0 ? (r < TM ? r : r - TM) : (r < TN ? r : r - TN);
        const int pc = g == 0 ? (isA ? 0 : 2) : g == 1 ? (isA ? 2 : 0) : 1;
        if (isA)
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fa[pc][k]) : "v"(abase), "i"((pc * 4 * MT + 16 * k) * 16));
        else
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[pc][k]) : "v"(b.addr(k)), "i"(B::off(pc, k)));
    }
    template <class B>
    __device__ __forceinline__ void rd_group(int g, uint32_t abase, const B& b) {
#pragma unroll
        for (int r = 0; r < TMN; ++r) rd(g, r, abase, b);
    }
    __device__ __forceinline__ void mf(int t, int q) {
        const int i = q / TN, j = q % TN;
        acc[i][j] = mfma_x6(fa[kPieceA[t]][i], fb[kPieceB[t]][j], acc[i][j]);
    }
    // the asm reads' results are used from here on (after the wait in front of it)
    __device__ __forceinline__ void fence_all() {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
#pragma unroll
            for (int i = 0; i < TM; ++i) asm volatile("" : "+v"(fa[pc][i]));
#pragma unroll
            for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(fb[pc][j]));
        }
    }

    // Blocks 0-2 of a chunk, up to the barrier's wait.  On entry R0 and R1 of the chunk are in flight
    // or landed (issued by the previous chunk's tail or the prologue).  (a_cur, b_cur): the chunk's A
    // stage and B addresses, for its R2 reads.
    template <class B>
    __device__ __forceinline__ void head(uint32_t a_cur, const B& b_cur) {
        // block 0 (needs R0): R2 of this chunk interleaved
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(TMN > 15 ? 15 : TMN) : "memory");
        fence_all();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            mf(0, q);
#pragma unroll
            for (int r = q * TMN / NB; r < (q + 1) * TMN / NB; ++r) rd(2, r, a_cur, b_cur);
            __builtin_amdgcn_sched_barrier(0);
        }
        // block 1 (needs R1)
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(TMN > 15 ? 15 : TMN) : "memory");
        fence_all();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            mf(1, q);
            __builtin_amdgcn_sched_barrier(0);
        }
        // block 2 (needs R2)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        fence_all();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            mf(2, q);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // The chunk's barrier: this stage read by all, the next stage landed -- all but the wave's
    // VMCNT newest LDS-DMA instructions.  The vmcnt is explicit: the compiler does not count LDS-DMA
    // as LDS writes at a workgroup barrier (it emitted a bare s_barrier here), and the fragment
    // reads are inline asm it cannot see.
    template <int VMCNT>
    __device__ __forceinline__ void barrier() {
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(VMCNT) : "memory");
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
    }
};

}  // namespace x6
}  // namespace opose
