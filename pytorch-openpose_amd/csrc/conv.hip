// conv.hip — implicit-GEMM convolution on the gfx950 fp32 matrix cores.
//
// Replaces the nn.Conv2d(+ReLU) / nn.MaxPool2d / torch.cat graph of
// hitmaxiang/pytorch-openpose src/model.py:7-22 (make_layers), :106-133 (body forward),
// :197-214 (hand forward).
//
// GEMM view of a stride-1 'same' convolution over a batch of NCHW frames:
//   out[m][p] = bias[m] + sum_k  W[m][k] * im2col[k][p]
//   m = output channel, p = (frame, y, x) flattened, k = (channel block, tap, channel).
// * A = weights, pre-transposed once at load time to Wt[Kpad][Mpad] (zero padded); a KC x MT
//   tile is KC rows of MT contiguous floats, copied to LDS by global_load_lds_dwordx4.
// * B = im2col gathered on the fly from the NCHW activation by buffer_load_dword ... lds:
//   every DMA covers one k row for 64 consecutive pixels (coalesced along x); zero padding
//   comes from the buffer range check (no branches, no register staging).
// * v_mfma_f32_32x32x2_f32: exact fp32 (bitwise an fmaf chain), 64 FLOP/clk/SIMD.  4 waves
//   (2x2) per workgroup for tiles up to 128x128, 8 waves of 64x64 for 128x256 / 256x128;
//   K is consumed in chunks of 32 through a double-buffered LDS tile (one barrier per chunk).
// * stream-K: the (tile, k-chunk) space is split evenly over the grid; tiles shared by
//   several workgroups leave fp32 partial slabs that conv_sk_fixup sums in k order
//   (deterministic), fusing bias + ReLU there.
// * epilogue fuses bias + ReLU and writes into a channel slice of a wider buffer, so the
//   reference's torch.cat([L1, L2, trunk]) (src/model.py:112-128) never materialises.
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace opose {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector (HIP's float4 class defeats SROA)
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int KC = 32;  // k rows per chunk
// waves per workgroup: 2 (M) x 2 (P) for tiles up to 128x128; 8 waves of 64x64 for the
// 128x256 / 256x128 tiles (one workgroup per CU: each 32-k weight tile in LDS feeds twice the
// MFMAs, or each gathered im2col row does)
constexpr int wg_waves(int mt, int pt) { return mt * pt >= 32768 ? 8 : 4; }

// TAP: K ordered (channel block of KC, tap, channel) with Cin padded to a multiple of KC -> one
// bounds check per pixel per chunk, a wave-uniform channel stride, and all taps of a channel
// block back to back, so a workgroup re-reads its shifted im2col rows from L2 (and L1) while
// they are resident (tap-outer order re-touched each channel after a full sweep of all
// channels -- 4 MB of live gathers per XCD, which thrashed L2).  Layers with Cin >= 32; else K is
// the OIHW flattening decoded through `ktab` (conv1_1: K = 27).
// KS: compile-time kernel size (1, 3, 7) so the tap decode folds; 0 = runtime a.ks.
template <int MT, int PT, bool TAP, int KS>
__global__ __launch_bounds__(64 * wg_waves(MT, PT), 8 / wg_waves(MT, PT)) void conv_igemm_f32(
    ConvArgs a, const int* __restrict__ ktab) {
    const int ks = KS ? KS : a.ks;
    constexpr int NW = wg_waves(MT, PT), NWM = NW == 8 ? MT / 64 : 2, NWP = NW / NWM;
    constexpr int WM = MT / NWM, WP = PT / NWP;
    constexpr int TM = WM / 32, TN = WP / 32;
    constexpr int PJ = PT / 64;             // pixel columns per lane
    constexpr int RW = KC / NW;             // k rows gathered per wave per chunk
    constexpr int A_SZ = KC * MT, B_SZ = KC * PT;
    constexpr int A_PW = A_SZ / 256 / NW;   // 1-KiB A pieces per wave per chunk

    // [2 stages][A tile KC x MT | B tile KC x PT] + bias; both tiles are filled by LDS-DMA
    // (buffer/global_load ... lds): no register staging, no ds_write pass.
    __shared__ __attribute__((aligned(16))) float lds[2 * (A_SZ + B_SZ) + MT];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hk = lane >> 5;
    const int nM = a.Mpad / MT, nP = (a.npix + PT - 1) / PT;
    const int nK = a.Kpad / KC;
    const int HW = a.H * a.W;
    const uint32_t HW4 = (uint32_t)HW * 4u;
    float* s_bias = lds + 2 * (A_SZ + B_SZ);
    const int wm0 = (wave % NWM) * WM;
    const int wp0 = (wave / NWM) * WP;

    // Stream-K: the (tile, k-chunk) iteration space is cut into gridDim.x equal contiguous
    // ranges, one per workgroup, so every CU gets the same work whatever the tile count
    // (a data-parallel grid of 472 tiles on 512 slots leaves 8 % of the chip idle and a
    // single-frame layer far more).  Ranges are XCD-contiguous (guide T1, bijective form):
    // tiles sharing im2col halo rows or a pixel tile's M-tiles share an L2.  A tile split over
    // several workgroups leaves float32 partials that conv_sk_fixup sums in k order.
    const int Gw = gridDim.x;
    const int id = xcd_contiguous_id(Gw, blockIdx.x);
    const long long I = (long long)nM * nP * a.ngroups * nK;
    const long long lo = (long long)id * I / Gw, hi = (long long)(id + 1) * I / Gw;

    // Segments run last-first: a range is [tail of tile t | whole tiles | head of tile t'], and
    // processing the head (k = 0 ..) before the tail (k = c0 ..) keeps every workgroup of an XCD
    // at nearly the same k chunk at the same time -- they then share each weight tile in L2
    // (forward order spreads the live k positions over the whole weight matrix: 3-6 MB, more
    // than an XCD's L2).  The partial slot stays tied to the range start (see conv_sk_fixup).
    for (long long itp = hi; itp > lo;) {
        const int tile = (int)((itp - 1) / nK);
        const int c_end = (int)(itp - (long long)tile * nK);
        const int c_begin = (int)max<long long>(0, lo - (long long)tile * nK);
        itp = (long long)tile * nK + c_begin;
        const int first = itp == lo;  // the segment holding the range start -> slot 2*id
        const int mt = tile % nM;
        const int rest = tile / nM;
        const int pt = rest % nP;
        const int g = rest / nP;
        const ConvGroup G = g == 0 ? a.g[0] : a.g[1];  // no dynamic kernarg indexing
        const int p0 = pt * PT;
        const int m0 = mt * MT;

        __syncthreads();  // the previous segment's epilogue is done with s_bias / the stages
        if (tid < MT) s_bias[tid] = (m0 + tid < G.cout) ? G.bias[m0 + tid] : 0.f;

        // ---- per-lane pixel state for the im2col gather.  The activation is read through a
        // buffer resource: an invalid (zero-padding) tap gets a byte offset >= num_records,
        // which the hardware range check turns into 0.0f -> the gather is branch free.
        const float* in_base = G.in + (size_t)G.in_coff * HW;
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc((void*)in_base, (short)0, (int)0x80000000u, 0x00020000);
        uint32_t poff[PJ];  // element offset of the lane's pixel (channel 0 of its frame)
        int py[PJ], px[PJ];
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
            int p = p0 + j * 64 + lane;
            const bool v = p < a.npix;
            int pc = v ? p : 0;
            int n = pc / HW;
            int r = pc - n * HW;
            py[j] = v ? r / a.W : -100000;  // out-of-range row => every tap invalid
            px[j] = r - (r / a.W) * a.W;
            poff[j] = (uint32_t)(n * G.in_cstride * HW + r);
        }

        floatx16 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        // per-chunk gather state (computed once per chunk)
        uint32_t base[PJ];
        int ch0 = 0;

        auto chunk_setup = [&](int c) __attribute__((always_inline)) {
            if constexpr (TAP) {
                const int taps = ks * ks;  // chunk c = (channel block, tap): wave-uniform scalars
                const int cb = c / taps;
                const int tap = c - cb * taps;
                ch0 = cb * KC + wave * RW;
                const int ky = tap / ks;
                const int dy = ky - a.pad, dx = tap - ky * ks - a.pad;
                const int shift = dy * a.W + dx;
#pragma unroll
                for (int j = 0; j < PJ; ++j) {
                    const int iy = py[j] + dy, ix = px[j] + dx;
                    const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                    // invalid taps start at 3 GiB: every row offset stays >= 2 GiB = num_records -> 0.0f
                    base[j] = ok ? (poff[j] + (uint32_t)shift) * 4u : 0xC0000000u;
                }
            }
        };
        // issue the LDS-DMA of B row r (this wave's) of chunk c into stage `buf`
        auto dma_b_row = [&](int c, int buf, int r) __attribute__((always_inline)) {
            float* Bs = lds + buf * (A_SZ + B_SZ) + A_SZ + (wave * RW + r) * PT;
            if constexpr (TAP) {
                const int ch = min(ch0 + r, a.Cin - 1);  // padded channels: any valid address (weights are 0)
                const uint32_t choff = (uint32_t)ch * HW4;
#pragma unroll
                for (int j = 0; j < PJ; ++j)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        rsrc, (lds_ptr_t)(Bs + j * 64), 4,
                        base[j] + choff, 0, 0, 0);
            } else {
                const int code = ktab[c * KC + wave * RW + r];  // (c << 8) | (ky << 4) | kx
                const int cch = code >> 8;
                const int dy = ((code >> 4) & 15) - a.pad;
                const int dx = (code & 15) - a.pad;
                const int delta = cch * HW + dy * a.W + dx;
#pragma unroll
                for (int j = 0; j < PJ; ++j) {
                    const int iy = py[j] + dy, ix = px[j] + dx;
                    const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                    const uint32_t off = ok ? (poff[j] + (uint32_t)delta) * 4u : 0xC0000000u;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(Bs + j * 64), 4, off, 0, 0, 0);
                }
            }
        };
        auto dma_a = [&](int c, int buf) __attribute__((always_inline)) {
            const int k0 = c * KC;
            float* As = lds + buf * (A_SZ + B_SZ);
#pragma unroll
            for (int i = 0; i < A_PW; ++i) {
                const int piece = wave * A_PW + i;
                const int f = piece * 256 + lane * 4;
                const int row = f / MT, col = f - row * MT;
                __builtin_amdgcn_global_load_lds((const void*)(G.wt + (size_t)(k0 + row) * a.Mpad + m0 + col),
                                                 (lds_ptr_t)(As + piece * 256), 16, 0, 0);
            }
        };

        chunk_setup(c_begin);
        dma_a(c_begin, 0);
#pragma unroll
        for (int r = 0; r < RW; ++r) dma_b_row(c_begin, 0, r);
        __syncthreads();  // s_waitcnt vmcnt(0) + barrier: stage 0 landed for every wave
        for (int c = c_begin; c < c_end; ++c) {
            const int buf = (c - c_begin) & 1;
            // the last chunk re-issues its own DMA into the free stage instead of branching:
            // a branch-free loop body lets the compiler keep the LDS reads 2 deep (lgkmcnt(2))
            const int cn = min(c + 1, c_end - 1);
            chunk_setup(cn);
            dma_a(cn, buf ^ 1);
            // Fragment reads are explicit ds_read_b32 with immediate offsets and counted waits:
            // the reads of k-step ks+1 are issued in front of k-step ks's MFMAs and waited for
            // with lgkmcnt(TM+TN) (LDS returns in order), so they have a whole k-step to land.
            // (Compiler-visible reads get lgkmcnt(0) once LDS-DMA is in flight, which stalls
            // the wave on the reads it has only just issued.)
            const uint32_t a_lds = (uint32_t)(uintptr_t)(lds_ptr_t)(lds + buf * (A_SZ + B_SZ) + wm0 + l31 + hk * MT);
            const uint32_t b_lds =
                (uint32_t)(uintptr_t)(lds_ptr_t)(lds + buf * (A_SZ + B_SZ) + A_SZ + wp0 + l31 + hk * PT);
            float av[2][TM], bv[2][TN];
            auto read_frags = [&](int step, float (&fa)[TM], float (&fb)[TN]) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    asm volatile("ds_read_b32 %0, %1 offset:%2"
                                 : "=v"(fa[i])
                                 : "v"(a_lds), "i"((2 * step * MT + i * 32) * 4));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    asm volatile("ds_read_b32 %0, %1 offset:%2"
                                 : "=v"(fb[j])
                                 : "v"(b_lds), "i"((2 * step * PT + j * 32) * 4));
            };
            read_frags(0, av[0], bv[0]);
#pragma unroll
            for (int ks2 = 0; ks2 < KC / 2; ++ks2) {
                const int cur = ks2 & 1, nxt = cur ^ 1;
                if (ks2 + 1 < KC / 2) read_frags(ks2 + 1, av[nxt], bv[nxt]);
                if (ks2 < RW) dma_b_row(cn, buf ^ 1, ks2);
                // wait for this step's fragments only (the next step's stay in flight); the "+v"
                // operands order the MFMAs after the wait
                if (ks2 + 1 < KC / 2) asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(TM + TN));
                else asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
                for (int i = 0; i < TM; ++i) asm volatile("" : "+v"(av[cur][i]));
#pragma unroll
                for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(bv[cur][j]));
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i], bv[cur][j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();  // next stage landed everywhere; this stage free
        }

        // ---- epilogue: whole tile -> bias + ReLU into the channel slice; part of a tile ->
        // float32 partial slab [MT][PT] in slot 2*id (first segment) or 2*id+1 (last)
        const bool whole = c_begin == 0 && c_end == nK;
        float* slab = a.partial + (size_t)(2 * id + (first ? 0 : 1)) * (MT * PT);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int pl = wp0 + j * 32 + l31;
            const int p = p0 + pl;
            if (!whole) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ml = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
                        // sc1: device-scope store, written through to the coherence point so
                        // the workgroup that reduces the tile (maybe on another XCD) sees it
                        asm volatile("global_store_dword %0, %1, off sc1" ::"v"(slab + ml * PT + pl),
                                     "v"(acc[i][j][r])
                                     : "memory");
                    }
                continue;
            }
            if (p >= a.npix) continue;
            const int n = p / HW;
            const int rem = p - n * HW;
            float* ob = G.out + ((size_t)n * G.out_cstride + G.out_coff) * HW + rem;
            float* ob2 = G.out2 ? G.out2 + ((size_t)n * G.out2_cstride + G.out2_coff) * HW + rem : nullptr;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
                    if (m < G.cout) {
                        float v = acc[i][j][r] + s_bias[m - m0];
                        if (G.relu) v = fmaxf(v, 0.f);
                        ob[(size_t)m * HW] = v;
                        if (ob2) ob2[(size_t)m * HW] = v;
                    }
                }
        }
    }
}

// Stream-K fixup: grid (tiles, MT*PT/1024); each thread finishes 4 consecutive pixels of one
// output channel of a tile that several workgroups shared: partial slabs summed in k order
// (deterministic), + bias, ReLU, written into the channel slice.
template <int MT, int PT>
__global__ __launch_bounds__(256) void conv_sk_fixup(ConvArgs a) {
    const int nM = a.Mpad / MT, nP = (a.npix + PT - 1) / PT;
    const int nK = a.Kpad / KC;
    const long long Gw = a.sk_grid;
    const long long I = (long long)nM * nP * a.ngroups * nK;
    const int tile = blockIdx.x;
    const long long x0 = (long long)tile * nK;
    const int w0 = (int)(((x0 + 1) * Gw - 1) / I);       // workgroup whose range holds x0
    const int w1 = (int)(((x0 + nK) * Gw - 1) / I);      // ... holds the tile's last chunk
    if (w0 == w1) return;  // one workgroup computed the whole tile and wrote it directly
    const int mt = tile % nM;
    const int rest = tile / nM;
    const int pt = rest % nP;
    const int g = rest / nP;
    const ConvGroup G = g == 0 ? a.g[0] : a.g[1];
    const int HW = a.H * a.W;
    const int e = (blockIdx.y * 256 + threadIdx.x) * 4;
    const int ml = e / PT, pl = e - ml * PT;
    const int m = mt * MT + ml;
    if (m >= G.cout) return;
    f32x4 v;
    for (int w = w0; w <= w1; ++w) {
        const long long lo_w = (long long)w * I / Gw;
        const int slot = (lo_w / nK == tile) ? 2 * w : 2 * w + 1;
        const f32x4 part = *reinterpret_cast<const f32x4*>(a.partial + (size_t)slot * (MT * PT) + e);
        v = (w == w0) ? part : v + part;
    }
    const float bias = G.bias[m];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = pt * PT + pl + k;
        if (p >= a.npix) break;
        float o = v[k] + bias;
        if (G.relu) o = fmaxf(o, 0.f);
        const int n = p / HW;
        const int rem = p - n * HW;
        G.out[((size_t)n * G.out_cstride + G.out_coff + m) * HW + rem] = o;
        if (G.out2) G.out2[((size_t)n * G.out2_cstride + G.out2_coff + m) * HW + rem] = o;
    }
}

// fills a buffer with a cheap hash in [-1, 1) (timing runs must not run on zeros: DVFS)
__global__ void fill_hash(float* p, size_t n, uint32_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t h = (uint32_t)i * 2654435761u ^ seed;
        h ^= h >> 15;
        h *= 2246822519u;
        h ^= h >> 13;
        const float v = (float)(h & 0xffffff) / 8388608.f - 1.f;
        p[i] = (seed & 0x80000000u) ? fmaxf(v, 0.f) : v;  // top seed bit: ReLU-like (half zeros)
    }
}

void launch_fill_hash(float* p, size_t n, uint32_t seed, hipStream_t st) {
    hipLaunchKernelGGL(fill_hash, dim3(2048), dim3(256), 0, st, p, n, seed);
}

// MaxPool2d(2, 2), floor mode (src/model.py:10-13); NCHW, C channels contiguous planes.
__global__ __launch_bounds__(256) void maxpool2x2(const float* __restrict__ in, float* __restrict__ out,
                                                  int NC, int H, int W) {
    const int Ho = H >> 1, Wo = W >> 1;
    const size_t total = (size_t)NC * Ho * Wo;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % Wo);
        const size_t t = e / Wo;
        const int y = (int)(t % Ho);
        const size_t nc = t / Ho;
        const float* s = in + (nc * H + 2 * y) * W + 2 * x;
        out[e] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1]));
    }
}

// ------------------------------------------------------------------ host launchers
template <int MT, int PT>
static void launch_tile(const ConvArgs& a, const int* ktab, hipStream_t st) {
    const dim3 grid(a.sk_grid);
    constexpr int NTH = 64 * wg_waves(MT, PT);
    if (!a.tap_major)
        hipLaunchKernelGGL((conv_igemm_f32<MT, PT, false, 0>), grid, dim3(NTH), 0, st, a, ktab);
    else if (a.ks == 7)
        hipLaunchKernelGGL((conv_igemm_f32<MT, PT, true, 7>), grid, dim3(NTH), 0, st, a, ktab);
    else if (a.ks == 3)
        hipLaunchKernelGGL((conv_igemm_f32<MT, PT, true, 3>), grid, dim3(NTH), 0, st, a, ktab);
    else if (a.ks == 1)
        hipLaunchKernelGGL((conv_igemm_f32<MT, PT, true, 1>), grid, dim3(NTH), 0, st, a, ktab);
    else
        hipLaunchKernelGGL((conv_igemm_f32<MT, PT, true, 0>), grid, dim3(NTH), 0, st, a, ktab);
    const int tiles = (a.Mpad / MT) * ((a.npix + PT - 1) / PT) * a.ngroups;
    if (a.sk_grid != tiles)
        hipLaunchKernelGGL((conv_sk_fixup<MT, PT>), dim3(tiles, MT * PT / 1024), dim3(256), 0, st, a);
}

void launch_conv(const ConvArgs& a, const int* ktab, int mt, int pt, hipStream_t st) {
    if (mt == 128 && pt == 128) launch_tile<128, 128>(a, ktab, st);
    else if (mt == 128 && pt == 256) launch_tile<128, 256>(a, ktab, st);
    else if (mt == 256 && pt == 128) launch_tile<256, 128>(a, ktab, st);
    else if (mt == 128 && pt == 64) launch_tile<128, 64>(a, ktab, st);
    else if (mt == 64 && pt == 128) launch_tile<64, 128>(a, ktab, st);
    else if (mt == 64 && pt == 64) launch_tile<64, 64>(a, ktab, st);
    else throw std::invalid_argument("unsupported conv tile");
}

void launch_maxpool(const float* in, float* out, int NC, int H, int W, hipStream_t st) {
    size_t total = (size_t)NC * (H / 2) * (W / 2);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(maxpool2x2, dim3(blocks), dim3(256), 0, st, in, out, NC, H, W);
}

}  // namespace opose
