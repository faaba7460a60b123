// shapelet.hip — shapelet search over motion data: MotionMat rows to joint features, the sliding
// distance of a window against ragged sequences, and the selection of the window that separates
// the labels best.
//
// Reference steps replaced (hitmaxiang/pytorch-openpose):
//  * srcmx/PreprocessingData.py:16-125   MotionJointFeatures (ProcessingTheNonValue,
//    CorrespondingValue, the nose-neck scale)        => feat_blocklast, feat_carry, feat_compute
//  * srcmx/utilmx.py:330-372             SlidingDistance(_torch)          => sliding_distance
//  * srcmx/utilmx.py:375-391 + srcmx/shapeletmodel.py:140-152  matrixprofile_torch and the
//    per-sample torch.min, for every window length of srcmx/shapeletlearning.py:123-175's loop at
//    once                                                                 => shapelet_mindist
//  * srcmx/shapeletmodel.py:157-209      Bipartition_score, the loss and the best-candidate update
//                                                                         => shapelet_score, shapelet_select
//  * srcmx/DataAugmentation.py:106-150   AugmentateOneShapelet's sliding distances, hits below
//    sigma and the thinning of neighbouring hits   => shapelet_scan_dist, shapelet_scan_pick
//
// The distance rule (fp32, one rounding per operation; this file is built without FMA contraction):
//   e(a, b) = sum over d ascending of (x[a,d] - y[b,d])^2, from +0
//   s(r, c) = sum over k ascending of e(r+k, c+k), from +0;  dist = sqrt(s)
// and a minimum over c is the first minimum of s.  s is never negative, so its bit pattern as an
// unsigned integer orders like its value.  The reference's running recurrence (add the new term,
// subtract the old) is not used: every s is the direct sum.
//
// Every address below derives from the validated integers of the call (off, m, D, the block table
// the host builds from them), never from a data value.
#include "common.h"
#include "kernels.h"
#include "shapelet.h"

namespace opose {

// the sequence a global row belongs to: the last j < n_seq with off[j] <= g (sequences may be empty)
__device__ inline int seq_of_row(const int64_t* __restrict__ off, int n_seq, int64_t g) {
    int lo = 0, hi = n_seq;  // off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------ features
// x or y of a joint, as float32: column c = 2 * joint + (0: x, 1: y) of a row of `joints` joints
__device__ inline float feat_load(const double* __restrict__ motion, int64_t row, int joints, int c) {
    return (float)motion[(row * joints + (c >> 1)) * 3 + (c & 1)];
}

// last[b][c]: the last row of fill block b whose column c is not zero, -1: none
__global__ __launch_bounds__(kFeatThreads) void feat_blocklast(const double* __restrict__ motion, int64_t L, int joints,
                                                               int nblocks, int32_t* __restrict__ last) {
    const int C = 2 * joints;
    const int64_t i = (int64_t)blockIdx.x * kFeatThreads + threadIdx.x;
    if (i >= (int64_t)nblocks * C) return;
    const int b = (int)(i / C), c = (int)(i % C);
    const int64_t r0 = (int64_t)b * kFeatRows;
    const int64_t r1 = min(r0 + kFeatRows, L);
    int32_t res = -1;
    for (int64_t r = r1 - 1; r >= r0; --r)
        if (feat_load(motion, r, joints, c) != 0.0f) {
            res = (int32_t)r;
            break;
        }
    last[i] = res;
}

// in place, per column: last[b][c] becomes the last non-zero row of the blocks before b (the carry)
__global__ __launch_bounds__(kFeatThreads) void feat_carry(int32_t* __restrict__ last, int nblocks, int C) {
    const int c = blockIdx.x * kFeatThreads + threadIdx.x;
    if (c >= C) return;
    int32_t run = -1;
    for (int b = 0; b < nblocks; ++b) {
        const int32_t own = last[(size_t)b * C + c];
        last[(size_t)b * C + c] = run;
        if (own >= 0) run = own;
    }
}

// One workgroup per fill block.  The block's filled x / y values go to LDS (modes 0, 1: a thread per
// column walks the block's rows from the carry, and a carry from before the row's own sequence does
// not count; mode 2: the first non-zero of rows r-1, r+1, r-2, r+2 of the sequence), then every
// output of the block is formed from them.  out [L][F][2], F = 6 or 46.
__global__ __launch_bounds__(kFeatThreads) void feat_compute(const double* __restrict__ motion, int64_t L, int joints,
                                                             const int64_t* __restrict__ off, int n_seq, int mode,
                                                             const int32_t* __restrict__ carry,
                                                             float* __restrict__ out) {
    __shared__ float vals[kFeatRows][120];
    __shared__ int64_t row_lo[kFeatRows], row_hi[kFeatRows];
    const int C = 2 * joints, t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kFeatRows;
    const int rows = (int)min((int64_t)kFeatRows, L - r0);
    if (t < rows) {
        const int j = seq_of_row(off, n_seq, r0 + t);
        row_lo[t] = off[j];
        row_hi[t] = off[j + 1];
    }
    __syncthreads();
    if (mode == 2) {
        for (int i = t; i < rows * C; i += kFeatThreads) {
            const int r = i / C, c = i % C;
            const int64_t g = r0 + r;
            float v = feat_load(motion, g, joints, c);
            if (v == 0.0f) {
                for (int s = 1; s <= 2; ++s) {
                    float u = 0.0f;
                    if (g - s >= row_lo[r]) u = feat_load(motion, g - s, joints, c);
                    if (u == 0.0f && g + s < row_hi[r]) u = feat_load(motion, g + s, joints, c);
                    if (u != 0.0f) {
                        v = u;
                        break;
                    }
                }
            }
            vals[r][c] = v;
        }
    } else if (t < C) {
        int64_t last = carry[(size_t)blockIdx.x * C + t];
        float lastv = last >= 0 ? feat_load(motion, last, joints, t) : 0.0f;
        for (int r = 0; r < rows; ++r) {
            float v = feat_load(motion, r0 + r, joints, t);
            if (v != 0.0f) {
                last = r0 + r;
                lastv = v;
            } else if (last >= row_lo[r]) {
                v = lastv;
            }
            vals[r][t] = v;
        }
    }
    __syncthreads();
    const int F = joints == 18 ? 6 : 46;
    for (int i = t; i < rows * F * 2; i += kFeatThreads) {
        const int r = i / (2 * F), f = (i >> 1) % F, k = i & 1;
        int joint, origin;
        if (f < 6) {
            joint = 2 + f;
            origin = 1;
        } else if (f < 26) {
            joint = 19 + (f - 6);
            origin = 18;
        } else {
            joint = 40 + (f - 26);
            origin = 39;
        }
        float vj = vals[r][2 * joint + k];
        const float vo = vals[r][2 * origin + k];
        if (mode == 2 && vj == 0.0f) vj = vo;
        float v = vj - vo;
        if (mode >= 1) {
            float nose = vals[r][1];
            const float neck = vals[r][3];
            if (mode == 2 && nose == 0.0f) nose = neck;
            const float scale = (nose - neck) + 1e-5f;
            v = v / scale;
        }
        out[((r0 + r) * F + f) * 2 + k] = v;
    }
}

void launch_motion_features(const double* motion, int64_t L, int joints, const int64_t* off, int n_seq, int mode,
                            int32_t* carry, float* out, hipStream_t st) {
    const int nblocks = (int)((L + kFeatRows - 1) / kFeatRows);
    const int C = 2 * joints;
    if (mode != 2) {
        const int64_t n = (int64_t)nblocks * C;
        hipLaunchKernelGGL(feat_blocklast, dim3((unsigned)((n + kFeatThreads - 1) / kFeatThreads)), dim3(kFeatThreads), 0,
                           st, motion, L, joints, nblocks, carry);
        hipLaunchKernelGGL(feat_carry, dim3((C + kFeatThreads - 1) / kFeatThreads), dim3(kFeatThreads), 0, st, carry,
                           nblocks, C);
    }
    hipLaunchKernelGGL(feat_compute, dim3(nblocks), dim3(kFeatThreads), 0, st, motion, L, joints, off, n_seq, mode, carry,
                       out);
}

// ------------------------------------------------------------------------------------ profile mode
// One thread per row of the batch: position c of its sequence, when the sequence has one there.
// dist is ragged, P_j values per sequence: sequence j starts at off[j] - j * (m - 1).
__global__ __launch_bounds__(kShpThreads) void sliding_distance(const float* __restrict__ pat, int m,
                                                                const float* __restrict__ seq,
                                                                const int64_t* __restrict__ off, int n_seq, int D,
                                                                float* __restrict__ dist) {
    const int64_t g = (int64_t)blockIdx.x * kShpThreads + threadIdx.x;
    if (g >= off[n_seq]) return;
    const int j = seq_of_row(off, n_seq, g);
    if (g + m > off[j + 1]) return;  // fewer than m rows left in the sequence
    float acc = 0.0f;
    for (int k = 0; k < m; ++k) {
        const float* x = pat + (size_t)k * D;
        const float* y = seq + (g + k) * D;
        float e = 0.0f;
        for (int d = 0; d < D; ++d) {
            const float t = x[d] - y[d];
            e = e + t * t;
        }
        acc = acc + e;
    }
    dist[g - (int64_t)j * (m - 1)] = sqrtf(acc);
}

void launch_sliding_distance(const float* pat, int m, const float* seq, const int64_t* off, int n_seq, int D, int64_t L,
                             float* dist, hipStream_t st) {
    hipLaunchKernelGGL(sliding_distance, dim3((unsigned)((L + kShpThreads - 1) / kShpThreads)), dim3(kShpThreads), 0, st,
                       pat, m, seq, off, n_seq, D, dist);
}

// ------------------------------------------------------------------------------------ mindist mode
// shapelet_mindist, workgroup (block table entry, target sequence j): for the entry's candidate
// starts r and each window length m_0 < m_1 < ... < m_{n-1} of `lens` (1 <= n <= kShpMaxLens), the
// min over c of s(r, c) and its first c.  Per block of kShpTC target positions:
//   1. E[a][q] = e(a, a + q - (kShpTR - 1)) for the rows a of the candidate window rows and the
//      diagonals q that the tile's outputs use -- a band, not the square -- accumulated in LDS while
//      D streams through the staging tiles xs / ys in chunks of kShpDC, d ascending;
//   2. s(r, c) = E[r][q] + E[r+1][q] + ... along its diagonal, k ascending from +0, one walk per
//      (start, position) for every length: E does not depend on m, so the partial sum after m_l
//      terms is, bit for bit, the s of length m_l, a snapshot compared against that length's
//      running (min, loc), which a thread keeps in registers for its positions c = sub,
//      sub + kShpSub, ...
// The block table is that of m_0, which has the most starts, and the band is sized for m_{n-1}; a
// start or position is compared at length m_l only when its m_l rows lie within its clip
// (blk.r0 + r + m_l <= len_i, c0 + c + m_l <= len_j), and as the lengths ascend the first that does
// not fit ends the walk, so no E entry beyond the two clips is read.  Position blocks ascend, so a
// strict < keeps a thread's first minimum.  The running pairs are kShpMaxLens scalars per thread
// (the loops over l are fully unrolled: never an indexed array); the kShpSub threads of a start
// are neighbouring lanes and merge on (bits, loc) by lane exchange.  No atomics: a result does not
// depend on scheduling.  Length l's rows go to rows[entry][l].out0 .. of min2 / loc.  LDS is
// dynamic: E [na][kShpND], xs [na][kShpDC + 1], ys [nb][kShpDC + 1] with na = kShpTR + m_max - 1,
// nb = kShpTC + m_max - 1.
constexpr int kShpND = kShpTR + kShpTC - 1;  // diagonals of a tile
constexpr size_t shp_lds_bytes(int m_max) {
    const int na = kShpTR + m_max - 1, nb = kShpTC + m_max - 1;
    return sizeof(float) * ((size_t)na * kShpND + (size_t)(na + nb) * (kShpDC + 1));
}
static_assert(kShpThreads == kShpTR * kShpSub, "threads = starts x sub-positions");
static_assert(kShpSub <= 64 && (kShpSub & (kShpSub - 1)) == 0 && 64 % kShpSub == 0, "a start's threads share a wave");
static_assert(shp_lds_bytes(kShpMaxM) <= 65536, "dynamic LDS within what a launch gets without an attribute call");

// Step 1 of a position block: the band E (na rows of kShpND diagonals) of candidate rows
// xo .. xo + xrows - 1 against target rows yo + c0 .. (nb of them, as far as the target's ylen rows
// reach), through the staging tiles xs [na][kShpDC + 1] and ys [nb][kShpDC + 1].  An entry is
// accumulated by one thread, d ascending; an entry of a row beyond xrows or ylen stays +0 and no
// row outside the two clips is read.  Ends before the barrier that makes E visible.
__device__ inline void shp_fill_band(float* __restrict__ E, float* __restrict__ xs, float* __restrict__ ys,
                                     const float* __restrict__ seq, int64_t xo, int xrows, int64_t yo, int ylen,
                                     int c0, int na, int nb, int D, int t) {
    const int nent = na * kShpND;
    for (int e = t; e < nent; e += kShpThreads) E[e] = 0.0f;
    for (int d0 = 0; d0 < D; d0 += kShpDC) {
        const int dc = min(kShpDC, D - d0);
        __syncthreads();  // the previous chunk's readers are done
        for (int i = t; i < na * kShpDC; i += kShpThreads) {
            const int a = i / kShpDC, d = i % kShpDC;
            xs[a * (kShpDC + 1) + d] = (a < xrows && d < dc) ? seq[(xo + a) * D + d0 + d] : 0.0f;
        }
        for (int i = t; i < nb * kShpDC; i += kShpThreads) {
            const int b = i / kShpDC, d = i % kShpDC;
            ys[b * (kShpDC + 1) + d] = (c0 + b < ylen && d < dc) ? seq[(yo + c0 + b) * D + d0 + d] : 0.0f;
        }
        __syncthreads();
        for (int e = t; e < nent; e += kShpThreads) {  // an entry stays with its thread
            const int a = e / kShpND, b = a + e % kShpND - (kShpTR - 1);
            if (a >= xrows || b < 0 || b >= nb || c0 + b >= ylen) continue;  // no output reads it
            const float* x = xs + a * (kShpDC + 1);
            const float* y = ys + b * (kShpDC + 1);
            float acc = E[e];
            for (int d = 0; d < dc; ++d) {
                const float v = x[d] - y[d];
                acc = acc + v * v;
            }
            E[e] = acc;
        }
    }
}

__global__ __launch_bounds__(kShpThreads) void shapelet_mindist(
    const float* __restrict__ seq, const int64_t* __restrict__ off, int n_seq, int D, const ShpLens lens,
    const ShpBlock* __restrict__ blocks, const ShpLenRows* __restrict__ rows, float* __restrict__ min2,
    int32_t* __restrict__ loc) {
    extern __shared__ float shp_lds[];
    const int t = threadIdx.x, j = blockIdx.y;
    const int m0 = lens.m[0], mx = lens.m[lens.n - 1];
    const int na = kShpTR + mx - 1, nb = kShpTC + mx - 1;
    float* E = shp_lds;
    float* xs = E + na * kShpND;
    float* ys = xs + na * (kShpDC + 1);
    const ShpBlock blk = blocks[blockIdx.x];
    const int64_t xo = off[blk.seq] + blk.r0;
    const int xleft = (int)(off[blk.seq + 1] - xo);     // rows of the candidate clip from the entry's first start on
    const int xrows = min(blk.nvalid + mx - 1, xleft);  // the window rows a valid output may read
    const int64_t yo = off[j];
    const int ylen = (int)(off[j + 1] - yo), P0 = ylen - m0 + 1;
    const int r = t / kShpSub, sub = t % kShpSub;
    uint32_t best[kShpMaxLens];
    int bloc[kShpMaxLens];
#pragma unroll
    for (int l = 0; l < kShpMaxLens; ++l) {
        best[l] = 0xffffffffu;
        bloc[l] = 0;
    }
    for (int c0 = 0; c0 < P0; c0 += kShpTC) {
        shp_fill_band(E, xs, ys, seq, xo, xrows, yo, ylen, c0, na, nb, D, t);
        __syncthreads();
        if (r < blk.nvalid) {
            for (int c = sub; c < kShpTC && c0 + c < P0; c += kShpSub) {
                const float* diag = E + r * kShpND + (c - r + kShpTR - 1);
                const int fit = min(xleft - r, ylen - (c0 + c));  // the longest window that fits both clips here
                float acc = 0.0f;
                int k = 0;
                bool go = true;
#pragma unroll
                for (int l = 0; l < kShpMaxLens; ++l) {
                    go = go && l < lens.n && lens.m[l] <= fit;
                    if (go) {
                        for (; k < lens.m[l]; ++k) acc = acc + diag[k * kShpND];
                        const uint32_t bits = __float_as_uint(acc);
                        if (bits < best[l]) {
                            best[l] = bits;
                            bloc[l] = c0 + c;
                        }
                    }
                }
            }
        }
        __syncthreads();  // E is zeroed next
    }
#pragma unroll
    for (int l = 0; l < kShpMaxLens; ++l) {
        if (l < lens.n) {  // uniform: every lane of the wave exchanges
            uint32_t b = best[l];
            int bl = bloc[l];
#pragma unroll
            for (int s = 1; s < kShpSub; s <<= 1) {
                const uint32_t ob = (uint32_t)__shfl_xor((int)b, s);
                const int ol = __shfl_xor(bl, s);
                if (ob < b || (ob == b && ol < bl)) {
                    b = ob;
                    bl = ol;
                }
            }
            const ShpLenRows lr = rows[(size_t)blockIdx.x * lens.n + l];
            if (sub == 0 && r < lr.nvalid) {
                const size_t o = (size_t)(lr.out0 + r) * n_seq + j;
                min2[o] = __uint_as_float(b);
                loc[o] = bl;
            }
        }
    }
}

void launch_shapelet_mindist(const float* seq, const int64_t* off, int n_seq, int D, const ShpLens& lens,
                             const ShpBlock* blocks, const ShpLenRows* rows, int n_blocks, float* min2, int32_t* loc,
                             hipStream_t st) {
    hipLaunchKernelGGL(shapelet_mindist, dim3(n_blocks, n_seq), dim3(kShpThreads), shp_lds_bytes(lens.m[lens.n - 1]), st,
                       seq, off, n_seq, D, lens, blocks, rows, min2, loc);
}

// ------------------------------------------------------------------------------------ score
// One workgroup per candidate row of min2 [n_cand][n_seq].  n_seq is n_labels, or 2 * n_labels with
// sequence k + n_labels the mirrored copy of k: sample k's key is then the smaller s of the pair,
// the original on a tie.  The samples are ordered by (bits of s, k) through a rank count, and
//   num  = max over t = 0 .. n_labels of negs + (positives - negatives among the first t)
//   loss = float64 sum, k ascending, of (double) sqrt(s_k) over the positive samples' own
//          (unmirrored) values, divided by their count.
__global__ __launch_bounds__(kShpThreads) void shapelet_score(const float* __restrict__ min2, int n_seq, int n_labels,
                                                              const uint8_t* __restrict__ labels, int negs,
                                                              int32_t* __restrict__ num, double* __restrict__ loss) {
    __shared__ uint32_t key[kShpMaxSeq];
    __shared__ uint8_t sorted[kShpMaxSeq];
    const int t = threadIdx.x;
    const float* row = min2 + (size_t)blockIdx.x * n_seq;
    for (int k = t; k < n_labels; k += kShpThreads) {
        uint32_t b = __float_as_uint(row[k]);
        if (n_seq == 2 * n_labels) {
            const uint32_t b2 = __float_as_uint(row[k + n_labels]);
            if (b2 < b) b = b2;
        }
        key[k] = b;
    }
    __syncthreads();
    for (int k = t; k < n_labels; k += kShpThreads) {
        const uint32_t mine = key[k];
        int rank = 0;
        for (int o = 0; o < n_labels; ++o) {
            const uint32_t v = key[o];
            rank += (v < mine || (v == mine && o < k)) ? 1 : 0;
        }
        sorted[rank] = labels[k];
    }
    __syncthreads();
    if (t == 0) {
        int correct = negs, mx = negs;
        for (int i = 0; i < n_labels; ++i) {
            correct += sorted[i] ? 1 : -1;
            mx = max(mx, correct);
        }
        num[blockIdx.x] = mx;
    } else if (t == 64) {  // a second wave: the loss does not wait for the prefix walk
        double acc = 0.0;
        for (int k = 0; k < n_labels; ++k)
            if (labels[k]) acc = acc + (double)sqrtf(row[k]);
        loss[blockIdx.x] = acc / (double)(n_labels - negs);
    }
}

void launch_shapelet_score(const float* min2, int n_cand, int n_seq, int n_labels, const uint8_t* labels, int negs,
                           int32_t* num, double* loss, hipStream_t st) {
    hipLaunchKernelGGL(shapelet_score, dim3(n_cand), dim3(kShpThreads), 0, st, min2, n_seq, n_labels, labels, negs, num,
                       loss);
}

// ------------------------------------------------------------------------------------ selection
// One workgroup.  The best of a chunk's n_cand candidates under (num larger, then loss smaller, then
// the earlier candidate) against the running winner kept in best / best_loss, which a later
// candidate replaces only when it is strictly better: the first candidate wins a full tie.
//   best int32[4]: the winner's sequence, its start in that sequence, its num, candidates scored
// A new winner's row of min2 / loc becomes dis (square roots) and locs.  first: no winner yet.
struct ShpPick {
    int num, q;
    double loss;
};
__device__ inline bool shp_better(const ShpPick& a, const ShpPick& b) {
    if (a.num != b.num) return a.num > b.num;
    if (a.loss != b.loss) return a.loss < b.loss;
    return a.q < b.q;
}

__global__ __launch_bounds__(kShpThreads) void shapelet_select(const int32_t* __restrict__ num,
                                                               const double* __restrict__ loss, int n_cand,
                                                               const ShpBlock* __restrict__ blocks, int n_blocks,
                                                               const float* __restrict__ min2,
                                                               const int32_t* __restrict__ loc, int n_seq, int first,
                                                               int32_t* __restrict__ best, double* __restrict__ best_loss,
                                                               float* __restrict__ dis, int32_t* __restrict__ locs) {
    __shared__ ShpPick pick[kShpThreads];
    __shared__ int winner;
    const int t = threadIdx.x;
    ShpPick p{-2, 0x7fffffff, 0.0};
    for (int q = t; q < n_cand; q += kShpThreads) {
        const ShpPick c{num[q], q, loss[q]};
        if (shp_better(c, p)) p = c;
    }
    pick[t] = p;
    __syncthreads();
    for (int s = kShpThreads / 2; s > 0; s >>= 1) {
        if (t < s && shp_better(pick[t + s], pick[t])) pick[t] = pick[t + s];
        __syncthreads();
    }
    if (t == 0) {
        const ShpPick w = pick[0];
        const int scored = first ? 0 : best[3];
        const bool take = first || w.num > best[2] || (w.num == best[2] && w.loss < *best_loss);
        winner = take ? w.q : -1;
        if (take) {
            int bi = 0;  // the table entry that holds output row w.q
            for (int i = 0; i < n_blocks; ++i)
                if (blocks[i].out0 <= w.q) bi = i;
            best[0] = blocks[bi].seq;
            best[1] = blocks[bi].r0 + (w.q - blocks[bi].out0);
            best[2] = w.num;
            *best_loss = w.loss;
        }
        best[3] = scored + n_cand;
    }
    __syncthreads();
    const int w = winner;
    if (w < 0) return;
    for (int k = t; k < n_seq; k += kShpThreads) {
        dis[k] = sqrtf(min2[(size_t)w * n_seq + k]);
        locs[k] = loc[(size_t)w * n_seq + k];
    }
}

void launch_shapelet_select(const int32_t* num, const double* loss, int n_cand, const ShpBlock* blocks, int n_blocks,
                            const float* min2, const int32_t* loc, int n_seq, int first, int32_t* best,
                            double* best_loss, float* dis, int32_t* locs, hipStream_t st) {
    hipLaunchKernelGGL(shapelet_select, dim3(1), dim3(kShpThreads), 0, st, num, loss, n_cand, blocks, n_blocks, min2, loc,
                       n_seq, first, best, best_loss, dis, locs);
}

// ------------------------------------------------------------------------------------ scan
// Every occurrence of many patterns in whole streams (srcmx/DataAugmentation.py:106-150).
//
// shapelet_scan_dist, workgroup (tile of kScanTC consecutive rows of the batch, group of kScanPG
// patterns of the chunk's table): every row g of the tile is a position -- c = g - off[j] of its
// stream j -- of every pattern of the group, and
//   dist[slot][g] = sqrt(s) where the position exists (g + m <= off[j + 1]),
//   mask[slot][g / 64] bit g % 64 = the position exists and dist < sigma (float32, strict),
// under the distance rule above: e over d ascending from +0, s over k ascending from +0.  Thread
// t takes position t % kScanTC against the kScanPT patterns of its thread set t / kScanTC, which
// is uniform over a wave: the pattern values are scalar loads.  The group is sorted by length; a
// thread walks k to its set's longest window and a pattern's s stops taking terms after its own
// m (rows past a pattern's end repeat its last row, and their e is dropped), so no row outside pat
// is read.  kLds: the tile's kScanTC + (group's longest m) - 1 rows are staged once into LDS (row
// stride D | 1: lanes read distinct banks) and serve every pattern of the group; else a thread
// reads its rows from global memory.  Rows past L read as +0 (LDS) or repeat row L - 1 (global):
// only positions that do not exist see them.  A wave's 64 positions are one mask word, written
// whole by lane 0 from a ballot: every word of the mask is written.  No atomics.
template <bool kLds>
__global__ __launch_bounds__(kScanThreads) void shapelet_scan_dist(
    const float* __restrict__ pat, const ScanPat* __restrict__ pats, const float* __restrict__ seq,
    const int64_t* __restrict__ off, int n_seq, int64_t L, int D, int64_t nwords, float* __restrict__ dist,
    unsigned long long* __restrict__ mask) {
    extern __shared__ float scan_lds[];
    const int t = threadIdx.x, c = t % kScanTC;
    const int set = __builtin_amdgcn_readfirstlane(t / kScanTC);
    const int64_t g0 = (int64_t)blockIdx.x * kScanTC;
    const ScanPat* grp = pats + (size_t)blockIdx.y * kScanPG;
    const int ld = D | 1;
    if (kLds) {
        const int rows = kScanTC + grp[kScanPG - 1].m - 1;
        for (int i = t; i < rows * D; i += kScanThreads) {
            const int r = i / D, d = i - r * D;
            scan_lds[r * ld + d] = g0 + r < L ? seq[(g0 + r) * D + d] : 0.0f;
        }
        __syncthreads();
    }
    const ScanPat* mine = grp + set * kScanPT;
    const float* x[kScanPT];
    int m[kScanPT];
    float s[kScanPT];
#pragma unroll
    for (int q = 0; q < kScanPT; ++q) {
        m[q] = mine[q].m;
        x[q] = pat + mine[q].row0 * D;
        s[q] = 0.0f;
    }
    const int64_t g = g0 + c;
    const int hm = m[kScanPT - 1];
    for (int k = 0; k < hm; ++k) {
        const float* y;
        if (kLds)
            y = scan_lds + (c + k) * ld;
        else
            y = seq + min(g + k, L - 1) * D;
        const float* xr[kScanPT];
        float e[kScanPT];
#pragma unroll
        for (int q = 0; q < kScanPT; ++q) {
            xr[q] = x[q] + (size_t)min(k, m[q] - 1) * D;
            e[q] = 0.0f;
        }
#pragma unroll 4
        for (int d = 0; d < D; ++d) {
            const float yv = y[d];
#pragma unroll
            for (int q = 0; q < kScanPT; ++q) {
                const float v = xr[q][d] - yv;
                e[q] = e[q] + v * v;
            }
        }
#pragma unroll
        for (int q = 0; q < kScanPT; ++q)
            if (k < m[q]) s[q] = s[q] + e[q];
    }
    int64_t end = 0;  // of the position's stream
    if (g < L) end = off[seq_of_row(off, n_seq, g) + 1];
#pragma unroll
    for (int q = 0; q < kScanPT; ++q) {
        const int slot = mine[q].slot;
        const float dv = sqrtf(s[q]);
        const bool exists = g < L && g + m[q] <= end;
        const unsigned long long word = __ballot(exists && dv < mine[q].sigma);
        if (slot < 0) continue;  // uniform: a group's filler entry
        if (exists) dist[(size_t)slot * L + g] = dv;
        if ((t & 63) == 0 && (g >> 6) < nwords) mask[(size_t)slot * nwords + (g >> 6)] = word;
    }
}

size_t shapelet_scan_lds_bytes(int m_max, int D) { return sizeof(float) * (size_t)(kScanTC + m_max - 1) * (D | 1); }

void launch_shapelet_scan_dist(const float* pat, const ScanPat* pats, int n_groups, int m_max, bool lds,
                               const float* seq, const int64_t* off, int n_seq, int64_t L, int D, float* dist,
                               uint64_t* mask, hipStream_t st) {
    const dim3 grid((unsigned)((L + kScanTC - 1) / kScanTC), n_groups);
    const int64_t nwords = (L + 63) / 64;
    unsigned long long* mk = reinterpret_cast<unsigned long long*>(mask);
    if (lds) {
        const size_t shm = shapelet_scan_lds_bytes(m_max, D);
        static size_t granted = 64 * 1024;
        if (shm > granted) {
            OPOSE_HIP_CHECK(hipFuncSetAttribute((const void*)shapelet_scan_dist<true>,
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
            granted = shm;
        }
        hipLaunchKernelGGL(shapelet_scan_dist<true>, grid, dim3(kScanThreads), shm, st, pat, pats, seq, off, n_seq, L, D,
                           nwords, dist, mk);
    } else {
        hipLaunchKernelGGL(shapelet_scan_dist<false>, grid, dim3(kScanThreads), 0, st, pat, pats, seq, off, n_seq, L, D,
                           nwords, dist, mk);
    }
}

// the mask of one given distance row (opose_debug_shapelet_pick): bit g = position g exists for a
// window of m rows and dist[g] < sigma
__global__ __launch_bounds__(kScanThreads) void shapelet_scan_mask(const float* __restrict__ dist,
                                                                   const int64_t* __restrict__ off, int n_seq, int64_t L,
                                                                   int m, float sigma, int64_t nwords,
                                                                   unsigned long long* __restrict__ mask) {
    const int64_t g = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
    bool hit = false;
    if (g < L) hit = g + m <= off[seq_of_row(off, n_seq, g) + 1] && dist[g] < sigma;
    const unsigned long long word = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && (g >> 6) < nwords) mask[g >> 6] = word;
}

void launch_shapelet_scan_mask(const float* dist, const int64_t* off, int n_seq, int64_t L, int m, float sigma,
                               uint64_t* mask, hipStream_t st) {
    hipLaunchKernelGGL(shapelet_scan_mask, dim3((unsigned)((L + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0,
                       st, dist, off, n_seq, L, m, sigma, (L + 63) / 64, reinterpret_cast<unsigned long long*>(mask));
}

// shapelet_scan_pick, one wave per pair (slot, stream j) of the chunk, pair = slot * n_seq + j: the
// walk over the pair's hits, c ascending, with the state (pre, last entry)
//   first hit, or 2 * (c - pre) > m:       a new entry (c, dist), pre = c
//   else dist < the last entry's (strict): the last entry becomes (c, dist), pre = c
//   else:                                  nothing
// (the reference's idex - preidx > m / 2 with true division).  The pair's mask words are read 64 a
// step, one per lane, cut to the pair's positions a .. e - 1 (a word may hold two streams); a
// ballot names the words with a hit and their set bits are taken in order; dist is read at hits
// only.  Every lane carries the same state.  write 0: counts[pair] = the entries.  write 1: the
// entries go to occ_pos / occ_dist from occ_off[pair] on, those at or past cap dropped.
__global__ __launch_bounds__(64 * kScanPickPairs) void shapelet_scan_pick(
    const float* __restrict__ dist, const unsigned long long* __restrict__ mask, const int32_t* __restrict__ m_slot,
    const int64_t* __restrict__ off, int n_seq, int64_t L, int64_t nwords, int n_pairs, int32_t* __restrict__ counts,
    const int64_t* __restrict__ occ_off, int32_t* __restrict__ occ_pos, float* __restrict__ occ_dist, int64_t cap,
    int write) {
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * kScanPickPairs + (threadIdx.x >> 6);
    if (pair >= n_pairs) return;  // the whole wave
    const int slot = pair / n_seq, j = pair - slot * n_seq;
    const int m = m_slot[slot];
    const int64_t a = off[j], e = off[j + 1] - m + 1;  // the pair's positions are rows a .. e - 1
    const int64_t base = write ? occ_off[pair] : 0;
    int cnt = 0;
    int64_t pre = 0;
    float lastd = 0.0f;
    if (e > a) {
        const unsigned long long* mw = mask + (size_t)slot * nwords;
        const float* dr = dist + (size_t)slot * L;
        const int64_t w0 = a >> 6, w1 = (e - 1) >> 6;
        for (int64_t wb = w0; wb <= w1; wb += 64) {
            const int64_t w = wb + lane;
            unsigned long long bits = 0;
            if (w <= w1) {
                bits = mw[w];
                if (w == w0) bits &= ~0ull << (a & 63);
                if (w == w1 && (e & 63) != 0) bits &= ~0ull >> (64 - (e & 63));
            }
            unsigned long long nz = __ballot(bits != 0);
            while (nz) {  // uniform
                const int wi = __builtin_ctzll(nz);
                nz &= nz - 1;
                const unsigned lo = (unsigned)__shfl((int)(unsigned)bits, wi);
                const unsigned hi = (unsigned)__shfl((int)(unsigned)(bits >> 32), wi);
                unsigned long long wbits = ((unsigned long long)hi << 32) | lo;
                while (wbits) {
                    const int64_t g = ((wb + wi) << 6) + __builtin_ctzll(wbits);
                    wbits &= wbits - 1;
                    const int64_t c = g - a;
                    const float d = dr[g];
                    bool put = false;
                    if (cnt == 0 || 2 * (c - pre) > m) {
                        ++cnt;
                        put = true;
                    } else if (d < lastd) {
                        put = true;
                    }
                    if (put) {
                        pre = c;
                        lastd = d;
                        const int64_t o = base + cnt - 1;
                        if (write && lane == 0 && o < cap) {
                            occ_pos[o] = (int32_t)c;
                            occ_dist[o] = d;
                        }
                    }
                }
            }
        }
    }
    if (!write && lane == 0) counts[pair] = cnt;
}

void launch_shapelet_scan_pick(const float* dist, const uint64_t* mask, const int32_t* m_slot, const int64_t* off,
                               int n_seq, int64_t L, int n_pairs, int32_t* counts, const int64_t* occ_off,
                               int32_t* occ_pos, float* occ_dist, int64_t cap, bool write, hipStream_t st) {
    hipLaunchKernelGGL(shapelet_scan_pick, dim3((n_pairs + kScanPickPairs - 1) / kScanPickPairs),
                       dim3(64 * kScanPickPairs), 0, st, dist, reinterpret_cast<const unsigned long long*>(mask), m_slot,
                       off, n_seq, L, (L + 63) / 64, n_pairs, counts, occ_off, occ_pos, occ_dist, cap, write ? 1 : 0);
}

// One workgroup: occ_off[i] = *running + the counts before i, for the chunk's n pairs (occ_off
// points at the chunk's first pair), occ_off[n] = the new running total, which stays on the device
// for the next chunk.  first: the running total starts at 0.
__global__ __launch_bounds__(kShpThreads) void shapelet_scan_offsets(const int32_t* __restrict__ counts, int n, int first,
                                                                     int64_t* __restrict__ running,
                                                                     int64_t* __restrict__ occ_off) {
    __shared__ int64_t part[kShpThreads];
    const int t = threadIdx.x;
    const int per = (n + kShpThreads - 1) / kShpThreads;
    const int i0 = min(t * per, n), i1 = min(i0 + per, n);
    int64_t sum = 0;
    for (int i = i0; i < i1; ++i) sum += counts[i];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = first ? 0 : *running;
        for (int i = 0; i < kShpThreads; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        *running = run;
        occ_off[n] = run;
    }
    __syncthreads();
    int64_t acc = part[t];
    for (int i = i0; i < i1; ++i) {
        occ_off[i] = acc;
        acc += counts[i];
    }
}

void launch_shapelet_scan_offsets(const int32_t* counts, int n, bool first, int64_t* running, int64_t* occ_off,
                                  hipStream_t st) {
    hipLaunchKernelGGL(shapelet_scan_offsets, dim3(1), dim3(kShpThreads), 0, st, counts, n, first ? 1 : 0, running,
                       occ_off);
}

}  // namespace opose
