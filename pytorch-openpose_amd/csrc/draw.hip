// draw.hip — body and hand skeletons drawn into uint8 frame batches.
//
// Reference steps replaced (hitmaxiang/pytorch-openpose):
//  * src/util.py:44-77       draw_bodypose: a disc per keypoint, then every limb as a translucent
//                            ellipse (cv2.circle, cv2.ellipse2Poly + fillConvexPoly + addWeighted)
//  * srcmx/utilmx.py:212-227 draw_handpose_by_opencv: 20 edges (cv2.line, thickness 2), 21 discs
//  * srcmx/MotionEstimation.py:281-295  DisplayPose: a MotionMat row as one person, then its hands
// OpenCV's own edge pixels are not restated: a pixel is covered by a rule on its integer
// offset from the primitive, the same rule tests/draw_cases.py states in NumPy, bit for bit.
//  * disc:  dx*dx + dy*dy <= 16, opaque
//  * limb:  with (c, s) = cos / sin of int(angle) degrees from draw_table.h, A = a + 0.5, B = 4.5,
//           u = dx*c + dy*s, v = dy*c - dx*s:  u*u*(B*B) + v*v*(A*A) <= (A*A)*(B*B) in float64,
//           uncontracted; a covered pixel becomes rint(old*0.4 + colour*0.6), ties to even
//  * line:  squared distance to the segment <= 1 in int64, opaque
// draw_setup turns every frame's record or pose row into a table of primitives in draw order;
// draw_pixels bins them by pixel tile and applies a tile's hits, in order, to pixels in registers.
#include "../../include/opose.h"
#include "common.h"
#include "draw_table.h"
#include "kernels.h"

namespace opose {

namespace {

enum { kDrawNone = 0, kDrawDisc = 1, kDrawLimb = 2, kDrawLine = 3 };
// int32 words of a primitive (kDrawPrimInts of them)
enum { kPKind = 0, kPColour, kPCx, kPCy, kPP0, kPP1, kPX0, kPY0, kPX1, kPY1 };

constexpr double kCoordMax = 16384.0;  // |coordinate| bound: keeps the line test inside int64
constexpr int kDiscRadius = 4;

__constant__ double kDrawTab[360][2] = {OPOSE_DRAW_TABLE};
// the first 17 limbs of limbSeq (src/util.py:46-48), 0-based, and colors (:50-52) as c0 | c1 << 8 | c2 << 16
__constant__ int kLimbA[19] = OPOSE_LIMB_A, kLimbB[19] = OPOSE_LIMB_B;
#define RGB(a, b, c) ((a) | ((b) << 8) | ((c) << 16))
__constant__ int kColours[18] = {RGB(255, 0, 0),   RGB(255, 85, 0),  RGB(255, 170, 0), RGB(255, 255, 0), RGB(170, 255, 0),
                                 RGB(85, 255, 0),  RGB(0, 255, 0),   RGB(0, 255, 85),  RGB(0, 255, 170), RGB(0, 255, 255),
                                 RGB(0, 170, 255), RGB(0, 85, 255),  RGB(0, 0, 255),   RGB(85, 0, 255),  RGB(170, 0, 255),
                                 RGB(255, 0, 255), RGB(255, 0, 170), RGB(255, 0, 85)};
constexpr int kHandLineColour = RGB(255, 0, 0), kHandDiscColour = RGB(0, 0, 255);
#undef RGB
__constant__ int kHandEdge[20][2] = {{0, 1},   {1, 2},   {2, 3},   {3, 4},   {0, 5},   {5, 6},   {6, 7},
                                     {7, 8},   {0, 9},   {9, 10},  {10, 11}, {11, 12}, {0, 13},  {13, 14},
                                     {14, 15}, {15, 16}, {0, 17},  {17, 18}, {18, 19}, {19, 20}};

__device__ __forceinline__ bool coord_ok(double v) { return v >= -kCoordMax && v <= kCoordMax; }  // NaN: no

// int(math.degrees(math.atan2(y, x))) mod 360.  The multiples of 45 degrees, where the exact angle
// is an integer and an ulp of atan2 would decide the truncation, are settled by comparisons; on
// every other direction the angle is far from an integer (tan of an integer degree is irrational).
__device__ int limb_degrees(double y, double x) {
    if (y == 0.0) return signbit(x) ? 180 : 0;
    if (x == 0.0) return y > 0.0 ? 90 : 270;
    if (fabs(y) == fabs(x)) return y > 0.0 ? (x > 0.0 ? 45 : 135) : (x > 0.0 ? 315 : 225);
    const int k = (int)(atan2(y, x) * (180.0 / 3.141592653589793));  // truncates toward zero
    return min(max(k < 0 ? k + 360 : k, 0), 359);
}

struct Prim {
    int kind = kDrawNone, colour = 0, cx = 0, cy = 0, p0 = 0, p1 = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    // the box [cx - ex, cx + ex] x [cy - ey, cy + ey] cut to the frame, half open; empty: zeros
    __device__ void box(int bx0, int by0, int bx1, int by1, int H, int W) {
        x0 = max(bx0, 0);
        y0 = max(by0, 0);
        x1 = min(bx1 + 1, W);
        y1 = min(by1 + 1, H);
        if (x0 >= x1 || y0 >= y1) x0 = y0 = x1 = y1 = 0;
    }
};

__device__ Prim disc_prim(double x, double y, int colour, int H, int W) {
    Prim p;
    p.kind = kDrawDisc;
    p.colour = colour;
    p.cx = (int)x;
    p.cy = (int)y;
    p.box(p.cx - kDiscRadius, p.cy - kDiscRadius, p.cx + kDiscRadius, p.cy + kDiscRadius, H, W);
    return p;
}

// src/util.py:66-72 with the reference's names: X holds the two y coordinates, Y the two x
__device__ Prim limb_prim(double Y0, double X0, double Y1, double X1, int colour, int H, int W) {
    Prim p;
    p.kind = kDrawLimb;
    p.colour = colour;
    p.cx = (int)((Y0 + Y1) / 2.0);
    p.cy = (int)((X0 + X1) / 2.0);
    const double dX = X0 - X1, dY = Y0 - Y1;
    p.p0 = (int)(sqrt(dX * dX + dY * dY) / 2.0);
    p.p1 = limb_degrees(dX, dY);
    // half extents of the grown ellipse, from above: |dx| <= |c| A + |s| B
    const double c = fabs(kDrawTab[p.p1][0]), s = fabs(kDrawTab[p.p1][1]), A = p.p0 + 0.5, B = 4.5;
    const int ex = (int)(c * A + s * B) + 1, ey = (int)(s * A + c * B) + 1;
    p.box(p.cx - ex, p.cy - ey, p.cx + ex, p.cy + ey, H, W);
    return p;
}

__device__ Prim line_prim(double x1, double y1, double x2, double y2, int H, int W) {
    Prim p;
    p.kind = kDrawLine;
    p.colour = kHandLineColour;
    p.cx = (int)x1;
    p.cy = (int)y1;
    p.p0 = (int)x2;
    p.p1 = (int)y2;
    p.box(min(p.cx, p.p0) - 1, min(p.cy, p.p1) - 1, max(p.cx, p.p0) + 1, max(p.cy, p.p1) + 1, H, W);
    return p;
}

// Where a frame's joints come from: its Body record (row == nullptr) or its MotionMat row.
struct Joints {
    const double* cand;
    const double* sub;
    int n_cand;
    const double* row;
    // body part i of `person`: 1 present with (x, y) in range, 0 absent, -1 a subset index past the
    // candidates or a coordinate that is not finite or out of range
    __device__ int get(int person, int i, double& x, double& y) const {
        if (row) {
            const double* p = row + 3 * i;
            if ((p[0] + p[1]) + p[2] == 0.0) return 0;  // sum(pose[i, :]) == 0
            x = p[0];
            y = p[1];
        } else {
            const int idx = cand_index(sub[(size_t)person * 20 + i], n_cand);
            if (idx == -1) return 0;
            if (idx < 0) return -1;
            x = cand[(size_t)idx * 4];
            y = cand[(size_t)idx * 4 + 1];
        }
        return coord_ok(x) && coord_ok(y) ? 1 : -1;
    }
};

}  // namespace

// One workgroup per frame, a thread per primitive slot (strided).  joints 0: the frame's Body
// record of layout L, every person; 18 / 60: its MotionMat row as one person (60: and two hands).
// Slots in draw order -- records: part-major discs (18 x people), then limb-major limbs (17 x
// people); a row: 18 discs, 17 limbs, then per hand 20 edges and 21 discs.  A slot that draws
// nothing has kind 0 and an empty box.  counts[n]: the frame's slots, 0 when its status is not OK.
// Nothing is addressed by a coordinate: record counts are clamped to the layout, subset indices
// are checked against n_cand, and the table index comes from limb_degrees' [0, 359].
__global__ __launch_bounds__(kDrawThreads) void draw_setup(const uint8_t* __restrict__ records, RecordLayout L,
                                                           const double* __restrict__ motion, int joints, int N, int H,
                                                           int W, int cap, int32_t* __restrict__ prims,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ status) {
    const int n = blockIdx.x;
    if (n >= N) return;
    Joints J{nullptr, nullptr, 0, nullptr};
    int st = OPOSE_OK, people = 1;
    if (joints == 0) {
        const uint8_t* rec = records + (size_t)n * L.bytes;
        const int32_t* hdr = reinterpret_cast<const int32_t*>(rec);
        st = hdr[0];
        people = 0;
        if (st == OPOSE_OK) {
            J.n_cand = min(max(hdr[1], 0), L.cand_cap());
            people = min(max(hdr[2], 0), L.max_people);
            J.cand = reinterpret_cast<const double*>(rec + L.cand_off);
            J.sub = reinterpret_cast<const double*>(rec + L.subset_off);
        }
    } else {
        J.row = motion + (size_t)n * joints * 3;
    }
    const int body = 35 * people;
    const int count = min(body + (joints == 60 ? 82 : 0), cap);
    int32_t* out = prims + (size_t)n * cap * kDrawPrimInts;
    int bad = 0;
    for (int slot = threadIdx.x; slot < count; slot += kDrawThreads) {
        Prim p;
        if (slot < 18 * people) {
            const int i = slot / people, person = slot - i * people;
            double x, y;
            const int r = J.get(person, i, x, y);
            if (r > 0) p = disc_prim(x, y, kColours[i], H, W);
            bad |= r < 0;
        } else if (slot < body) {
            const int t = slot - 18 * people, i = t / people, person = t - i * people;
            double xa, ya, xb, yb;
            const int ra = J.get(person, kLimbA[i], xa, ya), rb = J.get(person, kLimbB[i], xb, yb);
            if (ra > 0 && rb > 0) p = limb_prim(xa, ya, xb, yb, kColours[i], H, W);
            bad |= ra < 0 || rb < 0;
        } else {
            const int t = slot - body, hand = t / 41, e = t - hand * 41;
            const double* hp = J.row + 3 * (18 + 21 * hand);
            if (e < 20) {
                const double* a = hp + 3 * kHandEdge[e][0];
                const double* b = hp + 3 * kHandEdge[e][1];
                if (a[0] + a[1] != 0.0 && b[0] + b[1] != 0.0) {
                    if (coord_ok(a[0]) && coord_ok(a[1]) && coord_ok(b[0]) && coord_ok(b[1]))
                        p = line_prim(a[0], a[1], b[0], b[1], H, W);
                    else
                        bad = 1;
                }
            } else {  // no missing-keypoint check in the reference: a missing one draws at (0, 0)
                const double* a = hp + 3 * (e - 20);
                if (coord_ok(a[0]) && coord_ok(a[1]))
                    p = disc_prim(a[0], a[1], kHandDiscColour, H, W);
                else
                    bad = 1;
            }
        }
        int32_t* q = out + (size_t)slot * kDrawPrimInts;
        q[kPKind] = p.kind;
        q[kPColour] = p.colour;
        q[kPCx] = p.cx;
        q[kPCy] = p.cy;
        q[kPP0] = p.p0;
        q[kPP1] = p.p1;
        q[kPX0] = p.x0;
        q[kPY0] = p.y0;
        q[kPX1] = p.x1;
        q[kPY1] = p.y1;
        q[10] = q[11] = 0;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        const int result = st != OPOSE_OK ? st : (bad ? (int)OPOSE_E_ARG : (int)OPOSE_OK);
        status[n] = result;
        counts[n] = result == OPOSE_OK ? count : 0;
    }
}

namespace {

__device__ __forceinline__ int blend(int old, int colour) { return (int)rint((double)old * 0.4 + (double)colour * 0.6); }

}  // namespace

// One workgroup per kDrawTileW x kDrawTileH pixel tile of a frame, a thread per pixel.  The
// frame's primitives are walked in chunks of the workgroup size: each thread tests one primitive's
// box against the tile, the hits are compacted in draw order into LDS (wave64 ballot, popcount
// prefix, wave offsets through LDS), then every thread applies the chunk's hits in order to its
// pixel in registers.  A pixel is read once and written once; in place (dst == src) an untouched
// pixel is not written.  src and dst may be the same memory: a thread touches its own pixel only.
__global__ __launch_bounds__(kDrawThreads) void draw_pixels(const uint8_t* src, int64_t sfs, int64_t srs, uint8_t* dst,
                                                            int64_t dfs, int64_t drs, int H, int W,
                                                            const int32_t* __restrict__ prims,
                                                            const int32_t* __restrict__ counts, int cap, int inplace) {
    __shared__ int s_hit[kDrawThreads][6];
    __shared__ int s_wcnt[kDrawThreads / 64];
    const int n = blockIdx.z;
    const int tx0 = blockIdx.x * kDrawTileW, ty0 = blockIdx.y * kDrawTileH;
    const int tx1 = min(tx0 + kDrawTileW, W), ty1 = min(ty0 + kDrawTileH, H);
    const int px = tx0 + (int)threadIdx.x % kDrawTileW, py = ty0 + (int)threadIdx.x / kDrawTileW;
    const bool valid = px < W && py < H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int count = min(max(counts[n], 0), cap);
    const int32_t* table = prims + (size_t)n * cap * kDrawPrimInts;
    int c0 = 0, c1 = 0, c2 = 0;
    if (valid) {
        const uint8_t* p = src + (size_t)n * sfs + (size_t)py * srs + (size_t)px * 3;
        c0 = p[0];
        c1 = p[1];
        c2 = p[2];
    }
    bool changed = false;
    for (int base = 0; base < count; base += kDrawThreads) {
        const int i = base + threadIdx.x;
        bool hit = false;
        int q[6];
        if (i < count) {
            const int32_t* p = table + (size_t)i * kDrawPrimInts;
            hit = p[kPKind] != kDrawNone && p[kPX0] < tx1 && p[kPX1] > tx0 && p[kPY0] < ty1 && p[kPY1] > ty0;
            for (int k = 0; k < 6; ++k) q[k] = p[k];
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < kDrawThreads / 64; ++w) {
            const int c = s_wcnt[w];
            off += w < wave ? c : 0;
            total += c;
        }
        if (hit) {
            const int at = off + __popcll(m & ((1ull << lane) - 1ull));
            for (int k = 0; k < 6; ++k) s_hit[at][k] = q[k];
        }
        __syncthreads();
        if (valid) {
            for (int hI = 0; hI < total; ++hI) {
                const int kind = s_hit[hI][kPKind], colour = s_hit[hI][kPColour];
                const int dx = px - s_hit[hI][kPCx], dy = py - s_hit[hI][kPCy];
                const int p0 = s_hit[hI][kPP0], p1 = s_hit[hI][kPP1];
                if (kind == kDrawLimb) {
                    const double c = kDrawTab[p1][0], s = kDrawTab[p1][1];
                    const double fx = dx, fy = dy;
                    const double u = fx * c + fy * s;
                    const double v = fy * c - fx * s;
                    const double A = p0 + 0.5, B = 4.5;
                    if (u * u * (B * B) + v * v * (A * A) <= (A * A) * (B * B)) {
                        c0 = blend(c0, colour & 255);
                        c1 = blend(c1, (colour >> 8) & 255);
                        c2 = blend(c2, (colour >> 16) & 255);
                        changed = true;
                    }
                    continue;
                }
                const long long bx = dx, by = dy;
                bool covered;
                if (kind == kDrawDisc) {
                    covered = bx * bx + by * by <= kDiscRadius * kDiscRadius;
                } else {  // the segment from P = (cx, cy) to Q = (p0, p1)
                    const long long ax = (long long)p0 - s_hit[hI][kPCx], ay = (long long)p1 - s_hit[hI][kPCy];
                    const long long w = bx * ax + by * ay, L2 = ax * ax + ay * ay, d2 = bx * bx + by * by;
                    if (w <= 0) {
                        covered = d2 <= 1;
                    } else if (w >= L2) {
                        const long long ex = px - p0, ey = py - p1;
                        covered = ex * ex + ey * ey <= 1;
                    } else {
                        covered = d2 * L2 - w * w <= L2;
                    }
                }
                if (covered) {
                    c0 = colour & 255;
                    c1 = (colour >> 8) & 255;
                    c2 = (colour >> 16) & 255;
                    changed = true;
                }
            }
        }
        // (the next chunk's first barrier orders its s_hit writes after these reads)
    }
    if (valid && (changed || !inplace)) {
        uint8_t* p = dst + (size_t)n * dfs + (size_t)py * drs + (size_t)px * 3;
        p[0] = (uint8_t)c0;
        p[1] = (uint8_t)c1;
        p[2] = (uint8_t)c2;
    }
}

void launch_draw_setup(const uint8_t* records, const RecordLayout& L, const double* motion, int joints, int N, int H,
                       int W, int cap, int32_t* prims, int32_t* counts, int32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(draw_setup, dim3(N), dim3(kDrawThreads), 0, st, records, L, motion, joints, N, H, W, cap, prims,
                       counts, status);
}

void launch_draw_pixels(const uint8_t* src, int64_t sfs, int64_t srs, uint8_t* dst, int64_t dfs, int64_t drs, int N,
                        int H, int W, const int32_t* prims, const int32_t* counts, int cap, hipStream_t st) {
    const dim3 grid((W + kDrawTileW - 1) / kDrawTileW, (H + kDrawTileH - 1) / kDrawTileH, N);
    hipLaunchKernelGGL(draw_pixels, grid, dim3(kDrawThreads), 0, st, src, sfs, srs, dst, dfs, drs, H, W, prims, counts,
                       cap, (int)(src == dst));
}

}  // namespace opose
