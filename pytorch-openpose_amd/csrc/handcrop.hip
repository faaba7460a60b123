// handcrop.hip — the fast mode's hand extraction around the hand network: body pose -> hand boxes,
// frames + boxes -> boxsize x boxsize crops (network input), crop peaks -> frame coordinates.
//
// Reference steps replaced (hitmaxiang/pytorch-openpose):
//  * srcmx/Batch_model.py:74-84 + srcmx/utilmx.py:267-327  the one-person subset built from a
//                       MotionMat row and utilmx.handDetect on it            => hand_boxes
//  * srcmx/Batch_model.py:86-102  cv2.flip (left) + cv2.resize(crop, (boxsize, boxsize),
//                       INTER_CUBIC) on uint8, gray 128 for an absent hand, transforms.ToTensor;
//    srcmx/Batch_model.py:328-329  - 0.5 at scale 1                          => hand_crops
//  * srcmx/Batch_motion_Estimation.py:44-58  crop peaks -> frame pixels, rows of HandMat
//                                                                            => hand_backmap
// Compiled with -ffp-contract=off (see cubic.h): int() of a float64 expression at an integer
// boundary is where a fused multiply-add would show.
#include "../../include/opose.h"
#include "common.h"
#include "cubic.h"
#include "kernels.h"

namespace opose {

// joint i of a MotionMat row is missing iff sum(pose[i, :]) == 0 (Python's sum: ((0 + x) + y) + s)
__device__ __forceinline__ bool joint_missing(const double* pose, int i) {
    return ((0.0 + pose[3 * i]) + pose[3 * i + 1]) + pose[3 * i + 2] == 0.0;
}

// One thread per (frame, side); side 0 = left (shoulder 5, elbow 6, wrist 7), 1 = right (2, 3, 4).
// boxes [N][2][4] = {x, y, w, present}; an absent side is all zeros.  utilmx.handDetect line by
// line in float64 (d * d for its d ** 2), int() truncation last.
__global__ __launch_bounds__(64) void hand_boxes(const double* __restrict__ motion, int N, int H, int W,
                                                 int32_t* __restrict__ boxes) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * N) return;
    const int n = t >> 1, side = t & 1;
    const double* pose = motion + (size_t)n * 54;
    const int js = side ? 2 : 5, je = js + 1, jw = js + 2;
    int32_t* b = boxes + (size_t)t * 4;
    if (joint_missing(pose, js) || joint_missing(pose, je) || joint_missing(pose, jw)) {
        b[0] = b[1] = b[2] = b[3] = 0;
        return;
    }
    const double x1 = pose[3 * js], y1 = pose[3 * js + 1];
    const double x2 = pose[3 * je], y2 = pose[3 * je + 1];
    const double x3 = pose[3 * jw], y3 = pose[3 * jw + 1];
    double x = x3 + 0.33 * (x3 - x2);
    double y = y3 + 0.33 * (y3 - y2);
    const double dwe = sqrt((x3 - x2) * (x3 - x2) + (y3 - y2) * (y3 - y2));
    const double des = 0.9 * sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1));
    double width = 1.5 * (des > dwe ? des : dwe);  // Python max(a, b): b if b > a else a
    x = x - width / 2;
    y = y - width / 2;
    if (x < 0) x = 0;
    if (y < 0) y = 0;
    double w1 = width, w2 = width;
    if (x + width > (double)W) w1 = (double)W - x;
    if (y + width > (double)H) w2 = (double)H - y;
    width = w2 < w1 ? w2 : w1;  // Python min(w1, w2)
    b[0] = (int)x;
    b[1] = (int)y;
    b[2] = (int)width;
    b[3] = 1;
}

// One thread per output pixel of one slot (blockIdx.z over the 2N slots, left then right per
// frame).  A present slot whose box lies in the frame with w >= 1: cv2.resize of the (left:
// mirrored) w x w crop to bs x bs, the fixed-point arithmetic of preprocess_u8 with the taps
// clamped to the crop.  Anything else writes 128 and reads no pixel; a present slot with no
// usable box also gets status OPOSE_E_SHAPE (the reference dies in cv2.resize on an empty image).
// x: network input [2N][3][bs][bs] = v / 255.f - 0.5f (ToTensor, then Batch_hand's - 0.5), or
// nullptr; crops: uint8 [2N][bs][bs][3], or nullptr.
__global__ __launch_bounds__(256) void hand_crops(const uint8_t* __restrict__ src, int64_t frame_stride,
                                                  int64_t row_stride, int H, int W,
                                                  const int32_t* __restrict__ boxes, int bs,
                                                  float* __restrict__ x, uint8_t* __restrict__ crops,
                                                  int32_t* __restrict__ status) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    const int slot = blockIdx.z;
    if (col >= bs) return;
    const int32_t* b = boxes + (size_t)slot * 4;
    const int bx = b[0], by = b[1], w = b[2];
    const bool present = b[3] != 0;
    const bool usable = present && w >= 1 && bx >= 0 && by >= 0 && (int64_t)bx + w <= W && (int64_t)by + w <= H;
    if (col == 0 && row == 0) status[slot] = present && !usable ? (int32_t)OPOSE_E_SHAPE : 0;
    int v[3] = {128, 128, 128};
    if (usable) {
        const double scale = 1.0 / ((double)bs / (double)w);
        const CubicTap ty = cubic_tap(row, scale, w);
        const CubicTap tx = cubic_tap(col, scale, w);
        int ia[4], ib[4], sc[4];
        const bool left = (slot & 1) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ia[j] = coef_short(tx.c[j]);
            ib[j] = coef_short(ty.c[j]);
            sc[j] = bx + (left ? w - 1 - tx.i[j] : tx.i[j]);  // cv2.flip(crop, 1) before the resize
        }
        const uint8_t* f = src + (size_t)(slot >> 1) * frame_stride;
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint8_t* line = f + (size_t)(by + ty.i[r]) * row_stride;
            int hsum[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t* px = line + 3 * sc[j];
                hsum[0] += px[0] * ia[j];
                hsum[1] += px[1] * ia[j];
                hsum[2] += px[2] * ia[j];
            }
            acc[0] += hsum[0] * ib[r];
            acc[1] += hsum[1] * ib[r];
            acc[2] += hsum[2] * ib[r];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int q = (acc[c] + (1 << 21)) >> 22;
            v[c] = q < 0 ? 0 : (q > 255 ? 255 : q);
        }
    }
    const size_t plane = (size_t)bs * bs;
    const size_t pix = (size_t)row * bs + col;
    if (x) {
        float* o = x + (size_t)slot * 3 * plane + pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * plane] = (float)v[c] / 255.f - 0.5f;
    }
    if (crops) {
        uint8_t* o = crops + ((size_t)slot * plane + pix) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
    }
}

// One thread per (slot, part): srcmx/Batch_motion_Estimation.py:44-58 in its operation order.
// peaks [2N][21][3], found [2N][21] (slot = 2 * frame + side); handmat [N][42][3], left hand rows
// 0-20, right hand rows 21-41.
__global__ __launch_bounds__(64) void hand_backmap(const double* __restrict__ peaks, const int32_t* __restrict__ found,
                                                   const int32_t* __restrict__ boxes, int N, int bs,
                                                   double* __restrict__ handmat) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * N * 21) return;
    const int slot = t / 21, part = t - slot * 21;
    const int n = slot >> 1, side = slot & 1;
    double* o = handmat + ((size_t)n * 42 + side * 21 + part) * 3;
    if (!found[t]) {
        o[0] = o[1] = o[2] = 0.0;
        return;
    }
    const int32_t* b = boxes + (size_t)slot * 4;
    const double bx = (double)b[0], by = (double)b[1], w = (double)b[2];
    double x = (peaks[3 * (size_t)t] * w) / (double)bs;
    double y = (peaks[3 * (size_t)t + 1] * w) / (double)bs;
    if (side) x = x == 0 ? x : x + bx;
    else x = x == 0 ? x : ((w - x) - 1) + bx;
    y = y == 0 ? y : y + by;
    o[0] = x;
    o[1] = y;
    o[2] = peaks[3 * (size_t)t + 2];
}

void launch_hand_boxes(const double* motion, int N, int H, int W, int32_t* boxes, hipStream_t st) {
    hipLaunchKernelGGL(hand_boxes, dim3((2 * N + 63) / 64), dim3(64), 0, st, motion, N, H, W, boxes);
}

void launch_hand_crops(const uint8_t* src, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                       const int32_t* boxes, int bs, float* x, uint8_t* crops, int32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(hand_crops, dim3((bs + 255) / 256, bs, 2 * N), dim3(256), 0, st, src, frame_stride, row_stride,
                       H, W, boxes, bs, x, crops, status);
}

void launch_hand_backmap(const double* peaks, const int32_t* found, const int32_t* boxes, int N, int bs,
                         double* handmat, hipStream_t st) {
    hipLaunchKernelGGL(hand_backmap, dim3((2 * N * 21 + 63) / 64), dim3(64), 0, st, peaks, found, boxes, N, bs,
                       handmat);
}

}  // namespace opose
