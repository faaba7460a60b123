// posemat.hip — the fast mode's person choice: per-frame Body records -> PoseMat rows.
//
// Reference step replaced (hitmaxiang/pytorch-openpose):
//  * srcmx/Batch_motion_Estimation.py:88-107  the person with the largest left-shoulder x
//    (np.argmax: the first among equal maxima; an absent shoulder's -1 reads candidate[-1], the
//    last row, as Python's negative index does) and that person's 18 keypoints   => pose_select
// Values are copied, never computed: the rows are the record's float64 bits.
#include <limits>

#include "../../include/opose.h"
#include "common.h"
#include "kernels.h"

namespace opose {

// One wave64 per frame.  records: N records of layout L; pose [N][18][3]; status [N].
//  * header status != 0: zero row, status carried, nothing else of the record read;
//  * no person: zero row, status 0;
//  * a subset index outside the record's candidates: zero row, OPOSE_E_ARG.
// n_cand / n_people are clamped to the layout's capacity and every candidate index is checked
// against n_cand, so no address leaves the frame's record.
__global__ __launch_bounds__(64) void pose_select(const uint8_t* __restrict__ records, int N, RecordLayout L,
                                                  double* __restrict__ pose, int32_t* __restrict__ status) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (n >= N) return;
    const uint8_t* rec = records + (size_t)n * L.bytes;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(rec);
    double* out = pose + (size_t)n * 54;
    const int st = hdr[0];
    int result = st;
    int idx = -1;  // lanes < 18: the candidate row of key `lane`, -1: zeros
    const double* cand = reinterpret_cast<const double*>(rec + L.cand_off);
    if (st == 0) {
        const int n_cand = min(max(hdr[1], 0), L.cand_cap());
        const int n_people = min(max(hdr[2], 0), L.max_people);
        const double* sub = reinterpret_cast<const double*>(rec + L.subset_off);
        // lanes stride over people; ascending p per lane, so a strict > keeps the lane's first maximum
        double best = -std::numeric_limits<double>::infinity();
        int win = 0x7fffffff;
        int bad = 0;
        for (int p = lane; p < n_people; p += 64) {
            int i = cand_index(sub[(size_t)p * 20 + 5], n_cand);
            if (i == -1) i = n_cand - 1;  // candidate[-1]; no candidate at all: out of range
            if (i < 0) {
                bad = 1;
                continue;
            }
            const double x = cand[(size_t)i * 4];
            if (win == 0x7fffffff || x > best) {
                best = x;
                win = p;
            }
        }
        // wave argmax on (value, index): greater, or equal and lower index
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int ow = __shfl_xor(win, off, 64);
            if (ow != 0x7fffffff && (win == 0x7fffffff || ob > best || (ob == best && ow < win))) {
                best = ob;
                win = ow;
            }
        }
        bad = __syncthreads_or(bad);
        if (!bad && n_people > 0 && lane < 18) {
            idx = cand_index(sub[(size_t)win * 20 + lane], n_cand);
            if (idx == kBadIndex) bad = 1;
        }
        bad = __syncthreads_or(bad);
        if (bad) {
            result = OPOSE_E_ARG;
            idx = -1;
        }
    }
    if (lane < 18) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        if (idx >= 0) {
            const double* c = cand + (size_t)idx * 4;
            v0 = c[0];
            v1 = c[1];
            v2 = c[2];
        }
        out[3 * lane] = v0;
        out[3 * lane + 1] = v1;
        out[3 * lane + 2] = v2;
    }
    if (lane == 0) status[n] = result;
}

void launch_pose_select(const uint8_t* records, int N, const RecordLayout& L, double* pose, int32_t* status,
                        hipStream_t st) {
    hipLaunchKernelGGL(pose_select, dim3(N), dim3(64), 0, st, records, N, L, pose, status);
}

}  // namespace opose
