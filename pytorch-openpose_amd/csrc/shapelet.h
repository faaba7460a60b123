// shapelet.h — limits and tile constants of the shapelet search (shapelet.hip, engine_shapelet.cpp).
// tests/shapelet_cases.py and the shapelet GPU tests parse the constants below, so their edge lengths
// follow the code.
#pragma once
#include <cstdint>

namespace opose {

// limits: beyond them the entry points answer OPOSE_E_SHAPE
constexpr int kShpMaxM = 128;      // window length
constexpr int kShpMaxD = 1024;     // feature columns
constexpr int kShpMaxSeq = 4096;   // sequences of a ragged batch (grid y; the score kernel's LDS keys)
constexpr int64_t kShpMaxRows = 2147483647;  // L, rows of a ragged batch (int32 row indices)
// shapelet_mindist: a workgroup takes kShpTR candidate starts of one sequence against one target and
// walks the target's positions kShpTC at a time, streaming D through LDS kShpDC columns at a time
constexpr int kShpTR = 32;
constexpr int kShpTC = 32;
constexpr int kShpDC = 16;
constexpr int kShpThreads = 256;
constexpr int kShpSub = kShpThreads / kShpTR;  // threads sharing one candidate start's positions
// window lengths one call may share its distances among
constexpr int kShpMaxLens = 16;
// opose_shapelet_find: candidates per chunk when the caller passes max_cands = 0
constexpr int kShpDefaultCands = 2048;
// motion_features: rows per fill block (the carry of the forward fill crosses these)
constexpr int kFeatRows = 64;
constexpr int kFeatThreads = 256;
// opose_shapelet_scan: patterns and (pattern, stream) pairs of one call
constexpr int kScanMaxPat = 4096;
constexpr int kScanMaxPairs = 4194304;
// shapelet_scan_dist: a workgroup takes kScanTC consecutive rows of the batch as positions against
// a group of kScanPG patterns (sorted by length); its kScanThreads / kScanTC thread sets share the
// group's patterns, kScanPT each.  The stream tile goes to LDS when it fits kScanLdsBytes (two
// workgroups per CU), else the rows are read from global memory.
constexpr int kScanTC = 128;
constexpr int kScanPG = 16;
constexpr int kScanThreads = 256;
constexpr int kScanPT = kScanPG / (kScanThreads / kScanTC);  // patterns a thread accumulates
constexpr int kScanLdsBytes = 81920;
// shapelet_scan_pick: one wave per pair, kScanPickPairs pairs per workgroup, 64 mask words a step
constexpr int kScanPickPairs = 4;
// opose_shapelet_scan: patterns per chunk when the caller passes max_pats = 0 (the distance
// workspace is that many rows of L floats: 256 MB at L = 10^6)
constexpr int kScanDefaultPats = 64;
// opose_shapelet_net_train: models trained side by side in one call (grid z of the forward kernel)
constexpr int kNetMaxModels = 16;
// shapelet_net_forward: a workgroup of kNetTC threads takes kNetTC consecutive positions of one clip
// against one model's query, e over d in steps of kNetDU columns and a remainder.  The query goes
// to LDS when its m * D floats fit kNetQLdsBytes, the clip's tile of kNetTC + m - 1 rows when it
// fits kNetXLdsBytes (both together stay below the 64 KB a launch gets without an attribute call);
// what does not fit is read from global memory.
constexpr int kNetTC = 64;
constexpr int kNetDU = 4;
constexpr int kNetQLdsBytes = 16384;
constexpr int kNetXLdsBytes = 40960;
// shapelet_net_head (one workgroup per model) and shapelet_net_step (a thread per query element)
constexpr int kNetThreads = 256;

// kShpTR consecutive candidate starts r0 .. r0 + nvalid - 1 of sequence `seq`; out0: the row of the
// launch's output that start r0 writes
struct ShpBlock {
    int32_t seq, r0, nvalid, out0;
};

// shapelet_mindist: the ascending window lengths, passed by value as a kernel argument
struct ShpLens {
    int32_t n;
    int32_t m[kShpMaxLens];
};
// per (table entry, length): the entry's starts that are valid at that length -- its first nvalid --
// and the output row the first of them writes
struct ShpLenRows {
    int32_t out0, nvalid;
};

// shapelet_scan_dist: one pattern of a chunk's table (sorted by length, groups of kScanPG; a
// group's missing entries repeat its last pattern with slot -1).  row0: the pattern's first row in
// pat; slot: its row of the chunk's dist / mask workspace (the caller's order), -1: writes nothing
struct ScanPat {
    int64_t row0;
    int32_t m, slot;
    float sigma;
    int32_t pad;
};

// shapelet_net_*: one model of a training call.  row0: the first row of its query in the
// concatenated queries (and of its moments); m: the rows of its query
struct NetModel {
    int64_t row0;
    int32_t m, pad;
};

}  // namespace opose
