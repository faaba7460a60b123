// engine.h — what the engine*.cpp files of libopose's host runtime share: the handle (opose_ctx),
// the types that cross a file boundary, and the prototypes of the functions that do.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <queue>
#include <vector>

#include "../../include/opose.h"
#include "common.h"
#include "kernels.h"
#include "topology.h"

namespace opose {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------- device memory helpers
// Bumped whenever device memory that a captured hipGraph may reference is (re)allocated:
// graphs captured under an older epoch are dropped instead of replayed.
extern std::atomic<uint64_t> g_alloc_epoch;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    uint64_t pad_key = 0;  // X6P geometry whose padding units are known zero (0: none)
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    template <class T>
    T* ensure(size_t n, hipStream_t st) {
        size_t b = n * sizeof(T);
        if (b > bytes) {
            if (p) {
                (void)st;
                OPOSE_HIP_CHECK(hipDeviceSynchronize());  // the handle may have work on two streams
                OPOSE_HIP_CHECK(hipFree(p));
                p = nullptr;
            }
            size_t nb = std::max(b, bytes + bytes / 4);
            OPOSE_HIP_CHECK(hipMalloc(&p, nb));
            bytes = nb;
            pad_key = 0;
            g_alloc_epoch.fetch_add(1);
        }
        return static_cast<T*>(p);
    }
};

// Pinned host staging (small results copied back each call: a device-to-host copy into pageable
// memory goes through the runtime's staging buffer, ~35 us per copy on the box)
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    template <class T>
    T* ensure(size_t n) {
        const size_t b = n * sizeof(T);
        if (b > bytes) {
            if (p) {
                OPOSE_HIP_CHECK(hipDeviceSynchronize());  // a copy into it may still be in flight
                OPOSE_HIP_CHECK(hipHostFree(p));
                p = nullptr;
            }
            OPOSE_HIP_CHECK(hipHostMalloc(&p, b, hipHostMallocDefault));
            bytes = b;
        }
        return static_cast<T*>(p);
    }
};

// A GEMM-ready conv: one or two (combined) reference layers.
struct DevConv {
    std::string name;
    int cin = 0, cout = 0, ks = 0, pad = 0, K = 0, Kpad = 0, Mpad = 0;
    bool tap_major = false;  // K = (channel block of 32, tap, channel); see conv.hip
    float* wt = nullptr;
    float* bias = nullptr;
    int* ktab = nullptr;
    // split-bf16 (X6) form: [nK6][3][4][Mpad] units of 8 bf16, input channels in the physical
    // (group-aligned) order of the X6 activation buffers; see conv_x6.hip
    uint8_t* wx6 = nullptr;
    int nK6 = 0, cin_g = 0;
    bool small6 = false;
    // 3x3 / 7x7 layers: the same weights in pair order for conv_win_x6 (conv_win.hip)
    uint8_t* wx6p = nullptr;
    int nK6p = 0;
    // 3x3 layers: the Winograd F(2,3) weights U_v (x6_pack_weights_wino) for conv_wino_x6
    uint8_t* wwino = nullptr;
    int nKw = 0;
    // k-slab policy inputs (engine slab_count): the network, the layer's resolution level
    // (0: H .. 3: H/8) and whether it is one branch of a CPM pair (two GEMMs per launch)
    int net = 0, lvl = 0;
    bool pair = false;
    ~DevConv() {
        if (wx6) (void)hipFree(wx6);
        if (wx6p) (void)hipFree(wx6p);
        if (wwino) (void)hipFree(wwino);
        if (wt) (void)hipFree(wt);
        if (bias) (void)hipFree(bias);
        if (ktab) (void)hipFree(ktab);
    }
};

// The DevConv of every step of a forward (topology.h NetDesc), resolved once by
// opose_load_weights: pointers into opose_ctx::convs[net].
struct NetTable {
    std::vector<DevConv*> trunk;
    struct Stage {
        DevConv* open = nullptr;       // the opening layer, every branch in one conv (null: none)
        std::vector<DevConv*> mid[2];  // per branch
        DevConv* close[2][2] = {};     // per branch the closing 1x1 pair (a missing branch: null)
    } stages[kStages];
};

struct ProfEntry {
    std::string cls;
    std::string detail;  // optional second aggregation key (per layer / tile choice)
    double flops = 0;
    double bytes = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;  // null: not recorded (profiling off / filtered)
};

struct ProfAgg {
    long count = 0;
    double ms = 0, flops = 0, bytes = 0;
};

// geometry of one pyramid scale (engine_post.cpp geom)
struct ScaleGeom {
    double mult;      // scale * boxsize / H
    int Hs, Ws;       // cv2.resize output (cvRound(H * mult))
    int Hp, Wp;       // padded to stride
    int hl, wl;       // network output
    double up_sy, up_sx;  // final resize (Hs,Ws) -> (H,W) source steps
};

// geometry of a fast-mode frame (engine_api.cpp batch_geom)
struct BatchGeom {
    double scale;  // boxsize * scale_search / H
    int nh, nw;    // int(H * scale), int(W * scale)
    int Hp, Wp;    // padded to stride
};

struct GraphEntry {
    hipGraphExec_t exec = nullptr;
    uint64_t epoch = 0;
    bool eager = false;  // its capture was not one chain of nodes: run eagerly from then on
};

// launch plan of one conv launch signature (engine_plan.cpp plan_launch; opose_ctx::plans)
struct ConvPlan {
    int mt = 0, pt = 0, grid = 0;
    int* sched = nullptr;
};

struct Act {  // a channel slice of an NCHW activation buffer
    float* p;
    int cstride, coff;
};

struct TileChoice {
    int mt, pt, grid;  // tile shape, workgroups (grid == tiles: data parallel; else stream-K)
};

struct XAct {  // a group slice of an X6 buffer (or, f32: a channel slice of an fp32 NCHW buffer)
    void* p = nullptr;
    int c = 0, off = 0;  // f32: channels per frame / first channel
    uint32_t ps = 0;     // X6 piece stride (bytes)
    X6Layout l{};        // X6 unit addressing (common.h)
    bool f32 = false;
    bool padded = false;
    int ylo = 0, yhi = 0;  // X6P row-band view: rows conv taps may read (yhi == 0: the frame's)
};

// One GEMM of a conv launch (an X6Group): a scale's frames through one branch's weights.
// Hl: the frame height the k-slab policy sees (a row band's view passes its whole frame's rows;
// 0: H); slabs: set by the planner (a frame view inherits its segment's).
struct ConvSeg {
    DevConv* c;
    int N, H, W;
    XAct in, out, dup;  // dup: optional duplicate X6 destination
    bool relu;
    int Hl = 0;
    int slabs = 0;
};

// the kernel family of a segment (engine_plan.cpp seg_kernel)
enum { kKernelX6 = 0, kKernelWin = 1, kKernelWinFrames = 2, kKernelWino = 3 };

// A CPM stage's closing 1x1 pair (conv5_4 -> conv5_5, conv6_1 -> conv6_2, Mconv6 -> Mconv7) on one
// segment: out = c2(relu(c1(in))) (+ ReLU when relu2); `mid` holds c1's output when the pair runs
// as two launches.
struct ChainSeg {
    DevConv *c1, *c2;
    int N, H, W;
    XAct in, mid, out;
    bool relu2;
    int Hl = 0;  // ConvSeg::Hl of the two-launch form
};

// One scale of a network forward.  The scales of a pyramid (Hand()'s four, C5's) run in lockstep:
// layer by layer, one conv launch covers every scale (X6 groups with their own geometry), so a
// single crop's small layers share one grid instead of each filling a fraction of the chip.
struct NetSeg {
    const float* x;  // [N][3][Hp][Wp] fp32 network input
    int N, Hp, Wp;
    int slot;  // workspace set (opose_ctx::ws)
    int Hl = 0;  // the whole frame's input rows when x is a row band's rows (ConvSeg::Hl); 0: Hp
};

// Output rows [r0, r1) of one frame's CPM stages (opose_body_band_maps).  The stage buffers keep
// the whole frame's geometry; every stage layer runs on a view of the band's rows (X6P origin
// moved down r0 rows), whose padding rows are the neighbouring bands' rows: band_halo refreshes
// them before each 3x3 / 7x7 layer that reads them.  The trunk before the stages runs on the
// band's rows plus kBandTrunkMargin rows past each cut (recomputed, not exchanged).  Every conv of
// the band sums each pixel in the order of the whole frame's (ConvSeg::Hl = the frame's rows), so
// the band's maps are the whole frame's rows bit for bit.
struct Band {
    int r0, r1;
    float* maps;  // [57][r1 - r0][wl] fp32 device
    opose_halo_fn fn;  // nullptr: the library's RCCL send / recv (opose_rccl_init)
    void* user;
    uint8_t* xbuf;  // [send_up | send_dn | recv_up | recv_dn], cap bytes each
    size_t cap;
};

// RCCL entry points, resolved on first use: the library shares the RCCL a host framework already
// loaded (torch's), and callers that never split a frame never load it.
struct Rccl {
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclCommAbort) comm_abort = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    decltype(&ncclCommGetAsyncError) async_error = nullptr;
};

// A field of the handle redirected for a scope: holds `v` (or whatever the scope stores in it)
// until the guard goes, by return or by exception, then has the value it had before again.
template <class T>
struct Redirect {
    T& field;
    const T old;
    explicit Redirect(T& f) : field(f), old(f) {}
    Redirect(T& f, T v) : field(f), old(f) { f = v; }
    ~Redirect() { field = old; }
    Redirect(const Redirect&) = delete;
};

// ---------------------------------------------------------------- functions that cross files
// engine.cpp
bool env_flag(const char* name, bool dflt);  // a boolean switch: "0" / "1" first character, else dflt
hipError_t pooled_stream(hipStream_t* s, int priority);
// engine_weights.cpp
// lvl, pair: DevConv::lvl / pair (a layer outside the networks: 3, false)
void upload_conv(opose_ctx* h, int net, const std::string& key, const std::vector<const Spec*>& parts,
                 const std::vector<const float*>& w, const std::vector<const float*>& b, int lvl, bool pair,
                 const std::vector<int>& cmap = {});
// engine_plan.cpp
TileChoice choose_tile(int Mpad, const std::vector<int>& gpix, int nK, bool x6 = false, bool dp_only = false,
                       double* cost_out = nullptr);
int slab_count(opose_ctx* h, const DevConv* c, bool win, int N, int H, int W, bool pool);
int seg_kernel(opose_ctx* h, const ConvSeg& sg, bool pool);
ConvPlan plan_launch(opose_ctx* h, const std::vector<ConvSeg>& segs, bool win, bool pool, int nK, int Mpad);
// engine_net.cpp
XAct x6act(uint8_t* p, int cg, int goff, int N, int H, int W);
size_t x6p_plane(int N, int H, int W);
XAct x6pact(uint8_t* p, int cg, int goff, int N, int H, int W);
void run_conv_x6_segs(opose_ctx* h, const std::vector<ConvSeg>& segs, bool pool = false);
void launch_chain_segs(opose_ctx* h, const std::vector<ChainSeg>& segs);
std::vector<float*> net_forward_x6(opose_ctx* h, int net, const std::vector<NetSeg>& segs, const Band* band = nullptr);
float* net_forward(opose_ctx* h, int net, const float* x, int N, int Hp, int Wp);
// engine_post.cpp
ScaleGeom geom(double s, const opose_params& p, int H, int W);
ScaleGeom geom_from_pads(int hl, int wl, int pad_down, int pad_right, int H, int W);
// slot0: the mid set of the frames' first scale (scale s in set slot0 + s; one group of frames: 0)
void body_post_common(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, const opose_params& p,
                      uint8_t* rec_dev, int slot0 = 0);
void body_post_reserve(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, int slot0);
PafScales body_paf_scales(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, int slot0 = 0);
PafScales batch_paf_scales(const float* mid, int nh, int nw, int H, int W);
void batch_resize_chain(opose_ctx* h, int N, int H, int W, const float* maps, int cstride, int hl, int wl, int nh,
                        int nw, float* mid, float* heat);
void batch_post_common(opose_ctx* h, int N, int H, int W, const float* maps, int cstride, int hl, int wl, int nh,
                       int nw, const opose_params& p, uint8_t* rec_dev);
void hand_post_common(opose_ctx* h, int N, int H, int W, const std::vector<ScaleGeom>& gs, const opose_params& p,
                      double* peaks_out, int32_t* found_out, int flags, int mid_crop = 0, int out_crop = 0);
void batch_hand_post_common(opose_ctx* h, int N, int H, int W, const float* maps, int cstride, const opose_params& p,
                            double* peaks, int32_t* found, int flags);
void upsample_to_mid(opose_ctx* h, int s, const float* maps, int cstride, int N, const ScaleGeom& g, int C);
void body_to_mid(opose_ctx* h, int s, const float* maps, int cstride, int N, const ScaleGeom& g);
void hand_finish(opose_ctx* h, int N, double* peaks_out, int32_t* found_out, int flags);
uint8_t* records_dest(opose_ctx* h, int N, void* records, int flags);
int finish_records(opose_ctx* h, int N, void* records, uint8_t* rec_dev, int flags);
int finish_records_groups(opose_ctx* h, int n, const int* N, void* const* records, uint8_t* const* rec_dev, int flags);
// engine_api.cpp
void flush_post(opose_ctx* h);
void enter_main(opose_ctx* h);
const uint8_t* stage_frames(opose_ctx* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                            int64_t frame_stride, int flags);
void preprocess_scale(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                      const ScaleGeom& g, const opose_params& p, float* x, hipStream_t stream);
PrepSeg prep_seg(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                 const ScaleGeom& g, float* x);
void preprocess_segs(opose_ctx* h, PrepTable& t, int nseg, const opose_params& p);
BatchGeom batch_geom(const opose_params& p, int H, int W);
void batch_preprocess(const uint8_t* frames, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                      const BatchGeom& g, float* x, hipStream_t stream);
bool extract_batch_ok(int N, int boxsize);
bool draw_dims_ok(int N, int H, int W);
int draw_cap(const opose_ctx* h, int joints);
void run_draw_setup(opose_ctx* h, const uint8_t* rec_dev, const double* motion_dev, int joints, int N, int H, int W,
                    int32_t* prims, int32_t* counts, int32_t* status_dev);
void run_hand_crops(opose_ctx* h, const uint8_t* fd, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                    const int32_t* boxes_dev, int bs, float* x, uint8_t* crops, int32_t* status_dev);
// engine_rccl.cpp
const Rccl& rccl();
void rccl_check(ncclResult_t r);

}  // namespace opose

#define OPOSE_TRY(h, ...)                      \
    try {                                      \
        __VA_ARGS__;                           \
    } catch (const std::invalid_argument& e) { \
        if (h) (h)->err = e.what();            \
        return OPOSE_E_SHAPE;                  \
    } catch (const opose::HipError& e) {       \
        if (h) (h)->err = e.what();            \
        return OPOSE_E_HIP;                    \
    } catch (const std::exception& e) {        \
        if (h) (h)->err = e.what();            \
        return OPOSE_E_WEIGHTS;                \
    }

struct opose_ctx {
    // launch-sequence cache: per call signature, the device work of the first call runs
    // eagerly (allocating every buffer), the second is captured into a hipGraph, later calls
    // replay it (one launch instead of ~150: single-frame latency is launch bound)
    std::map<std::string, opose::GraphEntry> graphs;
    bool use_graphs = getenv("OPOSE_NO_GRAPH") == nullptr;
    // set while run_graphed captures: run_scales_concurrently then keeps the capture on one
    // stream (no forked branches in any captured graph, see run_graphed)
    bool capturing = false;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    int ppp = 128, maxp = 96;
    // weights
    std::map<std::string, std::unique_ptr<opose::DevConv>> convs[2];
    opose::NetTable table[2];  // valid while loaded[net]
    bool loaded[2] = {false, false};
    // workspace
    // network convolutions: fp32-accurate split-bf16 kernel (default) or the fp32 MFMA kernel
    // (OPOSE_CONV=f32)
    bool x6 = [] {
        const char* e = getenv("OPOSE_CONV");
        return !(e && std::string(e) == "f32");
    }();
    // MaxPool2d fused into the preceding conv's epilogue (default); OPOSE_FUSED_POOL=0 at handle
    // creation: separate maxpool_x6 launches (A/B; bit-identical results)
    bool fused_pool = opose::env_flag("OPOSE_FUSED_POOL", true);
    // conv1_1 by the direct first-layer kernel (default); OPOSE_FIRST_DIRECT=0: implicit GEMM
    bool first_direct = opose::env_flag("OPOSE_FIRST_DIRECT", true);
    // the batched 3x3 / 7x7 convs on padded inputs by conv_win_x6 (input window in LDS;
    // OPOSE_CONV7_WIN=0: conv_x6 over the im2col stream, the cross-check of tests/test_gpu_x6.py)
    bool win7 = opose::env_flag("OPOSE_CONV7_WIN", true);
    // OPOSE_WINO=1: 3x3 layers that would run whole tiles on the window kernel run as Winograd
    // F(2,3) along x instead (conv_wino_x6, 2/3 of the MFMAs).  Opt-in: fp32-accurate and correct
    // (tests/test_gpu_x6.py), but slower than the window kernel on this hardware
    bool wino = opose::env_flag("OPOSE_WINO", false);
    int force_kernel = -1;  // opose_debug_conv_x6's X6P path: the family under test
    // a pyramid's heat-map average in one launch (heat_full_scales); OPOSE_HEAT_SCALES=0: one
    // launch per scale into the float64 accumulator (the bit-identity cross-check of
    // tests/test_gpu_scale_shard.py)
    bool heat_scales = opose::env_flag("OPOSE_HEAT_SCALES", true);
    // a CPM stage's closing 1x1 pair in one launch (conv1x1_chain_x6); OPOSE_FUSE_1X1=0: two
    // launches through an HBM intermediate (the cross-check of tests/test_gpu_x6.py)
    bool fuse1x1 = opose::env_flag("OPOSE_FUSE_1X1", true);
    // conv1_1 -> conv1_2 (window kernel) hand-off as fp32 units, split by conv1_2 (default);
    // OPOSE_C11_F32=0: as X6 (A/B, bit-identical)
    bool c11_f32 = opose::env_flag("OPOSE_C11_F32", true);
    // multi-frame segments whose windows overflow the LDS run as one segment per frame on the
    // window kernel (run_conv_x6_segs); OPOSE_SPLIT_FRAMES=0: conv_x6 for such launches (A/B)
    bool split_frames = opose::env_flag("OPOSE_SPLIT_FRAMES", true);
    // conv1_2 + pool by conv3_pool_win_x6 (input window in LDS; OPOSE_CONV12_WIN=0: conv_x6's
    // pooled 64 x 128 tile over the im2col stream)
    bool win12 = opose::env_flag("OPOSE_CONV12_WIN", true);
    // conv launch plans per launch signature (tile, grid) and the device copies of their unit
    // schedules (X6Args::sched; never freed while the handle lives: captured graphs hold them)
    std::map<std::string, opose::ConvPlan> plans;
    std::map<std::string, int> slab_cache;  // engine slab_count
    std::vector<int*> sched_mem;
    std::vector<std::vector<int>> sched_host;  // sources of the asynchronous uploads
    opose::DevBuf frames, mids[2][opose::kMaxScales], avg, cnt, list, peak_pos, part_cnt, score, conn, conn_cnt, records, maps_in,
        hlab, hsums, hpeaks, hfound, list_score, hsel;
    // gauss_nms_resize's hot-tile list (its count is the word after the peak counts in `cnt`)
    opose::DevBuf hot_tiles;
    // fast-mode hand extraction (opose_batch_hand_boxes / _crops / _extract): staged poses, the
    // boxes and per-slot status, staged results
    opose::DevBuf hx_motion, hx_boxes, hx_status, hx_crops, hx_handmat;
    // fast-mode body extraction (opose_body_records_pose / opose_batch_body_extract): staged poses
    // and per-frame status (the records are in `records`)
    opose::DevBuf px_pose, px_status;
    // drawing (opose_draw_records / opose_draw_motion): the primitive tables, per-frame counts and
    // status, staged poses, and the canvases of a call whose `out` is host memory
    opose::DevBuf draw_prims, draw_counts, draw_status, draw_motion, draw_out;
    // shapelet search (engine_shapelet.cpp): staged inputs (sequences, offsets, labels, pattern or
    // MotionMat rows), the block table, a chunk's minima / locations / scores, the running winner
    // and staged outputs; for the several-lengths calls also the per-(entry, length) rows and the
    // per-length tables handed to the selection
    opose::DevBuf shp_seq, shp_off, shp_labels, shp_in, shp_blocks, shp_min2, shp_loc, shp_num, shp_loss, shp_best,
        shp_carry, shp_out, shp_lrows, shp_sel;
    // opose_shapelet_scan: the pattern table and window lengths, a chunk's distance rows and hit
    // masks, its per-pair counts, the running total, and the staged occurrence outputs
    opose::DevBuf scan_pats, scan_m, scan_dist, scan_mask, scan_counts, scan_total, scan_off, scan_pos, scan_odist;
    // opose_shapelet_net_train: the model table, the two (distance, location) key buffers, g, the
    // head's per-clip terms, and the staged state and outputs of a call on host memory
    opose::DevBuf net_tab, net_best, net_g, net_ws, net_state, net_out;
    // opose_tgcn_forward: the staged input, a chunk's three activation buffers (a block's input,
    // middle and output), and the logits and per-copy logits the caller did not give device room for
    opose::DevBuf tg_x, tg_act[3], tg_out;
    // opose_batch_hand_extract cuts its 2N crops into chunks the conv kernels can address (as
    // opose_hand_infer_crops does); OPOSE_EXTRACT_CHUNK=n at handle creation: n crops per chunk
    // instead (tests/test_gpu_hand_extract.py runs a small batch in two chunks)
    int extract_chunk = [] {
        const char* e = getenv("OPOSE_EXTRACT_CHUNK");
        return e ? std::atoi(e) : 0;
    }();
    // the segment table of the last launch_preprocess_segs (kPrepSegs rows; written on the stream
    // right before the launch that reads it)
    opose::DevBuf prep_table;
    opose::PinnedBuf hand_out;  // Hand() peaks + found, staged for the host
    // network workspace, one set per concurrently running scale (slot s runs on scale_stream(s);
    // slot 0 is the handle's stream): input, activations, k-slab partials
    struct NetWS {
        opose::DevBuf x, xband, x6in, x6A, x6B, x6P0, x6P1, x6Q0, x6Q1, x6S0, x6S1, x6T0, x6T1, x6U, bufA, bufB, S0, S1, T0, T1, U, partial;
    };
    NetWS ws[opose::kMaxScales];
    int slot = 0;
    NetWS& w() { return ws[slot]; }
    // the scales of one Hand() call run concurrently on their own streams (OPOSE_SCALE_STREAMS=0:
    // one after another on the handle's stream, captured into a hipGraph)
    bool scale_streams = opose::env_flag("OPOSE_SCALE_STREAMS", true);
    // split-bf16 path: a pyramid's networks (Hand()'s four scales, a multi-scale Body's) in
    // lockstep, one conv launch per layer for all of them (default); OPOSE_LOCKSTEP=0: one network
    // per scale, concurrent streams when scale_streams (the reference of the lockstep tests; the
    // same outputs bit for bit: a pixel's summation order does not depend on the launch).
    int lockstep = [] {
        const char* e = getenv("OPOSE_LOCKSTEP");
        return e ? std::atoi(e) : 1;
    }();
    hipStream_t sstream[opose::kMaxScales] = {};
    hipEvent_t ev_fork = nullptr, ev_join[opose::kMaxScales] = {};
    // Cross-call pipelining of opose_body_infer calls flagged OPOSE_PIPELINE (device input and
    // output).  Call k's network part (preprocess, conv stack,
    // x8 upsample) runs on `nstream`, its post-network part on `stream` after an event; call
    // k+1's network then overlaps call k's post-network kernels (latency-bound launches of a few
    // dozen workgroups, and the CUs a 236-tile conv grid leaves idle).  The x8 maps (the only
    // buffers both parts touch) alternate between two sets; `nstream` waits for the post part
    // of the call two back before overwriting a set, and for `stream` whenever another entry
    // point used the shared network workspace there since (main_dirty).  Every call ends with
    // `stream` ordered after its own network part.
    hipStream_t nstream = nullptr;
    int nstream_prio = 0;
    // OPOSE_PIPELINE_DEFER: the last call's post-network part, enqueued by the next pipelined
    // call after that call's network recorded ev_gate (before its trunk's conv3_1), or by
    // flush_post.  gate_ev: set while a network part should record the gate.
    struct DeferredPost {
        bool pending = false;
        int N = 0, H = 0, W = 0, set = 0;
        std::vector<opose::ScaleGeom> gs;
        opose_params p{};
        uint8_t* rec = nullptr;
    } dpost;
    hipEvent_t ev_gate = nullptr, gate_ev = nullptr;
    bool gate_done = false;
    hipEvent_t ev_net = nullptr, ev_main = nullptr, ev_post[2] = {nullptr, nullptr};
    // opose_wait_stream / opose_signal_stream / opose_set_stream: ordering against streams the
    // caller owns (a framework's current stream)
    hipEvent_t ev_ext = nullptr, ev_sig = nullptr;
    hipEvent_t ev_in = nullptr;  // opose_signal_input
    bool post_pending[2] = {false, false};
    bool main_dirty = false;
    int mid_set = 0, next_set = 0;
    opose::DevBuf& mid(int s) { return mids[mid_set][s]; }
    // profiling
    bool prof = false;
    bool detail = false;  // per-layer aggregation (opose_profile_enable(h, 2))
    bool prof_conv7_only = false;  // opose_profile_enable(h, 3)
    std::vector<opose::ProfEntry> pending;
    std::map<std::string, opose::ProfAgg> agg;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t get_event();
    void prof_begin(opose::ProfEntry& pe, const char* cls, double flops, double bytes);
    void prof_end(opose::ProfEntry& pe);
    void prof_drain(bool all = false);
    // RCCL communicator for row-band halo exchanges (opose_rccl_init) and this handle's band
    // neighbours (opose_set_band_peers; -1: none)
    ncclComm_t comm = nullptr;
    int band_up = -1, band_dn = -1;
    ~opose_ctx();
    void release();
};
