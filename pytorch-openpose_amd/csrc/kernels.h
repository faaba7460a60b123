// kernels.h — host-side launchers for the libopose kernels.
#pragma once
#include <vector>

#include "common.h"
#include "shapelet.h"
#include "x6_pack.h"

namespace opose {

constexpr int kMaxScales = 8;

// PAF maps of every scale for on-demand evaluation at paf_score's sample points: either the x8
// map mid[s] ([N][cm][hs][ws], channel 0 = PAF x) or, when low[s] is set, the network's low-res
// PAF channels ([N][lcm][hl][wl]), whose x8 values are evaluated where the final resize reads them
// (cv2.resize(fx=fy=8) then the resize to H x W, src/body.py:55-63: the same float32 expressions in
// the same order as the staged upsample, so the same values)
struct PafScales {
    const float* mid[kMaxScales];  // [N][cm][hs][ws] per scale
    const float* low[kMaxScales];  // [N][lcm][hl][wl] per scale, or nullptr
    int hs[kMaxScales], ws[kMaxScales];
    int hl[kMaxScales], wl[kMaxScales];
    double sy[kMaxScales], sx[kMaxScales];  // source step of the final resize to H x W
    int n, cm, lcm, H, W;
    int torch;  // 1: torch bicubic taps (Batch_body fast mode), 0: OpenCV INTER_CUBIC
};

// src/body.py:97-99: the 19 limbs' parts, 0-based (post.hip's device tables and the host's)
#define OPOSE_LIMB_A {1, 1, 2, 3, 5, 6, 1, 8, 9, 1, 11, 12, 1, 0, 14, 0, 15, 2, 5}
#define OPOSE_LIMB_B {2, 5, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 0, 14, 16, 15, 17, 16, 17}
constexpr int kHostLimbA[19] = OPOSE_LIMB_A, kHostLimbB[19] = OPOSE_LIMB_B;

struct Conn {
    int i, j;
    double s;
};

// conv.hip
void launch_conv(const ConvArgs& a, const int* ktab, int mt, int pt, hipStream_t st);
void launch_fill_hash(float* p, size_t n, uint32_t seed, hipStream_t st);
void launch_maxpool(const float* in, float* out, int NC, int H, int W, hipStream_t st);

// conv_x6.hip (split-bf16 fp32-accurate convolution, X6 activation format: common.h; the weight
// packers x6_pack_weights / _pairs / _wino: x6_pack.h)
void launch_conv_x6(const X6Args& a, int mt, int pt, hipStream_t st);
// X6Args with the groups' tiles and work units numbered for an mt x pt tile (X6Group::t0 / u0,
// X6Args::tiles / units)
X6Args x6_number_tiles(const X6Args& a, int mt, int pt);
// slab fixup of a numbered 128 x 256 tile grid (conv_win_x6); nothing when every tile is whole
void launch_conv_x6_fixup(const X6Args& a, int mt, int pt, hipStream_t st);
void launch_to_x6(const float* in, int cstride, int coff, int C, int N, int HW, uint8_t* out, int cg, int goff,
                  uint32_t ps, hipStream_t st);
void launch_from_x6(const uint8_t* in, int cg, int goff, uint32_t ps, int C, int N, int HW, float* out, int cstride,
                    int coff, hipStream_t st);
// f32_out: fp32 units of 8 channels ([N][8][H*W] x 32 bytes) for launch_conv3_pool_win_x6's f32_in
// conv1_1 / conv1_2 of a pyramid's scales in one launch each: one segment per scale (input,
// output, piece strides, geometry); b0 is set by the launcher
constexpr int kConv1Segs = 8;
struct Conv1Seg {
    const void* in;
    uint8_t* out;
    uint32_t ips, ops;
    int N, H, W, b0;
};
struct Conv1Segs {
    Conv1Seg s[kConv1Segs];
    int n;
};
void launch_conv_first_x6_segs(Conv1Segs segs, const float* wt, int Mpad, const float* bias, bool f32_out,
                               hipStream_t st);
void launch_conv3_pool_win_x6_segs(Conv1Segs segs, const uint8_t* wt, const float* bias, bool f32_in, hipStream_t st);
void launch_conv_first_x6(const float* x, int N, int Cin, int H, int W, const float* wt, int Mpad, const float* bias,
                          uint8_t* out, uint32_t ops, bool f32_out, hipStream_t st);
// zero the padding units of `planes` X6P (piece, group) planes of an N x H x W buffer (common.h)
void launch_x6p_clear_pads(uint8_t* const* bufs, const int* planes, int nbufs, int N, int H, int W, hipStream_t st);
// 3 rows (padded row index row0 / row1) of groups [g0, g0 + ng) of a one-frame X6P buffer (ps
// bytes per piece, gs units per group plane, P units per row) <-> packed blocks blk0 / blk1
// ([piece][group][3 P] units); directions by mask bit 0 / 1
void launch_x6p_halo(uint8_t* x6p, uint32_t ps, uint32_t gs, int g0, int ng, int P, int row0, int row1, void* blk0,
                     void* blk1, int mask, bool unpack, hipStream_t st);
void launch_maxpool_x6(const uint8_t* in, uint32_t ips, uint8_t* out, uint32_t ops, int NG, int H, int W,
                       hipStream_t st);
// conv1_2 (64 -> 64, 3x3 pad 1) + MaxPool2d(2, 2) from an 8-group X6 tensor (f32_in: fp32 units,
// split in the kernel), input window in LDS
void launch_conv3_pool_win_x6(const uint8_t* in, uint32_t ips, int N, int H, int W, const uint8_t* wt,
                              const float* bias, uint8_t* out, uint32_t ops, bool f32_in, hipStream_t st);
// conv1x1_chain.hip: two chained 1x1 convs (CPM stage ends) in one launch, 64-pixel tiles
void launch_conv1x1_chain_x6(const X6ChainArgs& a, hipStream_t st);
// conv_win.hip: the 7x7 / 3x3 convs with the im2col operand from an LDS window of the padded X6P
// input (pair-order weights: x6_pack_weights_pairs); 128 x 256 tiles, work units (tile, k slab)
// the windows of an N x H x W batch's tiles fit the LDS
bool conv_win_fits(int N, int H, int W, int ks);
// the window of any 256-pixel run of one frame W columns wide fits the LDS (whatever the height)
bool conv_win_fits_rows(int W, int ks);
void launch_conv_win_x6(const X6Args& a, hipStream_t st);
// Winograd F(2,3) along x for 3x3 layers on X6P inputs (conv_wino.hip): weights U_v in pair order,
// tile slots per frame of a batch (-1: the window does not fit), whole-tile launch
int wino_tpf(int N, int H, int W);
void launch_conv_wino_x6(const X6Args& a, hipStream_t st);
// imgproc.hip
void launch_preprocess(const uint8_t* src, int64_t frame_stride, int64_t row_stride, int N, int H, int W, int Hs,
                       int Ws, double sy, double sx, int Hp, int Wp, float pad_val, float* out, hipStream_t st);
// launch_preprocess for up to kPrepSegs segments, each with its own frames and geometry, in one
// launch (preprocess_u8_segs).  A segment's row of the table, which the kernel reads from device
// memory: launch_preprocess's arguments, then what prep_table_blocks fills in.
constexpr int kPrepSegs = kMaxScales;
struct PrepSeg {
    const uint8_t* src;  // N frames [H][W][3]
    float* out;          // [N][3][Hp][Wp]
    int64_t frame_stride, row_stride;
    double sy, sx;
    int N, H, W, Hs, Ws, Hp, Wp;
    int bx;         // workgroups per output row
    int block_end;  // workgroups of this and every earlier segment
    int reserved;   // (no padding bytes: the struct travels as kernel argument words)
};
struct PrepTable {
    PrepSeg s[kPrepSegs];
};
// Checks the segments t.s[0 .. nseg) and fills their bx / block_end, writes the table to table_dev
// (kPrepSegs rows of device memory) with a store kernel and launches preprocess_u8_segs on it: two
// launches on st, with nothing read from host memory after the call returns (a stream capture
// replays both).
void launch_preprocess_segs(PrepTable& t, int nseg, float pad_val, PrepSeg* table_dev, hipStream_t st);
void launch_upsample8(const float* in, int in_cstride, int in_coff, int C, int N, int hl, int wl, int Hs, int Ws,
                      float* out, hipStream_t st);
void launch_heat_full(const float* mid, int Cm, int coff, int P, int N, int Hs, int Ws, int H, int W, double sy,
                      double sx, int nscales, int accumulate, double* avg, hipStream_t st);
// every scale of a pyramid's heat average in one launch (imgproc.hip heat_full_scales)
constexpr int kHeatScales = 8;
struct HeatScale {
    const float* mid;  // [N][Cm][Hs][Ws] x8 maps of this scale
    int Cm, coff, Hs, Ws;
    double sy, sx;
};
struct HeatScales {
    HeatScale s[kHeatScales];
    int n;
    float ns;  // len(multiplier): every scale's map is divided by it (float32) before the float64 add
};
bool heat_full_scales_fits(const HeatScales& S, int H, int W);
void launch_heat_full_scales(const HeatScales& S, int N, int P, int H, int W, double* avg, hipStream_t st);
void launch_heat_full_f32(const float* mid, int Cm, int coff, int P, int N, int Hs, int Ws, int H, int W, double sy,
                          double sx, float* avg, hipStream_t st);

// Batch_body fast mode (torch bicubic conventions)
void launch_preprocess_torch(const uint8_t* src, int64_t frame_stride, int64_t row_stride, int N, int H, int W, int nh,
                             int nw, float scale_y, float scale_x, int Hp, int Wp, float* out, hipStream_t st);
void launch_upsample8_torch(const float* in, int in_cstride, int in_coff, int C, int N, int hl, int wl, int nh, int nw,
                            float* out, hipStream_t st);
void launch_resize_torch_f32(const float* mid, int Cm, int coff, int P, int N, int nh, int nw, int H, int W,
                             float* out, hipStream_t st);

// handcrop.hip: the fast mode's hand extraction (boxes [N][2][4] = {x, y, w, present}, slot =
// 2 * frame + side, left then right)
void launch_hand_boxes(const double* motion, int N, int H, int W, int32_t* boxes, hipStream_t st);
void launch_hand_crops(const uint8_t* src, int64_t frame_stride, int64_t row_stride, int N, int H, int W,
                       const int32_t* boxes, int bs, float* x, uint8_t* crops, int32_t* status, hipStream_t st);
void launch_hand_backmap(const double* peaks, const int32_t* found, const int32_t* boxes, int N, int bs,
                         double* handmat, hipStream_t st);

// posemat.hip: the fast mode's person choice, N records of layout L -> pose [N][18][3], status [N]
void launch_pose_select(const uint8_t* records, int N, const RecordLayout& L, double* pose, int32_t* status,
                        hipStream_t st);

// draw.hip: skeletons drawn into uint8 frames.  draw_setup writes per frame a table of `cap`
// primitive slots of kDrawPrimInts int32 each, in draw order -- kind (0 none, 1 disc, 2 limb,
// 3 line), colour (c0 | c1 << 8 | c2 << 16), centre x, y (a line's first end), two parameters (a
// limb's semi-axis a and table degree, a line's second end), the box x0, y0, x1, y1 cut to the
// frame (half open; empty: zeros), two zeros -- with the frame's slot count (0 unless its status is
// OPOSE_OK) and status.  joints 0: the frames' Body records of layout L (cap 35 * L.max_people);
// 18 / 60: MotionMat rows [N][joints][3] (cap 35 / 117).
constexpr int kDrawPrimInts = 12;
constexpr int kDrawThreads = 256, kDrawTileW = 32, kDrawTileH = 8;  // a workgroup's pixel tile
void launch_draw_setup(const uint8_t* records, const RecordLayout& L, const double* motion, int joints, int N, int H,
                       int W, int cap, int32_t* prims, int32_t* counts, int32_t* status, hipStream_t st);
// src / dst: N frames [H][W][3] with frame / row strides in bytes; dst may be src (in place)
void launch_draw_pixels(const uint8_t* src, int64_t sfs, int64_t srs, uint8_t* dst, int64_t dfs, int64_t drs, int N,
                        int H, int W, const int32_t* prims, const int32_t* counts, int cap, hipStream_t st);

// shapelet.hip: shapelet search over motion data (limits, tile constants and ShpBlock: shapelet.h).
// off [n_seq + 1] is the ragged batch's row offsets on the device; carry: nblocks x 2 * joints int32
// of workspace (nblocks = fill blocks of kFeatRows rows)
void launch_motion_features(const double* motion, int64_t L, int joints, const int64_t* off, int n_seq, int mode,
                            int32_t* carry, float* out, hipStream_t st);
void launch_sliding_distance(const float* pat, int m, const float* seq, const int64_t* off, int n_seq, int D, int64_t L,
                             float* dist, hipStream_t st);
// min2 / loc [rows][n_seq] for every length of `lens` (one or more) in one pass over shared
// distances: `blocks` is the table of the shortest length, rows [n_blocks][lens.n] gives each
// (entry, length) its first output row and its count of valid starts
void launch_shapelet_mindist(const float* seq, const int64_t* off, int n_seq, int D, const ShpLens& lens,
                             const ShpBlock* blocks, const ShpLenRows* rows, int n_blocks, float* min2, int32_t* loc,
                             hipStream_t st);
void launch_shapelet_score(const float* min2, int n_cand, int n_seq, int n_labels, const uint8_t* labels, int negs,
                           int32_t* num, double* loss, hipStream_t st);
void launch_shapelet_select(const int32_t* num, const double* loss, int n_cand, const ShpBlock* blocks, int n_blocks,
                            const float* min2, const int32_t* loc, int n_seq, int first, int32_t* best,
                            double* best_loss, float* dis, int32_t* locs, hipStream_t st);
// The scan (opose_shapelet_scan), per chunk of patterns.  pats: n_groups * kScanPG table entries,
// each group sorted by length (m_max: the longest of the table); dist [slots][L] and mask [slots]
// [ceil(L / 64)] are the chunk's workspace.  lds: stage the stream tiles in LDS, which needs
// shapelet_scan_lds_bytes(m_max, D) <= kScanLdsBytes.  L >= 1.
size_t shapelet_scan_lds_bytes(int m_max, int D);
void launch_shapelet_scan_dist(const float* pat, const ScanPat* pats, int n_groups, int m_max, bool lds,
                               const float* seq, const int64_t* off, int n_seq, int64_t L, int D, float* dist,
                               uint64_t* mask, hipStream_t st);
void launch_shapelet_scan_mask(const float* dist, const int64_t* off, int n_seq, int64_t L, int m, float sigma,
                               uint64_t* mask, hipStream_t st);
// pairs (slot, stream), slot-major; m_slot [slots]: the window length of each slot.  write false:
// counts [n_pairs]; true: the entries from occ_off[pair] on, those at or past cap dropped
void launch_shapelet_scan_pick(const float* dist, const uint64_t* mask, const int32_t* m_slot, const int64_t* off,
                               int n_seq, int64_t L, int n_pairs, int32_t* counts, const int64_t* occ_off,
                               int32_t* occ_pos, float* occ_dist, int64_t cap, bool write, hipStream_t st);
// occ_off [n + 1] of a chunk from its counts, continuing the running total kept at *running
void launch_shapelet_scan_offsets(const int32_t* counts, int n, bool first, int64_t* running, int64_t* occ_off,
                                  hipStream_t st);

// shapelet_net.hip: the learned shapelet model (opose_shapelet_net_train).  models [n_models] and the
// concatenated queries / moments they index; best [n_models][n_seq] keys (bits of s) << 32 | c, all
// ones before a forward launch; tiles: ceil(most positions of any clip and model / kNetTC)
size_t shapelet_net_q_bytes(int m, int D);
size_t shapelet_net_x_bytes(int m, int D);
void launch_shapelet_net_forward(const float* seq, const int64_t* off, int n_seq, int D, int t_pad,
                                 const NetModel* models, int n_models, int m_max, int tiles, const float* query,
                                 uint64_t* best, hipStream_t st);
// g [n_models][n_seq], ws [n_models][5][n_seq]; next, g, loss_out, dis / locs / correct and dhead may
// be null (shapelet_net.hip says what each is)
void launch_shapelet_net_head(const uint64_t* best, uint64_t* next, const uint8_t* labels, int n_seq, int n_models,
                              float* head, float* head_m, float* head_v, float step, float bc2s, bool update, float* g,
                              double* ws, double* loss_out, int64_t loss_stride, float* dis, int32_t* locs,
                              int32_t* correct, double* dhead, hipStream_t st);
// the query's Adam step in place, or with dq_out the gradient alone
void launch_shapelet_net_step(const float* seq, const int64_t* off, int n_seq, int D, const NetModel* models,
                              int n_models, int m_max, const uint64_t* best, const float* g, float* query, float* q_m,
                              float* q_v, float step, float bc2s, float* dq_out, hipStream_t st);

// tgcn.hip: the TGCN sign classifier (opose_tgcn_forward).  A graph-convolution layer is one launch
// of tgcn_gc: workgroup (column tile of kTgcnTN, group of kTgcnG samples), 4 waves, wave w owning
// rows 16 w .. 16 w + 15 of the kTgcnV padded nodes.
constexpr int kTgcnV = 64, kTgcnG = 4, kTgcnTN = 64, kTgcnThreads = 256;
constexpr int kTgcnMaxF = 1024, kTgcnMaxC = 4096, kTgcnMaxStage = 64;
// units (16 bytes, 8 bf16) of a layer's packed W [H tiles][F chunks of 32][3 pieces][4 k-groups][64
// columns] and of its packed att [2 k-steps][3 pieces][4 k-groups][64 rows]
inline size_t tgcn_w_units(int F, int H) {
    return (size_t)((H + kTgcnTN - 1) / kTgcnTN) * ((F + 31) / 32) * 3 * 4 * kTgcnTN;
}
constexpr size_t kTgcnAttUnits = 2 * 3 * 4 * kTgcnV;
struct TgcnLayer {
    const uint8_t* w;    // packed W
    const uint8_t* att;  // packed att
    const float* a;      // [V][H] folded batch-norm scale
    const float* c;      // [V][H] folded batch-norm shift (the layer's bias included)
    int F, H;
};
// x: sample n of the launch is rows of ld floats at x + ((n_in0 + n) / copies) V ld + ((n_in0 + n) %
// copies) F; res (or null) and out: [n][V][H] dense
void launch_tgcn_gc(const TgcnLayer& L, int V, const float* x, int64_t ld, int copies, int64_t n_in0, int n,
                    const float* res, float* out, hipStream_t st);
// y [n1 - n0][V][H]: the last layer's output of the global samples n0 .. n1 - 1 (sample = b copies +
// i); copy_logits [B copies][C] and logits [B][C] are indexed globally
void launch_tgcn_head(const float* y, int64_t n0, int64_t n1, int copies, int V, int H, int C, const float* fcT,
                      const float* fcb, float* copy_logits, float* logits, hipStream_t st);

// post.hip
void launch_gauss_nms(const void* avg, bool f32, int NP, int H, int W, double thre, int cap, int* cnt, int* list,
                      double* list_score, hipStream_t st);
// single scale: heat_full's resize of mid channels [coff, coff+P) fused into the wide NMS
// (requires gauss_nms_resize_fits: a true resize with source step sy <= 0.618 from a map of at
// most 4096 columns).  Two launches: a screen that lists the tiles whose sources can reach the
// threshold (hot_list: gauss_nms_resize_tiles ints, ids (np * tile rows + ty) * tile columns + tx
// in no defined order; *hot_cnt: their number, zero on entry), then the NMS over that list in a
// fixed grid (max_grid > 0 caps it: the debug hook's way to make few workgroups loop).
bool gauss_nms_resize_fits(int Hs, int Ws, int H, int W, double sy);
int gauss_nms_resize_tiles(int N, int P, int H, int W);
void launch_gauss_nms_resize(const float* mid, int Cm, int coff, int P, int N, int Hs, int Ws, int H, int W, double sy,
                             double sx, double thre, int cap, int* cnt, int* list, double* list_score, int* hot_cnt,
                             int* hot_list, int max_grid, hipStream_t st);
// Batch_body fast mode: 5x5 Gaussian (reflect pad, srcmx/utilmx.py:246-263) + findpeaks_torch
// (srcmx/utilmx.py:230-243) on heat [NP][H][W] float; scores = blurred values
void launch_blur5_nms(const float* heat, int NP, int H, int W, double thre, int cap, int* cnt, int* list,
                      double* list_score, hipStream_t st);
// Batch_hand fast mode: blurred (5x5, float64 out) + union-find seeds of blurred > thre
void launch_blur5_seed(const float* heat, int NP, int H, int W, double thre, double* blurred, int* lab, int* cnt,
                       hipStream_t st);
// sums: zeroed at every tile-local root (the component sums' only addresses; launch_hand_cc)
void launch_gauss_threshold(const double* avg, int NP, int H, int W, double thre, int* lab, int* cnt, double* sums,
                            hipStream_t st);
void launch_peaks_finalize(const int* cnt, const int* list, const double* list_score, int N, int H, int W,
                           const RecordLayout& L, uint8_t* records, int* peak_pos, int* part_cnt, hipStream_t st);
void launch_paf_score(const PafScales& S, const int* peak_pos, const int* part_cnt, int N, int cap, double thre2,
                      double* score, hipStream_t st);
void launch_limb_greedy(const double* score, const int* part_cnt, int N, int cap, Conn* conn, int* conn_cnt,
                        hipStream_t st);
void launch_assemble(const Conn* conn, const int* conn_cnt, const int* part_cnt, int N, const RecordLayout& L,
                     uint8_t* records, hipStream_t st);
// connections assemble_people stages in LDS at once: a frame with more takes them limb by limb
int assemble_stage(const RecordLayout& L);

// hand.hip
size_t hand_cc_workspace_bytes(int NP);
// tile_seeds: lab labelled per gauss_threshold tile (only tile edges left to join); else run seeds
// (blur5_seed)
void launch_hand_cc(double* avg, int NP, int H, int W, int* lab, double* sums, const int* cnt, double* peaks,
                    int* found, void* ws, bool tile_seeds, hipStream_t st);

}  // namespace opose
