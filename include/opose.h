/*
 * opose.h — C ABI of libopose.so, the MI355X-native OpenPose Body/Hand inference path.
 *
 * Drop-in boundary for hitmaxiang/pytorch-openpose `src/` (pure Python in the reference;
 * these entry points are what a ctypes/cffi binding of that path binds — see INTEGRATION.md):
 *
 *   reference interface (file:line)                         replaced by
 *   ------------------------------------------------------  -----------------------------------
 *   Body.__init__ / Hand.__init__  src/body.py:16-22,        opose_create + opose_load_weights
 *                                  src/hand.py:17-23
 *   util.transfer                  src/util.py:36-40         key mapping done by the caller; tensors
 *                                                            passed in reference state_dict order
 *   bodypose_model.forward         src/model.py:106-133      opose_body_forward
 *   handpose_model.forward         src/model.py:197-214      opose_hand_forward
 *   Body.__call__                  src/body.py:24-212        opose_body_infer
 *   Body.__call__ after the net    src/body.py:52-212        opose_body_post   (parity entry point)
 *   Hand.__call__                  src/hand.py:25-75         opose_hand_infer
 *   Hand.__call__ after the net    src/hand.py:51-75         opose_hand_post   (parity entry point)
 *   HandImageDataset.__getitem__   srcmx/Batch_model.py:     opose_batch_hand_boxes (+ utilmx.handDetect),
 *                                  69-104                    opose_batch_hand_crops (parity entry point)
 *   Batch_hand_extraction's loop   srcmx/Batch_motion_       opose_batch_hand_extract
 *                                  Estimation.py:19-65
 *   Batch_body_extraction's loop   srcmx/Batch_motion_       opose_batch_body_extract;
 *                                  Estimation.py:83-108      opose_body_records_pose (parity entry point)
 *   one scale of Body.__call__     src/body.py:36-50         opose_body_scale_maps; its output rows
 *                                                            opose_body_band_maps (C5 split)
 *   util.draw_bodypose             src/util.py:44-77         opose_draw_records
 *   DisplayPose's canvas           srcmx/MotionEstimation.py opose_draw_motion (draw_bodypose +
 *                                  :281-295                  utilmx.draw_handpose_by_opencv)
 *   MotionJointFeatures            srcmx/PreprocessingData   opose_motion_features
 *                                  .py:16-125
 *   SlidingDistance(_torch)        srcmx/utilmx.py:330-372   opose_sliding_distance
 *   ShapeletMatrixModel.train      srcmx/shapeletmodel.py:   opose_shapelet_find;
 *                                  97-209                    opose_shapelet_mindist (first stage)
 *   ShapeletsFinding.train's       srcmx/shapeletlearning    opose_shapelet_find_lengths;
 *   m_len loop                     .py:123-175               opose_shapelet_mindist_lengths
 *   DataAugmentation.              srcmx/DataAugmentation    opose_shapelet_scan;
 *   AugmentateOneShapelet          .py:78-153                opose_debug_shapelet_pick (the hit walk)
 *   ShapeletNetModel (train,       srcmx/shapeletmodel.py:   opose_shapelet_net_train;
 *   __call__, localizeshape)       11-90                     opose_debug_shapelet_net_grad (one backward)
 *   GCN_muti_att (eval forward)    cls/TGCN/tgcn_model.py:   opose_tgcn_create + opose_tgcn_forward;
 *                                  93-129                    opose_debug_tgcn_layer (one layer)
 *   test()'s four-copy mean        cls/TGCN/test_tgcn.py:    opose_tgcn_forward (copies)
 *                                  31-39
 *
 * Conventions: plain pointers and sizes only; 0 = OK, negative = error (see opose_status).
 * Host pointers are caller-owned and read-only; the library copies them. A handle owns one
 * device, one HIP stream (or the caller's, see opose_set_stream), its weights and workspace.
 * Calls on one handle must be serialised by the caller; handles are independent.
 */
#ifndef OPOSE_H
#define OPOSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct opose_ctx opose_t;

typedef enum opose_status {
    OPOSE_OK = 0,
    OPOSE_E_ARG = -1,        /* bad argument / null pointer                         */
    OPOSE_E_SHAPE = -2,      /* unsupported shape                                   */
    OPOSE_E_HIP = -3,        /* HIP runtime error (message in opose_last_error)     */
    OPOSE_E_WEIGHTS = -4,    /* weights missing or of the wrong shape               */
    OPOSE_E_CAPACITY = -5,   /* a per-frame record overflowed (peaks/people)        */
    OPOSE_E_ASSEMBLY = -6,   /* reference IndexError: a 3rd subset row matched a
                                connection (src/body.py:170-173)                    */
    OPOSE_E_TIMEOUT = -7,    /* opose_rccl_wait: the halo exchange made no progress
                                before the deadline (communicator aborted)          */
} opose_status;

enum { OPOSE_NET_BODY = 0, OPOSE_NET_HAND = 1 };

/* flags for *_infer / *_post / *_forward */
enum {
    OPOSE_IN_DEVICE = 1,     /* input pointer is device memory                      */
    OPOSE_OUT_DEVICE = 2,    /* output pointer is device memory; call is async on the
                                handle's stream                                     */
    OPOSE_PIPELINE = 4,      /* opose_body_infer with IN_DEVICE | OUT_DEVICE only: the
                                input frames are complete when the call is made (not
                                produced by work still queued on the handle's stream) and
                                stay unmodified until the handle's stream passes the
                                call. The call's network part then runs on a second
                                stream and overlaps the previous call's post-network
                                part; records are still complete in the handle's stream
                                order. Video-batch throughput mode.                 */
    OPOSE_PIPELINE_DEFER = 8,/* with OPOSE_PIPELINE: the call's post-network part is
                                enqueued by the next OPOSE_PIPELINE call once that call's
                                network has reached its trunk's conv3_1 (so it overlaps
                                the middle of the next network, not its first layers),
                                or by opose_flush.  The records are complete in the
                                handle's stream order only after that; the records and
                                frames buffers must stay alive until then.  Every other
                                entry point (and opose_synchronize / opose_signal_stream
                                / opose_set_stream / opose_destroy) flushes first.  */
};

#define OPOSE_MAX_SCALES 8

/* Hard-coded locals of the reference, exposed with the reference defaults
 * (src/body.py:25-31, src/hand.py:26-31). */
typedef struct opose_params {
    int n_scales;
    double scales[OPOSE_MAX_SCALES]; /* scale_search; Body default {0.5}, Hand {0.5,1,1.5,2} */
    double boxsize;                  /* 368  */
    int stride;                      /* 8    */
    int pad_value;                   /* 128  */
    double thre1;                    /* 0.1  body peak threshold                  */
    double thre2;                    /* 0.05 PAF sample threshold                 */
    double thre_hand;                /* 0.03 hand component threshold             */
} opose_params;

void opose_default_params(int net, opose_params* p);

/* ---- lifetime ---------------------------------------------------------------------- */
/* A handle is used by one thread at a time; handles on different threads run concurrently. */
int opose_create(int device, opose_t** out);
void opose_destroy(opose_t* h);
const char* opose_last_error(const opose_t* h);
/* The new stream is ordered after all work queued on the previous one (and on the pipelined
 * network stream). */
int opose_set_stream(opose_t* h, void* hip_stream);   /* NULL = the handle's own stream */
void* opose_get_stream(const opose_t* h);
int opose_synchronize(opose_t* h);
/* Enqueue a post-network part deferred by OPOSE_PIPELINE_DEFER (no-op otherwise): afterwards the
 * last call's records are complete in the handle's stream order. */
int opose_flush(opose_t* h);
/* Ordering against a caller's stream (e.g. the framework's current stream) for OPOSE_IN_DEVICE /
 * OPOSE_OUT_DEVICE calls.  The reference computes synchronously on one device, so these replace
 * the implicit ordering of its `torch.from_numpy(...).cuda()` / `.cpu()` round trips
 * (src/body.py:44-50).
 *   opose_wait_stream:   the handle's next work (either stream) starts after everything queued on
 *                        `hip_stream` so far: device inputs produced there are complete.
 *   opose_signal_stream: work queued on `hip_stream` from now on starts after everything queued
 *                        on the handle's stream so far: device outputs are complete, and buffers
 *                        the handle read can be freed or reused by `hip_stream`. */
int opose_wait_stream(opose_t* h, void* hip_stream);
int opose_signal_stream(opose_t* h, void* hip_stream);
/*   opose_signal_input:  work queued on `hip_stream` from now on starts once the handle has read
 *                        the device inputs of every call made so far, so those buffers may be
 *                        refilled there.  After OPOSE_PIPELINE calls that is the end of the last
 *                        call's network part, before its post-network part: the next frames'
 *                        upload overlaps the post-network kernels instead of waiting for them
 *                        (the reference's per-frame `.cuda()` upload, src/body.py:44-45, in a
 *                        video loop).  Otherwise it is opose_signal_stream. */
int opose_signal_input(opose_t* h, void* hip_stream);

/* Capacity of one Body record: peaks kept per part and people kept per frame.
 * Defaults 96 / 96.  Overflow makes the frame's status OPOSE_E_CAPACITY. */
int opose_set_capacity(opose_t* h, int peaks_per_part, int max_people);

/* Per-frame Body record (fixed size, the unit of the multi-GPU gather):
 *   int32  status, n_cand, n_people, reserved
 *   double candidate[18*peaks_per_part][4]    x, y, score, id  (src/body.py:160,211)
 *   double subset[max_people][20]             ids (-1) | total score | part count */
size_t opose_body_record_bytes(const opose_t* h);

/* ---- weights ------------------------------------------------------------------------ */
/* tensors[i] = host fp32 data of the i-th state_dict tensor in reference order
 * (weight, bias per conv; OIHW); shapes = n x 4 int64 (bias: {C,1,1,1}). */
int opose_load_weights(opose_t* h, int net, const float* const* tensors,
                       const int64_t* shapes, int n);

/* ---- network only (src/model.py forward) ------------------------------------------- */
/* x [N,3,Hp,Wp] fp32 NCHW (Hp, Wp multiples of 8); paf [N,38,Hp/8,Wp/8], heat [N,19,..] */
int opose_body_forward(opose_t* h, const float* x, int N, int Hp, int Wp,
                       float* paf, float* heat, int flags);
/* heat [N,22,Hp/8,Wp/8] */
int opose_hand_forward(opose_t* h, const float* x, int N, int Hp, int Wp, float* heat, int flags);
/* The networks of a scale pyramid in one lockstep pass, as Hand() runs them (src/hand.py:33-57
 * evaluates self.model once per scale_search entry): xs[i] [N[i],3,Hp[i],Wp[i]] -> heats[i]
 * [N[i],22,Hp[i]/8,Wp[i]/8], i < n <= OPOSE_MAX_SCALES; one conv launch per layer covers
 * every scale (split-bf16 path; the fp32 path runs the scales one after another). */
int opose_hand_forward_pyramid(opose_t* h, int n, const float* const* xs, const int* N, const int* Hp,
                               const int* Wp, float* const* heats, int flags);

/* ---- end to end ---------------------------------------------------------------------- */
/* bgr: N frames uint8 [H][W][3] (row stride `row_stride` bytes, frame stride
 * `frame_stride` bytes); records: N * opose_body_record_bytes(). Returns the worst
 * per-frame status (each record carries its own). */
int opose_body_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W,
                     int64_t row_stride, int64_t frame_stride, const opose_params* p,
                     void* records, int flags);

/* Body.__call__ (src/body.py:24-212) for n_groups groups of frames in one lockstep pass: group g is
 * N[g] frames uint8 [H[g]][W[g]][3] at bgr[g] with strides row_stride[g] / frame_stride[g] (bytes),
 * records[g] receives its N[g] records.  Replaces a loop of Body.__call__ over frames of different
 * sizes (a folder of photographs, several cameras): every (group, scale) pair is one segment of the
 * network's launches, so a conv launch per layer covers all of them, and one preprocess launch
 * reads every group's frames.  A group's records are those opose_body_infer gives for that group
 * alone, bit for bit, whatever runs beside it: a conv sums a pixel in an order fixed by the layer
 * and the group's own N x H x W.  n_groups * p->n_scales <= OPOSE_MAX_SCALES.
 * OPOSE_IN_DEVICE / OPOSE_OUT_DEVICE as opose_body_infer (every bgr[g] / every records[g]; the
 * pointer arrays themselves are host memory, read before the call returns); OPOSE_PIPELINE is not
 * taken (OPOSE_E_ARG).  Returns the worst per-frame status of all groups.  The fp32 path
 * (OPOSE_CONV=f32) and OPOSE_LOCKSTEP=0 run the groups one after another. */
int opose_body_infer_groups(opose_t* h, int n_groups, const uint8_t* const* bgr, const int* N,
                            const int* H, const int* W, const int64_t* row_stride,
                            const int64_t* frame_stride, const opose_params* p,
                            void* const* records, int flags);

/* Post-network body path on a single scale (what follows src/body.py:50):
 * maps [N,57,h,w] fp32 (channels 0..37 PAF, 38..56 heat), padded net input (h*8, w*8),
 * pad_down / pad_right as util.padRightDownCorner, frame H x W. */
int opose_body_post(opose_t* h, const float* maps, int N, int hl, int wl, int pad_down,
                    int pad_right, int H, int W, const opose_params* p, void* records, int flags);

/* ---- scale-sharded single-frame latency (one scale of src/body.py:34-50 per rank) ------- */
/* Geometry of scale s of p->scales for an H x W frame (src/body.py:35-41): out4 = {hl, wl,
 * pad_down, pad_right} = network output size and util.padRightDownCorner's pads. */
int opose_body_scale_geom(int H, int W, const opose_params* p, int s, int* out4);

/* Network maps of scale s only (src/body.py:36-50 for one m): maps [N,57,hl,wl] fp32
 * (channels 0..37 PAF, 38..56 heat), host memory unless OPOSE_OUT_DEVICE. */
int opose_body_scale_maps(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                          int64_t frame_stride, const opose_params* p, int s, float* maps, int flags);

/* Row band [r0, r1) of scale s's network maps for ONE frame, for splitting a large scale across
 * ranks (736x1312 is 53 % of the pyramid's FLOPs; src/body.py:36-50 for one
 * m, cut into output rows).  Every rank of a band group runs the VGG trunk on its band's rows
 * plus a 10-row margin past each cut (recomputed, not exchanged), then the six CPM stages
 * (src/model.py:106-133) on its own rows only.  Before each 3x3 / 7x7 stage layer that needs
 * them, the 3 rows on either side of the band are exchanged with the neighbouring bands: the
 * library packs its top and bottom 3 rows
 * into xbuf's send halves on its stream, calls fn(user, bytes, stream), and unpacks the recv
 * halves.  fn moves send_up to the band above (its recv_dn) and send_dn to the band below (its
 * recv_up), ordered on `stream` (a hipStream_t) or synchronously, and returns 0; it is called
 * 27 times per frame and never for a single band covering every row (fn == NULL: see below).
 *   xbuf: device memory, 4 x opose_body_band_halo_bytes(wl) bytes = [send_up | send_dn |
 *         recv_up | recv_dn];  r1 - r0 >= 3;  maps [57, r1-r0, wl] fp32 (host unless
 *         OPOSE_OUT_DEVICE);  bgr one H x W frame (device with OPOSE_IN_DEVICE).
 * Every conv sums each pixel in the order the whole frame's network does (k slabs fixed by the
 * layer and the frame), so concatenating every band's maps gives
 * opose_body_scale_maps(s) bit for bit. */
typedef int (*opose_halo_fn)(void* user, size_t bytes, void* stream);
/* fn == NULL: the library exchanges the halos itself, RCCL send/recv on the handle's stream with
 * the ranks set by opose_set_band_peers, over the communicator of opose_rccl_init (no host code
 * between the stage layers). */
int opose_rccl_unique_id(void* id, size_t len);  /* len >= 128; call on one rank, share the bytes */
int opose_rccl_init(opose_t* h, const void* id, int rank, int nranks);
/* A band rank failed: ncclCommAbort on the handle's communicator (this rank's own queued halo
 * send / recv exit) and drop it; opose_rccl_init builds a new one.  The abort does not reach the
 * neighbours' queued kernels: they bound their wait with opose_rccl_wait. */
int opose_rccl_abort(opose_t* h);
/* Wait for the handle's stream (where the RCCL halo send / recv of opose_body_band_maps run) with a
 * deadline.  Returns OPOSE_OK when the work completed.  If the communicator reports an
 * asynchronous error, or the stream is still busy after timeout_ms (a band neighbour failed and
 * will never post its side of an exchange), the handle's own communicator is aborted: RCCL's abort
 * flag makes this rank's queued send / recv kernels exit, so the stream drains instead of waiting
 * forever; returns OPOSE_E_HIP / OPOSE_E_TIMEOUT, and opose_rccl_init builds a new communicator.
 * A failing rank's ncclCommAbort cannot reach its neighbours' queued kernels (xGMI P2P has no
 * peer-failure signal), so each neighbour bounds its own wait with this call (src/dist.py). */
int opose_rccl_wait(opose_t* h, int timeout_ms);
int opose_set_band_peers(opose_t* h, int up, int dn);  /* communicator ranks; -1: none */
size_t opose_body_band_halo_bytes(int wl);
int opose_body_band_maps(opose_t* h, const uint8_t* bgr, int H, int W, int64_t row_stride,
                         const opose_params* p, int s, int r0, int r1, float* maps,
                         opose_halo_fn fn, void* user, void* xbuf, size_t xbuf_bytes, int flags);

/* Multi-scale post-network body path (src/body.py:51-203): maps[s] = [N,57,hl[s],wl[s]] of
 * every scale (any rank's output of opose_body_scale_maps, gathered); the per-scale x8 /
 * crop / resize, the float64 scale average and everything after it, as opose_body_infer. */
int opose_body_post_scales(opose_t* h, const float* const* maps, const int* hl, const int* wl,
                           const int* pad_down, const int* pad_right, int n_scales, int N, int H,
                           int W, const opose_params* p, void* records, int flags);

/* Batched "fast mode" of the reference (srcmx/Batch_model.py:137-204 Batch_body.__call__):
 * torch-bicubic pre/post-processing (inputs as transforms.ToTensor would give: uint8 / 255),
 * single scale p->scales[0] (Batch_body: 0.5), 5x5 Gaussian + peak scores from the blurred
 * heat map, then the same limb scoring / matching / assembly as Body.  Records as
 * opose_body_infer. */
int opose_batch_body_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const opose_params* p, void* records, int flags);

/* Post-network part of the fast mode (srcmx/Batch_model.py:159-204): maps = [N,57,hl,wl]
 * (PAF 38 | heat 19), nh x nw = int(H*s) x int(W*s) = the crop of the x8 maps, frame H x W. */
int opose_batch_body_post(opose_t* h, const float* maps, int N, int hl, int wl, int nh, int nw,
                          int H, int W, const opose_params* p, void* records, int flags);

/* Fast-mode hand (srcmx/Batch_model.py:310-354 Batch_hand.__call__): N crops already resized
 * to H x W (the data loader's boxsize, a multiple of 8) as uint8 BGR; network at scale 1,
 * torch bicubic x8, 5x5 Gaussian, components of blurred > p->thre_hand (Batch_hand: 0.035)
 * selected on the blurred map.  peaks [N][21][3] in the H x W frame, found [N][21]. */
int opose_batch_hand_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const opose_params* p, double* peaks, int32_t* found,
                           int flags);

/* Post-network part of the fast-mode hand (srcmx/Batch_model.py:334-354): maps = [N,22,hl,wl]
 * network outputs; peaks in the (8 hl) x (8 wl) frame. */
int opose_batch_hand_post(opose_t* h, const float* maps, int N, int hl, int wl, const opose_params* p,
                          double* peaks, int32_t* found, int flags);

/* ---- fast-mode hand extraction (srcmx/Batch_motion_Estimation.py:19-65 Batch_hand_extraction) -- */
/* Slots: every frame has two, left then right; slot = 2 * frame + side.  A box is int32
 * {x, y, w, present}: the square frame[y:y+w, x:x+w] utilmx.handDetect gives for that side, all
 * zeros when the side's shoulder, elbow or wrist is missing from the pose.  boxsize must be a
 * positive multiple of 8 (else OPOSE_E_ARG).  With OPOSE_IN_DEVICE the inputs (bgr, motion,
 * boxes) are device memory; with OPOSE_OUT_DEVICE the outputs are, and the call is asynchronous
 * on the handle's stream (it then returns OPOSE_OK: the per-slot status is the caller's to read).
 * A region of interest of larger frames is a pointer offset plus the frames' row_stride. */

/* HandImageDataset.__getitem__'s subset construction + utilmx.handDetect (srcmx/Batch_model.py:
 * 74-84, srcmx/utilmx.py:267-327) for N poses motion [N][18][3] (x, y, score; a joint whose three
 * values sum to 0 is missing) in H x W frames: boxes [N][2][4]. */
int opose_batch_hand_boxes(opose_t* h, const double* motion, int N, int H, int W, int32_t* boxes, int flags);

/* The crops HandImageDataset cuts (srcmx/Batch_model.py:86-99) as uint8 BGR
 * [N][2][boxsize][boxsize][3]: cv2.resize(INTER_CUBIC) of each box, the left hand's mirrored first
 * (cv2.flip(.., 1)); an absent slot is gray (128).  A present box with w < 1 or outside the frame
 * reads nothing, is written gray and makes the call return OPOSE_E_SHAPE (the reference dies in
 * cv2.resize there).  Parity entry point: opose_batch_hand_extract builds the network input in the
 * same kernel without the uint8 intermediate. */
int opose_batch_hand_crops(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const int32_t* boxes, int boxsize, uint8_t* crops, int flags);

/* N frames + their N body poses -> HandMat rows handmat [N][42][3] (left hand rows 0..20, right
 * 21..41; x, y in frame pixels, score; a missing part is 0, 0, 0): boxes, crops, the hand network
 * and Batch_hand's post-processing (p as opose_batch_hand_infer: p->thre_hand) on all 2N crops,
 * and the loop body of Batch_hand_extraction (srcmx/Batch_motion_Estimation.py:44-58), with no
 * host round trip in between.  An absent hand's positions are 0 and its scores whatever the
 * network finds on the gray crop, as the reference stores them.  status [N][2]: OPOSE_OK, or
 * OPOSE_E_SHAPE for a present box that is empty (see opose_batch_hand_crops); returns the worst. */
int opose_batch_hand_extract(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                             int64_t frame_stride, const double* motion, int boxsize, const opose_params* p,
                             double* handmat, int32_t* status, int flags);

/* ---- fast-mode body extraction (srcmx/Batch_motion_Estimation.py:68-113 Batch_body_extraction) -- */
/* The loop body of Batch_body_extraction (:88-107) on N Body records (made by opose_body_infer,
 * opose_batch_body_infer or a *_post entry point at the handle's current capacity; 8-byte
 * aligned): per frame the person with the largest left-shoulder x -- candidate[int(subset[p][5])][0],
 * an absent shoulder's -1 reading the last candidate row as Python's negative index does, the
 * first person among equal maxima as np.argmax -- and that person's keypoints as a PoseMat row
 * pose [N][18][3] (x, y, score; a missing keypoint, and every row of a frame without people, is
 * 0, 0, 0).  The values are copied: bit-exact float64.  status [N]: OPOSE_OK; the record's own
 * status when that is not OPOSE_OK (zero row; the rest of the record is not read); OPOSE_E_ARG for
 * a record whose subset names a candidate row it does not hold (zero row; no address outside the
 * record is read).  Records and outputs are host memory, or device memory with OPOSE_IN_DEVICE /
 * OPOSE_OUT_DEVICE; with OPOSE_OUT_DEVICE the call is asynchronous on the handle's stream and
 * returns OPOSE_OK (the per-frame status is the caller's to read), else it returns the worst
 * per-frame status.  Parity entry point. */
int opose_body_records_pose(opose_t* h, const void* records, int N, double* pose, int32_t* status, int flags);

/* N frames -> PoseMat rows: opose_batch_body_infer into a record buffer the library owns, then
 * opose_body_records_pose on it, on the handle's stream with no host round trip in between; the
 * records never leave the device.  Arguments as opose_batch_body_infer, pose / status / the return
 * value as opose_body_records_pose (a frame that overflows the record capacity: OPOSE_E_CAPACITY
 * and a zero row). */
int opose_batch_body_extract(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                             int64_t frame_stride, const opose_params* p, double* pose, int32_t* status,
                             int flags);

/* ---- drawing (src/util.py:44-77 draw_bodypose, srcmx/utilmx.py:212-227 draw_handpose_by_opencv,
 * srcmx/MotionEstimation.py:281-295 DisplayPose) ------------------------------------------------ */
/* Skeletons drawn over N frames bgr uint8 [H][W][3] (strides in bytes, as opose_body_infer; H, W <=
 * 16384) into `out`: a dense [N][H][W][3] buffer, or bgr itself to draw in place.  Colours go to
 * channels 0, 1, 2 in the order the reference lists them; every coordinate is truncated toward zero
 * first, as the reference's int() does.  The covered pixels follow one rule, restated in NumPy by
 * tests/draw_cases.py and equal to it bit for bit (OpenCV's own edge pixels are not restated):
 *   disc  (cv2.circle, radius 4)      dx*dx + dy*dy <= 16 from the centre; opaque
 *   limb  (ellipse2Poly + fillConvexPoly + addWeighted 0.4 / 0.6) about the reference's centre
 *         (int(mean x), int(mean y)), with a = int(length / 2), (c, s) = cos / sin of int(angle)
 *         whole degrees and A = a + 0.5, B = 4.5:  u = dx*c + dy*s, v = dy*c - dx*s, covered iff
 *         u*u*(B*B) + v*v*(A*A) <= (A*A)*(B*B) in float64; a covered pixel becomes
 *         rint(old * 0.4 + colour * 0.6), half to even; others keep their value
 *   line  (cv2.line, thickness 2)     squared distance to the segment <= 1, in integers; opaque
 * status [N] per frame: OPOSE_OK, or the frame is left as it was (in place: untouched; else copied)
 * -- OPOSE_E_ARG when a coordinate that would be drawn is not finite or outside +-16384.  With
 * OPOSE_IN_DEVICE the inputs (bgr and records / motion) are device memory; with OPOSE_OUT_DEVICE
 * out and status are, and the call is asynchronous on the handle's stream and returns OPOSE_OK;
 * else it returns the worst per-frame status.
 *
 * opose_draw_records: util.draw_bodypose(frame, candidate, subset) with each frame's Body record
 * (read as opose_body_records_pose reads it, at the handle's current capacity; 8-byte aligned):
 * discs part by part, then the first 17 limbs limb by limb, each over the people in subset order.
 * A record whose own status is not OPOSE_OK draws nothing and hands that status on; a subset index
 * the record does not hold is OPOSE_E_ARG. */
int opose_draw_records(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                       int64_t frame_stride, const void* records, uint8_t* out, int32_t* status, int flags);
/* DisplayPose's canvas for MotionMat rows motion [N][joints][3], joints 18 or 60: the row as one
 * person (joint i absent iff its three values sum to 0), and with 60 joints the two hands of
 * rows 18..38 and 39..59: per hand 20 edges between keypoints whose x + y is not 0, then a disc at
 * every one of the 21 keypoints (a missing one draws at (0, 0), as in the reference). */
int opose_draw_motion(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                      int64_t frame_stride, const double* motion, int joints, uint8_t* out, int32_t* status,
                      int flags);

/* ---- shapelet search over motion data (srcmx/PreprocessingData.py:16-125 MotionJointFeatures,
 * srcmx/utilmx.py:330-391 SlidingDistance / matrixprofile_torch, srcmx/shapeletmodel.py:93-209
 * ShapeletMatrixModel.train) -------------------------------------------------------------------- */
/* A ragged batch: seq float32 [L][D] row-major, n_seq sequences one after another (host memory, or
 * device memory with OPOSE_IN_DEVICE); off int64 [n_seq + 1], always host memory, off[0] = 0,
 * non-decreasing, off[n_seq] = L.  For a window of m rows sequence j has P_j = len_j - m + 1
 * positions.  off, m, D and every P_j >= 1 are checked before anything is launched: OPOSE_E_SHAPE
 * for a sequence shorter than m or a limit exceeded (m <= 128, D <= 1024, n_seq <= 4096, L < 2^31),
 * OPOSE_E_ARG otherwise.  With OPOSE_OUT_DEVICE the outputs are device memory and the call is
 * asynchronous on the handle's stream.
 *
 * The distance rule, all fp32, round to nearest, no fused multiply-add:
 *   e(a, b) = sum over d = 0 .. D-1 ascending of (x[a][d] - y[b][d])^2, starting from +0
 *   s(r, c) = sum over k = 0 .. m-1 ascending of e(r + k, c + k), starting from +0
 *   dist    = sqrt(s), correctly rounded
 * and a minimum over c is the first minimum of s (strict <, c ascending).  tests/shapelet_cases.py
 * states it in NumPy; the results equal that statement bit for bit.  (The reference fills its
 * distance matrix by the recurrence sqrt(prev^2 + new - old), which drifts: not reproduced.) */

/* MotionJointFeatures: MotionMat rows motion float64 [L][joints][3], joints 18 or 60, ragged by off
 * (len_j >= 0, L >= 1) -> out float32 [L][F][2], F = 6 (18 joints) or 46.  x, y are cast to float32
 * first; the score never reaches the output.  featuremode 0, 1: a zero takes the last non-zero
 * value at or before its row within its sequence (a leading zero stays); 2: a zero takes the first
 * non-zero of rows r-1, r+1, r-2, r+2 of its sequence, from the unfilled data.  Body joints 2..7
 * relative to joint 1, each hand's joints 1..20 relative to its joint 0 (rows 18, 39); in mode 2 a
 * zero coordinate of a non-origin joint (the nose included) is the origin's first.  Modes 1, 2:
 * divided by (nose.y - neck.y) + 1e-5f of the filled body group. */
int opose_motion_features(opose_t* h, const double* motion, const int64_t* off, int n_seq, int joints,
                          int featuremode, float* out, int flags);

/* SlidingDistance of one pattern [m][D] (device memory with OPOSE_IN_DEVICE, as seq) against every
 * sequence: dist float32, ragged, P_j values per sequence (sequence j's start at off[j] - j (m - 1)). */
int opose_sliding_distance(opose_t* h, const float* pattern, int m, const float* seq, const int64_t* off,
                           int n_seq, int D, float* dist, int flags);

/* The first stage of the search.  Candidates: every start r of the sequences cand_seqs[0 ..
 * n_cand_seqs) (host memory), rows ordered by (position in cand_seqs, r): n_cand = sum of their P_i.
 * min2 float32 [n_cand][n_seq] = min over c of s(r, c) against sequence j (the squared distance),
 * loc int32 [n_cand][n_seq] its first c. */
int opose_shapelet_mindist(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int m,
                           const int32_t* cand_seqs, int n_cand_seqs, float* min2, int32_t* loc, int flags);

/* The whole search (ShapeletMatrixModel.train).  labels uint8 [n_labels] (host memory, 0 / 1, at
 * least one 1); n_seq is n_labels, or 2 * n_labels with sequence k + n_labels the mirrored copy of
 * k.  Candidates: the starts of the sequences i < n_labels with label 1, i ascending then r
 * ascending, processed in chunks of at most max_cands (0: the library's default) so the workspace
 * is bounded; the running winner stays on the device.  Per candidate, with s_k the smaller s of
 * sample k's pair (the original on a tie; unmirrored: its own):
 *   order   the samples by (bits of s_k, k) ascending
 *   num     max over t = 0 .. n_labels of negs + (positives - negatives among the first t), negs
 *           the number of zero labels; the reference's score is num / n_labels
 *   loss    the float64 sum, k ascending, of (double) sqrt(s_k) over the positive samples' own
 *           (unmirrored) values, divided by their count
 * and a candidate replaces the best only with a larger num, or an equal num and a smaller loss.
 * best int32 [4]: the winner's sequence (shapeindex), its start, its num, candidates scored;
 * best_loss float64 [1]; dis float32 [n_seq] and locs int32 [n_seq]: the winner's distances and
 * locations against every sequence.  cand_num int32 / cand_loss float64 [candidates]: every
 * candidate's num and loss, or both NULL. */
int opose_shapelet_find(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int m,
                        const uint8_t* labels, int n_labels, int max_cands, int32_t* best, double* best_loss,
                        float* dis, int32_t* locs, int32_t* cand_num, double* cand_loss, int flags);

/* Several window lengths in one pass (the m_len loop of ShapeletsFinding.train,
 * srcmx/shapeletlearning.py:123-175, which searches range(15, 40, 2) over the same clips).  e(a, b)
 * does not depend on the window length, and the sum s(r, c) runs k ascending from +0, so its partial
 * sum after m terms is the s of length m: the distances are formed once, for the longest length, and
 * every shorter length is a snapshot of the same walk.  Per length the results equal the
 * single-length call's bit for bit.
 *
 * m_lens int32 [n_lens], host memory: 1 <= n_lens <= 16, every length >= 1, strictly ascending, the
 * last <= 128, and every sequence at least the last length long.  Checked before anything is
 * launched: OPOSE_E_ARG for n_lens < 1, a length below 1 or lengths that do not ascend strictly;
 * OPOSE_E_SHAPE for n_lens > 16, a last length beyond the limit or a sequence shorter than the last
 * length; the ragged batch otherwise as above.  A start r of sequence i is a candidate of length
 * m_l when r + m_l <= len_i, and a position c of sequence j is compared at length m_l when
 * c + m_l <= len_j: no window crosses into the next sequence.
 *
 * With n_cand_l = the sum of len_i - m_l + 1 over the candidate sequences, length l's results are
 * the dense block [n_cand_l][n_seq] that opose_shapelet_mindist(m_l) writes, rows by (position in
 * cand_seqs, r), and the blocks follow one another: length l's first row is row
 * n_cand_0 + ... + n_cand_{l-1} of min2 / loc (sum of all n_cand_l rows of n_seq values each). */
int opose_shapelet_mindist_lengths(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D,
                                   const int32_t* m_lens, int n_lens, const int32_t* cand_seqs, int n_cand_seqs,
                                   float* min2, int32_t* loc, int flags);

/* opose_shapelet_find for every length of m_lens: best int32 [n_lens][4] (per length: the winner's
 * sequence, its start, its num, the candidates scored at that length), best_loss float64 [n_lens],
 * dis float32 [n_lens][n_seq], locs int32 [n_lens][n_seq]; cand_num int32 / cand_loss float64: every
 * candidate's num and loss per length, concatenated as the rows of opose_shapelet_mindist_lengths
 * are (sum of n_cand_l values), or both NULL.  Labels and candidates as in opose_shapelet_find.
 * max_cands (0: the library's default) bounds the candidates of the shortest length per chunk; the
 * workspace is n_lens times that.  Each length keeps its own winner on the device across the
 * chunks; a chunk that holds only starts too late in their clips for a length scores nothing at
 * that length.  Per length the results equal opose_shapelet_find(m_l) bit for bit, whatever the
 * chunking. */
int opose_shapelet_find_lengths(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D,
                                const int32_t* m_lens, int n_lens, const uint8_t* labels, int n_labels,
                                int max_cands, int32_t* best, double* best_loss, float* dis, int32_t* locs,
                                int32_t* cand_num, double* cand_loss, int flags);

/* Every occurrence of n_pat patterns in n_seq whole streams (DataAugmentation.AugmentateOneShapelet,
 * srcmx/DataAugmentation.py:106-150, for all patterns and videos in one call).
 *
 * pat float32 [M][D], ragged by pat_off int64 [n_pat + 1] (host memory): pattern p is rows pat_off[p]
 * .. pat_off[p + 1] - 1, m_p = 1 .. 128 of them; pat is device memory with OPOSE_IN_DEVICE, as seq.
 * sigma float32 [n_pat], host memory.  seq / off: a ragged batch as above, except that a stream may
 * have any length >= 0: position c of stream j exists for pattern p when c + m_p <= len_j, and a
 * stream shorter than the pattern, or empty, has no positions and is no error.
 *
 * The rule.  dist_p(j, c) is the distance rule above (fp32, one rounding per operation, no fused
 * multiply-add; e over d ascending from +0, s over k ascending from +0, dist = sqrt(s) correctly
 * rounded): bit for bit what opose_sliding_distance returns for that pattern and stream.  A position
 * is a hit when dist < sigma_p, a strict float32 compare on the square root; a NaN or non-positive
 * sigma gives no hits.  The occurrences of a pair (p, j) come from one walk over its hits, c
 * ascending, with the state (pre, last entry):
 *   the first hit:                                 append (c, dist), pre = c
 *   a later hit with 2 (c - pre) > m_p:            append (c, dist), pre = c
 *   else, dist < the last entry's dist (strict):   the last entry becomes (c, dist), pre = c
 *   else:                                          nothing; pre stays
 * (the reference's idex - preidx > m / 2 with true division).  pre moves on a replacement, so a run
 * of falling distances drags its entry along and a run of rising ones does not, as in the
 * reference.  tests/shapelet_scan_cases.py states the rule in NumPy.
 *
 * occ_off int64 [n_pat * n_seq + 1], pattern-major: pair (p, j)'s entries are occ_off[p * n_seq + j]
 * .. occ_off[p * n_seq + j + 1] - 1 of occ_pos int32 (the position within its stream) and occ_dist
 * float32.  occ_off is always written in full, so its last value is the total; of the entries the
 * first min(total, cap) are written.  With host outputs the call returns OPOSE_E_CAPACITY when the
 * total exceeds cap (occ_off is valid: the caller can size a retry); with OPOSE_OUT_DEVICE the call
 * is asynchronous, returns OPOSE_OK, and the caller reads the total.
 *
 * The patterns are processed in chunks of max_pats (0: the library's default) consecutive patterns,
 * which bounds the workspace (a chunk's distances are max_pats rows of L floats); the running total
 * stays on the device and the result does not depend on the chunking.  Checked before anything is
 * launched: OPOSE_E_ARG for a null handle or pointer, n_pat < 1, n_seq < 1, D < 1, max_pats < 0,
 * cap < 0, offsets that do not start at 0 or that decrease, or a pattern of 0 rows; OPOSE_E_SHAPE
 * for n_pat > 4096, n_pat * n_seq > 2^22, n_seq > 4096, D > 1024, a pattern of more than 128 rows
 * or L >= 2^31. */
int opose_shapelet_scan(opose_t* h, const float* pat, const int64_t* pat_off, int n_pat, const float* sigma,
                        const float* seq, const int64_t* off, int n_seq, int D, int max_pats,
                        int64_t* occ_off, int32_t* occ_pos, float* occ_dist, int64_t cap, int flags);

/* Learning shapelets by gradient descent (ShapeletNetModel, srcmx/shapeletmodel.py:11-90, the model of
 * ShapeletsFinding's FindShaplets_Net_ED): n_models independent models over the same clips, each a
 * query [m_k][D] and a Linear(1, 2) head, trained by Adam on the cross-entropy of the head applied
 * to the clip's smallest squared sliding distance.  tests/shapelet_net_cases.py states the rule in
 * NumPy.
 *
 * Inputs.  seq / off: a ragged batch as above; labels uint8 [n_seq], host memory, 0 / 1.
 *   t_pad = 0: clip i has the positions c = 0 .. len_i - m_k, and every len_i >= m_k.
 *   t_pad >= every len_i and every m_k: the reference's zero-padded [N][D][T = t_pad] batch without
 *     materialising it: every clip has the positions c = 0 .. t_pad - m_k, a row at or past len_i
 *     reads as +0, and len_i >= 0.
 * The queries are concatenated, float32 [q_off[n_models]][D], ragged by q_off int64 [n_models + 1]
 * (host memory), as the patterns of opose_shapelet_scan are; head float32 [n_models][4] holds
 * (w0, w1, b0, b1) of each model's Linear(1, 2).
 *
 * Forward.  s_i(c) = sum over k ascending of ( sum over d ascending of (q[k][d] - x_i[c + k][d])^2 ),
 * fp32, each sum from +0, one rounding per operation, no fused multiply-add: the direct form, not
 * the reference's QQ + XX - 2 QX, which cancels.  d_i = the first minimum of s_i over c (strict <,
 * c ascending), loc_i its c; no square root (the reference's model works on the squared distance).
 * Given the same parameter bits, d_i and loc_i equal the NumPy statement's bit for bit.
 *
 * Head, per model, in float64 from the fp32 d_i, w, b, N = n_seq:
 *   z_ij = w_j d_i + b_j;  log p_ij = z_ij - (mx + log(exp(z_i0 - mx) + exp(z_i1 - mx))), mx the
 *   larger z;  loss = -(sum over i of log p_i[y_i]) / N;  dz_ij = (p_ij - [y_i = j]) / N;
 *   g_i = dz_i0 w_0 + dz_i1 w_1;  dw_j = sum over i of dz_ij d_i;  db_j = sum over i of dz_ij
 * every sum over i ascending from +0.  correct counts the clips with argmax_j z_ij == y_i, index 0
 * on a tie (as torch.max).
 *
 * Query gradient, fp32: dq[k][d] = sum over i ascending of (float) g_i * (2 * (q[k][d] - x_i[loc_i + k][d])).
 *
 * Adam (torch.optim.Adam's defaults: betas 0.9 / 0.999, eps 1e-8, no weight decay), one step count t
 * for all parameters, fp32 state, gradients rounded to fp32:
 *   m = m + (g - m) * (float)(1 - 0.9);  v = v * 0.999f + ((float)(1 - 0.999) * g) * g
 *   p = p - (float)(lr / (1 - 0.9^t)) * (m / (sqrt(v) / (float) sqrt(1 - 0.999^t) + 1e-8f))
 * No floating-point atomics anywhere: every sum has one order and two runs give identical bits.
 *
 * The state is the caller's, in and out: query, head, and the first and second moments of both
 * (q_m, q_v shaped like query; head_m, head_v like head; zero before the first step).  step0 is the
 * number of steps the state has taken, epochs (>= 0) the steps of this call: epoch e (0-based) is a
 * forward pass, the head with its update and the query update at t = step0 + e + 1, enqueued back
 * to back with no host wait.  Because the caller owns all state, a call of a epochs followed by
 * one of b epochs with step0 = a equals one call of a + b, bit for bit.
 *
 * Outputs, from a closing forward pass with the final parameters (what the reference's Net(X, Y)
 * returns): dis float32 and locs int32 [n_models][n_seq], loss float64 [n_models], correct int32
 * [n_models]; loss_hist float64 [n_models][epochs], each epoch's loss before its update, or NULL.
 * OPOSE_IN_DEVICE: seq is device memory.  OPOSE_OUT_DEVICE: the state and the outputs are device
 * memory and the call is asynchronous on the handle's stream; otherwise all are host memory.
 *
 * Checked before anything is launched, in this order:
 *   1. OPOSE_E_ARG   a null handle or pointer (loss_hist may be null)
 *   2. OPOSE_E_ARG   lr not above 0, epochs < 0, step0 < 0
 *   3. OPOSE_E_ARG   n_seq < 1, D < 1, n_models < 1, t_pad < 0
 *   4. OPOSE_E_SHAPE n_seq > 4096, D > 1024, n_models > 16
 *   5. OPOSE_E_ARG   off does not start at 0 or decreases;  OPOSE_E_SHAPE L >= 2^31
 *   6. OPOSE_E_ARG   q_off does not start at 0, or a query of no rows;  OPOSE_E_SHAPE a query of
 *                    more than 128 rows
 *   7. OPOSE_E_ARG   a label that is not 0 or 1
 *   8. OPOSE_E_SHAPE t_pad = 0 and a clip shorter than the longest query; t_pad > 0 and below the
 *                    longest clip or the longest query
 * A refused call leaves the state and the outputs untouched. */
int opose_shapelet_net_train(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int t_pad,
                             const uint8_t* labels, const int64_t* q_off, int n_models, float* query, float* head,
                             float* q_m, float* q_v, float* head_m, float* head_v, int64_t step0, int epochs,
                             double lr, float* dis, int32_t* locs, double* loss, int32_t* correct,
                             double* loss_hist, int flags);

/* Hand on N crops uint8 [H][W][3] (util.handDetect gives squares): peaks [N][21][3]
 * (x, y, score), found [N][21] (0 = part missing, the reference's [0,0,0] row). */
int opose_hand_infer(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                     int64_t frame_stride, const opose_params* p, double* peaks,
                     int32_t* found, int flags);

/* Hand on n square crops of different sizes (the hands util.handDetect finds in a batch of
 * frames): crops[i] = uint8 [sizes[i]][sizes[i]][3] with row stride row_strides[i].  Every
 * crop maps to the same network input per scale (scale * boxsize), so the network runs once
 * per scale for all crops; resize-back and component selection run per crop.  peaks [n][21][3],
 * found [n][21]; same per-crop results as opose_hand_infer up to fp32 network noise.
 * Replaces a loop of Hand.__call__ over crops (srcmx/MotionEstimation.py:186-201). */
int opose_hand_infer_crops(opose_t* h, const uint8_t* const* crops, const int* sizes,
                           const int64_t* row_strides, int n, const opose_params* p,
                           double* peaks, int32_t* found, int flags);

/* Post-network hand path: maps[s] = [N,22,hl[s],wl[s]] per scale s (pads per scale),
 * crop H x W. */
int opose_hand_post(opose_t* h, const float* const* maps, const int* hl, const int* wl,
                    const int* pad_down, const int* pad_right, int n_scales, int N, int H, int W,
                    const opose_params* p, double* peaks, int32_t* found, int flags);

/* ---- measurement ---------------------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by HIP events on the stream it runs on and
 * accumulated per kernel class.  enable: 0 off, 1 per class, 2 per class and per layer,
 * 3 the 7x7 conv class only (the dominant kernel: bench.py's live roofline at ~1/4 of the
 * event overhead).  opose_profile_read writes one JSON object. */
int opose_profile_enable(opose_t* h, int enable);
int opose_profile_reset(opose_t* h);
int opose_profile_read(opose_t* h, char* buf, size_t len);

/* ---- test hooks (parity tests call single stages; host pointers, synchronous) ----- */
/* one stride-1 conv: x [N,Cin,H,W], w [Cout,Cin,ks,ks], b [Cout] -> out [N,Cout,H,W];
 * mt/pt <= 0 select the production tile heuristic; splits > 0 forces that many stream-K
 * workgroups (== number of tiles: plain data-parallel grid) */
int opose_debug_conv(opose_t* h, const float* x, const float* w, const float* b, int N, int Cin, int H, int W,
                     int Cout, int ks, int pad, int relu, int mt, int pt, int splits, float* out);
/* mean time (ms) of one conv launch (ngroups GEMM groups) on hashed data over `reps`
 * launches; ablate bit 1 skips the im2col gather, bit 2 the weight load (timing only) */
int opose_debug_conv_time(opose_t* h, int N, int Cin, int H, int W, int Cout, int ks, int ngroups,
                          int mt, int pt, int splits, int ablate, int reps, float* ms);
/* The split-bf16 ("x6") conv kernel on one layer: x fp32 NCHW is split into three bf16 pieces,
 * convolved with six bf16 MFMA piece products per fp32 product, written fp32 (out_x6 = 0) or
 * split and rebuilt (out_x6 = 1). */
int opose_debug_conv_x6(opose_t* h, const float* x, const float* w, const float* b, int N, int Cin, int H,
                        int W, int Cout, int ks, int pad, int relu, int mt, int pt, int splits, int out_x6,
                        float* out);
/* Layer-level hooks of the network kernels (tests/test_gpu_conv_layers.py), each through the
 * launch path the forward uses; the host splits fp32 inputs into X6 and joins X6 outputs.
 *
 * One conv launch sequence (run_conv_x6_segs) over nseg = 1 .. 8 segments of one conv shape
 * (Cin, Cout, ks, pad ks / 2).  geom [nseg][6] per segment: N, H, W, forced k slabs (0: the
 * planner's count), weight set (< nw <= 2) and the output offset (first channel of the fp32 buffer
 * or first group of the X6 buffer).  x[i] [N,Cin,H,W]; w[k] [Cout,Cin,ks,ks], b[k] [Cout].
 * family: -1 the planner's choice, else 0 conv_x6, 1 the window kernel, 2 the window kernel per
 * frame, 3 Winograd (OPOSE_E_ARG when the shape does not fit the forced family).  pool: the fused
 * 2x2 max-pool (outputs H/2 x W/2).  in_padded: the input as X6P, else dense X6.  out_kind 0: fp32
 * NCHW buffers of out_total channels; 1 / 2: dense X6 / X6P buffers of out_total groups.  dup:
 * also a duplicate destination of the output's kind (X6 kinds only).  net, lvl, pair: the layer's
 * network, resolution level and CPM-pair flag as the slab policy sees them.
 * out[i] (and out_dup[i]) [N,Cout,Ho,Wo]; ran [nseg][2]: the family the planner names for the
 * segment and the k slabs it ran with; clobbered: 16-byte units (fp32 buffers: elements) outside
 * the written pixels' slice of any output allocation that the launch changed (every allocation is
 * filled with a byte pattern first; the pad channels of the last written group do not count). */
int opose_debug_conv_segs(opose_t* h, int nseg, const int* geom, const float* const* x, int nw,
                          const float* const* w, const float* const* b, int Cin, int Cout, int ks, int relu,
                          int family, int pool, int in_padded, int out_kind, int out_total, int dup, int net,
                          int lvl, int pair, float* const* out, float* const* out_dup, int* ran,
                          int64_t* clobbered);
/* The fused closing 1x1 pair (conv1x1_chain_x6) on nseg = 1 or 2 segments of 128-channel inputs
 * (geom [nseg][4]: N, H, W, weight set < nw <= 2): out[i] [N,cout2,H,W] = W2 relu(W1 x + b1) + b2
 * (+ ReLU when relu2), W1 [m1,128] with m1 = 128 or 512, W2 [cout2,m1] with cout2 <= 64; the input
 * as X6P (in_padded) or dense X6, the output as fp32 or (out_x6) an X6P slice. */
int opose_debug_chain(opose_t* h, int nseg, const int* geom, const float* const* x, int nw,
                      const float* const* w1, const float* const* b1, const float* const* w2,
                      const float* const* b2, int m1, int cout2, int relu2, int in_padded, int out_x6,
                      float* const* out);
/* The first two layers' own kernels on nseg = 1 .. 8 segments (geom [nseg][3]: N, H, W) in one
 * launch, bias and ReLU applied as in the networks.  stage 1: conv1_1 (conv_first_x6), x[i]
 * [N,3,H,W], w [64,3,3,3] -> out[i] [N,64,H,W]; f32: the kernel's fp32-unit output form, else X6.
 * stage 2: conv1_2 + MaxPool2d(2, 2) (conv3_pool_win_x6), x[i] [N,64,H,W], w [64,64,3,3] -> out[i]
 * [N,64,H/2,W/2]; f32: the kernel's fp32-unit input form, else X6. */
int opose_debug_conv1(opose_t* h, int stage, int nseg, const int* geom, const float* const* x, const float* w,
                      const float* b, int f32, float* const* out);
int opose_debug_conv_x6_time(opose_t* h, int N, int Cin, int H, int W, int Cout, int ks, int ngroups,
                             int mt, int pt, int splits, int reps, float* ms);
/* src/body.py:38-41 for one frame and one scale: out [3,Hp,Wp]; HpWp receives (Hp, Wp)
 * (out may be NULL to query the size) */
int opose_debug_preprocess(opose_t* h, const uint8_t* bgr, int H, int W, double scale, int pad_value,
                           float* out, int* HpWp);
/* The same for n_groups <= OPOSE_MAX_SCALES groups of N[g] dense frames [N[g],H[g],W[g],3] through
 * the one-launch form opose_body_infer_groups uses (preprocess_u8_segs): out[g] [N[g],3,Hp,Wp],
 * HpWp [n_groups][2] (out, or any out[g], may be NULL to query the sizes only) */
int opose_debug_preprocess_groups(opose_t* h, int n_groups, const uint8_t* const* bgr, const int* N,
                                  const int* H, const int* W, double scale, int pad_value,
                                  float* const* out, int* HpWp);
/* src/body.py:54-57,67 for one frame: maps [57,hl,wl] -> heat_avg [18,H,W] float64 and
 * (optional) the x8-upsampled, cropped PAF maps [38,Hs,Ws] float32 */
int opose_debug_heat(opose_t* h, const float* maps, int hl, int wl, int pad_down, int pad_right, int H, int W,
                     double* heat_avg, float* paf_mid);
/* src/hand.py:62-64 on NP float64 maps [NP,H,W]: binary = gaussian_filter(map, 3) > thre, then
 * label(binary, connectivity 2) -> labels [NP,H,W] int32: -1 off the binary map, else the
 * linear index (y * W + x) of the component's first pixel in raster order -- scipy.ndimage.label's
 * numbering order -- and sums [NP,H,W] float64: at a component's first pixel, the sum of the
 * map over the component (elsewhere undefined) */
int opose_debug_hand_label(opose_t* h, const double* maps, int NP, int H, int W, double thre, int32_t* labels,
                           double* sums);
/* The fast mode's stages (srcmx/Batch_model.py), each through the launchers the product path uses.
 * srcmx/Batch_model.py:147-150 for N uint8 BGR frames (strides in bytes) at `boxsize` and the one
 * scale `scale`: out [N,3,Hp,Wp]; HpWp receives (Hp, Wp) (out may be NULL to query the size) */
int opose_debug_batch_preprocess(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                                 int64_t frame_stride, double boxsize, double scale, float* out, int* HpWp);
/* srcmx/Batch_model.py:159-168: maps [N,57,hl,wl] (PAF 0..37, heat 38..56) -> heat [N,18,H,W]
 * float32, the map the blur and the peak search read, and (optional) mid [N,56,nh,nw], the x8
 * maps cropped to nh x nw */
int opose_debug_batch_heat(opose_t* h, const float* maps, int N, int hl, int wl, int nh, int nw, int H, int W,
                           float* heat, float* mid);
/* srcmx/utilmx.py:230-263 on NP float32 maps [NP,H,W]: 5x5 blur, then peaks > thre that are >=
 * their 4 neighbours -> cnt [NP] (every peak), list [NP,cap] (y * W + x of the first cap peaks,
 * in no order; unused slots -1) and score [NP,cap] (the blurred values) */
int opose_debug_blur5_nms(opose_t* h, const float* heat, int NP, int H, int W, double thre, int cap, int32_t* cnt,
                          int32_t* list, double* score);
/* srcmx/Batch_model.py:334-346 on NP float32 maps [NP,H,W]: blurred [NP,H,W] float64 (float32
 * values), binary = blurred > thre, labels and sums as opose_debug_hand_label's (sums over the
 * blurred map) */
int opose_debug_batch_hand_label(opose_t* h, const float* heat, int NP, int H, int W, double thre, double* blurred,
                                 int32_t* labels, double* sums);
/* The body matching kernels (src/body.py:88-208, shared by Body and Batch_body), each through the
 * launcher the product path uses, at the handle's capacity (opose_set_capacity: cap peaks per part,
 * max_people rows, the record layout of opose_body_record_bytes).  Whatever a kernel indexes with
 * is checked first (OPOSE_E_ARG): counts in [0, cap], positions in [0, H * W), connection indices
 * below their part's count.
 *
 * src/body.py:88-94 (np.nonzero's row-major order, the running ids): cnt [N,18] (may pass cap: the
 * capacity status), list / score [N,18,cap] (y * W + x and the map value of the first cap peaks of
 * each part, in any order) -> the N records' header and candidate rows, peak_pos [N,18,cap] (the
 * positions in row-major order, unused slots -1) and part_cnt [N,18] (the clamped counts) */
int opose_debug_peaks_finalize(opose_t* h, const int32_t* cnt, const int32_t* list, const double* score, int N,
                               int H, int W, void* records, int32_t* peak_pos, int32_t* part_cnt);
/* src/body.py:105-141, the score of every (i, j) pair of every limb: score [N,19,cap,cap] holds
 * limb k's nA x nB scores compactly (pair (i, j) at i * nB + j of the cap * cap block), -inf where
 * criterion1 / criterion2 fail; every other entry keeps the fill, all bits set (a NaN).  The PAF
 * maps as the product path makes them, from maps[s] [N,57,hl[s],wl[s]]: fast 0: n_scales scales
 * with ga / gb = pad_down / pad_right through body_to_mid (src/body.py:52-68); fast 1: one scale
 * with ga / gb = nh / nw through the torch resize chain (srcmx/Batch_model.py:159-168) */
int opose_debug_paf_score(opose_t* h, int fast, int n_scales, const float* const* maps, const int* hl, const int* wl,
                          const int* ga, const int* gb, const int32_t* peak_pos, const int32_t* part_cnt, int N,
                          int H, int W, double thre2, double* score);
/* src/body.py:143-155, the greedy matching in stable descending score order: score as above ->
 * conn_i / conn_j [N,19,cap] int32, conn_s [N,19,cap] (unused slots -1, -1, NaN) and conn_cnt
 * [N,19] (-1: a part of the limb is empty, the reference's special_k) */
int opose_debug_limb_greedy(opose_t* h, const double* score, const int32_t* part_cnt, int N, int32_t* conn_i,
                            int32_t* conn_j, double* conn_s, int32_t* conn_cnt);
/* src/body.py:157-208, assembly and pruning: records as opose_debug_peaks_finalize leaves them
 * (status, candidate rows) -> status, n_people and subset rows, in place.  A limb's connections
 * need not be a matching (the same index may appear twice: the only way to the third-row status
 * OPOSE_E_ASSEMBLY, src/body.py:170-173).  stage receives the number of connections a frame may
 * have for the kernel to stage them all at once; beyond, it stages limb by limb */
int opose_debug_assemble(opose_t* h, void* records, const int32_t* part_cnt, const int32_t* conn_i,
                         const int32_t* conn_j, const double* conn_s, const int32_t* conn_cnt, int N, int* stage);
/* The exact mode's peak finder and heat average, one launch each (own buffers, synchronous), through
 * the launchers Body's and Hand's post paths use.
 *
 * src/body.py:70-94 on NP maps [NP,H,W], float32 (is_f32) or float64 (gauss_nms_wide):
 * gaussian_filter(map, 3), peaks > thre that are >= their 4 neighbours (zero outside the map) ->
 * cnt [NP] (every peak, may pass cap), list [NP,cap] (y * W + x of the first cap peaks, in no
 * order; unused slots -1) and score [NP,cap] (the unsmoothed map at the peak; unused slots 0) */
int opose_debug_gauss_nms(opose_t* h, const void* maps, int is_f32, int NP, int H, int W, double thre, int cap,
                          int32_t* cnt, int32_t* list, double* score);
/* The same with the single scale's cv2.resize fused in (gauss_nms_resize, src/body.py:57,70-94):
 * channels [coff, coff + P) of the x8 maps mid [N,Cm,Hs,Ws] float32 resized to H x W with source
 * steps 1 / (H / Hs), 1 / (W / Ws), then as above on the N * P float32 maps: cnt [N * P], list /
 * score [N * P,cap].  OPOSE_E_ARG without a launch for a geometry the kernel does not take (an
 * identity resize, a vertical source step above 34 / 55, or Ws above 4096) */
int opose_debug_gauss_nms_resize(opose_t* h, const float* mid, int N, int Cm, int coff, int P, int Hs, int Ws, int H,
                                 int W, double thre, int cap, int32_t* cnt, int32_t* list, double* score);
/* The same call, with what its screen launch decided: hot_tiles [tiles], tiles = N * P *
 * ceil(H / 30) * ceil(W / 102), holds in its first *hot_cnt entries the ids (np * tile rows + ty) *
 * tile columns + tx of the tiles whose sources can reach thre (in no defined order; the others -1).
 * max_grid > 0 caps the NMS launch's grid, so that few workgroups loop over many tiles (0: the
 * production grid) */
int opose_debug_gauss_hot_tiles(opose_t* h, const float* mid, int N, int Cm, int coff, int P, int Hs, int Ws, int H,
                                int W, double thre, int cap, int max_grid, int32_t* cnt, int32_t* list, double* score,
                                int32_t* hot_cnt, int32_t* hot_tiles);
/* src/body.py:51-67 / src/hand.py:43-56, the heat average of n scales: channels [coff, coff + C) of
 * mids[s] [N,Cm,Hs[s],Ws[s]] float32, each resized to H x W (copied where it has that size), divided
 * by n in float32 and added in scale order from 0.0 in float64 -> avg [N * C,H,W] float64.
 * one_launch 1: every scale in one launch (heat_full_scales), OPOSE_E_ARG without a launch where
 * that form does not take the scales (more than 8, or a resizing scale with a vertical source step
 * above 2.4375); 0: a launch per scale (n <= 16), accumulating from the second on */
int opose_debug_heat_scales(opose_t* h, int n, const float* const* mids, const int* Hs, const int* Ws, int N, int Cm,
                            int coff, int C, int H, int W, int one_launch, double* avg);
/* The hand extraction kernels (srcmx/Batch_model.py:86-102, srcmx/Batch_motion_Estimation.py:44-58),
 * each through the call opose_batch_hand_extract makes, on host arrays and synchronously.
 * (hand_boxes needs no hook: opose_batch_hand_boxes takes the poses.)
 *
 * hand_crops on N frames and their boxes [N][2][4] (as opose_batch_hand_crops, with its checks of
 * N, boxsize and the strides): both output forms -- x [2N][3][boxsize][boxsize] float32, the
 * network input v / 255 - 0.5, and crops [2N][boxsize][boxsize][3] uint8; either may be NULL, not
 * both -- and status [2N], OPOSE_E_SHAPE for a present box that is empty or leaves the frame, which
 * does not make the call fail */
int opose_debug_hand_crops(opose_t* h, const uint8_t* bgr, int N, int H, int W, int64_t row_stride,
                           int64_t frame_stride, const int32_t* boxes, int boxsize, float* x, uint8_t* crops,
                           int32_t* status);
/* hand_backmap: peaks [2N][21][3] (x, y in crop pixels, score; read only where found [2N][21] is
 * not 0) and boxes [N][2][4] -> handmat [N][42][3] */
int opose_debug_hand_backmap(opose_t* h, const double* peaks, const int32_t* found, const int32_t* boxes, int N,
                             int boxsize, double* handmat);
/* The drawing setup kernel alone (src/util.py:53-72 up to the cv2 calls: which primitives, in which
 * order, with which integer parameters): src is N Body records at the handle's capacity (joints 0)
 * or MotionMat rows [N][joints][3] (joints 18 / 60) for H x W frames -> prims [N][cap][12] int32
 * with cap = 35 * max_people, 35 or 117 slots in draw order: kind (0 nothing, 1 disc, 2 limb, 3
 * line), colour c0 | c1 << 8 | c2 << 16, centre x, y (a line's first end), a limb's a and its
 * whole degrees mod 360 (a line's second end), the covering box x0, y0, x1, y1 cut to the frame
 * (half open; empty: zeros), two zeros.  counts [N]: the frame's slots, or 0 when its status is
 * not OPOSE_OK (its slots are then undefined); slots past the count are zero.  status [N] as
 * opose_draw_records / opose_draw_motion. */
int opose_debug_draw_prims(opose_t* h, const void* src, int N, int joints, int H, int W, int32_t* prims,
                           int32_t* counts, int32_t* status);
/* Stages two and three of opose_shapelet_find on given host arrays: min2 [n_cand][n_seq] and labels
 * [n_labels] -> every row's num [n_cand] and loss [n_cand], and the selection: winner int32 [4] = 0,
 * the winning row, its num, n_cand; win_loss its loss. */
int opose_debug_shapelet_score(opose_t* h, const float* min2, int n_cand, int n_seq, const uint8_t* labels,
                               int n_labels, int32_t* num, double* loss, int32_t* winner, double* win_loss);
/* The second stage of opose_shapelet_scan alone, for one pattern of m rows, on given host arrays:
 * dist float32 [L], one value per row of the ragged batch off [n_seq + 1] (the values at a stream's
 * last m - 1 rows, where no position exists, are ignored).  The hits are dist < sigma; occ_off
 * [n_seq + 1], occ_pos, occ_dist, cap and the return value as opose_shapelet_scan with host outputs. */
int opose_debug_shapelet_pick(opose_t* h, const float* dist, const int64_t* off, int n_seq, int m, float sigma,
                              int64_t* occ_off, int32_t* occ_pos, float* occ_dist, int64_t cap);
/* One backward pass of opose_shapelet_net_train for one model, with no update, on host arrays: for
 * the query [m][D] and head [4] given, g float32 [n_seq], dq float32 [m][D], dhead float64 [4] =
 * (dw0, dw1, db0, db1) and loss float64 [1] as that call's rule states them.  The batch, t_pad and
 * labels, their checks and the order of the checks as there. */
int opose_debug_shapelet_net_grad(opose_t* h, const float* seq, const int64_t* off, int n_seq, int D, int t_pad,
                                  const uint8_t* labels, const float* query, int m, const float* head, float* g,
                                  float* dq, double* dhead, double* loss);

/* ---- TGCN sign classifier (cls/TGCN/tgcn_model.py GCN_muti_att, evaluation mode) -------------
 * Inference only: Dropout is the identity and every BatchNorm1d(V * H) uses its running statistics,
 * as cls/TGCN/test_tgcn.py runs the model.
 *
 * Shapes: V nodes (the reference hard-codes 55), F_in input and H hidden features, C classes,
 * n_stage >= 0 residual blocks, is_resi.  1 + 2 n_stage graph-convolution layers: the stem F_in -> H,
 * then two H -> H layers per block.
 *
 * params: one float32 blob, n_params values.  Per layer, stem first, then each block's gc1 / bn1 and
 * gc2 / bn2:
 *     W [F][H] | att [V][V] | bias [H] | gamma [V H] | beta [V H] | running_mean [V H] | running_var [V H]
 * (F = F_in for the stem, H after it; the batch-norm arrays in the reference's view(b, -1) order,
 * element v H + f), then fc_out.weight [C][H] | fc_out.bias [C].
 *
 * Rule, for a sample x [V][F_in]:
 *   layer(x)[v][f] = tanhf( (sum over u of att[v][u] * (sum over k of x[u][k] W[k][f])) * a[v][f] + c[v][f] )
 *   with a = gamma / sqrt(running_var + bn_eps), c = beta + (bias - running_mean) * a, both formed
 *   in float64 at create time and rounded to float32 once;
 *   y = layer_stem(x); per block: y = layer_2(layer_1(y)) (+ y when is_resi);
 *   logits[c] = (sum over f of fc_w[c][f] * m[f]) + fc_b[c],  m[f] = (sum over v of y[v][f]) / V.
 * Order of every sum the kernels fix: both matrix products run on the bf16 matrix cores with each
 * fp32 operand as three exact bf16 pieces p0 + p1 + p2 and the six piece products (0,2) (0,0) (0,1)
 * (1,0) (2,0) (1,1) (A piece, B piece; A = x, then att).  x W: k in chunks of 32 ascending, per chunk
 * the six products in that order, one matrix instruction each, all into one fp32 accumulator from
 * +0.  att (x W): x W split again, then the nodes u in two steps 0..31 and 32..63 (att reads as 0 at
 * and past V), six products each, one accumulator from +0.  Then one multiply by a, one add of c
 * (no fused multiply-add), tanhf, one add of the residual.  Head: m[f] over v ascending from +0,
 * then one division; logits over f ascending from +0 (multiply, then add), then + fc_b[c]; all fp32.
 * The result is fp32-class, not bit-equal to a float64 evaluation (tests/tgcn_cases.py holds the
 * bound); bit for bit, a sample's result does not depend on the other samples of its call, on
 * max_samples, or on the run.
 *
 * opose_tgcn_create checks, in this order, before anything is allocated: null pointers, V, F_in, H,
 * C < 1 or n_stage < 0 (OPOSE_E_ARG); V > 64, F_in or H > 1024, C > 4096, n_stage > 64
 * (OPOSE_E_SHAPE); bn_eps <= 0, n_params not the count above, a running_var + bn_eps that is not
 * positive (OPOSE_E_ARG).  Several models may live on one handle; a model is used with the handle
 * that made it and destroyed before it (opose_tgcn_destroy waits for the handle's stream). */
typedef struct opose_tgcn opose_tgcn_t;
int opose_tgcn_create(opose_t* h, int V, int F_in, int H, int C, int n_stage, int is_resi, double bn_eps,
                      const float* params, int64_t n_params, opose_tgcn_t** model);
int opose_tgcn_destroy(opose_t* h, opose_tgcn_t* model);
/* x [B][V][copies F_in] float32: copy i of batch element b is columns [i F_in, (i + 1) F_in), read in
 * place (cls/TGCN/test_tgcn.py:31-39).  The B copies samples (sample = b copies + i) run in chunks
 * of max_samples (0: as many as keep an activation buffer within 64 MB), 1 + 2 n_stage + 1 launches
 * per chunk on the handle's stream.  copy_logits [B][copies][C] (or NULL) receives every copy's
 * logits, logits [B][C] = (sum over i ascending of copy_logits[b][i][c], fp32 from +0) / copies.
 * flags: OPOSE_IN_DEVICE / OPOSE_OUT_DEVICE as for the shapelet entry points (host outputs: the
 * call returns when they are written; device outputs: asynchronous on the handle's stream).
 * Checked before any launch: null pointers, B < 1, copies < 1, max_samples < 0 (OPOSE_E_ARG);
 * copies B >= 2^24 (OPOSE_E_SHAPE). */
int opose_tgcn_forward(opose_t* h, const opose_tgcn_t* model, const float* x, int B, int copies, int max_samples,
                       float* logits, float* copy_logits, int flags);
/* One graph-convolution layer alone on host arrays, synchronously: layer 0 is the stem, 1 + 2 s and
 * 2 + 2 s the two layers of block s.  x_in [B][V][F] (F the layer's input features), residual
 * [B][V][H] or NULL (added after tanhf whatever is_resi says), out [B][V][H]. */
int opose_debug_tgcn_layer(opose_t* h, const opose_tgcn_t* model, int layer, const float* x_in, int B,
                           const float* residual, float* out);

#ifdef __cplusplus
}
#endif
#endif /* OPOSE_H */
