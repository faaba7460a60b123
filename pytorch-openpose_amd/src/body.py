"""Body pose estimation with the reference's call surface (hitmaxiang/pytorch-openpose src/body.py).

    body = Body('body_pose_model.pth')
    candidate, subset = body(oriImg)          # oriImg: uint8 H x W x 3, BGR

Returns exactly what `Body.__call__` (src/body.py:24-212) returns:
* candidate: float64 [N, 4] rows (x, y, score, id), or shape (0,) when no peak exists;
* subset:    float64 [P, 20]: candidate ids per part (-1 = missing), total score, part count.

Everything after weight loading runs on the GPU in libopose: uint8 cubic resize + pad +
normalise, the VGG-19/CPM network (implicit-GEMM fp32 MFMA), x8 cubic upsample, resize
and scale averaging, Gaussian(sigma=3) peak NMS, PAF line integrals, greedy matching and
person assembly.  Only the fixed-size per-frame record crosses PCIe.

Extras beyond the reference (defaults = reference values, src/body.py:25-31):
scale_search, boxsize, stride, padValue, thre1, thre2, device; `Body.batch(frames)` runs
a video batch through one launch sequence; `Body.batch_mixed(frames)` / `Body.batch_groups`
run frames of different sizes in one lockstep pass; `Body.infer_records` (and
`Body.infer_records_groups`) keep inputs/outputs on the device (multi-GPU gather, benchmark).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native
from ._native import lib
from .model import bodypose_model, load_model


def _as_batch(frames):
    """[H, W, 3] -> [1, H, W, 3] (numpy array or torch tensor; anything else through numpy)."""
    if not hasattr(frames, "data_ptr"):
        frames = np.asarray(frames)
    return frames[None] if frames.ndim == 3 else frames


class Body(object):
    def __init__(self, model_path, device: int = 0, scale_search=(0.5,), boxsize=368, stride=8, padValue=128,
                 thre1=0.1, thre2=0.05, peaks_per_part=128, max_people=96):
        self.model = load_model(bodypose_model, model_path, device)
        self.handle = self.model.handle
        self.params = _native.default_params(_native.NET_BODY, scale_search=scale_search, boxsize=float(boxsize),
                                             stride=int(stride), pad_value=int(padValue), thre1=float(thre1),
                                             thre2=float(thre2))
        self.peaks_per_part, self.max_people = peaks_per_part, max_people
        self.handle.set_capacity(peaks_per_part, max_people)

    # ------------------------------------------------------------------ host API
    def __call__(self, oriImg):
        return self.batch(oriImg[None])[0]

    def batch(self, frames):
        """frames: uint8 [N, H, W, 3] (or a list of equally sized frames) -> list of (candidate, subset)."""
        if isinstance(frames, (list, tuple)):
            frames = np.stack(frames)
        frames, ptr, N, H, W, rs, fs, _ = _native.frames_view(np.asarray(frames))
        return self._records(N, lambda rec: lib.opose_body_infer(self.handle.h, ptr, N, H, W, rs, fs, self.params,
                                                                 rec, 0))

    def groups_per_pass(self):
        """Groups one opose_body_infer_groups call takes: every (group, scale) pair is a segment."""
        return max(1, _native.MAX_SCALES // self.params.n_scales)

    def batch_groups(self, groups):
        """groups: a list of uint8 arrays [N_g, H_g, W_g, 3] (or lists of equally sized frames), every
        group with its own size -> a list, one entry per group, of lists of (candidate, subset).

        The groups' networks run in one lockstep pass (opose_body_infer_groups), groups_per_pass()
        groups per call; a group's results are Body.batch(group)'s."""
        views = [_native.frames_view(np.stack(g) if isinstance(g, (list, tuple)) else np.asarray(g)) for g in groups]
        per, out = self.groups_per_pass(), []
        for i in range(0, len(views), per):
            out += self._records_groups(views[i:i + per])
        return out

    def batch_mixed(self, frames):
        """frames: a list of uint8 [H, W, 3] frames of any sizes -> list of (candidate, subset) in the
        frames' order.  Frames of one size form a group of batch_groups, the groups in the order
        their sizes first appear."""
        where = {}  # (H, W) -> indices into frames
        for i, f in enumerate(frames):
            where.setdefault(tuple(np.shape(f)[:2]), []).append(i)
        results = self.batch_groups([[frames[i] for i in idx] for idx in where.values()])
        out = [None] * len(frames)
        for idx, res in zip(where.values(), results):
            for i, r in zip(idx, res):
                out[i] = r
        return out

    def post(self, maps, pad, H, W):
        """Post-network path only (src/body.py:52-212) on one scale.

        maps: float32 [N, 57, h, w] (PAF channels 0..37, heat 38..56); pad: util.padRightDownCorner pad."""
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        N, c, hl, wl = maps.shape
        assert c == 57
        return self._records(N, lambda rec: lib.opose_body_post(self.handle.h, maps.ctypes.data, N, hl, wl,
                                                                int(pad[2]), int(pad[3]), int(H), int(W),
                                                                self.params, rec, 0))

    # ------------------------------------------------------------------ per-scale split
    def scale_geom(self, H, W):
        """[(hl, wl, pad_down, pad_right)] per scale of scale_search for an H x W frame."""
        out = []
        for s in range(self.params.n_scales):
            g = (ctypes.c_int * 4)()
            self.handle.check(lib.opose_body_scale_geom(int(H), int(W), self.params, s, g))
            out.append(tuple(int(v) for v in g))
        return out

    def scale_maps(self, frames, s, out=None):
        """Network maps of scale index `s` only: [N, 57, hl, wl] float32 (PAF 38 | heat 19).

        frames: uint8 [N,H,W,3] numpy (-> numpy) or a torch cuda tensor (-> torch cuda tensor,
        written into `out` when given, complete in torch's current-stream order)."""
        frames, ptr, N, H, W, rs, fs, dev = _native.frames_view(_as_batch(frames))
        hl, wl, _, _ = self.scale_geom(H, W)[s]
        if dev:
            import torch
            if out is None:
                out = torch.empty((N, 57, hl, wl), dtype=torch.float32, device=frames.device)
            assert out.is_contiguous() and tuple(out.shape) == (N, 57, hl, wl)
            # `out` complete in torch's stream order (e.g. an isend)
            self.handle.torch_call(lib.opose_body_scale_maps, ptr, N, H, W, rs, fs, self.params, s, out.data_ptr(),
                                   _native.DEVICE_IO)
            return out
        maps = np.empty((N, 57, hl, wl), np.float32)
        self.handle.check(lib.opose_body_scale_maps(self.handle.h, ptr, N, H, W, rs, fs, self.params, s,
                                                    maps.ctypes.data, 0))
        return maps

    def band_maps(self, frame, s, r0, r1, exchange=None):
        """Rows [r0, r1) of scale `s`'s network maps for one frame: [1, 57, r1-r0, wl] float32
        (opose_body_band_maps; src/body.py:36-50 for one m, cut into output rows).

        frame: uint8 [H,W,3] numpy (-> numpy) or torch cuda tensor (-> torch cuda tensor in
        torch's current-stream order).  exchange(xbuf, cap, nbytes, stream) moves the halo rows
        between neighbouring bands (src.dist.band_exchange): xbuf is the uint8 device tensor
        [send_up | send_dn | recv_up | recv_dn] of `cap` bytes each, `stream` the library's
        hipStream_t, on which the send halves are being packed.  Not needed when one band covers
        every row.  exchange="rccl": the library's own RCCL send/recv on its stream, with the
        communicator and neighbours of src.dist.init_band_comm / Handle.set_band_peers (no Python
        between the layers).  The bands of a frame put together are scale_maps(frame, s) bit for
        bit: every conv sums a pixel in the whole frame's order."""
        import torch
        frame, ptr, _, H, W, rs, _, dev = _native.frames_view(_as_batch(frame)[:1])
        hl, wl, _, _ = self.scale_geom(H, W)[s]
        cap = int(lib.opose_body_band_halo_bytes(wl))
        xbuf = getattr(self, "_band_xbuf", None)  # kept across calls (27 exchanges per call)
        if xbuf is None or xbuf.numel() < 4 * cap:
            xbuf = self._band_xbuf = torch.empty(4 * cap, dtype=torch.uint8,
                                                 device=torch.device("cuda", self.handle.device))
        err = []

        def _cb(user, nbytes, stream):
            try:
                if exchange is None:
                    raise RuntimeError("row band with neighbours but no exchange")
                exchange(xbuf[:4 * cap], cap, int(nbytes), stream)
                return 0
            except BaseException as e:  # reported after the call returns
                err.append(e)
                return 1

        cb = _native.HALO_FN() if exchange == "rccl" else _native.HALO_FN(_cb)  # NULL: the library's RCCL
        if dev:
            out = torch.empty((1, 57, r1 - r0, wl), dtype=torch.float32, device=frame.device)
        else:
            out = np.empty((1, 57, r1 - r0, wl), np.float32)
        # not Handle.torch_call: a callback's own exception goes before the library's status, only a
        # device call that succeeded signals, and a numpy call waits only (xbuf was allocated on
        # torch's stream) and never signals
        self.handle.wait_torch()
        rc = lib.opose_body_band_maps(self.handle.h, ptr, H, W, rs, self.params, s, r0, r1, _native._ptr(out), cb,
                                      None, xbuf.data_ptr(), 4 * cap, _native.DEVICE_IO if dev else 0)
        if err:
            raise err[0]
        self.handle.check(rc)
        if dev:
            self.handle.signal_torch()
        return out

    def post_scales(self, maps, H, W):
        """Multi-scale post-network path (src/body.py:51-212): maps[s] = [N,57,hl,wl] for every
        scale of scale_search (numpy, or torch cuda tensors) -> list of (candidate, subset)."""
        geoms = self.scale_geom(H, W)
        if len(maps) != len(geoms):
            raise ValueError("expected %d scale maps, got %d" % (len(geoms), len(maps)))
        dev = hasattr(maps[0], "data_ptr")
        if not dev:
            maps = [np.ascontiguousarray(m, dtype=np.float32) for m in maps]
        for m, (hl, wl, _, _) in zip(maps, geoms):
            if tuple(m.shape[1:]) != (57, hl, wl):
                raise ValueError("scale maps of shape %s, expected (N, 57, %d, %d)" % (tuple(m.shape), hl, wl))
        N = maps[0].shape[0]
        ns = len(maps)
        ptrs = (ctypes.c_void_p * ns)(*[m.data_ptr() if dev else m.ctypes.data for m in maps])
        if dev:
            self.handle.wait_torch()  # e.g. maps received by an irecv on torch's stream
        arr = [(ctypes.c_int * ns)(*[g[i] for g in geoms]) for i in range(4)]
        return self._records(N, lambda rec: lib.opose_body_post_scales(
            self.handle.h, ptrs, arr[0], arr[1], arr[2], arr[3], ns, N, int(H), int(W), self.params, rec,
            _native.IN_DEVICE if dev else 0))

    # ------------------------------------------------------------------ device API
    def infer_records(self, frames_dev, records_dev=None, pipeline=False, wait=True):
        """frames_dev: torch.uint8 cuda [N,H,W,3]; returns a torch.uint8 cuda [N, record_bytes] tensor.

        Asynchronous (no host synchronisation): ordered after torch's current stream, and the
        records are complete in that stream's order on return (opose_wait_stream /
        opose_signal_stream).  pipeline=True
        (OPOSE_PIPELINE, include/opose.h): the frames are complete now and are not modified until
        the handle's stream passes this call; the call's network then overlaps the previous
        call's post-processing (video-batch throughput).  pipeline="defer"
        (OPOSE_PIPELINE_DEFER): this call's post-processing is enqueued by the next pipelined
        call once that call's network reaches conv3_1, or by handle.flush() / synchronize() /
        decode_records(); keep frames and records alive until then.
        wait=False (pipelined calls only): do not order the call after torch's current stream.
        The caller guarantees that the frames are complete and that the records buffer is free
        (e.g. it synchronized the host on the upload's event): opose_wait_stream would put a
        marker on the caller's stream, and a stream that shares a hardware queue with the
        handle's post-processing stream then holds the next network back behind that work."""
        import torch
        frames_dev, ptr, N, H, W, row_stride, frame_stride, _ = _native.frames_view(frames_dev)
        if records_dev is None:
            records_dev = torch.empty((N, self.handle.record_bytes()), dtype=torch.uint8, device=frames_dev.device)
        if wait or not pipeline:
            self.handle.wait_torch()  # frames / records produced or last used on torch's stream
        self.handle.check(lib.opose_body_infer(self.handle.h, ptr, N, H, W, row_stride, frame_stride, self.params,
                                               records_dev.data_ptr(),
                                               _native.DEVICE_IO | (_native.PIPELINE if pipeline else 0)
                                               | (_native.PIPELINE_DEFER if pipeline == "defer" else 0)))
        if pipeline:
            # outputs stay in the handle's stream order (torch's stream must not wait for them, or
            # the next call's network could not overlap this call's post-processing): consumers
            # order themselves on handle.stream() (bench.py, src/dist.py) or call decode_records
            self.handle.hold(records_dev, frames_dev)
        else:
            self.handle.signal_torch()
        return records_dev

    def infer_records_groups(self, frames_dev_list, records_dev_list=None):
        """batch_groups on the device: frames_dev_list[g] torch.uint8 cuda [N_g, H_g, W_g, 3]; returns a
        list of torch.uint8 cuda [N_g, record_bytes] tensors (records_dev_list when given).

        Asynchronous, ordered after torch's current stream, and the records are complete in that
        stream's order on return, as infer_records (not pipelined).  groups_per_pass() groups per
        opose_body_infer_groups call."""
        import torch
        views = [_native.frames_view(f) for f in frames_dev_list]
        if records_dev_list is None:
            rb = self.handle.record_bytes()
            records_dev_list = [torch.empty((v[2], rb), dtype=torch.uint8, device=v[0].device) for v in views]
        if len(records_dev_list) != len(views):
            raise ValueError("expected one records tensor per group")
        per = self.groups_per_pass()
        for i in range(0, len(views), per):
            n, ptrs, N, H, W, rs, fs = _native.groups_args(views[i:i + per])
            recs = (ctypes.c_void_p * n)(*[r.data_ptr() for r in records_dev_list[i:i + per]])
            self.handle.torch_call(lib.opose_body_infer_groups, n, ptrs, N, H, W, rs, fs, self.params, recs,
                                   _native.DEVICE_IO)
        return records_dev_list

    def decode_records(self, records):
        """uint8 [N, record_bytes] (numpy or torch) -> list of (candidate, subset)."""
        if hasattr(records, "cpu"):
            if records.is_cuda:
                self.handle.signal_torch()  # pipelined records complete on the handle's stream
            records = records.cpu().numpy()
        return [self._decode(r) for r in np.asarray(records)]

    def poses(self, records):
        """uint8 [N, record_bytes] records of the handle's current capacity -> (pose float64
        [N, 18, 3], status int32 [N]): per frame the keypoints of the person with the largest
        left-shoulder x, the row `Batch_body_extraction` keeps (srcmx/Batch_motion_Estimation.py:
        88-107; src.pipeline.selected_pose on the decoded record), chosen and gathered on the
        device (opose_body_records_pose).  status: 0, the record's own status (zero row), or
        OPOSE_E_ARG for a record that indexes past its candidates (zero row).  numpy records give
        numpy results; a torch CUDA tensor gives CUDA tensors with no synchronisation, complete in
        torch's current-stream order."""
        rb = self.handle.record_bytes()
        if hasattr(records, "data_ptr") and records.is_cuda:
            import torch
            if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] != rb or len(records) < 1:
                raise ValueError("expected uint8 records [N, %d]" % rb)
            records = records.contiguous()
            N = len(records)
            pose = torch.empty((N, 18, 3), dtype=torch.float64, device=records.device)
            status = torch.empty((N,), dtype=torch.int32, device=records.device)
            self.handle.torch_call(lib.opose_body_records_pose, records.data_ptr(), N, pose.data_ptr(),
                                   status.data_ptr(), _native.DEVICE_IO)
            return pose, status
        if hasattr(records, "cpu"):
            records = records.cpu().numpy()
        records = np.ascontiguousarray(records)
        if records.dtype != np.uint8 or records.ndim != 2 or records.shape[1] != rb or len(records) < 1:
            raise ValueError("expected uint8 records [N, %d]" % rb)
        N = len(records)
        pose, status = np.zeros((N, 18, 3), np.float64), np.zeros((N,), np.int32)
        rc = lib.opose_body_records_pose(self.handle.h, records.ctypes.data, N, pose.ctypes.data, status.ctypes.data, 0)
        self._check_worst(rc, status)
        return pose, status

    # ------------------------------------------------------------------ drawing
    def draw_records_status(self, frames, records, out=None):
        """util.draw_bodypose (src/util.py:44-77) of every frame's Body record, on the device
        (opose_draw_records): frames uint8 [N, H, W, 3] (or one [H, W, 3]; a strided region of
        interest is taken as it is) and records uint8 [N, record_bytes] at the handle's current
        capacity -> (canvases, status int32 [N]).  out=None: new dense canvases; `out is frames`:
        drawn in place; else a dense uint8 [N, H, W, 3] buffer.  numpy in gives numpy out; torch
        CUDA frames and records give CUDA tensors with no synchronisation, complete in torch's
        current-stream order.  A frame whose status is not 0 (its record's own status, or
        OPOSE_E_ARG for an index past the candidates or a coordinate outside +-16384) is left as it
        was.  The covered pixels follow the rule include/opose.h states, which util.draw_bodypose's
        host rasteriser shares for the discs only."""
        rb = self.handle.record_bytes()
        dev = hasattr(records, "data_ptr") and records.is_cuda
        if not dev:
            records = np.ascontiguousarray(records.cpu().numpy() if hasattr(records, "cpu") else records)
        else:
            records = records.contiguous()
        if str(records.dtype).split(".")[-1] != "uint8" or records.ndim != 2 or records.shape[1] != rb:
            raise ValueError("expected uint8 records [N, %d]" % rb)
        return self._draw(lib.opose_draw_records, frames, records, (), out)

    def draw_motion_status(self, frames, motion, out=None):
        """DisplayPose's canvas (srcmx/MotionEstimation.py:281-295) for MotionMat rows motion
        [N, 18 | 60, 3] float64 over frames [N, H, W, 3], on the device (opose_draw_motion): the
        row as one person through draw_bodypose, then with 60 joints both hands as
        utilmx.draw_handpose_by_opencv draws them -> (canvases, status int32 [N]).  frames, out,
        memory spaces and status as draw_records_status."""
        dev = hasattr(motion, "data_ptr") and motion.is_cuda
        if not dev:
            motion = np.ascontiguousarray(motion.cpu().numpy() if hasattr(motion, "cpu") else motion, dtype=np.float64)
        else:
            motion = motion.contiguous()
        if str(motion.dtype).split(".")[-1] != "float64" or motion.ndim != 3 or motion.shape[1] not in (18, 60) \
                or motion.shape[2] != 3:
            raise ValueError("expected float64 MotionMat rows [N, 18 | 60, 3]")
        return self._draw(lib.opose_draw_motion, frames, motion, (int(motion.shape[1]),), out)

    def draw_records(self, frames, records, out=None):
        """draw_records_status's canvases; a frame's non-zero status raises what Body() raises for
        it (reading the status of CUDA inputs waits for the call)."""
        canvas, status = self.draw_records_status(frames, records, out)
        self.raise_draw_status(status)
        return canvas

    def draw_motion(self, frames, motion, out=None):
        """draw_motion_status's canvases; a frame's non-zero status raises (see draw_records)."""
        canvas, status = self.draw_motion_status(frames, motion, out)
        self.raise_draw_status(status)
        return canvas

    def raise_draw_status(self, status):
        """The per-frame status [N] of a draw call as draw_records / draw_motion raise it (nothing
        when all 0)."""
        if hasattr(status, "cpu"):
            status = status.cpu().numpy()
        for s in status[status != 0]:
            _native.raise_record_status(int(s), self.peaks_per_part, self.max_people)

    def _draw(self, fn, frames, src, extra, out):
        """fn(handle, frames..., src, *extra, out, status, flags) for frames / src / out in one
        memory space -> (canvases shaped like frames, status)."""
        batch = _as_batch(frames)
        v, ptr, N, H, W, rs, fs, dev = _native.frames_view(batch)
        if dev != bool(hasattr(src, "data_ptr") and src.is_cuda):
            raise ValueError("frames and what is drawn must both be numpy arrays or both CUDA tensors")
        if len(src) != N:
            raise ValueError("expected one record or MotionMat row per frame: %d" % N)
        if out is None:
            if dev:
                import torch
                canvas = torch.empty((N, H, W, 3), dtype=torch.uint8, device=v.device)
            else:
                canvas = np.empty((N, H, W, 3), np.uint8)
            optr = _native._ptr(canvas)
        else:
            canvas = _as_batch(out)
            ov, optr, oN, oH, oW, ors, ofs, odev = _native.frames_view(canvas)
            if (oN, oH, oW, odev) != (N, H, W, dev) or optr != _native._ptr(canvas):
                raise ValueError("out must be uint8 [%d, %d, %d, 3] in the frames' memory space" % (N, H, W))
            if optr == ptr and _native._ptr(batch) == ptr:
                if (ors, ofs) != (rs, fs):
                    raise ValueError("out overlaps the frames without being the frames")
            elif (ors, ofs) != (3 * W, 3 * W * H):
                raise ValueError("out must be dense, or the frames themselves to draw in place")
        if dev:
            import torch
            status = torch.empty((N,), dtype=torch.int32, device=v.device)
            self.handle.torch_call(fn, ptr, N, H, W, rs, fs, src.data_ptr(), *extra, optr, status.data_ptr(),
                                   _native.DEVICE_IO)
        else:
            status = np.zeros((N,), np.int32)
            rc = fn(self.handle.h, ptr, N, H, W, rs, fs, src.ctypes.data, *extra, optr, status.ctypes.data, 0)
            self._check_worst(rc, status)
        single = batch is not frames and getattr(frames, "ndim", 4) == 3
        return (canvas[0] if single and out is None else (out if out is not None else canvas)), status

    # ------------------------------------------------------------------ helpers
    def _check_worst(self, rc, status):
        """rc of a call that returns its worst per-frame status, `status` zeroed before the call: a
        code no frame carries is the call's own failure."""
        if rc != _native.OPOSE_OK and rc != int(status.min()):
            self.handle.check(rc)

    def _grow(self) -> bool:
        if self.peaks_per_part >= 1024 and self.max_people >= 256:
            return False
        self.peaks_per_part = min(1024, self.peaks_per_part * 2)
        self.max_people = min(256, self.max_people * 2)
        self.handle.set_capacity(self.peaks_per_part, self.max_people)
        return True

    def _records(self, N, call):
        """call(rec_ptr) -> rc fills N host records: run it, with the capacity doubled and the call
        repeated while a frame overflows its record, and decode -> list of (candidate, subset)."""
        while True:
            rec = np.empty((N, self.handle.record_bytes()), np.uint8)
            rc = call(rec.ctypes.data)
            if rc == _native.OPOSE_E_CAPACITY and self._grow():
                continue
            if rc not in (_native.OPOSE_OK, _native.OPOSE_E_CAPACITY, _native.OPOSE_E_ASSEMBLY):
                self.handle.check(rc)  # the two let through are per-frame statuses: _decode raises them
            return [self._decode(r) for r in rec]

    def _records_groups(self, views):
        """One opose_body_infer_groups call on the groups `views` (frames_view results) into host
        records, repeated as _records repeats its call -> per group a list of (candidate, subset)."""
        n, ptrs, N, H, W, rs, fs = _native.groups_args(views)
        while True:
            recs = [np.empty((v[2], self.handle.record_bytes()), np.uint8) for v in views]
            rc = lib.opose_body_infer_groups(self.handle.h, n, ptrs, N, H, W, rs, fs, self.params,
                                             (ctypes.c_void_p * n)(*[r.ctypes.data for r in recs]), 0)
            if rc == _native.OPOSE_E_CAPACITY and self._grow():
                continue
            if rc not in (_native.OPOSE_OK, _native.OPOSE_E_CAPACITY, _native.OPOSE_E_ASSEMBLY):
                self.handle.check(rc)
            return [[self._decode(r) for r in rec] for rec in recs]

    def _decode(self, rec):
        status, cand, subset = _native.decode_record(rec, self.peaks_per_part, self.max_people)
        _native.raise_record_status(status, self.peaks_per_part, self.max_people)
        return cand, subset
