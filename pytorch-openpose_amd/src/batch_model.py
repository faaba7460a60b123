"""The reference's batched "fast mode" (hitmaxiang/pytorch-openpose srcmx/Batch_model.py),
on the GPU.

    bb = Batch_body('body_pose_model.pth')
    results = bb(batch_images)       # [(candidate, subset), ...], one per frame

`Batch_body.__call__` (srcmx/Batch_model.py:137-204) differs from `Body` in numerics, not in
its person model: torch bicubic resizing of ToTensor'd frames (uint8 / 255), floor instead of
round image sizes, a single scale (0.5), a 5x5 Gaussian (srcmx/utilmx.py:246-263) instead of
scipy's sigma-3 filter, and peak scores read from the blurred map; limb scoring, greedy
matching and assembly are Body's (`FindBody_frame`, :206-300).  Here the whole call is one
libopose launch sequence (`opose_batch_body_infer`): torch-convention bicubic kernels,
the same conv network, a blur+NMS kernel, then the shared PAF / matching / assembly kernels.

Inputs: what the reference's DataLoader yields -- a float tensor [B, 3, h, w] in [0, 1]
(transforms.ToTensor of uint8 BGR frames; converted back to the exact uint8 values) -- or
uint8 frames [B, h, w, 3] directly.
"""
from __future__ import annotations

import numpy as np

from . import _native
from ._native import lib
from .body import Body
from .hand import _as_reference_array, hand_boxes, hand_outputs, pose_rows
from .model import handpose_model, load_model


def size_pad(g_scale, height, width, boxsize=368, stride=8):
    """Batch_body.calculate_size_pad (srcmx/Batch_model.py:302-307)."""
    scale = boxsize * g_scale / height
    h, w = int(height * scale), int(width * scale)
    return scale, h, w, (stride - (h % stride)) % stride, (stride - (w % stride)) % stride


def _as_uint8_frames(batch_images) -> np.ndarray:
    if hasattr(batch_images, "detach"):  # torch tensor [B, 3, h, w] float in [0, 1]
        t = batch_images.detach()
        if t.dtype.is_floating_point:
            t = (t * 255).round().clamp(0, 255).to(dtype=__import__("torch").uint8)
        return np.ascontiguousarray(t.permute(0, 2, 3, 1).cpu().numpy())
    a = np.asarray(batch_images)
    if a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3:
        return a
    if a.ndim == 4 and a.shape[1] == 3:
        return np.ascontiguousarray(np.clip(np.rint(a * 255), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
    raise ValueError("expected a [B,3,h,w] float batch in [0,1] or uint8 frames [B,h,w,3]")


def _frames_view(frames, recpoint):
    """_native.frames_view of frames [N, H, W, 3] uint8 (numpy, or a torch CUDA tensor) cut to
    recpoint [(x0, y0), (x1, y1)]: the region of interest is a pointer offset, not a copy."""
    if not hasattr(frames, "data_ptr"):
        frames = np.asarray(frames)
    if recpoint is not None and frames.ndim == 4:
        frames = frames[:, recpoint[0][1]:recpoint[1][1], recpoint[0][0]:recpoint[1][0], :]
    return _native.frames_view(frames)


class Batch_body(Body):
    def __init__(self, model_path, device: int = 0, scale_search=0.5, boxsize=368, stride=8, thre1=0.1, thre2=0.05,
                 peaks_per_part=128, max_people=96):
        super().__init__(model_path, device, scale_search=(float(scale_search),), boxsize=boxsize, stride=stride,
                         padValue=128, thre1=thre1, thre2=thre2, peaks_per_part=peaks_per_part,
                         max_people=max_people)
        self.scale_search, self.boxsize, self.stride = float(scale_search), boxsize, stride

    def __call__(self, batch_images):
        return self.batch(_as_uint8_frames(batch_images))

    def batch(self, frames):
        frames, ptr, N, H, W, rs, fs, _ = _native.frames_view(np.asarray(frames))
        return self._records(N, lambda rec: lib.opose_batch_body_infer(self.handle.h, ptr, N, H, W, rs, fs,
                                                                       self.params, rec, 0))

    def post(self, maps, H, W):
        """Post-network part only (srcmx/Batch_model.py:159-204): maps float32 [N, 57, hl, wl]
        (PAF 0..37, heat 38..56) for frames of H x W."""
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        N, c, hl, wl = maps.shape
        assert c == 57
        _, nh, nw, _, _ = size_pad(self.scale_search, H, W, self.boxsize, self.stride)
        return self._records(N, lambda rec: lib.opose_batch_body_post(self.handle.h, maps.ctypes.data, N, hl, wl, nh,
                                                                      nw, int(H), int(W), self.params, rec, 0))

    def infer_records(self, frames_dev, records_dev=None):
        """Device-resident uint8 frames [N, H, W, 3] -> device records (asynchronous)."""
        import torch
        frames_dev, ptr, N, H, W, rs, fs, _ = _native.frames_view(frames_dev)
        if records_dev is None:
            records_dev = torch.empty((N, self.handle.record_bytes()), dtype=torch.uint8, device=frames_dev.device)
        self.handle.torch_call(lib.opose_batch_body_infer, ptr, N, H, W, rs, fs, self.params, records_dev.data_ptr(),
                               _native.DEVICE_IO)
        return records_dev

    # ---- body extraction: the loop body of Batch_body_extraction
    # (srcmx/Batch_motion_Estimation.py:83-108) on the device
    def extract_device(self, frames_dev, recpoint=None):
        """Torch CUDA uint8 frames [N, H, W, 3] cut to recpoint [(x0, y0), (x1, y1)] (a pointer
        offset) -> (PoseMat rows float64 [N, 18, 3], status int32 [N]) as CUDA tensors, in one
        launch sequence (opose_batch_body_extract): the records stay in the library, the person
        with the largest left-shoulder x is chosen there (Body.poses).  Asynchronous: ordered after
        torch's current stream and complete in its order; no host round trip and no retry -- a
        frame that overflows the record capacity has status OPOSE_E_CAPACITY and a zero row."""
        import torch
        v, ptr, N, H, W, rs, fs, dev = _frames_view(frames_dev, recpoint)
        if not dev:
            raise ValueError("extract_device needs frames on the device")
        pose = torch.empty((N, 18, 3), dtype=torch.float64, device=v.device)
        status = torch.empty((N,), dtype=torch.int32, device=v.device)
        self.handle.torch_call(lib.opose_batch_body_extract, ptr, N, H, W, rs, fs, self.params, pose.data_ptr(),
                               status.data_ptr(), _native.DEVICE_IO)
        return pose, status

    def extract(self, frames, recpoint=None):
        """N frames (numpy [N, H, W, 3] uint8, or a torch CUDA uint8 tensor) cut to recpoint ->
        the rows of MotionMat Batch_body_extraction stores for them, float64 [N, 18, 3]:
        src.pipeline.selected_pose of every frame's (candidate, subset), without the records
        leaving the device.  Like Body(), a frame that overflows the record capacity doubles it and
        repeats the call; other per-frame statuses raise what Body() raises."""
        v, ptr, N, H, W, rs, fs, dev = _frames_view(frames, recpoint)
        while True:
            if dev:
                pose, status = (t.cpu().numpy() for t in self.extract_device(v))
            else:
                pose, status = np.zeros((N, 18, 3), np.float64), np.zeros((N,), np.int32)
                rc = lib.opose_batch_body_extract(self.handle.h, ptr, N, H, W, rs, fs, self.params, pose.ctypes.data,
                                                  status.ctypes.data, 0)
                self._check_worst(rc, status)
            if (status == _native.OPOSE_E_CAPACITY).any() and self._grow():
                continue
            for s in status:
                _native.raise_record_status(int(s), self.peaks_per_part, self.max_people)
            return pose


class Batch_hand(object):
    """srcmx/Batch_model.py:310-354: crops already resized to boxsize (the data loader's
    HandImageDataset does that with cv2) -> np.array [B, 21, 3] of (x, y, score) in crop
    pixels, float64 (int64 when nothing is found anywhere, as np.array of [0, 0, 0] rows).

    The stage that feeds it in the reference (the data loader's boxes, flips and cv2 resizes) and
    the back-mapping that follows it run on the device too: `boxes`, `crops`, `extract`."""

    def __init__(self, model_path, device: int = 0, thre=0.035):
        self.model = load_model(handpose_model, model_path, device)
        self.handle = self.model.handle
        self.params = _native.default_params(_native.NET_HAND, scale_search=(1.0,), thre_hand=float(thre))

    def __call__(self, batch_imgs):
        crops, ptr, N, H, W, rs, fs, _ = _native.frames_view(_as_uint8_frames(batch_imgs))
        peaks, found = hand_outputs(N)
        self.handle.check(lib.opose_batch_hand_infer(self.handle.h, ptr, N, H, W, rs, fs, self.params,
                                                     peaks.ctypes.data, found.ctypes.data, 0))
        return _as_reference_array(peaks, found)

    def post(self, heat):
        """Post-network part only (srcmx/Batch_model.py:334-354): heat float32 [B, 22, hl, wl]."""
        heat = np.ascontiguousarray(heat, dtype=np.float32)
        N, c, hl, wl = heat.shape
        assert c == 22
        peaks, found = hand_outputs(N)
        self.handle.check(lib.opose_batch_hand_post(self.handle.h, heat.ctypes.data, N, hl, wl, self.params,
                                                    peaks.ctypes.data, found.ctypes.data, 0))
        return _as_reference_array(peaks, found)

    # ---- hand extraction: HandImageDataset (srcmx/Batch_model.py:55-104) and the loop body of
    # Batch_hand_extraction (srcmx/Batch_motion_Estimation.py:29-60) on the device
    _frames_view = staticmethod(_frames_view)

    _motion = staticmethod(pose_rows)

    def boxes(self, motion, hw):
        """HandImageDataset's utilmx.handDetect call (srcmx/Batch_model.py:74-84) for N poses
        motion [N, 18, 3] in frames of hw = (H, W): int32 [N, 2, 4] = {x, y, w, present}, left
        then right; an absent side is zeros."""
        return hand_boxes(self.handle, motion, hw)

    @staticmethod
    def _raise_empty(bad):
        n, side = (int(i) for i in np.argwhere(bad)[0])
        raise ValueError("frame %d: the %s hand's box is empty (cv2.resize of an empty crop in the reference)"
                         % (n, ("left", "right")[side]))

    def crops(self, frames, motion, boxsize=368, recpoint=None):
        """The crops HandImageDataset cuts (srcmx/Batch_model.py:86-99): uint8
        [N, 2, boxsize, boxsize, 3], left (mirrored) then right, gray 128 where a hand is absent."""
        v, ptr, N, H, W, rs, fs, dev = self._frames_view(frames, recpoint)
        boxes = self.boxes(motion, (H, W))
        out = np.empty((N, 2, int(boxsize), int(boxsize), 3), np.uint8)
        boxes_in = boxes
        if dev:
            import torch
            boxes_in = torch.from_numpy(boxes).to(v.device)
            self.handle.wait_torch()
        rc = lib.opose_batch_hand_crops(self.handle.h, ptr, N, H, W, rs, fs, _native._ptr(boxes_in), int(boxsize),
                                        out.ctypes.data, _native.IN_DEVICE if dev else 0)
        if dev:  # not Handle.torch_call: torch may reuse v and boxes_in whatever rc says, read below
            self.handle.signal_torch()
        if rc == _native.OPOSE_E_SHAPE and ((boxes[:, :, 3] != 0) & (boxes[:, :, 2] < 1)).any():
            self._raise_empty((boxes[:, :, 3] != 0) & (boxes[:, :, 2] < 1))
        self.handle.check(rc)
        return out

    def extract_device(self, frames_dev, motion_dev, boxsize=368, recpoint=None):
        """extract_status() with everything on the device: torch CUDA uint8 frames [N, H, W, 3] and
        torch CUDA float64 poses [N, 18, 3] (e.g. Batch_body.extract_device's) -> (HandMat rows
        float64 [N, 42, 3], status int32 [N, 2]) as CUDA tensors.  Asynchronous: ordered after
        torch's current stream and complete in its order, no host round trip."""
        import torch
        v, ptr, N, H, W, rs, fs, dev = self._frames_view(frames_dev, recpoint)
        if not dev:
            raise ValueError("extract_device needs frames on the device")
        if not (hasattr(motion_dev, "is_cuda") and motion_dev.is_cuda and motion_dev.dtype == torch.float64
                and tuple(motion_dev.shape) == (N, 18, 3)):
            raise ValueError("expected one body pose [18, 3] per frame: a CUDA float64 motion [%d, 18, 3]" % N)
        m = motion_dev.contiguous()
        handmat = torch.empty((N, 42, 3), dtype=torch.float64, device=v.device)
        status = torch.empty((N, 2), dtype=torch.int32, device=v.device)
        self.handle.torch_call(lib.opose_batch_hand_extract, ptr, N, H, W, rs, fs, m.data_ptr(), int(boxsize),
                               self.params, handmat.data_ptr(), status.data_ptr(), _native.DEVICE_IO)
        return handmat, status

    def extract_status(self, frames, motion, boxsize=368, recpoint=None):
        """extract() without its check: (HandMat rows float64 [N, 42, 3], status int32 [N, 2]), a
        slot's status OPOSE_E_SHAPE where a present hand's box is empty.  With frames on the device,
        motion may be a torch CUDA float64 tensor too: it is then used where it is."""
        v, ptr, N, H, W, rs, fs, dev = self._frames_view(frames, recpoint)
        if dev:
            import torch
            if not (hasattr(motion, "is_cuda") and motion.is_cuda):
                motion = torch.from_numpy(self._motion(motion, N)).to(v.device)
            handmat, status = self.extract_device(v, motion, boxsize)
            return handmat.cpu().numpy(), status.cpu().numpy()
        motion = self._motion(motion, N)
        handmat = np.empty((N, 42, 3), np.float64)
        status = np.empty((N, 2), np.int32)
        rc = lib.opose_batch_hand_extract(self.handle.h, ptr, N, H, W, rs, fs, motion.ctypes.data, int(boxsize),
                                          self.params, handmat.ctypes.data, status.ctypes.data, 0)
        if rc != _native.OPOSE_E_SHAPE:
            self.handle.check(rc)
        return handmat, status

    def extract(self, frames, motion, boxsize=368, recpoint=None):
        """N frames (numpy [N, H, W, 3] uint8, or a torch CUDA uint8 tensor) and their body poses
        motion [N, 18, 3] -> HandMat rows float64 [N, 42, 3]: rows 0..20 the left hand, 21..41 the
        right, (x, y) in the pixels of the frame cut to recpoint [(x0, y0), (x1, y1)], score.  One
        launch sequence on the device: boxes, crops, the hand network, Batch_hand's
        post-processing, the back-mapping of Batch_hand_extraction's loop."""
        handmat, status = self.extract_status(frames, motion, boxsize, recpoint)
        self.raise_status(status)
        return handmat

    @classmethod
    def raise_status(cls, status):
        """The per-slot status [N, 2] of an extraction as extract() raises it (nothing when all 0)."""
        if (status == _native.OPOSE_E_SHAPE).any():
            cls._raise_empty(status == _native.OPOSE_E_SHAPE)
        if (status != 0).any():
            raise _native.OposeError(int(status.min()), "hand extraction failed")
