"""Video motion-matrix extraction (SURVEY §8 f rank 2) on the GPU Body/Hand.

Restates `Extract_MotionData_from_Video` (hitmaxiang/pytorch-openpose
srcmx/MotionEstimation.py:25-76) and the frame source `VideoDataset`
(srcmx/Batch_model.py:36-52): frames are read in order, cropped to the region of interest
`recpoint = [(x0, y0), (x1, y1)]` (frame[y0:y1, x0:x1]), run through the Body (+Hand)
pipeline, and stacked into MotionMat [frames, 18 or 60, 3] (x, y, score per joint: 18 body
joints, then 21 left-hand and 21 right-hand joints in "bodyhand" mode), saved with
joblib.dump like the reference.

Frames are processed in batches (one Body launch sequence per batch, all hands of a batch in
one crop-batched Hand pass) instead of one frame at a time; per-frame results are those of
`src.pipeline.motion_data_every_frame`.  Any iterable of uint8 BGR frames works as a source;
`VideoFrames` reads a video file through OpenCV when it is installed (it is not part of this
image: decode elsewhere and pass the frames, or pass any cv2.VideoCapture-like `capture`).

Like the reference, the matrix has one row per frame the container *reports*
(CAP_PROP_FRAME_COUNT, srcmx/MotionEstimation.py:45-50): rows of frames that never decode stay
zero, a video that decodes more frames than it reports raises IndexError, and a video that does
not open is reported and yields None (`Extract_MotionData_from_Video`, the reference's entry
point, :25-76).

Ingest (the reference's DataLoader over decoded frames, srcmx/Batch_model.py:36-52, 409-412, into
the per-video loop of srcmx/MotionEstimation.py:61-76): with a GPU, `extract_motion_data` streams
the batches through two pinned host buffers and two device frame buffers.  While batch k runs
Body on the GPU (Body.infer_records, pipelined with batch k-1's post-processing), batch k+1 is
cropped into the other pinned buffer and uploaded on its own copy stream, and batch k-1's
records (downloaded asynchronously to pinned memory) are decoded into poses on the host, its
hands running through Hand on the Hand handle's stream.  The poses are those of the host path
(`device=False`: Body.batch per batch), bit for bit.
"""
from __future__ import annotations

import numpy as np



CAP_PROP_FRAME_COUNT = 7  # cv2.CAP_PROP_FRAME_COUNT


class VideoFrames(object):
    """Sequential BGR frames of a video file, optionally cropped (VideoDataset semantics).

    capture: a cv2.VideoCapture-like factory (isOpened / get(CAP_PROP_FRAME_COUNT) / read);
    default cv2.VideoCapture.  len() is the count the container reports; `opened` is False for a
    file that does not open (then it has no frames)."""

    def __init__(self, videopath, crop=None, capture=None):
        if capture is None:
            try:
                import cv2
            except ImportError as e:  # pragma: no cover - cv2 is absent in this image
                raise ImportError("VideoFrames needs OpenCV (cv2) to decode video; pass decoded frames "
                                  "to extract_motion_data instead, or a capture factory") from e
            capture = cv2.VideoCapture
        self.video = capture(videopath)
        self.opened = bool(self.video.isOpened())
        self.crop = crop

    def __len__(self):
        return int(self.video.get(CAP_PROP_FRAME_COUNT)) if self.opened else 0

    def __iter__(self):
        while self.opened:
            ok, image = self.video.read()
            if not ok:
                return
            if self.crop is not None:
                image = image[self.crop[0][1]:self.crop[1][1], self.crop[0][0]:self.crop[1][0], :]
            yield image


def crop_roi(frame, recpoint):
    """frame[y0:y1, x0:x1] for recpoint [(x0, y0), (x1, y1)] (MotionEstimation.py:66)."""
    if recpoint is None:
        return frame
    return frame[recpoint[0][1]:recpoint[1][1], recpoint[0][0]:recpoint[1][0], :]


def _batches(frames, recpoint, batch):
    buf = []
    for frame in frames:
        buf.append(crop_roi(np.asarray(frame), recpoint))
        if len(buf) == batch:
            yield buf
            buf = []
    if buf:
        yield buf


def _host_poses(frames, body, hand, recpoint, mode, batch):
    from .pipeline import poses_from_results
    out = []
    for b in _batches(frames, recpoint, batch):
        arr = np.stack([np.ascontiguousarray(f) for f in b])
        out.append(poses_from_results(body.batch(arr), arr, hand, mode))
    return out


class _DeviceIngest(object):
    """Two pinned host frame buffers -> two device frame buffers (one copy stream each) ->
    Body.infer_records(pipeline=True) -> records downloaded to pinned host memory on the
    handle's stream; at most two batches in flight.

    A frame whose peaks or people overflow the record capacity (the reference has no limit) is
    run again through Body.batch, which grows the capacity and retries like Body(); later
    batches then get records of the grown size (a batch decodes with the layout it was
    submitted with)."""

    def __init__(self, body, batch, H, W):
        import torch
        self.torch = torch
        self.body = body
        self.batch = batch
        self.devc = torch.device("cuda", body.handle.device)
        self.host = [torch.empty((batch, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = [torch.empty((batch, H, W, 3), dtype=torch.uint8, device=self.devc) for _ in range(2)]
        self.rdev, self.rhost, self.layout = [None, None], [None, None], [None, None]
        self.cps = [torch.cuda.Stream(device=self.devc) for _ in range(2)]
        self.up_done = [None, None]    # upload of buffer i finished with host[i]
        self.rec_done = [None, None]   # records of buffer i on the host
        self.lib = body.handle.torch_stream()

    def submit(self, i, frames):
        torch = self.torch
        n = len(frames)
        if self.up_done[i] is not None:
            self.up_done[i].synchronize()  # host[i] free: its previous upload completed
        rb = self.body.handle.record_bytes()
        if self.rdev[i] is None or self.rdev[i].shape[1] != rb:  # (first use, or the capacity grew)
            self.rdev[i] = torch.empty((self.batch, rb), dtype=torch.uint8, device=self.devc)
            self.rhost[i] = torch.empty((self.batch, rb), dtype=torch.uint8).pin_memory()
        self.layout[i] = (self.body.peaks_per_part, self.body.max_people)
        np.stack(frames, out=self.host[i][:n].numpy())
        cp = self.cps[i]
        cp.wait_stream(self.lib)  # the call that last read dev[i] / wrote rdev[i] is done with them
        with torch.cuda.stream(cp):
            self.dev[i][:n].copy_(self.host[i][:n], non_blocking=True)
            self.up_done[i] = torch.cuda.Event()
            self.up_done[i].record(cp)
            # the library orders itself after this stream (opose_wait_stream): the upload above
            self.body.infer_records(self.dev[i][:n], self.rdev[i][:n], pipeline=True)
        with torch.cuda.stream(self.lib):
            self.rhost[i][:n].copy_(self.rdev[i][:n], non_blocking=True)
            self.rec_done[i] = torch.cuda.Event()
            self.rec_done[i].record(self.lib)

    def results(self, i, frames):
        from . import _native
        self.rec_done[i].synchronize()
        out = []
        for r, f in zip(self.rhost[i][:len(frames)].numpy(), frames):
            status, cand, subset = _native.decode_record(r, *self.layout[i])
            if status == _native.OPOSE_E_CAPACITY:
                out.extend(self.body.batch(np.ascontiguousarray(f)[None]))
            else:
                _native.raise_record_status(status, *self.layout[i])
                out.append((cand, subset))
        return out


def _device_poses(frames, body, hand, recpoint, mode, batch):
    from .pipeline import poses_from_results
    out, ing, pending, k = [], None, None, 0
    for b in _batches(frames, recpoint, batch):
        if ing is None:
            H, W = b[0].shape[:2]
            ing = _DeviceIngest(body, batch, H, W)
        if any(f.shape != b[0].shape for f in b) or b[0].shape[:2] != tuple(ing.host[0].shape[1:3]):
            raise ValueError("frames must have equal sizes after cropping")
        i = k % 2
        ing.submit(i, b)
        if pending is not None:  # the previous batch's poses while this one runs on the GPU
            pi, pframes = pending
            out.append(poses_from_results(ing.results(pi, pframes), pframes, hand, mode))
        pending = (i, b)
        k += 1
    if pending is not None:
        pi, pframes = pending
        out.append(poses_from_results(ing.results(pi, pframes), pframes, hand, mode))
    return out


def extract_motion_data(frames, body, hand=None, outpath=None, recpoint=None, mode="body", batch=32, device=None,
                        count=None):
    """MotionMat [count, 18 | 60, 3] float64 for an iterable of uint8 BGR frames (equal sizes
    after cropping).  mode "body" (18 joints) or "bodyhand" (needs `hand`); saved with
    joblib.dump when `outpath` is given, like Extract_MotionData_from_Video.  device=None: the
    pinned, double-buffered GPU ingest when torch sees a GPU, else host batches (Body.batch).

    count: rows of the matrix, the frame count the source reports (default len(frames) when it
    has one -- a VideoFrames' CAP_PROP_FRAME_COUNT -- else the frames decoded).  Frames past the
    decoded ones stay zero rows; more decoded frames than `count` raise IndexError, as the
    reference's preallocated MotionMat does (srcmx/MotionEstimation.py:45-50, 72-73)."""
    if mode not in ("body", "bodyhand"):
        raise ValueError("mode must be 'body' or 'bodyhand'")
    if mode == "bodyhand" and hand is None:
        raise ValueError("'bodyhand' mode needs a Hand")
    if device is None:
        try:
            import torch
            device = torch.cuda.is_available()
        except ImportError:
            device = False
    if count is None and hasattr(frames, "__len__"):
        count = len(frames)
    out = (_device_poses if device else _host_poses)(frames, body, hand, recpoint, mode, batch)
    joints = 60 if mode == "bodyhand" else 18
    poses = np.concatenate(out) if out else np.zeros((0, joints, 3))
    if count is None:
        count = len(poses)
    if len(poses) > count:
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (count, count))
    motion = np.zeros((count, joints, 3))
    motion[:len(poses)] = poses
    if outpath is not None:
        import joblib
        joblib.dump(motion, outpath)
    return motion


def Batch_hand_extraction(videopath, motiondata, recpoints, outpath, *, hand, batch=32, capture=None):
    """The reference's fast-mode hand pass (srcmx/Batch_motion_Estimation.py:19-65) on the GPU:
    the video's frames and the body MotionMat [T, 18, 3] of a first pass -> HandMat [T, 42, 3]
    (left hand rows 0..20, right 21..41), written to `outpath` with joblib.dump.  Returns None,
    like the reference.  AssertionError unless the container reports len(motiondata) frames
    (HandImageDataset, srcmx/Batch_model.py:63-64).  hand: a src.batch_model.Batch_hand (the
    reference's module-level batch_hand_estimation); each batch of frames is one Batch_hand.extract
    at the reference's boxsize 368, the region of interest recpoints [(x0, y0), (x1, y1)] applied
    as an offset into the whole frames.  capture: see VideoFrames."""
    import itertools
    boxsize = 368
    video = VideoFrames(videopath, capture=capture)
    FrameCounts = len(video)
    assert FrameCounts == len(motiondata)
    motiondata = np.asarray(motiondata, dtype=np.float64)
    COUNTS = len(motiondata)
    HandMat = np.zeros((COUNTS, 42, 3))
    count = 0
    for frames in _batches(itertools.islice(video, COUNTS), None, batch):
        n = len(frames)
        HandMat[count:count + n] = hand.extract(np.stack(frames), motiondata[count:count + n], boxsize, recpoints)
        for c in range(count + 1, count + n + 1):
            if c % 1000 == 0:
                print('%s-%d/%d' % (outpath, c, COUNTS))
        count += n
    if count < COUNTS:  # the reference slices the None a failed read returns (srcmx/Batch_model.py:70-71)
        raise TypeError("'NoneType' object is not subscriptable")
    import joblib
    joblib.dump(HandMat, outpath)
    print('the %s file is saved' % outpath)
    return None


def _fast_mode_pass(videopath, outpath, batch_size, capture, joints, rows_of):
    """What the reference's fast-mode body pass does around its model call
    (srcmx/Batch_motion_Estimation.py:68-113): a file that does not open is reported and yields
    None; one row of `joints` keypoints per frame the container reports, filled batch by batch
    with rows_of(frames [n, H, W, 3]) -> [n, joints, 3]; its progress prints, joblib.dump, its
    closing print.  Frames past the reported count are not read (the reference's DataLoader goes
    by len()); a container that reports more frames than decode ends as the reference's data
    loader does, slicing the None a failed read returns (srcmx/Batch_model.py:47-49)."""
    import itertools
    import os
    video = VideoFrames(videopath, capture=capture)
    if not video.opened:
        print('the file %s is not exist' % videopath)
        return None
    COUNTS = len(video)
    outname = os.path.split(outpath)[1]
    MotionMat = np.zeros((COUNTS, joints, 3))
    count = 0
    for frames in _batches(itertools.islice(video, COUNTS), None, batch_size):
        n = len(frames)
        MotionMat[count:count + n] = rows_of(np.stack(frames))
        for c in range(count + 1, count + n + 1):
            if c % 1000 == 0:
                print('%s-%d/%d' % (outname, c, COUNTS))
        count += n
    if count < COUNTS:
        raise TypeError("'NoneType' object is not subscriptable")
    import joblib
    joblib.dump(MotionMat, outpath)
    print('the %s file is saved' % outpath)
    return None


def Batch_body_extraction(videopath, outpath, batch_size, recpoint, *, body, capture=None):
    """The reference's fast-mode body pass (srcmx/Batch_motion_Estimation.py:68-113) on the GPU:
    the video's frames cut to recpoint [(x0, y0), (x1, y1)] -> MotionMat [T, 18, 3] (T = the
    container's frame count; per frame the person with the largest left-shoulder x), written to
    `outpath` with joblib.dump.  Returns None, like the reference; a video that does not open is
    reported on stdout and nothing is written.  body: a src.batch_model.Batch_body (the reference's
    module-level Batch_Body_model); each batch of frames is one Batch_body.extract, the region of
    interest applied as an offset into the whole frames.  capture: see VideoFrames."""
    return _fast_mode_pass(videopath, outpath, batch_size, capture, 18, lambda frames: body.extract(frames, recpoint))


def Batch_motion_extraction(videopath, outpath, batch_size, recpoint, *, body, hand, capture=None, render=None):
    """Both fast-mode passes of the reference (Batch_body_extraction, then Batch_hand_extraction
    on its poses, srcmx/Batch_motion_Estimation.py:19-113) in one pass over the video: MotionMat
    [T, 60, 3], body rows 0-17, left hand 18-38, right hand 39-59, written like
    Batch_body_extraction's.  Per batch the frames are uploaded once, Batch_body.extract_device's
    poses feed Batch_hand.extract_device (boxsize 368) on the device, and the [n, 60, 3] rows and
    the statuses come back in one download each; the two handles are ordered through torch's
    current stream.  A batch in which a frame overflows the body record capacity runs again
    through Batch_body.extract, which grows the capacity; other statuses raise what
    Batch_body.extract / Batch_hand.extract raise.

    render: an optional callable that receives each batch's canvases, the frames cut to recpoint
    with their rows drawn over them (Body.draw_motion; what the reference shows frame by frame with
    DisplayPose) as a CUDA uint8 tensor [n, H, W, 3]: drawn on the device from the [n, 60, 3]
    tensor the hand pass just produced, before anything is downloaded.  None: nothing changes."""
    import torch
    from . import _native
    from .batch_model import _frames_view
    devc = torch.device("cuda", body.handle.device)

    def rows_of(frames):
        dev = torch.from_numpy(frames).to(devc)
        pose, bstat = body.extract_device(dev, recpoint)
        handmat, hstat = hand.extract_device(dev, pose, 368, recpoint)
        rows_dev = torch.cat([pose, handmat], 1)
        if render is not None:
            view = _frames_view(dev, recpoint)[0]  # the region of interest as a strided view
            canvases, dstat = body.draw_motion_status(view, rows_dev)
        rows = rows_dev.cpu().numpy()
        bstat, hstat = bstat.cpu().numpy(), hstat.cpu().numpy()
        if (bstat == _native.OPOSE_E_CAPACITY).any():
            pose = body.extract(dev, recpoint)
            rows = np.concatenate([pose, hand.extract(dev, pose, 368, recpoint)], 1)
            if render is not None:
                render(body.draw_motion(view, torch.from_numpy(rows).to(devc)))
            return rows
        for s in bstat:
            _native.raise_record_status(int(s), body.peaks_per_part, body.max_people)
        hand.raise_status(hstat)
        if render is not None:
            body.raise_draw_status(dstat)
            render(canvases)
        return rows

    return _fast_mode_pass(videopath, outpath, batch_size, capture, 60, rows_of)


def Checkout_motion_data(frames, motion, recpoint=None, batch=32, *, body):
    """The reference's check of an extraction run (Checkout_motion_data / DisplayPose,
    srcmx/MotionEstimation.py:219-304) without its window: a generator of rendered uint8 batches
    [n, H, W, 3], frame k cut to recpoint [(x0, y0), (x1, y1)] with row k of the MotionMat motion
    [T, 18 | 60, 3] drawn over it (Body.draw_motion: body, and with 60 joints the hands), `batch`
    frames at a time, in order, until the frames run out.  The reference shows each with
    cv2.imshow; show, write or compare what this yields.  frames: any iterable of uint8 BGR frames
    (a VideoFrames); when it reports a length other than T, the reference's line is printed.  More
    frames than rows raise IndexError, as PoseMat[index] does there."""
    motion = np.asarray(motion, dtype=np.float64)
    if hasattr(frames, "__len__") and len(frames) != motion.shape[0]:
        print('the count number is not equal')
    index = 0
    for b in _batches(frames, recpoint, batch):
        n = len(b)
        if index + n > len(motion):
            raise IndexError("index %d is out of bounds for axis 0 with size %d" % (len(motion), len(motion)))
        yield body.draw_motion(np.stack([np.ascontiguousarray(f) for f in b]), motion[index:index + n])
        index += n


def Extract_MotionData_from_Video(videopath, outpath, Recpoint, mode="body", overwrite=False, *, body, hand=None,
                                  batch=32, device=None, capture=None):
    """The reference's entry point (srcmx/MotionEstimation.py:25-76) on the GPU Body / Hand:
    the video's frames cropped to Recpoint [(x0, y0), (x1, y1)], MotionMat [count, 18 | 60, 3]
    (count = CAP_PROP_FRAME_COUNT; frames that do not decode leave zero rows) written to
    `outpath` with joblib.dump.  Returns None, like the reference (the matrix is the file); a
    video that does not open is reported on stdout and nothing is written.  `overwrite` is
    unused, as in the reference.  body / hand: the estimators (the reference's module-level
    body_estimation / hand_estimation); capture: see VideoFrames."""
    import os
    del overwrite
    video = VideoFrames(videopath, crop=Recpoint, capture=capture)
    if not video.opened:
        print('the file %s is not exist' % videopath)
        return None
    count = len(video)
    outname = os.path.split(outpath)[1]

    def progress():
        for index, frame in enumerate(video):
            if index % 100 == 0:
                print('%s-%d/%d' % (outname, index, count))
            yield frame

    extract_motion_data(progress(), body, hand, outpath=outpath, mode=mode, batch=batch, device=device, count=count)
    print('%s is saved!' % outpath)
    return None
