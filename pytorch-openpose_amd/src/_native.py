"""ctypes binding of libopose.so (the C ABI declared in include/opose.h).

This is the only way the package computes anything: there is no CPU fallback.  If the
shared library is missing or fails to load, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OPOSE_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libopose.so"))

OPOSE_OK = 0
OPOSE_E_ARG, OPOSE_E_SHAPE, OPOSE_E_HIP, OPOSE_E_WEIGHTS, OPOSE_E_CAPACITY, OPOSE_E_ASSEMBLY = -1, -2, -3, -4, -5, -6
OPOSE_E_TIMEOUT = -7
NET_BODY, NET_HAND = 0, 1
IN_DEVICE, OUT_DEVICE, PIPELINE, PIPELINE_DEFER = 1, 2, 4, 8
DEVICE_IO = IN_DEVICE | OUT_DEVICE
MAX_SCALES = 8


class Params(C.Structure):
    _fields_ = [("n_scales", C.c_int), ("scales", C.c_double * MAX_SCALES), ("boxsize", C.c_double),
                ("stride", C.c_int), ("pad_value", C.c_int), ("thre1", C.c_double), ("thre2", C.c_double),
                ("thre_hand", C.c_double)]


# int (*opose_halo_fn)(void* user, size_t bytes, void* stream)
HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)


_P, _I, _L, _D, _S = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t
# name -> (restype, argtypes) of every symbol include/opose.h declares
SIGNATURES = {
    "opose_default_params": (None, [_I, C.POINTER(Params)]),
    "opose_create": (_I, [_I, C.POINTER(_P)]),
    "opose_destroy": (None, [_P]),
    "opose_last_error": (C.c_char_p, [_P]),
    "opose_set_stream": (_I, [_P, _P]),
    "opose_wait_stream": (_I, [_P, _P]),
    "opose_signal_stream": (_I, [_P, _P]),
    "opose_signal_input": (_I, [_P, _P]),
    "opose_get_stream": (_P, [_P]),
    "opose_synchronize": (_I, [_P]),
    "opose_flush": (_I, [_P]),
    "opose_set_capacity": (_I, [_P, _I, _I]),
    "opose_body_record_bytes": (_S, [_P]),
    "opose_load_weights": (_I, [_P, _I, C.POINTER(_P), _P, _I]),
    "opose_body_forward": (_I, [_P, _P, _I, _I, _I, _P, _P, _I]),
    "opose_hand_forward": (_I, [_P, _P, _I, _I, _I, _P, _I]),
    "opose_hand_forward_pyramid": (_I, [_P, _I, C.POINTER(_P), _P, _P, _P, C.POINTER(_P), _I]),
    "opose_body_infer": (_I, [_P, _P, _I, _I, _I, _L, _L, C.POINTER(Params), _P, _I]),
    "opose_body_infer_groups": (_I, [_P, _I, C.POINTER(_P), _P, _P, _P, _P, _P, C.POINTER(Params), C.POINTER(_P), _I]),
    "opose_body_post": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(Params), _P, _I]),
    "opose_body_scale_geom": (_I, [_I, _I, C.POINTER(Params), _I, _P]),
    "opose_body_scale_maps": (_I, [_P, _P, _I, _I, _I, _L, _L, C.POINTER(Params), _I, _P, _I]),
    "opose_body_post_scales": (_I, [_P, C.POINTER(_P), _P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(Params), _P, _I]),
    "opose_body_band_halo_bytes": (_S, [_I]),
    "opose_rccl_unique_id": (_I, [_P, _S]),
    "opose_rccl_init": (_I, [_P, _P, _I, _I]),
    "opose_rccl_abort": (_I, [_P]),
    "opose_rccl_wait": (_I, [_P, _I]),
    "opose_set_band_peers": (_I, [_P, _I, _I]),
    "opose_body_band_maps": (_I, [_P, _P, _I, _I, _L, C.POINTER(Params), _I, _I, _I, _P, HALO_FN, _P, _P, _S, _I]),
    "opose_hand_infer": (_I, [_P, _P, _I, _I, _I, _L, _L, C.POINTER(Params), _P, _P, _I]),
    "opose_hand_post": (_I, [_P, C.POINTER(_P), _P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(Params), _P, _P, _I]),
    "opose_hand_infer_crops": (_I, [_P, C.POINTER(_P), _P, _P, _I, C.POINTER(Params), _P, _P, _I]),
    "opose_batch_body_infer": (_I, [_P, _P, _I, _I, _I, _L, _L, C.POINTER(Params), _P, _I]),
    "opose_batch_body_post": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(Params), _P, _I]),
    "opose_batch_hand_infer": (_I, [_P, _P, _I, _I, _I, _L, _L, C.POINTER(Params), _P, _P, _I]),
    "opose_batch_hand_post": (_I, [_P, _P, _I, _I, _I, C.POINTER(Params), _P, _P, _I]),
    "opose_batch_hand_boxes": (_I, [_P, _P, _I, _I, _I, _P, _I]),
    "opose_batch_hand_crops": (_I, [_P, _P, _I, _I, _I, _L, _L, _P, _I, _P, _I]),
    "opose_batch_hand_extract": (_I, [_P, _P, _I, _I, _I, _L, _L, _P, _I, C.POINTER(Params), _P, _P, _I]),
    "opose_body_records_pose": (_I, [_P, _P, _I, _P, _P, _I]),
    "opose_batch_body_extract": (_I, [_P, _P, _I, _I, _I, _L, _L, C.POINTER(Params), _P, _P, _I]),
    "opose_profile_enable": (_I, [_P, _I]),
    "opose_profile_reset": (_I, [_P]),
    "opose_profile_read": (_I, [_P, C.c_char_p, _S]),
    "opose_debug_conv": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "opose_debug_preprocess": (_I, [_P, _P, _I, _I, _D, _I, _P, _P]),
    "opose_debug_preprocess_groups": (_I, [_P, _I, C.POINTER(_P), _P, _P, _P, _D, _I, C.POINTER(_P), _P]),
    "opose_debug_conv_time": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "opose_debug_conv_x6": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "opose_debug_conv_segs": (_I, [_P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P,
                                   _P]),
    "opose_debug_chain": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "opose_debug_conv1": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "opose_debug_conv_x6_time": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "opose_debug_heat": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "opose_debug_hand_label": (_I, [_P, _P, _I, _I, _I, _D, _P, _P]),
    "opose_debug_batch_preprocess": (_I, [_P, _P, _I, _I, _I, _L, _L, _D, _D, _P, _P]),
    "opose_debug_batch_heat": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "opose_debug_blur5_nms": (_I, [_P, _P, _I, _I, _I, _D, _I, _P, _P, _P]),
    "opose_debug_batch_hand_label": (_I, [_P, _P, _I, _I, _I, _D, _P, _P, _P]),
    "opose_debug_peaks_finalize": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "opose_debug_paf_score": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _D, _P]),
    "opose_debug_limb_greedy": (_I, [_P, _P, _P, _I, _P, _P, _P, _P]),
    "opose_debug_assemble": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "opose_debug_gauss_nms": (_I, [_P, _P, _I, _I, _I, _I, _D, _I, _P, _P, _P]),
    "opose_debug_gauss_nms_resize": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _D, _I, _P, _P, _P]),
    "opose_debug_gauss_hot_tiles": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _D, _I, _I, _P, _P, _P, _P, _P]),
    "opose_debug_heat_scales": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "opose_debug_hand_crops": (_I, [_P, _P, _I, _I, _I, _L, _L, _P, _I, _P, _P, _P]),
    "opose_debug_hand_backmap": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "opose_draw_records": (_I, [_P, _P, _I, _I, _I, _L, _L, _P, _P, _P, _I]),
    "opose_draw_motion": (_I, [_P, _P, _I, _I, _I, _L, _L, _P, _I, _P, _P, _I]),
    "opose_debug_draw_prims": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "opose_motion_features": (_I, [_P, _P, _P, _I, _I, _I, _P, _I]),
    "opose_sliding_distance": (_I, [_P, _P, _I, _P, _P, _I, _I, _P, _I]),
    "opose_shapelet_mindist": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _I]),
    "opose_shapelet_find": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I]),
    "opose_shapelet_mindist_lengths": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, _I, _P, _P, _I]),
    "opose_shapelet_find_lengths": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I]),
    "opose_debug_shapelet_score": (_I, [_P, _P, _I, _I, _P, _I, _P, _P, _P, _P]),
    "opose_shapelet_scan": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _L, _I]),
    "opose_debug_shapelet_pick": (_I, [_P, _P, _P, _I, _I, C.c_float, _P, _P, _P, _L]),
    "opose_shapelet_net_train": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _L, _I, _D, _P, _P, _P,
                                      _P, _P, _I]),
    "opose_debug_shapelet_net_grad": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P]),
    "opose_tgcn_create": (_I, [_P, _I, _I, _I, _I, _I, _I, _D, _P, _L, C.POINTER(_P)]),
    "opose_tgcn_destroy": (_I, [_P, _P]),
    "opose_tgcn_forward": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I]),
    "opose_debug_tgcn_layer": (_I, [_P, _P, _I, _P, _I, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libopose.so not found at {LIB_PATH}: build it with `make -C pytorch-openpose_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if "OPOSE_LIB" in os.environ and not hasattr(lib, name):
            continue  # an older build picked for a same-box A/B may predate later entry points
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class OposeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libopose error {code}: {msg}")
        self.code = code


def default_params(net: int, **kw) -> Params:
    p = Params()
    lib.opose_default_params(net, C.byref(p))
    if "scale_search" in kw and kw["scale_search"] is not None:
        ss = list(kw.pop("scale_search"))
        if not 1 <= len(ss) <= MAX_SCALES:
            raise ValueError("scale_search must have 1..8 entries")
        p.n_scales = len(ss)
        for i, s in enumerate(ss):
            p.scales[i] = float(s)
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def _ptr(a) -> int:
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a.data_ptr())  # torch tensor


def frames_view(frames, what="frames"):
    """uint8 [N, H, W, 3] frames (a numpy array or a torch tensor; what="crops": Hand's crops) as
    every frame entry point of the library takes them:
    (view, ptr, N, H, W, row_stride, frame_stride, on_device), strides in bytes.

    The library wants packed BGR pixels, rows at least 3*W and frames at least row_stride*H apart.
    A view that satisfies this is passed as it is (a region of interest stays a pointer offset);
    any other (channels or rows reversed, a permuted [N,3,H,W], overlapping rows) is copied once.
    A size-1 axis may carry any stride (0 for a numpy newaxis): it gets the dense one."""
    dev = hasattr(frames, "data_ptr")
    v = frames if dev else np.asarray(frames)
    if v.ndim != 4 or v.shape[3] != 3 or (str(v.dtype) != "torch.uint8" if dev else v.dtype != np.uint8):
        raise ValueError("expected uint8 crops [N, h, w, 3]" if what == "crops" else
                         "expected uint8 frames [N, H, W, 3]")
    N, H, W, _ = v.shape
    if N < 1 or H < 1 or W < 1:
        raise ValueError("no %s, or an empty region of interest" % what)
    for copied in (False, True):
        st = v.stride() if dev else v.strides
        row_stride = st[1] if H > 1 else 3 * W
        frame_stride = st[0] if N > 1 else row_stride * H
        if st[3] == 1 and (st[2] == 3 or W == 1) and row_stride >= 3 * W and frame_stride >= row_stride * H:
            return v, _ptr(v), N, H, W, int(row_stride), int(frame_stride), bool(dev and v.is_cuda)
        if copied:
            raise ValueError("%s with strides %s cannot be made dense" % (what, tuple(st)))
        v = v.contiguous() if dev else np.ascontiguousarray(v)


def groups_args(views):
    """frames_view results of the groups of one opose_body_infer_groups call -> the call's
    (n_groups, bgr, N, H, W, row_stride, frame_stride) as ctypes arrays."""
    n = len(views)
    return (n, (C.c_void_p * n)(*[v[1] for v in views]), (C.c_int * n)(*[v[2] for v in views]),
            (C.c_int * n)(*[v[3] for v in views]), (C.c_int * n)(*[v[4] for v in views]),
            (C.c_int64 * n)(*[v[5] for v in views]), (C.c_int64 * n)(*[v[6] for v in views]))


class Handle:
    """One device, one stream, weights + workspace (opose_t*)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        rc = lib.opose_create(int(device), C.byref(h))
        if rc != OPOSE_OK:
            raise OposeError(rc, "opose_create failed (no usable HIP device?)")
        self.h = h
        self.device = device
        # The handle runs on the library's own stream until the first device-tensor call
        # (wait_torch / signal_torch / hold): numpy-only callers never import torch or touch its
        # HIP context.  From then on the handle's stream is a torch pool stream (torch never
        # destroys those), so tensors whose last use is queued there (Handle.hold ->
        # record_stream) can be freed at any time, even after this handle is gone.  Torch hands
        # out its 32 pool streams per device round-robin: an unrelated torch.cuda.Stream() may be
        # the same HIP stream.  That only serialises the two users; opose_wait_stream /
        # opose_signal_stream order the library's streams correctly when a caller's stream is
        # the handle's own (tests/test_gpu_streams.py).
        self._torch_stream_obj = None

    def close(self):
        if getattr(self, "h", None):
            lib.opose_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != OPOSE_OK:
            raise OposeError(rc, (lib.opose_last_error(self.h) or b"").decode())
        return rc

    # ---- configuration
    def set_capacity(self, peaks_per_part: int, max_people: int):
        self.check(lib.opose_set_capacity(self.h, peaks_per_part, max_people))

    def record_bytes(self) -> int:
        return int(lib.opose_body_record_bytes(self.h))

    def set_stream(self, stream_ptr: int | None):
        self.check(lib.opose_set_stream(self.h, stream_ptr or None))

    def stream(self) -> int:
        return lib.opose_get_stream(self.h) or 0

    def torch_stream(self):
        """The handle's stream as a torch.cuda.Stream (adopting a torch pool stream first): what
        consumers of pipelined outputs order themselves on."""
        self._adopt_torch_stream()
        return self._torch_stream_obj

    def synchronize(self):
        self.check(lib.opose_synchronize(self.h))

    def flush(self):
        """Enqueue a post-network part deferred by a pipeline="defer" call (OPOSE_PIPELINE_DEFER):
        afterwards the last call's records are complete in the handle's stream order."""
        self.check(lib.opose_flush(self.h))

    # ---- RCCL for row-band halo exchanges (opose_body_band_maps with the library's exchange)
    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = lib.opose_rccl_unique_id(buf, 128)
        if rc != OPOSE_OK:
            raise OposeError(rc, "ncclGetUniqueId failed")
        return bytes(buf)

    def rccl_init(self, uid: bytes, rank: int, nranks: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid[:128])
        self.check(lib.opose_rccl_init(self.h, buf, int(rank), int(nranks)))

    def rccl_abort(self):
        """ncclCommAbort on the band communicator: this rank's own queued halo send / recv exit.
        It does not reach the neighbours' queued kernels; they bound their wait with rccl_wait."""
        self.check(lib.opose_rccl_abort(self.h))

    def rccl_wait(self, timeout_s: float):
        """Wait for the handle's stream (the RCCL halo exchanges of band_maps) for at most
        timeout_s.  A neighbour that failed, or an asynchronous RCCL error, makes the library abort
        this rank's communicator so its queued send / recv exit: TimeoutError / OposeError."""
        rc = lib.opose_rccl_wait(self.h, max(0, int(timeout_s * 1000)))
        if rc == OPOSE_E_TIMEOUT:
            raise TimeoutError((lib.opose_last_error(self.h) or b"").decode())
        self.check(rc)

    def set_band_peers(self, up, dn):
        self.check(lib.opose_set_band_peers(self.h, -1 if up is None else int(up), -1 if dn is None else int(dn)))

    # ---- ordering against torch's current stream (every device-tensor entry point)
    def _adopt_torch_stream(self):
        if self._torch_stream_obj is None:
            import torch
            self._torch_stream_obj = torch.cuda.Stream(device=torch.device("cuda", self.device))
            self.set_stream(self._torch_stream_obj.cuda_stream)  # ordered after the library's own stream

    def _torch_stream(self):
        import torch
        self._adopt_torch_stream()
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream or None)

    def wait_torch(self):
        """The handle's next work starts after everything queued on torch's current stream."""
        self.check(lib.opose_wait_stream(self.h, self._torch_stream()))

    def signal_torch(self):
        """Torch's current stream continues after everything queued on the handle: outputs are
        complete for torch consumers and the inputs the handle read may be freed/reused."""
        self.check(lib.opose_signal_stream(self.h, self._torch_stream()))

    def torch_call(self, fn, *args):
        """check(fn(handle, *args)) between wait_torch and signal_torch: a call whose device
        inputs come from torch's current stream and whose device outputs go back to it."""
        self.wait_torch()
        self.check(fn(self.h, *args))
        self.signal_torch()

    def signal_input(self, stream=None):
        """Work queued on `stream` (a torch.cuda.Stream; default torch's current stream) from now on
        starts once the handle has read the device inputs of every call so far: after pipelined
        calls, the end of the last call's network part (opose_signal_input)."""
        import torch
        self._adopt_torch_stream()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.check(lib.opose_signal_input(self.h, C.c_void_p(st.cuda_stream or None)))

    def hold(self, *tensors):
        """Keep the caching allocator from reusing these tensors' memory until the handle's
        stream passes this point (asynchronous calls whose outputs stay on the handle's stream)."""
        self._adopt_torch_stream()
        st = self._torch_stream_obj
        if st.cuda_stream != self.stream():
            raise RuntimeError("Handle.hold needs the handle on its torch pool stream (set_stream changed it)")
        for t in tensors:
            t.record_stream(st)

    # ---- weights
    def load_weights(self, net: int, tensors):
        """tensors: list of float32 C-contiguous numpy arrays in reference state_dict order."""
        arrs = [np.ascontiguousarray(t, dtype=np.float32) for t in tensors]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        shapes = np.ones((len(arrs), 4), np.int64)
        for i, a in enumerate(arrs):
            shapes[i, :a.ndim] = a.shape
        self.check(lib.opose_load_weights(self.h, net, ptrs, shapes.ctypes.data, len(arrs)))

    # ---- profiling
    def profile(self, enable: bool):
        self.check(lib.opose_profile_enable(self.h, int(enable)))

    def profile_reset(self):
        self.check(lib.opose_profile_reset(self.h))

    def profile_read(self) -> dict:
        import json
        buf = C.create_string_buffer(1 << 20)
        self.check(lib.opose_profile_read(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())


def record_bytes(peaks_per_part: int, max_people: int) -> int:
    return 16 + 32 * 18 * peaks_per_part + 160 * max_people


def encode_record(candidate, subset, peaks_per_part: int, max_people: int, status: int = 0) -> np.ndarray:
    """Inverse of decode_record (host-side; used by tests and tools)."""
    rec = np.zeros(record_bytes(peaks_per_part, max_people), np.uint8)
    cand = np.asarray(candidate, np.float64).reshape(-1, 4)
    sub = np.asarray(subset, np.float64).reshape(-1, 20)
    if len(cand) > 18 * peaks_per_part or len(sub) > max_people:
        raise ValueError("record capacity exceeded")
    rec[:16].view(np.int32)[:3] = (status, len(cand), len(sub))
    rec[16:16 + 32 * len(cand)].view(np.float64)[:] = cand.ravel()
    off = 16 + 32 * 18 * peaks_per_part
    rec[off:off + 160 * len(sub)].view(np.float64)[:] = sub.ravel()
    return rec


def decode_record(rec: np.ndarray, peaks_per_part: int, max_people: int):
    """One Body record (uint8 view) -> (status, candidate, subset) in the reference's dtypes."""
    hdr = rec[:16].view(np.int32)
    status, n_cand, n_people = int(hdr[0]), int(hdr[1]), int(hdr[2])
    cap_c = 18 * peaks_per_part
    cand = rec[16:16 + 32 * cap_c].view(np.float64).reshape(cap_c, 4)[:n_cand].copy()
    off = 16 + 32 * cap_c
    sub = rec[off:off + 160 * max_people].view(np.float64).reshape(max_people, 20)[:n_people].copy()
    if n_cand == 0:
        cand = np.array([])          # np.array([]) in the reference when no peak exists (src/body.py:160)
    if n_people == 0:
        sub = -1 * np.ones((0, 20))  # src/body.py:159
    return status, cand, sub


def raise_record_status(status: int, peaks_per_part: int, max_people: int):
    """A record's non-zero status as the exception the reference (or its absence of limits) means."""
    if status == OPOSE_E_ASSEMBLY:
        # the reference raises here when a third subset row matches (src/body.py:170-173)
        raise IndexError("list assignment index out of range")
    if status == OPOSE_E_CAPACITY:
        raise RuntimeError("libopose: per-frame capacity exceeded (peaks_per_part=%d, max_people=%d)"
                           % (peaks_per_part, max_people))
    if status != 0:
        raise OposeError(status, "frame failed")
