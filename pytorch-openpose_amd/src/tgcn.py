"""The TGCN sign classifier on the device: the reference's cls/TGCN/tgcn_model.py GCN_muti_att in
evaluation mode, driven as cls/TGCN/test_tgcn.py drives it and fed as cls/TGCN/datasetcreate.py
PoseDataset feeds it, through libopose's opose_tgcn_* entry points (include/opose.h states the rule;
tests/tgcn_cases.py restates it in NumPy float64).  Inference only.

Host arrays in give host arrays out.  torch CUDA tensors in give CUDA tensors out, ordered on
torch's current stream (Handle.torch_call), with no host round trip of the data."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native
from ._native import lib
from .shapelet import _empty, _is_dev, _run, default_handle

# samples per workgroup of the graph-convolution kernel (csrc/kernels.h kTgcnG)
SAMPLES_PER_WORKGROUP = 4
BN_EPS = 1e-5  # nn.BatchNorm1d's default, which the reference keeps

_BN = ("weight", "bias", "running_mean", "running_var")


def _host(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


class GCN_muti_att:
    """The reference's constructor surface, plus the node count its layers hard-code (55) and the
    handle.  p_dropout is accepted and unused: Dropout is the identity in evaluation mode."""

    def __init__(self, input_feature, hidden_feature, num_class, p_dropout=0.0, num_stage=1, is_resi=True,
                 n_nodes=55, handle=None):
        self.input_feature, self.hidden_feature, self.num_class = int(input_feature), int(hidden_feature), int(num_class)
        self.num_stage, self.is_resi, self.n_nodes = int(num_stage), bool(is_resi), int(n_nodes)
        self.p_dropout = p_dropout
        self._handle = handle
        self._params = None  # the float32 blob of opose_tgcn_create
        self._model = None   # (handle, opose_tgcn_t*)

    # ---- weights
    def layer_keys(self):
        """(gc prefix, bn prefix, input features) of the 1 + 2 num_stage layers, in the blob's order."""
        out = [("gc1", "bn1", self.input_feature)]
        for i in range(self.num_stage):
            out += [(f"gcbs.{i}.gc1", f"gcbs.{i}.bn1", self.hidden_feature),
                    (f"gcbs.{i}.gc2", f"gcbs.{i}.bn2", self.hidden_feature)]
        return out

    def expected_shapes(self) -> dict:
        """key -> shape of every tensor load_state_dict needs, in the blob's order."""
        V, H = self.n_nodes, self.hidden_feature
        sh = {}
        for gc, bn, F in self.layer_keys():
            sh[gc + ".weight"], sh[gc + ".att"], sh[gc + ".bias"] = (F, H), (V, V), (H,)
            for k in _BN:
                sh[bn + "." + k] = (V * H,)
        sh["fc_out.weight"], sh["fc_out.bias"] = (self.num_class, H), (self.num_class,)
        return sh

    def load_state_dict(self, sd):
        """The reference's own keys; num_batches_tracked (and any other key) is ignored.  ValueError
        on a missing key or a wrong shape."""
        parts = []
        for key, shape in self.expected_shapes().items():
            if key not in sd:
                raise ValueError("state dict has no " + key)
            a = _host(sd[key])
            if tuple(a.shape) != shape:
                raise ValueError("%s has shape %s, the model takes %s" % (key, tuple(a.shape), shape))
            parts.append(np.ascontiguousarray(a, np.float32).ravel())
        self._params = np.concatenate(parts)
        self._drop_model()
        return self

    def _drop_model(self):
        if self._model is not None:
            h, m = self._model
            self._model = None
            if getattr(h, "h", None):
                lib.opose_tgcn_destroy(h.h, m)

    def __del__(self):
        try:
            self._drop_model()
        except Exception:
            pass

    def _device_model(self, device):
        if self._params is None:
            raise ValueError("load_state_dict first: the model has no weights")
        h = self._handle or default_handle(device)
        if self._model is None or self._model[0] is not h:
            self._drop_model()
            m = C.c_void_p()
            h.check(lib.opose_tgcn_create(h.h, self.n_nodes, self.input_feature, self.hidden_feature, self.num_class,
                                          self.num_stage, int(self.is_resi), BN_EPS, self._params.ctypes.data,
                                          self._params.size, C.byref(m)))
            self._model = (h, m)
        return self._model

    def eval(self):
        return self

    # ---- forward
    def _input(self, x, copies):
        dev = _is_dev(x)
        if dev:
            import torch
            if x.dtype != torch.float32:
                raise ValueError("expected float32 input")
            x = x.contiguous()
        else:
            x = np.ascontiguousarray(_host(x), np.float32)
        if x.ndim != 3 or x.shape[1] != self.n_nodes or x.shape[2] != copies * self.input_feature or x.shape[0] < 1:
            raise ValueError("expected input [B >= 1, %d, %d]" % (self.n_nodes, copies * self.input_feature))
        return x, dev

    def forward_copies(self, x, copies=1, max_samples=0, copy_logits=False):
        """x [B, V, copies * F_in] -> logits [B, C], the mean over the copies (copy i is columns
        [i F_in, (i + 1) F_in), read in place); with copy_logits also every copy's [B, copies, C]."""
        copies = int(copies)
        if copies < 1:
            raise ValueError("copies must be positive")
        x, dev = self._input(x, copies)
        h, m = self._device_model(x.device.index if dev else 0)
        B = x.shape[0]
        out = _empty(dev, x, (B, self.num_class), np.float32)
        cl = _empty(dev, x, (B, copies, self.num_class), np.float32) if copy_logits else None
        _run(h, dev, lib.opose_tgcn_forward, m, _native._ptr(x), B, copies, int(max_samples), _native._ptr(out),
             _native._ptr(cl) if copy_logits else None, _native.DEVICE_IO if dev else 0)
        return (out, cl) if copy_logits else out

    def forward(self, x):
        return self.forward_copies(x, 1)

    __call__ = forward

    def debug_layer(self, layer, x_in, residual=None):
        """One graph-convolution layer alone on host arrays (opose_debug_tgcn_layer)."""
        h, m = self._device_model(0)
        x = np.ascontiguousarray(x_in, np.float32)
        out = np.empty((x.shape[0], self.n_nodes, self.hidden_feature), np.float32)
        r = None if residual is None else np.ascontiguousarray(residual, np.float32)
        h.check(lib.opose_debug_tgcn_layer(h.h, m, int(layer), x.ctypes.data, x.shape[0],
                                           None if r is None else r.ctypes.data, out.ctypes.data))
        return out

    def classify(self, X, num_copies=4, topk=1):
        """What test_tgcn.test does per batch: the mean of the num_copies slices' logits and its top
        classes -> (logits [B, C], indices [B, topk], best first)."""
        logits = self.forward_copies(X, num_copies)
        if _is_dev(logits):
            idx = logits.topk(int(topk), dim=1)[1]
        else:
            idx = np.argsort(-logits, axis=1, kind="stable")[:, :int(topk)]
        return logits, idx


def top_n_accuracy(truths, logits, n):
    """The reference's compute_top_n_accuracy (cls/TGCN/test_tgcn.py:76-83)."""
    truths, logits = _host(truths), _host(logits)
    best_n = np.argsort(logits, axis=1)[:, -int(n):]
    hits = sum(1 for i in range(truths.shape[0]) if truths[i] in best_n[i, :])
    return float(hits) / truths.shape[0]


def clip_inputs(data, ranges, num_samples, copies=1):
    """The classifier's input of n clips of one video: data [T, V, >= 2] (a MotionMat, or the
    [T, F, 2] of MotionJointFeatures, which the reference's PoseDataset feeds), ranges [n, 2] rows
    [begin, end) -> float32 [n, V, copies * 2 * num_samples].

    A clip of len frames gives the frame begin + floor(j * len / (copies * num_samples)) for
    j = k * copies + i, so each copy i spans the whole clip and a short clip repeats frames; its
    coordinate c lands in column i * 2 * num_samples + 2 * k + c.  (The reference's
    Random_select_frames(randommode=1) calls round on an array and cannot run; this is the stated
    replacement.)  Plumbing in torch or NumPy, no kernel."""
    dev = hasattr(data, "data_ptr")
    num_samples, copies = int(num_samples), int(copies)
    if num_samples < 1 or copies < 1:
        raise ValueError("num_samples and copies must be positive")
    if data.ndim != 3 or data.shape[2] < 2:
        raise ValueError("expected data [T, V, >= 2]")
    r = np.asarray(_host(ranges), np.int64).reshape(-1, 2)
    T, V = data.shape[0], data.shape[1]
    if (r[:, 0] < 0).any() or (r[:, 1] > T).any() or (r[:, 1] <= r[:, 0]).any():
        raise ValueError("a range is empty or leaves the data")
    n, S = len(r), copies * num_samples
    j = np.arange(S, dtype=np.int64)
    frames = r[:, :1] + (j[None, :] * (r[:, 1] - r[:, 0])[:, None]) // S      # [n, S], j = k * copies + i
    frames = frames.reshape(n, num_samples, copies).transpose(0, 2, 1)       # [n, i, k]
    if dev:
        import torch
        idx = torch.as_tensor(frames.reshape(-1), device=data.device)
        g = data[:, :, :2].to(torch.float32).index_select(0, idx).reshape(n, copies, num_samples, V, 2)
        return g.permute(0, 3, 1, 2, 4).reshape(n, V, copies * 2 * num_samples).contiguous()
    g = np.asarray(data)[:, :, :2].astype(np.float32)[frames.reshape(-1)].reshape(n, copies, num_samples, V, 2)
    return np.ascontiguousarray(g.transpose(0, 3, 1, 2, 4).reshape(n, V, copies * 2 * num_samples))
