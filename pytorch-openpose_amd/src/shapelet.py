"""Shapelet search over motion data on the device: the reference's srcmx/PreprocessingData.py
MotionJointFeatures, srcmx/utilmx.py SlidingDistance and srcmx/shapeletmodel.py
ShapeletMatrixModel.train through libopose's shapelet entry points (include/opose.h states the
distance, score and selection rules; tests/shapelet_cases.py restates them in NumPy).

Host arrays in give host arrays out.  torch CUDA tensors in give CUDA tensors out, ordered on
torch's current stream (Handle.torch_call), with no host round trip of the data; the row offsets and
labels are small host arrays either way."""
from __future__ import annotations

import numpy as np

from . import _native
from ._native import lib

_HANDLES = {}


def default_handle(device: int = 0) -> _native.Handle:
    """The handle the module-level functions share (one per device, made on first use)."""
    if device not in _HANDLES:
        _HANDLES[device] = _native.Handle(device)
    return _HANDLES[device]


def _is_dev(a) -> bool:
    return hasattr(a, "data_ptr") and a.is_cuda


def _offsets(lengths) -> np.ndarray:
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(np.asarray(lengths, np.int64), out=off[1:])
    return off


def _run(handle, dev, fn, *args):
    if dev:
        handle.torch_call(fn, *args)
    else:
        handle.check(fn(handle.h, *args))


def MotionJointFeatures(motiondata, datamode=None, featuremode=0, lengths=None, handle=None):
    """motiondata [T, C, 3] float64 with C = 18 ('pose') or 60 ('posehand') -> float32 [T, F, 2].
    lengths: the clips concatenated in motiondata (default: one clip); fills never cross a clip."""
    import torch
    dev = _is_dev(motiondata)
    m = motiondata.contiguous() if dev else np.ascontiguousarray(motiondata, np.float64)
    if m.ndim != 3 or m.shape[2] != 3 or (dev and m.dtype != torch.float64):
        raise ValueError("expected float64 motion data [T, C, 3]")
    T, Cn, _ = m.shape
    if datamode is None:
        datamode = {18: "pose", 60: "posehand"}.get(Cn)
    if datamode not in ("pose", "posehand") or Cn != {"pose": 18, "posehand": 60}[datamode]:
        raise Exception("please input correct datamode")
    off = _offsets([T] if lengths is None else lengths)
    if off[-1] != T:
        raise ValueError("lengths do not add up to the rows of motiondata")
    F = 6 if Cn == 18 else 46
    h = handle or default_handle(m.device.index if dev else 0)
    out = torch.empty((T, F, 2), dtype=torch.float32, device=m.device) if dev else np.empty((T, F, 2), np.float32)
    _run(h, dev, lib.opose_motion_features, _native._ptr(m), off.ctypes.data, len(off) - 1, Cn, int(featuremode),
         _native._ptr(out), _native.DEVICE_IO if dev else 0)
    return out


def _ragged(X):
    """X: a list of [T_i, D] arrays / tensors, or an [N, D, T] tensor -> (seq [L, D] float32, off, dev)."""
    import torch
    if isinstance(X, (list, tuple)):
        dev = _is_dev(X[0])
        if dev:
            seq = torch.cat([x.to(torch.float32) for x in X], dim=0).contiguous()
        else:
            seq = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32) for x in X], axis=0))
        return seq, _offsets([len(x) for x in X]), dev
    N, D, T = X.shape
    dev = _is_dev(X)
    if dev:
        seq = X.permute(0, 2, 1).reshape(-1, D).to(torch.float32).contiguous()
    else:
        seq = np.ascontiguousarray(np.asarray(X, np.float32).transpose(0, 2, 1).reshape(-1, D))
    return seq, _offsets([T] * N), dev


def SlidingDistance(pattern, sequence, handle=None):
    """The distance of pattern [m, D] to every window of sequence [n, D]: float32 [n - m + 1]."""
    import torch
    dev = _is_dev(sequence)
    if dev:
        s = sequence.to(torch.float32).contiguous()
        p = torch.as_tensor(pattern, dtype=torch.float32, device=s.device).contiguous()
    else:
        s = np.ascontiguousarray(sequence, np.float32)
        p = np.ascontiguousarray(pattern, np.float32)
    if s.ndim == 1:
        s, p = s.reshape(-1, 1), p.reshape(-1, 1)
    n, D = s.shape
    m = len(p)
    off = _offsets([n])
    h = handle or default_handle(s.device.index if dev else 0)
    n_out = max(n - m + 1, 0)
    out = torch.empty(n_out, dtype=torch.float32, device=s.device) if dev else np.empty(n_out, np.float32)
    _run(h, dev, lib.opose_sliding_distance, _native._ptr(p), m, _native._ptr(s), off.ctypes.data, 1, D,
         _native._ptr(out), _native.DEVICE_IO if dev else 0)
    return out


def _lengths(m_lens) -> np.ndarray:
    return np.ascontiguousarray([int(m) for m in m_lens], np.int32)


def _labels(labels) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels) != 0, np.uint8)


def _n_cand(off, seqs, m) -> int:
    """The candidate starts of the sequences `seqs` at window length m (those outside the batch,
    which the library refuses, count none)."""
    return int(sum(max(int(off[i + 1] - off[i]) - int(m) + 1, 0) for i in seqs if 0 <= i < len(off) - 1))


def _empty(dev, like, shape, np_dtype):
    import torch
    if dev:
        return torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=like.device)
    return np.empty(shape, np_dtype)


def _find_outputs(dev, like, lead, n_seq, n_cand, every):
    """The outputs of a find call, with leading dimensions `lead` (() or (n_lens,)): best lead + (4,),
    loss lead + (1,), dis and locs lead + (n_seq,), and nums / losses [n_cand] (None unless every)."""
    best, loss = _empty(dev, like, lead + (4,), np.int32), _empty(dev, like, lead + (1,), np.float64)
    dis, locs = _empty(dev, like, lead + (n_seq,), np.float32), _empty(dev, like, lead + (n_seq,), np.int32)
    nums = _empty(dev, like, n_cand, np.int32) if every else None
    losses = _empty(dev, like, n_cand, np.float64) if every else None
    return best, loss, dis, locs, nums, losses


def shapelet_mindist(seq, off, m, cand_seqs, handle=None):
    """The first stage alone on a ragged batch: (min2, loc) [n_cand, n_seq] (opose_shapelet_mindist)."""
    dev = _is_dev(seq)
    off = np.ascontiguousarray(off, np.int64)
    cs = np.ascontiguousarray(cand_seqs, np.int32)
    n_seq, n_cand = len(off) - 1, _n_cand(off, cs, m)
    h = handle or default_handle(seq.device.index if dev else 0)
    min2, loc = _empty(dev, seq, (n_cand, n_seq), np.float32), _empty(dev, seq, (n_cand, n_seq), np.int32)
    _run(h, dev, lib.opose_shapelet_mindist, _native._ptr(seq), off.ctypes.data, n_seq, seq.shape[1], int(m),
         cs.ctypes.data, len(cs), _native._ptr(min2), _native._ptr(loc), _native.DEVICE_IO if dev else 0)
    return min2, loc


def shapelet_find(seq, off, labels, m, max_cands=0, every=False, handle=None):
    """opose_shapelet_find on a ragged batch: a dict of best [4], loss, dis [n_seq], locs [n_seq] (and,
    with every=True, every candidate's num and loss).  Device inputs give device outputs."""
    dev = _is_dev(seq)
    off = np.ascontiguousarray(off, np.int64)
    lab = _labels(labels)
    n_seq, n = len(off) - 1, len(lab)
    n_cand = _n_cand(off, np.nonzero(lab)[0], m)
    h = handle or default_handle(seq.device.index if dev else 0)
    best, loss, dis, locs, nums, losses = _find_outputs(dev, seq, (), n_seq, n_cand, every)
    _run(h, dev, lib.opose_shapelet_find, _native._ptr(seq), off.ctypes.data, n_seq, seq.shape[1], int(m),
         lab.ctypes.data, n, int(max_cands), _native._ptr(best), _native._ptr(loss), _native._ptr(dis),
         _native._ptr(locs), _native._ptr(nums) if every else None, _native._ptr(losses) if every else None,
         _native.DEVICE_IO if dev else 0)
    return {"best": best, "loss": loss, "dis": dis, "locs": locs, "nums": nums, "losses": losses}


def shapelet_mindist_lengths(seq, off, m_lens, cand_seqs, handle=None):
    """shapelet_mindist for the ascending window lengths m_lens in one pass over shared distances
    (opose_shapelet_mindist_lengths): a list of (min2, loc) [n_cand_l, n_seq] per length, views of
    the two output buffers."""
    dev = _is_dev(seq)
    off = np.ascontiguousarray(off, np.int64)
    cs = np.ascontiguousarray(cand_seqs, np.int32)
    ml = _lengths(m_lens)
    n_seq = len(off) - 1
    starts = np.concatenate(([0], np.cumsum([_n_cand(off, cs, m) for m in ml], dtype=np.int64)))
    h = handle or default_handle(seq.device.index if dev else 0)
    shape = (int(starts[-1]), n_seq)
    min2, loc = _empty(dev, seq, shape, np.float32), _empty(dev, seq, shape, np.int32)
    _run(h, dev, lib.opose_shapelet_mindist_lengths, _native._ptr(seq), off.ctypes.data, n_seq, seq.shape[1],
         ml.ctypes.data, len(ml), cs.ctypes.data, len(cs), _native._ptr(min2), _native._ptr(loc),
         _native.DEVICE_IO if dev else 0)
    return [(min2[a:b], loc[a:b]) for a, b in zip(starts[:-1], starts[1:])]


def shapelet_find_lengths(seq, off, labels, m_lens, max_cands=0, every=False, handle=None):
    """opose_shapelet_find_lengths on a ragged batch: a list, per length of m_lens, of the dict
    shapelet_find returns (views of the call's output buffers).  Device inputs give device outputs."""
    dev = _is_dev(seq)
    off = np.ascontiguousarray(off, np.int64)
    lab = _labels(labels)
    ml = _lengths(m_lens)
    n_seq, n, nl = len(off) - 1, len(lab), len(ml)
    starts = np.concatenate(([0], np.cumsum([_n_cand(off, np.nonzero(lab)[0], m) for m in ml], dtype=np.int64)))
    h = handle or default_handle(seq.device.index if dev else 0)
    best, loss, dis, locs, nums, losses = _find_outputs(dev, seq, (nl,), n_seq, int(starts[-1]), every)
    _run(h, dev, lib.opose_shapelet_find_lengths, _native._ptr(seq), off.ctypes.data, n_seq, seq.shape[1],
         ml.ctypes.data, nl, lab.ctypes.data, n, int(max_cands), _native._ptr(best), _native._ptr(loss),
         _native._ptr(dis), _native._ptr(locs), _native._ptr(nums) if every else None,
         _native._ptr(losses) if every else None, _native.DEVICE_IO if dev else 0)
    return [{"best": best[l], "loss": loss[l], "dis": dis[l], "locs": locs[l],
             "nums": nums[starts[l]:starts[l + 1]] if every else None,
             "losses": losses[starts[l]:starts[l + 1]] if every else None} for l in range(nl)]


SCAN_FIRST_CAP = 1 << 20  # shapelet_scan's first guess at the occurrences when cap is None


def shapelet_scan(patterns, sigmas, seq, off, cap=None, max_pats=0, handle=None):
    """Every occurrence of the patterns (a list of [m_p, D] arrays or tensors) in the streams of the
    ragged batch seq [L, D] / off (opose_shapelet_scan; include/opose.h states the rule): position c
    of a stream is a hit of pattern p when its distance is below sigmas[p], and each run of
    neighbouring hits is thinned to one occurrence as the reference's AugmentateOneShapelet does.
    Returns {"off": int64 [n_pat * n_seq + 1] (pattern-major), "pos": int32 [total], "dist": float32
    [total]}.  Host in gives host out; a CUDA seq gives CUDA tensors on torch's current stream.
    cap: room for that many occurrences (more is an OposeError of code OPOSE_E_CAPACITY on the host
    path; on the device path the entries past cap are missing and off[-1] tells); None: a first
    guess, and one retry with the exact total when it was too small."""
    import torch
    dev = _is_dev(seq)
    off = np.ascontiguousarray(off, np.int64)
    sig = np.ascontiguousarray(sigmas, np.float32).reshape(-1)
    if len(sig) != len(patterns):
        raise ValueError("one sigma per pattern")
    pat_off = _offsets([len(p) for p in patterns])
    if dev:
        seq = seq.to(torch.float32).contiguous()
        pat = torch.cat([torch.as_tensor(p, dtype=torch.float32, device=seq.device).reshape(len(p), -1)
                         for p in patterns], dim=0).contiguous() if len(patterns) else seq[:0]
    else:
        seq = np.ascontiguousarray(seq, np.float32)
        pat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(len(p), -1) for p in patterns])
                                   if len(patterns) else seq[:0])
    D = seq.shape[1]
    if len(patterns) and pat.shape[1] != D:
        raise ValueError("patterns and streams differ in their feature columns")
    n_pat, n_seq = len(patterns), len(off) - 1
    h = handle or default_handle(seq.device.index if dev else 0)
    occ_off = _empty(dev, seq, max(n_pat * n_seq, 0) + 1, np.int64)

    def call(room):
        pos, dist = _empty(dev, seq, max(room, 1), np.int32), _empty(dev, seq, max(room, 1), np.float32)
        _run(h, dev, lib.opose_shapelet_scan, _native._ptr(pat), pat_off.ctypes.data, n_pat, sig.ctypes.data,
             _native._ptr(seq), off.ctypes.data, n_seq, D, int(max_pats), _native._ptr(occ_off), _native._ptr(pos),
             _native._ptr(dist), int(room), _native.DEVICE_IO if dev else 0)
        return pos, dist

    room = SCAN_FIRST_CAP if cap is None else int(cap)
    try:
        pos, dist = call(room)
    except _native.OposeError as e:
        if cap is not None or e.code != _native.OPOSE_E_CAPACITY:
            raise
        room = int(occ_off[-1])
        pos, dist = call(room)
    total = int(occ_off[-1])  # (the device path waits here for the call)
    if dev and cap is None and total > room:
        room = total
        pos, dist = call(room)
    n = min(total, room)
    return {"off": occ_off, "pos": pos[:n], "dist": dist[:n]}


class ShapeletMatrixModel:
    """The reference's brute-force shapelet model: train() keeps the window of a positive clip whose
    distances to all clips separate the labels best."""

    def __init__(self, handle=None):
        self.handle = handle

    def train(self, X, labels, m_len, mirror=None, max_cands=0):
        """X: a list of [T_i, D] arrays or an [N, D, T] tensor; labels: N values 0 / 1.  Sets
        shapeindex, cand (the window's start in clip shapeindex), locs (int16), dis, score.
        mirror 'x-mirror' / 'y-mirror': the copies with the even / odd feature columns negated are
        appended (made with torch on the device); locs, dis and the boolean `mirrored` are then the
        chosen of each pair.  (The reference's ShapeletMatrixModel_LR fails in these modes.)"""
        seq, off, n = self._batch(X, mirror)
        return self._take(shapelet_find(seq, off, labels, m_len, max_cands, handle=self.handle), n, mirror)

    def train_lengths(self, X, labels, m_lens, mirror=None, max_cands=0):
        """train for every window length of m_lens (ascending) in one search over shared distances:
        a list of models, one per length, each with m_len and the attributes train sets.  The
        mirrored copies are made and uploaded once."""
        seq, off, n = self._batch(X, mirror)
        res = shapelet_find_lengths(seq, off, labels, m_lens, max_cands, handle=self.handle)
        models = []
        for m, r in zip(m_lens, res):
            model = ShapeletMatrixModel(self.handle)._take(r, n, mirror)
            model.m_len = int(m)
            models.append(model)
        return models

    def _batch(self, X, mirror):
        """(seq, off, clips): the ragged batch of X, with the mirrored copies appended when asked."""
        import torch
        seq, off, dev = _ragged(X)
        n = len(off) - 1
        if mirror is not None:
            if mirror not in ("x-mirror", "y-mirror"):
                raise ValueError("mirror must be None, 'x-mirror' or 'y-mirror'")
            if not dev:
                device = torch.device("cuda", self.handle.device if self.handle else 0)
                seq = torch.from_numpy(seq).to(device)
            sign = torch.ones(seq.shape[1], dtype=torch.float32, device=seq.device)
            sign[(0 if mirror == "x-mirror" else 1)::2] = -1
            seq = torch.cat((seq, seq * sign), dim=0)
            off = np.concatenate((off, off[1:] + off[-1]))
        return seq, off, n

    def _take(self, res, n, mirror):
        """The model's attributes from one length's search result over n clips."""
        host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items() if v is not None}
        best, dis, locs = host["best"], host["dis"], host["locs"]
        self.shapeindex, self.cand = int(best[0]), int(best[1])
        self.score = int(best[2]) / n
        self.loss = float(host["loss"][0])
        if mirror is None:
            self.mirrored = np.zeros(n, bool)
        else:  # the smaller distance of each pair, the original on a tie.  sqrt keeps the order of s;
            # two s one rounding apart may share a square root, and the pair then reports the original
            # (same dis; the score was taken from the s values themselves)
            self.mirrored = dis[n:] < dis[:n]
        pick = np.arange(n) + n * self.mirrored
        self.dis = dis[pick].astype(np.float64)
        self.locs = locs[pick].astype(np.int16)
        return self


def brute_force_records(samples, labels, m_lens=range(15, 40, 2), mirror="x-mirror", max_cands=0, handle=None):
    """The arrays FindShaplets_brute_force_ED (srcmx/shapeletlearning.py:190-214) writes per window
    length, for every length of m_lens from one search and without the h5 file: {m: {"locs": int16
    [positives], "dists": float32 [positives], "shapelet": int16 [1], "score": float32 [1]}}."""
    lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels) != 0
    m_lens = [int(m) for m in m_lens]
    models = ShapeletMatrixModel(handle).train_lengths(samples, lab, m_lens, mirror=mirror, max_cands=max_cands)
    return {m: {"locs": model.locs[lab].astype(np.int16), "dists": model.dis[lab].astype(np.float32),
                "shapelet": np.array([model.shapeindex]).astype(np.int16),
                "score": np.array([model.score]).astype(np.float32)} for m, model in zip(m_lens, models)}
