"""Shapelet search over motion data on the device: the reference's srcmx/PreprocessingData.py
MotionJointFeatures, srcmx/utilmx.py SlidingDistance and srcmx/shapeletmodel.py
ShapeletMatrixModel.train through libopose's shapelet entry points (include/opose.h states the
distance, score and selection rules; tests/shapelet_cases.py restates them in NumPy), and the learned
model, srcmx/shapeletmodel.py ShapeletNetModel with the records of srcmx/shapeletlearning.py
FindShaplets_Net_ED, through opose_shapelet_net_train (tests/shapelet_net_cases.py).

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


NET_STATE = ("query", "head", "q_m", "q_v", "head_m", "head_v")


def shapelet_net_train(seq, off, labels, queries, heads, state=None, step0=0, epochs=0, lr=0.01, t_pad=0,
                       loss_hist=False, handle=None):
    """opose_shapelet_net_train on a ragged batch seq [L, D] / off: n_models models, one per query
    of `queries` (a list of [m_k, D]) and row of heads [n_models, 4] = (w0, w1, b0, b1), take
    `epochs` Adam steps side by side (include/opose.h states the rule; 0 epochs: the forward pass
    alone).  state: the dict a previous call returned, to continue it (its queries, heads, moments
    and step count then replace queries / heads / step0).  Nothing passed in is modified.

    Returns a dict: "query" (the concatenated queries [sum m_k, D]), "queries" (its per-model
    views), "head", "q_m", "q_v", "head_m", "head_v", "step", "q_off", and from the closing forward
    pass "dis" float32 / "locs" int32 [n_models, n_seq], "loss" float64 / "correct" int32
    [n_models]; "loss_hist" float64 [n_models, epochs] when asked for.  Host arrays in give host
    arrays out; a CUDA seq gives CUDA tensors, ordered on torch's current stream."""
    import torch
    dev = _is_dev(seq)
    off = np.ascontiguousarray(off, np.int64)
    lab = _labels(labels)
    n_seq = len(off) - 1
    if len(lab) != n_seq:
        raise ValueError("one label per clip")

    def own(a):  # a private float32 copy on the side of seq
        if dev:
            return torch.as_tensor(a, device=seq.device).to(torch.float32).contiguous().clone()
        return np.array(a.cpu() if hasattr(a, "cpu") else a, np.float32, order="C")

    if state is not None:
        st = {k: own(state[k]) for k in NET_STATE}
        q_off, step0 = np.ascontiguousarray(state["q_off"], np.int64), int(state["step"])
    else:
        qs = [own(q) for q in queries]
        q_off = _offsets([len(q) for q in qs])
        st = {"query": (torch.cat(qs, dim=0).contiguous() if dev else np.ascontiguousarray(np.concatenate(qs)))
              if len(qs) else own(np.zeros((0, 1)))}
        st["head"] = own(heads).reshape(-1, 4)
        for k, like in (("q_m", "query"), ("q_v", "query"), ("head_m", "head"), ("head_v", "head")):
            st[k] = torch.zeros_like(st[like]) if dev else np.zeros_like(st[like])
    n_models = len(q_off) - 1
    if dev:
        seq = seq.to(torch.float32).contiguous()
    else:
        seq = np.ascontiguousarray(seq, np.float32)
    D = seq.shape[1]
    if seq.shape[0] == 0:  # every clip empty (padded mode): a pointer to pass, no row of it is a clip's
        seq = torch.zeros((1, D), dtype=torch.float32, device=seq.device) if dev else np.zeros((1, D), np.float32)
    if st["query"].ndim != 2 or st["query"].shape[1] != D or len(st["query"]) != q_off[-1]:
        raise ValueError("queries and clips differ in their feature columns")
    if tuple(st["head"].shape) != (n_models, 4):
        raise ValueError("one head (w0, w1, b0, b1) per query")
    h = handle or default_handle(seq.device.index if dev else 0)
    epochs = int(epochs)
    dis, locs = _empty(dev, seq, (n_models, n_seq), np.float32), _empty(dev, seq, (n_models, n_seq), np.int32)
    loss, correct = _empty(dev, seq, n_models, np.float64), _empty(dev, seq, n_models, np.int32)
    hist = _empty(dev, seq, (n_models, max(epochs, 0)), np.float64) if loss_hist else None
    _run(h, dev, lib.opose_shapelet_net_train, _native._ptr(seq), off.ctypes.data, n_seq, D, int(t_pad),
         lab.ctypes.data, q_off.ctypes.data, n_models, *[_native._ptr(st[k]) for k in NET_STATE], int(step0), epochs,
         float(lr), _native._ptr(dis), _native._ptr(locs), _native._ptr(loss), _native._ptr(correct),
         _native._ptr(hist) if loss_hist else None, _native.DEVICE_IO if dev else 0)
    st.update({"queries": [st["query"][a:b] for a, b in zip(q_off[:-1], q_off[1:])], "q_off": q_off,
               "step": int(step0) + epochs, "dis": dis, "locs": locs, "loss": loss, "correct": correct})
    if loss_hist:
        st["loss_hist"] = hist
    return st


def _net_batch(X):
    """The clips of a ShapeletNetModel call -> (seq, off, t_pad, dev): an [N, D, T] batch is N clips
    of T rows (its padding is part of the data, as in the reference); a list of [T_i, D] clips is
    padded to the longest by the library's t_pad."""
    seq, off, dev = _ragged(X)
    t_pad = int(np.max(np.diff(off))) if isinstance(X, (list, tuple)) else 0
    return seq, off, t_pad, dev


class ShapeletNetModel:
    """The reference's learned shapelet model (srcmx/shapeletmodel.py:11-90) on libopose: a query
    [1, D, m] and a Linear(1, 2) head on the smallest squared sliding distance of each clip, trained
    by Adam on the cross-entropy.  X is an [N, D, T] array or tensor padded as in the reference, or
    a list of [T_i, D] clips (padded to the longest without materialising it); Y the N labels."""

    def __init__(self, shape, query=None, lr=0.01, handle=None):
        import torch
        m, d = shape
        if query is None:
            query = torch.randn(1, d, m, dtype=torch.float32)
        query = torch.as_tensor(query).detach().cpu().to(torch.float32)
        if tuple(query.shape) != (1, d, m):
            raise ValueError("query must be shaped [1, D, m]")
        cls = torch.nn.Linear(1, 2)  # on the CPU: a seeded run starts where the reference's does
        w, b = cls.weight.detach().numpy(), cls.bias.detach().numpy()
        self.shape, self.lr, self.handle = (int(m), int(d)), float(lr), handle
        self.state = {"query": np.ascontiguousarray(query[0].numpy().T), "q_off": np.array([0, m], np.int64),
                      "head": np.array([[w[0, 0], w[1, 0], b[0], b[1]]], np.float32), "step": 0}
        for k, like in (("q_m", "query"), ("q_v", "query"), ("head_m", "head"), ("head_v", "head")):
            self.state[k] = np.zeros_like(self.state[like])
        self.loss_hist = None

    @property
    def query(self):
        """float32 [1, D, m], as the reference's parameter."""
        return np.ascontiguousarray(self.state["query"].T[None])

    @property
    def head(self):
        return self.state["head"][0]

    def _call(self, X, Y, epochs, loss_hist=False):
        seq, off, t_pad, dev = _net_batch(X)
        if Y is None:
            Y = np.zeros(len(off) - 1, np.uint8)
        res = shapelet_net_train(seq, off, Y, None, None, state=self.state, epochs=epochs, lr=self.lr, t_pad=t_pad,
                                 loss_hist=loss_hist, handle=self.handle)
        return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items() if k != "queries"}

    def train(self, X, Y, epochs=10000):
        """`epochs` Adam steps, all enqueued at once; loss_hist keeps each epoch's loss."""
        res = self._call(X, Y, epochs, loss_hist=True)
        self.state = {k: res[k] for k in NET_STATE + ("q_off", "step")}
        self.loss_hist = res["loss_hist"][0]
        return self

    def __call__(self, X, Y):
        """(DIS float32 [N], loc int32 [N], score) of the current parameters."""
        res = self._call(X, Y, 0)
        return res["dis"][0], res["locs"][0], int(res["correct"][0]) / res["dis"].shape[1]

    def localizeshape(self, X):
        res = self._call(X, None, 0)
        return res["locs"][0], res["dis"][0]

    def getshapelet(self):
        """The learned window, float32 [m, D]."""
        return self.state["query"].copy()


def net_records(samples, labels, m_lens=range(15, 40, 2), init=None, epochs=10000, lr=0.01, handle=None):
    """The arrays FindShaplets_Net_ED (srcmx/shapeletlearning.py:223-310) writes per window length,
    for every length of m_lens from one training call and without the h5 file: {m: {"locs": int16
    [positives], "dists": float32 [positives], "shapelet": float32 [1, D, m], "score": float32 [1]}}.
    samples: a list of [T_i, D] clips, padded to the longest as the reference pads them.  Each
    length's query starts at a window of a clip: init maps a length to (clip, start), e.g. a
    brute-force model's (shapeindex, cand); a length it does not name takes the reference's
    fallback, clip 0 at start 127, and ValueError when that window does not fit the padded clip.
    Every head is a CPU nn.Linear(1, 2), drawn in the order of m_lens."""
    import torch
    lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels) != 0
    m_lens = [int(m) for m in m_lens]
    seq, off, t_pad, dev = _net_batch(list(samples))
    host = seq.cpu().numpy() if dev else seq
    queries, heads = [], []
    for m in m_lens:
        clip, start = (init or {}).get(m, (0, 127))
        clip, start = int(clip), int(start)
        if not 0 <= clip < len(off) - 1 or start < 0 or start + m > t_pad:
            raise ValueError("the starting window of length %d (clip %d, start %d) does not fit" % (m, clip, start))
        q = np.zeros((m, host.shape[1]), np.float32)  # rows past the clip's end are the padding
        rows = host[off[clip] + start:max(min(off[clip] + start + m, off[clip + 1]), off[clip] + start)]
        q[:len(rows)] = rows
        queries.append(q)
        cls = torch.nn.Linear(1, 2)
        w, b = cls.weight.detach().numpy(), cls.bias.detach().numpy()
        heads.append([w[0, 0], w[1, 0], b[0], b[1]])
    res = shapelet_net_train(seq, off, lab, queries, np.array(heads, np.float32), epochs=epochs, lr=lr, t_pad=t_pad,
                             handle=handle)
    def host(v):
        return v.cpu().numpy() if hasattr(v, "cpu") else v

    res = {k: [host(q) for q in v] if k == "queries" else host(v) for k, v in res.items()}
    return {m: {"locs": res["locs"][k][lab].astype(np.int16), "dists": res["dis"][k][lab].astype(np.float32),
                "shapelet": np.ascontiguousarray(res["queries"][k].T[None]).astype(np.float32),
                "score": np.array([int(res["correct"][k]) / len(lab)]).astype(np.float32)}
            for k, m in enumerate(m_lens)}


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
