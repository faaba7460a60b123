"""The learned shapelet model's rule in NumPy (include/opose.h states it too), and the seeded cases
the shapelet-net tests and scripts/gen_shapelet_net_golden.py share.

Clips are [T_i, D] arrays.  With t_pad = 0 clip i has the positions c = 0 .. T_i - m; with t_pad
> 0 every clip reads as t_pad rows, those at or past T_i as +0.  One model is a query [m, D] and a
head (w0, w1, b0, b1).  With dtype = float32 (the rule):

    s_i(c) = sum over k ascending of ( sum over d ascending of (q[k, d] - x_i[c + k, d])**2 )
             one rounding per operation, each sum from +0 (shapelet_cases.s_matrix's order)
    d_i    = the first minimum of s_i over c (by the bits of s), loc_i its c
    head   in float64 from the float32 d_i, w, b:  z_ij = w_j d_i + b_j, the log-softmax through
           the larger z, loss = -mean log p_i[y_i], dz_ij = (p_ij - [y_i = j]) / N,
           g_i = dz_i0 w_0 + dz_i1 w_1, dw_j = sum_i dz_ij d_i, db_j = sum_i dz_ij, i ascending
    dq     float32: sum over i ascending of float32(g_i) * (2 * (q[k, d] - x_i[loc_i + k, d]))
    Adam   torch's defaults on float32 state, gradients rounded to float32, one step count:
           m += (g - m) * f32(1 - 0.9); v = v * f32(0.999) + (f32(1 - 0.999) * g) * g
           p -= f32(lr / (1 - 0.9**t)) * (m / (sqrt(v) / f32(sqrt(1 - 0.999**t)) + f32(1e-8)))

With dtype = float64 every value above is float64: "the float64 statement" the goldens carry.
The loops over d, k and i are explicit; NumPy vectorises only over positions and elements, which
changes no rounding.  Every builder is cached and its arrays are shared: never modify them."""
import functools

import numpy as np

import shapelet_cases as sc
from shapelet_cases import F32, K, _rng

F64 = np.float64
TC, DU, THREADS = K["kNetTC"], K["kNetDU"], K["kNetThreads"]
Q_LDS, X_LDS, MAXMODELS = K["kNetQLdsBytes"], K["kNetXLdsBytes"], K["kNetMaxModels"]
MAXM, MAXD, MAXSEQ = sc.MAXM, sc.MAXD, sc.MAXSEQ
EPOCHS = (1, 5, 50, 200)   # where the goldens record the parameters
LR = 0.01


# ---------------------------------------------------------------------------------- the statement
def rows(x, t_pad, dtype=F32):
    """Clip x as the rule reads it: its rows, then +0 rows up to t_pad."""
    x = np.asarray(x, dtype)
    if not t_pad:
        return x
    out = np.zeros((t_pad, x.shape[1]), dtype)
    out[:len(x)] = x
    return out


def s_row(q, x, dtype=F32):
    """s(c) of query q [m, D] for every position of x [T, D]: dtype [T - m + 1]."""
    q, x = np.asarray(q, dtype), np.asarray(x, dtype)
    m, P = len(q), len(x) - len(q) + 1
    acc = np.zeros(P, dtype)
    for k in range(m):
        e = np.zeros(P, dtype)
        for d in range(q.shape[1]):
            t = q[k, d] - x[k:k + P, d]
            e = e + t * t
        acc = acc + e
    return acc


def forward(q, clips, t_pad=0, dtype=F32):
    """(d dtype [N], loc int32 [N]): the first minimum of s over each clip's positions."""
    d, loc = np.zeros(len(clips), dtype), np.zeros(len(clips), np.int32)
    for i, x in enumerate(clips):
        s = s_row(q, rows(x, t_pad, dtype), dtype)
        c = int(s.view(np.uint32 if dtype == F32 else np.uint64).argmin())  # s >= +0: bits order like values
        d[i], loc[i] = s[c], c
    return d, loc


def head_terms(d, labels, hd):
    """The head in float64: (loss, g [N], dhead [4] = (dw0, dw1, db0, db1), correct)."""
    w0, w1, b0, b1 = (F64(v) for v in hd)
    N = F64(len(d))
    loss = F64(0)
    sums = [F64(0)] * 4
    g, correct = np.zeros(len(d), F64), 0
    for i in range(len(d)):
        di, y = F64(d[i]), int(labels[i])
        z0, z1 = w0 * di + b0, w1 * di + b1
        mx = max(z0, z1)
        lse = mx + np.log(np.exp(z0 - mx) + np.exp(z1 - mx))
        lp0, lp1 = z0 - lse, z1 - lse
        dz0, dz1 = (np.exp(lp0) - (y == 0)) / N, (np.exp(lp1) - (y == 1)) / N
        g[i] = dz0 * w0 + dz1 * w1
        loss = loss + (lp1 if y else lp0)
        sums = [sums[0] + dz0 * di, sums[1] + dz1 * di, sums[2] + dz0, sums[3] + dz1]
        correct += int(z1 > z0) == y  # index 0 wins a tie
    return -(loss / N), g, np.array(sums, F64), correct


def query_grad(q, clips, loc, g, t_pad=0, dtype=F32):
    q = np.asarray(q, dtype)
    acc = np.zeros(q.shape, dtype)
    for i, x in enumerate(clips):
        xr = rows(x, max(t_pad, int(loc[i]) + len(q)) if t_pad else 0, dtype)
        win = xr[loc[i]:loc[i] + len(q)]
        acc = acc + dtype(g[i]) * (dtype(2) * (q - win))
    return acc


def grads(q, hd, clips, labels, t_pad=0, dtype=F32):
    """One backward pass: a dict of d, loc, loss, g (float64), dq, dhead (float64), correct."""
    d, loc = forward(q, clips, t_pad, dtype)
    loss, g, dhead, correct = head_terms(d, labels, hd)
    return {"d": d, "loc": loc, "loss": loss, "g": g, "dq": query_grad(q, clips, loc, g, t_pad, dtype),
            "dhead": dhead, "correct": correct}


def adam(p, g, m, v, t, lr, dtype=F32):
    """One Adam step of torch's form on arrays of dtype: (p, m, v) after it."""
    g = np.asarray(g, dtype)
    m = m + (g - m) * dtype(1.0 - 0.9)
    v = v * dtype(0.999) + (dtype(1.0 - 0.999) * g) * g
    step, bc2s = dtype(lr / (1.0 - 0.9 ** t)), dtype(np.sqrt(1.0 - 0.999 ** t))
    return p - step * (m / (np.sqrt(v) / bc2s + dtype(1e-8))), m, v


def new_state(q, hd, dtype=F32):
    q, hd = np.array(q, dtype), np.array(hd, dtype)
    return {"query": q, "head": hd, "q_m": np.zeros_like(q), "q_v": np.zeros_like(q),
            "head_m": np.zeros_like(hd), "head_v": np.zeros_like(hd), "step": 0}


def train(state, clips, labels, epochs, lr=LR, t_pad=0, dtype=F32, record=()):
    """`epochs` steps from `state` (not modified): (the new state, loss_hist, {epoch: (query, head,
    loc)} at the step counts of `record`)."""
    s = dict(state)
    hist, kept = [], {}
    for _ in range(epochs):
        r = grads(s["query"], s["head"], clips, labels, t_pad, dtype)
        hist.append(r["loss"])
        t = s["step"] + 1
        s["query"], s["q_m"], s["q_v"] = adam(s["query"], r["dq"], s["q_m"], s["q_v"], t, lr, dtype)
        s["head"], s["head_m"], s["head_v"] = adam(s["head"], r["dhead"], s["head_m"], s["head_v"], t, lr, dtype)
        s["step"] = t
        if t in record:
            kept[t] = (s["query"].copy(), s["head"].copy(), forward(s["query"], clips, t_pad, dtype)[1])
    return s, np.array(hist, F64), kept


def outputs(state, clips, labels, t_pad=0, dtype=F32):
    """What the closing forward pass returns: (dis, locs, loss, correct)."""
    d, loc = forward(state["query"], clips, t_pad, dtype)
    loss, _, _, correct = head_terms(d, labels, state["head"])
    return d, loc, loss, correct


def autograd(q, hd, clips, labels, T):
    """The reference's slidingdistance / min / Linear / CrossEntropyLoss (srcmx/shapeletmodel.py:
    36-42, 82-90) restated in float64 on the batch padded to T rows, and torch.autograd's
    gradients: a dict of loss, dq [m, D], dhead (dw0, dw1, db0, db1), g (the loss by d), d, loc."""
    import torch
    X = torch.from_numpy(padded(clips, T)).double()
    Y = torch.from_numpy(np.asarray(labels, np.int64))
    query = torch.from_numpy(np.ascontiguousarray(np.asarray(q, F64).T[None])).requires_grad_(True)
    w = torch.tensor([[float(hd[0])], [float(hd[1])]], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([float(hd[2]), float(hd[3])], dtype=torch.float64, requires_grad=True)
    QQ = torch.sum(torch.square(query))
    XX = torch.nn.functional.conv1d(torch.square(X), weight=torch.ones_like(query))
    QX = torch.nn.functional.conv1d(X, weight=query)
    DIS = (QQ + XX - 2 * QX).squeeze(dim=1)
    d, loc = torch.min(DIS, dim=1, keepdim=True)
    d.retain_grad()
    loss = torch.nn.CrossEntropyLoss()(torch.nn.functional.linear(d, w, b), Y)
    loss.backward()
    return {"loss": float(loss.detach()), "dq": query.grad[0].numpy().T,
            "dhead": np.array([w.grad[0, 0], w.grad[1, 0], b.grad[0], b.grad[1]], F64),
            "g": d.grad[:, 0].numpy(), "d": d[:, 0].detach().numpy(), "loc": loc[:, 0].numpy()}


# ---------------------------------------------------------------------------------- golden cases
GOLDEN_SEEDS = [0, 1, 2, 3, 4, 5]
GOLDEN_REJECTED = []
GOLDEN_N, GOLDEN_T, GOLDEN_D, GOLDEN_M = 12, 40, 6, 7


@functools.lru_cache(maxsize=None)
def golden_case(seed):
    """(clips, labels, query0 [m, D]): ragged clips of up to GOLDEN_T rows; the even ones are
    positive and hold the pattern with noise of sigma 0.05; the query starts at the pattern plus
    noise of sigma 0.5.  The head comes from the golden file (a CPU nn.Linear(1, 2) after
    torch.manual_seed(seed))."""
    rng = np.random.default_rng(7100 + seed)
    N, T, D, m = GOLDEN_N, GOLDEN_T, GOLDEN_D, GOLDEN_M
    pattern = rng.normal(size=(m, D)).astype(F32)
    lengths = rng.integers(T // 2, T + 1, N)
    lengths[rng.integers(N)] = T
    clips, labels = [], np.zeros(N, np.uint8)
    for i in range(N):
        x = rng.normal(size=(int(lengths[i]), D)).astype(F32)
        if i % 2 == 0:
            at = int(rng.integers(0, lengths[i] - m + 1))
            x[at:at + m] = pattern + rng.normal(scale=0.05, size=(m, D)).astype(F32)
            labels[i] = 1
        clips.append(x)
    query0 = (pattern + rng.normal(scale=0.5, size=(m, D))).astype(F32)
    return clips, labels, query0


def padded(clips, T):
    """The reference's batch: float32 [N, D, T], zero past each clip."""
    X = np.zeros((len(clips), clips[0].shape[1], T), F32)
    for i, x in enumerate(clips):
        X[i, :, :len(x)] = x.T
    return X


# ---------------------------------------------------------------------------------- forward cases
def q_bytes(m, D):
    return 4 * m * D


def x_bytes(m, D):
    return 4 * (TC + m - 1) * (D | 1)


def lds_path(queries):
    """(query in LDS, clip tile in LDS) as launch_shapelet_net_forward chooses for these queries."""
    m, D = max(len(q) for q in queries), queries[0].shape[1]
    return q_bytes(m, D) <= Q_LDS, x_bytes(m, D) <= X_LDS


def _clips(rng, lengths, D):
    return [rng.normal(size=(int(n), D)).astype(F32) for n in lengths]


# name -> (m, D, clip lengths, t_pad)
FORWARD_SHAPES = {
    "m1": (1, 5, (9, 1, 14), 0),
    "m128": (MAXM, 3, (MAXM, MAXM + TC, MAXM + 2 * TC + 9), 0),
    "D1": (5, 1, (30, 6, 5), 0),
    "D_chunk+1": (4, DU + 1, (11, 23), 0),
    "D1024": (2, MAXD, (7, 3), 0),
    "q_lds_under": (32, Q_LDS // 128 - 1, (40, 33), 0),
    "q_lds_over": (32, Q_LDS // 128 + 1, (40, 33), 0),
    "q_global_x_lds": (100, 45, (100, 180), 0),
    "one_tile": (6, 4, (TC + 5,), 0),
    "tile+1": (6, 4, (TC + 6,), 0),
    "tiles": (6, 4, (3 * TC + 10, 2 * TC + 5, 7), 0),
    "N1": (3, 2, (10,), 0),
    "pad_short": (6, 3, (2, 0, 9, 20), 25),
}
FORWARD_CASES = list(FORWARD_SHAPES) + ["first_of_two", "min_in_padding", "models3"]


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """(clips, queries, t_pad)"""
    rng = _rng("net_forward_" + name)
    if name in FORWARD_SHAPES:
        m, D, lengths, t_pad = FORWARD_SHAPES[name]
        return _clips(rng, lengths, D), [rng.normal(size=(m, D)).astype(F32)], t_pad
    if name == "first_of_two":
        # the query itself twice in a clip, in different tiles and within one: the first c wins
        m, D = 5, 3
        q = rng.normal(size=(m, D)).astype(F32)
        clips = _clips(rng, (3 * TC, TC), D)
        for at in (TC - 2, 2 * TC + 7):
            clips[0][at:at + m] = q
        for at in (9, 30):
            clips[1][at:at + m] = q
        return clips, [q], 0
    if name == "min_in_padding":
        # the query's first rows end the clip and its other rows are +0: s = 0 at len - 2 only
        m, D = 6, 3
        q = np.zeros((m, D), F32)
        q[:2] = rng.normal(size=(2, D)).astype(F32) + 3
        clips = _clips(rng, (12, 2, 17), D)
        for x in clips:
            x[-2:] = q[:2]
        return clips, [q], 17 + m
    if name == "models3":
        D = 7
        return (_clips(rng, (TC + 40, 35, 64), D),
                [rng.normal(size=(m, D)).astype(F32) for m in (9, 3, 31)], 0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def forward_expected(name):
    clips, queries, t_pad = forward_case(name)
    return [forward(q, clips, t_pad) for q in queries]


# ---------------------------------------------------------------------------------- gradient cases
# Values on a grid of 1/4 and small: every fp32 distance is then exact, so d and loc are the same
# in float32 and float64 and a float64 autograd differs from the rule only by what the gradient
# bound names (the rounding of g and the fp32 sum over the clips).
GRAD_CASES = {"N1": (1, 0), "N12": (12, 0), "N300": (300, 0), "all_in_padding": (12, 9)}


@functools.lru_cache(maxsize=None)
def grad_case(name):
    """(clips, labels, query, head, t_pad)"""
    rng = _rng("net_grad_" + name)
    N, t_pad = GRAD_CASES[name]
    m, D = 5, 3
    q = (rng.integers(-8, 9, (m, D)) / 4).astype(F32)
    if name == "all_in_padding":
        clips = [np.zeros((0, D), F32) for _ in range(N)]  # every window is padding
    else:
        clips = [(rng.integers(-8, 9, (int(n), D)) / 4).astype(F32) for n in rng.integers(m + 1, 3 * m, N)]
    labels = (np.arange(N) % 2 == 0).astype(np.uint8)
    head = np.array([0.03, -0.05, 0.2, -0.1], F32)
    return clips, labels, q, head, t_pad
