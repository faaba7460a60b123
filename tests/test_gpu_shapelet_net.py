"""GPU: the learned shapelet model (shapelet_net_forward / _head / _step in csrc/shapelet_net.hip,
opose_shapelet_net_train / opose_debug_shapelet_net_grad, and their Python forms in
src/shapelet.py) against the NumPy statement of tests/shapelet_net_cases.py, float64 autograd and
the reference's goldens.  Distances and locations are held to bit equality with the statement; the
trained parameters to the tolerance the golden generator measured.
tests/test_shapelet_net_cases.py shows on the CPU that each case has the geometry it claims."""
import json
import os

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

import shapelet_net_cases as nc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
STATE = ("query", "head", "q_m", "q_v", "head_m", "head_v")
OUTS = ("dis", "locs", "loss", "correct")


@pytest.fixture(scope="module")
def sh():
    from src import shapelet
    return shapelet


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "shapelet_net_ref.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLDEN, "shapelet_net_ref.npz")), meta


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def ragged(clips):
    D = clips[0].shape[1]
    return (np.ascontiguousarray(np.concatenate([np.asarray(x, F32).reshape(-1, D) for x in clips]), F32),
            np.cumsum([0] + [len(x) for x in clips]).astype(np.int64))


def same_bits(a, b, keys=STATE + OUTS):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def forward(sh, clips, queries, t_pad):
    seq, off = ragged(clips)
    n = len(queries)
    return sh.shapelet_net_train(seq, off, np.zeros(len(clips), np.uint8), queries, np.zeros((n, 4), F32), epochs=0,
                                 t_pad=t_pad)


# ---------------------------------------------------------------- 1. the forward pass alone
@pytest.mark.parametrize("name", nc.FORWARD_CASES)
def test_forward_equals_the_statement(sh, name):
    clips, queries, t_pad = nc.forward_case(name)
    got = forward(sh, clips, queries, t_pad)
    assert got["step"] == 0
    for k, (d, loc) in enumerate(nc.forward_expected(name)):
        assert np.array_equal(got["locs"][k], loc), (name, k)
        assert np.array_equal(bits(got["dis"][k]), bits(d)), (name, k)
    for k, q in enumerate(queries):  # epochs = 0 leaves the parameters alone
        assert np.array_equal(bits(got["queries"][k]), bits(q))
    if len(queries) > 1:  # side by side equals one at a time
        for k, q in enumerate(queries):
            one = forward(sh, clips, [q], t_pad)
            assert np.array_equal(bits(one["dis"][0]), bits(got["dis"][k]))
            assert np.array_equal(one["locs"][0], got["locs"][k])


# ---------------------------------------------------------------- 2. one backward pass
def debug_grad(native, sh, clips, labels, q, head, t_pad):
    seq, off = ragged(clips)
    if not len(seq):
        seq = np.zeros((1, q.shape[1]), F32)  # a pointer to pass; no row of it belongs to a clip
    n = len(clips)
    g, dq = np.full(n, -7, F32), np.full(q.shape, -7, F32)
    dhead, loss = np.full(4, -7, F64), np.full(1, -7, F64)
    q, head = np.ascontiguousarray(q, F32), np.ascontiguousarray(head, F32)
    lab = np.ascontiguousarray(labels, np.uint8)
    rc = native.lib.opose_debug_shapelet_net_grad(sh.default_handle().h, seq.ctypes.data, off.ctypes.data, n, q.shape[1],
                                                  t_pad, lab.ctypes.data, q.ctypes.data, len(q), head.ctypes.data,
                                                  g.ctypes.data, dq.ctypes.data, dhead.ctypes.data, loss.ctypes.data)
    return rc, g, dq, dhead, loss[0]


@pytest.mark.parametrize("name", list(nc.GRAD_CASES))
def test_gradients_equal_float64_autograd(native, sh, name):
    """The cases' values lie on a grid of 1/4, so every fp32 distance is exact (shown on the CPU) and
    the autograd sees the same d and loc.  What is left between it and the kernels:
      g     the float64 g_i, rounded once to float32: 2^-24 |g_i| (and float64 noise of exp / log
            and of the expansion form, ~1e-15 relative: 1e-12 of the largest |g| allows for it)
      dq    per element, S = sum_i |g_i * 2 (q - x_i)|: the rounding of g gives 2^-24 S; each
            product rounds once and the fp32 sum of N terms adds at most (N - 1) roundings of
            partial sums no larger than S: together below 8 N 2^-24 S
      dhead, loss   float64 sums of N <= 300 terms in a fixed order against torch's order: about
            N 2^-53 of the sum of magnitudes, far inside 1e-12 of it."""
    clips, labels, q, head, t_pad = nc.grad_case(name)
    N, m = len(clips), len(q)
    T = t_pad or max(len(x) for x in clips)
    if not t_pad:  # the autograd needs one T: zero rows behind a ragged clip add positions, so
        # compare on clips that all have the same length
        clips = [x[:m + 1] for x in clips]
        T = m + 1
        assert all(len(x) == T for x in clips)
    rc, g, dq, dhead, loss = debug_grad(native, sh, clips, labels, q, head, t_pad)
    assert rc == native.OPOSE_OK
    want = nc.autograd(q, head, clips, labels, T)
    u = 2.0 ** -24
    gerr = np.abs(g.astype(F64) - want["g"])
    print("g: worst %.3g of bound" % float(np.max(gerr / (u * np.abs(want["g"]) + 1e-12 * np.max(np.abs(want["g"]))))))
    assert np.all(gerr <= u * np.abs(want["g"]) + 1e-12 * np.max(np.abs(want["g"])))
    S = np.zeros(q.shape, F64)
    for i, x in enumerate(clips):
        win = nc.rows(x, T, F64)[want["loc"][i]:want["loc"][i] + m]
        S += np.abs(want["g"][i] * 2 * (q.astype(F64) - win))
    bound = 8 * N * u * S + u * S
    err = np.abs(dq.astype(F64) - want["dq"])
    print("dq: worst %.3g of bound" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)
    # |dz_ij| <= 1 / N, so the magnitudes of a head sum add up to at most max(1, the largest d)
    assert np.all(np.abs(dhead - want["dhead"]) <= 1e-12 * max(1.0, float(np.max(want["d"]))))
    assert abs(loss - want["loss"]) <= 1e-12 * max(abs(want["loss"]), 1.0)


# ---------------------------------------------------------------- 3. training against the goldens
@pytest.mark.parametrize("seed", nc.GOLDEN_SEEDS)
def test_training_follows_the_reference(sh, golden, seed):
    arrays, meta = golden
    atol = meta["param_atol"]
    clips, labels, q0 = nc.golden_case(seed)
    seq, off = ragged(clips)
    head0 = arrays["s%d_head0" % seed][None]
    res, hist, done = None, [], 0
    for e in nc.EPOCHS:
        if res is None:
            res = sh.shapelet_net_train(seq, off, labels, [q0], head0, epochs=e, lr=nc.LR, t_pad=nc.GOLDEN_T,
                                        loss_hist=True)
        else:
            res = sh.shapelet_net_train(seq, off, labels, None, None, state=res, epochs=e - done, lr=nc.LR,
                                        t_pad=nc.GOLDEN_T, loss_hist=True)
        done = e
        hist.append(res["loss_hist"][0])
        assert res["step"] == e
        for got, name in ((res["query"], "q"), (res["head"][0], "h")):
            diff = float(np.max(np.abs(got.astype(F64) - arrays["s%d_%s%d_f64" % (seed, name, e)])))
            print("seed %d epoch %d %s: %.3g (atol %.3g)" % (seed, e, name, diff, atol))
            assert diff <= atol
        assert np.array_equal(res["locs"][0], arrays["s%d_loc%d" % (seed, e)])
    assert np.array_equal(res["locs"][0], arrays["s%d_loc" % seed])
    assert int(res["correct"][0]) / len(labels) == 1.0 == float(arrays["s%d_score" % seed])
    hist = np.concatenate(hist)
    assert len(hist) == 200 and hist[199] < hist[0]


# ---------------------------------------------------------------- 4. the caller owns the state
def three_models(seed=0):
    clips, labels, q0 = nc.golden_case(seed)
    rng = np.random.default_rng(5)
    queries = [q0[:4].copy(), q0, rng.normal(size=(11, q0.shape[1])).astype(F32)]
    heads = np.array([[0.1, -0.2, 0.3, 0.0], [-0.4, 0.2, 0.0, 0.1], [0.05, 0.02, -0.3, 0.2]], F32)
    return clips, labels, queries, heads


def test_split_calls_equal_one_call_and_runs_repeat(sh):
    clips, labels, queries, heads = three_models()
    seq, off = ragged(clips)
    kw = dict(lr=nc.LR, t_pad=nc.GOLDEN_T, loss_hist=True)
    whole = sh.shapelet_net_train(seq, off, labels, queries, heads, epochs=7, **kw)
    again = sh.shapelet_net_train(seq, off, labels, queries, heads, epochs=7, **kw)
    same_bits(whole, again, STATE + OUTS + ("loss_hist",))
    a = sh.shapelet_net_train(seq, off, labels, queries, heads, epochs=3, **kw)
    b = sh.shapelet_net_train(seq, off, labels, None, None, state=a, epochs=4, **kw)
    assert b["step"] == 7
    same_bits(whole, b)
    assert np.array_equal(bits(np.concatenate([a["loss_hist"], b["loss_hist"]], axis=1)), bits(whole["loss_hist"]))
    assert not np.array_equal(bits(whole["query"]), bits(a["query"]))  # the steps did move it
    # the statement's seven steps land within its own rounding of the kernels' (same rule, same
    # order: the float64 exp / log of the head is all that may differ)
    s, _, _ = nc.train(nc.new_state(queries[1], heads[1]), clips, labels, 7, nc.LR, nc.GOLDEN_T)
    assert np.max(np.abs(s["query"] - whole["queries"][1])) <= 1e-6


def test_models_side_by_side_equal_models_alone(sh):
    clips, labels, queries, heads = three_models(1)
    seq, off = ragged(clips)
    kw = dict(epochs=6, lr=nc.LR, t_pad=nc.GOLDEN_T, loss_hist=True)
    together = sh.shapelet_net_train(seq, off, labels, queries, heads, **kw)
    for k, q in enumerate(queries):
        alone = sh.shapelet_net_train(seq, off, labels, [q], heads[k:k + 1], **kw)
        a, b = int(together["q_off"][k]), int(together["q_off"][k + 1])
        for key in ("query", "q_m", "q_v"):
            assert np.array_equal(bits(alone[key]), bits(together[key][a:b])), (k, key)
        for key in ("head", "head_m", "head_v", "dis", "locs", "loss", "correct", "loss_hist"):
            assert np.array_equal(bits(alone[key][0]), bits(together[key][k])), (k, key)


def test_ragged_mode_trains_too(sh):
    """t_pad = 0: positions end with each clip.  Against the statement's locations and, loosely, its
    parameters (the rule is the same; this guards the mode's plumbing)."""
    clips, labels, q0 = nc.golden_case(2)
    seq, off = ragged(clips)
    head = np.array([[0.1, -0.1, 0.0, 0.2]], F32)
    got = sh.shapelet_net_train(seq, off, labels, [q0], head, epochs=5, lr=nc.LR)
    s, _, _ = nc.train(nc.new_state(q0, head[0]), clips, labels, 5, nc.LR, 0)
    d, loc, loss, correct = nc.outputs(s, clips, labels, 0)
    assert np.array_equal(got["locs"][0], loc) and int(got["correct"][0]) == correct
    assert np.max(np.abs(got["query"] - s["query"])) <= 1e-6


# ---------------------------------------------------------------- 5. device in, device out
def test_cuda_tensors_on_another_stream(sh):
    clips, labels, queries, heads = three_models(3)
    seq, off = ragged(clips)
    kw = dict(epochs=5, lr=nc.LR, t_pad=nc.GOLDEN_T, loss_hist=True)
    want = sh.shapelet_net_train(seq, off, labels, queries, heads, **kw)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dseq = torch.from_numpy(seq).cuda(non_blocking=True)
        got = sh.shapelet_net_train(dseq, off, labels, [torch.from_numpy(q).cuda() for q in queries],
                                    torch.from_numpy(heads).cuda(), **kw)
        host = {k: got[k].cpu() for k in STATE + OUTS + ("loss_hist",)}
    stream.synchronize()
    assert all(got[k].is_cuda for k in STATE + OUTS)
    same_bits(want, host, STATE + OUTS + ("loss_hist",))


def test_device_buffers_are_untouched_past_their_ends(sh, native):
    clips, labels, queries, heads = three_models(4)
    seq, off = ragged(clips)
    epochs, n, N, pad = 4, len(queries), len(clips), 37
    want = sh.shapelet_net_train(seq, off, labels, queries, heads, epochs=epochs, lr=nc.LR, t_pad=nc.GOLDEN_T,
                                 loss_hist=True)
    q_off = np.ascontiguousarray(want["q_off"])
    lab = np.ascontiguousarray(labels, np.uint8)
    dev = torch.device("cuda")

    def roomy(a):  # the array, then `pad` sentinel elements
        a = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
        t = torch.full((a.numel() + pad,), -7, dtype=a.dtype)
        t[:a.numel()] = a
        return t.to(dev)

    qcat = np.concatenate(queries)
    st = [roomy(qcat), roomy(heads), roomy(np.zeros_like(qcat)), roomy(np.zeros_like(qcat)),
          roomy(np.zeros_like(heads)), roomy(np.zeros_like(heads))]
    outs = [roomy(np.zeros(n * N, F32)), roomy(np.zeros(n * N, np.int32)), roomy(np.zeros(n, F64)),
            roomy(np.zeros(n, np.int32)), roomy(np.zeros(n * epochs, F64))]
    dseq = torch.from_numpy(seq).to(dev)
    h = sh.default_handle()
    h.torch_call(native.lib.opose_shapelet_net_train, dseq.data_ptr(), off.ctypes.data, N, seq.shape[1], nc.GOLDEN_T,
                 lab.ctypes.data, q_off.ctypes.data, n, *[t.data_ptr() for t in st], 0, epochs, nc.LR,
                 *[t.data_ptr() for t in outs], native.DEVICE_IO)
    torch.cuda.synchronize()
    names = ("query", "head", "q_m", "q_v", "head_m", "head_v", "dis", "locs", "loss", "correct", "loss_hist")
    for name, t in zip(names, st + outs):
        t = t.cpu().numpy()
        assert np.all(t[-pad:] == -7), name
        assert np.array_equal(bits(t[:-pad]), bits(np.ascontiguousarray(want[name]).reshape(-1))), name


# ---------------------------------------------------------------- 6. refusals
def raw_args(clips, labels, queries, heads, t_pad, epochs=2):
    seq, off = ragged(clips)
    if not len(seq):
        seq = np.zeros((1, queries[0].shape[1]), F32)
    n, N = len(queries), len(clips)
    qcat = np.ascontiguousarray(np.concatenate(queries), F32)
    a = {"seq": seq, "off": off, "n_seq": N, "D": seq.shape[1], "t_pad": t_pad,
         "labels": np.ascontiguousarray(labels, np.uint8),
         "q_off": np.cumsum([0] + [len(q) for q in queries]).astype(np.int64), "n_models": n,
         "query": qcat, "head": np.ascontiguousarray(heads, F32), "q_m": np.full_like(qcat, 0.5),
         "q_v": np.full_like(qcat, 0.25), "head_m": np.full((n, 4), 0.5, F32), "head_v": np.full((n, 4), 0.25, F32),
         "step0": 3, "epochs": epochs, "lr": nc.LR,
         "dis": np.full((n, N), -7, F32), "locs": np.full((n, N), -7, np.int32), "loss": np.full(n, -7, F64),
         "correct": np.full(n, -7, np.int32), "loss_hist": np.full((n, max(epochs, 1)), -7, F64), "flags": 0}
    return a


ORDER = ("seq", "off", "n_seq", "D", "t_pad", "labels", "q_off", "n_models", "query", "head", "q_m", "q_v", "head_m",
         "head_v", "step0", "epochs", "lr", "dis", "locs", "loss", "correct", "loss_hist", "flags")
WRITTEN = ("query", "head", "q_m", "q_v", "head_m", "head_v", "dis", "locs", "loss", "correct", "loss_hist")


def raw_call(native, sh, a):
    vals = [None if a[k] is None else a[k].ctypes.data if isinstance(a[k], np.ndarray) else a[k] for k in ORDER]
    return native.lib.opose_shapelet_net_train(sh.default_handle().h, *vals)


def refusals():
    """name -> (change of the valid call's arguments, the code it must return)"""
    E_ARG, E_SHAPE = -1, -2
    big = lambda n: np.arange(n + 1, dtype=np.int64) * 7  # noqa: E731  (offsets of n clips of 7 rows)
    return {
        "null_seq": ({"seq": None}, E_ARG), "null_state": ({"q_v": None}, E_ARG), "null_out": ({"locs": None}, E_ARG),
        "lr_zero": ({"lr": 0.0}, E_ARG), "lr_negative": ({"lr": -0.01}, E_ARG), "lr_nan": ({"lr": float("nan")}, E_ARG),
        "epochs_negative": ({"epochs": -1}, E_ARG), "step0_negative": ({"step0": -1}, E_ARG),
        "no_clips": ({"n_seq": 0}, E_ARG), "no_columns": ({"D": 0}, E_ARG), "no_models": ({"n_models": 0}, E_ARG),
        "t_pad_negative": ({"t_pad": -1}, E_ARG),
        "too_many_clips": ({"n_seq": nc.MAXSEQ + 1, "off": big(nc.MAXSEQ + 1)}, E_SHAPE),
        "D_past_limit": ({"D": nc.MAXD + 1}, E_SHAPE),
        "too_many_models": ({"n_models": nc.MAXMODELS + 1, "q_off": big(nc.MAXMODELS + 1)}, E_SHAPE),
        "off_not_from_0": ({"off": "shift"}, E_ARG), "off_decreases": ({"off": "swap"}, E_ARG),
        "q_off_not_from_0": ({"q_off": "shift"}, E_ARG), "empty_query": ({"q_off": "empty"}, E_ARG),
        "m_past_limit": ({"q_off": np.array([0, nc.MAXM + 1], np.int64), "n_models": 1}, E_SHAPE),
        "label_2": ({"labels": "two"}, E_ARG),
        "clip_shorter_than_m": ({"t_pad": 0, "off": "short"}, E_SHAPE),
        "t_pad_below_a_clip": ({"t_pad": "below_clip"}, E_SHAPE), "t_pad_below_m": ({"t_pad": "below_m"}, E_SHAPE),
    }


@pytest.mark.parametrize("name", list(refusals()))
def test_refusals_return_their_code_and_touch_nothing(native, sh, name):
    clips, labels, queries, heads = three_models(5)
    a = raw_args(clips, labels, queries, heads, nc.GOLDEN_T)
    change, code = refusals()[name]
    for k, v in change.items():
        if isinstance(v, str):
            off, q_off = a["off"].copy(), a["q_off"].copy()
            m_max = int(np.max(np.diff(q_off)))
            if v == "shift":
                v = a[k] + 1
            elif v == "swap":
                off[3], off[4] = off[4] + 1, off[3]
                v = off
            elif v == "empty":
                q_off[1] = q_off[0]
                v = q_off
            elif v == "two":
                v = a["labels"].copy()
                v[-1] = 2
            elif v == "short":  # the clips keep their rows, but the first two trade some: one is below m
                off[1] = m_max - 1
                v = off
            elif v == "below_clip":
                v = int(np.max(np.diff(off))) - 1
            elif v == "below_m":  # every clip fits, the longest query does not
                a["off"] = np.arange(len(off), dtype=np.int64) * 3
                v = m_max - 1
        a[k] = v
    before = {k: a[k].copy() for k in WRITTEN if a[k] is not None}
    assert raw_call(native, sh, a) == code
    for k, v in before.items():
        assert np.array_equal(bits(a[k]), bits(v)), k


def test_valid_raw_call_passes(native, sh):
    """The arguments the refusals start from are themselves accepted (and loss_hist may be null)."""
    clips, labels, queries, heads = three_models(5)
    a = raw_args(clips, labels, queries, heads, nc.GOLDEN_T)
    a["loss_hist"] = None
    assert raw_call(native, sh, a) == native.OPOSE_OK
    assert not np.any(a["locs"] == -7) and not np.any(a["q_m"] == 0.5)
    clips, labels, q, head, t_pad = nc.grad_case("N12")
    assert debug_grad(native, sh, clips, [2] * 12, q, head, t_pad)[0] == native.OPOSE_E_ARG
    assert debug_grad(native, sh, clips, labels, np.zeros((nc.MAXM + 1, 3), F32), head, 0)[0] == native.OPOSE_E_SHAPE


# ---------------------------------------------------------------- 7. the reference's surface
def test_model_facade_on_a_golden_case(sh, golden):
    arrays, meta = golden
    seed = 0
    clips, labels, q0 = nc.golden_case(seed)
    X = nc.padded(clips, nc.GOLDEN_T)
    torch.manual_seed(seed)
    net = sh.ShapeletNetModel((len(q0), q0.shape[1]), query=torch.from_numpy(q0.T[None].copy()), lr=nc.LR)
    assert np.array_equal(net.head, arrays["s%d_head0" % seed])  # the seeded start is the reference's
    assert net.query.shape == (1, q0.shape[1], len(q0))
    net.train(X, labels, epochs=50)
    assert np.max(np.abs(net.getshapelet().astype(F64) - arrays["s%d_q50_f64" % seed])) <= meta["param_atol"]
    assert np.max(np.abs(net.head.astype(F64) - arrays["s%d_h50_f64" % seed])) <= meta["param_atol"]
    dis, loc, score = net(X, labels)
    assert np.array_equal(loc, arrays["s%d_loc50" % seed]) and 0.0 <= score <= 1.0
    loc2, dis2 = net.localizeshape(X)
    assert np.array_equal(loc2, loc) and np.array_equal(bits(dis2), bits(dis))
    # the low-level call on the padded rows, and the list form padded by the library: same bits
    seq = np.ascontiguousarray(X.transpose(0, 2, 1).reshape(-1, X.shape[1]))
    off = np.arange(len(clips) + 1, dtype=np.int64) * nc.GOLDEN_T
    low = sh.shapelet_net_train(seq, off, labels, [q0], arrays["s%d_head0" % seed][None], epochs=50, lr=nc.LR)
    assert np.array_equal(bits(low["query"]), bits(net.getshapelet())) and np.array_equal(bits(low["dis"][0]), bits(dis))
    torch.manual_seed(seed)
    net2 = sh.ShapeletNetModel((len(q0), q0.shape[1]), query=torch.from_numpy(q0.T[None].copy()), lr=nc.LR)
    net2.train([torch.from_numpy(x).cuda() for x in clips], torch.from_numpy(labels), epochs=50)
    assert np.array_equal(bits(net2.getshapelet()), bits(net.getshapelet()))
    assert len(net2.loss_hist) == 50 and net2.loss_hist[-1] < net2.loss_hist[0]


def test_net_records_start_from_the_brute_force_winners(sh):
    clips, labels, q0 = nc.golden_case(1)
    m_lens = [5, 7]
    models = sh.ShapeletMatrixModel().train_lengths(clips, labels, m_lens)
    init = {m: (mod.shapeindex, mod.cand) for m, mod in zip(m_lens, models)}
    torch.manual_seed(11)
    rec = sh.net_records(clips, labels, m_lens, init=init, epochs=20, lr=nc.LR)
    torch.manual_seed(11)
    heads = []
    for _ in m_lens:
        cls = torch.nn.Linear(1, 2)
        w, b = cls.weight.detach().numpy(), cls.bias.detach().numpy()
        heads.append([w[0, 0], w[1, 0], b[0], b[1]])
    queries = [clips[i][c:c + m] for m, (i, c) in init.items()]
    seq, off = ragged(clips)
    low = sh.shapelet_net_train(seq, off, labels, queries, np.array(heads, F32), epochs=20, lr=nc.LR,
                                t_pad=max(len(x) for x in clips))
    pos = labels != 0
    for k, m in enumerate(m_lens):
        r = rec[m]
        assert r["locs"].dtype == np.int16 and r["dists"].dtype == F32 and r["score"].dtype == F32
        assert r["shapelet"].shape == (1, q0.shape[1], m) and r["shapelet"].dtype == F32
        assert np.array_equal(r["locs"], low["locs"][k][pos]) and np.array_equal(bits(r["dists"]), bits(low["dis"][k][pos]))
        assert np.array_equal(bits(r["shapelet"][0].T), bits(low["queries"][k]))
        assert r["score"][0] == F32(int(low["correct"][k]) / len(labels))
    with pytest.raises(ValueError):  # the reference's fallback window (clip 0, start 127) does not fit
        sh.net_records(clips, labels, m_lens, epochs=1)
