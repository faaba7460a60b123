"""GPU: the TGCN sign classifier (csrc/tgcn.hip through opose_tgcn_* and src/tgcn.py) against the
float64 statement and the bounds of tests/tgcn_cases.py: one layer through the debug hook at the
geometries where the kernel takes another path, dictated one-hot inputs, bit-for-bit isolation of a
sample from its neighbours, its chunk and the handle's history, the copies, the whole network on the
reference's golden logits, the device path and every refusal."""
import ctypes as C

import numpy as np
import pytest

import tgcn_cases as tc
from conftest import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    from src import _native
    h = _native.Handle(0)
    yield h
    h.close()


def build(sd, V, C_, is_resi=True, handle=None):
    from src.tgcn import GCN_muti_att
    F, H = sd["gc1.weight"].shape
    m = GCN_muti_att(F, H, C_, num_stage=tc.num_stages(sd), is_resi=is_resi, n_nodes=V, handle=handle)
    return m.load_state_dict(sd)


def golden_model(name, handle):
    sd, X, ref, meta = tc.golden_case(name)
    g = tc.GOLDEN_CASES[name]
    return build(sd, tc.GOLDEN_V, g["C"], g["is_resi"], handle), X, ref, meta


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------ one layer
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("name", list(tc.LAYER_CASES))
def test_layer_within_bound(handle, name, residual):
    sd, x, res, refs = tc.layer_case(name)
    want, bound = refs[residual]
    got = build(sd, tc.LAYER_CASES[name]["V"], 2, handle=handle).debug_layer(0, x, res if residual else None)
    diff = np.abs(got.astype(np.float64) - want)
    print("%s residual=%d: largest difference %.3g, bound there %.3g, largest difference / bound %.3g"
          % (name, residual, diff.max(), bound.flat[diff.argmax()], (diff / bound).max()))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (diff <= bound).all()


@pytest.mark.parametrize("v,k", tc.ONE_HOT_AT)
def test_one_hot_input(handle, v, k):
    """x one-hot at (v, k): the whole output is tanh(a att[:, v] x W[k, :]); a transposed operand or
    leaking padding shows as a wrong or non-zero term."""
    sd, xval = tc.one_hot_model()
    g = tc.ONE_HOT_GEOM
    x = np.zeros((2, g["V"], g["F"]), np.float32)
    x[1, v, k] = xval
    got = build(sd, g["V"], 2, handle=handle).debug_layer(0, x)
    want, tol = tc.one_hot_expected(sd, xval, v, k)
    assert not got[0].any()  # c is 0: the all-zero sample gives tanh(0)
    diff = np.abs(got[1].astype(np.float64) - want)
    print("one-hot (%d, %d): largest difference / tolerance %.3g" % (v, k, (diff / tol).max()))
    assert (diff <= tol).all()


# ------------------------------------------------------------------------------------ isolation
def test_batch_equals_single_calls_bit_for_bit(handle):
    from src.tgcn import SAMPLES_PER_WORKGROUP as G
    sd, x, res, _ = tc.layer_case("ref_55_64_64")
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((G + 1,) + x.shape[1:]).astype(np.float32)
    m = build(sd, 55, 2, handle=handle)
    whole = m.debug_layer(0, xb)
    for i in range(G + 1):
        assert np.array_equal(bits(whole[i]), bits(m.debug_layer(0, xb[i:i + 1])[0])), i
    net, X, _, _ = golden_model("g0_f16_h32_c10_s2", handle)
    Xb = np.concatenate([X, X[::-1] * np.float32(0.5)])[:G + 1, :, :16]
    all_ = net(Xb)
    for i in range(G + 1):
        assert np.array_equal(bits(all_[i]), bits(net(Xb[i:i + 1])[0])), i


def test_nan_sample_leaves_the_others_bits(handle):
    from src.tgcn import SAMPLES_PER_WORKGROUP as G
    net, X, _, _ = golden_model("g0_f16_h32_c10_s2", handle)
    Xb = np.ascontiguousarray(X[:G + 1, :, :16])
    clean = net(Xb)
    Xn = Xb.copy()
    Xn[1] = np.nan
    dirty = net(Xn)
    keep = [i for i in range(G + 1) if i != 1]
    assert np.isnan(dirty[1]).all()
    assert np.array_equal(bits(dirty[keep]), bits(clean[keep]))
    sd, x, _, _ = tc.layer_case("odd_17_50_100")
    m = build(sd, 17, 2, handle=handle)
    xn = x.copy()
    xn[0] = np.nan
    assert np.array_equal(bits(m.debug_layer(0, xn)[1:]), bits(m.debug_layer(0, x)[1:]))


def test_handle_history_does_not_leak():
    """A V = 64 model run on values of 1e30, then the V = 55 golden case on the same handle: the bits
    of a fresh handle (rows 55..63 and stale workspace values are never read)."""
    from src import _native
    name = "g0_f16_h32_c10_s2"
    fresh = _native.Handle(0)
    net, X, _, _ = golden_model(name, fresh)
    want = net.forward_copies(X, tc.GOLDEN_COPIES)
    del net
    fresh.close()
    used = _native.Handle(0)
    big = build(tc.make_model("huge_v64", 64, 16, 32, 10, 2), 64, 10, handle=used)
    big.forward_copies(np.full((6, 64, 64), 1e30, np.float32), 4)
    sd, x, _, _ = tc.layer_case("full_64_64_64")
    build(sd, 64, 2, handle=used).debug_layer(0, np.full_like(x, 1e30))
    net, X, _, _ = golden_model(name, used)
    got = net.forward_copies(X, tc.GOLDEN_COPIES)
    assert np.array_equal(bits(got), bits(want))
    del net, big
    used.close()


def test_chunks_and_runs_give_the_same_bits(handle):
    net, X, _, _ = golden_model("g1_f24_h48_c7_s1_plain", handle)
    base, base_cl = net.forward_copies(X, tc.GOLDEN_COPIES, 0, True)
    for ms in (1, 2, 0, 5, 24):
        got, cl = net.forward_copies(X, tc.GOLDEN_COPIES, ms, True)
        assert np.array_equal(bits(got), bits(base)) and np.array_equal(bits(cl), bits(base_cl)), ms


# ------------------------------------------------------------------------------------ copies
@pytest.mark.parametrize("copies", [1, 3, 4])
def test_copies(handle, copies):
    net, X, _, _ = golden_model("g0_f16_h32_c10_s2", handle)
    F = 16
    Xc = np.ascontiguousarray(X[:, :, :copies * F])
    logits, cl = net.forward_copies(Xc, copies, 0, True)
    assert cl.shape == (tc.GOLDEN_B, copies, 10)
    for i in range(copies):
        alone = net(np.ascontiguousarray(Xc[:, :, i * F:(i + 1) * F]))
        assert np.array_equal(bits(cl[:, i]), bits(alone)), i
    assert np.array_equal(bits(logits), bits(tc.ordered_mean_f32(cl)))
    assert np.array_equal(bits(net.forward_copies(Xc, copies)), bits(logits))  # without copy_logits


# ------------------------------------------------------------------------------------ whole network
@pytest.mark.parametrize("name", list(tc.GOLDEN_CASES))
def test_network_on_the_golden_cases(handle, name):
    net, X, ref, meta = golden_model(name, handle)
    want, bound, want_cl = tc.golden_ref(name)
    got, cl = net.forward_copies(X, tc.GOLDEN_COPIES, 0, True)
    diff = np.abs(got.astype(np.float64) - want)
    report("tgcn %s: device vs float64 statement, largest difference %.3g (the reference's float32: %.3g), bound "
           "there %.3g" % (name, diff.max(), meta["max_diff"], bound.flat[diff.argmax()]))
    assert (diff <= bound).all()
    assert (np.abs(got - ref) <= 2 * bound).all()
    assert np.array_equal(got.argmax(1), ref.argmax(1)) and [int(v) for v in got.argmax(1)] == meta["top1"]
    # each copy against the statement's own per-copy logits (their bound is below the mean's times copies)
    assert (np.abs(cl - want_cl) <= tc.GOLDEN_COPIES * bound[:, None, :]).all()


def test_network_v46_without_blocks(handle):
    sd, X, (want, bound, _) = tc.small_net_case()
    net = build(sd, 46, 5, handle=handle)
    got = net.forward_copies(X, 3)
    diff = np.abs(got.astype(np.float64) - want)
    print("v46 s0: largest difference %.3g, bound there %.3g" % (diff.max(), bound.flat[diff.argmax()]))
    assert (diff <= bound).all()


def test_classify_and_top_n_accuracy(handle):
    from src.tgcn import top_n_accuracy
    net, X, ref, _ = golden_model("g0_f16_h32_c10_s2", handle)
    logits, idx = net.classify(X, num_copies=4, topk=3)
    assert np.array_equal(bits(logits), bits(net.forward_copies(X, 4)))
    assert idx.shape == (tc.GOLDEN_B, 3) and np.array_equal(idx[:, 0], logits.argmax(1))
    assert np.array_equal(idx, np.argsort(-logits, axis=1, kind="stable")[:, :3])
    truths = ref.argmax(1).copy()
    truths[0] = (truths[0] + 1) % 10
    for n in (1, 3, 10):
        best = np.argsort(logits, axis=1)[:, -n:]
        want = sum(truths[i] in best[i] for i in range(len(truths))) / len(truths)
        assert top_n_accuracy(truths, logits, n) == want
    assert top_n_accuracy(truths, logits, 1) == 5 / 6 and top_n_accuracy(truths, logits, 10) == 1.0


# ------------------------------------------------------------------------------------ device path
def test_device_tensors_on_a_side_stream(handle):
    import torch
    from src import _native
    from src._native import lib
    net, X, _, _ = golden_model("g0_f16_h32_c10_s2", handle)
    want, want_cl = net.forward_copies(X, 4, 0, True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Xd = torch.from_numpy(X).cuda(non_blocking=True)
        got, cl = net.forward_copies(Xd, 4, 2, True)
        logits2, idx = net.classify(Xd, 4, 2)
        got_h, cl_h, idx_h = got.cpu(), cl.cpu(), idx.cpu()
    side.synchronize()
    assert got.is_cuda and cl.is_cuda and idx.is_cuda
    assert np.array_equal(bits(got_h.numpy()), bits(want)) and np.array_equal(bits(cl_h.numpy()), bits(want_cl))
    assert np.array_equal(idx_h.numpy()[:, 0], want.argmax(1))
    # over-allocated outputs: nothing past [B, C] / [B, copies, C] is written
    pad, nl, ncl = 64, want.size, want_cl.size
    with torch.cuda.stream(side):
        out = torch.full((nl + pad,), -7.0, device="cuda")
        ocl = torch.full((ncl + pad,), -7.0, device="cuda")
        h, m = net._device_model(0)
        h.torch_call(lib.opose_tgcn_forward, m, _native._ptr(Xd), tc.GOLDEN_B, 4, 3, _native._ptr(out), _native._ptr(ocl),
                     _native.DEVICE_IO)
        out_h, ocl_h = out.cpu().numpy(), ocl.cpu().numpy()
    side.synchronize()
    assert np.array_equal(bits(out_h[:nl]), bits(want).ravel()) and (out_h[nl:] == -7.0).all()
    assert np.array_equal(bits(ocl_h[:ncl]), bits(want_cl).ravel()) and (ocl_h[ncl:] == -7.0).all()


# ------------------------------------------------------------------------------------ refusals
def test_refusals(handle):
    from src import _native
    from src._native import OPOSE_E_ARG as ARG, OPOSE_E_SHAPE as SHAPE, lib
    V, F, H, Cn, S = 5, 3, 4, 2, 1
    sd = tc.make_model("refusals", V, F, H, Cn, S)
    net = build(sd, V, Cn, handle=handle)
    p = net._params
    n = p.size
    mp = C.c_void_p()

    def create(V=V, F=F, H=H, Cn=Cn, S=S, eps=1e-5, params=p.ctypes.data, n=n, out=C.byref(mp)):
        return lib.opose_tgcn_create(handle.h, V, F, H, Cn, S, 1, eps, params, n, out)

    assert create(params=None) == ARG and create(out=None) == ARG
    for kw in (dict(V=0), dict(F=0), dict(H=0), dict(Cn=0), dict(S=-1), dict(eps=0.0), dict(eps=-1e-5), dict(n=n - 1),
               dict(n=n + 1)):
        assert create(**kw) == ARG, kw
    for kw in (dict(V=65), dict(F=1025), dict(H=1025), dict(Cn=4097), dict(S=65)):
        assert create(**kw) == SHAPE, kw
    bad = p.copy()
    var0 = F * H + V * V + H + 3 * V * H  # the stem's running_var
    bad[var0 + 2] = -2e-5
    assert create(params=bad.ctypes.data) == ARG
    bad[var0 + 2] = np.nan
    assert create(params=bad.ctypes.data) == ARG
    assert mp.value is None  # no model was made
    assert b"running_var" in lib.opose_last_error(handle.h)

    h, m = net._device_model(0)
    x = np.zeros((2, V, 2 * F), np.float32)
    out = np.full((2, Cn), -7.0, np.float32)

    def fwd(model=m, x=x.ctypes.data, B=2, copies=2, ms=0, out=out.ctypes.data):
        return lib.opose_tgcn_forward(handle.h, model, x, B, copies, ms, out, None, 0)

    for kw in (dict(model=None), dict(x=None), dict(out=None), dict(B=0), dict(copies=0), dict(ms=-1)):
        assert fwd(**kw) == ARG, kw
    assert fwd(B=1 << 22, copies=4) == SHAPE
    assert fwd(B=1 << 24, copies=1) == SHAPE
    assert (out == -7.0).all()
    assert fwd() == _native.OPOSE_OK and np.isfinite(out).all()

    lo = np.full((1, V, H), -7.0, np.float32)
    xi = np.zeros((1, V, F), np.float32)
    dbg = lambda layer=0, x=xi.ctypes.data, B=1, m=m, o=lo.ctypes.data: lib.opose_debug_tgcn_layer(  # noqa: E731
        handle.h, m, layer, x, B, None, o)
    for kw in (dict(m=None), dict(x=None), dict(o=None), dict(layer=-1), dict(layer=3), dict(B=0)):
        assert dbg(**kw) == ARG, kw
    assert dbg(B=1 << 24) == SHAPE
    assert (lo == -7.0).all()
    assert lib.opose_tgcn_destroy(handle.h, None) == ARG and lib.opose_tgcn_destroy(None, m) == ARG
