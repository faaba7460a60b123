"""GPU: what the C entry points answer to bad calls, and that a handle works on after an error.

* Rejections: one call per row of the table below, with the status the entry point's source gives
  it; after OPOSE_E_SHAPE / OPOSE_E_WEIGHTS the handle holds a message (opose_last_error).
* Recovery: an error thrown while the handle's stream, workspace slot, mid set, gate event or
  forced kernel family is redirected (pipelined body, per-scale streams, the conv debug hook) must
  leave the handle as it was: the next calls equal a fresh handle's, bit for bit.

No case faults the device: every error is thrown on the host before, or instead of, the launch
that would need the missing state."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_image

pytestmark = pytest.mark.gpu

H16 = W16 = 16  # frames
HL = WL = 2     # maps


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


def _body_without_weights(native):
    """A Body whose handle has no weights yet (Body.__init__ loads them)."""
    from src.body import Body
    from src.model import bodypose_model
    b = Body.__new__(Body)
    b.model = bodypose_model(0)
    b.handle = b.model.handle
    b.params = native.default_params(native.NET_BODY)
    b.peaks_per_part, b.max_people = 128, 96
    b.handle.set_capacity(128, 96)
    return b


def _hand_without_weights(native):
    from src.hand import Hand
    from src.model import handpose_model
    h = Hand.__new__(Hand)
    h.model = handpose_model(0)
    h.handle = h.model.handle
    h.params = native.default_params(native.NET_HAND)
    return h


def _load(obj, sd):
    from src import util
    obj.model.load_state_dict(util.transfer(obj.model, sd))


def _with_env(env, make):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ints(*v):
    return np.array(v, np.int32)


def _rejections(native):
    """(id, expected status, call(handle) -> status); the handle is fresh and has no weights."""
    lib, P = native.lib, native.default_params
    frame = np.zeros((1, H16, W16, 3), np.uint8)
    thin = np.zeros((1, 1000, 1, 3), np.uint8)
    maps57 = np.zeros((1, 57, HL, WL), np.float32)
    maps22 = np.zeros((1, 22, HL, WL), np.float32)
    x = np.zeros((1, 3, 16, 16), np.float32)
    out = np.zeros(1 << 17, np.uint8)     # records / peaks / maps: larger than any case writes
    found = np.zeros(64, np.int32)
    rs, fs = 3 * W16, 3 * W16 * H16
    bp, hp = P(native.NET_BODY), P(native.NET_HAND)
    no_scales, stride4 = P(native.NET_BODY), P(native.NET_BODY)
    no_scales.n_scales = 0
    stride4.stride = 4
    mp57 = (C.c_void_p * 9)(*[maps57.ctypes.data] * 9)
    mp22 = (C.c_void_p * 1)(maps22.ctypes.data)
    hl9, wl9, zero9 = _ints(*[HL] * 9), _ints(*[WL] * 9), _ints(*[0] * 9)
    pad_r = _ints(8 * WL)
    pad_d = _ints(8 * HL)
    A, S, Wt = native.OPOSE_E_ARG, native.OPOSE_E_SHAPE, native.OPOSE_E_WEIGHTS

    def infer(h, p, row_stride=rs):
        return lib.opose_body_infer(h, frame.ctypes.data, 1, H16, W16, row_stride, fs, p, out.ctypes.data, 0)
    return [
        ("body_infer-row_stride", A, lambda h: infer(h, bp, rs - 1)),
        ("body_infer-n_scales0", S, lambda h: infer(h, no_scales)),
        ("body_infer-stride4", S, lambda h: infer(h, stride4)),
        ("body_infer-no_weights", Wt, lambda h: infer(h, bp)),
        ("body_post-pad_down", A, lambda h: lib.opose_body_post(h, maps57.ctypes.data, 1, HL, WL, 8 * HL, 0, H16, W16,
                                                                bp, out.ctypes.data, 0)),
        ("body_post_scales-9", A, lambda h: lib.opose_body_post_scales(
            h, mp57, hl9.ctypes.data, wl9.ctypes.data, zero9.ctypes.data, zero9.ctypes.data, 9, 1, H16, W16, bp,
            out.ctypes.data, 0)),
        ("body_post_scales-pad_right", A, lambda h: lib.opose_body_post_scales(
            h, mp57, hl9.ctypes.data, wl9.ctypes.data, zero9.ctypes.data, pad_r.ctypes.data, 1, 1, H16, W16, bp,
            out.ctypes.data, 0)),
        ("hand_post-pad_down", S, lambda h: lib.opose_hand_post(
            h, mp22, hl9.ctypes.data, wl9.ctypes.data, pad_d.ctypes.data, zero9.ctypes.data, 1, 1, H16, W16, hp,
            out.ctypes.data, found.ctypes.data, 0)),
        ("batch_hand_infer-H12", A, lambda h: lib.opose_batch_hand_infer(
            h, frame.ctypes.data, 1, 12, W16, rs, fs, hp, out.ctypes.data, found.ctypes.data, 0)),
        ("batch_body_infer-empty", S, lambda h: lib.opose_batch_body_infer(
            h, thin.ctypes.data, 1, 1000, 1, 3, 3000, bp, out.ctypes.data, 0)),
        ("body_forward-Hp12", A, lambda h: lib.opose_body_forward(h, x.ctypes.data, 1, 12, 16, out.ctypes.data,
                                                                 out.ctypes.data, 0)),
        ("set_capacity-0", A, lambda h: lib.opose_set_capacity(h, 0, 1)),
        ("load_weights-net2", A, lambda h: lib.opose_load_weights(h, 2, mp22, hl9.ctypes.data, 1)),
        ("body_band_maps-2rows", A, lambda h: lib.opose_body_band_maps(
            h, frame.ctypes.data, H16, W16, rs, bp, 0, 0, 2, out.ctypes.data, native.HALO_FN(), None, out.ctypes.data,
            out.nbytes, 0)),
    ]


REJECTION_IDS = ["body_infer-row_stride", "body_infer-n_scales0", "body_infer-stride4", "body_infer-no_weights",
                 "body_post-pad_down", "body_post_scales-9", "body_post_scales-pad_right", "hand_post-pad_down",
                 "batch_hand_infer-H12", "batch_body_infer-empty", "body_forward-Hp12", "set_capacity-0",
                 "load_weights-net2", "body_band_maps-2rows"]


@pytest.mark.parametrize("case", REJECTION_IDS)
def test_rejection(native, case):
    name, expected, call = next(r for r in _rejections(native) if r[0] == case)
    handle = native.Handle(0)
    rc = call(handle.h)
    print(f"{name}: status {rc}, expected {expected}")
    assert rc == expected
    if expected in (native.OPOSE_E_SHAPE, native.OPOSE_E_WEIGHTS):
        assert native.lib.opose_last_error(handle.h)


def test_set_capacity_limits(native):
    """The largest capacities (1024 peaks per part, 256 people: csrc/common.h) are accepted, one
    more of either is OPOSE_E_ARG."""
    handle = native.Handle(0)
    assert native.lib.opose_set_capacity(handle.h, 1024, 256) == native.OPOSE_OK
    assert native.lib.opose_set_capacity(handle.h, 1025, 256) == native.OPOSE_E_ARG
    assert native.lib.opose_set_capacity(handle.h, 1024, 257) == native.OPOSE_E_ARG


def _same_people(got, exp):
    (c, s), (ec, es) = got, exp
    assert np.array_equal(c, ec) and np.array_equal(s, es)


def test_pipelined_body_recovers_from_missing_weights(native):
    from src.body import Body
    from src.weights import seeded_state_dict
    sd = seeded_state_dict("body", 0)
    img = golden_image(np.load(os.path.join(GOLDEN, "body_e2e_21_96x128.npz")))
    body = _body_without_weights(native)
    small = torch.zeros((1, H16, W16, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(native.OposeError) as e:
        body.infer_records(small, pipeline=True)
    assert e.value.code == native.OPOSE_E_WEIGHTS
    _load(body, sd)
    exp = Body(sd)(img)
    print(f"fresh handle: {len(exp[0])} candidates, {len(exp[1])} people")
    _same_people(body(img), exp)
    rec = body.infer_records(torch.from_numpy(img[None]).cuda(), pipeline=True)
    body.handle.flush()
    _same_people(body.decode_records(rec)[0], exp)


def test_scale_streams_recover_from_missing_weights(native):
    from src.hand import Hand
    from src.weights import seeded_state_dict
    sd = seeded_state_dict("hand", 0)
    env = {"OPOSE_LOCKSTEP": "0", "OPOSE_SCALE_STREAMS": "1"}
    hand = _with_env(env, lambda: _hand_without_weights(native))
    with pytest.raises(native.OposeError) as e:
        hand(np.zeros((H16, W16, 3), np.uint8))
    assert e.value.code == native.OPOSE_E_WEIGHTS
    _load(hand, sd)
    crop = np.random.default_rng(64).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    exp = _with_env(env, lambda: Hand(sd))(crop)
    got = hand(crop)
    assert got.dtype == exp.dtype and np.array_equal(got, exp)


def _conv_x6(native, handle, x, w, b, mt):
    N, Cin, H, W = x.shape
    Cout, _, ks, _ = w.shape
    out = np.empty((N, Cout, H, W), np.float32)
    rc = native.lib.opose_debug_conv_x6(handle.h, x.ctypes.data, w.ctypes.data, b.ctypes.data, N, Cin, H, W, Cout, ks,
                                        ks // 2, 1, mt, 0, 0, 1, out.ctypes.data)
    return rc, out


def test_debug_conv_restores_the_forced_family(native):
    rng = np.random.default_rng(7)
    x7 = rng.standard_normal((1, 8, 8, 8), dtype=np.float32)
    w7 = rng.standard_normal((128, 8, 7, 7), dtype=np.float32)
    x3 = rng.standard_normal((1, 64, 8, 8), dtype=np.float32)
    w3 = rng.standard_normal((128, 64, 3, 3), dtype=np.float32) * np.float32(0.05)
    b = rng.standard_normal(128, dtype=np.float32)
    handle, fresh = native.Handle(0), native.Handle(0)
    rc, _ = _conv_x6(native, handle, x7, w7, b, -3)  # Winograd takes 3x3 layers only
    assert rc == native.OPOSE_E_SHAPE
    rc, got = _conv_x6(native, handle, x3, w3, b, -2)
    assert rc == native.OPOSE_OK
    rc, exp = _conv_x6(native, fresh, x3, w3, b, -2)
    assert rc == native.OPOSE_OK
    assert np.abs(exp).max() > 0 and np.array_equal(got, exp)
