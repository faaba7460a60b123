"""GPU: the split-bf16 kernels' output bits, pinned.

The accuracy tests of tests/test_gpu_x6.py would pass with another summation order; these do
not.  Every case's raw fp32 output bytes are hashed (SHA-256) and compared with the digest in
tests/golden/x6_pinned.json, which scripts/gen_x6_pinned.py wrote from the library of the commit
the JSON names.  A refactor of conv_x6 / conv_win / conv_wino / conv1x1_chain keeps every digest;
a change of a kernel's arithmetic or k order regenerates the file and says so.

Each entry also carries the digest of its inputs (the seeded arrays, and for the networks the
seeded weights), asserted first: another NumPy random stream fails there, by name.

Cases: every row of test_gpu_x6.CASES with both epilogues (fp32 NCHW and the X6 split store),
three WINO_CASES rows on the window kernel (mt = -2) and on Winograd (mt = -3), and four whole
networks: the body at (2, 3, 72, 104) by default, with OPOSE_WINO=1 and with OPOSE_CONV7_WIN=0,
and the hand pyramid (48, 96, 144) of one crop -- the chain kernel, the pooled epilogues,
conv1_1 / conv1_2 and the slab fixup.  The fp32 MFMA forwards (OPOSE_CONV=f32; conv.hip has no
atomics, its stream-K fixup folds in a fixed order) are pinned too: the body at the same shape
and the hand network at (2, 3, 40, 24)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x6_pinned.json")

CONV_ROWS = [  # test_gpu_x6.CASES
    (1, 3, 40, 72, 64, 3, 0, 0, 0),
    (2, 64, 20, 24, 96, 3, 0, 0, 0),
    (2, 128, 23, 41, 128, 7, 128, 256, 0),
    (2, 128, 23, 41, 256, 7, 256, 128, 0),
    (2, 185, 17, 19, 128, 7, 128, 128, 0),
    (3, 64, 30, 33, 128, 3, 128, 64, 37),
    (2, 96, 23, 41, 128, 3, 64, 128, 300),
    (2, 128, 17, 19, 38, 1, 64, 64, 0),
    (1, 150, 9, 13, 128, 7, 64, 64, 5),
    (2, 64, 23, 41, 64, 3, 64, 128, 0),
    (3, 64, 30, 33, 64, 3, 64, 128, 40),
]
WINO_ROWS = [(2, 128, 23, 41, 256), (3, 40, 11, 13, 128), (2, 128, 9, 7, 96)]  # of test_gpu_x6.WINO_CASES
BODY_SHAPE = (2, 3, 72, 104)
HAND_SIZES = (48, 96, 144)
HAND_F32_SHAPE = (2, 3, 40, 24)  # two frames, a 5 x 3 output map: conv.hip's stream-K fixup runs


def _conv_inputs(N, Cin, H, W, Cout, ks, seed):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((N, Cin, H, W), dtype=np.float32), 0)
    w = rng.standard_normal((Cout, Cin, ks, ks), dtype=np.float32) * np.float32(np.sqrt(2 / (Cin * ks * ks)))
    b = rng.standard_normal(Cout, dtype=np.float32) * np.float32(0.1)
    return x, w, b


def _conv(native, handle, x, w, b, mt, pt, splits, out_x6):
    N, Cin, H, W = x.shape
    Cout, _, ks, _ = w.shape
    out = np.empty((N, Cout, H, W), np.float32)
    handle.check(native.lib.opose_debug_conv_x6(handle.h, x.ctypes.data, w.ctypes.data, b.ctypes.data, N, Cin, H, W,
                                                Cout, ks, ks // 2, 1, mt, pt, splits, out_x6, out.ctypes.data))
    return [out]


def _body(env):
    def run(native, handle):
        from src.model import bodypose_model
        from src.weights import seeded_state_dict
        from test_gpu_x6 import _model_outputs
        x = np.random.default_rng(10).random(BODY_SHAPE, dtype=np.float32) - np.float32(0.5)
        return [x] + list(seeded_state_dict("body", 0).values()), lambda: list(_model_outputs(bodypose_model, "body", x, env))
    return run


def _hand(native, handle):
    from src.weights import seeded_state_dict
    from test_gpu_x6 import _hand_model
    rng = np.random.default_rng(17)
    xs = [rng.random((1, 3, s, s), dtype=np.float32) - np.float32(0.5) for s in HAND_SIZES]
    return xs + list(seeded_state_dict("hand", 0).values()), lambda: list(_hand_model({}).forward_pyramid(xs))


def _hand_f32(native, handle):
    from src.model import handpose_model
    from src.weights import seeded_state_dict
    from test_gpu_x6 import _model_outputs
    x = np.random.default_rng(12).random(HAND_F32_SHAPE, dtype=np.float32) - np.float32(0.5)
    env = {"OPOSE_CONV": "f32"}
    return [x] + list(seeded_state_dict("hand", 0).values()), lambda: list(_model_outputs(handpose_model, "hand", x, env))


def _cases():
    """id -> f(native, handle) -> (input arrays, thunk giving the output arrays)"""
    out = {}
    for (N, Cin, H, W, Cout, ks, mt, pt, splits) in CONV_ROWS:
        for ox in (0, 1):
            def run(native, handle, a=(N, Cin, H, W, Cout, ks, Cin * 7 + ks), k=(mt, pt, splits, ox)):
                xwb = _conv_inputs(*a)
                return list(xwb), lambda: _conv(native, handle, *xwb, *k)
            out[f"conv-{N}x{Cin}x{H}x{W}-{Cout}-k{ks}-mt{mt}-pt{pt}-s{splits}-{'x6' if ox else 'f32'}"] = run
    for (N, Cin, H, W, Cout) in WINO_ROWS:
        for mt, fam in ((-2, "win"), (-3, "wino")):
            def run(native, handle, a=(N, Cin, H, W, Cout, 3, Cin * 3 + W), mt=mt):
                xwb = _conv_inputs(*a)
                return list(xwb), lambda: _conv(native, handle, *xwb, mt, 0, 0, 1)
            out[f"{fam}-{N}x{Cin}x{H}x{W}-{Cout}"] = run
    out["net-body"] = _body({})
    out["net-body-wino"] = _body({"OPOSE_WINO": "1"})
    out["net-body-no-conv7-win"] = _body({"OPOSE_CONV7_WIN": "0"})
    out["net-hand-pyramid"] = _hand
    out["net-body-f32"] = _body({"OPOSE_CONV": "f32"})
    out["net-hand-f32"] = _hand_f32
    return out


CASES = _cases()


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert a.dtype == np.float32
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def handle(native):
    return native.Handle(0)


@pytest.fixture(scope="module")
def pinned():
    with open(PINNED) as f:
        return json.load(f)


def test_pinned_file_covers_the_cases(pinned):
    assert sorted(pinned["cases"]) == sorted(CASES) and len(pinned["commit"]) == 40


@pytest.mark.parametrize("cid", sorted(CASES))
def test_x6_output_bits_pinned(native, handle, pinned, cid):
    want = pinned["cases"][cid]
    inputs, run = CASES[cid](native, handle)
    assert digest(inputs) == want["inputs"], "the seeded inputs changed (NumPy stream?), not the kernels"
    assert digest(run()) == want["outputs"], f"{cid}: output bits differ from commit {pinned['commit'][:7]}'s"
