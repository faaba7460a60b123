"""GPU: Body on groups of frames of different sizes in one lockstep pass (opose_body_infer_groups,
Body.batch_groups / batch_mixed / infer_records_groups).

What holds: a group's records are the records of `Body.batch(group)` on a handle that runs nothing
else, bit for bit, whatever runs beside the group, in whatever order -- a conv sums a pixel in an
order fixed by the layer and the group's own N x H x W (csrc/engine_plan.cpp slab_count), and the
one preprocess launch of all segments (preprocess_u8_segs) is preprocess_u8's arithmetic.

Records are compared as the C calls leave them (ctypes, not the decoded tuples): the header and
every row the header counts, byte for byte.  Rows past the counts are never written by the library
(they hold whatever the buffer held) and are not compared.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

from conftest import GOLDEN, golden_image

pytestmark = pytest.mark.gpu

RNG = np.random.default_rng(2024)


def _noise(n, h, w):
    return RNG.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _golden(name):
    return np.load(os.path.join(GOLDEN, name))


E21, E22 = _golden("body_e2e_21_96x128.npz"), _golden("body_e2e_22_120x90.npz")
# the issue's three groups: 2 x 96x128 (the golden image and its mirror), 1 x 120x90 (golden), 3 x
# 53x97 (noise); network widths 245, 138 and 337 columns at scale 0.5: none a multiple of 8
GROUPS = [np.stack([golden_image(E21), golden_image(E21)[:, ::-1]]), golden_image(E22)[None].copy(), _noise(3, 53, 97)]
assert [g.shape[:3] for g in GROUPS] == [(2, 96, 128), (1, 120, 90), (3, 53, 97)]
FIVE = GROUPS + [_noise(1, 64, 80), _noise(2, 72, 56)]
NINE = [_noise(1, h, w)[0] for h, w in [(40, 64), (48, 56), (53, 97), (56, 72), (64, 80), (72, 56), (80, 104),
                                         (96, 128), (120, 90)]]


def _sd():
    from src.weights import seeded_state_dict
    return seeded_state_dict("body", 0)


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def body():
    from src.body import Body
    return Body(_sd())


@pytest.fixture(scope="module")
def alone():
    """The reference: a Body whose handle only ever runs one group per call."""
    from src.body import Body
    return Body(_sd())


@pytest.fixture(scope="module")
def body2():
    from src.body import Body
    return Body(_sd(), scale_search=(0.5, 1.0))


@pytest.fixture(scope="module")
def alone2():
    from src.body import Body
    return Body(_sd(), scale_search=(0.5, 1.0))


# ---------------------------------------------------------------- raw calls
def infer_groups(body, groups, flags=0):
    """opose_body_infer_groups on host groups -> (rc, one uint8 [N, record_bytes] array per group)"""
    from src import _native
    views = [_native.frames_view(np.asarray(g)) for g in groups]
    n, ptrs, N, H, W, rs, fs = _native.groups_args(views)
    recs = [np.zeros((v[2], body.handle.record_bytes()), np.uint8) for v in views]
    rc = _native.lib.opose_body_infer_groups(body.handle.h, n, ptrs, N, H, W, rs, fs, body.params,
                                             (C.c_void_p * n)(*[r.ctypes.data for r in recs]), flags)
    return rc, recs


def infer_alone(body, frames):
    """opose_body_infer, the call Body.batch makes -> (rc, uint8 [N, record_bytes])"""
    from src import _native
    _, ptr, N, H, W, rs, fs, _ = _native.frames_view(np.asarray(frames))
    rec = np.zeros((N, body.handle.record_bytes()), np.uint8)
    rc = _native.lib.opose_body_infer(body.handle.h, ptr, N, H, W, rs, fs, body.params, rec.ctypes.data, 0)
    return rc, rec


def live(rec, ppp):
    """What the library wrote of one record: (status, n_cand, n_people), candidate rows, subset rows."""
    status, n_cand, n_people = (int(v) for v in rec[:16].view(np.int32)[:3])
    off = 16 + 32 * 18 * ppp
    return (status, n_cand, n_people), rec[16:16 + 32 * n_cand].tobytes(), rec[off:off + 160 * n_people].tobytes()


def assert_same_records(got, exp, ppp):
    assert got.shape == exp.shape
    for n, (a, b) in enumerate(zip(got, exp)):
        la, lb = live(a, ppp), live(b, ppp)
        assert la[0] == lb[0], (n, la[0], lb[0])
        assert la[1] == lb[1], "frame %d: candidate rows differ" % n
        assert la[2] == lb[2], "frame %d: subset rows differ" % n


def assert_groups_equal_alone(body, alone, groups, order=None):
    """Every group's records from one groups call on `body` == opose_body_infer's on `alone`."""
    order = list(range(len(groups))) if order is None else order
    rc, recs = infer_groups(body, [groups[i] for i in order])
    worst = 0
    for i, rec in zip(order, recs):
        rc1, exp = infer_alone(alone, groups[i])
        worst = min(worst, rc1)
        assert_same_records(rec, exp, body.peaks_per_part)
    assert rc == worst
    return recs


def assert_as_reference(cand, subset, d):
    """tests/test_gpu_parity.py test_body_end_to_end_vs_reference at allowance 0"""
    ref_c, ref_s = d["candidate"], d["subset"]
    assert cand.shape == ref_c.shape and np.array_equal(cand[:, :2], ref_c[:, :2])
    np.testing.assert_allclose(cand[:, 2], ref_c[:, 2], rtol=1e-3, atol=1e-4)
    assert np.array_equal(cand[:, 3], np.arange(len(cand)))
    assert subset.shape == ref_s.shape
    assert np.array_equal(subset[:, :18], ref_s[:, :18]) and np.array_equal(subset[:, 19], ref_s[:, 19])
    np.testing.assert_allclose(subset[:, 18], ref_s[:, 18], rtol=1e-3)


class CountingLib:
    """src.body's `lib` with the groups calls counted (groups per call)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "opose_body_infer_groups":
            return fn

        def counted(h, n, *args):
            self.calls.append(n)
            return fn(h, n, *args)
        return counted


# ---------------------------------------------------------------- 1. preprocess
def test_preprocess_groups_bits(native):
    handle = native.Handle(0)
    n = len(GROUPS)
    N, H, W = ((C.c_int * n)(*[g.shape[i] for g in GROUPS]) for i in range(3))
    ptrs = (C.c_void_p * n)(*[g.ctypes.data for g in GROUPS])
    hw = (C.c_int * (2 * n))()
    handle.check(native.lib.opose_debug_preprocess_groups(handle.h, n, ptrs, N, H, W, 0.5, 128, None, hw))
    assert [hw[2 * g + 1] for g in range(n)] == [248, 144, 344]  # 245, 138, 337 columns padded
    outs = [np.full((g.shape[0], 3, hw[2 * i], hw[2 * i + 1]), np.nan, np.float32) for i, g in enumerate(GROUPS)]
    handle.check(native.lib.opose_debug_preprocess_groups(handle.h, n, ptrs, N, H, W, 0.5, 128,
                                                          (C.c_void_p * n)(*[o.ctypes.data for o in outs]), hw))
    for g, out in zip(GROUPS, outs):
        for frame, got in zip(g, out):
            frame = np.ascontiguousarray(frame)
            one = (C.c_int * 2)()
            exp = np.empty(got.shape, np.float32)
            handle.check(native.lib.opose_debug_preprocess(handle.h, frame.ctypes.data, frame.shape[0], frame.shape[1],
                                                           0.5, 128, exp.ctypes.data, one))
            assert tuple(one) == got.shape[1:]
            assert np.array_equal(got, exp)
            assert (got[:, :, -1] == 0).all() and np.abs(got).max() <= 0.5  # pad columns: 128 / 256 - 0.5


# ---------------------------------------------------------------- 2, 3. records
def test_groups_equal_batch_and_reference(body, alone):
    recs = assert_groups_equal_alone(body, alone, GROUPS)
    out = [body.decode_records(r) for r in recs]
    assert_as_reference(*out[0][0], E21)
    assert_as_reference(*out[1][0], E22)
    assert len(out[0][0][0]) > 0 and len(out[0][0][1]) > 0  # peaks and people: the rows compared exist
    # the public call: the same people
    for g, res, exp in zip(GROUPS, body.batch_groups(GROUPS), out):
        assert len(res) == len(g)
        for (c, s), (ec, es) in zip(res, exp):
            assert np.array_equal(c, ec) and np.array_equal(s, es)


def test_group_order_does_not_matter(body, alone):
    assert_groups_equal_alone(body, alone, GROUPS, order=[2, 1, 0])


# ---------------------------------------------------------------- 4. multi-scale
def test_two_scales_three_groups(body2, alone2):
    assert_groups_equal_alone(body2, alone2, GROUPS)


def test_two_scales_five_groups_need_two_passes(body2, alone2, native, monkeypatch):
    rc, _ = infer_groups(body2, FIVE)  # 10 segments
    assert rc == native.OPOSE_E_ARG
    from src import body as body_mod
    counting = CountingLib(native.lib)
    monkeypatch.setattr(body_mod, "lib", counting)
    res = body2.batch_groups(FIVE)
    assert counting.calls == [4, 1]
    for g, got in zip(FIVE, res):
        exp = alone2.batch(g)
        assert len(got) == len(exp) == len(g)
        for (c, s), (ec, es) in zip(got, exp):
            assert np.array_equal(c, ec) and np.array_equal(s, es)


# ---------------------------------------------------------------- 5. nine sizes
def test_nine_sizes_mixed(body, alone, native, monkeypatch):
    from src import body as body_mod
    counting = CountingLib(native.lib)
    monkeypatch.setattr(body_mod, "lib", counting)
    order = [4, 0, 8, 2, 6, 1, 7, 3, 5]
    frames = [NINE[i] for i in order]
    res = body.batch_mixed(frames)
    assert counting.calls == [8, 1]
    assert len(res) == 9
    for f, (c, s) in zip(frames, res):
        ec, es = alone(f)
        assert np.array_equal(c, ec) and np.array_equal(s, es)


def test_mixed_groups_equal_sizes(body, alone, native, monkeypatch):
    """Frames of one size, interleaved with another: two groups, results in input order."""
    from src import body as body_mod
    counting = CountingLib(native.lib)
    monkeypatch.setattr(body_mod, "lib", counting)
    frames = [GROUPS[2][0], GROUPS[0][0], GROUPS[2][1], GROUPS[0][1], GROUPS[2][2]]
    res = body.batch_mixed(frames)
    assert counting.calls == [2]
    exp = {0: alone.batch(GROUPS[0]), 2: alone.batch(GROUPS[2])}
    for (c, s), (g, i) in zip(res, [(2, 0), (0, 0), (2, 1), (0, 1), (2, 2)]):
        assert np.array_equal(c, exp[g][i][0]) and np.array_equal(s, exp[g][i][1])


# ---------------------------------------------------------------- 6. device I/O
def test_device_records_equal_host_records(body):
    rc, host = infer_groups(body, GROUPS)
    assert rc == 0
    dev = [torch.from_numpy(g).cuda() for g in GROUPS]
    recs = body.infer_records_groups(dev)
    torch.cuda.synchronize()
    assert [tuple(r.shape) for r in recs] == [h.shape for h in host]
    for r, h in zip(recs, host):
        assert_same_records(r.cpu().numpy(), h, body.peaks_per_part)
    # into the caller's tensors, again (the launch sequence is replayed from its cache by now)
    mine = [torch.zeros_like(r) for r in recs]
    for _ in range(3):
        assert body.infer_records_groups(dev, mine) is mine
    torch.cuda.synchronize()
    for r, h in zip(mine, host):
        assert_same_records(r.cpu().numpy(), h, body.peaks_per_part)


# ---------------------------------------------------------------- 7. capacity
def test_capacity_status_and_growth(native):
    """peaks_per_part=2 at thre1=1.4.  The seeded weights' heat maps reach 1.9, and at the default
    threshold every frame here has more than 2 peaks of some part.  At 1.4 the CPU oracle
    (oracle/body_post.py find_peaks on the oracle network's maps) counts at most 12 and 14 peaks per
    part in the two 96x128 frames and 4 in the 120x90 frame, and 1, 0 and 0 in the three noise
    frames: two groups overflow, the group between them does not."""
    from src.body import Body
    kw = dict(thre1=1.4, peaks_per_part=2)
    small, ref = Body(_sd(), **kw), Body(_sd(), **kw)
    groups = [GROUPS[0], GROUPS[2], GROUPS[1]]
    full, ok = native.OPOSE_E_CAPACITY, native.OPOSE_OK
    rc, recs = infer_groups(small, groups)
    status = [[int(r[:4].view(np.int32)[0]) for r in rec] for rec in recs]
    print("per-frame status at peaks_per_part=2:", status)
    assert rc == full and status == [[full, full], [ok, ok, ok], [full]]
    # An overflowing record holds whichever 2 peaks of a part reached the list first (post.hip
    # push_peak takes slots with an atomic counter): its rows are no output and differ from call to
    # call, so they are not compared; its status and its counted candidates are.  The group between
    # the two overflowing ones is Body.batch's byte for byte.
    for rec, g, st in zip(recs, groups, status):
        rc1, exp = infer_alone(ref, g)
        assert rc1 == min(st)
        if rc1 == ok:
            assert_same_records(rec, exp, 2)
        else:
            assert [live(r, 2)[0] for r in rec] == [live(r, 2)[0] for r in exp]
    res = small.batch_groups(groups)
    assert small.peaks_per_part == 16  # 2 -> 4 -> 8 -> 16: the mirrored frame's 14 peaks fit
    grown = Body(_sd(), thre1=1.4, peaks_per_part=small.peaks_per_part, max_people=small.max_people)
    for g, got in zip(groups, res):
        exp = grown.batch(g)
        assert len(got) == len(exp) == len(g)
        for (c, s), (ec, es) in zip(got, exp):
            assert np.array_equal(c, ec) and np.array_equal(s, es)
    assert max(len(c) for got in res for c, _ in got) > 2 * 3  # rows past the first capacity came back


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors_leave_the_handle_usable(body, alone, native):
    lib, h, E = native.lib, body.handle.h, native.OPOSE_E_ARG
    views = [native.frames_view(g) for g in GROUPS]
    n, ptrs, N, H, W, rs, fs = native.groups_args(views)
    recs = [np.zeros((v[2], body.handle.record_bytes()), np.uint8) for v in views]
    rp = (C.c_void_p * n)(*[r.ctypes.data for r in recs])
    good = [n, ptrs, N, H, W, rs, fs, body.params, rp, 0]

    def call(**kw):
        names = ["n", "ptrs", "N", "H", "W", "rs", "fs", "params", "rp", "flags"]
        return lib.opose_body_infer_groups(h, *[kw.get(k, v) for k, v in zip(names, good)])

    def arr(a, i, v):
        b = type(a)(*a)
        b[i] = v
        return b

    for k in ("ptrs", "N", "H", "W", "rs", "fs", "rp"):
        assert call(**{k: None}) == E, k
    assert call(n=0) == E and call(n=-1) == E
    assert call(ptrs=arr(ptrs, 1, None)) == E and call(rp=arr(rp, 2, None)) == E
    for k, a in (("N", N), ("H", H), ("W", W)):
        assert call(**{k: arr(a, 1, 0)}) == E and call(**{k: arr(a, 2, -3)}) == E, k
    assert call(rs=arr(rs, 0, 3 * 128 - 1)) == E
    assert call(fs=arr(fs, 0, 3 * 128 * 96 - 1)) == E
    assert call(flags=native.PIPELINE) == E and call(flags=native.DEVICE_IO | native.PIPELINE_DEFER) == E
    three = native.default_params(native.NET_BODY, scale_search=(0.5, 0.75, 1.0))
    assert call(params=three) == E  # 3 groups x 3 scales
    nine = [np.zeros((1, 16, 16, 3), np.uint8)] * 9
    assert infer_groups(body, nine)[0] == E
    assert all(not r.any() for r in recs)  # nothing was written
    assert_groups_equal_alone(body, alone, GROUPS)


# ---------------------------------------------------------------- 9. other paths
def _child():
    """Run in a fresh process with the path's environment variable set from its start."""
    from src import _native
    from src.body import Body
    body, alone = Body(_sd()), Body(_sd())
    for scales in ((0.5,), (0.5, 1.0)):  # the same two handles at one scale, then at two
        body.params = alone.params = _native.default_params(_native.NET_BODY, scale_search=scales)
        recs = assert_groups_equal_alone(body, alone, GROUPS)
        assert any(live(r, body.peaks_per_part)[0][1] > 0 for rec in recs for r in rec)
    print("child ok")


@pytest.mark.parametrize("env", [{"OPOSE_LOCKSTEP": "0"}, {"OPOSE_CONV": "f32"}], ids=["no_lockstep", "f32"])
def test_other_paths_in_a_fresh_process(env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env={**os.environ, **env},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
