"""CPU: the Python binding's shared call glue -- _native.frames_view (the one frames-to-strides
step), Body._records (the one capacity retry loop) and the record status mapping that
Body._decode and the video ingest share.

No compute calls: like tests/test_abi.py this needs the built library only to import _native."""
import ctypes
import types

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import as_strided

import conftest  # noqa: F401  (puts the package on sys.path)
from src import _native
from src.body import Body

RNG = np.random.default_rng(7)
BIG = RNG.integers(0, 256, (6, 9, 11, 3), dtype=np.uint8)      # buffers the views below are cut from
PLANAR = RNG.integers(0, 256, (3, 3, 5, 7), dtype=np.uint8)    # [N, 3, H, W]

# name -> (cut(buffer) -> [N, H, W, 3] view of at most [3, 5, 7, 3], buffer, copied?)
VIEWS = {
    "contiguous": (lambda a: a, np.ascontiguousarray(BIG[:3, :5, :7]), False),
    "roi": (lambda a: a[:3, 2:7, 3:10], BIG, False),
    "every_second_frame": (lambda a: a[::2, :5, :7], BIG, False),
    "newaxis_n1": (lambda a: a[None], np.ascontiguousarray(BIG[0, :5, :7]), False),
    "n1_of_roi": (lambda a: a[4:5, 1:6, 2:9], BIG, False),
    "h1": (lambda a: a[:3, 4:5, 2:9], BIG, False),
    "h1_n1_newaxes": (lambda a: a[None, None], np.ascontiguousarray(BIG[0, 0, :7]), False),
    "channels_reversed": (lambda a: a[:3, :5, :7, ::-1], BIG, True),
    "rows_reversed": (lambda a: a[:3, 4::-1, :7], BIG, True),
    "frames_reversed": (lambda a: a[2::-1, :5, :7], BIG, True),
    "every_second_pixel": (lambda a: a[:3, :5, ::2], BIG, True),
    "planar_permuted": (lambda a: a.swapaxes(1, 3).swapaxes(1, 2), PLANAR, True),  # [N,3,H,W] -> [N,H,W,3]
}


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("name", list(VIEWS))
def test_frames_view(name, kind):
    cut, buf, copied = VIEWS[name]
    buf = buf.copy()
    frames = cut(buf)
    if kind == "torch":
        try:
            frames = cut(torch.from_numpy(buf))
        except ValueError:  # torch has no negative steps: the same pixels as torch.flip lays them out, dense
            buf, cut, copied = np.ascontiguousarray(frames), (lambda a: a), False
            frames = torch.from_numpy(buf)
    want = cut(buf).copy()
    assert want.shape[0] <= 3 and want.shape[1] <= 5 and want.shape[2] <= 7
    view, ptr, N, H, W, rs, fs, on_device = _native.frames_view(frames)
    got = view if kind == "numpy" else view.numpy()
    assert (N, H, W, 3) == want.shape == got.shape and not on_device
    assert np.array_equal(got, want)
    assert ptr == got.ctypes.data and rs >= 3 * W and fs >= rs * H
    # what the library reads: N*H*W*3 bytes from ptr with these strides
    assert np.array_equal(as_strided(got, (N, H, W, 3), (fs, rs, 3, 1)), want)
    assert np.shares_memory(got, buf) == (not copied)
    if N == 1:
        assert fs == rs * H
    if H == 1:
        assert rs == 3 * W
    if not copied and N > 1 and H > 1:
        assert (fs, rs) == cut(buf).strides[:2]  # a valid view goes through as it is


@pytest.mark.parametrize("wrap", [np.asarray, torch.from_numpy], ids=["numpy", "torch"])
def test_frames_view_rejects(wrap):
    ok = np.zeros((2, 5, 7, 3), np.uint8)
    for bad in (ok.astype(np.float32), ok[0], np.zeros((2, 5, 7, 4), np.uint8), ok[:, 3:3], ok[:, :, 7:], ok[:0]):
        with pytest.raises(ValueError):
            _native.frames_view(wrap(bad))
    with pytest.raises(ValueError, match=r"expected uint8 frames \[N, H, W, 3\]"):
        _native.frames_view(wrap(ok[0]))
    with pytest.raises(ValueError, match=r"expected uint8 crops \[N, h, w, 3\]"):
        _native.frames_view(wrap(ok[0]), "crops")


# ---- Body._records on a stub handle
class StubHandle:
    def __init__(self, peaks_per_part, max_people):
        self.cap = (peaks_per_part, max_people)
        self.set_calls = []

    def record_bytes(self):
        return _native.record_bytes(*self.cap)

    def set_capacity(self, peaks_per_part, max_people):
        self.cap = (peaks_per_part, max_people)
        self.set_calls.append(self.cap)

    def check(self, rc):
        if rc != _native.OPOSE_OK:
            raise _native.OposeError(rc, "stub")


def _stub_body(peaks_per_part=2, max_people=1):
    body = object.__new__(Body)
    body.handle = StubHandle(peaks_per_part, max_people)
    body.peaks_per_part, body.max_people = peaks_per_part, max_people
    return body


CAND = np.array([[1, 2, 0.5, 0], [3, 4, 0.25, 1], [5, 6, 0.75, 2]], np.float64)
SUBSET = np.concatenate([np.arange(18.0), [1.5, 3.0]])[None]


def _writer(body, rcs, status=0, seen=None):
    """A call(rec_ptr) that fills two records of the handle's current layout and answers rcs in turn."""
    rcs = list(rcs)

    def call(ptr):
        cap = body.handle.cap
        if seen is not None:
            seen.append(cap)
        rec = _native.encode_record(CAND, SUBSET, *cap, status=status)
        for n in range(2):  # writes record_bytes() of the current capacity per frame
            ctypes.memmove(ptr + n * len(rec), rec.ctypes.data, len(rec))
        return rcs.pop(0)
    return call


def test_records_grow_and_retry():
    body, seen = _stub_body(2, 1), []
    full = _native.OPOSE_E_CAPACITY
    out = body._records(2, _writer(body, [full, full, _native.OPOSE_OK], seen=seen))
    assert seen == [(2, 1), (4, 2), (8, 4)]  # three calls, each on records of the capacity then current
    assert body.handle.set_calls == [(4, 2), (8, 4)] and (body.peaks_per_part, body.max_people) == (8, 4)
    assert len(out) == 2
    for cand, subset in out:
        assert np.array_equal(cand, CAND) and np.array_equal(subset, SUBSET)


def test_records_capacity_at_the_limit_raises():
    body, seen = _stub_body(1024, 256), []
    full = _native.OPOSE_E_CAPACITY
    with pytest.raises(RuntimeError, match=r"capacity exceeded \(peaks_per_part=1024, max_people=256\)") as e:
        body._records(2, _writer(body, [full], status=full, seen=seen))
    assert len(seen) == 1 and not body.handle.set_calls and not isinstance(e.value, _native.OposeError)


def test_records_assembly_and_argument_errors():
    body = _stub_body()
    with pytest.raises(IndexError, match="list assignment index out of range"):
        body._records(2, _writer(body, [_native.OPOSE_E_ASSEMBLY], status=_native.OPOSE_E_ASSEMBLY))
    with pytest.raises(_native.OposeError) as e:
        body._records(2, _writer(body, [_native.OPOSE_E_ARG]))
    assert e.value.code == -1


@pytest.mark.parametrize("status,exc", [(_native.OPOSE_E_ASSEMBLY, IndexError), (0, None),
                                        (_native.OPOSE_E_CAPACITY, RuntimeError), (_native.OPOSE_E_HIP, _native.OposeError)])
def test_status_mapping_is_shared_by_decode_and_ingest(status, exc):
    """Body._decode and _DeviceIngest.results raise the same exception for a record's status;
    only capacity differs on purpose: the ingest runs that frame again through Body.batch."""
    from src.motion import _DeviceIngest
    body = _stub_body(2, 1)
    rec = _native.encode_record(CAND, SUBSET[:1], 2, 1, status=status)
    ing = object.__new__(_DeviceIngest)
    ing.rec_done = [types.SimpleNamespace(synchronize=lambda: None)]
    ing.rhost = [torch.from_numpy(rec[None].copy())]
    ing.layout = [(2, 1)]
    reran = []
    ing.body = types.SimpleNamespace(batch=lambda f: reran.append(f.shape) or [("again", "again")])
    frame = np.zeros((4, 5, 3), np.uint8)

    def raised(fn):
        try:
            return fn(), None
        except Exception as e:  # compared below
            return None, e

    a, ea = raised(lambda: body._decode(rec))
    b, eb = raised(lambda: ing.results(0, [frame]))
    if status == _native.OPOSE_E_CAPACITY:
        assert isinstance(ea, RuntimeError) and eb is None and b == [("again", "again")] and reran == [(1, 4, 5, 3)]
        return
    assert not reran and type(ea) is type(eb) and str(ea) == str(eb)
    if exc is None:
        assert ea is None and np.array_equal(b[0][0], a[0]) and np.array_equal(b[0][1], a[1])
    else:
        assert type(ea) is exc
        if exc is _native.OposeError:
            assert ea.code == eb.code == status
