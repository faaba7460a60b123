"""CPU: the Python glue of Body.batch_groups / batch_mixed / _records_groups on a stub handle and a
stub opose_body_infer_groups (as tests/test_binding_glue.py does for Body._records): the grouping
by frame size and the input order restored, the passes of at most MAX_SCALES // n_scales groups,
the capacity retry, and the pointer and geometry arrays the C call receives.

The stub call reads each frame's first pixel through the pointer and strides it was given and
answers a record whose one candidate row is (that pixel's blue value, H, W, N): a result names the
frame it was computed from."""
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
from src import _native
from src import body as body_mod
from src.body import Body
from test_binding_glue import StubHandle


class StubLib:
    """opose_body_infer_groups on host memory; rcs: the return values of the first calls (then 0)"""

    def __init__(self, body, rcs=()):
        self.body, self.rcs, self.calls = body, list(rcs), []

    def opose_body_infer_groups(self, h, n, ptrs, N, H, W, rs, fs, params, recs, flags):
        cap = self.body.handle.cap
        call = {"n": n, "cap": cap, "flags": flags, "n_scales": params.n_scales, "groups": []}
        for g in range(n):
            call["groups"].append((ptrs[g], N[g], H[g], W[g], rs[g], fs[g]))
            for i in range(N[g]):
                first = ctypes.cast(ptrs[g] + i * fs[g], ctypes.POINTER(ctypes.c_uint8))[0]
                rec = _native.encode_record([[first, H[g], W[g], N[g]]], np.zeros((0, 20)), *cap)
                ctypes.memmove(recs[g] + i * len(rec), rec.ctypes.data, len(rec))
        self.calls.append(call)
        return self.rcs.pop(0) if self.rcs else _native.OPOSE_OK


def _stub(monkeypatch, scale_search=(0.5,), rcs=(), cap=(2, 1)):
    body = object.__new__(Body)
    body.handle = StubHandle(*cap)
    body.handle.h = None
    body.peaks_per_part, body.max_people = cap
    body.params = _native.default_params(_native.NET_BODY, scale_search=scale_search)
    lib = StubLib(body, rcs)
    monkeypatch.setattr(body_mod, "lib", lib)
    return body, lib


def _frame(tag, h, w):
    f = np.zeros((h, w, 3), np.uint8)
    f[0, 0, 0] = tag
    return f


def _tags(results):
    """per result (tag, H, W, N of its group)"""
    return [tuple(int(v) for v in cand[0]) for cand, _ in results]


def test_mixed_groups_by_shape_and_restores_order(monkeypatch):
    body, lib = _stub(monkeypatch)
    sizes = [(5, 7), (4, 9), (5, 7), (6, 6), (4, 9), (5, 7), (9, 4)]
    frames = [_frame(10 + i, h, w) for i, (h, w) in enumerate(sizes)]
    res = body.batch_mixed(frames)
    counts = {s: sizes.count(s) for s in sizes}
    assert _tags(res) == [(10 + i, h, w, counts[(h, w)]) for i, (h, w) in enumerate(sizes)]
    assert all(s.shape == (0, 20) for _, s in res)
    (call,) = lib.calls
    # groups in first-appearance order of their sizes; (4, 9) and (9, 4) are different groups
    assert [(N, H, W) for _, N, H, W, _, _ in call["groups"]] == [(3, 5, 7), (2, 4, 9), (1, 6, 6), (1, 9, 4)]
    assert call["flags"] == 0


def test_mixed_equal_sizes_make_one_group(monkeypatch):
    body, lib = _stub(monkeypatch)
    res = body.batch_mixed([_frame(i, 4, 6) for i in range(5)])
    assert _tags(res) == [(i, 4, 6, 5) for i in range(5)]
    assert [c["n"] for c in lib.calls] == [1]
    assert body.batch_mixed([]) == [] and len(lib.calls) == 1


@pytest.mark.parametrize("scale_search,passes", [((0.5,), [8, 1]), ((0.5, 1.0), [4, 4, 1]),
                                                 ((0.5, 1.0, 1.5), [2, 2, 2, 2, 1]), ((1,) * 8, [1] * 9)],
                         ids=["1", "2", "3", "8"])
def test_passes_of_at_most_max_scales_segments(monkeypatch, scale_search, passes):
    body, lib = _stub(monkeypatch, scale_search)
    groups = [np.stack([_frame(20 + g, 3 + g, 5)] * (1 + g % 2)) for g in range(9)]
    res = body.batch_groups(groups)
    assert [c["n"] for c in lib.calls] == passes
    assert all(c["n"] * c["n_scales"] <= _native.MAX_SCALES and c["n_scales"] == len(scale_search) for c in lib.calls)
    assert [len(r) for r in res] == [len(g) for g in groups]
    assert [_tags(r) for r in res] == [[(20 + g, 3 + g, 5, 1 + g % 2)] * (1 + g % 2) for g in range(9)]


def test_capacity_grows_and_the_pass_is_repeated(monkeypatch):
    full = _native.OPOSE_E_CAPACITY
    # nine groups, one scale: the first pass overflows twice, the second pass once
    body, lib = _stub(monkeypatch, rcs=[full, full, _native.OPOSE_OK, full])
    groups = [_frame(g, 4, 4 + g)[None] for g in range(9)]
    res = body.batch_groups(groups)
    assert [(c["n"], c["cap"]) for c in lib.calls] == [(8, (2, 1)), (8, (4, 2)), (8, (8, 4)), (1, (8, 4)), (1, (16, 8))]
    assert body.handle.set_calls == [(4, 2), (8, 4), (16, 8)] and (body.peaks_per_part, body.max_people) == (16, 8)
    assert [_tags(r) for r in res] == [[(g, 4, 4 + g, 1)] for g in range(9)]


def test_capacity_at_the_limit_raises_and_errors_pass_through(monkeypatch):
    body, lib = _stub(monkeypatch, rcs=[_native.OPOSE_E_ARG])
    with pytest.raises(_native.OposeError) as e:
        body.batch_groups([_frame(1, 4, 4)[None]])
    assert e.value.code == _native.OPOSE_E_ARG and len(lib.calls) == 1
    # at the largest capacity the status is the frames' own: decoded (here: records that carry none)
    body, lib = _stub(monkeypatch, rcs=[_native.OPOSE_E_CAPACITY], cap=(1024, 256))
    assert _tags(body.batch_groups([_frame(1, 4, 4)[None]])[0]) == [(1, 4, 4, 1)]
    assert len(lib.calls) == 1 and not body.handle.set_calls


def test_pointer_arrays_of_the_call(monkeypatch):
    body, lib = _stub(monkeypatch)
    big = np.zeros((4, 12, 16, 3), np.uint8)
    big[:, 2, 3, 0] = [31, 32, 33, 34]  # the first pixels of the region of interest below
    dense = np.stack([_frame(41, 6, 5), _frame(42, 6, 5)])
    roi = big[1:4, 2:9, 3:11]                      # a view: passed as it is, with the buffer's strides
    listed = [_frame(51, 3, 8), _frame(52, 3, 8)]  # a list of frames: stacked
    flipped = dense[:, :, ::-1]                    # not addressable with positive strides: copied once
    res = body.batch_groups([dense, roi, listed, flipped])
    (call,) = lib.calls
    g = call["groups"]
    assert g[0] == (dense.ctypes.data, 2, 6, 5, 15, 90)
    assert g[1] == (roi.ctypes.data, 3, 7, 8, 16 * 3, 12 * 16 * 3) and roi.ctypes.data == big[1, 2, 3].ctypes.data
    assert g[2][1:] == (2, 3, 8, 24, 72)
    assert g[3][1:] == (2, 6, 5, 15, 90) and g[3][0] != dense.ctypes.data
    assert [_tags(r) for r in res] == [[(41, 6, 5, 2), (42, 6, 5, 2)], [(32, 7, 8, 3), (33, 7, 8, 3), (34, 7, 8, 3)],
                                       [(51, 3, 8, 2), (52, 3, 8, 2)], [(0, 6, 5, 2), (0, 6, 5, 2)]]
    with pytest.raises(ValueError, match=r"expected uint8 frames \[N, H, W, 3\]"):
        body.batch_groups([dense.astype(np.float32)])
    with pytest.raises(ValueError):  # a ragged group is an error, as in Body.batch
        body.batch_groups([[_frame(1, 4, 4), _frame(2, 5, 4)]])
