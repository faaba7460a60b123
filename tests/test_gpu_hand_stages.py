"""GPU: the three kernels of the fast mode's hand extraction -- hand_boxes, hand_crops, hand_backmap
(csrc/handcrop.hip) -- one at a time, each against the oracle of the same lines of the reference
(oracle/hand_extract.py), at the geometries the scene fixtures never reach: every clip and the tie of
hand_boxes, box widths 1 .. 128 on both sides at boxsize 8 and 64 with boxes flush with every frame
edge, boxsize 368's second column block, both clamps of the resize, the network-input form x, slots
whose box is empty or leaves the frame, and hand_backmap's zero branches at widths from 1 to 400.
hand_boxes runs through opose_batch_hand_boxes, the other two through opose_debug_hand_crops and
opose_debug_hand_backmap; a last test chains the three.  Also the Hand's preprocess at the source
steps of small square crops.

Every comparison is bit equality: integer boxes, bytes, float32 and float64 values in a fixed
operation order (floats are compared as their bit patterns).  The cases are in
tests/hand_stage_cases.py; tests/test_hand_stage_cases.py asserts that each reaches its branch.

The whole file (53 tests) takes 1.7 s on an MI355X."""
import numpy as np
import pytest

import hand_stage_cases as hc
from oracle import hand_extract as he

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from src import _native
    return _native


@pytest.fixture(scope="module")
def handle(native):
    return native.Handle(0)


# ------------------------------------------------------------------------------- the hooks
def gpu_boxes(native, h, motion, hw):
    motion = np.ascontiguousarray(motion, np.float64)
    out = np.full((len(motion), 2, 4), -7, np.int32)
    h.check(native.lib.opose_batch_hand_boxes(h.h, motion.ctypes.data, len(motion), hw[0], hw[1], out.ctypes.data, 0))
    return out


def gpu_crops(native, h, frames, boxes, bs, want_x=True, want_crops=True):
    """frames uint8 [N, H, W, 3] with any row stride -> (crops [N, 2, bs, bs, 3], status [N, 2],
    x [N, 2, 3, bs, bs]); an output not asked for is None."""
    N, H, W, _ = frames.shape
    assert frames.strides[2:] == (3, 1)
    boxes = np.ascontiguousarray(boxes, np.int32)
    x = np.full((N, 2, 3, bs, bs), np.nan, np.float32) if want_x else None
    crops = np.full((N, 2, bs, bs, 3), 7, np.uint8) if want_crops else None
    status = np.full((N, 2), -7, np.int32)
    h.check(native.lib.opose_debug_hand_crops(h.h, frames.ctypes.data, N, H, W, frames.strides[1], frames.strides[0],
                                              boxes.ctypes.data, bs, x.ctypes.data if want_x else None,
                                              crops.ctypes.data if want_crops else None, status.ctypes.data))
    return crops, status, x


def gpu_backmap(native, h, peaks, found, boxes, bs):
    N = len(boxes)
    peaks, found = np.ascontiguousarray(peaks, np.float64), np.ascontiguousarray(found, np.int32)
    boxes = np.ascontiguousarray(boxes, np.int32)
    out = np.full((N, 42, 3), np.nan)
    h.check(native.lib.opose_debug_hand_backmap(h.h, peaks.ctypes.data, found.ctypes.data, boxes.ctypes.data, N, bs,
                                                out.ctypes.data))
    return out


def same_bits(got, ref):
    """equal as bit patterns: -0.0 is not 0.0, a NaN is not overlooked"""
    view = {4: np.uint32, 8: np.uint64}[ref.dtype.itemsize]
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got.view(view), ref.view(view))


def _differing(got, ref, shape_of_slot):
    bad = np.flatnonzero((got != ref).reshape((-1,) + shape_of_slot).any(tuple(range(1, 1 + len(shape_of_slot)))))
    return "slots %s differ" % bad.tolist()[:12]


# ------------------------------------------------------------------------------------ boxes
@pytest.mark.parametrize("name", list(hc.BOXES))
def test_hand_boxes(native, handle, name):
    motion, hw, ref, _ = hc.box_case(name)
    got = gpu_boxes(native, handle, motion, hw)
    assert got.dtype == np.int32 and np.array_equal(got, ref), _differing(got, ref, (4,))


# ------------------------------------------------------------------------------------ crops
# set A once contiguous and once as a view with row stride 3 * 176; set B contiguous
CROP_PARAMS = [r + (s,) for r in hc.CROP_RUNS for s in ((False, True) if r[0] == "A" else (False,))]


@pytest.mark.parametrize("run", CROP_PARAMS, ids=lambda r: "%s_%s_%d_bs%d" % r[:4] + ("_stride176" if r[4] else ""))
def test_hand_crops(native, handle, run):
    group, content, which, bs, strided = run
    frames, boxes = hc.crop_input(group, content, which)
    if not strided:
        frames = np.ascontiguousarray(frames)
    assert (frames.strides[1] != 3 * frames.shape[2]) == strided
    ref_crops, ref_status, ref_x = hc.crop_case(group, content, which, bs)
    crops, status, x = gpu_crops(native, handle, frames, boxes, bs)
    assert np.array_equal(status, ref_status), (status.ravel().tolist(), ref_status.ravel().tolist())
    assert crops.dtype == np.uint8 and np.array_equal(crops, ref_crops), _differing(crops, ref_crops, (bs, bs, 3))
    if bs > 256:  # every column, the second 256-thread block's among them
        assert np.array_equal(crops[:, :, :, 256:], ref_crops[:, :, :, 256:]) and ref_crops[:, :, :, 256:].std() > 0
    assert same_bits(x, ref_x), _differing(x.view(np.uint32), ref_x.view(np.uint32), (3, bs, bs))
    # each form alone, as the product asks for them, is the same
    only_c, st_c, none_x = gpu_crops(native, handle, frames, boxes, bs, want_x=False)
    none_c, st_x, only_x = gpu_crops(native, handle, frames, boxes, bs, want_crops=False)
    assert none_x is None and none_c is None
    assert np.array_equal(only_c, ref_crops) and same_bits(only_x, ref_x)
    assert np.array_equal(st_c, ref_status) and np.array_equal(st_x, ref_status)


def test_hand_crops_hook_checks_its_arguments(native, handle):
    frames, boxes = hc.crop_input("A", "random", 0)
    frames = np.ascontiguousarray(frames[:2])
    N, H, W, _ = frames.shape
    crops = np.zeros((N, 2, 8, 8, 3), np.uint8)
    status = np.zeros((N, 2), np.int32)
    args = dict(N=N, bs=8, rs=3 * W, fs=3 * W * H)
    for change in (dict(N=0), dict(N=32768), dict(bs=0), dict(bs=12), dict(rs=3 * W - 1), dict(fs=3 * W * H - 1)):
        a = dict(args, **change)
        rc = native.lib.opose_debug_hand_crops(handle.h, frames.ctypes.data, a["N"], H, W, a["rs"], a["fs"],
                                               boxes.ctypes.data, a["bs"], None, crops.ctypes.data, status.ctypes.data)
        assert rc == native.OPOSE_E_ARG, change
    rc = native.lib.opose_debug_hand_crops(handle.h, frames.ctypes.data, N, H, W, 3 * W, 3 * W * H, boxes.ctypes.data, 8,
                                           None, None, status.ctypes.data)
    assert rc == native.OPOSE_E_ARG


# ---------------------------------------------------------------------------------- backmap
@pytest.mark.parametrize("case", hc.BACKMAP, ids=lambda c: "n%d_bs%d" % c)
def test_hand_backmap(native, handle, case):
    N, bs = case
    peaks, found, boxes = hc.backmap_case(N, bs)
    ref = he.backmap(peaks, found, boxes, bs)
    got = gpu_backmap(native, handle, peaks, found, boxes, bs)
    assert same_bits(got, ref), _differing(got.view(np.uint64), ref.view(np.uint64), (3,))


# --------------------------------------------------------------------------------- the chain
def test_boxes_crops_backmap_agree_on_slots_and_sides(native, handle):
    frames, motion, peaks, found, bs = hc.chain_case()
    hw = frames.shape[1:3]
    ref_boxes = he.boxes(motion, hw)
    ref_crops, ref_status, ref_x = he.crops(frames, ref_boxes, bs)
    ref_hm = he.backmap(peaks, found, ref_boxes, bs)
    boxes = gpu_boxes(native, handle, motion, hw)
    crops, status, x = gpu_crops(native, handle, frames, boxes, bs)
    hm = gpu_backmap(native, handle, peaks, found, boxes, bs)
    assert np.array_equal(boxes, ref_boxes)
    assert np.array_equal(crops, ref_crops) and np.array_equal(status, ref_status) and same_bits(x, ref_x)
    assert same_bits(hm, ref_hm)
    # slot 2 * frame + side in all three: the left hand's crop is the mirrored one and its rows 0-20
    # are mapped back mirrored, the right hand's rows 21-41 are not
    for n, side in ((0, 0), (0, 1), (3, 0), (5, 1)):
        bx, by, w, present = ref_boxes[n, side]
        assert present
        k = int(np.flatnonzero(found[2 * n + side] & (peaks[2 * n + side, :, 0] != 0))[0])
        px = peaks[2 * n + side, k, 0] * w / bs
        assert hm[n, 21 * side + k, 0] == (px + bx if side else w - px - 1 + bx)
    assert (crops[1, 0] == 128).all() and (crops[4, 1] == 128).all()


# -------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("case", hc.PREPROCESS, ids=lambda c: "w%d_scale%g" % c)
def test_preprocess_of_small_square_crops(native, handle, case):
    """Hand's resize + pad + normalise (src/hand.py:32-41) of a w x w crop: destination steps of
    scale * 368 / w source pixels, up to 36.8 for w = 20 and 92 for w = 8."""
    from oracle.body_post import preprocess
    w, scale = case
    img = hc.preprocess_case(w)
    hw = np.zeros(2, np.int32)
    handle.check(native.lib.opose_debug_preprocess(handle.h, img.ctypes.data, w, w, scale, 128, None, hw.ctypes.data))
    ref, _, _ = preprocess(img, scale * 368 / w)
    assert ref.shape == (1, 3, hw[0], hw[1])
    out = np.full(ref.shape[1:], np.nan, np.float32)
    handle.check(native.lib.opose_debug_preprocess(handle.h, img.ctypes.data, w, w, scale, 128, out.ctypes.data,
                                                   hw.ctypes.data))
    assert same_bits(out, np.ascontiguousarray(ref[0]))
