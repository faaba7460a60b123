"""GPU: the fast mode's hand extraction (`Batch_hand.boxes` / `crops` / `extract`:
opose_batch_hand_boxes / _crops / _extract) against the reference's own outputs
(tests/golden/hand_extract_*.npz, tools/gen_hand_extract_golden.py: HandImageDataset and
Batch_hand_extraction run with shims on the planted frames of oracle.glue_standins).

Bar: boxes and crops exact (float64 geometry and fixed-point uint8 resize have one right answer);
HandMat x, y exact, scores within the float32 noise tests/test_gpu_batch_model.py allows this
network (rtol 1e-3, atol 1e-5)."""
import os

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

from conftest import GOLDEN
from oracle import glue_standins
from oracle.hand_extract import backmap

pytestmark = pytest.mark.gpu

ROI = glue_standins.ROI
H, W = ROI[1][1] - ROI[0][1], ROI[1][0] - ROI[0][0]
E_SHAPE = -2


@pytest.fixture(scope="module")
def scenes():
    d = dict(np.load(os.path.join(GOLDEN, "hand_extract_scenes.npz")))
    d["full"] = np.stack([glue_standins.video_frame(int(s)) for s in d["seeds"]])
    d["roi"] = np.ascontiguousarray(d["full"][:, ROI[0][1]:ROI[1][1], ROI[0][0]:ROI[1][0]])
    # a side is present iff its shoulder, elbow and wrist are in the pose (left 5-7, right 2-4)
    there = d["motion"].sum(2) != 0
    d["present"] = np.stack([there[:, 5:8].all(1), there[:, 2:5].all(1)], 1)
    return d


@pytest.fixture(scope="module")
def bh():
    from src.batch_model import Batch_hand
    from src.weights import seeded_state_dict
    return Batch_hand(seeded_state_dict("hand", 0))


@pytest.fixture(scope="module")
def batch64(bh, scenes):
    """extract() of the five frames at boxsize 64 (shared, not modified)."""
    return bh.extract(scenes["full"], scenes["motion"], 64, ROI)


def _same_handmat(got, ref):
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got[..., :2], ref[..., :2])
    np.testing.assert_allclose(got[..., 2], ref[..., 2], rtol=1e-3, atol=1e-5)


def test_boxes_equal_the_reference_params(bh, scenes):
    boxes = bh.boxes(scenes["motion"], (H, W))
    assert boxes.dtype == np.int32 and boxes.shape == (5, 2, 4)
    assert np.array_equal(boxes[:, 0, :3], scenes["leftparams"]) and np.array_equal(boxes[:, 1, :3], scenes["rightparams"])
    assert np.array_equal(boxes[:, :, 3] != 0, scenes["present"])
    assert not boxes[~scenes["present"]].any()
    assert scenes["present"].sum() == 7  # absent sides and present ones both occur


@pytest.mark.parametrize("boxsize", [64, 32])
@pytest.mark.parametrize("strided", [True, False], ids=["recpoint", "contiguous"])
def test_crops_equal_the_reference_bytes(bh, scenes, boxsize, strided):
    if strided:  # row_stride = 3 * 400 != 3 * W
        crops = bh.crops(scenes["full"], scenes["motion"], boxsize, ROI)
    else:
        crops = bh.crops(scenes["roi"], scenes["motion"], boxsize)
    ref = scenes["crops%d" % boxsize]
    assert crops.dtype == np.uint8 and crops.shape == ref.shape
    assert np.array_equal(crops, ref)
    assert (crops[~scenes["present"]] == 128).all()
    if strided:  # device-resident frames: the same bytes
        assert np.array_equal(bh.crops(torch.from_numpy(scenes["full"]).cuda(), scenes["motion"], boxsize, ROI), ref)


def test_extract_is_crops_then_batch_hand_then_backmap(bh, scenes, batch64):
    crops = bh.crops(scenes["full"], scenes["motion"], 64, ROI)
    peaks = bh(crops.reshape(10, 64, 64, 3))
    ref = backmap(peaks, None, bh.boxes(scenes["motion"], (H, W)), 64)  # (every row of peaks as it is)
    print("composition: parts found per hand", (ref[..., 2] != 0).reshape(5, 2, 21).sum(2).tolist())
    assert (ref[..., 2] != 0).any()  # not a comparison of zeros
    _same_handmat(batch64, ref)


def test_extract_end_to_end_matches_reference(bh, scenes):
    e = np.load(os.path.join(GOLDEN, "hand_extract_e2e_368.npz"))
    assert np.array_equal(e["motion"], scenes["motion"])
    got = bh.extract(scenes["full"], e["motion"], 368, ROI)
    ref = e["handmat"]
    present = np.repeat(scenes["present"], 21, axis=1)  # [5, 42]
    assert got.shape == ref.shape == (5, 42, 3)
    assert np.array_equal(got[present][:, :2], ref[present][:, :2])
    assert not got[~present][:, :2].any() and not ref[~present][:, :2].any()
    np.testing.assert_allclose(got[..., 2], ref[..., 2], rtol=1e-3, atol=1e-5)
    assert (ref[present][:, 2] != 0).sum() > 100 and (ref[~present][:, 2] != 0).any()
    # device-resident frames (the region of interest a strided view of them) give the same
    dev = torch.from_numpy(scenes["full"]).cuda()
    assert np.array_equal(bh.extract(dev, e["motion"], 368, ROI), got)
    assert np.array_equal(bh.extract(dev[:, ROI[0][1]:ROI[1][1], ROI[0][0]:ROI[1][0]], e["motion"], 368), got)


def test_single_frame_equals_its_row_of_the_batch(bh, scenes, batch64):
    for n in (2, 3):  # no hand at all; both hands
        one = bh.extract(scenes["full"][n:n + 1], scenes["motion"][n:n + 1], 64, ROI)
        _same_handmat(one, batch64[n:n + 1])


def test_two_chunks_equal_one(scenes, batch64, monkeypatch):
    from src.batch_model import Batch_hand
    from src.weights import seeded_state_dict
    monkeypatch.setenv("OPOSE_EXTRACT_CHUNK", "6")  # read when the handle is created: 10 crops = 6 + 4
    chunked = Batch_hand(seeded_state_dict("hand", 0))
    _same_handmat(chunked.extract(scenes["full"], scenes["motion"], 64, ROI), batch64)
    _same_handmat(chunked.extract(scenes["roi"], scenes["motion"], 64), batch64)  # a second call reuses the buffers


def test_empty_box_is_a_shape_error_for_its_slot_only(bh, scenes, batch64):
    motion = scenes["motion"].copy()
    motion[2, 2:5] = (10.0, 10.0, 1.0)  # frame 2 (no hands): right shoulder, elbow and wrist coincide
    boxes = bh.boxes(motion, (H, W))
    assert boxes[2, 1].tolist() == [10, 10, 0, 1]
    handmat, status = bh.extract_status(scenes["full"], motion, 64, ROI)
    expect = np.zeros((5, 2), np.int32)
    expect[2, 1] = E_SHAPE
    assert np.array_equal(status, expect)
    keep = np.ones((5, 42), bool)
    keep[2, 21:] = False
    _same_handmat(handmat[keep], batch64[keep])
    with pytest.raises(ValueError, match="frame 2.*right"):
        bh.extract(scenes["full"], motion, 64, ROI)
    with pytest.raises(ValueError, match="frame 2.*right"):
        bh.crops(scenes["full"], motion, 64, ROI)
