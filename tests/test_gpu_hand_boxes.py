"""GPU: `Hand.boxes` (util.handDetect on the device for a batch of poses, shared with
`Batch_hand.boxes`) on the planted poses of the fast-mode tests
(tests/golden/hand_extract_scenes.npz): five frames, 7 hands present (4 right, 3 left; frame 1's
boxes clipped at the corner) and 3 absent.  Exact: float64 geometry has one right answer."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  before libopose loads: the library then shares torch's HIP runtime

from conftest import GOLDEN
from oracle import glue_standins

pytestmark = pytest.mark.gpu

ROI = glue_standins.ROI
H, W = ROI[1][1] - ROI[0][1], ROI[1][0] - ROI[0][0]


def test_boxes_equal_the_reference_params():
    from src import util
    from src.hand import Hand
    from src.weights import seeded_state_dict
    d = np.load(os.path.join(GOLDEN, "hand_extract_scenes.npz"))
    there = d["motion"].sum(2) != 0  # a side is present iff its shoulder, elbow and wrist are in the pose
    present = np.stack([there[:, 5:8].all(1), there[:, 2:5].all(1)], 1)
    boxes = Hand(seeded_state_dict("hand", 0)).boxes(d["motion"], (H, W))
    assert boxes.dtype == np.int32 and boxes.shape == (5, 2, 4)
    assert np.array_equal(boxes[:, 0, :3], d["leftparams"]) and np.array_equal(boxes[:, 1, :3], d["rightparams"])
    assert np.array_equal(boxes[:, :, 3] != 0, present) and not boxes[~present].any()
    assert present.sum() == 7 and present[:, 0].sum() == 3
    # the boxes util.handDetect gives Hand in src.pipeline, from the one-person subset of each pose
    for n, pose in enumerate(d["motion"]):
        subset, candidate = np.zeros((1, 20)), np.zeros((20, 4))
        for i in range(18):
            subset[0, i] = -1 if sum(pose[i, :]) == 0 else i
            candidate[i, :2] = pose[i, :2]
        host = {int(not left): [x, y, w, 1] for x, y, w, left in util.handDetect_shape(candidate, subset, (H, W))}
        assert [host.get(side, [0, 0, 0, 0]) for side in (0, 1)] == boxes[n].tolist()
