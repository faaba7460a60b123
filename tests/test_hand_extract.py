"""CPU: the host side of the fast mode's hand extraction against the reference's own outputs
(tests/golden/hand_extract_scenes.npz, tools/gen_hand_extract_golden.py): `util.handDetect_shape`
restates utilmx.handDetect, and `motion.Batch_hand_extraction` keeps the reference entry point's
frame-count assertion, batching, file and prints.  The device side: test_gpu_hand_extract.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import glue_standins


def test_hand_detect_shape_reproduces_reference_params():
    from src import util
    d = np.load(os.path.join(GOLDEN, "hand_extract_scenes.npz"))
    (x0, y0), (x1, y1) = glue_standins.ROI
    for pose, lp, rp in zip(d["motion"], d["leftparams"], d["rightparams"]):
        # the one-person subset HandImageDataset builds from a pose (srcmx/Batch_model.py:74-82)
        subset, candidate = np.zeros((1, 20)), np.zeros((20, 4))
        for i in range(18):
            subset[0, i] = -1 if sum(pose[i, :]) == 0 else i
            candidate[i, :2] = pose[i, :2]
        got = {bool(left): [x, y, w] for x, y, w, left in util.handDetect_shape(candidate, subset, (y1 - y0, x1 - x0))}
        assert got.get(True, [0, 0, 0]) == lp.tolist() and got.get(False, [0, 0, 0]) == rp.tolist()
        assert (True in got) == bool(lp.any()) and (False in got) == bool(rp.any())
    assert not d["leftparams"][0].any() and not d["rightparams"][2].any()  # the fixture has absent sides


class StubHand:
    def __init__(self):
        self.calls = []

    def extract(self, frames, motion, boxsize=368, recpoint=None):
        self.calls.append((frames.shape, len(motion), boxsize, recpoint))
        return np.full((len(frames), 42, 3), float(len(self.calls)))


def test_batch_hand_extraction_asserts_the_frame_count(tmp_path):
    from src.motion import Batch_hand_extraction
    hand = StubHand()
    with pytest.raises(AssertionError):  # clip_short.avi reports 7 frames
        Batch_hand_extraction("clip_short.avi", np.zeros((5, 18, 3)), glue_standins.ROI, str(tmp_path / "h.pkl"),
                              hand=hand, capture=glue_standins.FakeCapture)
    with pytest.raises(AssertionError):  # a file that does not open reports none
        Batch_hand_extraction("missing.avi", np.zeros((5, 18, 3)), glue_standins.ROI, str(tmp_path / "h.pkl"),
                              hand=hand, capture=glue_standins.FakeCapture)
    assert not hand.calls and not os.path.exists(tmp_path / "h.pkl")


def test_batch_hand_extraction_fills_handmat_batch_by_batch(tmp_path, capsys):
    import joblib
    from src.motion import Batch_hand_extraction
    hand = StubHand()
    out = str(tmp_path / "hand.pkl")
    motion = np.arange(3 * 18 * 3, dtype=np.float64).reshape(3, 18, 3)
    assert Batch_hand_extraction("clip_exact.avi", motion, glue_standins.ROI, out, hand=hand, batch=2,
                                 capture=glue_standins.FakeCapture) is None
    # whole frames go in: the region of interest is the callee's offset, at the reference's boxsize
    assert hand.calls == [((2, 300, 400, 3), 2, 368, glue_standins.ROI), ((1, 300, 400, 3), 1, 368, glue_standins.ROI)]
    mat = joblib.load(out)
    assert mat.shape == (3, 42, 3) and (mat[:2] == 1).all() and (mat[2] == 2).all()
    assert capsys.readouterr().out == "the %s file is saved\n" % out
