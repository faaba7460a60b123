"""Fixtures of the fast mode's hand extraction (test infrastructure; runs where the reference is
checked out, like oracle/gen_golden.py, whose shims it installs).  Writes only data, under
tests/golden/:

* hand_extract_scenes.npz   the reference's `HandImageDataset` (srcmx/Batch_model.py:55-104) on
  five planted frames: motion [5,18,3], leftparams / rightparams [5,3], and the crops it returns
  (ToTensor output x 255, rounded: uint8 [5,2,b,b,3], left then right) at boxsize 64 (every crop
  enlarged) and 32 (every present crop reduced).
* hand_extract_e2e_368.npz  motion and the HandMat [5,42,3] of the reference's
  `Batch_hand_extraction` (srcmx/Batch_motion_Estimation.py:19-65) at its hard-coded boxsize 368,
  with `oracle.network.seeded_state_dict("hand", 0)` in handpose_model.  The frames are not
  stored: tests regenerate them from the seeds (oracle.glue_standins.video_frame).

The frames are glue_standins.video_frame(seed) for seeds 900-904 (300 x 400, region of interest
glue_standins.ROI = 240 x 320); the poses are the person Batch_body_extraction selects (largest
left-shoulder x, :92-105) of glue_standins.scene(seed, 240, 320).  They cover absent hands,
boxes clipped at the frame's edge, mirrored (left) and plain (right) crops.

`Batch_hand_extraction` itself runs here: the module imports under the shims, its DataLoader
collates the dataset's items on the CPU, and its module-level `batch_hand_estimation` is set to a
reference Batch_hand built as oracle.gen_golden.ref_batch_hand builds it.  Stand-ins: cv2
(oracle.cv_resize) with a VideoCapture over the planted frames, transforms.ToTensor on
oracle.batch_post.to_tensor.

Checked before anything is written: on every 368 crop, gray ones included, no part's blurred
maximum lies within 1e-3 of Batch_hand's 0.035 threshold, so a GPU's float32 summation order
cannot flip a part between found and missing.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_hand_extract_golden.py
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import batch_post, glue_standins  # noqa: E402
from oracle import gen_golden as gg  # noqa: E402
from oracle import network as onet  # noqa: E402

SEEDS = (900, 901, 902, 903, 904)
THRE, MARGIN = 0.035, 1e-3


class _ToTensor:
    def __call__(self, img):
        return batch_post.to_tensor(np.asarray(img)[None])[0]


class _Capture:
    """cv2.VideoCapture over the planted frames, whatever the path."""

    def __init__(self, path):
        self.i = 0

    def isOpened(self):
        return True

    def get(self, prop):
        assert prop == glue_standins.CAP_PROP_FRAME_COUNT
        return float(len(SEEDS))

    def read(self):
        if self.i >= len(SEEDS):
            return False, None
        self.i += 1
        return True, glue_standins.video_frame(SEEDS[self.i - 1])


def install():
    gg.install_batch_shims()
    sys.path.insert(0, gg.REF)
    cv2 = sys.modules["cv2"]
    cv2.VideoCapture = _Capture
    cv2.CAP_PROP_FRAME_COUNT = glue_standins.CAP_PROP_FRAME_COUNT
    sys.modules["torchvision.transforms"].ToTensor = _ToTensor


def selected_pose(seed):
    """Batch_body_extraction's choice of person (srcmx/Batch_motion_Estimation.py:88-107)."""
    (x0, y0), (x1, y1) = glue_standins.ROI
    candidate, subset = glue_standins.scene(seed, y1 - y0, x1 - x0)
    pose = np.zeros((18, 3))
    if len(subset) >= 1:
        lsx = np.zeros((len(subset),))
        for person in range(len(subset)):
            lsx[person] = candidate[int(subset[person][5])][0]
        best = np.argmax(lsx)
        for key in range(18):
            idx = int(subset[best][key])
            if idx != -1:
                pose[key, :] = candidate[idx][:3]
    return pose


def to_u8(t):
    return np.ascontiguousarray(np.rint(t.numpy() * 255).astype(np.uint8).transpose(1, 2, 0))


def dataset_items(BM, motion, boxsize):
    ds = BM.HandImageDataset("planted.avi", motion, glue_standins.ROI, boxsize)
    assert len(ds) == len(SEEDS)
    crops, lp, rp = [], [], []
    for i in range(len(ds)):
        left, leftparams, right, rightparams = ds[i]
        crops.append(np.stack([to_u8(left), to_u8(right)]))
        lp.append(np.asarray(leftparams, np.float64))
        rp.append(np.asarray(rightparams, np.float64))
    return np.stack(crops), np.stack(lp), np.stack(rp)


def check_margin(crops_u8, model):
    flat = crops_u8.reshape((-1,) + crops_u8.shape[2:])
    worst = np.inf
    with torch.no_grad():
        for c in flat:
            heat = model(batch_post.to_tensor(c[None]) - 0.5)
            heat = torch.nn.functional.interpolate(heat, scale_factor=8, mode="bicubic")
            peak = batch_post.blur5(heat)[0, :21].amax(dim=(1, 2)).numpy()
            worst = min(worst, float(np.abs(peak - THRE).min()))
    assert worst > MARGIN, "a part's blurred maximum is %g from the threshold: pick other seeds" % worst
    return worst


def main():
    install()
    torch.set_num_threads(8)
    import Batch_model as BM
    import Batch_motion_Estimation as BME
    from src.model import handpose_model

    motion = np.stack([selected_pose(s) for s in SEEDS])
    crops64, lp, rp = dataset_items(BM, motion, 64)
    crops32, lp32, rp32 = dataset_items(BM, motion, 32)
    assert np.array_equal(lp, lp32) and np.array_equal(rp, rp32)
    np.savez_compressed(os.path.join(gg.OUT, "hand_extract_scenes.npz"), seeds=np.array(SEEDS), motion=motion,
                        leftparams=lp, rightparams=rp, crops64=crops64, crops32=crops32)
    print("wrote hand_extract_scenes.npz; left", lp.tolist(), "right", rp.tolist())

    m = handpose_model().eval()
    sd = onet.seeded_state_dict("hand", 0)
    m.load_state_dict({k: sd[".".join(k.split(".")[1:])] for k in m.state_dict().keys()})
    crops368, _, _ = dataset_items(BM, motion, 368)
    print("threshold margin", check_margin(crops368, m))
    BME.batch_hand_estimation = gg.ref_batch_hand(m)
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        out = os.path.join(tmp, "hand.pkl")
        BME.Batch_hand_extraction("planted.avi", motion, glue_standins.ROI, out)
        import joblib
        handmat = joblib.load(out)
    assert handmat.shape == (len(SEEDS), 42, 3)
    np.savez_compressed(os.path.join(gg.OUT, "hand_extract_e2e_368.npz"), seeds=np.array(SEEDS), motion=motion,
                        handmat=handmat)
    print("wrote hand_extract_e2e_368.npz; found parts per hand",
          (handmat[:, :, 2].reshape(len(SEEDS), 2, 21) != 0).sum(2).tolist())


if __name__ == "__main__":
    main()
