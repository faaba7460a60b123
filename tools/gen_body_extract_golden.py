"""Fixture of the fast mode's body extraction (test infrastructure; runs where the reference is
checked out, like tools/gen_hand_extract_golden.py, whose shims it installs).  Writes only data:
tests/golden/body_extract.npz, the MotionMat rows [T, 18, 3] the reference's own
`Batch_body_extraction` (srcmx/Batch_motion_Estimation.py:68-113) dumps, with its module-level
`Batch_Body_model` set per case:

* scenes       a stand-in returning glue_standins.scene(seed, 240, 320) for the frames
               glue_standins.video_frame(seed), seeds 900-904, cut to glue_standins.ROI (the scene
               is looked up by the cropped frame's content), batches of 2;
* clip_exact   the same stand-in over glue_standins.FakeCapture's "clip_exact.avi" (seeds 903, 900,
               904): the file tests/test_body_extract.py expects src.motion.Batch_body_extraction
               to write;
* planted_702, planted_701   the reference Batch_body on the planted maps of
               batch_body_planted_702_100x180_b2.npz / _701_240x320_b2.npz
               (oracle.gen_golden.ref_batch_body(PlantedBatch(paf, heat)));
* e2e_23       the reference Batch_body with oracle.network.seeded_state_dict("body", 0) on the two
               96 x 128 frames of batch_body_e2e_23_96x128_b2.npz.

Checked before anything is written, so a changed seed cannot silently lose a case: every row is
the selection of the (candidate, subset) the existing fixtures store; scene 900 is won through
candidate[-1] by a person without a left shoulder, 902 has no person, 903 one; e2e_23's frame 0
has 89 people and an ordinary winner (person 60, x = 123), frame 1 has 88 people whose maximum,
124, is candidate[-1][0], shared by the 20 people without a left shoulder, the first of whom
(person 68) wins; both frames fit the default record capacity.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_body_extract_golden.py
"""
from __future__ import annotations

import os
import sys
import tempfile
import zlib

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import batch_post, glue_standins  # noqa: E402
from oracle import gen_golden as gg  # noqa: E402
from oracle import network as onet  # noqa: E402

SEEDS = (900, 901, 902, 903, 904)


class _ToTensor:
    def __call__(self, img):
        return batch_post.to_tensor(np.asarray(img)[None])[0]


class _Capture:
    """cv2.VideoCapture over the frames in _Capture.frames (count: what the container reports)."""
    frames, count = (), 0

    def __init__(self, path):
        self.i = 0

    def isOpened(self):
        return True

    def get(self, prop):
        assert prop == glue_standins.CAP_PROP_FRAME_COUNT
        return float(self.count)

    def read(self):
        if self.i >= len(self.frames):
            return False, None
        self.i += 1
        return True, self.frames[self.i - 1]

    def release(self):
        pass


class _FakeCapture(glue_standins.FakeCapture):
    def release(self):
        pass


def install():
    gg.install_batch_shims()
    sys.path.insert(0, gg.REF)
    cv2 = sys.modules["cv2"]
    cv2.CAP_PROP_FRAME_COUNT = glue_standins.CAP_PROP_FRAME_COUNT
    sys.modules["torchvision.transforms"].ToTensor = _ToTensor


class SceneModel:
    """Batch_Body_model stand-in: the planted scene of every frame of the batch, by content."""

    def __init__(self):
        self.scenes = {}
        for seed in SEEDS:
            key = zlib.crc32(glue_standins.frame(seed, 240, 320).tobytes())
            self.scenes[key] = glue_standins.scene(seed, 240, 320)

    def __call__(self, batch_images):
        u8 = np.rint(batch_images.numpy() * 255).astype(np.uint8).transpose(0, 2, 3, 1)
        return [tuple(a.copy() for a in self.scenes[zlib.crc32(np.ascontiguousarray(f).tobytes())]) for f in u8]


def winner(candidate, subset):
    """(person np.argmax picks, its subset[.][5], every person's left-shoulder x) (:92-98)."""
    lsx = np.array([candidate[int(subset[p][5])][0] for p in range(len(subset))])
    best = int(np.argmax(lsx))
    return best, int(subset[best][5]), lsx


def row_of(candidate, subset):
    pose = np.zeros((18, 3))
    if len(subset) >= 1:
        best = winner(candidate, subset)[0]
        for key in range(18):
            idx = int(subset[best][key])
            if idx != -1:
                pose[key, :] = candidate[idx][:3]
    return pose


def run(BME, capture, frames, count, model, batch_size, recpoint, path="planted.avi"):
    """The reference's Batch_body_extraction over `frames` -> the MotionMat it dumps."""
    import joblib
    cv2 = sys.modules["cv2"]
    cv2.VideoCapture = capture
    _Capture.frames, _Capture.count = frames, count
    BME.Batch_Body_model = model
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        out = os.path.join(tmp, "body.pkl")
        BME.Batch_body_extraction(path, out, batch_size, recpoint)
        mat = joblib.load(out)
    assert mat.shape == (count, 18, 3) and mat.dtype == np.float64
    return mat


def main():
    install()
    torch.set_num_threads(8)
    import Batch_motion_Estimation as BME
    from src.model import bodypose_model

    out = {"seeds": np.array(SEEDS)}
    # ---- planted scenes
    scenes = [glue_standins.scene(s, 240, 320) for s in SEEDS]
    out["scenes"] = run(BME, _Capture, [glue_standins.video_frame(s) for s in SEEDS], len(SEEDS), SceneModel(), 2,
                        glue_standins.ROI)
    assert all(np.array_equal(r, row_of(*sc)) for r, sc in zip(out["scenes"], scenes))
    best, shoulder, lsx = winner(*scenes[0])
    assert shoulder == -1 and lsx[best] == scenes[0][0][-1][0] and (lsx < lsx[best]).sum() == len(lsx) - 1, \
        "scene 900 must be won through candidate[-1]"
    assert len(scenes[2][1]) == 0 and not out["scenes"][2].any(), "scene 902 must have no person"
    assert len(scenes[3][1]) == 1 and out["scenes"][3].any(), "scene 903 must have one person"
    seeds, count = glue_standins.VIDEOS["clip_exact.avi"]
    out["clip_exact"] = run(BME, _FakeCapture, (), count, SceneModel(), 2, glue_standins.ROI, "clip_exact.avi")
    assert np.array_equal(out["clip_exact"], out["scenes"][[SEEDS.index(s) for s in seeds]])

    # ---- the reference Batch_body on planted maps
    for name in ("batch_body_planted_702_100x180_b2", "batch_body_planted_701_240x320_b2"):
        d = np.load(os.path.join(gg.OUT, name + ".npz"))
        H, W = (int(v) for v in d["img_hw"])
        B = len(d["paf"])
        frames = list(np.random.default_rng(B).integers(0, 256, (B, H, W, 3), dtype=np.uint8))  # (the maps are planted)
        key = "planted_" + name.split("_")[3]
        out[key] = run(BME, _Capture, frames, B, gg.ref_batch_body(gg.PlantedBatch(d["paf"], d["heat"])), B, None)
        for i in range(B):
            assert len(d[f"subset{i}"]) >= 1 and out[key][i].any()
            assert np.array_equal(out[key][i], row_of(d[f"candidate{i}"], d[f"subset{i}"])), (key, i)

    # ---- the seeded reference network end to end
    d = np.load(os.path.join(gg.OUT, "batch_body_e2e_23_96x128_b2.npz"))
    m = bodypose_model().eval()
    sd = onet.seeded_state_dict("body", 0)
    m.load_state_dict({k: sd[".".join(k.split(".")[1:])] for k in m.state_dict().keys()})
    out["e2e_23"] = run(BME, _Capture, list(d["frames"]), 2, gg.ref_batch_body(m), 2, None)
    for i in range(2):
        c, s = d[f"candidate{i}"], d[f"subset{i}"]
        assert np.array_equal(out["e2e_23"][i], row_of(c, s)), ("e2e_23", i)
        assert len(c) <= 18 * 128 and len(s) <= 96, "e2e_23 must fit the default record capacity"
    best, shoulder, lsx = winner(d["candidate0"], d["subset0"])
    assert (len(d["subset0"]), best, shoulder != -1, lsx[best]) == (89, 60, True, 123.0), (best, shoulder, lsx[best])
    best, shoulder, lsx = winner(d["candidate1"], d["subset1"])
    absent = d["subset1"][:, 5] == -1
    assert (len(d["subset1"]), best, shoulder, lsx[best]) == (88, 68, -1, 124.0), (best, shoulder, lsx[best])
    assert d["candidate1"][-1][0] == 124.0 and absent.sum() == 20 and int(np.argmax(absent)) == 68
    assert (lsx == 124.0).sum() == 20, "the tie must be among the people without a left shoulder"
    assert len(d["candidate0"]) == 996 and len(d["candidate1"]) == 1051

    np.savez_compressed(os.path.join(gg.OUT, "body_extract.npz"), **out)
    print("wrote body_extract.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
