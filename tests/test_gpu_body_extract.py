"""GPU: the fast mode's body extraction (`Body.poses`, `Batch_body.extract` / `extract_device`:
opose_body_records_pose / opose_batch_body_extract) and its chain into the hands
(`Batch_hand.extract_device`, `motion.Batch_motion_extraction`) against the reference's own outputs
(tests/golden/body_extract.npz, tools/gen_body_extract_golden.py: the reference's
Batch_body_extraction run with shims).

Bar: the person choice copies float64 values, so records in give the reference's rows bit for bit;
end to end x, y exact and scores within the float32 noise tests/test_gpu_batch_model.py allows
this network on this fixture (rtol 1e-3, atol 1e-6); every composition (extract = selected_pose of
the decoded records, the chain = extract then Batch_hand.extract) exact."""
import os

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

from conftest import GOLDEN
from oracle import glue_standins
from test_body_extract import CASES

pytestmark = pytest.mark.gpu

ROI = glue_standins.ROI
E_ARG, E_SHAPE, E_CAPACITY, E_ASSEMBLY = -1, -2, -5, -6
SEEDS = (900, 901, 902, 903, 904)


@pytest.fixture(scope="module")
def bb():
    from src.batch_model import Batch_body
    from src.weights import seeded_state_dict
    return Batch_body(seeded_state_dict("body", 0))


@pytest.fixture(scope="module")
def bh():
    from src.batch_model import Batch_hand
    from src.weights import seeded_state_dict
    return Batch_hand(seeded_state_dict("hand", 0))


@pytest.fixture(scope="module")
def e2e():
    d = dict(np.load(os.path.join(GOLDEN, "batch_body_e2e_23_96x128_b2.npz")))
    d["rows"] = np.load(os.path.join(GOLDEN, "body_extract.npz"))["e2e_23"]
    return d


@pytest.fixture(scope="module")
def e2e_rows(bb, e2e):
    """bb.extract of the two e2e_23 frames (shared, not modified)."""
    return bb.extract(e2e["frames"])


def _poses(body, records, device):
    """body.poses on numpy records or on a CUDA tensor of them -> numpy (pose, status)."""
    if not device:
        pose, status = body.poses(records)
        assert isinstance(pose, np.ndarray) and isinstance(status, np.ndarray)
    else:
        pose, status = body.poses(torch.from_numpy(records).cuda())
        assert pose.is_cuda and status.is_cuda
        pose, status = pose.cpu().numpy(), status.cpu().numpy()
    assert pose.dtype == np.float64 and pose.shape == (len(records), 18, 3)
    assert status.dtype == np.int32 and status.shape == (len(records),)
    return pose, status


# ---------------------------------------------------------------- 1. the kernel against the reference
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
def test_poses_of_golden_records_equal_the_reference_rows(bb, device):
    from src import _native
    # every case, then the empty scene and the candidate[-1] winner once more at other frame indices
    cases = CASES + [CASES[2], CASES[0]]
    assert len(cases) == 13 and bb.handle.record_bytes() == 89104
    records = np.stack([_native.encode_record(c, s, 128, 96) for _, c, s, _ in cases])
    pose, status = _poses(bb, records, device)
    assert not status.any()
    for (name, _, _, row), got in zip(cases, pose):
        assert np.array_equal(got, row), name
    for n, (name, _, _, row) in enumerate(cases[:11]):  # each alone
        one, st = _poses(bb, records[n:n + 1], device)
        assert st.tolist() == [0] and np.array_equal(one[0], row), name


# ---------------------------------------------------------------- 2. edge records
def _bare_body(peaks_per_part, max_people):
    """Body.poses needs the handle only: no weights."""
    from src import _native
    from src.body import Body
    body = object.__new__(Body)
    body.handle = _native.Handle(0)
    body.handle.set_capacity(peaks_per_part, max_people)  # opose_set_capacity
    return body


def _raw_record(ppp, maxp, status, n_cand, n_people, cand, subset, fill):
    """A record whose float64 body is `fill` wherever cand / subset do not reach."""
    from src import _native
    rec = np.zeros(_native.record_bytes(ppp, maxp), np.uint8)
    rec[:16].view(np.int32)[:3] = (status, n_cand, n_people)
    rec[16:].view(np.float64)[:] = fill
    rec[16:16 + 32 * len(cand)].view(np.float64)[:] = np.asarray(cand, np.float64).ravel()
    off = 16 + 32 * 18 * ppp
    rec[off:off + 160 * len(subset)].view(np.float64)[:] = np.asarray(subset, np.float64).ravel()
    return rec


def _people(rng, n_people, n_cand, shoulder_x):
    """n_people people over n_cand candidates; person p's left shoulder is candidate p, x = shoulder_x[p]."""
    cand = np.column_stack([rng.integers(0, 300, n_cand), rng.integers(0, 300, n_cand), rng.random(n_cand),
                            np.arange(n_cand)]).astype(np.float64)
    cand[:n_people, 0] = shoulder_x
    subset = rng.integers(-1, n_cand, (n_people, 20)).astype(np.float64)
    subset[:, 5] = np.arange(n_people)
    return cand, subset


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
def test_a_record_with_a_status_is_not_read(bb, device):
    recs = np.stack([_raw_record(128, 96, st, 700, 50, [], [], np.nan) for st in (E_ASSEMBLY, E_CAPACITY)])
    pose, status = _poses(bb, recs, device)
    assert status.tolist() == [E_ASSEMBLY, E_CAPACITY] and not pose.any() and not np.isnan(pose).any()


@pytest.mark.parametrize("ppp,maxp", [(128, 96), (4, 3), (16, 192)], ids=["default", "cap_4_3", "maxp_192"])
def test_full_ties_and_garbage_past_the_counts(ppp, maxp):
    """n_people == maxp with the winner last (maxp 192: lanes stride over people three times); an
    all-equal left-shoulder x (person 0 wins); 1e300 beyond n_cand / n_people never read; at the
    default and at two other capacities set through opose_set_capacity."""
    from src.pipeline import selected_pose
    body = _bare_body(ppp, maxp)
    rng = np.random.default_rng(ppp * 1000 + maxp)
    n_cand = min(18 * ppp, maxp + 40)
    assert n_cand >= maxp
    scenes = []
    scenes.append(_people(rng, maxp, n_cand, np.arange(maxp)))             # full, the winner last
    scenes.append(_people(rng, maxp, n_cand, np.full(maxp, 77.0)))         # all equal: person 0
    scenes.append(_people(rng, maxp - 1, n_cand - 1, rng.permutation(maxp - 1)))  # garbage row / candidate behind
    scenes.append(_people(rng, 2, 5, [3.0, 3.0]))                           # a tie of two, mostly garbage
    desc = np.arange(maxp)[::-1].astype(np.float64)
    desc[-1] = desc[0]                                                     # first and last tie: the first wins
    scenes.append(_people(rng, maxp, n_cand, desc))
    recs = np.stack([_raw_record(ppp, maxp, 0, len(c), len(s), c, s, 1e300) for c, s in scenes])
    want = np.stack([selected_pose(c, s) for c, s in scenes])
    assert np.array_equal(want[0][5], scenes[0][0][maxp - 1][:3]) and np.array_equal(want[1][5], scenes[1][0][0][:3])
    assert np.array_equal(want[4][5], scenes[4][0][0][:3]) and (want < 1e299).all()
    for device in (False, True):
        pose, status = _poses(body, recs, device)
        assert not status.any() and np.array_equal(pose, want)
    with pytest.raises(ValueError):  # records of another capacity
        body.poses(np.zeros((1, 89104 + 16), np.uint8))


@pytest.mark.parametrize("where", ["winner_key", "other_shoulder", "no_candidates", "negative"])
def test_an_index_past_the_candidates_fails_its_frame_only(bb, where):
    from src import _native
    from src.pipeline import selected_pose
    rng = np.random.default_rng(5)
    good = [_people(rng, 7, 30, rng.permutation(7)) for _ in range(2)]
    cand, subset = _people(rng, 7, 30, np.arange(7))
    n_cand = 30
    if where == "winner_key":
        subset[6, 11] = 30.0           # the winner's keypoint 11 names candidate[n_cand]
    elif where == "other_shoulder":
        subset[2, 5] = 1e12            # Python's IndexError comes from any person's left shoulder
    elif where == "no_candidates":
        n_cand = 0                     # candidate[-1] of an empty candidate
        subset[:, 5] = -1
    else:
        subset[6, 3] = -7.0            # Python would count from the end: not a row the reference means
    bad = _raw_record(128, 96, 0, n_cand, 7, cand, subset, 1e300)
    recs = np.stack([_native.encode_record(*good[0], 128, 96), bad, _native.encode_record(*good[1], 128, 96)])
    for device in (False, True):
        pose, status = _poses(bb, recs, device)
        assert status.tolist() == [0, E_ARG, 0] and not pose[1].any()
        assert np.array_equal(pose[0], selected_pose(*good[0])) and np.array_equal(pose[2], selected_pose(*good[1]))


# ---------------------------------------------------------------- 3. end to end
def test_extract_end_to_end_matches_reference(bb, e2e, e2e_rows):
    from src.pipeline import selected_pose
    got, ref = e2e_rows, e2e["rows"]
    assert got.shape == ref.shape == (2, 18, 3) and got.dtype == np.float64
    assert np.array_equal(got[..., :2], ref[..., :2])
    np.testing.assert_allclose(got[..., 2], ref[..., 2], rtol=1e-3, atol=1e-6)
    assert (ref[..., 2] != 0).any(axis=1).all()  # a person in both frames: not a comparison of zeros
    # the composition: the same launch sequence's records, decoded and selected on the host
    assert np.array_equal(got, np.stack([selected_pose(*r) for r in bb(e2e["frames"])]))


def test_extract_of_a_region_of_interest_and_of_device_frames(bb, e2e, e2e_rows):
    big = np.random.default_rng(1).integers(0, 256, (2, 120, 160, 3), dtype=np.uint8)
    big[:, 10:106, 20:148] = e2e["frames"]
    rec = [(20, 10), (148, 106)]
    assert np.array_equal(bb.extract(big, rec), e2e_rows)  # strided rows
    dev = torch.from_numpy(big).cuda()
    assert np.array_equal(bb.extract(dev, rec), e2e_rows)
    assert np.array_equal(bb.extract(torch.from_numpy(e2e["frames"]).cuda()), e2e_rows)
    pose, status = bb.extract_device(dev, rec)
    assert pose.is_cuda and status.is_cuda and not status.cpu().numpy().any()
    assert np.array_equal(pose.cpu().numpy(), e2e_rows)
    # a frame alone: another batch size, whose convs may sum in another order -> the end-to-end bar
    one = bb.extract(e2e["frames"][1:])
    assert np.array_equal(one[..., :2], e2e["rows"][1:, :, :2])
    np.testing.assert_allclose(one[..., 2], e2e["rows"][1:, :, 2], rtol=1e-3, atol=1e-6)


# ---------------------------------------------------------------- 4. capacity
def test_capacity_overflow_is_reported_on_the_device_and_grown_on_the_host(e2e, e2e_rows):
    from src.batch_model import Batch_body
    from src.weights import seeded_state_dict
    small = Batch_body(seeded_state_dict("body", 0), peaks_per_part=8)
    dev = torch.from_numpy(e2e["frames"]).cuda()
    pose, status = small.extract_device(dev)
    assert status.cpu().numpy().tolist() == [E_CAPACITY, E_CAPACITY] and not pose.cpu().numpy().any()
    assert small.peaks_per_part == 8  # no retry there
    assert np.array_equal(small.extract(e2e["frames"]), e2e_rows)
    assert small.peaks_per_part > 8
    assert np.array_equal(small.extract(dev), e2e_rows)


# ---------------------------------------------------------------- 5. the chain into the hands
class Capture:
    """cv2.VideoCapture over glue_standins.video_frame(900..904)."""

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


def test_motion_extraction_is_body_extract_then_hand_extract(bb, bh, tmp_path, capsys):
    import joblib
    from src.motion import Batch_motion_extraction
    full = np.stack([glue_standins.video_frame(s) for s in SEEDS])
    out = str(tmp_path / "motion.pkl")
    # one batch of five, as the compositions below: bit equality needs the same batch size
    assert Batch_motion_extraction("v.avi", out, 5, ROI, body=bb, hand=bh, capture=Capture) is None
    assert capsys.readouterr().out == "the %s file is saved\n" % out
    mat = joblib.load(out)
    assert mat.shape == (5, 60, 3) and mat.dtype == np.float64
    body_rows = bb.extract(full, ROI)
    print("chain: body keypoints per frame", (body_rows[..., 2] != 0).sum(1).tolist())
    ref = np.concatenate([body_rows, bh.extract(full, body_rows, 368, ROI)], 1)
    assert np.array_equal(mat, ref)
    dev = torch.from_numpy(full).cuda()
    pose_dev, _ = bb.extract_device(dev, ROI)
    handmat, status = bh.extract_device(dev, pose_dev, 368, ROI)
    assert handmat.is_cuda and not status.cpu().numpy().any()
    assert np.array_equal(mat, np.concatenate([pose_dev.cpu().numpy(), handmat.cpu().numpy()], 1))


def test_hand_extract_takes_device_poses(bh):
    e = np.load(os.path.join(GOLDEN, "hand_extract_e2e_368.npz"))
    full = np.stack([glue_standins.video_frame(int(s)) for s in e["seeds"]])
    dev = torch.from_numpy(full).cuda()
    want = bh.extract(dev, e["motion"], 368, ROI)  # numpy motion
    assert (want[..., 2] != 0).sum() > 100
    motion_dev = torch.from_numpy(e["motion"]).cuda()
    handmat, status = bh.extract_device(dev, motion_dev, 368, ROI)
    assert handmat.is_cuda and status.is_cuda and tuple(status.shape) == (5, 2) and not status.cpu().numpy().any()
    assert np.array_equal(handmat.cpu().numpy(), want)
    assert np.array_equal(bh.extract(dev, motion_dev, 368, ROI), want)
    assert np.array_equal(bh.extract(full, motion_dev, 368, ROI), want)  # host frames: the poses come down
    with pytest.raises(ValueError):
        bh.extract_device(dev, motion_dev[:4], 368, ROI)
    with pytest.raises(ValueError):
        bh.extract_device(dev, motion_dev.float(), 368, ROI)


def test_an_empty_hand_box_in_the_chain_raises(bh, tmp_path):
    from src.motion import Batch_motion_extraction
    motion = np.load(os.path.join(GOLDEN, "hand_extract_e2e_368.npz"))["motion"].copy()
    motion[2, 2:5] = (10.0, 10.0, 1.0)  # frame 2: right shoulder, elbow and wrist coincide

    class PlantedBody:
        """Batch_body.extract_device stand-in: the planted poses, on the device."""
        peaks_per_part, max_people = 128, 96
        handle = bh.handle

        def extract_device(self, frames_dev, recpoint=None):
            n = len(frames_dev)
            return (torch.from_numpy(motion[:n]).to(frames_dev.device),
                    torch.zeros((n,), dtype=torch.int32, device=frames_dev.device))

    out = str(tmp_path / "motion.pkl")
    with pytest.raises(ValueError, match="frame 2.*right"):
        Batch_motion_extraction("v.avi", out, 5, ROI, body=PlantedBody(), hand=bh, capture=Capture)
    assert not os.path.exists(out)
