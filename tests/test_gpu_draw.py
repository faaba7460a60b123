"""GPU: drawing (opose_draw_records / opose_draw_motion, `Body.draw_records` / `Body.draw_motion`,
csrc/draw.hip) against the statement of tests/draw_cases.py.  Every comparison is bit equality:
the rule is integer arithmetic, float64 operations in a fixed order on table literals, and one
rint."""
import ctypes
import os

import numpy as np
import pytest
import torch  # before libopose loads: the library then shares torch's HIP runtime

import draw_cases as dc
from conftest import GOLDEN
from oracle import glue_standins

pytestmark = pytest.mark.gpu

H, W = dc.HW


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


def _debug_prims(body, src, joints, hw):
    from src import _native
    N = len(src)
    cap = 35 * body.max_people if joints == 0 else (117 if joints == 60 else 35)
    prims = np.full((N, cap, dc.PRIM_INTS), -7, np.int32)
    counts, status = np.full((N,), -7, np.int32), np.full((N,), -7, np.int32)
    src = np.ascontiguousarray(src)
    body.handle.check(_native.lib.opose_debug_draw_prims(body.handle.h, src.ctypes.data, N, joints, hw[0], hw[1],
                                                         prims.ctypes.data, counts.ctypes.data, status.ctypes.data))
    return prims, counts, status


# ---------------------------------------------------------------- 1. the setup stage
@pytest.mark.parametrize("kind", ["int", "ninths", "raw"])
def test_setup_derives_limb_parameters_as_the_statement(bb, kind):
    t = dc.limb_table(kind)
    rows = dc.limb_rows(t)
    prims, counts, status = _debug_prims(bb, rows, 18, dc.LIMB_HW)
    assert not status.any() and (counts == 35).all()
    got = prims[:, 18, 2:6]
    want = np.array([dc.limb_params(*r) for r in t], np.int32)
    bad = np.nonzero((got != want).any(1))[0]
    print("%s: %d of %d limbs differ" % (kind, len(bad), len(t)), t[bad[:5]].tolist(), got[bad[:5]].tolist(),
          want[bad[:5]].tolist())
    assert len(bad) == 0
    ref, cnt = dc.prim_table([dc.prims_of_motion(r, *dc.LIMB_HW)[0] for r in rows[::7]], 35)
    assert np.array_equal(prims[::7], ref) and (cnt == 35).all()


@pytest.mark.parametrize("joints", [18, 60])
def test_setup_tables_of_motion_rows(bb, joints):
    rows = dc.motion_rows(joints)
    prims, counts, status = _debug_prims(bb, rows, joints, dc.HW)
    ref, cnt = dc.prim_table([dc.prims_of_motion(r, H, W)[0] for r in rows], 117 if joints == 60 else 35)
    assert not status.any() and np.array_equal(counts, cnt) and np.array_equal(prims, ref)


def test_setup_tables_of_records(bb):
    from src import _native
    cases = dc.record_cases()
    recs = np.stack([_native.encode_record(c, s, bb.peaks_per_part, bb.max_people, st) for _, c, s, st, _ in cases])
    prims, counts, status = _debug_prims(bb, recs, 0, dc.HW)
    assert status.tolist() == [want for *_, want in cases]
    for n, (name, c, s, st, want) in enumerate(cases):
        ref, _ = dc.prims_of_record(c, s, H, W, st)
        assert counts[n] == len(ref), name
        if want == dc.OK:
            assert np.array_equal(prims[n, :len(ref)], ref) and not prims[n, len(ref):].any(), name


# ---------------------------------------------------------------- 2. opose_draw_motion
def _motion_want(frames, rows):
    out = [dc.draw_motion_statement(f, r) for f, r in zip(frames, rows)]
    assert all(st == dc.OK for _, st in out)
    return np.stack([c for c, _ in out])


@pytest.mark.parametrize("joints", [18, 60])
def test_draw_motion_host_and_device_in_and_out_of_place(bb, joints):
    frames, rows = dc.noise_frames(3), dc.motion_rows(joints)
    want = _motion_want(frames, rows)
    assert (want != frames).any(axis=(1, 2, 3)).all()
    # host memory, a new canvas and a given one
    got = bb.draw_motion(frames, rows)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    out = np.zeros_like(frames)
    assert bb.draw_motion(frames, rows, out=out) is out and np.array_equal(out, want)
    # in place
    work = frames.copy()
    assert bb.draw_motion(work, rows, out=work) is work and np.array_equal(work, want)
    # device memory
    fd, rd = torch.from_numpy(frames).cuda(), torch.from_numpy(rows).cuda()
    got, status = bb.draw_motion_status(fd, rd)
    assert got.is_cuda and status.is_cuda and not status.cpu().numpy().any()
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(fd.cpu().numpy(), frames)
    assert bb.draw_motion(fd, rd, out=fd) is fd and np.array_equal(fd.cpu().numpy(), want)
    # one frame
    assert np.array_equal(bb.draw_motion(frames[1], rows[1:2]), want[1])


def test_draw_motion_on_a_region_of_interest(bb):
    """A strided view of larger frames: rows and frames further apart than the view is wide, drawn
    in place (nothing outside the view changes) and into a dense canvas."""
    rows = dc.motion_rows(60)
    big = dc.noise_frames(3, (H + 9, W + 14), seed=4301)
    view = np.s_[:, 4:4 + H, 6:6 + W]
    want = _motion_want(big[view], rows)
    assert np.array_equal(bb.draw_motion(big[view], rows), want)
    for device in (False, True):
        work = torch.from_numpy(big.copy()).cuda() if device else big.copy()
        roi = work[view]
        bb.draw_motion(roi, torch.from_numpy(rows).cuda() if device else rows, out=roi)
        got = work.cpu().numpy() if device else work
        assert np.array_equal(got[view], want)
        outside = np.ones(big.shape, bool)
        outside[view] = False
        assert np.array_equal(got[outside], big[outside])


def test_draw_motion_refuses_coordinates_it_cannot_draw(bb):
    from src import _native
    frames = dc.noise_frames(3)
    rows = dc.motion_rows(60).copy()
    rows[0, 7, 1] = np.inf        # a body joint
    rows[2, 44, 0] = -16385.0     # a hand keypoint
    want1 = dc.draw_motion_statement(frames[1], rows[1])[0]
    for device in (False, True):
        f = torch.from_numpy(frames).cuda() if device else frames
        r = torch.from_numpy(rows).cuda() if device else rows
        got, status = bb.draw_motion_status(f, r)
        got, status = (got.cpu().numpy(), status.cpu().numpy()) if device else (got, status)
        assert status.tolist() == [dc.E_ARG, dc.OK, dc.E_ARG]
        assert np.array_equal(got[0], frames[0]) and np.array_equal(got[1], want1) and np.array_equal(got[2], frames[2])
    work = frames.copy()
    with pytest.raises(_native.OposeError):
        bb.draw_motion(work, rows, out=work)
    assert np.array_equal(work[[0, 2]], frames[[0, 2]]) and np.array_equal(work[1], want1)
    # arguments: joints, frame size
    st = np.zeros(3, np.int32)
    args = (frames.ctypes.data, 3, H, W, 3 * W, 3 * W * H, rows.ctypes.data)
    assert _native.lib.opose_draw_motion(bb.handle.h, *args, 42, work.ctypes.data, st.ctypes.data, 0) == dc.E_ARG
    assert _native.lib.opose_draw_motion(bb.handle.h, frames.ctypes.data, 3, H, 16385, 3 * 16385, 3 * 16385 * H,
                                         rows.ctypes.data, 60, work.ctypes.data, st.ctypes.data, 0) == dc.E_ARG


# ---------------------------------------------------------------- 3. opose_draw_records
def test_draw_records_people_statuses_and_order(bb):
    from src import _native
    cases = dc.record_cases()
    frames = dc.noise_frames(len(cases), seed=4302)
    recs = np.stack([_native.encode_record(c, s, bb.peaks_per_part, bb.max_people, st) for _, c, s, st, _ in cases])
    want = [dc.draw_records_statement(f, c, s, st) for f, (_, c, s, st, _) in zip(frames, cases)]
    want_status = [st for _, st in want]
    want = np.stack([c for c, _ in want])
    assert want_status == [w for *_, w in cases]
    assert np.array_equal(want[0], frames[0]) and all(np.array_equal(want[n], frames[n]) for n in (3, 4, 5, 6))
    for device in (False, True):
        f = torch.from_numpy(frames).cuda() if device else frames
        r = torch.from_numpy(recs).cuda() if device else recs
        got, status = bb.draw_records_status(f, r)
        got, status = (got.cpu().numpy(), status.cpu().numpy()) if device else (got, status)
        assert status.tolist() == want_status
        for n, (name, *_) in enumerate(cases):
            assert np.array_equal(got[n], want[n]), name
    # in place: the refused frames are untouched, and the worst status is the call's
    work = frames.copy()
    st = np.zeros(len(cases), np.int32)
    rc = _native.lib.opose_draw_records(bb.handle.h, work.ctypes.data, len(cases), H, W, 3 * W, 3 * W * H,
                                        recs.ctypes.data, work.ctypes.data, st.ctypes.data, 0)
    assert rc == dc.E_CAPACITY and st.tolist() == want_status and np.array_equal(work, want)
    with pytest.raises(RuntimeError, match="capacity"):
        bb.draw_records(frames[3:4], recs[3:4])
    ok = [0, 1, 2]
    assert np.array_equal(bb.draw_records(frames[ok], recs[ok]), want[ok])


def test_draw_records_reads_nothing_past_the_counts():
    """Another capacity (opose_set_capacity 4 / 3, 105 slots a frame), the record full: 1e300 wherever
    the candidates and people do not reach would be a coordinate out of range if it were read; header
    counts past the capacity are clamped to it; a record with a status is not read at all."""
    from src import _native
    from src.body import Body
    body = object.__new__(Body)  # drawing needs the handle only: no weights
    body.handle = _native.Handle(0)
    body.handle.set_capacity(4, 3)
    body.peaks_per_part, body.max_people = 4, 3
    rng = np.random.default_rng(4600)
    poses = np.zeros((3, 18, 3))
    poses[:, :, 0], poses[:, :, 1] = np.rint(rng.random((3, 18)) * W), np.rint(rng.random((3, 18)) * H)
    poses[:, :, 2] = 0.5
    full_c, full_s = dc.people_record(poses)        # 54 of 72 candidate rows, 3 of 3 people
    poses[2] = 0.0
    poses[:2, 9:] = 0.0
    part_c, part_s = dc.people_record(poses[:2])    # 18 rows, 2 people

    def raw(status, n_cand, n_people, cand, subset, fill):
        rec = np.zeros(_native.record_bytes(4, 3), np.uint8)
        rec[:16].view(np.int32)[:3] = (status, n_cand, n_people)
        rec[16:].view(np.float64)[:] = fill
        rec[16:16 + 32 * len(cand)].view(np.float64)[:] = cand.ravel()
        rec[16 + 32 * 72:16 + 32 * 72 + 160 * len(subset)].view(np.float64)[:] = subset.ravel()
        return rec

    recs = np.stack([raw(0, len(full_c), 3, full_c, full_s, 1e300), raw(0, len(part_c), 2, part_c, part_s, 1e300),
                     raw(0, 10 ** 6, 1000, full_c, full_s, 0.0), raw(dc.E_CAPACITY, 700, 50, full_c[:0], full_s[:0], np.nan)])
    frames = dc.noise_frames(4, seed=4303)
    want = np.stack([dc.draw_records_statement(frames[0], full_c, full_s)[0],
                     dc.draw_records_statement(frames[1], part_c, part_s)[0],
                     dc.draw_records_statement(frames[2], full_c, full_s)[0], frames[3]])
    for device in (False, True):
        f = torch.from_numpy(frames).cuda() if device else frames
        r = torch.from_numpy(recs).cuda() if device else recs
        got, status = body.draw_records_status(f, r)
        got, status = (got.cpu().numpy(), status.cpu().numpy()) if device else (got, status)
        assert status.tolist() == [0, 0, 0, dc.E_CAPACITY] and np.array_equal(got, want)
    with pytest.raises(ValueError):  # records of another capacity
        body.draw_records_status(frames, np.zeros((4, 89104), np.uint8))


# ---------------------------------------------------------------- 4. end to end
def test_draw_records_of_the_golden_frame(bb):
    """Body's own records of the body_e2e_21 frame, drawn where they are: the statement on the
    golden's (candidate, subset) -- x, y exact there, and a score moves no pixel."""
    from src.body import Body
    from src.weights import seeded_state_dict
    body = Body(seeded_state_dict("body", 0))
    e = np.load(os.path.join(GOLDEN, "body_e2e_21_96x128.npz"))
    want, st = dc.draw_records_statement(e["img"], e["candidate"], e["subset"])
    assert st == dc.OK and (want != e["img"]).any()
    frame = torch.from_numpy(e["img"][None]).cuda()
    first = body.draw_records(frame, body.infer_records(frame))
    assert first.is_cuda and np.array_equal(first.cpu().numpy()[0], want)
    for _ in range(2):
        again = body.draw_records(frame, body.infer_records(frame))
        assert np.array_equal(again.cpu().numpy(), first.cpu().numpy())
    assert np.array_equal(frame.cpu().numpy()[0], e["img"])


# ---------------------------------------------------------------- 5. the device chain
SEEDS = (900, 901, 902)


class Capture:
    """cv2.VideoCapture over glue_standins.video_frame(SEEDS)."""

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


def test_motion_extraction_renders_its_rows(bb, bh, tmp_path):
    import joblib
    from src.motion import Batch_motion_extraction, Checkout_motion_data, VideoFrames
    roi = glue_standins.ROI
    plain, drawn = str(tmp_path / "plain.pkl"), str(tmp_path / "drawn.pkl")
    Batch_motion_extraction("v.avi", plain, 3, roi, body=bb, hand=bh, capture=Capture)
    seen = []
    Batch_motion_extraction("v.avi", drawn, 3, roi, body=bb, hand=bh, capture=Capture,
                            render=lambda canvases: seen.append(canvases))
    mat = joblib.load(drawn)
    assert mat.shape == (3, 60, 3) and np.array_equal(mat, joblib.load(plain))
    assert len(seen) == 1 and seen[0].is_cuda and seen[0].dtype == torch.uint8
    full = np.stack([glue_standins.video_frame(s) for s in SEEDS])
    cut = full[:, roi[0][1]:roi[1][1], roi[0][0]:roi[1][0]]
    want = bb.draw_motion(cut, mat)
    got = seen[0].cpu().numpy()
    assert got.shape == cut.shape and np.array_equal(got, want) and (want != cut).any()
    assert np.array_equal(want[0], dc.draw_motion_statement(cut[0], mat[0])[0])
    # the reference's check of a run, batch by batch
    batches = list(Checkout_motion_data(VideoFrames("v.avi", capture=Capture), mat, roi, batch=2, body=bb))
    assert [len(b) for b in batches] == [2, 1] and np.array_equal(np.concatenate(batches), want)
