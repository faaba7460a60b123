"""CPU: the host side of the fast mode's body extraction against the reference's own outputs
(tests/golden/body_extract.npz, tools/gen_body_extract_golden.py: the reference's
Batch_body_extraction run with shims): `_native.encode_record` inverts `decode_record`,
`pipeline.selected_pose` is the person choice of srcmx/Batch_motion_Estimation.py:88-107, and
`motion.Batch_body_extraction` keeps the reference entry point's file, prints and failures.
The device side: test_gpu_body_extract.py."""
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import glue_standins

ROI = glue_standins.ROI


def golden_cases():
    """[(name, candidate, subset, the reference's MotionMat row)] of every case of the fixture."""
    g = np.load(os.path.join(GOLDEN, "body_extract.npz"))
    cases = []
    for i, seed in enumerate(g["seeds"]):
        c, s = glue_standins.scene(int(seed), 240, 320)
        cases.append(("scene_%d" % seed, c, s, g["scenes"][i]))
    for key, name in (("planted_702", "batch_body_planted_702_100x180_b2"),
                      ("planted_701", "batch_body_planted_701_240x320_b2"), ("e2e_23", "batch_body_e2e_23_96x128_b2")):
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        for i in range(len(g[key])):
            cases.append(("%s_%d" % (key, i), d["candidate%d" % i], d["subset%d" % i], g[key][i]))
    return cases


CASES = golden_cases()


def _same_record(got, status, cand, subset):
    st, c, s = got
    assert st == status
    assert c.shape == np.shape(cand) and c.dtype == np.float64 and np.array_equal(c, cand)
    assert s.shape == subset.shape and s.dtype == np.float64 and np.array_equal(s, subset)


@pytest.mark.parametrize("name,cand,subset,row", CASES, ids=[c[0] for c in CASES])
def test_encode_record_round_trips(name, cand, subset, row):
    from src import _native
    rec = _native.encode_record(cand, subset, 128, 96)
    assert rec.dtype == np.uint8 and rec.shape == (_native.record_bytes(128, 96),) == (89104,)
    _same_record(_native.decode_record(rec, 128, 96), 0, cand, subset)


def test_encode_record_small_capacity_empty_frame_and_status():
    from src import _native
    cand = np.array([[1, 2, 0.5, 0], [3, 4, 0.25, 1], [5, 6, 0.75, 2]], np.float64)
    subset = -np.ones((3, 20))
    subset[:, 5] = (2, -1, 0)
    rec = _native.encode_record(cand, subset, 4, 3, status=_native.OPOSE_E_ASSEMBLY)
    assert len(rec) == _native.record_bytes(4, 3) == 16 + 32 * 18 * 4 + 160 * 3
    _same_record(_native.decode_record(rec, 4, 3), _native.OPOSE_E_ASSEMBLY, cand, subset)
    empty_c, empty_s = glue_standins.scene(902, 240, 320)
    rec = _native.encode_record(empty_c, empty_s, 4, 3)
    assert not rec.any()
    _same_record(_native.decode_record(rec, 4, 3), 0, empty_c, empty_s)
    with pytest.raises(ValueError):
        _native.encode_record(cand, -np.ones((4, 20)), 4, 3)
    with pytest.raises(ValueError):
        _native.encode_record(np.zeros((73, 4)), subset, 4, 3)


@pytest.mark.parametrize("name,cand,subset,row", CASES, ids=[c[0] for c in CASES])
def test_selected_pose_equals_the_reference_row(name, cand, subset, row):
    from src.pipeline import selected_pose
    got = selected_pose(cand, subset)
    assert got.shape == (18, 3) and got.dtype == np.float64
    assert np.array_equal(got, row)


def test_the_fixture_holds_its_edge_cases():
    by = {c[0]: c for c in CASES}
    assert len(CASES) == 11
    _, c, s, row = by["scene_900"]  # won through candidate[-1] by the person without a left shoulder
    lsx = np.array([c[int(p[5])][0] for p in s])
    assert s[np.argmax(lsx)][5] == -1 and row[5].tolist() == [0, 0, 0] and row.any()
    assert len(by["scene_902"][2]) == 0 and not by["scene_902"][3].any()
    assert len(by["scene_903"][2]) == 1
    _, c, s, row = by["e2e_23_1"]  # a tie among the 20 people without a left shoulder: the first wins
    lsx = np.array([c[int(p[5])][0] for p in s])
    assert (lsx == lsx.max()).sum() == 20 and np.argmax(lsx) == 68 and np.array_equal(np.flatnonzero(lsx == lsx.max()),
                                                                                     np.flatnonzero(s[:, 5] == -1))


class GoldenBody:
    """body.extract stand-in: the reference's row of every frame, looked up by the frame's region
    of interest."""

    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "body_extract.npz"))
        self.rows = {zlib.crc32(glue_standins.frame(int(s), 240, 320).tobytes()): r
                     for s, r in zip(g["seeds"], g["scenes"])}
        self.calls = []

    def extract(self, frames, recpoint=None):
        self.calls.append((frames.shape, recpoint))
        (x0, y0), (x1, y1) = recpoint
        return np.stack([self.rows[zlib.crc32(np.ascontiguousarray(f[y0:y1, x0:x1]).tobytes())] for f in frames])


def test_batch_body_extraction_writes_the_reference_file(tmp_path, capsys):
    import joblib
    from src.motion import Batch_body_extraction
    body, out = GoldenBody(), str(tmp_path / "video-exact-body.pkl")
    assert Batch_body_extraction("clip_exact.avi", out, 2, ROI, body=body, capture=glue_standins.FakeCapture) is None
    # whole frames go in, one extract per batch: the region of interest is the callee's offset
    assert body.calls == [((2, 300, 400, 3), ROI), ((1, 300, 400, 3), ROI)]
    mat = joblib.load(out)
    ref = np.load(os.path.join(GOLDEN, "body_extract.npz"))["clip_exact"]
    assert mat.dtype == np.float64 and mat.shape == ref.shape == (3, 18, 3) and np.array_equal(mat, ref)
    assert capsys.readouterr().out == "the %s file is saved\n" % out


def test_batch_body_extraction_unopened_path(tmp_path, capsys):
    from src.motion import Batch_body_extraction
    body, out = GoldenBody(), str(tmp_path / "b.pkl")
    assert Batch_body_extraction("dir/missing.avi", out, 2, ROI, body=body, capture=glue_standins.FakeCapture) is None
    assert capsys.readouterr().out == "the file dir/missing.avi is not exist\n"
    assert not body.calls and not os.path.exists(out)


def test_batch_body_extraction_short_container(tmp_path):
    from src.motion import Batch_body_extraction
    out = str(tmp_path / "b.pkl")
    with pytest.raises(TypeError, match="'NoneType' object is not subscriptable"):  # reports 7, decodes 5
        Batch_body_extraction("clip_short.avi", out, 2, ROI, body=GoldenBody(), capture=glue_standins.FakeCapture)
    assert not os.path.exists(out)


def test_batch_body_extraction_reads_no_more_than_reported(tmp_path):
    import joblib
    from src.motion import Batch_body_extraction
    body, out = GoldenBody(), str(tmp_path / "b.pkl")
    Batch_body_extraction("clip_overflow.avi", out, 2, ROI, body=body, capture=glue_standins.FakeCapture)  # 3 of 5
    assert [c[0][0] for c in body.calls] == [2, 1]
    assert np.array_equal(joblib.load(out), np.load(os.path.join(GOLDEN, "body_extract.npz"))["scenes"][:3])


def test_batch_body_extraction_progress_prints(tmp_path, capsys):
    from src.motion import Batch_body_extraction

    class Capture:  # 2000 tiny frames
        def __init__(self, path):
            self.i = 0

        def isOpened(self):
            return True

        def get(self, prop):
            return 2000.0

        def read(self):
            self.i += 1
            return (True, np.zeros((2, 2, 3), np.uint8)) if self.i <= 2000 else (False, None)

    class Body:
        def extract(self, frames, recpoint=None):
            return np.zeros((len(frames), 18, 3))

    out = str(tmp_path / "sub" / "video-001-body.pkl")
    os.mkdir(tmp_path / "sub")
    Batch_body_extraction("v.avi", out, 32, None, body=Body(), capture=Capture)
    assert capsys.readouterr().out == ("video-001-body.pkl-1000/2000\nvideo-001-body.pkl-2000/2000\n"
                                       "the %s file is saved\n" % out)
