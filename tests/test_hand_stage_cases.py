"""CPU: the oracle of the hand extraction stage tests (oracle/hand_extract.py) reproduces the
reference's own outputs, and the inputs of tests/test_gpu_hand_stages.py reach every branch, edge
and clamp they are there for -- counted on the oracle alone, so that a badly seeded case fails
here and not on the GPU."""
import os

import numpy as np
import pytest

import hand_stage_cases as hc
from conftest import GOLDEN
from oracle import glue_standins
from oracle import hand_extract as he


@pytest.mark.parametrize("name", hc.ALL_CASES)
def test_input_digests(name):
    assert hc.case_digest(name) == hc.INPUT_DIGESTS[name]
    assert sorted(hc.INPUT_DIGESTS) == sorted(hc.ALL_CASES)


# ------------------------------------------------------------------ the oracle against the reference
def test_oracle_reproduces_the_reference_outputs():
    d = np.load(os.path.join(GOLDEN, "hand_extract_scenes.npz"))
    (x0, y0), (x1, y1) = glue_standins.ROI
    frames = np.stack([glue_standins.video_frame(int(s)) for s in d["seeds"]])[:, y0:y1, x0:x1]
    boxes = he.boxes(d["motion"], (y1 - y0, x1 - x0))
    assert np.array_equal(boxes[:, 0, :3], d["leftparams"]) and np.array_equal(boxes[:, 1, :3], d["rightparams"])
    assert boxes[:, :, 3].sum() == 7 and not boxes[boxes[:, :, 3] == 0].any()
    for bs in (64, 32):
        crops, status, x = he.crops(frames, boxes, bs)
        assert np.array_equal(crops, d["crops%d" % bs]) and not status.any()
        assert x.dtype == np.float32 and x.shape == (5, 2, 3, bs, bs)
        assert x.min() >= -0.5 and x.max() <= 0.5


# ------------------------------------------------------------------------------------ boxes
def test_box_cases_take_every_branch():
    count = dict.fromkeys(he.BRANCHES + ("right_only", "bottom_only", "right_and_bottom"), 0)
    kinds = set()
    for name in hc.BOXES:
        motion, hw, ref, taken = hc.box_case(name)
        assert np.isfinite(motion).all() and np.abs(motion).max() < 2.0 ** 31
        assert len(taken) == int(ref[:, :, 3].sum())
        if name.startswith("int"):
            assert np.array_equal(motion[:, :, :2], np.rint(motion[:, :, :2]))
        if name.startswith("ninths"):
            assert np.array_equal(motion[:, :, :2], np.rint(motion[:, :, :2] * 9) / 9)
            assert (motion[:, :, :2] != np.rint(motion[:, :, :2])).mean() > 0.5
        kinds.add(name.split("_")[0])
        for t in taken:
            for b in t:
                count[b] += 1
            count["right_only"] += "right" in t and "bottom" not in t
            count["bottom_only"] += "bottom" in t and "right" not in t
            count["right_and_bottom"] += "right" in t and "bottom" in t
        # the kernel squares with d * d, the reference with pow(d, 2): the same boxes on these cases
        assert np.array_equal(he.boxes(motion, hw, square=lambda v: v * v), ref)
    print("branches taken:", count)
    assert min(count.values()) >= 5, count
    assert kinds == {"int", "ninths", "raw", "edges"}
    assert sum(len(hc.box_case(n)[0]) for n in hc.BOXES if n.startswith("int")) >= 200
    assert {len(hc.box_case(n)[0]) for n in hc.BOXES} >= {1, 32, 33, 65}
    assert {hc.BOXES[n][0] for n in hc.BOXES} == {(240, 320), (97, 131)}


def test_box_knife_edges():
    cases = hc._edge_poses()
    motion, hw, ref, _ = hc.box_case("edges_240x320")
    byname = {c[0]: (c[1], ref[k], c[2]) for k, c in enumerate(cases)}
    for name, (_, got, expect) in byname.items():
        if expect is not None:
            assert got.tolist() == expect, name
    for side in (0, 1):
        s = "_side%d" % side
        sh, el, wr = he.SIDES[side]
        # the tie is a tie in floating point, the 3-4-5 arms are exact
        p = byname["tie" + s][0]
        des = np.hypot(*(p[el, :2] - p[sh, :2]))
        assert 0.9 * des == np.hypot(*(p[wr, :2] - p[el, :2])) == 90.0
        assert byname["345_dwe" + s][1][side].tolist()[2:] == [150, 1]
        assert byname["coincident" + s][1][side].tolist() == [10, 10, 0, 1]
        assert byname["far_right" + s][1][side][2] < 0 and byname["far_right" + s][1][side][3] == 1
        assert byname["far_below" + s][1][side][2] < 0
        wide = byname["wider_than_frame" + s][1][side]
        assert wide[0] == 0 and wide[1] == 0 and wide[2] == 240   # both corners clipped, min(W - 0, H - 0)
        for j in range(3):
            assert not byname["missing_joint%d" % j + s][1].any()
            assert not byname["zero_sum_joint%d" % j + s][1].any()    # (7, -7, 0) counts as missing
            assert byname["origin_joint%d" % j + s][1][side][3] == 1  # (0, 0, score) as present
        assert not byname["cancelling_score" + s][1].any()


# ------------------------------------------------------------------------------------ crops
def test_crop_boxes_cover_every_width_and_edge():
    c = hc.CROP_A
    seen = {0: set(), 1: set()}
    for which in (0, 1):
        b = hc.crop_boxes_a(which)
        assert b.shape == (64, 2, 4) and (b[..., 3] == 1).all()
        assert all(he.usable(box, (c["H"], c["W"])) for box in b.reshape(-1, 4))
        x, y, w = b[..., 0].ravel(), b[..., 1].ravel(), b[..., 2].ravel()
        for flush in (x == 0, x + w == c["W"], y == 0, y + w == c["H"]):
            assert flush.sum() >= 32, flush.sum()
        for side in (0, 1):
            seen[side] |= set(b[:, side, 2].tolist())
    assert seen[0] == seen[1] == set(range(1, 129))   # w == boxsize 8 and 64 among them
    for which in (0, 1):
        b = hc.crop_boxes_b(which)
        assert all(he.usable(box, (400, 416)) for box in b.reshape(-1, 4))
    for side in (0, 1):  # each width on each side
        assert {int(w) for which in (0, 1) for w in hc.crop_boxes_b(which)[:, side, 2]} == {1, 367, 368, 400}
    for content in hc.CONTENTS:
        frames, _ = hc.crop_input("A", content, 0)
        assert frames.shape == (64, 128, 160, 3) and frames.strides == (128 * 3 * 176, 3 * 176, 3, 1)
        assert hc.crop_input("B", content, 0)[0].flags.c_contiguous


def test_crop_bad_slots():
    c = hc.CROP_A
    good, bad = hc.crop_boxes_a(0).reshape(-1, 4), hc.crop_boxes_a(2).reshape(-1, 4)
    changed = np.flatnonzero((good != bad).any(1))
    assert changed.tolist() == sorted(hc.BAD_SLOTS)
    for content in hc.CONTENTS:
        for bs in c["bs"]:
            crops0, status0, _ = hc.crop_case("A", content, 0, bs)
            crops2, status2, x2 = hc.crop_case("A", content, 2, bs)
            crops0, crops2 = crops0.reshape(128, bs, bs, 3), crops2.reshape(128, bs, bs, 3)
            assert not status0.any()
            for k in range(128):
                if k in hc.BAD_SLOTS:
                    assert (crops2[k] == 128).all()
                    assert status2.ravel()[k] == (hc.E_SHAPE if hc.BAD_SLOTS[k][3] else 0)
                else:
                    assert status2.ravel()[k] == 0 and np.array_equal(crops2[k], crops0[k])
            gray = x2.reshape(128, 3, bs, bs)[sorted(hc.BAD_SLOTS)]
            assert (gray == np.float32(128) / np.float32(255) - np.float32(0.5)).all()
    kinds = {"w0": 0, "wneg": 0, "xneg": 0, "right": 0, "bottom": 0, "absent": 0}
    for k, (x, y, w, present) in hc.BAD_SLOTS.items():
        frame = k // 2
        # where a kernel without the check would read: 2 pixels around the box (|w| for w < 1), all
        # inside the staged frames, which have a frame before and one after this one
        assert 1 <= frame < c["N"] - 1
        assert y - 2 - max(0, -w) >= -c["H"] and y + max(w, 0) + 2 <= 2 * c["H"]
        kinds["absent"] += not present
        kinds["w0"] += present and w == 0
        kinds["wneg"] += present and w < 0
        kinds["xneg"] += present and x < 0
        kinds["right"] += present and w > 0 and x + w == c["W"] + 1
        kinds["bottom"] += present and w > 0 and y + w == c["H"] + 1
        if not present:
            assert he.usable((x, y, w), (c["H"], c["W"]))
    assert min(kinds.values()) >= 2, kinds


def test_crop_values_reach_both_clamps():
    lo = hi = 0
    for which in (0, 1):
        frames, boxes = hc.crop_input("A", "pattern", which)
        crops = hc.crop_case("A", "pattern", which, 64)[0]
        for n in range(0, 64, 3):
            for side in (0, 1):
                x, y, w, _ = boxes[n, side]
                src = frames[n, y:y + w, x:x + w]
                v = he.resize_unclamped(src[:, ::-1] if side == 0 else src, 64)
                assert np.array_equal(np.clip(v, 0, 255), crops[n, side])
                lo += int((v < 0).sum())
                hi += int((v > 255).sum())
    print("pre-clamp values below 0: %d, above 255: %d" % (lo, hi))
    assert lo > 100 and hi > 100
    # pass 0's slot 63 (w == boxsize 64): every byte value reaches the output
    assert hc.crop_boxes_a(0)[31, 1, 2] == 64
    assert np.unique(hc.crop_case("A", "random", 0, 64)[0][31, 1]).size == 256
    pattern = hc.crop_frames("A", "pattern")
    assert set(np.unique(pattern)) == {0, 255}


# ---------------------------------------------------------------------------------- backmap
def test_backmap_cases():
    pairs = set()
    for N, bs in hc.BACKMAP:
        peaks, found, boxes = hc.backmap_case(N, bs)
        assert peaks.shape == (2 * N, 21, 3) and found.shape == (2 * N, 21) and boxes.shape == (N, 2, 4)
        on = found != 0
        assert np.isnan(peaks[~on]).all() and (~on).sum() >= 2 * N
        xy = peaks[on][:, :2]
        assert np.array_equal(xy, np.rint(xy)) and xy.min() == 0 and xy.max() == bs - 1
        for side in (0, 1):
            p, f = peaks[side::2], on[side::2]
            assert ((p[..., 0] == 0) & (p[..., 1] != 0) & f).sum() >= N
            assert ((p[..., 0] != 0) & (p[..., 1] == 0) & f).sum() >= N
            assert ((p[..., 0] == 0) & (p[..., 1] == 0) & f).sum() >= N
            pairs |= {(side, int(w)) for w in boxes[:, side, 2]}
        s = peaks[on][:, 2]
        assert (s < 0).any() and ((s != 0) & (np.abs(s) < np.finfo(np.float64).tiny)).sum() >= 2 * N
        absent = ~boxes[..., 3].astype(bool).ravel()
        assert absent.any() and not boxes.reshape(-1, 4)[absent].any() and on[absent].any()
        ref = he.backmap(peaks, found, boxes, bs)
        assert np.isfinite(ref).all()
        rows = ref.reshape(N, 2, 21, 3).reshape(2 * N, 21, 3)
        assert not rows[~on].any()
        assert np.array_equal(rows[on][:, 2].view(np.uint64), peaks[on][:, 2].view(np.uint64))
    assert pairs == {(side, w) for side in (0, 1) for w in hc.BACKMAP_WIDTHS}


def test_chain_case():
    frames, motion, peaks, found, bs = hc.chain_case()
    boxes = he.boxes(motion, frames.shape[1:3])
    assert len(motion) == 6 and boxes[:, :, 3].tolist() == [[1, 1], [0, 1], [1, 1], [1, 1], [1, 0], [1, 1]]
    crops, status, _ = he.crops(frames, boxes, bs)
    assert not status.any() and (crops[1, 0] == 128).all() and (crops[4, 1] == 128).all()
    # no two slots alike but the two gray ones: a permutation of slots or sides cannot go unnoticed
    assert len({row.tobytes() for row in crops.reshape(12, -1)}) == 11
    hm = he.backmap(peaks, found, boxes, bs).reshape(12, -1)
    assert len({row.tobytes() for row in hm}) == 12
