"""CPU: the drawing statement (tests/draw_cases.py) against the reference's expressions and today's
host rasteriser, and what its case tables cover -- counted on the statement alone, so the GPU tests
(tests/test_gpu_draw.py) are known to exercise what they claim."""
import math

import numpy as np
import pytest

import draw_cases as dc
from conftest import report
from src import util


# ---------------------------------------------------------------- the trig table
def test_table_is_cos_sin_of_whole_degrees():
    assert len(dc.TABLE) == 360
    assert [dc.TABLE[k] for k in (0, 90, 180, 270)] == [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
    for k, (c, s) in enumerate(dc.TABLE):
        rc, rs = math.cos(math.radians(k)), math.sin(math.radians(k))
        if k % 90:  # (libm's own axis values are 6e-17, not 0: the table is exact there)
            assert abs(c - rc) <= math.ulp(rc) and abs(s - rs) <= math.ulp(rs), k


def test_blend_is_the_identity_on_an_unchanged_pixel():
    """The reference blends the whole canvas 0.4 / 0.6 with a copy that differs inside the limb
    only; outside, rint(0.4 c + 0.6 c) == c, so leaving uncovered pixels alone is the same."""
    c = np.arange(256, dtype=np.float64)
    assert np.array_equal(np.rint(c * 0.4 + c * 0.6), c)


# ---------------------------------------------------------------- limb parameters
@pytest.mark.parametrize("kind", ["int", "ninths", "raw"])
def test_limb_params_equal_the_reference_expressions(kind):
    t = dc.limb_table(kind)
    lengths, diag = set(), 0
    for xa, ya, xb, yb in t:
        cx, cy, a, k = dc.reference_limb_params(xa, ya, xb, yb)
        assert dc.limb_params(xa, ya, xb, yb) == (cx, cy, a, k % 360), (xa, ya, xb, yb)
        if kind == "int":
            sq = (xa - xb) ** 2 + (ya - yb) ** 2
            if math.isqrt(int(sq)) ** 2 == sq and xa != xb and ya != yb:
                lengths.add(int(sq))
            diag += abs(xa - xb) == abs(ya - yb)
    if kind == "int":
        # Pythagorean lengths (36 + 64: length / 2 sits on the integer 5) and the exact diagonals
        assert 100 in lengths and len(lengths) >= 10 and diag == 4 * 40 + 1


def test_a_negative_angle_truncates_toward_zero():
    cx, cy, a, k = dc.limb_params(27, 17, 15, 25)  # atan2(-8, 12) = -33.69 degrees
    assert k == (-33) % 360 and math.floor(math.degrees(math.atan2(-8, 12))) == -34


# ---------------------------------------------------------------- discs and limbs against util.py
def test_disc_mask_equals_fill_disc():
    H, W = 23, 31
    for cx, cy in [(10, 9), (0, 0), (30, 22), (-3, 5), (33, 11), (15, -4), (15, 26), (-9, -9)]:
        ref = np.zeros((H, W, 3), np.uint8)
        util._fill_disc(ref, cx, cy, 4, [1, 2, 3])
        p = dc.disc_prim(cx, cy, 1 | 2 << 8 | 3 << 16, H, W)
        assert np.array_equal(dc.draw(np.zeros((H, W, 3), np.uint8), [p]), ref), (cx, cy)
        m = dc.covered(p, H, W)
        assert not m.any() or (p[6] <= np.nonzero(m)[1].min() and np.nonzero(m)[1].max() < p[8])


def test_limbs_against_the_host_rasteriser_are_measured_not_gated():
    """util.draw_bodypose fills cv2.ellipse2Poly's polygon with matplotlib's contains_points(radius
    0.5): no pixel rule anyone can restate, so the share of differing pixels is a figure (DESIGN
    §7), not a bar.  What is asserted: the two agree away from the boundary."""
    H, W = 96, 128
    rng = np.random.default_rng(4500)
    differ = total = limbs = 0
    while limbs < 200:
        xa, xb = rng.random(2) * W
        ya, yb = rng.random(2) * H
        cx, cy, a, k = dc.limb_params(xa, ya, xb, yb)
        if a < 2:
            continue
        limbs += 1
        mine = dc.covered(dc.limb_prim(xa, ya, xb, yb, 0, H, W), H, W)
        ref = np.zeros((H, W, 3), np.uint8)
        util._fill_convex(ref, util._ellipse_poly((cx, cy), (a, 4), k), [255, 255, 255])
        theirs = ref[..., 0] != 0
        differ += int((mine != theirs).sum())
        total += int(mine.sum())
        # a pixel both call differently has a neighbour (8-connected) outside or inside both
        core = np.zeros_like(mine)
        core[1:-1, 1:-1] = np.all([np.roll(np.roll(mine & theirs, dy, 0), dx, 1)[1:-1, 1:-1]
                                   for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
        assert not (core & (mine != theirs)).any()
    line = "draw: %d of %d limb pixels (%.1f %%) differ from util._fill_convex on %d seeded limbs" % (
        differ, total, 100.0 * differ / total, limbs)
    print(line)
    report(line)


# ---------------------------------------------------------------- what the cases cover
def _limb_prims(prims):
    return [p for p in prims if p[0] == dc.LIMB]


def test_boxes_hold_every_covered_pixel():
    H, W = dc.HW
    tables = [dc.prims_of_motion(r, H, W)[0] for j in (18, 60) for r in dc.motion_rows(j)]
    tables += [dc.prims_of_record(c, s, H, W)[0] for _, c, s, st, want in dc.record_cases() if want == dc.OK]
    seen = 0
    for prims in tables:
        for p in prims:
            if p[0] == dc.NONE:
                continue
            ys, xs = np.nonzero(dc.covered(p, H, W))
            if len(ys):
                seen += 1
                assert p[6] <= xs.min() and xs.max() < p[8] and p[7] <= ys.min() and ys.max() < p[9], p
            # (an empty box may still cover nothing: the box is an upper bound)
    assert seen > 300


def test_the_cases_cover_what_the_gpu_tests_claim():
    H, W = dc.HW
    cases = {name: (c, s) for name, c, s, _, _ in dc.record_cases()}
    nine, _ = dc.prims_of_record(*cases["nine_people"], H, W)
    assert len(nine) == 315 > dc.CHUNK  # more primitives than one compaction chunk
    assert (nine[dc.CHUNK:, 0] != dc.NONE).any()  # and the second chunk draws
    # pixels under limbs of different people: the limb-major order shows.  (The order of the people
    # alone cannot: limbs that swap places then share an index, so a colour, and two blends
    # towards one colour commute.  Drawn person by person, limbs of different colours swap.)
    c9, s9 = cases["nine_people"]
    owners = np.zeros((H, W), int)
    for n in range(9):
        one = _limb_prims(dc.prims_of_record(c9, s9[n:n + 1], H, W)[0])
        owners += np.any([dc.covered(p, H, W) for p in one], 0)
    assert (owners >= 2).sum() > 50
    frame = dc.noise_frames(1)[0]
    want = dc.draw_records_statement(frame, c9, s9)[0]
    assert np.array_equal(want, dc.draw_records_statement(frame, c9, s9[::-1])[0])
    limbs = nine[18 * 9:].reshape(17, 9, dc.PRIM_INTS)
    person_major = np.concatenate([nine[:18 * 9], limbs.transpose(1, 0, 2).reshape(-1, dc.PRIM_INTS)])
    assert not np.array_equal(want, dc.draw(frame, person_major))
    assert not np.array_equal(want, dc.draw(frame, nine[::-1]))
    # the edge pose: a limb fully outside, a limb over each edge, a = 0, a negative angle
    limbs = _limb_prims(dc.prims_of_motion(dc.motion_rows(18)[1], H, W)[0])
    assert any(p[6:10].tolist() == [0, 0, 0, 0] for p in limbs)
    masks = [dc.covered(p, H, W) for p in limbs]
    for edge in (np.s_[:, 0], np.s_[:, -1], np.s_[0, :], np.s_[-1, :]):
        assert any(m[edge].any() for m in masks)
    assert any(p[4] == 0 and m.any() for p, m in zip(limbs, masks))
    assert any(p[5] == (-33) % 360 for p in limbs)
    # a missing hand keypoint draws its disc at (0, 0); x + y == 0 draws a disc and no edge
    hands = dc.prims_of_motion(dc.motion_rows(60)[0], H, W)[0][35:]
    assert [p[:4].tolist() for p in hands[41 + 20:]] == [[dc.DISC, 255 << 16, 0, 0]] * 21
    assert (hands[41:41 + 20, 0] == dc.NONE).all() and (hands[:20, 0] == dc.LINE).all()
    mixed = dc.prims_of_motion(dc.motion_rows(60)[1], H, W)[0][35:]
    assert 0 < (mixed[:20, 0] == dc.LINE).sum() < 20
    assert [dc.DISC, 255 << 16, 5, -5] in [p[:4].tolist() for p in mixed]
    # the statuses of the frames that must stay untouched
    for name, c, s, st, want in dc.record_cases():
        prims, got = dc.prims_of_record(c, s, H, W, st)
        assert got == want and (want == dc.OK or len(prims) == 0), name
    bad = dc.motion_rows(60)[2].copy()
    bad[40, 0] = np.nan
    assert dc.prims_of_motion(bad, H, W)[1] == dc.E_ARG


def test_the_golden_person_draws():
    """The end-to-end fixture of the GPU test has people whose limbs land inside the frame."""
    import os
    from conftest import GOLDEN
    e = np.load(os.path.join(GOLDEN, "body_e2e_21_96x128.npz"))
    prims, st = dc.prims_of_record(e["candidate"], e["subset"], 96, 128)
    assert st == dc.OK and len(_limb_prims(prims)) >= 3
    assert not np.array_equal(dc.draw(e["img"], prims), e["img"])
