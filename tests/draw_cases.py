"""The drawing rule stated once, and the case tables of the drawing tests (tests/test_gpu_draw.py on
the GPU, tests/test_draw_cases.py for the statement and the inputs alone).

The statement is plain NumPy / integer Python: which primitives a Body record or a MotionMat row
draws, in which order, with which integer parameters (`prims_of_record`, `prims_of_motion`: the
table opose_debug_draw_prims returns), and which pixels each covers (`draw`).  The cos / sin of a
limb's whole degrees are the literals of csrc/draw_table.h, parsed, never recomputed.  `draw`
tests every pixel of the frame against every primitive and ignores the boxes, so a box that is too
small on the device shows as a missing pixel.  Every comparison is bit equality.

Inputs are seeded and pinned by digests.
"""
import functools
import hashlib
import math
import os
import re

import numpy as np

from conftest import PKG
from src.util import _COLORS, _HAND_EDGES, _LIMBS

OK, E_ARG, E_CAPACITY = 0, -1, -5
NONE, DISC, LIMB, LINE = 0, 1, 2, 3
PRIM_INTS = 12
COORD_MAX = 16384.0
CHUNK = 256  # primitives draw_pixels compacts at a time (csrc/kernels.h kDrawThreads)
LIMB_PAIRS = [(a - 1, b - 1) for a, b in _LIMBS[:17]]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def _table():
    src = open(os.path.join(PKG, "csrc", "draw_table.h")).read()
    v = [float.fromhex(t) for t in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", src)]
    assert len(v) == 720
    return [(v[2 * k], v[2 * k + 1]) for k in range(360)]


TABLE = _table()


# ------------------------------------------------------------------------------------ limb parameters
def limb_degrees(y, x):
    """int(math.degrees(math.atan2(y, x))) % 360.  At the multiples of 45 degrees the exact angle is
    an integer and an ulp of atan2 would decide int(): they are settled by comparisons."""
    if y == 0:
        return 180 if math.copysign(1.0, x) < 0 else 0
    if x == 0:
        return 90 if y > 0 else 270
    if abs(y) == abs(x):
        return (45 if x > 0 else 135) if y > 0 else (315 if x > 0 else 225)
    return int(math.degrees(math.atan2(y, x))) % 360


def limb_params(xa, ya, xb, yb):
    """(cx, cy, a, k) of the limb from joint (xa, ya) to joint (xb, yb): src/util.py:66-72 with the
    reference's names (X holds the y coordinates, Y the x), sqrt for its `** 0.5` and k mod 360."""
    Y0, Y1, X0, X1 = float(xa), float(xb), float(ya), float(yb)
    dX, dY = X0 - X1, Y0 - Y1
    return int((Y0 + Y1) / 2), int((X0 + X1) / 2), int(math.sqrt(dX * dX + dY * dY) / 2), limb_degrees(dX, dY)


def reference_limb_params(xa, ya, xb, yb):
    """src/util.py:62-72 as the reference writes it, on a two-row candidate: (int(mY), int(mX),
    int(length / 2), int(angle))."""
    candidate = np.array([[xa, ya, 1.0, 0.0], [xb, yb, 1.0, 1.0]], dtype=np.float64)
    index = np.array([0.0, 1.0])
    Y = candidate[index.astype(int), 0]
    X = candidate[index.astype(int), 1]
    mX = np.mean(X)
    mY = np.mean(Y)
    length = ((X[0] - X[1]) ** 2 + (Y[0] - Y[1]) ** 2) ** 0.5
    angle = math.degrees(math.atan2(X[0] - X[1], Y[0] - Y[1]))
    return int(mY), int(mX), int(length / 2), int(angle)


# ------------------------------------------------------------------------------------ primitives
def _colour(c):
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def _prim(kind, colour, cx, cy, p0, p1, box, H, W):
    x0, y0, x1, y1 = max(box[0], 0), max(box[1], 0), min(box[2] + 1, W), min(box[3] + 1, H)
    if x0 >= x1 or y0 >= y1:
        x0 = y0 = x1 = y1 = 0
    return [kind, colour, cx, cy, p0, p1, x0, y0, x1, y1, 0, 0]


def disc_prim(x, y, colour, H, W):
    cx, cy = int(x), int(y)
    return _prim(DISC, colour, cx, cy, 0, 0, (cx - 4, cy - 4, cx + 4, cy + 4), H, W)


def limb_prim(xa, ya, xb, yb, colour, H, W):
    cx, cy, a, k = limb_params(xa, ya, xb, yb)
    c, s, A, B = abs(TABLE[k][0]), abs(TABLE[k][1]), a + 0.5, 4.5
    ex, ey = int(c * A + s * B) + 1, int(s * A + c * B) + 1  # the grown ellipse's half extents, from above
    return _prim(LIMB, colour, cx, cy, a, k, (cx - ex, cy - ey, cx + ex, cy + ey), H, W)


def line_prim(x1, y1, x2, y2, H, W):
    px, py, qx, qy = int(x1), int(y1), int(x2), int(y2)
    return _prim(LINE, _colour([255, 0, 0]), px, py, qx, qy,
                 (min(px, qx) - 1, min(py, qy) - 1, max(px, qx) + 1, max(py, qy) + 1), H, W)


EMPTY = [0] * PRIM_INTS


def _coord_ok(*v):
    return all(-COORD_MAX <= x <= COORD_MAX for x in v)  # False for NaN


def _body_prims(people, joint, H, W):
    """35 * people slots in draw order; joint(person, i) -> None (absent), "bad", or (x, y).
    Returns (slots, bad)."""
    slots, bad = [], False
    for i in range(18):
        for n in range(people):
            j = joint(n, i)
            bad |= j == "bad"
            slots.append(disc_prim(j[0], j[1], _colour(_COLORS[i]), H, W) if isinstance(j, tuple) else EMPTY)
    for i, (pa, pb) in enumerate(LIMB_PAIRS):
        for n in range(people):
            a, b = joint(n, pa), joint(n, pb)
            bad |= a == "bad" or b == "bad"
            both = isinstance(a, tuple) and isinstance(b, tuple)
            slots.append(limb_prim(a[0], a[1], b[0], b[1], _colour(_COLORS[i]), H, W) if both else EMPTY)
    return slots, bad


def _finish(slots, bad, status):
    if status != OK or bad:
        return np.zeros((0, PRIM_INTS), np.int32), (status if status != OK else E_ARG)
    return np.array(slots, np.int32).reshape(-1, PRIM_INTS), OK


def prims_of_record(candidate, subset, H, W, status=OK):
    """(prims [35 * people, 12] int32, status) of draw_bodypose(frame, candidate, subset)."""
    if status != OK:
        return _finish([], False, status)
    candidate = np.asarray(candidate, np.float64).reshape(-1, 4)
    subset = np.asarray(subset, np.float64).reshape(-1, 20)

    def joint(n, i):
        v = subset[n][i]
        if not (v > -2.0 and v < len(candidate)):
            return "bad"
        if int(v) == -1:
            return None
        x, y = candidate[int(v)][:2]
        return (float(x), float(y)) if _coord_ok(x, y) else "bad"

    return _finish(*_body_prims(len(subset), joint, H, W), OK)


def prims_of_motion(row, H, W):
    """(prims [35 | 117, 12] int32, status) of DisplayPose's canvas for one MotionMat row."""
    row = np.asarray(row, np.float64)

    def joint(n, i):
        if sum(row[i, :]) == 0:
            return None
        x, y = row[i, :2]
        return (float(x), float(y)) if _coord_ok(x, y) else "bad"

    slots, bad = _body_prims(1, joint, H, W)
    if len(row) == 60:
        for peaks in np.reshape(row[18:, :2], (2, -1, 2)):
            for e0, e1 in _HAND_EDGES:
                (x1, y1), (x2, y2) = peaks[e0], peaks[e1]
                if (x1 + y1 != 0) and (x2 + y2 != 0):
                    ok = _coord_ok(x1, y1, x2, y2)
                    bad |= not ok
                    slots.append(line_prim(x1, y1, x2, y2, H, W) if ok else EMPTY)
                else:
                    slots.append(EMPTY)
            for x, y in peaks:
                ok = _coord_ok(x, y)
                bad |= not ok
                slots.append(disc_prim(x, y, _colour([0, 0, 255]), H, W) if ok else EMPTY)
    return _finish(slots, bad, OK)


# ------------------------------------------------------------------------------------ pixels
def covered(prim, H, W):
    """bool [H, W]: the pixels of an H x W frame the primitive covers (its box is not consulted)."""
    kind, _, cx, cy, p0, p1 = (int(v) for v in prim[:6])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    dx, dy = xx - cx, yy - cy
    if kind == DISC:
        return dx * dx + dy * dy <= 16
    if kind == LIMB:
        c, s = TABLE[p1]
        fx, fy = dx.astype(np.float64), dy.astype(np.float64)
        u = fx * c + fy * s
        v = fy * c - fx * s
        A, B = p0 + 0.5, 4.5
        return u * u * (B * B) + v * v * (A * A) <= (A * A) * (B * B)
    if kind == LINE:
        ax, ay = p0 - cx, p1 - cy
        w, L2, d2 = dx * ax + dy * ay, ax * ax + ay * ay, dx * dx + dy * dy
        ex, ey = xx - p0, yy - p1
        return np.where(w <= 0, d2 <= 1, np.where(w >= L2, ex * ex + ey * ey <= 1, d2 * L2 - w * w <= L2))
    return np.zeros((H, W), bool)


def draw(canvas, prims):
    """The primitives applied in order to a copy of the uint8 canvas [H, W, 3]."""
    out = np.array(canvas, np.uint8)
    H, W = out.shape[:2]
    for p in prims:
        if p[0] == NONE:
            continue
        m = covered(p, H, W)
        colour = np.array([p[1] & 255, (p[1] >> 8) & 255, (p[1] >> 16) & 255], np.float64)
        if p[0] == LIMB:
            out[m] = np.rint(out[m].astype(np.float64) * 0.4 + colour * 0.6).astype(np.uint8)
        else:
            out[m] = colour.astype(np.uint8)
    return out


def draw_records_statement(frame, candidate, subset, status=OK):
    """(canvas, status): a frame whose status is not OK is returned as it is."""
    prims, st = prims_of_record(candidate, subset, frame.shape[0], frame.shape[1], status)
    return draw(frame, prims), st


def draw_motion_statement(frame, row):
    prims, st = prims_of_motion(row, frame.shape[0], frame.shape[1])
    return draw(frame, prims), st


def prim_table(prims_list, cap):
    """[N, cap, 12] int32 and counts [N] as opose_debug_draw_prims lays them out."""
    out = np.zeros((len(prims_list), cap, PRIM_INTS), np.int32)
    for n, p in enumerate(prims_list):
        out[n, :len(p)] = p
    return out, np.array([len(p) for p in prims_list], np.int32)


# ------------------------------------------------------------------------------------ case tables
HW = (37, 53)  # frames of the pixel cases: a partial 32 x 8 tile in both directions
LIMB_HW = (240, 320)  # frame of the displacement tables (their boxes are cut to it)
LIMB_DIGESTS = {"int": "c258a4a1aa95b1c3", "ninths": "a2d4e0a973d960ab", "raw": "486acfafbe65f007"}


@functools.lru_cache(maxsize=None)
def limb_table(kind):
    """float64 [n, 4]: joints (xa, ya) and (xb, yb).  "int": every integer displacement of
    [-40, 40]^2 from (100, 90), Pythagorean lengths and every multiple of 45 degrees among them;
    "ninths" / "raw": seeded joints on multiples of 1/9 / anywhere, displacements up to 120."""
    H, W = LIMB_HW
    if kind == "int":
        d = np.array([(dx, dy) for dy in range(-40, 41) for dx in range(-40, 41)], np.float64)
        a = np.tile([100.0, 90.0], (len(d), 1))
    else:
        rng = np.random.default_rng({"ninths": 4101, "raw": 4102}[kind])
        a = rng.random((2000, 2)) * [W, H]
        d = (rng.random((2000, 2)) * 2 - 1) * 120
        if kind == "ninths":
            a, d = np.rint(a * 9.0) / 9.0, np.rint(d * 9.0) / 9.0
    t = np.concatenate([a, a + d], 1)
    assert digest(t) == LIMB_DIGESTS[kind], (kind, digest(t))
    return t


def limb_rows(table):
    """MotionMat rows [n, 18, 3] whose only joints are 1 and 2: limb 0, slot 18 of the table."""
    rows = np.zeros((len(table), 18, 3))
    rows[:, 1, :2], rows[:, 2, :2] = table[:, :2], table[:, 2:]
    rows[:, 1:3, 2] = 1.0
    return rows


def noise_frames(n, hw=HW, seed=4300):
    return np.random.default_rng(seed).integers(0, 256, size=(n,) + tuple(hw) + (3,), dtype=np.uint8)


def _edge_pose():
    """The hand-made body of frame 1 (H x W = 37 x 53): a limb over each frame edge, limbs fully
    outside, a = 0 inside the frame, a negative angle that is no integer."""
    p = np.zeros((18, 3))
    for j, xy in {1: (26, 18), 2: (-10, 12),   # (1, 2) over the left edge
                  3: (-30, 5),                 # (2, 3) fully outside
                  5: (70, 20),                 # (1, 5) over the right edge
                  6: (60, -9),                 # (5, 6) fully outside
                  8: (20, -12),                # (1, 8) over the top edge
                  11: (30, 50),                # (1, 11) over the bottom edge
                  0: (27, 17),                 # (1, 0): length sqrt(2), a = 0, 135 degrees
                  14: (40, 10.5),              # (0, 14)
                  15: (15, 25),                # (0, 15): atan2(-8, 12) = -33.69 -> -33
                  13: (16384.0, -16384.0)}.items():  # the coordinate bound itself: a disc far outside
        p[j] = (xy[0], xy[1], 0.5)
    return p


MOTION_DIGESTS = {18: "73f5e4440e8532de", 60: "aa69a83c4d90e8d8"}


@functools.lru_cache(maxsize=None)
def motion_rows(joints):
    """MotionMat rows [3, joints, 3] for three HW frames: a seeded integer pose with two joints
    missing, the hand-made edge pose, a seeded pose on multiples of 1/9 reaching 6 pixels past the
    frame; with 60 joints the hands: seeded, all missing, keypoints missing / outside / with
    x + y == 0, ninths."""
    H, W = HW
    rng = np.random.default_rng(4200)
    rows = np.zeros((3, joints, 3))
    rows[0, :18, 0], rows[0, :18, 1], rows[0, :18, 2] = np.rint(rng.random(18) * W), np.rint(rng.random(18) * H), 0.5
    rows[0, [3, 9]] = 0.0
    rows[1, :18] = _edge_pose()
    rows[2, :18, 0] = np.rint((rng.random(18) * (W + 12) - 6) * 9.0) / 9.0
    rows[2, :18, 1] = np.rint((rng.random(18) * (H + 12) - 6) * 9.0) / 9.0
    rows[2, :18, 2] = 0.25
    rows[2, [6, 16]] = 0.0
    if joints == 60:
        rows[0, 18:39, 0], rows[0, 18:39, 1] = np.rint(rng.random(21) * W), np.rint(rng.random(21) * H)
        rows[0, 18:39, 2] = 0.75  # (the right hand stays missing: 21 discs at (0, 0), no edge)
        rows[1, 18:60, 0] = np.rint(rng.random(42) * (W + 20) - 10)
        rows[1, 18:60, 1] = np.rint(rng.random(42) * (H + 20) - 10)
        rows[1, [19, 23, 40], :2] = 0.0      # missing keypoints between present ones
        rows[1, 30, :2] = (5.0, -5.0)        # x + y == 0: no edge, a disc at (5, -5)
        rows[1, 45, :2] = (52.0, 36.0)       # the frame's last pixel
        rows[2, 18:60, 0] = np.rint((rng.random(42) * W) * 9.0) / 9.0
        rows[2, 18:60, 1] = np.rint((rng.random(42) * H) * 9.0) / 9.0
        rows[2, 18:60, 2] = rng.random(42)
    assert digest(rows) == MOTION_DIGESTS[joints], (joints, digest(rows))
    return rows


def people_record(poses):
    """(candidate [n, 4], subset [P, 20]) of poses [P, 18, 3] (a joint whose score is 0 is missing),
    ids in part-major order as Body numbers its peaks."""
    poses = np.asarray(poses, np.float64).reshape(-1, 18, 3)
    subset = -np.ones((len(poses), 20))
    cand = []
    for i in range(18):
        for n, p in enumerate(poses):
            if p[i, 2] != 0:
                subset[n, i] = len(cand)
                cand.append([p[i, 0], p[i, 1], p[i, 2], len(cand)])
    subset[:, 19] = (subset[:, :18] >= 0).sum(1)
    subset[:, 18] = 1.0
    return np.array(cand, np.float64).reshape(-1, 4), subset


RECORD_DIGEST = "63a2ac3e3e454344"


@functools.lru_cache(maxsize=None)
def record_cases():
    """[(name, candidate, subset, record status, expected status)] for HW frames: 0, 1 and 9 people
    (9: 315 primitives, more than one chunk; seeded integer joints up to 4 pixels outside the frame,
    one in seven missing, so limbs of different people overlap), then the frames that must stay
    untouched."""
    H, W = HW
    rng = np.random.default_rng(4400)
    nine = np.zeros((9, 18, 3))
    nine[:, :, 0] = np.rint(rng.random((9, 18)) * (W + 8) - 4)
    nine[:, :, 1] = np.rint(rng.random((9, 18)) * (H + 8) - 4)
    nine[:, :, 2] = (rng.random((9, 18)) > 1.0 / 7.0) * 0.5
    one = _edge_pose()[None]
    c9, s9 = people_record(nine)
    c1, s1 = people_record(one)
    bad_index = s1.copy()
    bad_index[0, 5] = len(c1)  # one past the candidates
    inf = c1.copy()
    inf[3, 1] = np.inf
    far = c1.copy()
    far[2, 0] = 16385.0
    cases = [("no_people", np.zeros((0, 4)), np.zeros((0, 20)), OK, OK),
             ("one_person", c1, s1, OK, OK),
             ("nine_people", c9, s9, OK, OK),
             ("record_status", c9, s9, E_CAPACITY, E_CAPACITY),
             ("index_past_candidates", c1, bad_index, OK, E_ARG),
             ("inf_coordinate", inf, s1, OK, E_ARG),
             ("coordinate_past_bound", far, s1, OK, E_ARG)]
    d = digest(*[a for _, c, s, _, _ in cases for a in (c, s)])
    assert d == RECORD_DIGEST, d
    return cases
