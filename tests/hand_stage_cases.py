"""Case tables of the hand extraction stage tests (tests/test_gpu_hand_stages.py on the GPU,
tests/test_hand_stage_cases.py for the inputs and the oracle alone): plain NumPy on the CPU,
seeded, every input pinned by a digest.  The oracle is oracle/hand_extract.py; every comparison is
bit equality (integer boxes, bytes, float32 and float64 values in a fixed operation order).

Poses whose box changes when `x3 + 0.33 * d` or `dx*dx + dy*dy` is evaluated fused were not
searched for; no case here is known to tell a contracted build from an exact one.
"""
import functools
import hashlib

import numpy as np

from oracle import hand_extract as he

E_SHAPE = he.E_SHAPE


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


# ------------------------------------------------------------------------------------ boxes
def _pose(shoulder, elbow, wrist, side, score=0.5):
    """One pose with the three joints of one side (0 left, 1 right); every other joint missing."""
    p = np.zeros((18, 3))
    for j, xy in zip(he.SIDES[side], (shoulder, elbow, wrist)):
        p[j] = (xy[0], xy[1], score)
    return p


def _random_poses(kind, hw, n, seed):
    """n poses whose arms are short enough for most boxes to fit the frame, some hanging over each
    edge: a wrist anywhere from 30 pixels outside the frame, the elbow and shoulder within a
    fifth of the frame of it.  kind: integer coordinates, multiples of 1/9, raw doubles."""
    rng = np.random.default_rng(seed)
    H, W = hw
    reach = max(H, W) / 5.0

    def snap(v):
        if kind == "int":
            return np.rint(v)
        if kind == "ninths":
            return np.rint(v * 9.0) / 9.0
        return v

    out = np.zeros((n, 18, 3))
    for k in range(n):
        out[k, :, 2] = 1.0 - rng.random(18)
        out[k, :, 0] = snap(rng.random(18) * W)
        out[k, :, 1] = snap(rng.random(18) * H)
        for sh, el, wr in he.SIDES:
            wrist = np.array([rng.random() * (W + 60) - 30, rng.random() * (H + 60) - 30])
            elbow = wrist + (rng.random(2) * 2 - 1) * reach
            shoulder = elbow + (rng.random(2) * 2 - 1) * reach
            out[k, wr, :2], out[k, el, :2], out[k, sh, :2] = snap(wrist), snap(elbow), snap(shoulder)
    return out


def _edge_poses():
    """Hand-made poses for the 240 x 320 frame, (name, pose, expected [left box, right box] or None)."""
    Z = [0, 0, 0, 0]
    cases = []

    def only(side, box):
        return [box + [1], Z] if side == 0 else [Z, box + [1]]
    base = ((8.0, 4.0), (80.0, 100.0), (180.0, 100.0))  # shoulder -> elbow (72, 96): 120; -> wrist (100, 0)
    for side in (0, 1):
        # 3-4-5 x 24 upper arm: 0.9 * 120 = 108 > 100, width 162, width / 2 = 81; 0.33 * 100 = 33.0:
        # the corner (180 + 33 - 81, 100 - 81) and the width are exact integers
        cases.append(("345_des_side%d" % side, _pose(*base, side), only(side, [132, 19, 162])))
        # the same arm 26 to the right: x + width == 320 exactly, no clip
        moved = tuple((x + 26.0, y) for x, y in base)
        cases.append(("x_plus_width_is_W_side%d" % side, _pose(*moved, side), only(side, [158, 19, 162])))
        # and 59 down: y + width == 240 exactly
        moved = tuple((x, y + 59.0) for x, y in base)
        cases.append(("y_plus_width_is_H_side%d" % side, _pose(*moved, side), only(side, [132, 78, 162])))
        # one more pixel: clipped by one
        moved = tuple((x + 27.0, y + 60.0) for x, y in base)
        cases.append(("one_past_both_side%d" % side, _pose(*moved, side), only(side, [159, 79, 161])))
        # 3-4-5 x 20 forearm (60, 80): dwe 100 leads 0.9 * 50, width 150 exactly
        cases.append(("345_dwe_side%d" % side, _pose((70.0, 10.0), (100.0, 50.0), (160.0, 130.0), side), None))
        # 0.9 * 100 == 90.0 == dwe: the tie of max(dwe, 0.9 * des)
        cases.append(("tie_side%d" % side, _pose((40.0, 20.0), (100.0, 100.0), (154.0, 172.0), side), None))
        # coincident joints: width 0, present
        cases.append(("coincident_side%d" % side, _pose((10.0, 10.0), (10.0, 10.0), (10.0, 10.0), side),
                      only(side, [10, 10, 0])))
        # a wrist far right of the frame: W - x is negative
        cases.append(("far_right_side%d" % side, _pose((900.0, 100.0), (950.0, 100.0), (1000.0, 100.0), side), None))
        # far below
        cases.append(("far_below_side%d" % side, _pose((100.0, 700.0), (100.0, 750.0), (100.0, 800.0), side), None))
        # an arm longer than the frame: width 1.5 * 400, clipped at all four edges
        cases.append(("wider_than_frame_side%d" % side,
                      _pose((-90.0, -190.0), (-90.0, -200.0), (150.0, 120.0), side), None))
        # each joint missing in turn, then "missing" only by its sum, then present at the origin
        for j in range(3):
            pts = [base[0], base[1], base[2]]
            p = _pose(*pts, side)
            p[he.SIDES[side][j]] = 0.0
            cases.append(("missing_joint%d_side%d" % (j, side), p, [Z, Z]))
            p = _pose(*pts, side)
            p[he.SIDES[side][j]] = (7.0, -7.0, 0.0)
            cases.append(("zero_sum_joint%d_side%d" % (j, side), p, [Z, Z]))
            p = _pose(*pts, side)
            p[he.SIDES[side][j]] = (0.0, 0.0, 0.25)
            cases.append(("origin_joint%d_side%d" % (j, side), p, None))
        # a sum that cancels only with the score: 3 + 4 - 7
        p = _pose(*base, side)
        p[he.SIDES[side][2]] = (3.0, 4.0, -7.0)
        cases.append(("cancelling_score_side%d" % side, p, [Z, Z]))
    return cases


# name -> ((H, W), builder of motion [N, 18, 3]); N = 1, 32, 33, 65 and the 64-thread block's 2 N > 64
BOXES = {
    "int_240x320_n200": ((240, 320), lambda: _random_poses("int", (240, 320), 200, 11)),
    "int_97x131_n65": ((97, 131), lambda: _random_poses("int", (97, 131), 65, 12)),
    "ninths_240x320_n33": ((240, 320), lambda: _random_poses("ninths", (240, 320), 33, 13)),
    "ninths_97x131_n100": ((97, 131), lambda: _random_poses("ninths", (97, 131), 100, 14)),
    "raw_240x320_n100": ((240, 320), lambda: _random_poses("raw", (240, 320), 100, 15)),
    "raw_97x131_n32": ((97, 131), lambda: _random_poses("raw", (97, 131), 32, 16)),
    "raw_97x131_n1": ((97, 131), lambda: _random_poses("raw", (97, 131), 1, 17)),
    "edges_240x320": ((240, 320), lambda: np.stack([c[1] for c in _edge_poses()])),
}


@functools.lru_cache(maxsize=None)
def box_case(name):
    """(motion float64 [N, 18, 3], (H, W), the oracle's boxes int32 [N, 2, 4], the branches each
    present side took, in slot order)."""
    hw, build = BOXES[name]
    motion = np.ascontiguousarray(build(), np.float64)
    taken = []
    ref = he.boxes(motion, hw, taken=taken)
    return motion, hw, ref, taken


# ------------------------------------------------------------------------------------ crops
CROP_A = dict(N=64, H=128, W=160, pad_w=176, bs=(8, 64))
CROP_B = dict(N=2, H=400, W=416, bs=(368,))
CROP_B_WIDTHS = {0: (1, 367, 368, 400), 1: (367, 1, 400, 368)}
CONTENTS = ("random", "pattern")


def _pattern(rng, H, W):
    """0 / 255 blocks 1 to 3 pixels wide and high, per channel: the steepest edges a cubic sees."""
    def blocks(n):
        sizes = rng.integers(1, 4, n)
        return np.repeat(np.arange(n), sizes)[:n]
    rows, cols = blocks(H), blocks(W)
    vals = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return vals[rows][:, cols]


def _anchored(rng, w, H, W, edge):
    """A w x w box flush with one frame edge (0 left, 1 right, 2 top, 3 bottom), else anywhere."""
    x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - w + 1))
    return [(0, y), (W - w, y), (x, 0), (x, H - w)][edge]


@functools.lru_cache(maxsize=None)
def crop_boxes_a(which):
    """boxes int32 [64, 2, 4] of set A.  which 0: slot k has w = k + 1; 1: w = 128 - k; every box
    present and inside the frame, a quarter of them flush with each edge.  which 2: pass 0 with
    the unusable and the absent slots of BAD_SLOTS planted."""
    c = CROP_A
    rng = np.random.default_rng(200 + which % 2)
    edges = rng.permutation(np.arange(2 * c["N"]) % 4)
    b = np.zeros((2 * c["N"], 4), np.int32)
    for k in range(2 * c["N"]):
        w = k + 1 if which != 1 else 128 - k
        x, y = _anchored(rng, w, c["H"], c["W"], int(edges[k]))
        b[k] = (x, y, w, 1)
    if which == 2:
        for k, box in BAD_SLOTS.items():
            b[k] = box
    return b.reshape(c["N"], 2, 4)


# slot -> box of pass 2 of set A.  None is on frame 0 or 63 and every box starts at row >= 1 well
# inside frames that have neighbours on both sides: a kernel that ignored the check would read other
# pixels of the staged frames, and return wrong bytes.
BAD_SLOTS = {
    20: (60, 50, 0, 1), 21: (60, 50, 0, 1),          # present, w = 0
    30: (60, 50, -3, 1), 31: (70, 40, -40, 1),       # present, w < 0
    40: (-1, 50, 20, 1), 41: (-7, 30, 33, 1),        # present, x < 0
    50: (160 + 1 - 25, 40, 25, 1), 51: (160 + 1 - 64, 20, 64, 1),   # x + w == W + 1
    60: (30, 128 + 1 - 31, 31, 1), 61: (50, 128 + 1 - 8, 8, 1),     # y + w == H + 1
    70: (10, 10, 40, 0), 71: (80, 60, 64, 0),        # absent, with a box that fits the frame
    80: (40, -2, 16, 1),                              # present, y < 0
}


@functools.lru_cache(maxsize=None)
def crop_frames(group, content):
    """uint8 frames of set "A" ([64, 128, 176, 3]: the tests take [:, :, :160] for the strided run
    and its contiguous copy for the other) or "B" ([2, 400, 416, 3])."""
    rng = np.random.default_rng({"A": 300, "B": 301}[group] + CONTENTS.index(content))
    if group == "A":
        N, H, W = CROP_A["N"], CROP_A["H"], CROP_A["pad_w"]
    else:
        N, H, W = CROP_B["N"], CROP_B["H"], CROP_B["W"]
    if content == "random":
        f = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    else:
        f = np.ascontiguousarray(np.stack([_pattern(rng, H, W) for _ in range(N)]))
    if group == "A" and content == "random":
        # every byte value inside the w == 64 box of pass 0 (slot 63): at boxsize 64 they all reach the output
        x, y, w, _ = crop_boxes_a(0).reshape(-1, 4)[63]
        blk = f[31, y:y + w, x:x + w].reshape(-1).copy()
        blk[:256] = np.arange(256)
        f[31, y:y + w, x:x + w] = blk.reshape(w, w, 3)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def crop_boxes_b(which):
    c = CROP_B
    rng = np.random.default_rng(210 + which)
    b = np.zeros((4, 4), np.int32)
    for k, w in enumerate(CROP_B_WIDTHS[which]):
        x, y = _anchored(rng, w, c["H"], c["W"], (k + which) % 4)
        b[k] = (x, y, w, 1)
    return b.reshape(2, 2, 4)


def crop_input(group, content, which):
    """(frames uint8 [N, H, W, 3], a view with row stride 3 * 176 for set A; boxes int32 [N, 2, 4])."""
    if group == "A":
        return crop_frames("A", content)[:, :, :CROP_A["W"]], crop_boxes_a(which)
    return crop_frames("B", content), crop_boxes_b(which)


@functools.lru_cache(maxsize=None)
def crop_case(group, content, which, bs):
    """The oracle's (crops uint8 [N, 2, bs, bs, 3], status int32 [N, 2], x float32 [N, 2, 3, bs, bs])."""
    frames, boxes = crop_input(group, content, which)
    out = he.crops(frames, boxes, bs)
    for a in out:
        a.setflags(write=False)
    return out


CROP_RUNS = ([("A", content, which, bs) for content in CONTENTS for which in (0, 1, 2) for bs in CROP_A["bs"]]
             + [("B", content, which, 368) for content in CONTENTS for which in (0, 1)])


# ---------------------------------------------------------------------------------- backmap
BACKMAP = [(2, 8), (2, 64), (2, 368), (40, 8), (40, 64), (40, 368)]   # (N, boxsize)
BACKMAP_WIDTHS = (1, 33, 53, 368, 400, 0)                             # 0: an absent (all-zero) box


@functools.lru_cache(maxsize=None)
def backmap_case(N, bs):
    """(peaks float64 [2N, 21, 3], found int32 [2N, 21], boxes int32 [N, 2, 4]): integer peaks in
    [0, bs) with x == 0, y == 0 and both planted on both sides, NaN rows where found is 0, scores
    of both signs with denormals among them; widths cycle so that each meets each side."""
    rng = np.random.default_rng(400 + N * 1000 + bs)
    slots = 2 * N
    boxes = np.zeros((slots, 4), np.int32)
    for s in range(slots):
        w = BACKMAP_WIDTHS[(s + s // 12) % 6] if N > 2 else (1, 400, 0, 53)[s]
        if w:
            boxes[s] = (rng.integers(0, 300), rng.integers(0, 300), w, 1)
    peaks = np.empty((slots, 21, 3))
    peaks[..., 0] = rng.integers(0, bs, (slots, 21))
    peaks[..., 1] = rng.integers(0, bs, (slots, 21))
    peaks[..., 2] = rng.standard_normal((slots, 21))
    peaks[:, 0, :2] = np.stack([np.zeros(slots), np.maximum(peaks[:, 0, 1], 1)], 1)   # x == 0 only
    peaks[:, 1, :2] = np.stack([np.maximum(peaks[:, 1, 0], 1), np.zeros(slots)], 1)   # y == 0 only
    peaks[:, 2, :2] = 0                     # both
    peaks[:, 3, :2] = bs - 1                # the far corner
    peaks[:, 4, 2] = 5e-324 * rng.integers(1, 1000, slots)     # denormal scores
    peaks[:, 5, 2] = -2.0 ** -1060
    peaks[:, 6, 2] = -0.0
    found = np.ones((slots, 21), np.int32)
    found[rng.random((slots, 21)) < 0.2] = 0
    found[:, :7] = 1
    found[:, 7] = 0
    peaks[found == 0] = np.nan
    return peaks, found, boxes.reshape(N, 2, 4)


# --------------------------------------------------------------------------------- the chain
@functools.lru_cache(maxsize=None)
def chain_case():
    """Poses whose boxes all fit their 240 x 320 frame -> (frames uint8 [N, 240, 320, 3], motion,
    peaks [2N, 21, 3] and found [2N, 21] planted per slot, boxsize)."""
    motion, hw, ref, _ = box_case("int_240x320_n200")
    ok = [n for n in range(len(motion))
          if all(he.usable(ref[n, s], hw) for s in (0, 1)) and ref[n, 0, 2] != ref[n, 1, 2]][:6]
    motion = motion[ok].copy()
    motion[1, he.SIDES[0][1]] = 0.0   # frame 1 has no left hand,
    motion[4, he.SIDES[1][2]] = 0.0   # frame 4 no right hand
    rng = np.random.default_rng(500)
    frames = rng.integers(0, 256, (len(ok), hw[0], hw[1], 3), dtype=np.uint8)
    bs = 64
    peaks = np.empty((2 * len(ok), 21, 3))
    peaks[..., :2] = rng.integers(0, bs, (2 * len(ok), 21, 2))
    peaks[..., 2] = rng.random((2 * len(ok), 21))
    found = (rng.random((2 * len(ok), 21)) < 0.8).astype(np.int32)
    return frames, motion, peaks, found, bs


# -------------------------------------------------------------------------------- preprocess
# (w, scale): square hand crops at Hand's four scales (src/hand.py:26-32, multiplier scale * 368 / w)
PREPROCESS = [(20, 0.5), (20, 1.0), (20, 1.5), (20, 2.0), (33, 0.5), (33, 1.0), (33, 1.5), (33, 2.0), (8, 2.0)]


@functools.lru_cache(maxsize=None)
def preprocess_case(w):
    img = np.random.default_rng(600 + w).integers(0, 256, (w, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------ input digests
INPUT_DIGESTS = {
    "boxes:int_240x320_n200": "35ff0061e747bbb2",
    "boxes:int_97x131_n65": "bef3a90695b7904d",
    "boxes:ninths_240x320_n33": "04ca42e2fa49b90e",
    "boxes:ninths_97x131_n100": "241136d0ef088b1a",
    "boxes:raw_240x320_n100": "dd94d68fcd84a677",
    "boxes:raw_97x131_n32": "3d9f6bb95a333500",
    "boxes:raw_97x131_n1": "eaae2a9182ab1b3b",
    "boxes:edges_240x320": "58c1bf3e9f34e335",
    "crops:A,pattern,0": "579e300bf9ac5c2b",
    "crops:A,pattern,1": "940d0db8de980fa8",
    "crops:A,pattern,2": "8bdc97116ac87864",
    "crops:A,random,0": "8e6dcc5a85c41679",
    "crops:A,random,1": "cdb2ebf1b7ad75f7",
    "crops:A,random,2": "8ab949462e4aa487",
    "crops:B,pattern,0": "e9f1b129ae12f592",
    "crops:B,pattern,1": "4741863836d17787",
    "crops:B,random,0": "50434514d62a2f11",
    "crops:B,random,1": "9fa98dea03e6665c",
    "backmap:2,8": "028f7ffc7be721ab",
    "backmap:2,64": "ddfa5f6ee3888802",
    "backmap:2,368": "188067f5389b671d",
    "backmap:40,8": "cb85c0ce3e97a76e",
    "backmap:40,64": "90d34af3d8237dc3",
    "backmap:40,368": "34d29f83e2e0d972",
    "chain:0": "6ccd2a4cdd988107",
    "preprocess:8": "3c1cd113fc2671ea",
    "preprocess:20": "b522c9d87eac1c7d",
    "preprocess:33": "42344f12e5e91917",
}


def case_digest(name):
    kind, _, rest = name.partition(":")
    if kind == "boxes":
        return digest(box_case(rest)[0])
    if kind == "crops":
        group, content, which = rest.split(",")
        return digest(*crop_input(group, content, int(which)))
    if kind == "backmap":
        N, bs = (int(v) for v in rest.split(","))
        return digest(*backmap_case(N, bs))
    if kind == "chain":
        return digest(*chain_case()[:4])
    assert kind == "preprocess"
    return digest(preprocess_case(int(rest)))


ALL_CASES = (["boxes:" + n for n in BOXES]
             + sorted({"crops:%s,%s,%d" % c[:3] for c in CROP_RUNS})
             + ["backmap:%d,%d" % c for c in BACKMAP] + ["chain:0"]
             + ["preprocess:%d" % w for w in sorted({c[0] for c in PREPROCESS})])
