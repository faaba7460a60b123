"""ORACLE (test infrastructure only): the fast mode's hand extraction around the hand network,
restated step by step from hitmaxiang/pytorch-openpose:

* boxes     srcmx/Batch_model.py:74-84 (the one-person subset of a MotionMat row) and
            srcmx/utilmx.py:267-320 (utilmx.handDetect), in Python floats
* crops     srcmx/Batch_model.py:86-99 (slice, cv2.flip of the left hand, cv2.resize INTER_CUBIC),
            :101-102 transforms.ToTensor and :328-329 the - 0.5 at scale 1
* backmap   srcmx/Batch_motion_Estimation.py:44-58 (crop peaks -> frame pixels, rows of HandMat)

Slots as the library numbers them: slot = 2 * frame + side, side 0 the left hand (shoulder 5,
elbow 6, wrist 7), side 1 the right (2, 3, 4).  A box is int32 {x, y, w, present}.

`** 2`: the reference squares with the scalar power of a float64, which is libm's pow(d, 2.0).
That is d * d for every d whose square is exact (integers, small dyadic fractions) but not for
every double: about 7 in 10000 random doubles differ in the last bit.  `boxes` takes the squaring
as an argument so that a test can show its cases do not rest on the difference.
"""
from __future__ import annotations

import math

import numpy as np

from .cv_resize import axis_table, resize_cubic

E_SHAPE = -2  # OPOSE_E_SHAPE
SIDES = ((5, 6, 7), (2, 3, 4))  # (shoulder, elbow, wrist) of the left and of the right arm
BRANCHES = ("xneg", "yneg", "right", "bottom", "des>dwe", "dwe>=des")


def _pow2(d):
    return d ** 2


def hand_box(x1, y1, x2, y2, x3, y3, hw, square=_pow2, taken=None):
    """srcmx/utilmx.py:297-320 for one arm -> [int(x), int(y), int(width)]; `taken` (a set)
    receives the names of the branches the arm took."""
    image_height, image_width = hw
    taken = set() if taken is None else taken
    x = x3 + 0.33 * (x3 - x2)
    y = y3 + 0.33 * (y3 - y2)
    dwe = math.sqrt(square(x3 - x2) + square(y3 - y2))
    des = math.sqrt(square(x2 - x1) + square(y2 - y1))
    taken.add("des>dwe" if 0.9 * des > dwe else "dwe>=des")
    width = 1.5 * max(dwe, 0.9 * des)
    x -= width / 2
    y -= width / 2
    if x < 0:
        x = 0
        taken.add("xneg")
    if y < 0:
        y = 0
        taken.add("yneg")
    width1 = width
    width2 = width
    if x + width > image_width:
        width1 = image_width - x
        taken.add("right")
    if y + width > image_height:
        width2 = image_height - y
        taken.add("bottom")
    width = min(width1, width2)
    return [int(x), int(y), int(width)]


def boxes(motion, hw, square=_pow2, taken=None):
    """motion [N, 18, 3] float64 (x, y, score) in frames of hw = (H, W) -> int32 [N, 2, 4].
    A joint is missing iff Python's sum of its row is 0 (srcmx/Batch_model.py:78); a side with a
    missing joint is all zeros.  `taken` (a list) receives one set of branch names per present
    side, in slot order."""
    motion = np.asarray(motion, np.float64)
    out = np.zeros((len(motion), 2, 4), np.int32)
    for n, pose in enumerate(motion):
        rows = [[float(v) for v in pose[i, :]] for i in range(18)]
        missing = [sum(r) == 0 for r in rows]
        for side, joints in enumerate(SIDES):
            if any(missing[j] for j in joints):
                continue
            (x1, y1), (x2, y2), (x3, y3) = (rows[j][:2] for j in joints)
            t = set()
            out[n, side, :3] = hand_box(x1, y1, x2, y2, x3, y3, hw, square, t)
            out[n, side, 3] = 1
            if taken is not None:
                taken.append(t)
    return out


def usable(box, hw):
    """The slice frame[y:y+w, x:x+w] is the w x w square the box names, w >= 1."""
    x, y, w = (int(v) for v in box[:3])
    return w >= 1 and x >= 0 and y >= 0 and x + w <= hw[1] and y + w <= hw[0]


def resize_unclamped(src, bs):
    """The uint8 branch of oracle.cv_resize.resize_cubic for a square bs x bs destination before its
    clamp to [0, 255]: int64 [bs, bs, C].  (No copy at bs == w: the cubic at source step 1.)"""
    sh, sw = src.shape[:2]
    xt, xc = axis_table(bs, sw, 1.0 / (bs / sw))
    yt, yc = axis_table(bs, sh, 1.0 / (bs / sh))
    ia = np.clip(np.rint(xc * np.float32(2048.0)).astype(np.int64), -32768, 32767)
    ib = np.clip(np.rint(yc * np.float32(2048.0)).astype(np.int64), -32768, 32767)
    S = src.astype(np.int64)
    h = sum(S[:, xt[:, j], :] * ia[None, :, j, None] for j in range(4))
    v = sum(h[yt[:, j], :, :] * ib[:, j, None, None] for j in range(4))
    return (v + (1 << 21)) >> 22


def crops(frames, boxes, bs):
    """frames uint8 [N, H, W, 3], boxes [N, 2, 4] -> (crops uint8 [N, 2, bs, bs, 3], status int32
    [N, 2], x float32 [N, 2, 3, bs, bs]).  An absent slot is gray 128 (srcmx/Batch_model.py:86-87)
    with status 0.  A present box that is empty or leaves the frame, where the reference dies in
    cv2.resize or resizes another rectangle than the box, is gray with status OPOSE_E_SHAPE."""
    frames = np.asarray(frames)
    N, H, W, _ = frames.shape
    out = np.full((N, 2, bs, bs, 3), 128, np.uint8)
    status = np.zeros((N, 2), np.int32)
    for n in range(N):
        for side in range(2):
            x, y, w, present = (int(v) for v in boxes[n, side])
            if not present:
                continue
            if not usable((x, y, w), (H, W)):
                status[n, side] = E_SHAPE
                continue
            tempimg = frames[n, y:y + w, x:x + w, :]
            if side == 0:
                tempimg = tempimg[:, ::-1]  # cv2.flip(.., 1)
            out[n, side] = resize_cubic(np.ascontiguousarray(tempimg), (bs, bs))
    # ToTensor: HWC uint8 -> CHW float32 / 255; Batch_hand: - 0.5
    x = np.transpose(out, (0, 1, 4, 2, 3)).astype(np.float32) / np.float32(255) - np.float32(0.5)
    return out, status, np.ascontiguousarray(x)


def backmap(peaks, found, boxes, bs):
    """peaks [2N, 21, 3] (x, y in crop pixels, score), found [2N, 21] or None, boxes [N, 2, 4] ->
    HandMat rows float64 [N, 42, 3]: the loop body of Batch_hand_extraction
    (srcmx/Batch_motion_Estimation.py:42-58) in numpy, in its operation order.  A row with found 0
    is what the reference's peak search returns for a part it did not find, zeros, whatever
    `peaks` holds there; found None takes every row as it is."""
    peaks = np.array(peaks, dtype=np.float64).reshape(-1, 21, 3)
    if found is not None:
        peaks[np.asarray(found).reshape(-1, 21) == 0] = 0.0
    out = np.zeros((len(boxes), 42, 3))
    for n in range(len(boxes)):
        r = peaks[2 * n + 1].copy()
        rx, ry, rw = np.asarray(boxes[n, 1, :3]).astype(np.float64)
        r[:, :2] = r[:, :2] * rw / bs
        r[:, 0] = np.where(r[:, 0] == 0, r[:, 0], r[:, 0] + rx)
        r[:, 1] = np.where(r[:, 1] == 0, r[:, 1], r[:, 1] + ry)
        out[n, 21:] = r
        lft = peaks[2 * n].copy()
        lx, ly, lw = np.asarray(boxes[n, 0, :3]).astype(np.float64)
        lft[:, :2] = lft[:, :2] * lw / bs
        lft[:, 0] = np.where(lft[:, 0] == 0, lft[:, 0], lw - lft[:, 0] - 1 + lx)
        lft[:, 1] = np.where(lft[:, 1] == 0, lft[:, 1], lft[:, 1] + ly)
        out[n, :21] = lft
    return out
