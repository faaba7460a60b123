"""Case tables of the body matching stage tests (tests/test_gpu_match_stages.py on the GPU,
tests/test_match_stage_cases.py for the inputs and their conditions alone): peaks_finalize,
paf_score, limb_greedy and assemble_people, each fed through its debug hook.

Every input is seeded, every expected output comes from the oracle (oracle/body_post.py:
upsample_map, limb_scores, connect_limbs, assemble; oracle/batch_post.py resize_chain for the fast
mode's taps) or, for the two stages the oracle has no separate function for, from the plain NumPy
of the same lines of the reference: np.nonzero's order and the running ids for peaks_finalize, a
stable descending sort and a greedy walk for limb_greedy (test_match_stage_cases.py checks that
walk against connect_limbs).  All four kernels are float64 in the reference's operation order, so
every exact-mode comparison is equality.
"""
import functools
import hashlib

import numpy as np
import torch

import fast_stage_cases as fc
from oracle import batch_post, body_post
from oracle.body_post import LIMB_SEQ, MAP_IDX, MID_NUM

LIMB_A = [a - 1 for a, _ in LIMB_SEQ]
LIMB_B = [b - 1 for _, b in LIMB_SEQ]
PAF_X = [m[0] - 19 for m in MAP_IDX]
DEFAULT_CAP = (128, 96)         # peaks per part, people: a new handle's capacity
FILL = np.uint64(0xffffffffffffffff)  # what opose_debug_paf_score leaves in an entry it did not write
THRE2 = 0.05
# limb_greedy: the thread that holds pair e, its wave and its register slot; pairs from TAIL on are
# re-read from memory every round
GR_THREADS, GR_WAVE, GR_REG = 256, 64, 8
TAIL = GR_THREADS * GR_REG
# paf_score: pairs one workgroup column covers per trip of its loop (25 pairs x 64 blocks)
PAF_TRIP = 25 * 64


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def record_bytes(cap, maxp):
    return 16 + 32 * 18 * cap + 160 * maxp


def make_records(cap, maxp, frames, subset_fill=0.0):
    """uint8 [N, record_bytes]: per frame (status, candidate rows [n, 4], subset rows [m, 20] or
    None); the subset rows the frame does not set hold subset_fill."""
    rec = np.zeros((len(frames), record_bytes(cap, maxp)), np.uint8)
    off = 16 + 32 * 18 * cap
    for n, (status, cand, subset) in enumerate(frames):
        cand = np.asarray(cand, np.float64).reshape(-1, 4)
        m = 0 if subset is None else len(subset)
        rec[n, :16].view(np.int32)[:] = (status, len(cand), m, 0)
        rec[n, 16:16 + 32 * len(cand)].view(np.float64)[:] = cand.ravel()
        sub = rec[n, off:].view(np.float64)
        sub[:] = subset_fill
        if m:
            sub[:20 * m] = np.asarray(subset, np.float64).ravel()
    return rec


# --------------------------------------------------------------------------- peaks_finalize
# name -> capacity, frame size, and per frame the arrival order and the raw count of every part
# (a count in a dict: that part; every other part gets a seeded count below `small`)
FINALIZE = {
    # 0, 1, 64, 127 and 128 peaks in one frame; reversed raster order, then two seeded shuffles with
    # other counts per frame: the `before` sums and the frame strides
    "cap128": dict(cap=(128, 96), hw=(24, 31), small=40, frames=[
        ("reversed", {0: 0, 1: 1, 2: 64, 3: 127, 4: 128}),
        ("shuffled", {0: 128, 5: 0, 9: 127, 17: 65}),
        ("shuffled", {3: 0, 4: 0, 16: 1, 17: 128})]),
    # the largest capacity: 1024 peaks ranked by 128 threads
    "cap1024": dict(cap=(1024, 256), hw=(40, 60), small=30, frames=[("shuffled", {2: 1000, 7: 1024, 8: 0})]),
    # one peak too many in part 11 only: status -5, the clamped total, every row still exact
    "overflow": dict(cap=(128, 96), hw=(24, 31), small=40, frames=[("shuffled", {11: 129}), ("shuffled", {})]),
}


@functools.lru_cache(maxsize=None)
def finalize_case(name):
    """Inputs cnt [N, 18], list / score [N, 18, cap] of opose_debug_peaks_finalize and what it must
    answer: records [N, bytes], peak_pos [N, 18, cap], part_cnt [N, 18]."""
    c = FINALIZE[name]
    (cap, maxp), (H, W) = c["cap"], c["hw"]
    rng = np.random.default_rng(7000 + sum(map(ord, name)))
    N = len(c["frames"])
    cnt = np.zeros((N, 18), np.int32)
    lst = np.full((N, 18, cap), -1, np.int32)
    score = np.zeros((N, 18, cap), np.float64)
    pos = np.full((N, 18, cap), -1, np.int32)
    pcnt = np.zeros((N, 18), np.int32)
    frames = []
    for n, (order, counts) in enumerate(c["frames"]):
        cand, over = [], False
        for p in range(18):
            raw = counts.get(p, int(rng.integers(0, c["small"])))
            k = min(raw, cap)
            over |= raw > cap
            where = np.sort(rng.choice(H * W, k, replace=False)).astype(np.int32)
            arrive = where[::-1] if order == "reversed" else rng.permutation(where)
            val = rng.random(k)
            cnt[n, p], lst[n, p, :k], score[n, p, :k] = raw, arrive, val
            # src/body.py:88-94: np.nonzero of the part's mask, the map's value there, the running id
            mask, smap = np.zeros((H, W), bool), np.zeros((H, W))
            mask.ravel()[arrive] = True
            smap.ravel()[arrive] = val
            ys, xs = np.nonzero(mask)
            cand += [(xs[i], ys[i], smap[ys[i], xs[i]], len(cand) + i) for i in range(k)]
            pos[n, p, :k], pcnt[n, p] = ys * W + xs, k
        frames.append((-5 if over else 0, cand, None))
    return dict(cap=cap, maxp=maxp, N=N, H=H, W=W, cnt=cnt, list=lst, score=score,
                records=make_records(cap, maxp, frames), peak_pos=pos, part_cnt=pcnt)


# -------------------------------------------------------------------------------- paf_score
# name -> frame size, scales [(hl, wl, pad_down, pad_right)], seed
PAF = {
    "a_resize": dict(hw=(60, 81), scales=[(6, 8, 2, 5)], seed=0),            # 46 x 59 -> 60 x 81
    "b_frame": dict(hw=(45, 63), scales=[(6, 8, 3, 1)], seed=0),             # the cropped x8 map is the frame
    "c_rows_equal": dict(hw=(45, 70), scales=[(6, 8, 3, 1)], seed=0),        # Hs == H, Ws != W: a resize at step 1.0
    "d_three_scales": dict(hw=(60, 81), seed=0,                              # 31 x 38, 46 x 59 and 93 x 122 -> 60 x 81
                           scales=[(4, 5, 1, 2), (6, 8, 2, 5), (12, 16, 3, 6)]),
}
PAF_FAST = dict(hw=(60, 81), low=(7, 9), crop=(53, 70), seed=0)
BIG_PARTS = (1, 2, 3, 4)   # limbs 0, 2 and 3 join two of them: 45 x 45 pairs and more


def paf_maps(rng, N, hl, wl, dirs):
    """maps [N, 57, hl, wl] float32: every limb's PAF pair is its dominant direction plus noise."""
    maps = (0.3 * rng.standard_normal((N, 57, hl, wl))).astype(np.float32)
    for k in range(19):
        for c in range(2):
            maps[:, PAF_X[k] + c] = (dirs[k, c] + 0.35 * rng.standard_normal((N, hl, wl))).astype(np.float32)
    return maps


def paf_peaks(rng, N, H, W, cap):
    """peak_pos [N, 18, cap] (row-major per part, unused -1) and part_cnt [N, 18]: the big parts hold
    45 .. 47 peaks with the four corners and a point on every border among them (so pairs of two big
    parts meet on the same pixel); the other parts hold a few or none."""
    pos = np.full((N, 18, cap), -1, np.int32)
    pcnt = np.zeros((N, 18), np.int32)
    fixed = [0, W - 1, (H - 1) * W, H * W - 1, W // 2, (H - 1) * W + W // 3, (H // 2) * W, (H // 3) * W + W - 1]
    for n in range(N):
        for p in range(18):
            if p in BIG_PARTS:
                k = 45 + (n + p) % 3
                rest = np.setdiff1d(np.arange(H * W), fixed)
                where = np.concatenate([fixed, rng.choice(rest, k - len(fixed), replace=False)])
            else:
                k = (0, 1, 3, 5, 0, 2)[(p + 2 * n) % 6]
                where = rng.choice(H * W, k, replace=False)
            pos[n, p, :k], pcnt[n, p] = np.sort(where), k
    return pos, pcnt


def all_peaks_of(pos, pcnt, W):
    """one frame's peak_pos / part_cnt as the oracle's all_peaks (scores 0: no stage here reads them)."""
    out, ident = [], 0
    for p in range(18):
        out.append([(int(v) % W, int(v) // W, 0.0, ident + i) for i, v in enumerate(pos[p, :pcnt[p]])])
        ident += int(pcnt[p])
    return out


def pair_details(cand_a, cand_b, paf_x, paf_y):
    """What limb_scores (src/body.py:118-141) decides a limb's pairs from, restated so the conditions
    can see it: norm [nA, nB], the ten sample products s [nA, nB, 10], the sample coordinates before
    rint (x, y) and the score (test_match_stage_cases.py holds it equal to limb_scores')."""
    xa = np.array([c[0] for c in cand_a], np.int64)[:, None]
    ya = np.array([c[1] for c in cand_a], np.int64)[:, None]
    xb = np.array([c[0] for c in cand_b], np.int64)[None, :]
    yb = np.array([c[1] for c in cand_b], np.int64)[None, :]
    vx, vy = xb - xa, yb - ya
    norm = np.sqrt((vx * vx + vy * vy).astype(np.float64)) + 1e-10
    t = np.arange(MID_NUM, dtype=np.float64)

    def lin(a, b):
        a = np.broadcast_to(a, vx.shape).astype(np.float64)
        b = np.broadcast_to(b, vx.shape).astype(np.float64)
        pts = t[None, None, :] * ((b - a) / (MID_NUM - 1))[..., None] + a[..., None]
        pts[..., -1] = b
        return pts

    fx, fy = lin(xa, xb), lin(ya, yb)
    sx, sy = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)
    s = paf_x[sy, sx] * (vx / norm)[..., None] + paf_y[sy, sx] * (vy / norm)[..., None]
    acc = 0.0 + s[..., 0]
    for k in range(1, MID_NUM):
        acc = acc + s[..., k]
    prior = 0.5 * paf_x.shape[0] / norm - 1
    return norm, s, fx, fy, acc / MID_NUM + np.where(prior > 0, 0.0, prior)


def score_blocks(pos, pcnt, pafs, H, W, cap, details=None):
    """Expected output of opose_debug_paf_score as uint64 bit patterns [N, 19, cap * cap]: limb k's
    where(accept, score, -inf) over its first nA * nB entries, FILL beyond.  pafs[n]: [H, W, 38].
    details: a list that receives (n, k, score, accept, norm, s, fx, fy) per non-empty limb."""
    N = len(pafs)
    out = np.full((N, 19, cap * cap), FILL, np.uint64)
    for n in range(N):
        peaks = all_peaks_of(pos[n], pcnt[n], W)
        for k in range(19):
            ca, cb = peaks[LIMB_A[k]], peaks[LIMB_B[k]]
            if not ca or not cb:
                continue
            px, py = pafs[n][:, :, PAF_X[k]], pafs[n][:, :, PAF_X[k] + 1]
            score, accept = body_post.limb_scores(ca, cb, px, py, H, THRE2)
            out[n, k, :score.size] = np.where(accept, score, -np.inf).ravel().view(np.uint64)
            if details is not None:
                details.append((n, k, score, accept) + pair_details(ca, cb, px, py)[:4])
    return out


@functools.lru_cache(maxsize=None)
def paf_case(name):
    """maps (one [N, 57, hl, wl] per scale), the scales, peak_pos, part_cnt, the float64 PAF average
    per frame and the expected score bit patterns, at the default capacity, N = 2."""
    c = PAF[name]
    H, W = c["hw"]
    cap, N = DEFAULT_CAP[0], 2
    rng = np.random.default_rng(8000 + c["seed"] * 100 + sum(map(ord, name)))
    ang = rng.uniform(0, 2 * np.pi, 19)
    dirs = np.stack([np.cos(ang), np.sin(ang)], 1)
    maps = [paf_maps(rng, N, hl, wl, dirs) for hl, wl, _, _ in c["scales"]]
    pos, pcnt = paf_peaks(rng, N, H, W, cap)
    pafs = []
    for n in range(N):
        avg = np.zeros((H, W, 38))
        for m, (hl, wl, pd, pr) in zip(maps, c["scales"]):  # src/body.py:60-68
            avg += body_post.upsample_map(m[n, :38], [0, 0, pd, pr], (8 * hl, 8 * wl), (H, W)) / len(maps)
        pafs.append(avg)
    return dict(cap=cap, N=N, H=H, W=W, maps=maps, scales=c["scales"], peak_pos=pos, part_cnt=pcnt, pafs=pafs,
                expect=score_blocks(pos, pcnt, pafs, H, W, cap))


@functools.lru_cache(maxsize=None)
def paf_fast_case():
    """The fast mode's taps: maps [2, 57, 7, 9], geometry, peaks, and per limb of each frame
    (n, k, entries) -> the float32 and the float64 oracle's (score, accept, sample products)."""
    c = PAF_FAST
    (H, W), (hl, wl), (nh, nw) = c["hw"], c["low"], c["crop"]
    cap, N = DEFAULT_CAP[0], 2
    rng = np.random.default_rng(8500 + c["seed"])
    ang = rng.uniform(0, 2 * np.pi, 19)
    maps = paf_maps(rng, N, hl, wl, np.stack([np.cos(ang), np.sin(ang)], 1))
    pos, pcnt = paf_peaks(rng, N, H, W, cap)
    limbs = {}
    for dt in (fc.F32, fc.F64):
        full = batch_post.resize_chain(torch.from_numpy(maps[:, :38]), (H, W, nh, nw), dtype=dt)[1]
        pafs = full.numpy().transpose(0, 2, 3, 1)
        det = []
        score_blocks(pos, pcnt, pafs, H, W, cap, det)
        for n, k, score, accept, _, s, _, _ in det:
            limbs.setdefault((n, k), []).append((score, accept, s))
    return dict(cap=cap, N=N, H=H, W=W, maps=maps, low=(hl, wl), crop=(nh, nw), peak_pos=pos, part_cnt=pcnt,
                limbs=limbs)


def paf_fast_reference(case):
    """Flat over every pair of every limb: (frame, limb, entry), score32, score64, accept32, accept64
    and `decided`: where the float64 oracle decides every sample against thre2 and the score against
    zero by more than 8 e_ref, e_ref being the float32 oracle's largest error in the same quantity."""
    idx, s32, s64, a32, a64, p32, p64 = [], [], [], [], [], [], []
    for (n, k), ((sc32, ac32, pr32), (sc64, ac64, pr64)) in sorted(case["limbs"].items()):
        e = np.arange(sc64.size)
        idx.append(np.stack([np.full_like(e, n), np.full_like(e, k), e], 1))
        s32.append(sc32.ravel()), s64.append(sc64.ravel()), a32.append(ac32.ravel()), a64.append(ac64.ravel())
        p32.append(pr32.reshape(-1, MID_NUM)), p64.append(pr64.reshape(-1, MID_NUM))
    idx, s32, s64, a32, a64, p32, p64 = (np.concatenate(v) for v in (idx, s32, s64, a32, a64, p32, p64))
    e_sample, e_score = fc.e_ref(p32, p64), fc.e_ref(s32, s64)
    decided = (np.abs(p64 - THRE2).min(1) > fc.DECIDE * e_sample) & (np.abs(s64) > fc.DECIDE * e_score)
    return idx, s32, s64, a32, a64, decided


# ------------------------------------------------------------------------------ limb_greedy
def greedy(block, nA, nB):
    """src/body.py:143-151 on a limb's compact score block: the pairs above -inf in stable
    descending order, each taken unless its i or j is used, until min(nA, nB) are -> [(i, j, s)]."""
    sc = np.asarray(block[:nA * nB], np.float64)
    live = np.flatnonzero(sc > -np.inf)
    order = live[np.argsort(-sc[live], kind="stable")]
    used_a, used_b, rows = set(), set(), []
    for e in order:
        i, j = int(e) // nB, int(e) % nB
        if i in used_a or j in used_b:
            continue
        rows.append((i, j, float(sc[e])))
        used_a.add(i)
        used_b.add(j)
        if len(rows) >= min(nA, nB):
            break
    return rows


def tie_rounds(block, nA, nB):
    """Per round of the greedy walk, the entries e = i * nB + j that hold the largest score among the
    pairs still free (the candidates the kernel's scan, shuffle and merge choose the smallest of)."""
    sc = np.asarray(block[:nA * nB], np.float64).reshape(nA, nB).copy()
    rounds = []
    for i, j, s in greedy(block, nA, nB):
        rounds.append(np.flatnonzero(sc.ravel() == s))
        assert rounds[-1][0] == i * nB + j
        sc[i, :] = -np.inf
        sc[:, j] = -np.inf
    return rounds


# name -> capacity and, per frame, the part counts and the kind of score block of the limbs named
# (every other limb with two non-empty parts: normal scores, 40 % of them -inf)
GREEDY = {
    "cap128": dict(cap=(128, 96), frames=[
        # limbs: 0 128x128, 1 128x1, 2 128x100, 3 100x1, 4 1x128, 5 empty part, 6 128x16, 7 16x16 (one
        # register slot), 8 16x45, 9 128x46, 10 46x45 (just over 2048), 11 45x45 (just under),
        # 12 128x1, 13 1x1, 14 1x12, 15 1x20, 16 20x30 all -inf, 17 128x12 running out, 18 1x30
        dict(parts=[1, 128, 128, 100, 1, 1, 128, 0, 16, 16, 45, 46, 45, 45, 1, 20, 12, 30],
             kinds={16: "none", 17: "few"}),
        # 0 128x128 on 4 levels, 1 128x128 normal, 4 128x128 all equal, the rest small
        dict(parts=[3, 128, 128, 5, 2, 128, 128, 9, 0, 4, 7, 33, 1, 6, 2, 60, 64, 65],
             kinds={0: "levels", 4: "equal"})]),
    # dynamic LDS of 2 * cap flags: 200 x 256
    "cap256": dict(cap=(256, 96), frames=[
        dict(parts=[0, 200, 256, 3, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 0], kinds={})]),
}


@functools.lru_cache(maxsize=None)
def greedy_case(name):
    """score [N, 19, cap * cap], part_cnt [N, 18] and per (frame, limb) the expected rows (None: a
    part of the limb is empty, conn_cnt -1)."""
    c = GREEDY[name]
    cap = c["cap"][0]
    rng = np.random.default_rng(9000 + sum(map(ord, name)))
    N = len(c["frames"])
    score = np.full((N, 19, cap * cap), np.nan)
    pcnt = np.array([f["parts"] for f in c["frames"]], np.int32)
    expect = {}
    for n, f in enumerate(c["frames"]):
        for k in range(19):
            nA, nB = int(pcnt[n, LIMB_A[k]]), int(pcnt[n, LIMB_B[k]])
            if nA == 0 or nB == 0:
                expect[n, k] = None
                continue
            kind = f["kinds"].get(k, "normal")
            v = rng.standard_normal(nA * nB)
            if kind == "normal":
                v[rng.random(v.size) < 0.4] = -np.inf
            elif kind == "none":
                v[:] = -np.inf
            elif kind == "few":  # accepted pairs in 5 of the rows only: they run out before min(nA, nB)
                v.reshape(nA, nB)[~np.isin(np.arange(nA), rng.choice(nA, 5, replace=False))] = -np.inf
            elif kind == "levels":
                v = rng.integers(0, 4, v.size) * 0.25 + 0.125
            elif kind == "equal":
                v[:] = 0.75
            score[n, k, :v.size] = v
            expect[n, k] = greedy(score[n, k], nA, nB)
    return dict(cap=cap, maxp=c["cap"][1], N=N, score=score, part_cnt=pcnt, expect=expect)


# -------------------------------------------------------------------------- assemble_people
def scene(seed, P, vis=0.8, wrong=0.15, spurious=0.01, extra=0, total=None):
    """One frame for assemble_people: P planted people, each part visible with probability vis
    where its parent in the limb tree is (the neck has none), and a share of spurious peaks beside them, in
    shuffled order; per limb a matching that joins each
    person's two parts (5 % dropped), with a share `wrong` of the links' far ends swapped between two
    people, and links among the spurious peaks.  A fifth of the people score low (the mean prune),
    sparse people and spurious pairs stay below four parts (the count prune).  extra: that many more
    links of limb 0 between peaks of their own, added after every draw; total: connections beyond
    this many are cut from the last limbs back.
    -> (all_peaks, connection_all, special_k) as oracle.body_post.assemble takes them."""
    rng = np.random.default_rng(seed)
    quality = np.where(rng.random(P) < 0.2, 0.25, 1.0)
    seen = np.zeros((P, 18), bool)  # the neck, then each part of the limb tree where its parent is seen
    seen[:, 1] = rng.random(P) < vis
    for k in range(17):
        seen[:, LIMB_B[k]] = seen[:, LIMB_A[k]] & (rng.random(P) < vis)
    owners = []  # per part: the person of each peak (-1: spurious), in the order of the peak list
    for p in range(18):
        own = list(np.flatnonzero(seen[:, p])) + [-1] * int(rng.binomial(P + 20, spurious))
        owners.append([int(q) for q in rng.permutation(own)])
    peaks = [[(int(rng.integers(0, 600)), int(rng.integers(0, 300)),
               float(rng.uniform(0.3, 1.0) * (quality[q] if q >= 0 else 0.6))) for q in own] for own in owners]
    links, special = [], []
    for k in range(19):
        oa, ob = owners[LIMB_A[k]], owners[LIMB_B[k]]
        if not oa or not ob:
            special.append(k)
            links.append([])
            continue
        at_b = {q: j for j, q in enumerate(ob) if q >= 0}
        lk = [[i, at_b[q], q] for i, q in enumerate(oa) if q >= 0 and q in at_b and rng.random() > 0.05]
        for a in range(len(lk) - 1):  # a wrong link: two people exchange their far ends
            if rng.random() < wrong:
                lk[a][1], lk[a + 1][1] = lk[a + 1][1], lk[a][1]
        free_a = [i for i, q in enumerate(oa) if q == -1]
        free_b = [j for j, q in enumerate(ob) if q == -1]
        lk += [[i, j, -1] for i, j in zip(free_a, free_b) if rng.random() < 0.5]
        lk = [(i, j, float(rng.uniform(0.2, 1.0) * (quality[q] if q >= 0 else 0.6))) for i, j, q in lk]
        links.append([lk[o] for o in np.argsort([-r[2] for r in lk], kind="stable")])
    for e in range(extra):  # (after every draw: the scene is its twin's plus these)
        links[0].append((len(peaks[1]), len(peaks[2]), 0.5))
        peaks[1].append((601 + e, 301, 0.5))
        peaks[2].append((601 + e, 302, 0.5))
    start = np.concatenate([[0], np.cumsum([len(p) for p in peaks])])
    all_peaks = [[r + (int(start[p]) + i,) for i, r in enumerate(peaks[p])] for p in range(18)]
    conns = [[[all_peaks[LIMB_A[k]][i][3], all_peaks[LIMB_B[k]][j][3], sc, i, j] for i, j, sc in links[k]]
             for k in range(19)]
    if total is not None:
        k = 18
        while sum(len(c) for c in conns) > total:
            if conns[k]:
                conns[k].pop()
            else:
                k -= 1
    return all_peaks, [np.array(c, np.float64).reshape(-1, 5) for c in conns], special


INDEX_ERROR = [(0, [(0, 0), (1, 1), (2, 2)]), (1, [(1, 0), (0, 0), (2, 0)])]


def index_error_scene():
    """Three peaks per part and two limbs, the second no matching: limb 0 (parts 1, 2) opens rows 0,
    1, 2; limb 1 (parts 1, 5) ends all its links on peak 0 of part 5.  The link from peak 1 finds row
    1 by part 1 and writes part 5 into it; the link from peak 0 finds row 0 by part 1 and row 1 by
    part 5, both hold parts 1 and 2, so the conflict branch writes part 5 into row 0 as well; the link
    from peak 2 then finds rows 0 and 1 by part 5 and row 2 by part 1: subset_idx[2] = j, the
    reference's IndexError (src/body.py:170-173)."""
    all_peaks = [[(10 * p + i, 7 * i + p, 0.5 + 0.1 * i, 3 * p + i) for i in range(3)] for p in range(18)]
    conns = [np.zeros((0, 5)) for _ in range(19)]
    for k, links in INDEX_ERROR:
        conns[k] = np.array([[3 * LIMB_A[k] + i, 3 * LIMB_B[k] + j, 0.9 - 0.1 * i, i, j] for i, j in links])
    return all_peaks, conns, []


def expected_frame(scn, maxp, status_in=0, trace=None):
    """(status, candidate rows, subset rows or None) assemble_people must leave for a scene: the
    oracle's subset; -6 where the oracle raises IndexError, -5 where its rows pass max_people at any
    time (the kernel keeps no subset then), the incoming status where that is not 0."""
    all_peaks, conns, special = scn
    cand = [r for part in all_peaks for r in part]
    if status_in:
        return status_in, cand, None
    tr = {} if trace is None else trace
    try:
        _, subset = body_post.assemble(all_peaks, conns, special, tr)
    except IndexError:
        return -6, cand, None
    return (-5, cand, None) if tr["peak_rows"] > maxp else (0, cand, subset)


def assemble_inputs(cap, maxp, scenes, status_in=None, subset_fill=0.0):
    """The arrays opose_debug_assemble takes for these frames, and the records it must leave."""
    N = len(scenes)
    status_in = status_in or [0] * N
    pcnt = np.zeros((N, 18), np.int32)
    ci = np.full((N, 19, cap), -1, np.int32)
    cj = np.full((N, 19, cap), -1, np.int32)
    cs = np.full((N, 19, cap), np.nan)
    ccnt = np.zeros((N, 19), np.int32)
    before, after = [], []
    for n, (all_peaks, conns, special) in enumerate(scenes):
        pcnt[n] = [len(p) for p in all_peaks]
        for k in range(19):
            m = len(conns[k])
            ccnt[n, k] = -1 if k in special else m
            if m:
                ci[n, k, :m], cj[n, k, :m], cs[n, k, :m] = conns[k][:, 3], conns[k][:, 4], conns[k][:, 2]
        exp = expected_frame(scenes[n], maxp, status_in[n])
        before.append((status_in[n], exp[1], None))
        after.append(exp)
    return dict(cap=cap, maxp=maxp, N=N, part_cnt=pcnt, conn_i=ci, conn_j=cj, conn_s=cs, conn_cnt=ccnt,
                records=make_records(cap, maxp, before, subset_fill),
                expect=make_records(cap, maxp, after, subset_fill))


# name -> capacity and the frames: scene() arguments, "index_error", or ("status", code, scene args).
# The seeds are the first that meet the conditions test_match_stage_cases.py asserts
ASSEMBLE = {
    "p5": dict(cap=DEFAULT_CAP, frames=[dict(seed=3, P=5)]),
    "p40": dict(cap=DEFAULT_CAP, frames=[dict(seed=2, P=40)]),
    # more than 64 rows, and a merge that drops a row below 64 while more than 64 exist
    "p60": dict(cap=DEFAULT_CAP, frames=[dict(seed=2, P=60)]),
    # exactly max_people rows at the peak, and its twin with one more link of its own
    "p100_rows96": dict(cap=DEFAULT_CAP, frames=[dict(seed=47, P=100)]),
    "p100_rows97": dict(cap=DEFAULT_CAP, frames=[dict(seed=47, P=100, extra=1)]),
    # 72 KB of LDS, more connections than it stages at once, more than 128 rows
    "p200_cap1024": dict(cap=(1024, 256), frames=[dict(seed=0, P=200)]),
    "index_error": dict(cap=DEFAULT_CAP, frames=["index_error", dict(seed=1, P=5)]),
    "status_in": dict(cap=DEFAULT_CAP, frames=[("status", -5, dict(seed=2, P=5)), dict(seed=3, P=5)], fill=7.0),
    "mixed3": dict(cap=DEFAULT_CAP, frames=[dict(seed=4, P=5), "index_error", dict(seed=5, P=40)]),
}
TALLY_CASES = ("p5", "p40", "p60", "p100_rows96")  # together: every branch and both prune reasons
STAGE_CAP = (128, 256)   # the capacity of the total == stage / stage + 1 pair
STAGE_SCENE = dict(seed=1, P=100)


def _scenes(frames):
    scenes, status = [], []
    for f in frames:
        code = 0
        if isinstance(f, tuple):
            _, code, f = f
        scenes.append(index_error_scene() if f == "index_error" else scene(**f))
        status.append(code)
    return scenes, status


@functools.lru_cache(maxsize=None)
def assemble_case(name):
    c = ASSEMBLE[name]
    scenes, status = _scenes(c["frames"])
    out = assemble_inputs(c["cap"][0], c["cap"][1], scenes, status, c.get("fill", 0.0))
    out["scenes"] = scenes
    return out


@functools.lru_cache(maxsize=None)
def assemble_total_case(total):
    """One frame at STAGE_CAP with exactly `total` connections."""
    scn = scene(total=total, **STAGE_SCENE)
    out = assemble_inputs(STAGE_CAP[0], STAGE_CAP[1], [scn])
    out["scenes"] = [scn]
    return out


# ------------------------------------------------------------------------------------ chain
CHAIN = ["body_planted_403_53x97_p2", "body_planted_501_368x656_p14"]


def chain_case(golden, rng):
    """A planted golden (np.load) as the chain's inputs: the peak list of its candidate rows in
    shuffled arrival order (the parts' sizes from the oracle's peak search on the golden's maps:
    the rows themselves do not name their part), maps [1, 57, hl, wl], pads and the frame size."""
    H, W = (int(v) for v in golden["img_hw"])
    pad, padded = [int(v) for v in golden["pad"]], tuple(int(v) for v in golden["padded_hw"])
    heat = body_post.upsample_map(golden["heat"], pad, padded, (H, W)).astype(np.float64)
    peaks = body_post.find_peaks(heat, 0.1)
    cand = np.asarray(golden["candidate"], np.float64).reshape(-1, 4)
    assert np.array_equal(np.array([r for p in peaks for r in p], np.float64).reshape(-1, 4), cand)
    cap = DEFAULT_CAP[0]
    cnt = np.array([[len(p) for p in peaks]], np.int32)
    lst = np.full((1, 18, cap), -1, np.int32)
    score = np.zeros((1, 18, cap))
    start = 0
    for p in range(18):
        rows = cand[start:start + cnt[0, p]][rng.permutation(cnt[0, p])]
        lst[0, p, :len(rows)] = rows[:, 1] * W + rows[:, 0]
        score[0, p, :len(rows)] = rows[:, 2]
        start += cnt[0, p]
    maps = np.concatenate([golden["paf"], golden["heat"]], 0)[None].astype(np.float32)
    return dict(H=H, W=W, cnt=cnt, list=lst, score=score, maps=np.ascontiguousarray(maps),
                pads=(pad[2], pad[3]), candidate=cand, subset=np.asarray(golden["subset"], np.float64))
