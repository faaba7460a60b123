"""The shapelet search rule in NumPy, written so the order of operations can be read off, and the
seeded cases the shapelet tests and scripts/gen_shapelet_golden.py share.

The rule (include/opose.h states it too).  All arithmetic is float32, one rounding per operation:

    e(a, b) = sum over d = 0 .. D-1 ascending of (x[a, d] - y[b, d])**2, from +0
    s(r, c) = sum over k = 0 .. m-1 ascending of e(r + k, c + k), from +0
    dist    = sqrt(s)

A minimum over c is the first minimum of s; s is never negative, so its bits as an unsigned integer
order like its value, and the statement compares bits as the kernels do.  The loops over d and k
below are explicit; NumPy vectorises only over (a, b), which does not change any rounding."""
import functools
import hashlib
import os
import re

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------- distances
def e_matrix(x, y):
    """e(a, b) for every row a of x [n, D] and b of y [l, D]: float32 [n, l]."""
    x = np.ascontiguousarray(x, F32)
    y = np.ascontiguousarray(y, F32)
    acc = np.zeros((len(x), len(y)), F32)
    for d in range(x.shape[1]):
        t = x[:, None, d] - y[None, :, d]
        acc = acc + t * t
    return acc


def s_matrix(x, y, m):
    """s(r, c) for every start r of x and c of y: float32 [len(x) - m + 1, len(y) - m + 1]."""
    e = e_matrix(x, y)
    R, P = len(x) - m + 1, len(y) - m + 1
    acc = np.zeros((R, P), F32)
    for k in range(m):
        acc = acc + e[k:k + R, k:k + P]
    return acc


def first_min(s):
    """(min, loc) along the last axis: the first minimum, by the bits of s."""
    bits = np.ascontiguousarray(s, F32).view(np.uint32)
    loc = bits.argmin(axis=-1)  # the first occurrence of the minimum
    return np.take_along_axis(s, loc[..., None], -1)[..., 0], loc.astype(np.int32)


def sliding_distance(pattern, seqs):
    """SlidingDistance of pattern [m, D] against every sequence: the ragged dist, concatenated."""
    m = len(pattern)
    return np.concatenate([np.sqrt(s_matrix(pattern, y, m)[0]) for y in seqs])


def mindist(seqs, cand_seqs, m):
    """min over c of s(r, c) and its first c, for every start r of the sequences cand_seqs against
    every sequence: min2 float32 [n_cand, n_seq], loc int32 [n_cand, n_seq]; rows by (i, r).
    e is taken once per candidate sequence against all rows of the batch; a window that would
    cross into the next sequence is never read."""
    off = np.cumsum([0] + [len(y) for y in seqs])
    cat = np.concatenate([np.asarray(y, F32) for y in seqs])
    mins, locs = [], []
    for i in cand_seqs:
        x = np.asarray(seqs[i], F32)
        e = e_matrix(x, cat)
        R, G = len(x) - m + 1, len(cat) - m + 1
        s = np.zeros((R, G), F32)
        for k in range(m):
            s = s + e[k:k + R, k:k + G]
        mn = np.empty((R, len(seqs)), F32)
        lc = np.empty((R, len(seqs)), np.int32)
        for j in range(len(seqs)):
            mn[:, j], lc[:, j] = first_min(s[:, off[j]:off[j + 1] - m + 1])
        mins.append(mn)
        locs.append(lc)
    return np.concatenate(mins), np.concatenate(locs)


# ---------------------------------------------------------------------------------- score
def pair_keys(s_row, n_labels):
    """The samples' keys: the bits of s_k, or with mirrored copies (n_seq = 2 n_labels) the bits of
    the smaller s of the pair, the original on a tie; and which of the pair was taken."""
    bits = np.ascontiguousarray(s_row, F32).view(np.uint32)
    if len(bits) == n_labels:
        return bits.copy(), np.zeros(n_labels, bool)
    assert len(bits) == 2 * n_labels
    mirrored = bits[n_labels:] < bits[:n_labels]
    return np.where(mirrored, bits[n_labels:], bits[:n_labels]), mirrored


def candidate_score(s_row, labels):
    """(num, loss) of one candidate from its squared minima s_row [n_seq]."""
    labels = np.asarray(labels)
    n = len(labels)
    key, _ = pair_keys(s_row, n)
    order = np.lexsort((np.arange(n), key))  # by (bits, k): a stable sort by distance
    negs = int(n - np.count_nonzero(labels))
    correct = num = negs
    for k in order:
        correct += 1 if labels[k] else -1
        num = max(num, correct)
    acc = np.float64(0.0)
    for k in range(n):  # the positive samples' own (unmirrored) distances, k ascending
        if labels[k]:
            acc = acc + np.float64(np.sqrt(F32(s_row[k])))
    return num, acc / np.float64(n - negs)


def select(nums, losses):
    """The winner's row: a later candidate replaces the best only when strictly better."""
    best = 0
    for q in range(1, len(nums)):
        if nums[q] > nums[best] or (nums[q] == nums[best] and losses[q] < losses[best]):
            best = q
    return best


def find(seqs, labels, m):
    """The whole search over seqs (n_labels of them, or 2 n_labels with the mirrored copies last)."""
    labels = np.asarray(labels, np.uint8)
    cands = [i for i in range(len(labels)) if labels[i]]
    min2, loc = mindist(seqs, cands, m)
    rows = [(i, r) for i in cands for r in range(len(seqs[i]) - m + 1)]
    sc = [candidate_score(row, labels) for row in min2]
    nums = np.array([v[0] for v in sc], np.int32)
    losses = np.array([v[1] for v in sc], np.float64)
    w = select(nums, losses)
    return {"shapeindex": rows[w][0], "cand": rows[w][1], "num": int(nums[w]), "loss": float(losses[w]),
            "n_cand": len(rows), "dis": np.sqrt(min2[w]), "locs": loc[w].copy(), "min2": min2, "loc": loc,
            "nums": nums, "losses": losses}


def mirror_copies(seqs, mode):
    """'x-mirror' / 'y-mirror': the copies with the even / odd feature columns negated."""
    sign = np.ones(np.asarray(seqs[0]).shape[1], F32)
    sign[{"x-mirror": 0, "y-mirror": 1}[mode]::2] = -1
    return [np.asarray(y, F32) * sign for y in seqs]


def train(seqs, labels, m, mirror=None):
    """ShapeletMatrixModel.train under the rule: the model's attributes as a dict.  With a mirror
    mode the copies are appended; dis / locs / mirrored are then the chosen of each pair."""
    seqs = [np.asarray(y, F32) for y in seqs]
    n = len(labels)
    allseqs = seqs + mirror_copies(seqs, mirror) if mirror else seqs
    res = find(allseqs, labels, m)
    w = sum(len(seqs[i]) - m + 1 for i in range(res["shapeindex"]) if labels[i]) + res["cand"]
    _, mirrored = pair_keys(res["min2"][w], n)
    pick = np.arange(n) + n * mirrored
    return {"shapeindex": res["shapeindex"], "cand": res["cand"], "score": res["num"] / n, "num": res["num"],
            "loss": res["loss"], "dis": res["dis"][pick], "locs": res["locs"][pick].astype(np.int16),
            "mirrored": mirrored, "dis_all": res["dis"], "locs_all": res["locs"]}


# ---------------------------------------------------------------------------------- features
BODY_KEEP = list(range(2, 8))
GROUPS = ((0, 18, 1, BODY_KEEP), (18, 39, 0, list(range(1, 21))), (39, 60, 0, list(range(1, 21))))


def fill_forward(v):
    """Per column: a zero takes the last non-zero value at or before its row; a leading zero stays."""
    rows = np.arange(len(v))[:, None]
    last = np.maximum.accumulate(np.where(v != 0, rows, -1), axis=0)  # index of the last non-zero row
    return np.where(last >= 0, np.take_along_axis(v, np.maximum(last, 0), 0), v)


def fill_nearby(v):
    """Per column: a zero takes, from the unfilled data, the first non-zero of rows r-1, r+1, r-2,
    r+2 that exist."""
    out = v.copy()
    T = len(v)
    for r in range(T):
        for c in np.nonzero(v[r] == 0)[0]:
            for q in (r - 1, r + 1, r - 2, r + 2):
                if 0 <= q < T and v[q, c] != 0:
                    out[r, c] = v[q, c]
                    break
    return out


def motion_features(motion, lengths=None, featuremode=0):
    """MotionJointFeatures: motion float64 [L, joints, 3] (joints 18 or 60), ragged by lengths ->
    float32 [L, F, 2]."""
    motion = np.asarray(motion)
    L, J, _ = motion.shape
    assert J in (18, 60)
    lengths = [L] if lengths is None else list(lengths)
    assert sum(lengths) == L
    xy = motion[:, :, :2].astype(F32)  # the cast comes first; the score column is never used
    out = []
    a = 0
    for n in lengths:
        v = xy[a:a + n].reshape(n, 2 * J)
        a += n
        v = (fill_nearby(v) if featuremode == 2 else fill_forward(v)).reshape(n, J, 2)
        parts = []
        for lo, hi, origin, keep in GROUPS[:1 if J == 18 else 3]:
            g = v[:, lo:hi]
            o = g[:, origin:origin + 1]
            if featuremode == 2:
                g = np.where(g == 0, o, g)  # a missing joint sits on the origin (the nose included)
            rel = g - o
            if lo == 0:
                nose_y = rel[:, 0, 1]  # fl(nose.y - neck.y) of the filled (and replaced) body group
            parts.append(rel[:, keep])
        data = np.concatenate(parts, axis=1)
        if featuremode >= 1:
            data = data / (nose_y + F32(1e-5))[:, None, None]
        out.append(data.astype(F32))
    return np.concatenate(out)


# ---------------------------------------------------------------------------------- seeded cases
def make_set(seed, n_clips, D, m, n_pos, smooth=False, planted=False, integer=False, max_extra=25):
    """(seqs, labels): n_clips float32 clips of m .. m + max_extra rows, the first n_pos labelled 1
    after a seeded shuffle.  smooth: cumulative sums; planted: one shared window (plus noise) written
    into every positive clip; integer: small integers (exact arithmetic, so ties can be built)."""
    rng = np.random.default_rng(seed)
    labels = np.zeros(n_clips, np.uint8)
    labels[rng.permutation(n_clips)[:n_pos]] = 1
    lens = rng.integers(m, m + max_extra + 1, n_clips)
    seqs = []
    for n in lens:
        if integer:
            x = rng.integers(-4, 5, (n, D)).astype(F32)
        else:
            x = rng.standard_normal((n, D)).astype(F32)
            if smooth:
                x = np.cumsum(x * F32(0.3), axis=0, dtype=F32)
        seqs.append(x)
    if planted:
        pat = rng.standard_normal((m, D)).astype(F32) * F32(2)
        for i in np.nonzero(labels)[0]:
            p = int(rng.integers(0, len(seqs[i]) - m + 1))
            seqs[i][p:p + m] = pat + rng.standard_normal((m, D)).astype(F32) * F32(0.05)
    return seqs, labels


def make_motion(seed, lengths, joints, zero_frac=0.3):
    """MotionMat rows float64 [sum(lengths), joints, 3] with zero_frac of the x / y values zero."""
    rng = np.random.default_rng(seed)
    L = int(sum(lengths))
    mot = rng.uniform(20, 600, (L, joints, 3))
    mot[:, :, 2] = rng.uniform(0, 1, (L, joints))
    mot[:, :, :2][rng.random((L, joints, 2)) < zero_frac] = 0
    return mot


# the sets of tests/golden/shapelet_ref.npz: (seed, clips, D, m, positives, smooth, planted)
GOLDEN_SETS = [
    (0, 10, 1, 2, 3, False, False),
    (1, 12, 3, 5, 4, False, True),
    (2002, 14, 12, 9, 5, True, False),
    (1003, 10, 92, 15, 3, False, True),
    (1004, 16, 3, 15, 6, True, True),
    (5, 12, 12, 2, 4, False, False),
    (6, 10, 92, 5, 5, True, False),
    (7, 14, 1, 9, 4, True, True),
    (5008, 12, 12, 15, 6, False, True),
    (9, 16, 3, 2, 8, True, False),
]
# seeds the generator tried and replaced (by seed + 1000): all named the same winner as the reference
# and float64, but were further from float64 than the reference in one of the two error checks
GOLDEN_REJECTED = [2, 1002, 3, 4, 8, 1008, 2008, 3008, 4008]
GOLDEN_MOTION =[(100, [7, 1, 12], 18), (101, [9, 15], 60)]


# ---------------------------------------------------------------------------------- edge cases
# The cases below take their sizes from the constants of csrc/shapelet.h (T = kShpThreads, the tile
# edges, the limits), so they follow the code.  Every builder is cached and its arrays are shared by
# the tests: never modify them.  Every seeded input is pinned by a digest (EDGE_DIGESTS).
def constants():
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(os.path.dirname(here), "pytorch-openpose_amd", "csrc", "shapelet.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}


K = constants()
T, TR, TC, DC = K["kShpThreads"], K["kShpTR"], K["kShpTC"], K["kShpDC"]
MAXM, MAXD, MAXSEQ = K["kShpMaxM"], K["kShpMaxD"], K["kShpMaxSeq"]
DEFAULT_CANDS, FEAT_ROWS = K["kShpDefaultCands"], K["kFeatRows"]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def _rng(name):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))


def lengths_to_total(rng, total, lo, hi):
    """Lengths of lo .. hi rows that add up to total (the last takes what is left, below hi + lo)."""
    out, left = [], total
    while left:
        n = int(rng.integers(lo, hi + 1))
        if left - n < lo:
            n = left
        out.append(n)
        left -= n
    return out


# ---- 1. sliding_distance over several workgroups: one thread per row, T rows per workgroup
SLIDING_M, SLIDING_D = 4, 3
SLIDING_TOTALS = {"total_T-1": T - 1, "total_T": T, "total_T+1": T + 1, "total_2T+5": 2 * T + 5}
SLIDING_CASES = list(SLIDING_TOTALS) + ["ends_at_T", "straddles_T", "300_short"]


def sliding_lengths(name):
    m, rng = SLIDING_M, _rng("sliding/" + name)
    if name in SLIDING_TOTALS:
        return lengths_to_total(rng, SLIDING_TOTALS[name], m, m + 20)
    if name == "ends_at_T":  # the third sequence's first row is the second workgroup's first thread
        return [T // 2 - 3, T // 2 + 3, 30, 50]
    if name == "straddles_T":  # the second sequence's last window starts at row T - 1; its m - 1
        return [T - 50, 50 + m - 1, 40]  # tail rows, which have no window, are rows T .. T + m - 2
    return [int(v) for v in rng.integers(m, m + 3, 300)]  # seq_of_row's search over 300 sequences


@functools.lru_cache(maxsize=None)
def sliding_case(name):
    """(pattern [m, D], seqs)"""
    rng = _rng("sliding-data/" + name)
    pat = rng.standard_normal((SLIDING_M, SLIDING_D)).astype(F32)
    seqs = [rng.standard_normal((n, SLIDING_D)).astype(F32) for n in sliding_lengths(name)]
    return pat, seqs


# ---- 2. shapelet_score / shapelet_select on synthetic min2 rows
SCORE_LABEL_SIZES = [T - 1, T, T + 1, 2 * T + 3, MAXSEQ]
SCORE_MIRROR_SIZES = [T + 5, MAXSEQ // 2]
SELECT_SIZES = [T - 1, T, T + 1, 2 * T + 7]
SELECT_LABELS = 12
# the members of a full tie, per case: the first must win
SELECT_TIES = {
    "select_tie_%d" % (T - 1): (T - 1, [3, T - 2]),
    "select_tie_%d" % T: (T, [3, T - 1]),
    "select_tie_%d" % (T + 1): (T + 1, [1, T]),            # thread 1 holds the first, thread 0 (second trip) the other
    "select_tie_%d" % (2 * T + 7): (2 * T + 7, [5, 5 + T, 5 + T + 1]),  # one thread's two trips, and its neighbour
    "select_tie_first_past_T": (2 * T + 7, [T + 9, 2 * T + 4]),   # first member >= T, in a higher thread than the other
    "select_tie_lower_thread_later": (2 * T + 7, [7, T + 2]),     # thread 2 holds the later member, thread 7 the first
}
# equal num, the smaller loss later: (n_cand, [(row, loss)]), the last must win
SELECT_NUM_TIE = (2 * T + 7, [(3, 2.0), (T + 3, 1.5), (T + 10, 1.0)])
SCORE_CASES = (["labels_%d" % n for n in SCORE_LABEL_SIZES] + ["all_positive", "one_positive", "all_keys_equal"]
               + ["mirror_%d" % n for n in SCORE_MIRROR_SIZES] + ["select_last_%d" % n for n in SELECT_SIZES]
               + list(SELECT_TIES) + ["select_num_tie"])


def score_pairs(n):
    """The planted pairs of equal keys of a row of n samples: (k, k + T), which one thread meets in
    two trips of its loops, and (k, k + T + 1), which two threads meet; with the value of each."""
    pairs = []
    for i in range(8):
        if 5 * i + T < n:
            pairs.append((5 * i, 5 * i + T, i + 0.5))
        if 5 * i + 1 + T + 1 < n:
            pairs.append((5 * i + 1, 5 * i + 1 + T + 1, 20 + i + 0.5))
    return pairs


def _key_rows(rng, n_cand, n):
    """Keys from 40 small integers, so equal keys abound; row 1 all equal; the planted pairs (unique
    values, halves) in every other row, with the pair's labels different."""
    rows = rng.integers(0, 40, (n_cand, n)).astype(F32)
    rows[1] = 7
    labels = (rng.random(n) < 0.4).astype(np.uint8)
    labels[:2] = (1, 0)
    for i, (a, b, v) in enumerate(score_pairs(n)):
        rows[[0] + list(range(2, n_cand)), a] = v
        rows[[0] + list(range(2, n_cand)), b] = v
        labels[[a, b]] = (i & 1, 1 - (i & 1))
    return rows, labels


def _best_row(labels, loss):
    """A row that separates the labels fully: num = len(labels), loss = `loss` exactly."""
    return np.where(labels != 0, F32(loss * loss), F32(50))


@functools.lru_cache(maxsize=None)
def score_case(name):
    """(min2 [n_cand, n_seq] float32, labels uint8 [n_labels]); n_seq is n_labels or, in the mirror
    cases, 2 n_labels."""
    rng = _rng("score/" + name)
    if name.startswith("labels_"):
        return _key_rows(rng, 6, int(name[7:]))
    if name in ("all_positive", "one_positive"):
        rows, labels = _key_rows(rng, 6, T + 1)
        labels[:] = name == "all_positive"
        labels[T] = 1  # the single positive is a sample of the second trip
        return rows, labels
    if name == "all_keys_equal":
        rows, labels = _key_rows(rng, 3, 2 * T + 3)
        rows[:] = 9
        return rows, labels
    if name.startswith("mirror_"):
        n = int(name[7:])
        first = rng.integers(1, 40, (6, n)).astype(F32)
        delta = rng.integers(-1, 2, (6, n))  # the mirrored copy is smaller, equal, larger
        delta[:, T:T + 3] = (-1, 0, 1)       # each of them at some k >= T
        second = first + delta.astype(F32)
        labels = (rng.random(n) < 0.4).astype(np.uint8)
        labels[:2] = (1, 0)
        return np.concatenate([first, second], axis=1), labels
    labels = np.zeros(SELECT_LABELS, np.uint8)
    labels[rng.permutation(SELECT_LABELS)[:SELECT_LABELS // 2]] = 1
    if name.startswith("select_last_"):
        n_cand, planted = int(name[12:]), [(int(name[12:]) - 1, 1.0)]
    elif name == "select_num_tie":
        n_cand, planted = SELECT_NUM_TIE
    else:
        n_cand, planted = SELECT_TIES[name][0], [(q, 1.0) for q in SELECT_TIES[name][1]]
    rows = rng.integers(2, 41, (n_cand, SELECT_LABELS)).astype(F32)  # every loss at least sqrt(2)
    rows[:, np.nonzero(labels == 0)[0][0]] = 1  # a negative comes first: num is below n_labels
    for q, loss in planted:
        rows[q] = _best_row(labels, loss)
    return rows, labels


@functools.lru_cache(maxsize=None)
def score_expected(name):
    """(nums, losses, winner) of score_case(name) under the statement."""
    rows, labels = score_case(name)
    sc = [candidate_score(row, labels) for row in rows]
    nums, losses = np.array([v[0] for v in sc], np.int32), np.array([v[1] for v in sc], np.float64)
    return nums, losses, select(nums, losses)


# ---- 3. shapelet_mindist: long windows against several blocks, the D chunks, the limits
MINDIST_LONG_M = [TC + 1, 2 * TC + 3, MAXM]
MINDIST_LONG_P = [1, TR - 1, TR, TR + 1, 2 * TC + 3]
MINDIST_CHUNK_D = [DC, 2 * DC, 3 * DC - 1]
MINDIST_REAL = (["long_m%d" % m for m in MINDIST_LONG_M] + ["chunks_D%d" % D for D in MINDIST_CHUNK_D]
                + ["max_D", "workload", "300_seqs"])
MINDIST_CASES = MINDIST_REAL + ["max_seq", "long_tie"]
LONG_TIE_PLACES = (2, TC + 13, 2 * TC + 26)  # one per position block, m apart or more


@functools.lru_cache(maxsize=None)
def mindist_case(name):
    """(seqs, m, cand_seqs)"""
    rng = _rng("mindist/" + name)

    def normals(lengths, D):
        return [rng.standard_normal((n, D)).astype(F32) for n in lengths]

    if name.startswith("long_m"):  # every candidate block count meets every position block count
        m = int(name[6:])
        return normals([m - 1 + P for P in MINDIST_LONG_P], DC + 1), m, list(range(len(MINDIST_LONG_P)))
    if name.startswith("chunks_D"):  # dc == kShpDC on the last chunk, and one short of it
        return normals([3, 10, TC + 5], int(name[8:])), 3, [0, 1, 2]
    if name == "max_D":
        return normals([2, 5, 9], MAXD), 2, [0, 1, 2]
    if name == "workload":  # the shape scripts/shapelet_timing.py times, made small
        return normals([int(v) for v in rng.integers(60, 91, 6)], 92), 25, list(range(6))
    if name == "300_seqs":
        return normals([int(v) for v in rng.integers(5, 9, 300)], 3), 5, [0, 150, 299]
    if name == "max_seq":  # the accepted side of the kShpMaxSeq limit (grid y)
        seqs = [rng.integers(-4, 5, (n, 1)).astype(F32) for n in rng.integers(1, 3, MAXSEQ)]
        return seqs, 1, [0, MAXSEQ // 2, MAXSEQ - 1]
    assert name == "long_tie"  # the same window in three position blocks: the lowest location wins
    m = TC + 5
    seqs = [rng.integers(-4, 5, (n, 3)).astype(F32) for n in (m + 2, LONG_TIE_PLACES[-1] + m + 4)]
    seqs[1] += 50  # nothing else comes near the planted window
    for p in LONG_TIE_PLACES:
        seqs[1][p:p + m] = seqs[0][1:1 + m]
    return seqs, m, [0]


@functools.lru_cache(maxsize=None)
def mindist_expected(name):
    seqs, m, cands = mindist_case(name)
    return mindist(seqs, cands, m)


# ---- 4. opose_shapelet_find across chunks and ties
TIE_FIND_ROWS = (TR + 3, TR + 6 + 1)  # the candidate rows of the two planted windows of find_case("tie")
TIE_FIND_SPLIT = TR + 5   # max_cands that puts them into different chunks, cutting a block of clip 1
CUT_CANDS = 40            # max_cands of the "cut_*" cases: not a multiple of kShpTR
CUT_WINNERS = {"cut_second_block": (0, 36), "cut_after_cut": (0, 45), "cut_next_clip": (2, 5)}
FIND_CASES = ["default_chunks", "tie"] + list(CUT_WINNERS)


def chunk_table(lengths, labels, m, cap):
    """opose_shapelet_find's chunks as engine_shapelet.cpp cuts them: per chunk the table entries
    (clip, first start, starts, first output row)."""
    chunks, cur, nc = [], [], 0
    for i in np.nonzero(labels)[0]:
        P, r = lengths[i] - m + 1, 0
        while r < P:
            if nc == cap:
                chunks.append(cur)
                cur, nc = [], 0
            n = min(TR, P - r, cap - nc)
            cur.append((int(i), r, n, nc))
            nc += n
            r += n
    return chunks + [cur] if cur else chunks


@functools.lru_cache(maxsize=None)
def find_case(name):
    """(seqs, labels, m)"""
    rng = _rng("find/" + name)
    if name == "default_chunks":  # more than kShpDefaultCands candidates: max_cands = 0 cuts a chunk
        labels = np.array([1, 0] * 5, np.uint8)
        n_pos = DEFAULT_CANDS // 5 + 50
        lens = [int(rng.integers(n_pos, n_pos + 21)) if y else int(rng.integers(3, 9)) for y in labels]
        seqs = [rng.integers(-12, 13, (n, 1)).astype(F32) for n in lens]
        seqs[0][:lens[1]] = seqs[1]  # the first candidates are at distance 0 from a negative: no winner at row 0
        return seqs, labels, 1
    if name == "tie":  # one window in two positive clips: candidates TIE_FIND_ROWS tie fully
        m, D = 3, 2
        pat = rng.integers(-4, 5, (m, D)).astype(F32)
        seqs = [rng.integers(20, 30, (TR + 8, D)).astype(F32) for _ in range(5)]
        seqs[1][TR + 3:TR + 3 + m] = pat  # row TR + 3 of clip 1's TR + 6 starts
        seqs[3][1:1 + m] = pat            # row (TR + 6) + 1
        return seqs, np.array([0, 1, 0, 1, 0], np.uint8), m
    # a unique winner at a chosen (clip, start): the exact window there, the window with one element
    # one higher / one lower in the other two positive clips (their distances to the winner are 1 and
    # to each other 2), negatives far from everything
    clip, start = CUT_WINNERS[name]
    m, D = 4, 3
    labels = np.array([1, 0, 1, 1, 0, 0], np.uint8)
    seqs = [rng.integers(20, 30, (n, D)).astype(F32) for n in (m - 1 + 50, 15, m - 1 + 30, m - 1 + 17, 14, 16)]
    pat = rng.integers(-4, 5, (m, D)).astype(F32)
    for i, delta in zip([clip] + [k for k in (0, 2, 3) if k != clip], (0, 1, -1)):
        p = start if i == clip else 3
        seqs[i][p:p + m] = pat
        seqs[i][p + 1, 1] += delta
    return seqs, labels, m


@functools.lru_cache(maxsize=None)
def find_expected(name):
    seqs, labels, m = find_case(name)
    return find(seqs, labels, m)


# ---- 5. features: empty sequences, the fill block's edges, the search, refused carries
FEATURE_CASES = ["empty", "L_rows", "L_rows+1", "300_rows", "carry"]
FEATURE_LENGTHS = {
    "empty": [0, 5, 0, 0, 7, FEAT_ROWS, 3, 0],   # at the start, two in the middle, at the end
    "L_rows": [20, FEAT_ROWS - 20],
    "L_rows+1": [20, FEAT_ROWS - 19],
    "300_rows": [1] * 300,
    # sequence 1 crosses the first fill-block boundary; sequence 2 ends and sequence 3 starts on the second
    "carry": [FEAT_ROWS - 24, FEAT_ROWS - 4, 28, 30],
}


@functools.lru_cache(maxsize=None)
def feature_case(name, joints):
    """(motion float64 [L, joints, 3], lengths)"""
    lengths = FEATURE_LENGTHS[name]
    mot = make_motion(int(_rng("features/%s/%d" % (name, joints)).integers(1 << 31)), lengths, joints)
    if name == "carry":
        R = FEAT_ROWS
        a, b = lengths[0], lengths[0] + lengths[1]  # sequence 1 is rows a .. b - 1; b + lengths[2] == 2 R
        assert a < R < b and b + lengths[2] == 2 * R
        # joint 2, x: non-zero in sequence 0's last row, zero all through sequence 1.  The second fill
        # block's carry is that row: before the sequence, so refused -- the zeros stay
        mot[a - 1, 2, 0] = 123.5
        mot[a:b, 2, 0] = 0
        # joint 3, x: its last non-zero is a row of sequence 1 in the first fill block: accepted
        mot[R - 10, 3, 0] = 234.5
        mot[R - 9:b, 3, 0] = 0
        # joint 4, x: sequence 3 starts on a block boundary with zeros; the carry is sequence 2's last row
        mot[2 * R - 1, 4, 0] = 345.5
        mot[2 * R:2 * R + 3, 4, 0] = 0
        # mode 2, joint 5: a zero at the first row of sequence 3 (r - 1 is another sequence's, r + 1 is not)
        mot[2 * R - 1, 5, :2] = 456.5
        mot[2 * R, 5, :2] = 0
        mot[2 * R + 1, 5, :2] = 56.5
        # mode 2, joint 6: zeros at the last two rows of sequence 2 (r + 1 and r + 2 are another sequence's)
        mot[2 * R - 3, 6, :2] = 67.5
        mot[2 * R - 2:2 * R, 6, :2] = 0
        mot[2 * R:2 * R + 2, 6, :2] = 567.5
    return mot, lengths


# ---- the seeded inputs' digests: a change of a seed or of a recipe shows up here, not as a
# silently different test (tests/test_shapelet_cases.py compares)
def edge_digests():
    out = {}
    for n in SLIDING_CASES:
        pat, seqs = sliding_case(n)
        out["sliding/" + n] = digest(pat, *seqs)
    for n in SCORE_CASES:
        out["score/" + n] = digest(*score_case(n))
    for n in MINDIST_CASES:
        seqs, m, cands = mindist_case(n)
        out["mindist/" + n] = digest(np.array([m] + cands), *seqs)
    for n in FIND_CASES:
        seqs, labels, m = find_case(n)
        out["find/" + n] = digest(np.array([m]), labels, *seqs)
    for n in FEATURE_CASES:
        for joints in (18, 60):
            mot, lengths = feature_case(n, joints)
            out["features/%s/%d" % (n, joints)] = digest(mot, np.array(lengths))
    return out


# (the names carry sizes cut to the constants of csrc/shapelet.h: a changed constant renames cases
# and its new inputs are pinned anew)
EDGE_DIGESTS = {
    'sliding/total_T-1': '91fee08c56c287eb',
    'sliding/total_T': '1682e96d512d9d80',
    'sliding/total_T+1': '9e78dfb066f6a479',
    'sliding/total_2T+5': 'f6c8150b8313bbb9',
    'sliding/ends_at_T': '814da997d0d62d1f',
    'sliding/straddles_T': 'e143654d1f687a34',
    'sliding/300_short': '29db5da2e7706877',
    'score/labels_255': '94f8788d61444f9e',
    'score/labels_256': '5ff9e26a853a0efc',
    'score/labels_257': 'af90689450169d1a',
    'score/labels_515': '9ef22b3be744e2ce',
    'score/labels_4096': '73b6821c8a204ce9',
    'score/all_positive': '6a37958dbb95a406',
    'score/one_positive': '7ad735c24b6ecba9',
    'score/all_keys_equal': '690c7e763e48e5db',
    'score/mirror_261': '6dd33b304b6d6df2',
    'score/mirror_2048': '6d82f8805c977239',
    'score/select_last_255': '6dc49921c035c103',
    'score/select_last_256': 'f4be94e81595b4f6',
    'score/select_last_257': '67e9679db420c32f',
    'score/select_last_519': '20f0bb47777cb095',
    'score/select_tie_255': '0e9f3f2f004244e8',
    'score/select_tie_256': '3bec26f7fe972d49',
    'score/select_tie_257': 'f9da777a10e3407d',
    'score/select_tie_519': '7c3c1a2d885c4a6f',
    'score/select_tie_first_past_T': '9afbeb59c4197429',
    'score/select_tie_lower_thread_later': 'd5b0ae7347e82c4f',
    'score/select_num_tie': 'fc85867f179e87fe',
    'mindist/long_m33': '09b96d5c8c7aa87f',
    'mindist/long_m67': 'b8fa5c2fa0740036',
    'mindist/long_m128': '7c829e6bf934308b',
    'mindist/chunks_D16': 'f3838b98539ca45d',
    'mindist/chunks_D32': '1f97587621431cb1',
    'mindist/chunks_D47': '384145c1a8e7af1d',
    'mindist/max_D': 'b51057bc55496c27',
    'mindist/workload': 'f3e13be61bcca28d',
    'mindist/300_seqs': 'e3fd1a89fa28a0aa',
    'mindist/max_seq': '6bff64d358693ede',
    'mindist/long_tie': 'b69ce35016f331c4',
    'find/default_chunks': '741797923221d3bf',
    'find/tie': '321861c843e9def8',
    'find/cut_second_block': 'ae67a8c776283885',
    'find/cut_after_cut': '1370b598ea900ffa',
    'find/cut_next_clip': '70952dec8b1f84ef',
    'features/empty/18': '4aa5e674ceeebf23',
    'features/empty/60': 'fa0fd7a479c4e887',
    'features/L_rows/18': '16a2c87f2d954a3f',
    'features/L_rows/60': '305aebb797b43db7',
    'features/L_rows+1/18': 'abb27d0e9004b61d',
    'features/L_rows+1/60': '3c0e35ebaa7115bb',
    'features/300_rows/18': '5c24f177568eff33',
    'features/300_rows/60': 'c47f74c8f001a621',
    'features/carry/18': 'f6d54b44ec7c8abd',
    'features/carry/60': '7155a730a2b50504',
}
