"""The search over several window lengths in NumPy, and the seeded cases its tests share.

The rule is that of tests/shapelet_cases.py (include/opose.h states it).  The walk
s(r, c) = sum over k ascending of e(r + k, c + k) starts from +0, so its partial sum after m terms
is the s of window length m: one e per candidate clip and one running s give every length as a
snapshot, and the statement below takes them that way.  tests/test_shapelet_lengths_cases.py shows
that each snapshot equals shapelet_cases.mindist / find of that length bit for bit.

Every case builder is cached and its arrays are shared by the tests: never modify them.  The sizes
come from the constants of csrc/shapelet.h (shapelet_cases.K), so they follow the code."""
import functools

import numpy as np

import shapelet_cases as sc

F32 = np.float32
TR, TC, DC, MAXM = sc.TR, sc.TC, sc.DC, sc.MAXM
MAXLENS = sc.K["kShpMaxLens"]
REFERENCE_LENGTHS = list(range(15, 40, 2))  # srcmx/shapeletlearning.py:136 with its defaults


# ---------------------------------------------------------------------------------- the statement
def mindist_lengths(seqs, cand_seqs, m_lens):
    """[(min2, loc)] per length, each as shapelet_cases.mindist gives it for that length: one e per
    candidate clip against all rows of the batch, one running s whose k-th term is added for every
    start and position that still has k + 1 rows, and a snapshot after term m - 1 of each length m."""
    m_lens = list(m_lens)
    assert m_lens and m_lens[0] >= 1 and all(a < b for a, b in zip(m_lens, m_lens[1:]))
    off = np.cumsum([0] + [len(y) for y in seqs])
    cat = np.concatenate([np.asarray(y, F32) for y in seqs])
    mins, locs = [[] for _ in m_lens], [[] for _ in m_lens]
    for i in cand_seqs:
        x = np.asarray(seqs[i], F32)
        e = sc.e_matrix(x, cat)
        n, G = len(x), len(cat)
        s = np.zeros((n, G), F32)
        for k in range(m_lens[-1]):
            s = s[:n - k, :G - k] + e[k:, k:]  # rows r <= n - k - 1, positions g <= G - k - 1
            if k + 1 in m_lens:
                m, l = k + 1, m_lens.index(k + 1)
                mn = np.empty((n - m + 1, len(seqs)), F32)
                lc = np.empty((n - m + 1, len(seqs)), np.int32)
                for j in range(len(seqs)):  # a window that would cross into the next clip is left out
                    mn[:, j], lc[:, j] = sc.first_min(s[:, off[j]:off[j + 1] - m + 1])
                mins[l].append(mn)
                locs[l].append(lc)
    return [(np.concatenate(a), np.concatenate(b)) for a, b in zip(mins, locs)]


def find_lengths(seqs, labels, m_lens):
    """The whole search per length: a list of the dicts shapelet_cases.find returns."""
    labels = np.asarray(labels, np.uint8)
    cands = [i for i in range(len(labels)) if labels[i]]
    out = []
    for m, (min2, loc) in zip(m_lens, mindist_lengths(seqs, cands, m_lens)):
        rows = [(i, r) for i in cands for r in range(len(seqs[i]) - m + 1)]
        scores = [sc.candidate_score(row, labels) for row in min2]
        nums = np.array([v[0] for v in scores], np.int32)
        losses = np.array([v[1] for v in scores], np.float64)
        w = sc.select(nums, losses)
        out.append({"shapeindex": rows[w][0], "cand": rows[w][1], "num": int(nums[w]), "loss": float(losses[w]),
                    "n_cand": len(rows), "dis": np.sqrt(min2[w]), "locs": loc[w].copy(), "min2": min2, "loc": loc,
                    "nums": nums, "losses": losses})
    return out


def length_chunks(lengths, labels, m_lens, cap):
    """opose_shapelet_find_lengths' chunks: shapelet_cases.chunk_table for the shortest length, and
    per chunk and length the entries (clip, first start, starts valid at that length)."""
    out = []
    for chunk in sc.chunk_table(lengths, labels, m_lens[0], cap):
        out.append([[(i, r, min(max(lengths[i] - m + 1 - r, 0), n)) for i, r, n, _ in chunk] for m in m_lens])
    return out


def _rng(name):
    return sc._rng("lengths/" + name)


def _normals(rng, lengths, D):
    return [rng.standard_normal((n, D)).astype(F32) for n in lengths]


# ---------------------------------------------------------------------------------- mindist cases
ONE_LENGTHS = [1, 15, MAXM]
EDGE_LENGTHS = {"short": [1, 2, 3], "long": [3, 4, 9, TC + 1, TC + 8]}
FULL_LENGTHS = {"low": list(range(1, MAXLENS + 1)), "high": list(range(MAXM - MAXLENS + 1, MAXM + 1))}
TIE_LENGTHS = [2, 3, 7]
SUB = sc.T // TR  # threads that share one candidate start's positions: position c falls to thread c % SUB
_TIE_STEP = SUB * -(-TIE_LENGTHS[-1] // SUB)
# the repeated window's positions in the target: all three fall to one thread of the start, two in
# one position block and one in the next, so a thread that kept its last minimum would show
TIE_PLACES = (3, 3 + _TIE_STEP, TC + 3 + _TIE_STEP)
VALIDITY_LENGTHS = [4, 11]
MINDIST_CASES = (["one_m%d" % m for m in ONE_LENGTHS] + ["edges_" + k for k in EDGE_LENGTHS]
                 + ["full_" + k for k in FULL_LENGTHS] + ["reference", "ties", "tail_position", "clip_boundary"])


@functools.lru_cache(maxsize=None)
def mindist_case(name):
    """(seqs, m_lens, cand_seqs)"""
    rng = _rng("mindist/" + name)
    if name.startswith("one_m"):  # one length: the dynamic LDS at its smallest, a usual and its largest size
        m = int(name[5:])
        return _normals(rng, [m, m + 5, m + TC + 2], 4), [m], [0, 1, 2]
    if name.startswith("edges_"):  # a clip with one start at the longest length; block edges that move with m
        lens = EDGE_LENGTHS[name[6:]]
        mx = lens[-1]
        rows = [mx, mx + 1, mx + TR - 1, mx + TR, mx + TR + 1, mx + 2 * TC + 3]
        return _normals(rng, rows, DC + 3), lens, list(range(len(rows)))
    if name.startswith("full_"):  # every running pair in use; "high": the largest LDS
        return _normals(rng, [MAXM, MAXM + TR + 1], 3), FULL_LENGTHS[name[5:]], [0, 1]
    if name == "reference":
        return _normals(rng, [39, 52, 67, 80], 92), REFERENCE_LENGTHS, [0, 1, 2, 3]
    mx = (TIE_LENGTHS if name == "ties" else VALIDITY_LENGTHS)[-1]
    if name == "ties":  # rows 1 .. mx of clip 0 three times in clip 1, nothing else near: exact arithmetic
        seqs = [rng.integers(-4, 5, (n, 3)).astype(F32) for n in (mx + 3, TIE_PLACES[-1] + mx + 5)]
        seqs[1] += 50
        for p in TIE_PLACES:
            seqs[1][p:p + mx] = seqs[0][1:1 + mx]
        return seqs, TIE_LENGTHS, [0]
    # the first m0 rows of clip 0, nearly, in the last m0 rows of clip 1: the short length's location
    # is P_0 - 1, past the long length's last position.  "clip_boundary": clip 2 opens with rows
    # m0 .. mx - 1 of clip 0, so the window of mx rows that starts there and runs on into clip 2
    # would be the long length's minimum
    m0 = VALIDITY_LENGTHS[0]
    seqs = _normals(rng, [mx + 4, mx + TC + 3, mx + 6], 3)
    seqs[1] += F32(40)
    seqs[2] += F32(40)
    seqs[1][-m0:] = seqs[0][:m0] + rng.standard_normal((m0, 3)).astype(F32) * F32(0.01)
    if name == "clip_boundary":
        seqs[2][:mx - m0] = seqs[0][m0:mx]
    else:
        assert name == "tail_position"
    return seqs, VALIDITY_LENGTHS, [0]


@functools.lru_cache(maxsize=None)
def mindist_expected(name):
    seqs, m_lens, cands = mindist_case(name)
    return mindist_lengths(seqs, cands, m_lens)


# ---------------------------------------------------------------------------------- find cases
FIND_LENGTHS = (3, 8, 14, 20)
FIND_SEEDS = (0, 1)
FIND_WINNERS_SEED0 = [(2, 15), (2, 10), (7, 2), (7, 1)]  # they differ between the lengths
FIND_CANDS = (0, 40)


@functools.lru_cache(maxsize=None)
def find_set(seed, mirror=None):
    """(seqs, labels): shapelet_cases.make_set, with the x-mirrored copies appended when asked."""
    seqs, labels = sc.make_set(seed, 12, 5, 20, 4, smooth=True, planted=True, max_extra=30)
    return (seqs + sc.mirror_copies(seqs, mirror) if mirror else seqs), labels


@functools.lru_cache(maxsize=None)
def find_expected(seed, mirror=None):
    seqs, labels = find_set(seed, mirror)
    return find_lengths(seqs, labels, FIND_LENGTHS)


# chunk traps, all with max_cands = CHUNK_CANDS.  A window of the longest length is planted exactly
# in one positive clip and with one element one higher / lower in two others, everything else far.
CHUNK_CANDS = 8
CHUNK_CASES = {
    # lengths, rows per clip, labels, {clip: (start, delta)}
    # clip 0 has P_0 = 24: three chunks, the third (starts 16 .. 23) without a candidate at length 14
    "empty_chunk": ([3, 14], [26, 20, 30, 27, 19], [1, 0, 1, 1, 0], {2: (6, 0), 3: (2, 1)}),
    # the same, the long length's winner in the first chunk: the chunks after the empty one must not take over
    "empty_chunk_early_winner": ([3, 14], [26, 20, 30, 27, 19], [1, 0, 1, 1, 0], {0: (1, 0), 2: (6, 1), 3: (2, -1)}),
    # clip 0 has P_0 = TR + 2; its last entry (starts TR, TR + 1) shares a chunk with clip 2's first
    # starts and is empty at length 6, where clip 2's rows of that chunk begin at row 0, not row 2
    "empty_entry": ([3, 6], [TR + 4, 12, 20, 17, 11], [1, 0, 1, 1, 0], {2: (4, 0), 3: (3, 1), 0: (9, -1)}),
}


@functools.lru_cache(maxsize=None)
def chunk_case(name):
    """(seqs, labels, m_lens)"""
    rng = _rng("chunk/" + name)
    m_lens, rows, labels, places = CHUNK_CASES[name]
    mx, D = m_lens[-1], 3
    seqs = [rng.integers(20, 30, (n, D)).astype(F32) for n in rows]
    pat = rng.integers(-4, 5, (mx, D)).astype(F32)
    for i, (p, delta) in places.items():
        seqs[i][p:p + mx] = pat
        seqs[i][p + mx - 2, 1] += delta
    return seqs, np.array(labels, np.uint8), m_lens


@functools.lru_cache(maxsize=None)
def chunk_expected(name):
    seqs, labels, m_lens = chunk_case(name)
    return find_lengths(seqs, labels, m_lens)
