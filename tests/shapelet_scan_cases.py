"""The shapelet scan rule in NumPy, and the seeded cases the scan tests and
scripts/gen_shapelet_scan_golden.py share (include/opose.h states the rule too).

Distances are those of shapelet_cases (float32, one rounding per operation, e over d ascending, s
over k ascending, dist = sqrt(s)).  For pattern p (m rows) and stream j, position c exists when
c + m <= len_j; it is a hit when dist < sigma_p (float32, strict).  The occurrences of a pair come
from one walk over its hits, c ascending, with the state (pre, last entry):

    first hit:                                  append (c, dist), pre = c
    later hit with 2 * (c - pre) > m:           append (c, dist), pre = c
    else dist < the last entry's dist (strict): the last entry becomes (c, dist), pre = c
    else:                                       nothing, pre stays

The cases take their sizes from the constants of csrc/shapelet.h.  Every builder is cached and its
arrays are shared by the tests: never modify them."""
import functools

import numpy as np

import shapelet_cases as sc
from shapelet_cases import F32, K, _rng

TC, PG, THREADS, LDS_BYTES = K["kScanTC"], K["kScanPG"], K["kScanThreads"], K["kScanLdsBytes"]
MAXPAT, MAXPAIRS, DEFAULT_PATS = K["kScanMaxPat"], K["kScanMaxPairs"], K["kScanDefaultPats"]
MAXM, MAXD, MAXSEQ = sc.MAXM, sc.MAXD, sc.MAXSEQ
PT = PG // (THREADS // TC)   # patterns one thread accumulates: a group's thread sets split there
STEP_ROWS = 64 * 64          # rows the pick walk covers per step (64 mask words of 64 rows)


# ---------------------------------------------------------------------------------- the statement
def walk(dist, sigma, m):
    """The occurrences of one pair from its positions' distances dist float32 [P]: [(c, dist)]."""
    dist = np.asarray(dist, F32)
    out, pre = [], None
    for c in np.nonzero(dist < F32(sigma))[0]:  # a NaN or non-positive sigma: no hits
        d = dist[c]
        if pre is None or 2 * (int(c) - pre) > m:
            out.append((int(c), d))
            pre = int(c)
        elif d < out[-1][1]:
            out[-1] = (int(c), d)
            pre = int(c)
    return out


def pack(per_pair):
    """Lists of (c, dist) per pair, in order -> (off int64, pos int32, dist float32)."""
    off = np.concatenate(([0], np.cumsum([len(v) for v in per_pair]))).astype(np.int64)
    flat = [e for v in per_pair for e in v]
    return off, np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], F32)


def distances(pattern, y):
    """dist of every position of stream y for pattern [m, D]: float32 [max(len(y) - m + 1, 0)]."""
    m = len(pattern)
    if len(y) < m:
        return np.zeros(0, F32)
    return np.sqrt(sc.s_matrix(pattern, y, m)[0])


def scan(patterns, sigmas, seqs):
    """opose_shapelet_scan: (off [n_pat * n_seq + 1], pos, dist), pattern-major."""
    return pack([walk(distances(np.asarray(p, F32), np.asarray(y, F32)), s, len(p))
                 for p, s in zip(patterns, sigmas) for y in seqs])


def pick(dist, off, m, sigma):
    """opose_debug_shapelet_pick: dist [L] holds one value per row; a stream's last m - 1 rows are
    no positions."""
    return pack([walk(dist[a:max(b - m + 1, a)], sigma, m) for a, b in zip(off[:-1], off[1:])])


def lds_bytes(m_max, D):
    """The LDS tile of shapelet_scan_dist: kScanTC + m_max - 1 rows of D | 1 floats."""
    return 4 * (TC + m_max - 1) * (D | 1)


def takes_lds_path(patterns):
    return lds_bytes(max(len(p) for p in patterns), np.asarray(patterns[0]).shape[1]) <= LDS_BYTES


# ---------------------------------------------------------------------------------- pick cases
# dictated distance profiles: (dist [L], off, m, sigma, expected per stream or None)
FAR, SIGMA = F32(9.0), F32(1.0)
PICK_CASES = ["even_m", "odd_m", "falling_run", "rising_run", "equal_run", "at_sigma", "word_boundary", "step_boundary",
              "all_hits", "no_hits", "mid_word", "two_in_word", "empty_and_short"]


def _profile(lengths, hits):
    """Streams of the given lengths, FAR everywhere except hits {(stream, c): dist}."""
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    dist = np.full(int(off[-1]), FAR, F32)
    for (j, c), d in hits.items():
        assert 0 <= c < lengths[j]
        dist[off[j] + c] = F32(d)
    return dist, off


@functools.lru_cache(maxsize=None)
def pick_case(name):
    """(dist, off, m, sigma, expected): expected is the hand-derived list of (c, dist) per stream, or
    None where only the statement says."""
    rng = _rng("scan-pick/" + name)
    if name == "even_m":  # m = 8: a hit m / 2 after pre is not new and replaces only when smaller; m / 2 + 1 is new
        dist, off = _profile([40, 40], {(0, 10): .5, (0, 14): .4, (0, 18): .6, (0, 19): .7,
                                        (1, 10): .5, (1, 14): .6, (1, 15): .6})
        return dist, off, 8, SIGMA, [[(14, .4), (19, .7)], [(10, .5), (15, .6)]]
    if name == "odd_m":  # m = 9: a gap of 4 is not new (8 > 9 fails), a gap of 5 is
        dist, off = _profile([40, 40], {(0, 10): .5, (0, 14): .6, (0, 15): .6,
                                        (1, 10): .5, (1, 14): .4, (1, 18): .3, (1, 23): .9})
        return dist, off, 9, SIGMA, [[(10, .5), (15, .6)], [(18, .3), (23, .9)]]
    if name in ("falling_run", "rising_run", "equal_run"):  # a run of 2 m + 4 hits, m = 6 and m = 7
        hits, want = {}, []
        for j, m in enumerate((6, 7)):
            n = 2 * m + 4
            vals = {"falling_run": np.linspace(.9, .1, n), "rising_run": np.linspace(.1, .9, n),
                    "equal_run": np.full(n, .5)}[name].astype(F32)
            for i in range(n):
                hits[(j, 5 + i)] = vals[i]
            if name == "falling_run":  # the entry is dragged to the run's end
                want.append([(5 + n - 1, vals[-1])])
            else:  # the first hit, then a new entry every floor(m / 2) + 1; never a replacement
                want.append([(5 + i, vals[i]) for i in range(0, n, m // 2 + 1)])
        # one m per call: the two streams are two cases, told apart by the caller
        dist, off = _profile([60, 60], hits)
        return dist, off, (6, 7), SIGMA, want
    if name == "at_sigma":  # dist == sigma is no hit; one float32 below is
        below = np.nextafter(SIGMA, F32(0))
        dist, off = _profile([30], {(0, 3): SIGMA, (0, 12): below, (0, 20): SIGMA})
        return dist, off, 4, SIGMA, [[(12, below)]]
    if name == "word_boundary":  # a falling run over rows 60 .. 70: two mask words
        vals = np.linspace(.9, .1, 11).astype(F32)
        dist, off = _profile([100], {(0, 60 + i): vals[i] for i in range(11)})
        return dist, off, 30, SIGMA, [[(70, vals[-1])]]
    if name == "step_boundary":  # a stream of 64 * 64 + 70 rows, a falling run over the walk's step
        vals = np.linspace(.9, .1, 12).astype(F32)
        dist, off = _profile([STEP_ROWS + 70], {(0, STEP_ROWS - 6 + i): vals[i] for i in range(12)})
        dist[5], dist[STEP_ROWS + 60] = F32(.5), F32(.25)
        return dist, off, 8, SIGMA, [[(5, F32(.5)), (STEP_ROWS + 5, vals[-1]), (STEP_ROWS + 60, F32(.25))]]
    if name == "all_hits":
        dist = rng.uniform(.1, .9, 300).astype(F32)
        return dist, np.array([0, 300], np.int64), 5, SIGMA, None
    if name == "no_hits":
        dist, off = _profile([70, 90], {})
        return dist, off, 5, SIGMA, [[], []]
    if name == "mid_word":  # stream 1 starts at row 37; stream 0's last m - 1 rows are below sigma and no positions
        m = 6
        dist, off = _profile([37, 50], {(0, 32): .1, (0, 33): .1, (0, 34): .1, (0, 35): .1, (0, 36): .1,
                                        (0, 31): .7, (1, 0): .6, (1, 2): .5})
        return dist, off, m, SIGMA, [[(31, .7)], [(2, .5)]]
    if name == "two_in_word":
        dist, off = _profile([20, 25], {(0, 3): .5, (0, 15): .4, (1, 0): .3, (1, 19): .2})
        return dist, off, 4, SIGMA, [[(3, .5), (15, .4)], [(0, .3), (19, .2)]]
    assert name == "empty_and_short"  # streams of 0, m - 1 and m rows between ordinary ones
    m = 5
    dist, off = _profile([0, 12, m - 1, 0, m, 9], {(1, 2): .5, (2, 0): .1, (4, 0): .3, (4, 1): .1, (5, 4): .2})
    return dist, off, m, SIGMA, [[], [(2, .5)], [], [], [(0, .3)], [(4, .2)]]


def pick_calls(name):
    """The calls of a pick case: [(dist, off, m, sigma, expected or None)], one per window length."""
    dist, off, m, sigma, want = pick_case(name)
    if not isinstance(m, tuple):
        return [(dist, off, m, sigma, want)]
    # per length: the stream made for that length alone
    return [(dist[off[j]:off[j + 1]], np.array([0, off[j + 1] - off[j]], np.int64), mj, sigma, [want[j]])
            for j, mj in enumerate(m)]


# ---------------------------------------------------------------------------------- distance cases
DIST_CASES = ["tile_edges", "one_pattern", "full_group", "group_plus_one", "mixed_lengths", "D1", "D4", "D7", "D92",
              "lds_fits", "lds_over", "global_max", "integer_planted", "long_stream", "chunks"]


def _quantile_sigmas(patterns, seqs, q):
    """Per pattern the q-quantile of its distances over all streams (an exact distance value: the
    position that holds it is no hit), or 1 when it has no position."""
    out = []
    for p in patterns:
        d = np.concatenate([distances(p, y) for y in seqs])
        out.append(np.sort(d)[int(len(d) * q)] if len(d) else F32(1))
    return np.array(out, F32)


def _smooth(rng, n, D):
    return np.cumsum(rng.standard_normal((n, D)).astype(F32) * F32(0.3), axis=0, dtype=F32)


def _cut(rng, seqs, m):
    """A window of m rows cut from a stream long enough, plus a little noise."""
    j = [i for i, y in enumerate(seqs) if len(y) >= m][0]
    a = int(rng.integers(0, len(seqs[j]) - m + 1))
    return seqs[j][a:a + m] + rng.standard_normal((m, seqs[j].shape[1])).astype(F32) * F32(0.05)


@functools.lru_cache(maxsize=None)
def dist_case(name):
    """(patterns, sigmas, seqs)"""
    rng = _rng("scan-dist/" + name)

    def streams(lengths, D):
        return [_smooth(rng, n, D) for n in lengths]

    def finish(pat_lengths, seqs, q=0.2):
        pats = [_cut(rng, seqs, m) for m in pat_lengths]
        return pats, _quantile_sigmas(pats, seqs, q), seqs

    if name == "tile_edges":  # stream lengths around the tile, and m - 1, m and 0 rows mixed in
        m = 7
        return finish([m], streams([TC - 1, 0, TC, m - 1, TC + 1, m, 2 * TC + 1, 0], 5))
    if name == "one_pattern":
        return finish([11], streams([90, 40], 3))
    if name == "full_group":  # kScanPG patterns: both thread sets full
        return finish([3 + (i * 5) % 11 for i in range(PG)], streams([150, 33, 70], 3))
    if name == "group_plus_one":  # a second group with one pattern and kScanPG - 1 fillers
        return finish([3 + (i * 7) % 13 for i in range(PG + 1)], streams([150, 33, 70], 3))
    if name == "mixed_lengths":  # one group, m = 1, 2, 37 and kShpMaxM: streams shorter than some of them
        return finish([37, 1, MAXM, 2], streams([MAXM + 40, 36, 1, MAXM, 2 * TC + 9], 4))
    if name in ("D1", "D4", "D7", "D92"):  # the feature loop's unrolled blocks: none, whole, partial, the workload's
        return finish([9, 15, 4], streams([TC + 30, 60], int(name[1:])))
    if name in ("lds_fits", "lds_over"):  # D = 92: the longest window the LDS tile takes, and one more
        m = max(v for v in range(1, MAXM + 1) if lds_bytes(v, 92) <= LDS_BYTES) + (name == "lds_over")
        return finish([m, 15], streams([m + 50, m - 1, m], 92))
    if name == "global_max":  # D = kShpMaxD, m = kShpMaxM: the global-read path at the limits
        return finish([MAXM, 3], streams([MAXM + 12, 5], MAXD))
    if name == "integer_planted":  # exact arithmetic: dist == 0 at the copies, perfect squares elsewhere
        seqs = [rng.integers(-3, 4, (n, 2)).astype(F32) for n in (TC + 20, 50)]
        pat = seqs[0][30:36].copy()
        seqs[1][10:16] = pat
        seqs[0][TC - 3:TC + 3] = pat  # a copy across the tile edge
        seqs[1][25:31], seqs[1][38:44] = pat, pat
        seqs[1][25, 0] += 3           # a copy at distance 3 exactly (s = 9), and one at 2 (s = 4)
        seqs[1][40, 1] += 2
        pats = [pat, pat.copy(), pat.copy()]
        # sigma 0.5: only the exact copies; 3: also the copy at 2, not the one at 3; 0: nothing
        return pats, np.array([0.5, 3, 0], F32), seqs
    if name == "long_stream":  # crosses the pick walk's 64-word step; periodic, so the hits come all along it
        seqs = [(np.sin(np.arange(n)[:, None] / F32(7) + np.arange(2)[None, :])
                 + rng.standard_normal((n, 2)) * 0.1).astype(F32) for n in (STEP_ROWS + 70, 100)]
        return finish([5, 12], seqs, q=0.05)
    assert name == "chunks"  # max_pats 1, 2 and the default must agree
    return finish([9, 4, 30, 15, 4], streams([200, 3, 77], 6))


@functools.lru_cache(maxsize=None)
def dist_expected(name):
    return scan(*dist_case(name))


# ---------------------------------------------------------------------------------- reference cases
# tests/golden/shapelet_scan_ref.npz: DataAugmentation.AugmentateOneShapelet on seeded videos
AUG_VIDEO_FRAMES = {"v0": 150, "v1": 97, "v2": 260}
AUG_SEEDS = [0, 1, 2, 3, 4, 5]
AUG_REJECTED = []  # seeds replaced by seed + 1000 (none)
AUG_SETTINGS = [(9, 0, None), (15, 1, None), (24, 2, None), (15, 1, 64)]  # (m, featuremode, MaxSegLength)
AUG_CLIP = ("v0", 40, 110)  # the positive clip the found window is cut from: video, [begin, end)
AUG_LOC = 12                # the window's start within that clip
AUG_QUANTILE = 0.15         # sigma: this quantile of the window's distances over the whole videos
AUG_CASES = [(seed, m, fm, seg) for seed in AUG_SEEDS for m, fm, seg in AUG_SETTINGS]


@functools.lru_cache(maxsize=None)
def aug_videos(seed):
    """{videokey: MotionMat float64 [T, 60, 3]}: smooth random walks around a standing pose, a few
    x / y values zero (missing joints), as the motion files hold them."""
    rng = np.random.default_rng(7000 + seed)
    out = {}
    for key, T in AUG_VIDEO_FRAMES.items():
        base = rng.uniform(100, 500, (1, 60, 2))
        base[0, 0, 1], base[0, 1, 1] = 100.0, 180.0  # nose above neck: the scale never comes near 0
        xy = base + np.cumsum(rng.standard_normal((T, 60, 2)) * 2.0, axis=0)
        # a slow common sway, so that windows far apart in time look alike and hits come in runs
        xy += 25.0 * np.sin(np.arange(T)[:, None, None] / 9.0 + rng.uniform(0, 6, (1, 60, 2)))
        mot = np.concatenate([xy, rng.uniform(0.2, 1.0, (T, 60, 1))], axis=2)
        zero = rng.random((T, 60)) < 0.02
        zero[:, :2] = False
        mot[zero, :2] = 0
        out[key] = mot
    return out


def aug_features(motion, featuremode):
    """MotionJointFeatures on the float32 cast, flattened: what the reference slides over."""
    f = sc.motion_features(np.asarray(motion).astype(F32), None, featuremode)
    return f.reshape(len(f), -1)


@functools.lru_cache(maxsize=None)
def aug_case(seed, m, featuremode):
    """(pattern [m, 92], sigma): the window of AUG_CLIP at AUG_LOC, and its threshold."""
    videos = aug_videos(seed)
    key, a, b = AUG_CLIP
    pattern = np.ascontiguousarray(aug_features(videos[key][a:b], featuremode)[AUG_LOC:AUG_LOC + m])
    d = np.concatenate([distances(pattern, aug_features(v, featuremode)) for v in videos.values()])
    return pattern, np.sort(d)[int(len(d) * AUG_QUANTILE)]


def aug_statement(seed, m, featuremode, seg):
    """AugmentateOneShapelet under the statement: {videokey: [(position, dist)]}."""
    import math
    pattern, sigma = aug_case(seed, m, featuremode)
    out = {}
    for key, mot in aug_videos(seed).items():
        N = len(mot)
        segs = [(0, N)] if seg is None else [(max(i * seg - m, 0), min((i + 1) * seg, N))
                                             for i in range(math.ceil(N / seg))]
        out[key] = [(a + c, d) for a, b in segs
                    for c, d in walk(distances(pattern, aug_features(mot[a:b], featuremode)), sigma, m)]
    return out


def aug_name(seed, m, featuremode, seg):
    return "s%d_m%d_f%d_%s" % (seed, m, featuremode, "whole" if seg is None else "seg%d" % seg)


# two seeded word records for GetShapeletPattern: {m: {"locs", "dists", "shapelet", "score"}}
PATTERN_RECORD_SEEDS = [11, 12]


@functools.lru_cache(maxsize=None)
def pattern_record(seed):
    rng = np.random.default_rng(seed)
    n_pos = 17
    rec = {}
    for m in range(15, 40, 2):
        rec[m] = {"locs": rng.integers(0, 30, n_pos).astype(np.int16),
                  "dists": rng.uniform(0.5, 9.0, n_pos).astype(F32),
                  "shapelet": np.array([rng.integers(0, n_pos)]).astype(np.int16),
                  # few distinct scores: mode 1 has ties to break by the average distance
                  "score": np.array([rng.integers(6, 9) / 10]).astype(F32)}
    return rec
