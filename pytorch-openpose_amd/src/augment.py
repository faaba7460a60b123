"""Every occurrence of found shapelets across whole videos: the reference's
srcmx/DataAugmentation.py DataAugmentation (GetShapeletPattern, AugmentateOneShapelet,
DataAugmentate) without its h5 files, on src.shapelet.shapelet_scan.

What differs from the reference: records and videos are dicts, not h5 files; every pattern of
every word goes through one scan (per window length when MaxSegLength is given, whose segments
depend on the length); a segment shorter than the pattern contributes nothing (the reference's
SlidingDistance fails on it); distances follow the library's rule (include/opose.h), which sums in
another order than the reference, so they agree to a few float32 roundings, not bit for bit."""
from __future__ import annotations

import math
import re

import numpy as np

from . import shapelet as _shapelet

_LEVEL = re.compile(r"^\d+$")


def _level_keys(word_record):
    """The record's window-length keys in the reference's order: h5py lists a group's keys sorted as
    strings."""
    return sorted((k for k in word_record if _LEVEL.match(str(k))), key=str)


def GetShapeletPattern(word_record, mode=0, scale=0.3):
    """word_record: {m: {"locs", "dists", "shapelet", "score"}} as brute_force_records returns per
    word ("shapelet" int16 [1]: the index of the clip the window was found in; or, for a learned
    shapelet, the [m, D] array itself).  Returns the reference's list of (levelkey, shapelet, sigma),
    levelkey a string.  mode 0: every length, sigma = sorted(dists)[int(len * scale)].  mode 1: the
    one best length by score, then by the smaller average distance, with the reference's arithmetic
    (validnum = int(len * scale), avgdist = sum(dists[:validnum]) / (validnum - 1), sigma =
    dists[validnum - 1]); as there, the single entry is None when no score is above 0."""
    shapelets = []
    if mode == 0:
        for key in _level_keys(word_record):
            rec = word_record[key]
            dists = np.sort(np.asarray(rec["dists"]))
            shapelets.append((str(key), np.asarray(rec["shapelet"]), dists[int(len(dists) * scale)]))
    elif mode == 1:
        best = {"score": 0, "avgdist": float("inf"), "shapelet": None}
        for key in _level_keys(word_record):
            rec = word_record[key]
            score = np.asarray(rec["score"])[0]
            dists = np.sort(np.asarray(rec["dists"]))
            validnum = int(len(dists) * scale)
            avgdist = np.sum(dists[:validnum]) / (validnum - 1)
            sigma = dists[validnum - 1]
            if score > best["score"] or (score == best["score"] and best["avgdist"] > avgdist):
                best = {"score": score, "avgdist": avgdist, "shapelet": (str(key), np.asarray(rec["shapelet"]), sigma)}
        shapelets.append(best["shapelet"])
    return shapelets


def _joints(motion, datamode):
    """The joints MotionJointFeatures reads in this datamode: 'pose' uses the body's 18 only."""
    motion = np.asarray(motion)
    if datamode == "pose" and motion.shape[1] == 60:
        return motion[:, :18]
    return motion


def _features(motion, datamode, featuremode, lengths, handle):
    """MotionJointFeatures of clips concatenated in motion, flattened to [rows, D] float32; the data
    goes through float32 first, as the reference casts it."""
    motion = np.ascontiguousarray(_joints(motion, datamode).astype(np.float32), np.float64)
    if len(motion) == 0:
        return np.zeros((0, 12 if motion.shape[1] == 18 else 92), np.float32)
    out = _shapelet.MotionJointFeatures(motion, datamode, featuremode, lengths=lengths, handle=handle)
    return out.reshape(len(out), -1)


def segments(N, m, MaxSegLength):
    """The reference's segments of a video of N frames for a window of m rows: [(begidx, endidx)]."""
    if MaxSegLength is None:
        return [(0, N)]
    return [(max(i * MaxSegLength - m, 0), min((i + 1) * MaxSegLength, N)) for i in range(math.ceil(N / MaxSegLength))]


def _scan_videos(patterns, sigmas, videos, datamode, featuremode, MaxSegLength, handle, scan=None):
    """Per pattern {videokey: [(position, distance), ...]}.  All patterns of one window length share
    their streams (the videos' segments for that length): one feature call over all segments and one
    scan per length, or one of each for everything when MaxSegLength is None."""
    scan = scan or _shapelet.shapelet_scan
    keys = list(videos)
    results = [None] * len(patterns)
    groups = {}
    for i, p in enumerate(patterns):
        groups.setdefault(None if MaxSegLength is None else len(p), []).append(i)
    for m, members in groups.items():
        segs = [(key, b, e) for key in keys for b, e in segments(len(videos[key]), m, MaxSegLength)]
        lengths = [e - b for _, b, e in segs]
        if segs:
            motion = np.concatenate([_joints(videos[key], datamode)[b:e] for key, b, e in segs])
            feats = _features(motion, datamode, featuremode, lengths, handle)
        else:
            feats = np.zeros((0, np.asarray(patterns[members[0]]).shape[1]), np.float32)
        for i in members:
            results[i] = {key: [] for key in keys}
        if not segs:
            continue
        off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
        res = scan([patterns[i] for i in members], [sigmas[i] for i in members], feats, off, handle=handle)
        occ, pos, dist = (np.asarray(res[k]) for k in ("off", "pos", "dist"))
        for q, i in enumerate(members):
            for s, (key, b, _) in enumerate(segs):
                a, z = occ[q * len(segs) + s], occ[q * len(segs) + s + 1]
                results[i][key].extend((int(b + c), float(d)) for c, d in zip(pos[a:z], dist[a:z]))
    return results


def AugmentateOneShapelet(shapeletdata, sigma, videos, datamode, featuremode, MaxSegLength=None, handle=None):
    """The occurrences of one pattern shapeletdata [m, D] (features, as MotionJointFeatures flattened
    gives them) in every video of videos {videokey: MotionMat [T, 60 | 18, 3]}: {videokey: [(position,
    distance), ...]}.  MaxSegLength None: each video is one stream.  A value: the reference's segments
    begidx = max(i * MaxSegLength - m, 0), endidx = min((i + 1) * MaxSegLength, N); features per
    segment, the walk's state reset per segment, positions offset by begidx, the segments' results
    concatenated (duplicates at the seams included)."""
    pattern = np.ascontiguousarray(shapeletdata, np.float32)
    return _scan_videos([pattern], [sigma], videos, datamode, featuremode, MaxSegLength, handle)[0]


def shapelet_window(word_record, levelkey, shapelet, videos, clips_of_word, datamode, featuremode, handle=None):
    """The [m, D] window of a found shapelet, cut as the reference cuts it: the features of clip
    ranges[index] of video videokeys[index], rows locs[index] : locs[index] + m, index = shapelet[0]."""
    if len(shapelet) != 1:
        return np.ascontiguousarray(shapelet, np.float32)  # a learned shapelet is its own data
    videokeys, ranges = clips_of_word
    rec = word_record[levelkey] if levelkey in word_record else word_record[int(levelkey)]
    index = int(shapelet[0])
    begidx, endidx = (int(v) for v in ranges[index])
    loc = int(np.asarray(rec["locs"])[index])
    clip = np.asarray(videos[videokeys[index]])[begidx:endidx]
    feats = _features(clip, datamode, featuremode, None, handle)
    return np.ascontiguousarray(feats[loc:loc + int(levelkey)])


def DataAugmentate(records, videos, clips, datamode, featuremode, mode=0, scale=0.3, MaxSegLength=None, handle=None):
    """DataAugmentation.DataAugmentate for records {word: word_record} over videos {videokey:
    MotionMat}: {"word/levelkey": {videokey: array}}, each array what the reference stores,
    np.array(list of (position, distance)): float64 [n, 2], or shape (0,) when there is none.

    clips {word: (videokeys, sampleidxs)}: the videokey and [begin, end) frame range of each of the
    word's positive clips.  A found shapelet's record holds index = shapelet[0], which the reference
    uses as an index into these positives' arrays and into locs; that is right when a word's
    positives come first among its samples, as they do in the reference's sampler, and it is kept.

    The patterns of all words go through one shapelet_scan over features computed once (with
    MaxSegLength: one per window length, see the module's note)."""
    names, patterns, sigmas = [], [], []
    for word, word_record in records.items():
        for item in GetShapeletPattern(word_record, mode, scale):
            if item is None:
                raise ValueError("no window length of %r has a score above 0" % (word,))
            levelkey, shapelet, sigma = item
            names.append("%s/%s" % (word, levelkey))
            patterns.append(shapelet_window(word_record, levelkey, shapelet, videos, clips.get(word), datamode,
                                            featuremode, handle))
            sigmas.append(sigma)
    found = _scan_videos(patterns, sigmas, videos, datamode, featuremode, MaxSegLength, handle)
    return {name: {key: np.array(pairs) for key, pairs in res.items()} for name, res in zip(names, found)}
