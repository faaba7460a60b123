"""Writes tests/golden/shapelet_scan_ref.npz (+ .json): what the reference's
srcmx/DataAugmentation.py computes on the seeded cases of tests/shapelet_scan_cases.py.  The
reference is imported read-only through oracle.gen_golden's shims; its two h5 files are nested
dicts.

    python scripts/gen_shapelet_scan_golden.py

Per case of AUG_CASES (seed, m, featuremode, MaxSegLength): DataAugmentation.AugmentateOneShapelet's
positions and distances per video, for the found window of AUG_CLIP at AUG_LOC with the sigma of
aug_case.  Per record of PATTERN_RECORD_SEEDS: GetShapeletPattern's (levelkey, sigma) lists in modes
0 and 1.  The inputs are regenerated from their seeds by the tests.

A case is kept only when the reference and the NumPy statement give the same positions; a seed that
fails is replaced by seed + 1000 and must then be recorded in AUG_REJECTED, and at most one seed
may need that.  The distances differ by the order of summation: the largest relative difference
over the kept cases, times four, is the tolerance the tests read from the sidecar."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import shapelet_scan_cases as cases  # noqa: E402
from oracle import gen_golden  # noqa: E402


class Tree(dict):
    """A nested dict read like an h5 file: tree["a/b/c"] walks the levels."""

    def __getitem__(self, key):
        node = self
        for part in str(key).split("/"):
            node = dict.__getitem__(node, part)
        return node


def augmenter(cls, shapeletfile, videos, max_seg):
    aug = object.__new__(cls)
    aug.shapeletfile = shapeletfile
    aug.h5motionfile = Tree({"posedata": {"pose": {k: v[:, :18] for k, v in videos.items()}},
                             "handdata": {"hand": {k: v[:, 18:] for k, v in videos.items()}}})
    aug.outputpath = None
    aug.MaxSegLength = max_seg
    return aug


def one_case(cls, seed, m, fm, seg):
    """(same positions, arrays, largest relative distance difference)"""
    videos = cases.aug_videos(seed)
    pattern, sigma = cases.aug_case(seed, m, fm)
    key, a, b = cases.AUG_CLIP
    word = {"sampleidxs": np.array([[0, 30], [a, b]]), "videokeys": ["v1", key],
            "loginfo": ["fx:1-datamode:posehand-featuremode:%d" % fm],
            str(m): {"locs": np.array([3, cases.AUG_LOC], np.int16), "shapelet": np.array([1], np.int16)}}
    N = max(len(v) for v in videos.values())
    aug = augmenter(cls, Tree({"word": word}), videos, N + 1 if seg is None else seg)
    ref = aug.AugmentateOneShapelet("word", (str(m), word[str(m)]["shapelet"], sigma), sigma)
    ours = cases.aug_statement(seed, m, fm, seg)
    same, arrays, rel = True, {}, 0.0
    for vk in videos:
        rp = np.array([p for p, _ in ref[vk]], np.int64)
        rd = np.array([d for _, d in ref[vk]], np.float64)
        op = np.array([p for p, _ in ours[vk]], np.int64)
        od = np.array([d for _, d in ours[vk]], np.float64)
        if not np.array_equal(rp, op):
            same = False
            continue
        nz = rd != 0  # the window's own place is at distance 0 under both
        if not np.array_equal(od[~nz], rd[~nz]):
            same = False
            continue
        if nz.any():
            rel = max(rel, float(np.max(np.abs(rd[nz] - od[nz]) / rd[nz])))
        arrays["%s_pos" % vk], arrays["%s_dist" % vk] = rp, rd
    return same, arrays, rel, float(sigma), sum(len(v) for v in ref.values())


def main():
    gen_golden.install_batch_shims()
    sys.path.insert(0, gen_golden.REF)  # utilmx imports the reference's src.util
    import DataAugmentation
    cls = DataAugmentation.DataAugmentation
    arrays, meta = {}, {"cases": [], "seeds_rejected": cases.AUG_REJECTED}
    worst, stale = 0.0, []
    for seed in cases.AUG_SEEDS:
        use = seed
        while True:
            res = [one_case(cls, use, m, fm, seg) for m, fm, seg in cases.AUG_SETTINGS]
            if all(r[0] for r in res):
                break
            stale.append(use)
            use += 1000
        for (m, fm, seg), (_, arr, rel, sigma, n) in zip(cases.AUG_SETTINGS, res):
            name = cases.aug_name(seed, m, fm, seg)
            for k, v in arr.items():
                arrays["%s_%s" % (name, k)] = v
            arrays["%s_sigma" % name] = np.float32(sigma)
            worst = max(worst, rel)
            meta["cases"].append({"name": name, "seed_used": use, "occurrences": n, "max_rel_diff": rel})
    assert not stale, "seeds %s fail: put seed + 1000 into AUG_SEEDS and the seed into AUG_REJECTED" % stale
    for seed in cases.PATTERN_RECORD_SEEDS:
        rec = cases.pattern_record(seed)
        tree = Tree({"w": {str(m): v for m, v in rec.items()}})
        tree["w"]["loginfo"] = ["not a level key"]
        aug = augmenter(cls, tree, {}, 1)
        for mode in (0, 1):
            got = aug.GetShapeletPattern("w", mode=mode, scale=0.3)
            arrays["pattern%d_mode%d_keys" % (seed, mode)] = np.array([int(k) for k, _, _ in got], np.int32)
            arrays["pattern%d_mode%d_sigmas" % (seed, mode)] = np.array([s for _, _, s in got], np.float32)
    meta["max_rel_diff"] = worst
    meta["dist_rtol"] = 4 * worst
    meta["reference"] = "hitmaxiang/pytorch-openpose srcmx/DataAugmentation.py"
    meta["numpy"], meta["torch"] = np.__version__, torch.__version__
    path = os.path.join(REPO, "tests", "golden", "shapelet_scan_ref.npz")
    np.savez_compressed(path, **arrays)
    with open(path[:-4] + ".json", "w") as f:
        json.dump(meta, f, indent=1)
    print(path, os.path.getsize(path), "bytes; max relative difference", worst)


if __name__ == "__main__":
    main()
