"""Writes tests/golden/shapelet_ref.npz (+ .json): what the reference computes on the seeded cases of
tests/shapelet_cases.py.  The reference is imported read-only through oracle.gen_golden's shims.

    python scripts/gen_shapelet_golden.py

Per set of GOLDEN_SETS: ShapeletMatrixModel.train's shapeindex, locs, dis and score, the float64 row
minima of the winner, and SlidingDistance of the set's first window against its clips (reference
and float64).  Per clip batch of GOLDEN_MOTION: MotionJointFeatures in modes 0 / 1 / 2, clip by clip
on the float32 cast.  The inputs are regenerated from their seeds by the tests.

A set is kept only when the reference, the float32 statement and float64 name the same shapeindex,
candidate and locs, and the statement is no further from float64 than the reference is; a seed that
fails is replaced by seed + 1000, and the seeds tried are written to the sidecar."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import shapelet_cases as sc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def find64(seqs, labels, m):
    """The search in float64 throughout: (shapeindex, cand, locs, dis)."""
    s64 = [np.asarray(y, np.float64) for y in seqs]
    best = None
    for i in np.nonzero(labels)[0]:
        for r in range(len(s64[i]) - m + 1):
            w = s64[i][r:r + m]
            d = np.empty(len(s64))
            loc = np.empty(len(s64), np.int64)
            for j, y in enumerate(s64):
                v = np.array([np.sum(np.square(y[c:c + m] - w)) for c in range(len(y) - m + 1)])
                loc[j] = np.argmin(v)
                d[j] = np.sqrt(v[loc[j]])
            order = np.argsort(d, kind="stable")
            negs = int(len(labels) - labels.sum())
            correct = num = negs
            for k in order:
                correct += 1 if labels[k] else -1
                num = max(num, correct)
            loss = float(np.mean(d[labels == 1]))
            if best is None or num > best[0] or (num == best[0] and loss < best[1]):
                best = (num, loss, int(i), r, loc.copy(), d.copy())
    return best[2], best[3], best[4], best[5]


def one_set(args, mods):
    seqs, labels = sc.make_set(*args)
    m = args[3]
    model = mods["shapeletmodel"].ShapeletMatrixModel()
    model.train([y.copy() for y in seqs], torch.from_numpy(labels.astype(np.int64)), m)
    ours = sc.train(seqs, labels, m)
    i64, c64, loc64, dis64 = find64(seqs, labels, m)
    ref_cand = int(model.locs[model.shapeindex])  # the winner's window lies at distance 0 from itself
    same = (int(model.shapeindex) == ours["shapeindex"] == i64 and ref_cand == ours["cand"] == c64
            and np.array_equal(model.locs, ours["locs"]) and np.array_equal(loc64, ours["locs"])
            and model.score == ours["score"])
    pat = seqs[0][:m]
    sd_ref = np.concatenate([mods["utilmx"].SlidingDistance(pat.copy(), y.copy()) for y in seqs])
    sd64 = np.concatenate([mods["utilmx"].SlidingDistance(pat.astype(np.float64), y.astype(np.float64)) for y in seqs])
    sd_ours = sc.sliding_distance(pat, seqs)
    err = {"dis_ref": float(np.abs(model.dis - dis64).max()), "dis_ours": float(np.abs(ours["dis"] - dis64).max()),
           "sd_ref": float(np.abs(sd_ref - sd64).max()), "sd_ours": float(np.abs(sd_ours - sd64).max())}
    ok = same and err["dis_ours"] <= err["dis_ref"] and err["sd_ours"] <= err["sd_ref"]
    out = {"shapeindex": np.int32(model.shapeindex), "cand": np.int32(ref_cand), "locs": model.locs.astype(np.int16),
           "dis": model.dis.astype(np.float64), "score": np.float64(model.score), "dis64": dis64,
           "sd": sd_ref.astype(np.float32), "sd64": sd64}
    return ok, out, err


def main():
    gen_golden.install_batch_shims()
    sys.path.insert(0, gen_golden.REF)  # utilmx imports the reference's src.util
    import PreprocessingData
    import shapeletmodel
    import utilmx
    mods = {"shapeletmodel": shapeletmodel, "utilmx": utilmx}
    arrays, meta = {}, {"sets": [], "seeds_tried": len(sc.GOLDEN_SETS) + len(sc.GOLDEN_REJECTED),
                        "seeds_rejected": sc.GOLDEN_REJECTED}
    stale = []
    for n, args in enumerate(sc.GOLDEN_SETS):
        args = list(args)
        while True:
            ok, out, err = one_set(tuple(args), mods)
            if ok:
                break
            stale.append(args[0])
            args[0] += 1000
        if args[0] != sc.GOLDEN_SETS[n][0]:
            print("set %d: seed %d of GOLDEN_SETS fails, %d passes" % (n, sc.GOLDEN_SETS[n][0], args[0]))
        for k, v in out.items():
            arrays["set%d_%s" % (n, k)] = v
        meta["sets"].append({"args": args, "max_abs_err_vs_float64": err})
    for n, (seed, lengths, joints) in enumerate(sc.GOLDEN_MOTION):
        mot = sc.make_motion(seed, lengths, joints)
        off = np.cumsum([0] + lengths)
        for mode in (0, 1, 2):
            ref = [PreprocessingData.MotionJointFeatures(mot[a:b].astype(np.float32), featuremode=mode)
                   for a, b in zip(off[:-1], off[1:])]
            ref = np.concatenate(ref)
            assert ref.dtype == np.float32
            assert np.array_equal(ref, sc.motion_features(mot, lengths, mode), equal_nan=True)
            arrays["motion%d_mode%d" % (n, mode)] = ref
    assert not stale, "move the seeds %s to GOLDEN_REJECTED and put their replacements into GOLDEN_SETS" % stale
    meta["reference"] ="hitmaxiang/pytorch-openpose srcmx/shapeletmodel.py, utilmx.py, PreprocessingData.py"
    meta["numpy"], meta["torch"] = np.__version__, torch.__version__
    path = os.path.join(REPO, "tests", "golden", "shapelet_ref.npz")
    np.savez_compressed(path, **arrays)
    with open(path[:-4] + ".json", "w") as f:
        json.dump(meta, f, indent=1)
    print(path, os.path.getsize(path), "bytes;", meta["seeds_tried"], "seeds tried")


if __name__ == "__main__":
    main()
