"""One timing of the shapelet search at roughly the reference's working size (a reading of
srcmx/shapeletlearning.py's defaults): 100 positive and 100 negative clips of 60 to 150 frames,
D = 92, m = 25, x-mirrored.  A single run each, not a gate.

    python scripts/shapelet_timing.py gpu         # the library: host clock and opose_profile_read
    python scripts/shapelet_timing.py statement   # tests/shapelet_cases.py on this machine's CPU
    python scripts/shapelet_timing.py reference   # the reference's ShapeletMatrixModel.train (its
                                                  # unmirrored model: the mirrored one cannot run)
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "pytorch-openpose_amd")):
    sys.path.insert(0, p)

M, D = 25, 92


def clips(n_pos=100, n_neg=100, seed=2024):
    rng = np.random.default_rng(seed)
    pat = rng.standard_normal((M, D)).astype(np.float32)
    seqs = []
    for i in range(n_pos + n_neg):
        n = int(rng.integers(60, 151))
        x = np.cumsum(rng.standard_normal((n, D)).astype(np.float32) * np.float32(0.3), axis=0, dtype=np.float32)
        if i < n_pos:
            p = int(rng.integers(0, n - M + 1))
            x[p:p + M] = x[p] + pat + rng.standard_normal((M, D)).astype(np.float32) * np.float32(0.1)
        seqs.append(x)
    labels = np.array([1] * n_pos + [0] * n_neg, np.uint8)
    return seqs, labels


def main(what):
    seqs, labels = clips()
    out = {"what": what, "clips": len(seqs), "rows": int(sum(len(y) for y in seqs)), "D": D, "m": M}
    if what == "gpu":
        import torch  # noqa: F401  (before libopose loads)
        from src import shapelet
        h = shapelet.default_handle()
        model = shapelet.ShapeletMatrixModel()
        model.train(seqs[:4] + seqs[-4:], np.array([1] * 4 + [0] * 4, np.uint8), M, mirror="x-mirror")  # load, allocate
        for run in (1, 2):
            h.profile(True)
            h.profile_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.train(seqs, labels, M, mirror="x-mirror")
            out["host_s_run%d" % run] = time.perf_counter() - t0
            h.synchronize()
            prof = h.profile_read()
            out["kernels_ms_run%d" % run] = {k: round(v["ms"], 3) for k, v in prof.items()
                                             if isinstance(v, dict) and "ms" in v and k.startswith("shapelet")}
            h.profile(False)
        out["winner"] = [model.shapeindex, model.cand, model.score]
    elif what == "statement":
        import shapelet_cases as sc
        n = len(labels)
        allseqs = seqs + sc.mirror_copies(seqs, "x-mirror")
        t0 = time.perf_counter()
        best = None
        for i in range(n):
            if not labels[i]:
                continue
            min2, loc = sc.mindist(allseqs, [i], M)
            for r, row in enumerate(min2):
                num, loss = sc.candidate_score(row, labels)
                if best is None or num > best[0] or (num == best[0] and loss < best[1]):
                    best = (num, loss, i, r)
            if i % 10 == 0:
                print("clip %d: %.1f s" % (i, time.perf_counter() - t0), flush=True)
        out["host_s"] = time.perf_counter() - t0
        out["winner"] = [best[2], best[3], best[0] / n]
    else:
        import torch
        from oracle import gen_golden
        gen_golden.install_batch_shims()
        sys.path.insert(0, gen_golden.REF)
        import shapeletmodel
        model = shapeletmodel.ShapeletMatrixModel()
        t0 = time.perf_counter()
        model.train([y.copy() for y in seqs], torch.from_numpy(labels.astype(np.int64)), M)
        out["host_s"] = time.perf_counter() - t0
        out["winner"] = [int(model.shapeindex), int(model.locs[model.shapeindex]), float(model.score)]
        out["threads"] = torch.get_num_threads()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "gpu")
