"""One timing of the search over the reference's window lengths, range(15, 40, 2), on the workload
of scripts/shapelet_timing.py (100 positive and 100 negative clips of 60 to 150 frames, D = 92,
x-mirrored): 13 ShapeletMatrixModel.train calls against one train_lengths call.  Not a gate.

    python scripts/shapelet_lengths_timing.py loop      # 13 train calls, one per length
    python scripts/shapelet_lengths_timing.py lengths   # one train_lengths call

Each prints one JSON line: per run the host clock around the calls and the opose_profile_read
kernel times, and the winners per length (the two modes must agree).  OPOSE_LIB=<an older
libopose.so> runs `loop` on that library, so a baseline and this build can be alternated on one
machine."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "scripts"), os.path.join(REPO, "pytorch-openpose_amd")):
    sys.path.insert(0, p)

from shapelet_timing import D, clips  # noqa: E402

M_LENS = list(range(15, 40, 2))


def main(what, runs=2):
    import torch  # before libopose loads
    from src import shapelet
    seqs, labels = clips()
    h = shapelet.default_handle()
    model = shapelet.ShapeletMatrixModel()
    small, small_labels = seqs[:4] + seqs[-4:], np.array([1] * 4 + [0] * 4, np.uint8)

    def search(X, y):
        if what == "loop":
            return [shapelet.ShapeletMatrixModel().train(X, y, m, mirror="x-mirror") for m in M_LENS]
        return model.train_lengths(X, y, M_LENS, mirror="x-mirror")

    search(small, small_labels)  # load, allocate
    out = {"what": what, "lib": os.environ.get("OPOSE_LIB", "this build"), "clips": len(seqs),
           "rows": int(sum(len(y) for y in seqs)), "D": D, "m_lens": M_LENS}
    for run in range(1, runs + 1):
        h.profile(True)
        h.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        models = search(seqs, labels)
        out["host_s_run%d" % run] = round(time.perf_counter() - t0, 5)
        h.synchronize()
        prof = h.profile_read()
        out["kernels_ms_run%d" % run] = {k: round(v["ms"], 3) for k, v in prof.items()
                                         if isinstance(v, dict) and "ms" in v and k.startswith("shapelet")}
        h.profile(False)
    out["winners"] = [[m.shapeindex, m.cand, m.score] for m in models]
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "lengths")
