"""Writes tests/golden/shapelet_net_ref.npz (+ .json): what the reference's float32
srcmx/shapeletmodel.py ShapeletNetModel computes on the CPU on the seeded cases of
tests/shapelet_net_cases.py, beside the float64 NumPy statement's values.  The reference is
imported read-only through oracle.gen_golden's shims.

    python scripts/gen_shapelet_net_golden.py

Per seed of GOLDEN_SEEDS: the head a CPU nn.Linear(1, 2) draws after torch.manual_seed(seed), then
the query, head and locations after 1, 5, 50 and 200 epochs of ShapeletNetModel.train at lr 0.01,
and the final DIS, loc and score of Net(X, Y); the float64 statement (shapelet_net_cases.train with
dtype float64, from the same start) at the same epochs.  The clips and the starting query are
regenerated from the seed by the tests.

A case is kept only when the reference's locations equal the float64 statement's at every recorded
epoch and its final score is 1.0; a seed that fails is replaced by seed + 1000 and must then be
recorded in GOLDEN_REJECTED, and at most one seed may need that.  The largest difference between a
reference parameter and the float64 statement's over the kept cases and epochs, times four, is the
tolerance the tests read from the sidecar (the factor covers a different but equally valid float32
order of summation)."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import shapelet_net_cases as nc  # noqa: E402
from oracle import gen_golden  # noqa: E402


def head_of(net):
    w, b = net.CLS.weight.detach().numpy(), net.CLS.bias.detach().numpy()
    return np.array([w[0, 0], w[1, 0], b[0], b[1]], np.float32)


def one_case(model_cls, seed):
    """(kept, arrays, per-epoch largest parameter difference)"""
    clips, labels, q0 = nc.golden_case(seed)
    m, D = q0.shape
    X = torch.from_numpy(nc.padded(clips, nc.GOLDEN_T))
    Y = torch.from_numpy(labels.astype(np.int64))
    torch.manual_seed(seed)
    net = model_cls(shape=(m, D), query=torch.from_numpy(q0.T[None].copy()), lr=nc.LR)
    head0 = head_of(net)
    _, _, want = nc.train(nc.new_state(q0, head0, nc.F64), clips, labels, nc.EPOCHS[-1], nc.LR, nc.GOLDEN_T,
                          nc.F64, record=nc.EPOCHS)
    arrays, diffs, kept, done = {"head0": head0}, {}, True, 0
    for e in nc.EPOCHS:
        with contextlib.redirect_stdout(io.StringIO()):  # train prints its progress
            net.train(X, Y, epochs=e - done)
        done = e
        q = net.getshapelet().numpy().astype(np.float32)
        hd = head_of(net)
        loc = net.localizeshape(X)[0].numpy().astype(np.int32)
        wq, wh, wloc = want[e]
        kept = kept and np.array_equal(loc, wloc)
        diffs[e] = float(max(np.max(np.abs(q.astype(np.float64) - wq)), np.max(np.abs(hd.astype(np.float64) - wh))))
        arrays.update({"q%d" % e: q, "h%d" % e: hd, "loc%d" % e: loc, "q%d_f64" % e: wq, "h%d_f64" % e: wh})
    dis, loc, score = net(X, Y)
    arrays.update({"dis": dis.numpy().astype(np.float32), "loc": loc.numpy().astype(np.int32),
                   "score": np.float64(score)})
    return kept and score == 1.0, arrays, diffs


def main():
    gen_golden.install_batch_shims()
    sys.path.insert(0, gen_golden.REF)  # utilmx imports the reference's src.util
    import shapeletmodel
    arrays, meta = {}, {"cases": [], "seeds_rejected": nc.GOLDEN_REJECTED}
    worst, stale = 0.0, []
    for seed in nc.GOLDEN_SEEDS:
        use = seed
        while True:
            kept, arr, diffs = one_case(shapeletmodel.ShapeletNetModel, use)
            if kept:
                break
            stale.append(use)
            use += 1000
        for k, v in arr.items():
            arrays["s%d_%s" % (seed, k)] = v
        worst = max(worst, max(diffs.values()))
        meta["cases"].append({"seed": seed, "seed_used": use, "max_param_diff": {str(e): v for e, v in diffs.items()}})
    assert not stale, "seeds %s fail: put seed + 1000 into GOLDEN_SEEDS and the seed into GOLDEN_REJECTED" % stale
    meta["max_param_diff"] = worst
    meta["param_atol"] = 4 * worst
    meta["epochs"] = list(nc.EPOCHS)
    meta["reference"] = "hitmaxiang/pytorch-openpose srcmx/shapeletmodel.py ShapeletNetModel (float32, CPU)"
    meta["numpy"], meta["torch"], meta["torch_threads"] = np.__version__, torch.__version__, torch.get_num_threads()
    path = os.path.join(REPO, "tests", "golden", "shapelet_net_ref.npz")
    np.savez_compressed(path, **arrays)
    with open(path[:-4] + ".json", "w") as f:
        json.dump(meta, f, indent=1)
    print(path, os.path.getsize(path), "bytes; largest parameter difference", worst)
    for c in meta["cases"]:
        print(c)


if __name__ == "__main__":
    main()
