"""Timing of learning a word's shapelets by gradient descent: 200 clips of 300 frames, D = 92, the 13
window lengths range(15, 40, 2).  Not a gate.

    python scripts/shapelet_net_timing.py ours  [--epochs E]   # one opose_shapelet_net_train call, all lengths
    python scripts/shapelet_net_timing.py torch [--epochs E]   # plain torch on the same GPU, a length after another
    python scripts/shapelet_net_timing.py check                # CPU: the torch restatement against the goldens
    python scripts/shapelet_net_timing.py ab [--epochs E] [--runs R] [--out FILE] [--limit S]

`torch` restates the loop of the reference's ShapeletNetModel.train with the same operations (two
conv1d for the distances, min, Linear, CrossEntropyLoss, torch.optim.Adam).  Each of `ours` / `torch`
warms its shapes up, times one run on the host clock around work that ends in a device
synchronise, and prints one JSON line.  `ab` runs the two in fresh processes, alternating, R times
each, appends every line to FILE and prints the medians with their spread and the ratio."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "pytorch-openpose_amd")):
    sys.path.insert(0, p)

N, T, D, M_LENS, LR = 200, 300, 92, list(range(15, 40, 2)), 0.01
LAUNCHES_PER_EPOCH = 3  # forward, head, query step: csrc/engine_shapelet.cpp


def workload():
    """(X [N, T, D] float32, labels, queries per length, heads [13, 4]): noise clips, the even ones
    holding a 39-frame pattern at a random place; each length's query starts at its first rows
    plus noise."""
    rng = np.random.default_rng(4242)
    X = rng.standard_normal((N, T, D)).astype(np.float32)
    pattern = rng.standard_normal((max(M_LENS), D)).astype(np.float32)
    labels = (np.arange(N) % 2 == 0).astype(np.uint8)
    for i in range(0, N, 2):
        at = int(rng.integers(0, T - len(pattern) + 1))
        X[i, at:at + len(pattern)] = pattern + rng.standard_normal(pattern.shape).astype(np.float32) * 0.05
    queries = [(pattern[:m] + rng.standard_normal((m, D)) * 0.5).astype(np.float32) for m in M_LENS]
    heads = rng.uniform(-1, 1, (len(M_LENS), 4)).astype(np.float32)
    return X, labels, queries, heads


class TorchNet:
    """The reference's model in plain torch: the squared sliding distance as |q|^2 + conv(x^2, 1) -
    2 conv(x, q), its minimum per clip, a Linear(1, 2) and the cross-entropy, stepped by one Adam
    over the query and the head."""

    def __init__(self, query, head, lr, device):
        import torch
        self.q = torch.tensor(np.ascontiguousarray(query.T[None]), device=device, requires_grad=True)  # [1, D, m]
        self.ones = torch.ones_like(self.q)
        self.cls = torch.nn.Linear(1, 2).to(device)
        with torch.no_grad():
            self.cls.weight.copy_(torch.tensor([[head[0]], [head[1]]]))
            self.cls.bias.copy_(torch.tensor([head[2], head[3]]))
        self.opt = torch.optim.Adam([self.q, self.cls.weight, self.cls.bias], lr=lr)
        self.ce = torch.nn.CrossEntropyLoss()

    def distances(self, X):
        import torch
        import torch.nn.functional as F
        return (torch.sum(torch.square(self.q)) + F.conv1d(torch.square(X), self.ones) - 2 * F.conv1d(X, self.q))[:, 0]

    def fit(self, X, Y, epochs):
        import torch
        for _ in range(epochs):
            d = torch.min(self.distances(X), dim=1, keepdim=True)[0]
            loss = self.ce(self.cls(d), Y)
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()

    def locate(self, X):
        import torch
        with torch.no_grad():
            return torch.min(self.distances(X), dim=1)


def run_ours(epochs):
    import torch  # before libopose loads
    from src import shapelet
    X, labels, queries, heads = workload()
    seq = torch.from_numpy(X.reshape(N * T, D)).cuda()
    off = np.arange(N + 1, dtype=np.int64) * T
    qd, hd = [torch.from_numpy(q).cuda() for q in queries], torch.from_numpy(heads).cuda()
    shapelet.shapelet_net_train(seq, off, labels, qd, hd, epochs=20, lr=LR)  # every shape of the timed call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = shapelet.shapelet_net_train(seq, off, labels, qd, hd, epochs=epochs, lr=LR)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    locs = res["locs"].cpu().numpy()
    return {"what": "ours", "seconds": s, "correct": res["correct"].cpu().numpy().tolist(),
            "locs_digest": hashlib.sha256(locs.tobytes()).hexdigest()[:16],
            "us_per_launch": s / epochs / LAUNCHES_PER_EPOCH * 1e6, "launches_per_epoch": LAUNCHES_PER_EPOCH}


def run_torch(epochs):
    import torch
    X, labels, queries, heads = workload()
    dev = torch.device("cuda")
    Xd = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).to(dev)  # [N, D, T]
    Y = torch.from_numpy(labels.astype(np.int64)).to(dev)
    for q, h in zip(queries, heads):  # every length's shapes, not timed
        TorchNet(q, h, LR, dev).fit(Xd, Y, 5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    correct = []
    for q, h in zip(queries, heads):
        net = TorchNet(q, h, LR, dev)
        net.fit(Xd, Y, epochs)
        d, _ = net.locate(Xd)
        with torch.no_grad():
            correct.append(int((torch.max(net.cls(d[:, None]), dim=1)[1] == Y).sum()))
    torch.cuda.synchronize()
    return {"what": "torch", "seconds": time.perf_counter() - t0, "correct": correct}


def check():
    """CPU: the torch restatement lands on the reference's goldens within their tolerance."""
    import torch
    import shapelet_net_cases as nc
    arrays = np.load(os.path.join(REPO, "tests", "golden", "shapelet_net_ref.npz"))
    with open(os.path.join(REPO, "tests", "golden", "shapelet_net_ref.json")) as f:
        atol = json.load(f)["param_atol"]
    worst = 0.0
    for seed in nc.GOLDEN_SEEDS:
        clips, labels, q0 = nc.golden_case(seed)
        X = torch.from_numpy(nc.padded(clips, nc.GOLDEN_T))
        Y = torch.from_numpy(labels.astype(np.int64))
        net = TorchNet(q0, arrays["s%d_head0" % seed], nc.LR, torch.device("cpu"))
        net.fit(X, Y, 50)
        diff = float(np.max(np.abs(net.q.detach().numpy()[0].T.astype(np.float64) - arrays["s%d_q50_f64" % seed])))
        assert np.array_equal(net.locate(X)[1].numpy(), arrays["s%d_loc50" % seed]), seed
        assert diff <= atol, (seed, diff, atol)
        worst = max(worst, diff)
    print(json.dumps({"what": "check", "worst_query_diff": worst, "atol": atol}))


def ab(epochs, runs, out, limit):
    lines = {"ours": [], "torch": []}
    for _ in range(runs):
        for what in ("ours", "torch"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), what, "--epochs", str(epochs)],
                               capture_output=True, text=True, timeout=limit)
            if r.returncode != 0:  # nothing more is started after a failed run
                sys.exit("%s failed (%d):\n%s" % (what, r.returncode, r.stderr[-2000:]))
            line = r.stdout.strip().splitlines()[-1]
            lines[what].append(json.loads(line))
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")
            print(line, flush=True)
    summary = {"what": "summary", "epochs": epochs, "runs": runs}
    for what, ls in lines.items():
        ms = sorted(l["ms_per_epoch"] for l in ls)
        summary[what] = {"median_ms_per_epoch": float(np.median(ms)), "min": ms[0], "max": ms[-1]}
    summary["ratio"] = summary["torch"]["median_ms_per_epoch"] / summary["ours"]["median_ms_per_epoch"]
    line = json.dumps(summary)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("ours", "torch", "check", "ab"))
    ap.add_argument("--epochs", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=float, default=300, help="seconds one child process of ab may take")
    a = ap.parse_args()
    if a.what == "check":
        check()
    elif a.what == "ab":
        ab(a.epochs, a.runs, a.out, a.limit)
    else:
        res = run_ours(a.epochs) if a.what == "ours" else run_torch(a.epochs)
        res.update({"epochs": a.epochs, "lengths": len(M_LENS), "ms_per_epoch": res["seconds"] / a.epochs * 1e3})
        print(json.dumps(res))
