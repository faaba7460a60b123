"""Timing of the TGCN sign classifier's evaluation: 1,024 clips, V = 55, F_in = 100, H = 256, four
residual blocks, 100 classes, four copies (4,096 samples a forward pass).  Not a gate.

    python scripts/tgcn_timing.py ours  [--reps R]   # opose_tgcn_forward on device tensors
    python scripts/tgcn_timing.py torch [--reps R]   # plain fp32 torch on the same GPU
    python scripts/tgcn_timing.py check              # CPU: the torch restatement against the goldens
    python scripts/tgcn_timing.py ab [--reps R] [--runs N] [--out FILE] [--limit S]

`torch` restates the reference's evaluation loop (cls/TGCN/test_tgcn.py:31-39 over
cls/TGCN/tgcn_model.py) with the same operations: per copy a sliced input, two matmuls and a bias
per layer, batch_norm on running statistics, tanh, the residual, the node mean, a Linear; then the
stack and mean of the copies.  Each of `ours` / `torch` warms up, times R forward passes on the host
clock around work that ends in a device synchronise, and prints one JSON line.  `ab` runs the two in
fresh processes, alternating, N times each, appends every line to FILE and prints the medians and
the ratio.  `ours` also reports the share of the six-product bf16 MFMA ceiling it reaches: the
padded matrix-core work of its launches (64 node rows, k in 32s, columns in 64s, six products) over
the time, against 2.5e15 FLOP/s."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "pytorch-openpose_amd")):
    sys.path.insert(0, p)

B, V, F, H, S, C, COPIES = 1024, 55, 100, 256, 4, 100, 4
BF16_PEAK = 2.5e15


def workload():
    import tgcn_cases as tc
    sd = tc.make_model("timing", V, F, H, C, S)
    X = tc.make_input("timing", B, V, COPIES * F)
    return sd, X


class TorchNet:
    """The reference's model in plain torch, evaluation mode, from a state dict of its keys."""

    def __init__(self, sd, is_resi, device):
        import torch
        self.sd = {k: torch.as_tensor(np.asarray(v), device=device) for k, v in sd.items()}
        self.stages = sum(1 for k in sd if k.startswith("gcbs.") and k.endswith(".gc1.weight"))
        self.is_resi = is_resi

    def layer(self, x, gc, bn):
        import torch
        import torch.nn.functional as Fn
        s = self.sd
        y = torch.matmul(s[gc + ".att"], torch.matmul(x, s[gc + ".weight"])) + s[gc + ".bias"]
        b, n, f = y.shape
        y = Fn.batch_norm(y.view(b, -1), s[bn + ".running_mean"], s[bn + ".running_var"], s[bn + ".weight"],
                          s[bn + ".bias"], False, 0.1, 1e-5).view(b, n, f)
        return torch.tanh(y)

    def forward(self, x):
        import torch
        y = self.layer(x, "gc1", "bn1")
        for i in range(self.stages):
            z = self.layer(self.layer(y, f"gcbs.{i}.gc1", f"gcbs.{i}.bn1"), f"gcbs.{i}.gc2", f"gcbs.{i}.bn2")
            y = z + y if self.is_resi else z
        return torch.nn.functional.linear(torch.mean(y, dim=1), self.sd["fc_out.weight"], self.sd["fc_out.bias"])

    def evaluate(self, X, copies):
        import torch
        stride = X.size()[2] // copies
        outs = [self.forward(X[:, :, i * stride:(i + 1) * stride]) for i in range(copies)]
        return torch.mean(torch.stack(outs, dim=1), dim=1)


def mfma_flops():
    """the padded six-product matrix-core work of one forward pass of `ours`"""
    hp = (H + 63) // 64 * 64
    per = lambda f: 6 * 2 * 64 * hp * ((f + 31) // 32 * 32 + 64)  # noqa: E731  (x W, then att over 64 nodes)
    return B * COPIES * (per(F) + 2 * S * per(H))


def run_ours(reps):
    import torch  # before libopose loads
    from src.tgcn import GCN_muti_att
    sd, X = workload()
    net = GCN_muti_att(F, H, C, num_stage=S, n_nodes=V).load_state_dict(sd)
    Xd = torch.from_numpy(X).cuda()
    for _ in range(3):
        out = net.forward_copies(Xd, COPIES)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = net.forward_copies(Xd, COPIES)
    torch.cuda.synchronize()
    s = (time.perf_counter() - t0) / reps
    return {"what": "ours", "ms_per_forward": s * 1e3, "launches": (1 + 2 * S + 1) * -(-B * COPIES // chunk_samples()),
            "mfma_ceiling_share": mfma_flops() / s / BF16_PEAK, "top1_digest": int(out.argmax(1).sum())}


def chunk_samples():
    return max(4, (1 << 24) // (V * H))  # csrc/engine_tgcn.cpp's default chunk


def run_torch(reps):
    import torch
    sd, X = workload()
    net = TorchNet(sd, True, torch.device("cuda"))
    Xd = torch.from_numpy(X).cuda()
    with torch.no_grad():
        for _ in range(3):
            out = net.evaluate(Xd, COPIES)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = net.evaluate(Xd, COPIES)
        torch.cuda.synchronize()
    s = (time.perf_counter() - t0) / reps
    return {"what": "torch", "ms_per_forward": s * 1e3, "top1_digest": int(out.argmax(1).sum())}


def check():
    """CPU: the torch restatement gives the reference's golden logits (float32 rounding apart)."""
    import torch
    import tgcn_cases as tc
    worst = 0.0
    for name, g in tc.GOLDEN_CASES.items():
        sd, X, ref, _ = tc.golden_case(name)
        with torch.no_grad():
            got = TorchNet(sd, g["is_resi"], torch.device("cpu")).evaluate(torch.from_numpy(X), tc.GOLDEN_COPIES).numpy()
        _, bound, _ = tc.golden_ref(name)
        diff = np.abs(got.astype(np.float64) - ref)
        assert (diff <= 2 * bound).all() and np.array_equal(got.argmax(1), ref.argmax(1)), name
        worst = max(worst, float(diff.max()))
    print(json.dumps({"what": "check", "worst_logit_diff": worst}))


def ab(reps, runs, out, limit):
    lines = {"ours": [], "torch": []}
    for _ in range(runs):
        for what in ("ours", "torch"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), what, "--reps", str(reps)],
                               capture_output=True, text=True, timeout=limit)
            if r.returncode != 0:  # nothing more is started after a failed run
                sys.exit("%s failed (%d):\n%s" % (what, r.returncode, r.stderr[-2000:]))
            line = r.stdout.strip().splitlines()[-1]
            lines[what].append(json.loads(line))
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")
            print(line, flush=True)
    summary = {"what": "summary", "reps": reps, "runs": runs}
    for what, ls in lines.items():
        ms = sorted(l["ms_per_forward"] for l in ls)
        summary[what] = {"median_ms_per_forward": float(np.median(ms)), "min": ms[0], "max": ms[-1]}
    summary["ratio"] = summary["torch"]["median_ms_per_forward"] / summary["ours"]["median_ms_per_forward"]
    summary["same_top1"] = len({l["top1_digest"] for ls in lines.values() for l in ls}) == 1
    line = json.dumps(summary)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("ours", "torch", "check", "ab"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=float, default=200, help="seconds one child process of ab may take")
    a = ap.parse_args()
    if a.what == "check":
        check()
    elif a.what == "ab":
        ab(a.reps, a.runs, a.out, a.limit)
    else:
        print(json.dumps(run_ours(a.reps) if a.what == "ours" else run_torch(a.reps)))
