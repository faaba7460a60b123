"""One timing of finding every occurrence of found shapelets across whole videos: 130 patterns (10
words x the window lengths range(15, 40, 2), D = 92) against 4 videos of 50,000 frames, sigma at
the 5 % quantile of each pattern's distances.  Not a gate.

    python scripts/shapelet_scan_timing.py scan   # one shapelet_scan call
    python scripts/shapelet_scan_timing.py loop   # SlidingDistance per pattern and video + the NumPy walk

`loop` is what the library could do before opose_shapelet_scan.  Each mode prints one JSON line:
the host clock around the work (device data in, occurrences on the host out), the
opose_profile_read kernel times with their flop and byte counts, and a digest of the occurrences,
which the two modes must share."""
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "pytorch-openpose_amd")):
    sys.path.insert(0, p)

import shapelet_scan_cases as cases  # noqa: E402

D, WORDS, M_LENS, VIDEOS, FRAMES, QUANTILE = 92, 10, list(range(15, 40, 2)), 4, 50000, 0.05


def workload():
    """(patterns, videos): videos of a few slow oscillations per column plus noise, so a window has
    look-alikes all along them; a pattern is a window of a video plus a little noise."""
    rng = np.random.default_rng(2024)
    t = np.arange(FRAMES, dtype=np.float32)[:, None]
    videos = []
    for _ in range(VIDEOS):
        freq = rng.uniform(0.02, 0.2, (1, D)).astype(np.float32)
        phase = rng.uniform(0, 6.28, (1, D)).astype(np.float32)
        videos.append((np.sin(t * freq + phase) + rng.standard_normal((FRAMES, D)).astype(np.float32) * 0.3)
                      .astype(np.float32))
    patterns = []
    for w in range(WORDS):
        v, a = videos[w % VIDEOS], int(rng.integers(0, FRAMES - 64))
        for m in M_LENS:
            patterns.append(v[a:a + m] + rng.standard_normal((m, D)).astype(np.float32) * 0.05)
    return patterns, videos


def main(what):
    import torch  # before libopose loads
    from src import shapelet
    patterns, videos = workload()
    h = shapelet.default_handle()
    dev = [torch.from_numpy(v).cuda() for v in videos]
    pdev = [torch.from_numpy(p).cuda() for p in patterns]
    # the thresholds (not timed): per pattern the 5 % quantile of its distances over all videos
    sigmas = []
    for p in pdev:
        d = torch.cat([shapelet.SlidingDistance(p, v) for v in dev])
        sigmas.append(float(torch.sort(d).values[int(len(d) * QUANTILE)]))
    sigmas = np.array(sigmas, np.float32)
    seq = torch.cat(dev)
    off = np.arange(VIDEOS + 1, dtype=np.int64) * FRAMES
    h.profile(True)
    h.profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if what == "scan":
        res = shapelet.shapelet_scan(pdev, sigmas, seq, off)
        occ, pos, dist = (res[k].cpu().numpy() for k in ("off", "pos", "dist"))
    else:
        pairs = [cases.walk(shapelet.SlidingDistance(p, v).cpu().numpy(), s, len(p))
                 for p, s in zip(pdev, sigmas) for v in dev]
        occ, pos, dist = cases.pack(pairs)
    host_s = time.perf_counter() - t0
    h.synchronize()
    prof = h.profile_read()
    digest = hashlib.sha256(occ.tobytes() + pos.tobytes() + dist.tobytes()).hexdigest()[:16]
    print(json.dumps({"what": what, "patterns": len(patterns), "rows": int(off[-1]), "D": D, "host_s": round(host_s, 4),
                      "occurrences": int(occ[-1]), "digest": digest,
                      "kernels": {k: {f: v[f] for f in ("ms", "count", "flops", "bytes") if f in v}
                                  for k, v in prof.items() if isinstance(v, dict) and "ms" in v}}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "scan")
