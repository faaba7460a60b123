"""Writes tests/golden/x6_pinned.json: the SHA-256 of every pinned case's inputs and raw fp32
outputs (tests/test_gpu_x6_pinned.py holds the cases), from the library that is built in the tree
(or OPOSE_LIB=<other .so>), with the commit it was built from.  Needs the GPU.

  python scripts/gen_x6_pinned.py <commit hash of the library> [out.json]

Run it on the commit whose bits are to be kept, before a kernel source changes."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "pytorch-openpose_amd"), REPO):
    sys.path.insert(0, p)


def main():
    import test_gpu_x6_pinned as t
    from src import _native
    commit = sys.argv[1]
    assert len(commit) == 40, "the full commit hash of the library's source"
    path = sys.argv[2] if len(sys.argv) > 2 else t.PINNED
    handle = _native.Handle(0)
    cases = {}
    for cid in sorted(t.CASES):
        inputs, run = t.CASES[cid](_native, handle)
        cases[cid] = {"inputs": t.digest(inputs), "outputs": t.digest(run())}
        print(cid, cases[cid]["outputs"][:16], flush=True)
    with open(path, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(cases), "cases")


if __name__ == "__main__":
    main()
