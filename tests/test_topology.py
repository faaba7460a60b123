"""CPU: the network descriptions of the host runtime (csrc/topology.cpp) against the oracle's
restatement of the reference topology (oracle/network.py).

topology.cpp is standard C++, so it is compiled here with a small main (tests/topology_main.cpp)
into a program of its own that prints both descriptions; nothing of the library is loaded."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pytorch-openpose_amd", "csrc")
sys.path.insert(0, REPO)


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    """net -> {"groups": [...], "layer": [[...], ...], "trunk": ..., "shared": ..., "cmap": [...]}"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("topology") / "topology_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(CSRC, "topology.cpp"),
                    os.path.join(REPO, "tests", "topology_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    nets = {}
    for line in out.splitlines():
        key, *vals = line.split()
        if key == "net":
            cur = nets[vals[0]] = {"layer": [], "trunk": [], "shared": []}
        elif key in ("groups", "cmap"):
            cur[key] = [int(v) for v in vals]
        else:
            cur[key].append([vals[0]] + [v if key == "shared" else int(v) for v in vals[1:]])
    return nets


@pytest.mark.parametrize("net", ["body", "hand"])
def test_state_dict_order_is_the_oracles(desc, net):
    from oracle.network import conv_specs
    assert [tuple(r) for r in desc[net]["layer"]] == [tuple(e) for e in conv_specs(net)]


@pytest.mark.parametrize("net", ["body", "hand"])
def test_trunk_levels_and_pools(desc, net):
    trunk = desc[net]["trunk"]
    n = {"body": 12, "hand": 15}[net]
    assert [r[0] for r in trunk] == [r[0] for r in desc[net]["layer"][:n]]
    assert [r[0] for r in trunk if r[2]] == ["conv1_2", "conv2_2", "conv3_4"]
    assert [r[1] for r in trunk] == [0, 0, 1, 1, 2, 2, 2, 2] + [3] * (n - 8)
    # as the layer names' prefixes give them
    assert all(r[1] == {"conv1_": 0, "conv2_": 1, "conv3_": 2}.get(r[0][:6], 3) for r in trunk)


def test_shared_pairs(desc):
    bases = ["conv5_1_CPM"] + [f"Mconv1_stage{s}" for s in range(2, 7)]
    assert desc["body"]["shared"] == [[b + "_L1+L2", b + "_L1", b + "_L2"] for b in bases]
    assert desc["hand"]["shared"] == []


def test_cmap_and_group_layout(desc):
    assert desc["body"]["cmap"] == [c if c < 38 else c + 2 if c < 57 else c + 7 for c in range(185)]
    assert desc["hand"]["cmap"] == [c if c < 22 else c + 2 for c in range(150)]
    assert desc["body"]["groups"] == [24, 32, 128]
    assert desc["hand"]["groups"] == [19, 16, 64]
