"""CPU: the host weight packers of the split-bf16 kernels (csrc/x6_pack.cpp) against a NumPy
restatement of the unit layout [slot][piece][4 k-groups][Mpad][8] (csrc/x6_pack.h).

x6_pack.cpp is standard C++, so it is compiled here with a small main (tests/x6_pack_main.cpp)
into a program of its own and run on seeded weights; nothing of the library is loaded.  The
restatement splits by round-to-nearest-even on the bit pattern, and its three pieces must rejoin
to the weight exactly.  Shapes: Cin <= 8 with padded taps (5, 3, 3), a 1x1 head (38, 128, 1),
a ragged last channel group with padded pairs (9, 20, 7), and (9, 20, 3) for Winograd; Mpad 64
and 128."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pytorch-openpose_amd", "csrc")


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("x6_pack") / "x6_pack_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(CSRC, "x6_pack.cpp"),
                    os.path.join(REPO, "tests", "x6_pack_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, mode, w, Mpad):
    cout, cin, ks, _ = w.shape
    wf, of = str(tmp_path / "w.f32"), str(tmp_path / "out.u16")
    w.tofile(wf)
    r = subprocess.run([exe, mode, str(cout), str(cin), str(ks), str(Mpad), wf, of], check=True,
                       capture_output=True, text=True)
    return int(r.stdout), np.fromfile(of, np.uint16)


def _rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint32)


def _bf(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """[3, ...] uint16 pieces of float32 x; they rejoin exactly"""
    h0 = _rne(x)
    r = x - _bf(h0)
    h1 = _rne(r)
    h2 = _rne(r - _bf(h1))
    assert np.array_equal((_bf(h0) + _bf(h1)) + _bf(h2), x)
    return np.stack([h0, h1, h2]).astype(np.uint16)


def _layout(slots, Mpad, cout, cin, source):
    """source(slot, gi) -> (group, [cout, cin] float32 plane) or None for an empty k-group"""
    out = np.zeros((slots, 3, 4, Mpad, 8), np.uint16)
    for s in range(slots):
        for gi in range(4):
            src = source(s, gi)
            if src is None:
                continue
            grp, plane = src
            n = min(8, cin - grp * 8)
            if n > 0:
                out[s, :, gi, :cout, :n] = split3(np.ascontiguousarray(plane[:, grp * 8:grp * 8 + n]))
    return out.ravel()


def _weights(cout, cin, ks, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((cout, cin, ks, ks), dtype=np.float32) * np.float32(np.sqrt(2 / (cin * ks * ks)))
    w.ravel()[::7] *= np.float32(1e-3)  # a spread of exponents
    return w


SHAPES = [(5, 3, 3), (38, 128, 1), (9, 20, 7)]


@pytest.mark.parametrize("Mpad", [64, 128])
@pytest.mark.parametrize("cout,cin,ks", SHAPES)
def test_pack_weights(packer, tmp_path, cout, cin, ks, Mpad):
    w = _weights(cout, cin, ks, 1)
    taps, cin_g = ks * ks, (cin + 7) // 8
    small = cin_g == 1
    nK = (taps + 3) // 4 if small else ((cin_g + 3) // 4) * taps

    def source(c, gi):
        tap, grp = (c * 4 + gi, 0) if small else (c % taps, (c // taps) * 4 + gi)
        return None if tap >= taps else (grp, w.reshape(cout, cin, taps)[:, :, tap])

    got_nK, got = _run(packer, tmp_path, "plain", w, Mpad)
    assert got_nK == nK
    assert np.array_equal(got, _layout(nK, Mpad, cout, cin, source))


@pytest.mark.parametrize("Mpad", [64, 128])
@pytest.mark.parametrize("cout,cin,ks", SHAPES)
def test_pack_weights_pairs(packer, tmp_path, cout, cin, ks, Mpad):
    w = _weights(cout, cin, ks, 2)
    taps, cin_g = ks * ks, (cin + 7) // 8
    nK = (cin_g * taps + 3) // 4

    def source(c, gi):
        q = 4 * c + gi
        return None if q // taps >= cin_g else (q // taps, w.reshape(cout, cin, taps)[:, :, q % taps])

    got_nK, got = _run(packer, tmp_path, "pairs", w, Mpad)
    assert got_nK == nK
    assert np.array_equal(got, _layout(nK, Mpad, cout, cin, source))


@pytest.mark.parametrize("Mpad", [64, 128])
def test_pack_weights_wino(packer, tmp_path, Mpad):
    cout, cin = 9, 20
    w = _weights(cout, cin, 3, 3)
    cin_g = (cin + 7) // 8
    nK = (cin_g * 3 + 3) // 4
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
    wd = w.astype(np.float64)
    # U_v[m][c][ky] = sum_kx G[v][kx] w[m][c][ky][kx], summed left to right in float64, rounded once
    U = ((G[:, None, None, None, 0] * wd[None, ..., 0] + G[:, None, None, None, 1] * wd[None, ..., 1])
         + G[:, None, None, None, 2] * wd[None, ..., 2]).astype(np.float32)

    def source(s, gi):
        q = 4 * (s >> 2) + gi
        return None if q // 3 >= cin_g else (q // 3, U[s & 3, :, :, q % 3])

    got_nK, got = _run(packer, tmp_path, "wino", w, Mpad)
    assert got_nK == nK
    assert np.array_equal(got, _layout(4 * nK, Mpad, cout, cin, source))
