// x6_pack.h — host-side weight packers of the split-bf16 kernels (x6_pack.cpp).  Standard C++
// only, so the packers also build and run without the HIP runtime (tests/test_x6_pack.py).
//
// All three write units of 8 bf16 in the layout [slot][piece][4 k-groups][Mpad][8]: a slot is what
// one 16x16x32 MFMA k-step consumes (a chunk; for Winograd a (chunk, transform) step), piece p of a
// weight is the p-th term of its exact three-way bf16 split, and entries nothing maps to are 0.
#pragma once
#include <cstdint>
#include <vector>

namespace opose {

// x -> three bf16 pieces (round to nearest even of x, of the remainder, of its remainder):
// h[0] + h[1] + h[2] == x exactly
void split3_host(float x, uint16_t (&h)[3]);

// weights [cout][cin][ks][ks] (fp32, physical input channel order).  conv_x6: chunk c, k-group gi =
// (channel group 4 (c / taps) + gi, tap c % taps), or for cin <= 8 (group 0, tap 4c + gi)
void x6_pack_weights(const float* w, int cout, int cin, int ks, int Mpad, int* nK_out, std::vector<uint16_t>& out);
// conv_win_x6, pair order: chunk c, k-group gi = pair q = 4c + gi = (group q / taps, tap q % taps)
void x6_pack_weights_pairs(const float* w, int cout, int cin, int ks, int Mpad, int* nK_out,
                           std::vector<uint16_t>& out);
// conv_wino_x6 (3x3): slot 4c + v holds U_v = sum_kx G[v][kx] w[..][ky][kx] (float64, rounded to
// fp32 once) of pair q = 4c + gi = (group q / 3, kernel row q % 3)
void x6_pack_weights_wino(const float* w, int cout, int cin, int Mpad, int* nK_out, std::vector<uint16_t>& out);

}  // namespace opose
