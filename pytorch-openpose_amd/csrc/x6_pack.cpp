// x6_pack.cpp — host-side weight packers of the split-bf16 kernels: one writer of the unit layout
// (x6_pack_units) and the three k orders as mappings over it (x6_pack.h).
#include "x6_pack.h"

#include <cstring>

namespace opose {

namespace {
uint32_t bf16_rne_host(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
float bf16_value(uint32_t h) {
    const uint32_t u = h << 16;
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

// out[slot][piece][gi][m][e] for m < cout; source(slot, gi) gives the k-group's reader
// (m, e, float& x) -> false where the entry is empty
template <class Source>
void x6_pack_units(int slots, int cout, int Mpad, std::vector<uint16_t>& out, Source&& source) {
    out.assign((size_t)slots * 12 * Mpad * 8, 0);
    for (int s = 0; s < slots; ++s)
        for (int gi = 0; gi < 4; ++gi) {
            const auto value = source(s, gi);
            for (int m = 0; m < cout; ++m)
                for (int e = 0; e < 8; ++e) {
                    float x;
                    if (!value(m, e, x)) continue;
                    uint16_t h[3];
                    split3_host(x, h);
                    for (int pc = 0; pc < 3; ++pc) out[(((size_t)s * 12 + pc * 4 + gi) * Mpad + m) * 8 + e] = h[pc];
                }
        }
}
}  // namespace

void split3_host(float x, uint16_t (&h)[3]) {
    const uint32_t h0 = bf16_rne_host(x);
    const float r = x - bf16_value(h0);
    const uint32_t h1 = bf16_rne_host(r);
    h[0] = (uint16_t)h0;
    h[1] = (uint16_t)h1;
    h[2] = (uint16_t)bf16_rne_host(r - bf16_value(h1));
}

void x6_pack_weights(const float* w, int cout, int cin, int ks, int Mpad, int* nK_out, std::vector<uint16_t>& out) {
    const int taps = ks * ks, cin_g = (cin + 7) / 8;
    const bool small = cin_g == 1;
    const int nK = *nK_out = small ? (taps + 3) / 4 : ((cin_g + 3) / 4) * taps;
    x6_pack_units(nK, cout, Mpad, out, [=](int c, int gi) {
        const int tap = small ? c * 4 + gi : c % taps, grp = small ? 0 : (c / taps) * 4 + gi;
        return [=](int m, int e, float& x) {
            const int ch = grp * 8 + e;
            if (tap >= taps || ch >= cin) return false;
            x = w[((size_t)m * cin + ch) * taps + tap];
            return true;
        };
    });
}

void x6_pack_weights_pairs(const float* w, int cout, int cin, int ks, int Mpad, int* nK_out,
                           std::vector<uint16_t>& out) {
    const int taps = ks * ks, cin_g = (cin + 7) / 8;
    const int nK = *nK_out = (cin_g * taps + 3) / 4;
    x6_pack_units(nK, cout, Mpad, out, [=](int c, int gi) {
        const int q = 4 * c + gi, grp = q / taps, tap = q % taps;
        return [=](int m, int e, float& x) {
            const int ch = grp * 8 + e;
            if (ch >= cin) return false;  // covers the pairs past the last group
            x = w[((size_t)m * cin + ch) * taps + tap];
            return true;
        };
    });
}

void x6_pack_weights_wino(const float* w, int cout, int cin, int Mpad, int* nK_out, std::vector<uint16_t>& out) {
    const int cin_g = (cin + 7) / 8;
    const int nK = *nK_out = (cin_g * 3 + 3) / 4;
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    x6_pack_units(4 * nK, cout, Mpad, out, [=](int s, int gi) {
        const int q = 4 * (s >> 2) + gi, grp = q / 3, ky = q % 3;
        const double* g = G[s & 3];
        return [=](int m, int e, float& x) {
            const int ch = grp * 8 + e;
            if (ch >= cin) return false;
            const float* wr = w + (((size_t)m * cin + ch) * 3 + ky) * 3;
            x = (float)(g[0] * (double)wr[0] + g[1] * (double)wr[1] + g[2] * (double)wr[2]);
            return true;
        };
    });
}

}  // namespace opose
