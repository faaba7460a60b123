// unionfind.h — the union-find of the Hand() component labelling, shared by gauss_threshold
// (post.hip: a tile's components, labels in LDS) and the kernels that join and flatten them over
// the whole map (hand.hip: labels in global memory).
#pragma once
#include <hip/hip_runtime.h>

namespace opose {

// gauss_threshold's tile (post.hip), whose edges cc_border (hand.hip) joins
constexpr int TW = 64, TH = 32;

// L[x] = parent of x, a root is its own parent; every link points at a smaller index, so a
// component's root is its first pixel.  P: int*, or volatile int* where other lanes of the
// workgroup relink roots concurrently and every step has to re-read (LDS labels)
template <typename P>
__device__ __forceinline__ int uf_find(P L, int x) {
    int p = L[x];
    while (p != x) {
        x = p;
        p = L[x];
    }
    return x;
}

template <typename P>
__device__ __forceinline__ void uf_union(P L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        // link root a (larger) under b; succeeds iff a was still a root
        const int old = atomicMin(const_cast<int*>(L) + a, b);
        if (old == a) return;
        a = old;
    }
}

}  // namespace opose
