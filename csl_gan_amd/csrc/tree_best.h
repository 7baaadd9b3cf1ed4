// The candidate record, the tie rule and the wave reduction that the split searches on cache bytes share (tree_kernels.hip: 32-bit
// counts; boost_kernels.hip: 64-bit counts).  Included after device_prims.h.
#pragma once
#include "device_prims.h"

namespace cslgan {

template <typename C>
struct TreeBestT {
    double s;                            // -1: no candidate (a score is >= 0)
    int j, v, vh;
    C nL, pL;
};

// a before b: the larger score, then the smaller feature, then the smaller byte
__device__ __forceinline__ bool tree_better(double as, int aj, int av, double bs, int bj, int bv) {
    return as > bs || (as == bs && (aj < bj || (aj == bj && av < bv)));
}

template <typename C>
__device__ __forceinline__ void tree_wave_best(TreeBestT<C>& b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        TreeBestT<C> t;
        t.s = __shfl_xor(b.s, o, 64);
        t.j = __shfl_xor(b.j, o, 64);
        t.v = __shfl_xor(b.v, o, 64);
        t.vh = __shfl_xor(b.vh, o, 64);
        t.nL = __shfl_xor(b.nL, o, 64);
        t.pL = __shfl_xor(b.pL, o, 64);
        if (tree_better(t.s, t.j, t.v, b.s, b.j, b.v)) b = t;
    }
}

}  // namespace cslgan
