// Pieces shared by the one-vs-rest classifiers on cache rows (logreg_kernels.hip, mlp_kernels.hip): the stable loss / residual
// terms of a logit and the 16-byte row loads that never read beyond the matrix.  Included after device_prims.h.
#pragma once
#include "device_prims.h"

namespace cslgan {

// softplus(-s z) and sigmoid(z) from one exponential of -|z|: no overflow for any finite z.
__device__ __forceinline__ void lr_terms(float z, bool positive, float& loss, float& resid) {
    const float e = expf(-fabsf(z));
    const float sz = positive ? z : -z;                          // s z
    loss = (sz < 0.f ? -sz : 0.f) + log1pf(e);                   // max(-s z, 0) + log(1 + exp(-|z|))
    const float sig = (z >= 0.f ? 1.f : e) / (1.f + e);
    resid = sig - (positive ? 1.f : 0.f);
}

// Bytes [col, col + 16) of the row that starts at byte `start` of x (col a multiple of 16), zero from column D on and when !ok (a
// row that does not exist).  AL: D % 16 == 0, so the 16 bytes are one aligned word inside the row; the load is unconditional, from
// offset 0 where there is nothing to read, followed by a select: no branch, so the loads of one fetch stay in flight together.
// Otherwise they are assembled from the two ALIGNED words that hold them (per-lane shift: lanes hold different rows), and words that
// reach beyond the last byte of x (`total`; `whole` = total & ~15) are never touched: those bytes are read one by one.
template <bool AL>
__device__ __forceinline__ u32x4 lrb_load16(const unsigned char* __restrict__ x, unsigned long long total, unsigned long long whole,
                                            unsigned long long start, int col, int D, bool ok) {
    u32x4 v = {0u, 0u, 0u, 0u};
    const int valid = D - col;
    if (AL) {
        const bool in = ok && valid > 0;
        const u32x4 got = *reinterpret_cast<const u32x4*>(x + (in ? start + (unsigned long long)col : 0ull));      // total >= 16
        v.x = in ? got.x : 0u; v.y = in ? got.y : 0u; v.z = in ? got.z : 0u; v.w = in ? got.w : 0u;
        return v;
    }
    if (!ok || valid <= 0) return v;
    const unsigned long long a = start + (unsigned long long)col;
    const int s = (int)(a & 15u);
    const unsigned long long g = a - (unsigned long long)s;
    if (g + 32ull <= whole) {
        const u32x4 lo = *reinterpret_cast<const u32x4*>(x + g);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(x + g + 16);
        const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const int ds = s >> 2, bs = s & 3;
        unsigned t[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) t[j] = ds == 0 ? w[j] : (ds == 1 ? w[j + 1] : (ds == 2 ? w[j + 2] : w[(j + 3) & 7]));   // j + 3 <= 7
        v.x = __builtin_amdgcn_alignbyte(t[1], t[0], bs);
        v.y = __builtin_amdgcn_alignbyte(t[2], t[1], bs);
        v.z = __builtin_amdgcn_alignbyte(t[3], t[2], bs);
        v.w = __builtin_amdgcn_alignbyte(t[4], t[3], bs);
    } else {
        unsigned b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned long long q = a + (unsigned long long)j;
            const unsigned byte = q < total ? (unsigned)x[q] : 0u;
            b[j >> 2] |= byte << (8 * (j & 3));
        }
        v.x = b[0]; v.y = b[1]; v.z = b[2]; v.w = b[3];
    }
    if (valid < 16) {                                           // the bytes past the row's end hold the next row or nothing
        unsigned m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nb = valid - 4 * j;
            m[j] = nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u));
        }
        v.x &= m[0]; v.y &= m[1]; v.z &= m[2]; v.w &= m[3];
    }
    return v;
}

// byte e (0 .. 15, a compile-time constant after unrolling) of a 16-byte word as the exact float 0 .. 255
__device__ __forceinline__ float lrb_byte(const u32x4& v, int e) {
    const unsigned d = (e >> 2) == 0 ? v.x : ((e >> 2) == 1 ? v.y : ((e >> 2) == 2 ? v.z : v.w));
    return (float)((d >> (8 * (e & 3))) & 0xffu);
}

}  // namespace cslgan
