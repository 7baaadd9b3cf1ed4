// The frame shared by the K-contiguous implicit-GEMM kernels: where a gather workgroup sits (igemm_kc_kernel,
// igemm_kc_bf16_kernel), the row-offset staging (those two and igemm_halo_kernel), the accumulator store (igemm_kc_kernel,
// igemm_halo_kernel), plus the host-side operand ranges and tile planning of the gather kernels (the bf16-stored launchers of
// igemm_bf16s.hip included).  The kernels keep their own loaders, LDS layouts and inner products.
#pragma once
#include "common.h"
#include "device_prims.h"
#include "igemm.h"

namespace cslgan {

// ---- device -----------------------------------------------------------------------------------------------------------------
// xcd remap, class search, tap table (s_tap[t] = ty << 16 | tx & 0xffff; visible after the caller's barrier) and the loader
// rows of a gather workgroup: thread (lrow = tid / 8, q = tid % 8) loads 4 k of rows lrow + 32 i of both operands.
//   a_img: image base in elements; a_iy = -2^20 marks a row past M; b_off: byte offset of row n in the class's filter
//   matrix, BUF_OOB when n >= Nn.  Returns the workgroup's class.
template <int BM, int BN>
__device__ __forceinline__ const KcClass& kc_locate(const KcParams& p, int* s_tap, int& split, int& m0, int& n0,
                                                    int (&a_img)[BM / 32], int (&a_iy)[BM / 32], int (&a_ix)[BM / 32], unsigned (&b_off)[BN / 32]) {
    const int tid = threadIdx.x;
    const int nwg = p.tiles_m * p.tiles_n;
    split = blockIdx.x / nwg;
    const int wg = xcd_remap(blockIdx.x - split * nwg, nwg);
    const int tile_mg = wg / p.tiles_n, tile_n = wg - tile_mg * p.tiles_n;
    int ci = 0;
#pragma unroll 1
    while (ci + 1 < p.n_cls && tile_mg >= p.cls[ci + 1].tile0) ++ci;
    const KcClass& kc = p.cls[ci];
    const int M = kc.M, OHc = kc.OHc, OWc = kc.OWc, Kdim = kc.Kdim;
    m0 = (tile_mg - kc.tile0) * BM;
    n0 = tile_n * BN;

    if (tid < IG_MAX_TAPS) s_tap[tid] = ((int)kc.ty[tid] << 16) | ((int)kc.tx[tid] & 0xffff);

    const int lrow = tid >> 3;   // 0..31
#pragma unroll
    for (int i = 0; i < BM / 32; ++i) {
        const int m = m0 + lrow + 32 * i;
        const bool ok = m < M;
        const RowCoord rc = kc_decode_row(ok ? m : 0, OHc, OWc, kc.patch);
        a_img[i] = rc.img * p.AH * p.AW * p.AC;
        a_iy[i] = ok ? rc.oy * p.sy : -(1 << 20);
        a_ix[i] = rc.ox * p.sx;
    }
#pragma unroll
    for (int i = 0; i < BN / 32; ++i) {
        const int n = n0 + lrow + 32 * i;
        b_off[i] = n < p.Nn ? 4u * (unsigned)n * (unsigned)Kdim : BUF_OOB;
    }
    return kc;
}

// Element offsets of the tile's BM output rows (and of their residual operand) into s_off / s_roff; -1 marks a row past M.
// dense: the caller knows out offset == m * ldo (single class, row-major rows, no residual).  patch: kc_decode_row's row order.
// M, OHc, OWc: the class's row grid as the kernel already holds it from its prologue (read again from kc here, the values left
// their registers over the K loop and three igemm_kc_bf16_kernel instantiations allocated 2-4 VGPRs more: one wave per SIMD).
template <int BM>
__device__ __forceinline__ void kc_stage_row_offsets(const KcParams& p, const KcClass& kc, int M, int OHc, int OWc, int m0, int patch, bool dense,
                                                     int* s_off, int* s_roff) {
    const int tid = threadIdx.x;
    if (tid < BM) {
        const int m = m0 + tid;
        int off = -1, roff = 0;
        if (m < M) {
            if (dense) {
                off = m * p.ldo;
            } else {
                const RowCoord rc = kc_decode_row(m, OHc, OWc, patch);
                off = kc_out_offset(p, kc, rc);
                if (p.res) roff = kc_res_offset(p, kc, rc);
            }
        }
        s_off[tid] = off;
        s_roff[tid] = roff;
    }
}

// A wavefront's TM x TN accumulators (32x32 MFMA layout: lane r = column, register v = row (v & 3) + 8 (v >> 2) + 4 h)
// through acc -> +bias -> +res -> act -> mask -> store.  row0: the wave's first row within the tile; col0: its first column
// in the output.  SPLITK compiles in the split-K form: partial sums are added atomically into the zeroed output, the bias
// by slice 0 only (the host splits K only for purely linear epilogues).  The parameters are read once, in front of the loops.
// Users: igemm_kc_kernel and igemm_halo_kernel.  igemm_kc_bf16_kernel keeps the same loop in its body: behind a function
// boundary, even as a literal copy, its <128,64,.,.,1> instantiations allocate 97-100 VGPRs instead of 94 (5 -> 4 waves per SIMD).
template <int TM, int TN, bool SPLITK>
__device__ __forceinline__ void kc_store_tile(const f32x16 (&acc)[TM][TN], const KcParams& p, const int* s_off, const int* s_roff,
                                              int row0, int col0, int r, int h, int split = 0) {
    const bool atomic_out = SPLITK && p.ksplit > 1;
    float* const out = p.out;
    const float* const bias = p.bias;
    const float* const res = p.res;
    const float* const mask = p.mask;
    const int act = p.act, Nn = p.Nn;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = col0 + j * 32 + r;
        if (n >= Nn) continue;
        const float bv = (bias && (!SPLITK || split == 0)) ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = row0 + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                const int off = s_off[row];
                if (off < 0) continue;
                float val = acc[i][j][v] + bv;
                if (atomic_out) {
                    atomicAdd(out + off + n, val);
                    continue;
                }
                if (res) val += res[s_roff[row] + n];
                val = apply_act(val, act);
                if (mask) val = lrelu_mask(val, mask[off + n]);
                out[off + n] = val;
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// cslgan_conv_t.compute -> KcParams::bf16 / bfloat16 pieces per operand: 0 = exact fp32, 1 = bf16, 3 = three-piece fp32 emulation
inline int kc_pieces(int compute) { return compute == CSLGAN_COMPUTE_BF16 ? 1 : (compute == CSLGAN_COMPUTE_BF16X3 ? 3 : 0); }

inline long long kc_tiles_for(const KcParams& p, int BM, int BN) {
    long long tm = 0;
    for (int c = 0; c < p.n_cls; ++c) tm += (p.cls[c].M + BM - 1) / BM;
    return tm * ((p.Nn + BN - 1) / BN);
}

// (Templates on the parameter struct: KcParams or the bf16-stored KsParams of igemm_bf16s.hip, which share these fields.)
// Byte ranges of both operands for the buffer descriptors and the reciprocal the loaders divide k by: k / AC as umulhi(k, ceil(2^32 / AC)),
// exact while k < 2^32 / AC.  a_es / w_es: bytes per element of a / the filter matrices; bk: the kernel's K tile (k runs up to Kdim + bk);
// who prefixes the messages; ac1_exact: the caller's loaders take k itself when AC == 1, where no reciprocal fits 32 bits.
template <typename P>
inline int kc_operand_ranges(P& p, int a_es, int w_es, int bk, const char* who, bool ac1_exact = false) {
    const long long n_img = p.cls[0].M / ((long long)p.cls[0].OHc * p.cls[0].OWc);
    const long long a_b = (long long)a_es * n_img * p.AH * p.AW * p.AC;
    long long w_end = 0, kmax = 0;
    for (int c = 0; c < p.n_cls; ++c) {
        const long long e = (long long)p.cls[c].w_off + (long long)p.Nn * p.cls[c].Kdim;
        w_end = e > w_end ? e : w_end;
        kmax = p.cls[c].Kdim > kmax ? p.cls[c].Kdim : kmax;
    }
    CSLGAN_REQUIRE(a_b < (long long)BUF_OOB && w_es * w_end < (long long)BUF_OOB, "%s: operand larger than 4 GB", who);
    p.a_bytes = (unsigned)a_b;
    p.w_bytes = (unsigned)(w_es * w_end);
    if (ac1_exact && p.AC == 1 && kmax + bk < (1ll << 31)) { p.ac_recip = 0xFFFFFFFFu; return CSLGAN_OK; }
    CSLGAN_REQUIRE(p.AC >= 2 && (kmax + bk) * (long long)p.AC < (1ll << 32), "%s: K too large for reciprocal division", who);
    p.ac_recip = (unsigned)(((1ull << 32) + (unsigned long long)p.AC - 1) / (unsigned long long)p.AC);
    return CSLGAN_OK;
}

// Tile grid of a K-contiguous launch: tile0 per class, tiles_m and tiles_n.  Returns the number of tiles.
template <typename P>
inline long long kc_assign_tiles(P& p, int BM, int BN) {
    int tm = 0;
    for (int c = 0; c < p.n_cls; ++c) {
        p.cls[c].tile0 = tm;
        tm += (p.cls[c].M + BM - 1) / BM;
    }
    p.tiles_m = tm;
    p.tiles_n = (p.Nn + BN - 1) / BN;
    return (long long)p.tiles_m * p.tiles_n;
}

// kc_assign_tiles and the split-K factor of a gather launch; zeroes the output when K is split.
// out_elems: floats of the output tensor, or 0 to forbid splitting.  The grid is tiles_m * tiles_n * ksplit workgroups.
inline int kc_plan_tiles(KcParams& p, int BM, int BN, long long out_elems, hipStream_t st) {
    const int tiles = (int)kc_assign_tiles(p, BM, BN);
    // split K only for purely linear epilogues and launches that would leave most CUs idle
    p.ksplit = 1;
    int nk_max = 0;
    for (int c = 0; c < p.n_cls; ++c) {
        const int nk = (p.cls[c].Kdim + IG_BK - 1) / IG_BK;
        nk_max = nk > nk_max ? nk : nk_max;
    }
    if (tiles < 96 && nk_max >= 16 && p.act == CSLGAN_ACT_NONE && !p.res && !p.mask && out_elems > 0) {
        const int want = (256 + tiles - 1) / tiles, cap = nk_max / 4;
        p.ksplit = want < cap ? want : cap;
        if (p.ksplit < 1) p.ksplit = 1;
    }
    if (p.ksplit > 1) return zero_floats(p.out, (size_t)out_elems, st);
    return CSLGAN_OK;
}

// Gather launches enumerate 8x8 patches where the class grid allows it ...
template <typename P>
inline void kc_mark_patches(P& p) {
    for (KcClass* k = p.cls; k < p.cls + p.n_cls; ++k) k->patch = (k->T > 1 && k->OHc % 8 == 0 && k->OWc % 8 == 0) ? 1 : 0;
}

// ... and vecA / vecB: 16-byte loads of a / the filter are legal.
inline void kc_mark_patches_and_vec(KcParams& p, bool& vecA, bool& vecB) {
    kc_mark_patches(p);
    bool kd4 = true;
    for (int c = 0; c < p.n_cls; ++c) kd4 = kd4 && (p.cls[c].Kdim % 4 == 0) && (p.cls[c].w_off % 4 == 0);
    vecA = (p.AC % 4 == 0) && aligned16(p.a);
    vecB = kd4 && aligned16(p.w);
}

}  // namespace cslgan
