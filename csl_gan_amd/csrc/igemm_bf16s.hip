// bf16 STORAGE path (BASELINE.json configs[4]: "CelebA 128x128 DCResNet bf16 ... HBM-bound per-sample grads"; SURVEY §8(d)
// "bf16 storage / fp32 accumulate").  gfx950 only.
//
// igemm_bf16.hip computes on the bf16 matrix cores but reads fp32 tensors and rounds them on the way into LDS: a 128x128
// tile then moves 32 KB per 1.05 MFLOP and the kernels sit on L2 bandwidth at 0.10-0.13 of the bf16 MFMA peak.  Here the
// ACTIVATIONS, the ACTIVATION GRADIENTS and a pre-rounded copy of the FILTERS are bfloat16 in HBM (fp32 master weights, fp32
// accumulation, fp32 weight gradients / norms / clip / noise / Adam):
//
//   igemm_kcs_kernel   forward conv / linear and data gradient: a 16-byte global load is 8 consecutive k of one row = exactly
//                      one operand of v_mfma_f32_32x32x16_bf16, stored to LDS as it is (no conversion, half the bytes of the
//                      fp32 loader, K tile 64); the epilogue (bias, residual, activation, LeakyReLU mask) writes bf16 or fp32.
//   igemm_halos_kernel stride-1 forward convs with an LDS-resident input halo.
//   round / repack     the fp32 master filter rounded once per parameter version (plain KRSC order for the forward conv: round_bf16,
//                      cast_kernels.hip; per-parity-class [C][taps][K] matrices for the data gradient), cached by the caller.
//
// The other kernels of the storage mode sit with their fp32 forms: the weight gradient in igemm_mcs.hip, the 1x1 stream in
// conv1x1.hip, the critic's head in linear_k1.hip, the bias gradient in igemm_mc.hip, casts and activation backward in cast_kernels.hip.
//
// Numerics: every product is bf16(a)*bf16(b) exactly, summed in fp32; what is new against CSLGAN_COMPUTE_BF16 on fp32 tensors is
// ONE extra rounding per stored activation / activation gradient (relative 2^-9), i.e. the same order as the operand rounding
// the matrix core needs anyway.
//
// Replaces (reference file:line): nn.Conv2d / nn.Linear forward and autograd data gradients (DCResNet_models.py:131-132,145).
#include "common.h"
#include "device_prims.h"
#include "igemm.h"
#include "kc_frame.h"
#include "conv_classes.h"

namespace cslgan {

// ---- K-contiguous form on bf16 tensors -------------------------------------------------------------------------------------
struct KsParams {
    const void* a;               // bf16 [img][AH][AW][AC]
    unsigned a_bytes, w_bytes;
    unsigned ac_recip;           // ceil(2^32 / AC)
    int AH, AW, AC, VH, VW, sy, sx;
    const void* w;               // bf16 class matrices [Nn][Kdim] at element offset cls[].w_off
    int Nn;
    void* out;                   // bf16 or fp32 (template)
    int OHf, OWf, osy, osx, ldo, dense_out;
    const float* bias;
    const void* res;             // same indexing as out; bf16 when res_bf16
    int res_bf16;
    const void* mask;            // same indexing as out; bf16 when mask_bf16
    int mask_bf16;
    int act;
    int n_cls, tiles_m, tiles_n;
    const void* w3;              // igemm_halos: the filter as bf16 in step-major order [chunk * T + tap][n][16 k] (split_filter_x3_kernel<1>)
    int w3_off[IG_MAX_CLS];      // igemm_halos: element offset of each class's step-major matrix in w3 (data-gradient parity classes)
    KcClass cls[IG_MAX_CLS];
};

constexpr int KS_BK = 64;        // k per LDS tile = 8 entries of 8 bf16 (16 bytes)

// Epilogue of the gather and halo kernels.  The MFMAs are issued with the FILTER fragment as the first operand and the pixel fragment
// as the second, so the accumulator's lane index r is the PIXEL and its register index v the output channel
// (v & 3) + 8 (v >> 2) + 4 h: a lane holds 4 x 4 consecutive channels of one pixel.  Bias, residual and mask are read as 4-element
// vectors and the result leaves as one 8-byte (bf16) or 16-byte (fp32) store per group; the lanes (r, h = 0) and (r, h = 1) write
// adjacent pieces.  With the pixel on v (the usual operand order) every element was its own 2-byte store, 64 B contiguous per 32
// lanes: 64 store instructions per lane and tile, 0.05 of the 0.30 ms of the critic's first 64-channel conv.
template <int TM, int TN, bool OUT_BF16>
__device__ __forceinline__ void ks_epilogue(const f32x16 (&acc)[TM][TN], const KsParams& p, const int* s_off, int row0, int col0, int r, int h) {
    // vector path: 4-channel groups never straddle the channel count or a row, and every base pointer is 16-byte aligned
    const bool vec = !(p.Nn & 3) && !(p.ldo & 3) &&
        !((reinterpret_cast<unsigned long long>(p.out) | reinterpret_cast<unsigned long long>(p.res) | reinterpret_cast<unsigned long long>(p.mask) |
           reinterpret_cast<unsigned long long>(p.bias)) & 15ull);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int off = s_off[row0 + i * 32 + r];
        if (off < 0) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = col0 + j * 32 + 8 * g + 4 * h;
                if (n >= p.Nn) continue;
                float val[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) val[e] = acc[i][j][4 * g + e];
                if (vec) {
                    if (p.bias) {
                        const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
                        val[0] += b.x; val[1] += b.y; val[2] += b.z; val[3] += b.w;
                    }
                    if (p.res) {
                        if (p.res_bf16) {
                            const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(p.res) + off + n);
                            val[0] += bf_lo(u.x); val[1] += bf_hi(u.x);
                            val[2] += bf_lo(u.y); val[3] += bf_hi(u.y);
                        } else {
                            const float4 u = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.res) + off + n);
                            val[0] += u.x; val[1] += u.y; val[2] += u.z; val[3] += u.w;
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) val[e] = apply_act(val[e], p.act);
                    if (p.mask) {
                        float mv[4];
                        if (p.mask_bf16) {
                            const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(p.mask) + off + n);
                            mv[0] = bf_lo(u.x); mv[1] = bf_hi(u.x);
                            mv[2] = bf_lo(u.y); mv[3] = bf_hi(u.y);
                        } else {
                            const float4 u = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.mask) + off + n);
                            mv[0] = u.x; mv[1] = u.y; mv[2] = u.z; mv[3] = u.w;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) val[e] = lrelu_mask(val[e], mv[e]);
                    }
                    if (OUT_BF16) *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.out) + off + n) = make_uint2(pack_bf16(val[0], val[1]), pack_bf16(val[2], val[3]));
                    else *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + off + n) = make_float4(val[0], val[1], val[2], val[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (n + e >= p.Nn) continue;
                        float x = val[e] + (p.bias ? p.bias[n + e] : 0.f);
                        if (p.res) x += p.res_bf16 ? bf2f(reinterpret_cast<const unsigned short*>(p.res)[off + n + e]) : reinterpret_cast<const float*>(p.res)[off + n + e];
                        x = apply_act(x, p.act);
                        if (p.mask) {
                            const float mv = p.mask_bf16 ? bf2f(reinterpret_cast<const unsigned short*>(p.mask)[off + n + e]) : reinterpret_cast<const float*>(p.mask)[off + n + e];
                            x = lrelu_mask(x, mv);
                        }
                        if (OUT_BF16) reinterpret_cast<unsigned short*>(p.out)[off + n + e] = bf16_rne(x);
                        else reinterpret_cast<float*>(p.out)[off + n + e] = x;
                    }
                }
            }
        }
    }
}

// Element offsets of the tile's BM output rows into s_off (residual and mask share them); -1 marks a row past M.
// dense: the caller knows out offset == m * ldo (single class, row-major rows).  patch: kc_decode_row's row order.
template <int BM>
__device__ __forceinline__ void ks_stage_row_offsets(const KsParams& p, const KcClass& kc, int M, int OHc, int OWc, int m0, int patch, bool dense,
                                                     int* s_off) {
    const int tid = threadIdx.x;
    if (tid < BM) {
        const int m = m0 + tid;
        int off = -1;
        if (m < M) {
            if (dense) {
                off = m * p.ldo;
            } else {
                const RowCoord rc = kc_decode_row(m, OHc, OWc, patch);
                off = ((rc.img * p.OHf + rc.oy * p.osy + kc.oy0) * p.OWf + rc.ox * p.osx + kc.ox0) * p.ldo;
            }
        }
        s_off[tid] = off;
    }
}

template <int BM, int BN, int WAVES_M, int WAVES_N, bool OUT_BF16>
__global__ __launch_bounds__(256, 2) void igemm_kcs_kernel(const KsParams p) {
    constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
    static_assert(WAVES_M * WAVES_N == 4 && TM >= 1 && TN >= 1, "bad tile");
    constexpr int A_ES = BM + 1, B_ES = BN + 1;             // uint4 (16-byte) units per LDS entry, padded by 16 B
    constexpr int A_PASS = BM / 32, B_PASS = BN / 32;
    __shared__ __attribute__((aligned(16))) uint4 As[2][8 * A_ES];
    __shared__ __attribute__((aligned(16))) uint4 Bs[2][8 * B_ES];
    __shared__ int s_tap[IG_MAX_TAPS];
    __shared__ int s_off[BM];

    const int tid = threadIdx.x;
    const int nwg = p.tiles_m * p.tiles_n;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int tile_mg = wg / p.tiles_n, tile_n = wg - tile_mg * p.tiles_n;
    int ci = 0;
#pragma unroll 1
    while (ci + 1 < p.n_cls && tile_mg >= p.cls[ci + 1].tile0) ++ci;
    const KcClass& kc = p.cls[ci];
    const int M = kc.M, OHc = kc.OHc, OWc = kc.OWc, Kdim = kc.Kdim;
    const int m0 = (tile_mg - kc.tile0) * BM, n0 = tile_n * BN;

    if (tid < IG_MAX_TAPS) s_tap[tid] = ((int)kc.ty[tid] << 16) | ((int)kc.tx[tid] & 0xffff);

    const int lrow = tid >> 3;   // 0..31
    const int e = tid & 7;       // LDS entry (8 consecutive k) within the 64-k tile: 8 lanes read 128 contiguous bytes of a row
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.a, p.a_bytes);
    const __amdgpu_buffer_rsrc_t w_rsrc = make_rsrc(reinterpret_cast<const unsigned short*>(p.w) + kc.w_off, p.w_bytes - 2u * (unsigned)kc.w_off);
    int a_img[A_PASS], a_iy[A_PASS], a_ix[A_PASS];
#pragma unroll
    for (int i = 0; i < A_PASS; ++i) {
        const int m = m0 + lrow + 32 * i;
        const bool ok = m < M;
        const RowCoord rc = kc_decode_row(ok ? m : 0, OHc, OWc, kc.patch);
        a_img[i] = rc.img * p.AH * p.AW * p.AC;
        a_iy[i] = ok ? rc.oy * p.sy : -(1 << 20);
        a_ix[i] = rc.ox * p.sx;
    }
    unsigned b_off[B_PASS];
#pragma unroll
    for (int i = 0; i < B_PASS; ++i) {
        const int n = n0 + lrow + 32 * i;
        b_off[i] = n < p.Nn ? 2u * (unsigned)n * (unsigned)Kdim : BUF_OOB;
    }
    __syncthreads();

    // Two register sets: the loads of K tile t+2 are issued before the MFMAs of tile t and written to LDS after the MFMAs of tile
    // t+1 — two tiles of matrix work (>= 2 x 512 MFMA cycles per wave) to cover the L2 / HBM latency of a gathered load.  With one
    // set (loads one tile ahead) the kernel waited on its loads every iteration: 390-500 TF.
    u32x4 ra0[A_PASS], rb0[B_PASS], ra1[A_PASS], rb1[B_PASS];
    auto load_tile = [&](int kt, u32x4 (&ra)[A_PASS], u32x4 (&rb)[B_PASS]) {
        // Branch-free offsets: an invalid element ORs BUF_OOB into its (always computed) offset, which the buffer descriptor's range
        // check turns into a zero load.  Written as `ok ? offset : OOB` the compiler put every load into its own exec-masked block
        // (nine s_and_saveexec per half iteration), which also kept it from issuing the eight loads back to back.
        const int kb = kt * KS_BK + e * 8;
        const bool kin = kb < Kdim;
        const int t = (int)__umulhi((unsigned)(kin ? kb : 0), p.ac_recip);
        const int c = (kin ? kb : 0) - t * p.AC;
        const int tap = s_tap[t];
        const int ty = tap >> 16, tx = (int)(short)(tap & 0xffff);
        const unsigned kbad = kin ? 0u : BUF_OOB;
#pragma unroll
        for (int i = 0; i < A_PASS; ++i) {
            const int iy = a_iy[i] + ty, ix = a_ix[i] + tx;
            const unsigned bad = ((unsigned)iy < (unsigned)p.VH && (unsigned)ix < (unsigned)p.VW) ? kbad : BUF_OOB;
            ra[i] = buf_load4_raw(a_rsrc, (2u * (unsigned)(a_img[i] + (iy * p.AW + ix) * p.AC + c)) | bad);
        }
#pragma unroll
        for (int i = 0; i < B_PASS; ++i)
            rb[i] = buf_load4_raw(w_rsrc, ((b_off[i] + 2u * (unsigned)kb) | kbad | (b_off[i] == BUF_OOB ? BUF_OOB : 0u)));
    };
    auto store_tile = [&](int buf, const u32x4 (&ra)[A_PASS], const u32x4 (&rb)[B_PASS]) {
#pragma unroll
        for (int i = 0; i < A_PASS; ++i) As[buf][e * A_ES + lrow + 32 * i] = __builtin_bit_cast(uint4, ra[i]);
#pragma unroll
        for (int i = 0; i < B_PASS; ++i) Bs[buf][e * B_ES + lrow + 32 * i] = __builtin_bit_cast(uint4, rb[i]);
    };

    const int lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wid / WAVES_N, wn = wid - wm * WAVES_N;
    const int arow0 = wm * TM * 32 + r, brow0 = wn * TN * 32 + r;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    auto mma_tile = [&](int buf) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            bf16x8 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = __builtin_bit_cast(bf16x8, As[buf][(2 * s + h) * A_ES + arow0 + i * 32]);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = __builtin_bit_cast(bf16x8, Bs[buf][(2 * s + h) * B_ES + brow0 + j * 32]);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[j], af[i], acc[i][j], 0, 0, 0);   // filter first: see ks_epilogue
        }
    };

    const int nk = (Kdim + KS_BK - 1) / KS_BK;
    load_tile(0, ra0, rb0);
    load_tile(1, ra1, rb1);          // past the last tile every offset is out of range -> zeros, never multiplied
    store_tile(0, ra0, rb0);
    __syncthreads();
    // ONE loop exit: with a break between the halves the epilogue had two live-in states for the accumulators and the register
    // allocator copied all 64 of them (32 v_mov_b64) plus the staging registers between the halves of every iteration — 107 moves per
    // 16 MFMAs, most of the "8 vector instructions per MFMA" the PMC counters showed.  An odd tile count multiplies one all-zero tile.
    for (int kt = 0; kt < nk; kt += 2) {
        load_tile(kt + 2, ra0, rb0);
        mma_tile(0);
        store_tile(1, ra1, rb1);     // tile kt + 1 (zeros past the end)
        __syncthreads();
        load_tile(kt + 3, ra1, rb1);
        mma_tile(1);
        store_tile(0, ra0, rb0);     // tile kt + 2
        __syncthreads();
    }

    // ---- epilogue: output offsets per row (residual and mask share them), then bias / residual / activation / mask ----------
    ks_stage_row_offsets<BM>(p, kc, M, OHc, OWc, m0, kc.patch, p.dense_out && !kc.patch, s_off);
    __syncthreads();
    ks_epilogue<TM, TN, OUT_BF16>(acc, p, s_off, wm * TM * 32, n0 + wn * TN * 32, r, h);
}

// ---- stride-1 convs with an LDS-resident input halo (the generator's 5x5 / 3x3 convs on bf16 activations) ---------------------
// igemm_halo_x3_kernel<BN, 1> (igemm_bf16.hip) with bfloat16 activations in HBM: a workgroup owns two 8x8 output patches x BN
// channels; per 16-channel chunk the (8+R-1) x (8+S-1) halo of each patch is staged in LDS ONCE (a pixel's 16 channels are two
// 16-byte loads, stored as loaded — no conversion) and every tap reads its A fragments from that image at a per-tap offset; the
// filter never touches LDS: it is streamed pre-rounded in step-major order straight into a 4-deep register ring.  Against the
// gather form above the input is read from L2 / HBM once per chunk instead of once per tap.
constexpr int HS_MAX = 12 * 12;        // pixels per patch halo (8+4 squared: up to 5x5 taps)

template <int BN, bool OUT_BF16>
__global__ __launch_bounds__(256, 2) void igemm_halos_kernel(const KsParams p) {
    constexpr int RING = 4;
    constexpr int PATCHES = 2, WN = 2;                       // waves 2 (M: one 8x8 patch each) x 2 (N halves)
    constexpr int BM = 64 * PATCHES, TM = 2, TN = BN / (32 * WN);
    __shared__ __attribute__((aligned(16))) uint2 Hs[PATCHES * HS_MAX * 4];     // [patch][pixel][4 x (4 ch bf16)]
    __shared__ int s_tapoff[IG_MAX_TAPS];
    __shared__ int s_off[BM];

    const int tid = threadIdx.x;
    const int nwg = p.tiles_m * p.tiles_n;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int tile_mg = wg / p.tiles_n, tile_n = wg - tile_mg * p.tiles_n;
    int ci = 0;
#pragma unroll 1
    while (ci + 1 < p.n_cls && tile_mg >= p.cls[ci + 1].tile0) ++ci;      // data gradient: one class per output parity, each its own tiles
    const KcClass& kc = p.cls[ci];
    const int M = kc.M, OHc = kc.OHc, OWc = kc.OWc, T = kc.T;
    const int m0 = (tile_mg - kc.tile0) * BM, n0 = tile_n * BN;
    const int HW_ = kc.halo_w, hpix = kc.halo_h * kc.halo_w;
    const int img_stride = p.AH * p.AW * p.AC;

    // tap offset in uint2 units; bit 0 = parity of the tap's halo-row offset (selects the swizzled base)
    if (tid < IG_MAX_TAPS) s_tapoff[tid] = ((((int)kc.ty[tid] - kc.ty_min) * HW_ + ((int)kc.tx[tid] - kc.tx_min)) * 4) | (((int)kc.ty[tid] - kc.ty_min) & 1);

    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.a, p.a_bytes);
    int p_img[PATCHES], p_y0[PATCHES], p_x0[PATCHES];
    bool p_ok[PATCHES];
#pragma unroll
    for (int pp = 0; pp < PATCHES; ++pp) {
        const int m = m0 + 64 * pp;
        p_ok[pp] = m < M;
        const RowCoord rc = kc_decode_row(p_ok[pp] ? m : 0, OHc, OWc, 1);     // first row of the patch = its top-left pixel
        p_img[pp] = rc.img * img_stride;
        p_y0[pp] = rc.oy + kc.ty_min;
        p_x0[pp] = rc.ox + kc.tx_min;
    }
    const int lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wid / WN, wn = wid - wm * WN;             // wm = patch index
    // filter: lane (r, h), tile j reads 8 consecutive k of filter row n0 + wn*TN*32 + j*32 + r of one step = one 16-byte load
    const __amdgpu_buffer_rsrc_t w3_rsrc = make_rsrc(reinterpret_cast<const unsigned short*>(p.w3) + p.w3_off[ci], 2u * (unsigned)p.Nn * (unsigned)kc.Kdim);
    const unsigned step_bytes = 32u * (unsigned)p.Nn;
    unsigned b_off[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + j * 32 + r;
        b_off[j] = n < p.Nn ? 32u * (unsigned)n + 16u * (unsigned)h : BUF_OOB;
    }
    u32x4 rb[RING][TN];
    const int n_steps = (p.AC >> 4) * T;
    auto load_b = [&](int step, int slot) {                 // filter slice of `step` (= chunk * T + tap); zeros past the end
        const unsigned kb = (unsigned)step * step_bytes;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            rb[slot][j] = buf_load4_raw(w3_rsrc, ((b_off[j] + kb) | ((step >= n_steps || b_off[j] == BUF_OOB) ? BUF_OOB : 0u)));
        }
    };
    // halo staging: PATCHES x hpix pixels x 2 halves of 8 channels; <= PATCHES*144*2/256 = 2.25 / 4.5 16-byte loads per thread
    constexpr int HREG = (PATCHES * HS_MAX * 2 + 255) / 256;
    u32x4 rh[HREG];
    const int h_total = PATCHES * hpix * 2;
    auto fetch_halo = [&](int cc) {
#pragma unroll
        for (int j = 0; j < HREG; ++j) {
            const int idx = tid + 256 * j;
            const int half = idx & 1, pixg = idx >> 1;
            const int pp = idx < h_total ? pixg / hpix : 0;
            const int pix = pixg - pp * hpix;
            const int hy = pix / HW_, hx = pix - hy * HW_;
            // (select chains, not p_y0[pp]: a dynamically indexed register array goes to scratch)
            int sy0 = p_y0[0], sx0 = p_x0[0], simg = p_img[0];
            bool sok = p_ok[0];
#pragma unroll
            for (int q = 1; q < PATCHES; ++q) {
                sy0 = pp == q ? p_y0[q] : sy0; sx0 = pp == q ? p_x0[q] : sx0; simg = pp == q ? p_img[q] : simg; sok = pp == q ? p_ok[q] : sok;
            }
            const int iy = sy0 + hy, ix = sx0 + hx;
            const bool ok = idx < h_total && sok && (unsigned)iy < (unsigned)p.VH && (unsigned)ix < (unsigned)p.VW;
            rh[j] = buf_load4_raw(a_rsrc, (2u * (unsigned)(simg + (iy * p.AW + ix) * p.AC + cc * 16 + half * 8)) | (ok ? 0u : BUF_OOB));
        }
    };
    auto commit_halo = [&]() {
#pragma unroll
        for (int j = 0; j < HREG; ++j) {
            const int idx = tid + 256 * j;
            if (idx < h_total) {
                const int half = idx & 1, pixg = idx >> 1;
                const int pp = pixg / hpix;
                const int pix = pixg - pp * hpix;
                // the two 16-byte halves of a pixel are swapped on odd halo rows (the two patch rows a 16-lane ds_read_b128 group
                // covers then hit disjoint banks)
                const int at = (pp * HS_MAX + pix) * 4 + 2 * (half ^ ((pix / HW_) & 1));
                *reinterpret_cast<uint4*>(&Hs[at]) = __builtin_bit_cast(uint4, rh[j]);
            }
        }
    };

    // uint2 offset of this lane's pixel (tap 0,0 corner) per MFMA tile; a tap landing on an odd halo row reads the other 16-byte half
    // of the pixel (half-swap swizzle): a_pix + (a_half ^ (odd << 1)) — arithmetic, not a [2][TM] table (that went to scratch)
    int a_pix[TM], a_half[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int qq = i * 32 + r;                           // row within the patch
        a_pix[i] = (wm * HS_MAX + (qq >> 3) * HW_ + (qq & 7)) * 4;
        a_half[i] = (h ^ ((qq >> 3) & 1)) << 1;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    fetch_halo(0);
#pragma unroll
    for (int q = 0; q < RING; ++q) load_b(q, q);
    commit_halo();
    __syncthreads();

    bf16x8 af_n[TM];
    auto read_a = [&](int t) {
        const int tw = s_tapoff[t], toff = tw & ~1, odd = tw & 1;
#pragma unroll
        for (int i = 0; i < TM; ++i) af_n[i] = *reinterpret_cast<const bf16x8*>(&Hs[a_pix[i] + (a_half[i] ^ (odd << 1)) + toff]);
    };
    read_a(0);

    auto k_step = [&](int s, int SL) {
        const int cc = s / T, t = s - cc * T;
        const int t_fetch = T > 3 ? T - 3 : 0;
        const bool last_chunk = (cc + 1) * 16 >= p.AC;
        if (t == t_fetch && !last_chunk) fetch_halo(cc + 1);
        bf16x8 bf[TN], af[TM];
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = __builtin_bit_cast(bf16x8, rb[SL][j]);
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = af_n[i];
        load_b(s + RING, SL);
        const bool boundary = t == T - 1;
        if (!boundary) read_a(t + 1);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[j], af[i], acc[i][j], 0, 0, 0);   // filter first: see ks_epilogue
        if (boundary) {
            if (!last_chunk) {                 // the halo image is the only shared state: one barrier pair per CHUNK, none per tap
                __syncthreads();
                commit_halo();
                __syncthreads();
            }
            if (s + 1 < n_steps) read_a(0);
        }
    };
    for (int s = 0; s < n_steps; s += RING) {
        k_step(s, 0);
        if (s + 1 < n_steps) k_step(s + 1, 1);
        if (s + 2 < n_steps) k_step(s + 2, 2);
        if (s + 3 < n_steps) k_step(s + 3, 3);
    }
    __syncthreads();

    ks_stage_row_offsets<BM>(p, kc, M, OHc, OWc, m0, 1, false, s_off);
    __syncthreads();
    ks_epilogue<TM, TN, OUT_BF16>(acc, p, s_off, wm * 64, n0 + wn * TN * 32, r, h);
}

// stride-1 classes (one for a forward conv; the output-parity classes of a strided data gradient), each on an 8x8-patchable grid of at
// least 16x16, channels a multiple of 16, 2..25 taps within a 12x12 halo, >= 64 filters
static bool halos_eligible(const KsParams& p) {
    if (p.n_cls < 1 || p.sy != 1 || p.sx != 1 || (p.AC & 15) || p.Nn < 64 || !aligned16(p.a)) return false;
    for (int c = 0; c < p.n_cls; ++c) {
        const KcClass& k = p.cls[c];
        if (k.T < 2 || (k.M & 63) || (k.OHc & 7) || (k.OWc & 7) || k.OHc < 16 || k.OWc < 16) return false;
        int ymin, ymax, xmin, xmax;
        tap_range(k, ymin, ymax, xmin, xmax);
        if (ymax - ymin > 4 || xmax - xmin > 4) return false;
    }
    return true;
}

static int launch_halos(KsParams& p, bool out_bf16, hipStream_t st) {
    long long w_el = 0;
    for (int c = 0; c < p.n_cls; ++c) {
        KcClass& k = p.cls[c];
        int ymin, ymax, xmin, xmax;
        tap_range(k, ymin, ymax, xmin, xmax);
        k.ty_min = ymin; k.tx_min = xmin; k.halo_h = 8 + ymax - ymin; k.halo_w = 8 + xmax - xmin;
        k.patch = 1;
        p.w3_off[c] = k.w_off;             // a class's step-major matrix has the size of its plain one: same offsets
        w_el += (long long)p.Nn * k.Kdim;
    }
    const KcClass& k0 = p.cls[0];
    const long long n_img = k0.M / ((long long)k0.OHc * k0.OWc);
    const long long a_b = 2ll * n_img * p.AH * p.AW * p.AC;
    CSLGAN_REQUIRE(a_b < (long long)BUF_OOB && 2ll * w_el < (long long)BUF_OOB, "igemm_halos: operand larger than 4 GB");
    p.a_bytes = (unsigned)a_b;
    const bool wide = p.Nn > 64;
    // (A four-patch form for the 64-filter layers — one patch per wave, each wave all 64 filters, four MFMAs per step instead of two —
    // was built and measured same-box: 312 vs 396 TF on the 128x128x64 layer, 257 vs 324 and 309 vs 363 on the others.  The steps are
    // paced by the filter slices every wave streams from L1 / L2, not by MFMAs per operand load; it was removed again.)
    kc_assign_tiles(p, 128, wide ? 128 : 64);        // (narrow: exactly 64 filters, one column tile)
    const dim3 grid((unsigned)(p.tiles_m * p.tiles_n)), block(256);
    note_kernel("igemm_halos_kernel<%d>", wide ? 128 : 64);
    auto kernel = wide ? (out_bf16 ? igemm_halos_kernel<128, true> : igemm_halos_kernel<128, false>)
                       : (out_bf16 ? igemm_halos_kernel<64, true> : igemm_halos_kernel<64, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, st, p);
    return check_launch("igemm_halos_kernel");
}

template <int BM, int BN, int WM, int WN>
static int launch_kcs_tile(KsParams& p, bool out_bf16, hipStream_t st) {
    const long long tiles = kc_assign_tiles(p, BM, BN);
    if (tiles > 0x7fffffffll) { set_error("igemm_kcs: grid too large"); return CSLGAN_ERR_INVALID_ARG; }
    const dim3 grid((unsigned)tiles), block(256);
    note_kernel("igemm_kcs_kernel<%d,%d>", BM, BN);
    if (out_bf16) hipLaunchKernelGGL((igemm_kcs_kernel<BM, BN, WM, WN, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((igemm_kcs_kernel<BM, BN, WM, WN, false>), grid, block, 0, st, p);
    return check_launch("igemm_kcs_kernel");
}

static int launch_kcs(KsParams& p, bool out_bf16, hipStream_t st) {
    long long rows = 0, rows128 = 0;
    for (int c = 0; c < p.n_cls; ++c) { rows += p.cls[c].M; rows128 += (p.cls[c].M + 127) / 128; }
    if (rows <= 0 || p.Nn <= 0) return CSLGAN_OK;
    for (int c = 0; c < p.n_cls; ++c)
        CSLGAN_REQUIRE(p.cls[c].Kdim % 8 == 0 && p.cls[c].w_off % 8 == 0, "igemm_kcs: reduction length must be a multiple of 8");
    CSLGAN_REQUIRE(p.AC % 8 == 0 && aligned16(p.a) && aligned16(p.w), "igemm_kcs: channels must be a multiple of 8 and operands 16-byte aligned");
    if (int rc = kc_operand_ranges(p, 2, 2, KS_BK, "igemm_kcs")) return rc;
    kc_mark_patches(p);
    if (p.Nn <= 64) return launch_kcs_tile<128, 64, 2, 2>(p, out_bf16, st);
    if (rows128 * ((p.Nn + 127) / 128) >= 256) return launch_kcs_tile<128, 128, 2, 2>(p, out_bf16, st);
    return launch_kcs_tile<64, 128, 1, 4>(p, out_bf16, st);
}

// data-gradient classes: wt[off_cls + (c*Tc + t)*K + k] = bf16(w[((k*R + kh)*S + kw)*C + c]) for the (kh, kw) of the class's tap t
struct DgradRepack {
    int K, R, S, C, n_cls;
    int cls_off[IG_MAX_CLS], cls_T[IG_MAX_CLS];
    signed char kh[IG_MAX_CLS][IG_MAX_TAPS], kw[IG_MAX_CLS][IG_MAX_TAPS];
};

__global__ void repack_dgrad_bf16_kernel(const float* __restrict__ w, unsigned short* __restrict__ wt, DgradRepack a) {
    const int cls = blockIdx.y;
    const int Tc = a.cls_T[cls];
    const long long total = (long long)a.C * Tc * a.K;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % a.K);
        const long long rest = i / a.K;
        const int t = (int)(rest % Tc), c = (int)(rest / Tc);
        wt[a.cls_off[cls] + i] = bf16_rne(w[(((long long)k * a.R + a.kh[cls][t]) * a.S + a.kw[cls][t]) * a.C + c]);
    }
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

// y = act(conv(x, w) + bias [+ residual]) with x bf16 [N,H,W,C] (C % 8 == 0), the filter read from wb_ws = bf16(w) in KRSC order
// (written here when repack != 0), y bf16 or fp32.
int cslgan_conv2d_fwd_bf16s(const cslgan_conv_t* c, const void* x, const float* w, void* wb_ws, int repack, const float* bias,
                            const void* residual, int res_bf16, int act, void* y, int y_bf16, void* stream) {
    CSLGAN_REQUIRE(c && x && w && wb_ws && y, "conv2d_fwd_bf16s: null argument");
    int rc = check_conv(c, "conv2d_fwd_bf16s", false);
    if (rc) return rc;
    CSLGAN_REQUIRE(act >= 0 && act <= 3, "conv2d_fwd_bf16s: unknown activation %d", act);
    CSLGAN_REQUIRE(c->C % 8 == 0, "conv2d_fwd_bf16s: C=%d is not a multiple of 8", c->C);
    hipStream_t st = (hipStream_t)stream;
    if (c->K == 1 && c->H == 1 && c->W == 1 && c->R == 1 && c->S == 1 && c->stride == 1 && c->pad == 0 && !residual && !y_bf16 && c->N <= 65535 &&
        aligned16(x) && aligned16(w))         // the critic's head: a dot product per row (linear_k1.hip)
        return launch_linear_k1s_fwd(c, x, w, bias, act, reinterpret_cast<float*>(y), st);
    const long long wn = (long long)c->K * c->R * c->S * c->C;
    if (conv1x1s_eligible(c, residual) && aligned16(x) && aligned16(w) && aligned16(wb_ws)) {      // the generator's shortcut convs: a stream over pixels (conv1x1.hip)
        if (repack && (rc = round_bf16(w, wb_ws, wn, st))) return rc;
        return launch_conv1x1s(c, x, wb_ws, bias, act, y, y_bf16, st);
    }
    KsParams p{};
    p.a = x; p.AH = c->H; p.AW = c->W; p.AC = c->C; p.VH = c->H; p.VW = c->W; p.sy = p.sx = c->stride;
    p.w = wb_ws; p.Nn = c->K; p.out = y; p.OHf = c->P; p.OWf = c->Q; p.osy = p.osx = 1; p.ldo = c->K; p.dense_out = 1;
    p.bias = bias; p.res = residual; p.res_bf16 = res_bf16; p.mask = nullptr; p.mask_bf16 = 0; p.act = act;
    p.n_cls = 1;
    KcClass& k = p.cls[0];
    k.M = c->N * c->P * c->Q; k.OHc = c->P; k.OWc = c->Q; k.T = c->R * c->S; k.Kdim = k.T * c->C; k.w_off = 0; k.oy0 = k.ox0 = 0;
    fill_forward_taps(k.ty, k.tx, c->R, c->S, c->pad);
    // the layout of the bf16 filter copy follows the kernel, and the kernel follows the SHAPE alone (a layer always takes the same
    // route, so a cached copy is always in the layout its reader expects): step-major for the LDS-halo form, plain KRSC otherwise
    const bool halo = halos_eligible(p) && aligned16(w) && aligned16(wb_ws) && wn % 4 == 0;
    if (repack) {
        CSLGAN_REQUIRE(aligned16(w) && aligned16(wb_ws), "conv2d_fwd_bf16s: filter must be 16-byte aligned");
        rc = halo ? split_filter_x3(w, c->K, c->R * c->S, c->C, wb_ws, st, 1) : round_bf16(w, wb_ws, wn, st);
        if (rc) return rc;
    }
    if (halo) {
        p.w3 = wb_ws;
        return launch_halos(p, y_bf16 != 0, st);
    }
    return launch_kcs(p, y_bf16 != 0, st);
}

// gx = conv_transpose(gy, w) (* lrelu'(mask)) with gy bf16 [N,P,Q,K] (K % 8 == 0), the per-parity-class filter matrices read from
// wt_ws (bf16, K*R*S*C elements, written here when repack != 0), gx bf16 or fp32, mask (nullable) of gx's shape and element type.
int cslgan_conv2d_dgrad_bf16s(const cslgan_conv_t* c, const void* gy, const float* w, void* wt_ws, int repack, const void* mask,
                              void* gx, int gx_bf16, void* stream) {
    CSLGAN_REQUIRE(c && gy && w && wt_ws && gx, "conv2d_dgrad_bf16s: null argument");
    int rc = check_conv(c, "conv2d_dgrad_bf16s", false);
    if (rc) return rc;
    CSLGAN_REQUIRE(c->stride >= 1 && c->stride <= 2, "conv2d_dgrad_bf16s: stride %d unsupported", c->stride);
    CSLGAN_REQUIRE(c->K % 8 == 0, "conv2d_dgrad_bf16s: K=%d is not a multiple of 8", c->K);
    const int s = c->stride;
    hipStream_t st = (hipStream_t)stream;
    DgradRepack ra{};
    ra.K = c->K; ra.R = c->R; ra.S = c->S; ra.C = c->C;
    KsParams p{};
    p.a = gy; p.AH = c->P; p.AW = c->Q; p.AC = c->K; p.VH = c->P; p.VW = c->Q; p.sy = p.sx = 1;
    p.w = wt_ws; p.Nn = c->C; p.out = gx; p.OHf = c->H; p.OWf = c->W; p.osy = p.osx = s; p.ldo = c->C;
    p.dense_out = (s == 1) ? 1 : 0;
    p.bias = nullptr; p.res = nullptr; p.mask = mask; p.mask_bf16 = gx_bf16; p.act = CSLGAN_ACT_NONE;
    ClassTaps src;
    const int ncls = build_dgrad_classes(c, p.cls, src);
    CSLGAN_REQUIRE(ncls > 0, "conv2d_dgrad_bf16s: a parity class has no taps (filter smaller than stride)");
    for (int cls = 0; cls < ncls; ++cls) {
        const KcClass& k = p.cls[cls];
        for (int t = 0; t < k.T; ++t) { ra.kh[cls][t] = src.kh[cls][t]; ra.kw[cls][t] = src.kw[cls][t]; }
        ra.cls_T[cls] = k.T; ra.cls_off[cls] = k.w_off;
    }
    p.n_cls = ncls; ra.n_cls = ncls;
    // The data gradient always runs on the gather form, whose class matrices are plain [C][taps][K].  Measured (128x128, same run,
    // gather vs LDS-halo): conv2's data gradient into 64 channels 0.652 vs 0.682 ms at 384 rows (247 / 236 TF), conv3's into 128
    // channels 0.386 vs 0.473 ms (417 / 340 TF): with 4-9 taps per class the halo's reuse does not pay for its one-MFMA-tile-per-wave
    // steps.
    if (repack) {
        unsigned gxn = (unsigned)(((long long)c->K * c->C * c->R * c->S / (s * s) + 255) / 256);
        gxn = gxn > 1024 ? 1024 : (gxn < 1 ? 1 : gxn);
        hipLaunchKernelGGL(repack_dgrad_bf16_kernel, dim3(gxn, (unsigned)ncls), dim3(256), 0, st, w, reinterpret_cast<unsigned short*>(wt_ws), ra);
        rc = check_launch("repack_dgrad_bf16_kernel");
        if (rc) return rc;
    }
    return launch_kcs(p, gx_bf16 != 0, st);
}

}  // extern "C"
