// Weight gradients on bf16-STORED tensors (the storage mode of igemm_bf16s.hip): grouped / per-sample gradients and clip-weighted sums
// from bfloat16 gy and x, fp32 accumulation, in the M-contiguous form of igemm_mc.hip through gfx950's transposing LDS read.  gfx950 only.
// Replaces (reference file:line): the Opacus-fork per-sample weight gradients (train.py:373,387), clip() + accumulate (train.py:399-402).
#include "common.h"
#include "device_prims.h"
#include "igemm.h"
#include "conv_classes.h"

namespace cslgan {

// ---- M-contiguous form (weight gradient) on bf16 tensors ----------------------------------------------------------------------
//   gw[g][m][n] = alpha * sum_{k in group g} GY[k][m] * X(k, n),   k -> (img, oy, ox),  n -> (tap, c)
struct MsParams {
    const void* gy;      // bf16 [N][P][Q][Kc]
    const void* x;       // bf16 [N][H][W][C]
    int N, H, W, C, P, Q, Kc, T, Ndim, stride, group, n_groups;
    float alpha;
    void* gw;            // [n_groups][Kc][Ndim] fp32 (bf16 when out_bf16) or null
    int out_bf16;
    float* sq;           // [n_groups] or null
    int tiles_m, tiles_n, ksplit;
    const float* row_scale;   // igemm_mcs_tr_kernel<., true>: [N] fp32 weight of each sample's WHOLE gradient, applied in fp32 to the sample's
                              // accumulated product (clip-weighted sums: sum_b f_b g_b with every g_b exactly the bf16-MFMA gradient)
    signed char ty[IG_MAX_TAPS], tx[IG_MAX_TAPS];
};

constexpr int MS_BK = 64;        // pixels per LDS tile

// The [pixel][channel] tiles go to LDS as they are loaded (row-major, 256-byte rows,
// 16-byte chunks XOR-swizzled by the row so that both the row writes and the transposed reads are conflict-free) and the MFMA
// operands come back through ds_read_b64_tr_b16, gfx950's transposing LDS read: per 16-lane group a block of 4 rows (pixels) x 16
// columns (channels) is delivered column-major, i.e. each lane receives 4 consecutive k of ITS channel; two such reads are one
// operand of v_mfma_f32_32x32x16_bf16.  A K tile is 8 global loads, 8 ds_write_b128 and 32 transposed reads per thread (an earlier
// form that transposed 8x8 blocks in registers cost ~100 vector instructions per thread and K tile beside 16 MFMAs per wave and
// measured 176-208 TF against 259-339 TF here; DESIGN.md, appendix of retired switches).
// Q8: Q % 8 == 0, so the 8 consecutive pixels a thread gathers lie in one output row of one image (one decode per tile).

// SCALED (clip-weighted sums for ghost clipping): P*Q is a multiple of the 64-pixel K tile, so every K tile lies
// in ONE sample; when a sample's last tile has been multiplied its accumulated product is folded into a second accumulator with the
// sample's fp32 weight (acc_sum += f_b * acc; acc = 0).  The weight never touches a bfloat16 operand: the summed contribution of
// sample b is f_b times exactly the gradient the unscaled kernel materialises, so the clipped sum keeps the sensitivity bound to fp32
// rounding (scaling gy by f_b before the matrix core would round f_b * gy to bfloat16: a 2^-8 relative slack on that bound).
template <bool Q8, bool SCALED = false>
__global__ __launch_bounds__(256, 2) void igemm_mcs_tr_kernel(const MsParams p) {
    constexpr int OPB = 64 * 256;                           // bytes of one operand tile: 64 pixels x 128 channels x 2 B
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * OPB];     // [buffer][operand]
    __shared__ float s_red[4];

    const int tid = threadIdx.x;
    const int per_g = p.tiles_m * p.tiles_n;
    const int split = p.ksplit > 1 ? blockIdx.x % p.ksplit : 0;
    const int bid = p.ksplit > 1 ? blockIdx.x / p.ksplit : blockIdx.x;
    const int g = bid / per_g;
    const int tl = bid - g * per_g;
    const int tile_m = tl / p.tiles_n, tile_n = tl - tile_m * p.tiles_n;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int PQ = p.P * p.Q;
    const int Ktot = p.group * PQ;
    const long long pix_base = (long long)g * p.group * PQ;

    const bool is_a = tid < 128;
    const int lt = tid & 127;
    const int c16 = lt & 15;             // this thread's 16-byte chunk (8 channels) of a pixel row: 16 lanes cover its 256 bytes
    const int c8 = c16 * 8;
    const int kg = lt >> 4;              // its group of 8 pixels within the 64-pixel tile
    const int nb = n0 + c8;
    const bool b_ok = nb < p.Ndim;
    const int b_t = b_ok ? nb / p.C : 0;
    const int b_c = nb - b_t * p.C;
    const int b_ty = p.ty[b_t], b_tx = p.tx[b_t];
    const bool a_ok = m0 + c8 < p.Kc;
    // buffer loads with branch-free offsets (an invalid element ORs BUF_OOB into its offset -> the range check returns zeros): see
    // igemm_kcs_kernel — as `if (valid) v = *ptr` every load sat in its own exec-masked block
    const __amdgpu_buffer_rsrc_t gy_rsrc = make_rsrc(p.gy, (unsigned)(2ll * p.N * PQ * p.Kc));
    const __amdgpu_buffer_rsrc_t x_rsrc = make_rsrc(p.x, (unsigned)(2ll * p.N * p.H * p.W * p.C));
    auto bld = [](__amdgpu_buffer_rsrc_t r, unsigned off) {
        const u32x4 v = buf_load4_raw(r, off);
        return make_uint4(v[0], v[1], v[2], v[3]);
    };

    // two register sets: tile t+2 is loaded under the MFMAs of tile t and written to LDS after those of tile t+1 (see igemm_kcs_kernel)
    uint4 rv0[8], rv1[8];
    int k_lim = Ktot;            // pixels this workgroup may read (its K range when the reduction is split): past it every load is zero
    auto load_tile = [&](int kt, uint4 (&rv)[8]) {
        const int kk0 = kt * MS_BK + kg * 8;
        if (is_a) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                rv[j] = bld(gy_rsrc, (2u * (((unsigned)pix_base + (unsigned)(kk0 + j)) * (unsigned)p.Kc + (unsigned)(m0 + c8))) | ((a_ok && kk0 + j < k_lim) ? 0u : BUF_OOB));
        } else if (Q8) {
            const int il = kk0 / PQ;
            const int pix = kk0 - il * PQ;
            const int oy = pix / p.Q, ox0 = pix - oy * p.Q;
            const int img = g * p.group + il;           // (32-bit: the entry checks that both operands are below 4 GB)
            const int iy = oy * p.stride + b_ty;
            const unsigned row_bad = (b_ok && kk0 < k_lim && iy >= 0 && iy < p.H) ? 0u : BUF_OOB;
            const unsigned src = 2u * (unsigned)(((img * p.H + iy) * p.W) * p.C + b_c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ix = (ox0 + j) * p.stride + b_tx;
                rv[j] = bld(x_rsrc, (src + 2u * (unsigned)(ix * p.C)) | row_bad | ((unsigned)ix < (unsigned)p.W ? 0u : BUF_OOB));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = kk0 + j;
                const int kc2 = kk < k_lim ? kk : 0;
                const int il = kc2 / PQ;
                const int pix = kc2 - il * PQ;
                const int oy = pix / p.Q, ox = pix - oy * p.Q;
                const int img = g * p.group + il;
                const int iy = oy * p.stride + b_ty, ix = ox * p.stride + b_tx;
                const bool ok = b_ok && kk < k_lim && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                rv[j] = bld(x_rsrc, (2u * (unsigned)(((img * p.H + iy) * p.W + ix) * p.C + b_c)) | (ok ? 0u : BUF_OOB));
            }
        }
    };
    // row (pixel) kr of a tile, 16-byte chunk ch: byte offset 256*kr + 16*(ch ^ (((kr & 3) << 2) | ((kr >> 2) & 3)))
    auto store_tile = [&](int buf, const uint4 (&rv)[8]) {
        unsigned char* dst = smem + (buf * 2 + (is_a ? 0 : 1)) * OPB;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kr = kg * 8 + j;
            const int sw = ((j & 3) << 2) | ((kr >> 2) & 3);
            *reinterpret_cast<uint4*>(dst + 256 * kr + 16 * (c16 ^ sw)) = rv[j];
        }
    };

    const int lane = tid & 63, wid = tid >> 6;
    const int h = lane >> 5;
    const int wm = wid >> 1, wn = wid & 1;
    // transposed-read addresses (bytes within an operand tile) of this lane for k-step 0: [4-row half u][32-row tile i]
    const int gq = (lane >> 2) & 3, gp = lane & 3, ghalf = (lane >> 4) & 1;       // row q and column quad p within the 16-lane group; which 16 of the 32 rows
    int a_tr[2][2], b_tr[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int kr = 8 * h + 4 * u + gq;
            const int sw = (gq << 2) | ((2 * h + u) & 3);
            const int cha = (wm * 64 + i * 32) / 8 + 2 * ghalf + (gp >> 1), chb = (wn * 64 + i * 32) / 8 + 2 * ghalf + (gp >> 1);
            a_tr[u][i] = 256 * kr + 16 * (cha ^ sw) + 8 * (gp & 1);
            b_tr[u][i] = 256 * kr + 16 * (chb ^ sw) + 8 * (gp & 1);
        }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    const int nk_all = (Ktot + MS_BK - 1) / MS_BK;
    int kt0 = 0, nk = nk_all;
    if (p.ksplit > 1) {
        const int per = (nk_all + p.ksplit - 1) / p.ksplit;
        kt0 = split * per;
        nk = kt0 + per < nk_all ? kt0 + per : nk_all;
        if (kt0 >= nk) return;      // uniform across the workgroup
    }
    k_lim = nk * MS_BK < Ktot ? nk * MS_BK : Ktot;
    auto mma_tile = [&](int buf) {
        const unsigned char* As = smem + (buf * 2) * OPB;
        const unsigned char* Bs = As + OPB;
#pragma unroll
        for (int s = 0; s < 4; ++s) {       // 16 pixels per step: rows 16 s .. 16 s + 15 = +4096 bytes per step
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(As + a_tr[0][i] + 4096 * s));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(As + a_tr[1][i] + 4096 * s));
                const uint4 w = make_uint4(__builtin_bit_cast(uint2, lo).x, __builtin_bit_cast(uint2, lo).y, __builtin_bit_cast(uint2, hi).x, __builtin_bit_cast(uint2, hi).y);
                af[i] = __builtin_bit_cast(bf16x8, w);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(Bs + b_tr[0][j] + 4096 * s));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(Bs + b_tr[1][j] + 4096 * s));
                const uint4 w = make_uint4(__builtin_bit_cast(uint2, lo).x, __builtin_bit_cast(uint2, lo).y, __builtin_bit_cast(uint2, hi).x, __builtin_bit_cast(uint2, hi).y);
                bf[j] = __builtin_bit_cast(bf16x8, w);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    };
    if (SCALED) {
        // one register set (the second accumulator needs the registers); a sample = tiles_per_sample consecutive K tiles
        f32x16 acc_sum[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc_sum[i][j][v] = 0.f;
        const int tps = PQ / MS_BK;
        load_tile(kt0, rv0);
        store_tile(0, rv0);
        __syncthreads();
        int in_sample = 0;
        for (int kt = kt0; kt < nk; ++kt) {
            const int buf = (kt - kt0) & 1;
            if (kt + 1 < nk) load_tile(kt + 1, rv0);
            mma_tile(buf);
            if (++in_sample == tps) {            // uniform: the sample's product is complete
                in_sample = 0;
                const float f = p.row_scale[(long long)g * p.group + kt / tps];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int v = 0; v < 16; ++v) { acc_sum[i][j][v] = fmaf(f, acc[i][j][v], acc_sum[i][j][v]); acc[i][j][v] = 0.f; }
            }
            if (kt + 1 < nk) store_tile(buf ^ 1, rv0);
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = acc_sum[i][j];
    } else {
    load_tile(kt0, rv0);
    load_tile(kt0 + 1, rv1);         // past the group's pixels every lane loads zeros (kk >= Ktot)
    store_tile(0, rv0);
    __syncthreads();
    for (int kt = kt0; kt < nk; kt += 2) {      // one loop exit (see igemm_kcs_kernel): an odd tile count multiplies one all-zero tile
        load_tile(kt + 2, rv0);
        mma_tile(0);
        store_tile(1, rv1);          // tile kt + 1 (zeros past k_lim)
        __syncthreads();
        load_tile(kt + 3, rv1);
        mma_tile(1);
        store_tile(0, rv0);          // tile kt + 2
        __syncthreads();
    }
    }

    // ---- epilogue: scale, store, per-group sum of squares (as igemm_mc) ------------------------
    const int r = lane & 31;
    float ss = 0.f;
    float* __restrict__ outg = (p.gw && !p.out_bf16) ? reinterpret_cast<float*>(p.gw) + (long long)g * p.Kc * p.Ndim : nullptr;
    unsigned short* __restrict__ outh = (p.gw && p.out_bf16) ? reinterpret_cast<unsigned short*>(p.gw) + (long long)g * p.Kc * p.Ndim : nullptr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + r;
        if (n >= p.Ndim) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = m0 + wm * 64 + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                if (m >= p.Kc) continue;
                float val = p.alpha * acc[i][j][v];
                if (p.out_bf16) {
                    const unsigned short u = bf16_rne(val);
                    if (outh) outh[(long long)m * p.Ndim + n] = u;
                    val = bf2f(u);
                }
                ss = fmaf(val, val, ss);
                if (outg) {
                    if (p.ksplit > 1) atomicAdd(&outg[(long long)m * p.Ndim + n], val);
                    else outg[(long long)m * p.Ndim + n] = val;
                }
            }
        }
    }
    if (p.sq && p.ksplit <= 1) {
        const float tot = block_sum_256(ss, s_red);
        if (tid == 0) atomicAdd(p.sq + g, tot);
    }
}

// The argument checks both entries share, after their own null checks; `who` prefixes the messages.
static int mcs_check(const cslgan_conv_t* c, const void* gy, const void* x, int group, const char* who) {
    if (int rc = check_conv(c, who, false)) return rc;
    CSLGAN_REQUIRE(group >= 1 && c->N % group == 0, "%s: N=%d not divisible by group=%d", who, c->N, group);
    CSLGAN_REQUIRE(c->K % 8 == 0 && c->C % 8 == 0 && aligned16(gy) && aligned16(x), "%s: K and C must be multiples of 8, operands 16-byte aligned", who);
    CSLGAN_REQUIRE(2ll * c->N * c->P * c->Q * c->K < (long long)BUF_OOB && 2ll * c->N * c->H * c->W * c->C < (long long)BUF_OOB, "%s: operand larger than 4 GB", who);
    return CSLGAN_OK;
}

// Launch parameters of a checked call: 128x128 tiles, K not split.
static MsParams mcs_params(const cslgan_conv_t* c, const void* gy, const void* x, int group, float alpha, void* gw, int gw_bf16, float* sq,
                           const float* row_scale) {
    MsParams p{};
    p.gy = gy; p.x = x; p.N = c->N; p.H = c->H; p.W = c->W; p.C = c->C; p.P = c->P; p.Q = c->Q; p.Kc = c->K;
    p.T = c->R * c->S; p.Ndim = p.T * c->C; p.stride = c->stride; p.group = group; p.n_groups = c->N / group;
    p.alpha = alpha; p.gw = gw; p.sq = sq; p.out_bf16 = gw_bf16; p.row_scale = row_scale; p.ksplit = 1;
    fill_forward_taps(p.ty, p.tx, c->R, c->S, c->pad);
    p.tiles_m = (p.Kc + 127) / 128;
    p.tiles_n = (p.Ndim + 127) / 128;
    return p;
}

// The launch of both entries: row_scale selects the clip-weighted kernel, Q % 8 == 0 the one-decode-per-tile loader.
static int mcs_launch(const MsParams& p, const char* who, hipStream_t st) {
    const long long nb = (long long)p.n_groups * p.tiles_m * p.tiles_n * p.ksplit;
    CSLGAN_REQUIRE(nb <= 0x7fffffffll, "%s: grid too large", who);
    const dim3 grid((unsigned)nb), block(256);
    note_kernel(p.row_scale ? "igemm_mcs_tr_kernel<128,128,scaled>" : "igemm_mcs_tr_kernel<128,128>");
    const bool q8 = p.Q % 8 == 0;
    auto kernel = p.row_scale ? (q8 ? igemm_mcs_tr_kernel<true, true> : igemm_mcs_tr_kernel<false, true>)
                              : (q8 ? igemm_mcs_tr_kernel<true, false> : igemm_mcs_tr_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, st, p);
    return check_launch("igemm_mcs_tr_kernel");
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

// gw[N/group][K][R][S][C] (fp32, or bf16 when gw_bf16) and / or sq[N/group] += ||alpha * gw_g||^2 from bf16 gy [N,P,Q,K] and
// bf16 x [N,H,W,C] (K % 8 == 0, C % 8 == 0).
int cslgan_conv2d_wgrad_grouped_bf16s(const cslgan_conv_t* c, const void* gy, const void* x, int group, float alpha, void* gw, int gw_bf16,
                                      float* sq, void* stream) {
    CSLGAN_REQUIRE(c && gy && x, "conv2d_wgrad_bf16s: null argument");
    CSLGAN_REQUIRE(gw || sq, "conv2d_wgrad_bf16s: neither gw nor sq requested");
    int rc = mcs_check(c, gy, x, group, "conv2d_wgrad_bf16s");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    MsParams p = mcs_params(c, gy, x, group, alpha, gw, gw_bf16, sq, nullptr);
    if ((rc = wgrad_plan_split(p, MS_BK, 8, 2, st))) return rc;
    if ((rc = mcs_launch(p, "conv2d_wgrad_bf16s", st))) return rc;
    return wgrad_split_norms(p, st);
}

// gw[N/group][K][R][S][C] (fp32) = alpha * sum_{n in group} row_scale[n] * (per-sample weight gradient of sample n), from bf16 gy and
// bf16 x: clip() + accumulate for ghost-clipped layers (train.py:399-402) in the bf16 storage mode.  row_scale [N] fp32 is applied in
// fp32 to each sample's accumulated product (igemm_mcs_tr_kernel<., true>), never to a bfloat16 operand.  Needs P*Q % 64 == 0.
int cslgan_conv2d_wgrad_scaled_bf16s(const cslgan_conv_t* c, const void* gy, const void* x, const float* row_scale, int group, float alpha,
                                     float* gw, void* stream) {
    CSLGAN_REQUIRE(c && gy && x && row_scale && gw, "conv2d_wgrad_scaled_bf16s: null argument");
    if (int rc = mcs_check(c, gy, x, group, "conv2d_wgrad_scaled_bf16s")) return rc;
    CSLGAN_REQUIRE((c->P * c->Q) % MS_BK == 0, "conv2d_wgrad_scaled_bf16s: P*Q=%d is not a multiple of %d (a K tile must lie in one sample)", c->P * c->Q, MS_BK);
    return mcs_launch(mcs_params(c, gy, x, group, alpha, gw, 0, nullptr, row_scale), "conv2d_wgrad_scaled_bf16s", (hipStream_t)stream);
}

}  // extern "C"
