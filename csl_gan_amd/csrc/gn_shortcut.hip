// ResBlockUp's bn1 apply, depth-to-space shuffle and 1x1 shortcut conv (DCResNet_models.py:29-34) in one streaming kernel.
// The two-launch form wrote the raw input x a second time in the shuffled layout only for the shortcut conv to read it once; here
// a loaded float4 of x[n][h][w][4c' .. 4c'+3] — the four sub-pixels (i, j) of shuffled channel c' — is normalised and stored to
// a_ps from registers and its raw values go to four LDS sub-tiles [ij][row][C/4 + 4], from which the shortcut
//   s[n][2h+i][2w+j][k] = bias[k] + sum_c' wf[k][c'] x[n][h][w][4c'+2i+j]
// is multiplied exactly as conv1x1_kernel does (csrc/conv1x1.hip: 32x32x2 fp32 MFMA, k = 8g + 4h + e on both operands so a
// fragment is one ds_read_b128, the filter through LDS 64 outputs at a time, the next tile's rows in registers meanwhile).
// A workgroup walks TR-source-row tiles of ONE image: mean, rstd, gamma and beta are per-thread constants (256 % (C/4) == 0).
// TR = 32: wavefront w multiplies sub-tile ij = w (32 output rows x 64 filters); TR = 16 (C/4 = 128, where 32 rows of 512
// channels and a filter slice would leave one workgroup per CU): 64 output rows, wavefront w takes rows 32 (w & 1) .. and filters
// 32 (w >> 1) .. of the slice.  gfx950 only.
#include "common.h"
#include "device_prims.h"
#include "gn_apply.h"

namespace cslgan {

constexpr int GS_MAX_GROUPS = 256;

struct GsParams {
    const float* x;      // [N][HW][C]
    const float* gamma;  // [C]
    const float* beta;   // [C]
    const float* part;   // [N][n_part][groups][2]
    const float* wf;     // [K][C/4]
    const float* bias;   // [K] or null
    float* stats;        // [N][groups][2]
    float* a_ps;         // [N][2H][2W][C/4]
    float* s;            // [N][2H][2W][K]
    int HW, W, cpg, n_groups, n_part, K, relu, tiles;      // tiles: per image
    float eps;
};

template <int CQ, int TR>
__global__ __launch_bounds__(256, CQ == 32 ? 4 : 2) void gn_shortcut_kernel(const GsParams p) {
    constexpr int LD = CQ + 4, C = 4 * CQ, ROWS = 4 * TR;
    constexpr int RSTEP = 256 / CQ, AREG = TR / RSTEP;   // source rows per pass of the workgroup, float4 of a tile per thread
    constexpr int WREG = 64 * (CQ / 4) / 256;            // float4 of a 64-filter slice per thread
    constexpr int NT = TR == 32 ? 2 : 1;                 // 32-filter tiles per wavefront
    __shared__ __attribute__((aligned(16))) float As[ROWS * LD];
    __shared__ __attribute__((aligned(16))) float Ws[64 * LD];
    __shared__ int s_row[ROWS];                          // output pixel (within the image) of each tile row
    __shared__ float s_st[2 * GS_MAX_GROUPS];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int cq = tid & (CQ - 1), rl0 = tid / CQ;
    const long long n = blockIdx.y;
    const float cnt = (float)p.HW * (float)p.cpg;
    const float inv_cnt = 1.f / cnt;
    gn_combine_chan(p.part, n, p.n_part, p.n_groups, cnt, s_st, p.stats, blockIdx.x == 0);
    __syncthreads();
    float mean[4], rstd[4], ga[4], be[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        gn_group_stat(s_st, (4 * cq + e) / p.cpg, inv_cnt, p.eps, mean[e], rstd[e]);
        ga[e] = p.gamma[4 * cq + e];
        be[e] = p.beta[4 * cq + e];
    }
    const float* xi = p.x + n * p.HW * C;
    float* ai = p.a_ps + n * p.HW * C;
    float* si = p.s + n * 4 * p.HW * p.K;                // launcher: 4 * HW * K < 2^31
    const int W = p.W;
    const int arow = (TR == 32 ? wid : (wid & 1)) * 32;  // this wavefront's rows of As
    const int fo = TR == 32 ? 0 : (wid >> 1) * 32;       // and its filters of a slice

    float4 ra[AREG];                                      // the next tile's rows and the next filter slice wait in registers
    f32x4 rw[WREG];                                       // (a native vector: plain copies of a float4 struct become a memcpy through scratch)
    float rb[NT], bv[NT];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int j = 0; j < AREG; ++j)
            ra[j] = *reinterpret_cast<const float4*>(xi + (size_t)(tile * TR + rl0 + j * RSTEP) * C + 4 * cq);
    };
    auto fetch_w = [&](int n0) {
#pragma unroll
        for (int j = 0; j < WREG; ++j) {
            const int idx = tid + 256 * j;
            rw[j] = *reinterpret_cast<const f32x4*>(p.wf + (size_t)(n0 + idx / (CQ / 4)) * CQ + (idx % (CQ / 4)) * 4);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) rb[j] = p.bias ? p.bias[n0 + fo + j * 32 + r] : 0.f;
    };
    const int first = blockIdx.x;
    if (first < p.tiles) {
        fetch(first);
        fetch_w(0);
    }
    for (int tile = first; tile < p.tiles; tile += gridDim.x) {
        __syncthreads();                                  // the previous tile's reads are done
        if (tid < ROWS) {
            const unsigned rl = tile * TR + (tid % TR), hh = rl / (unsigned)W, ww = rl - hh * (unsigned)W;
            const int ij = tid / TR;
            s_row[tid] = (2 * hh + (ij >> 1)) * 2 * W + 2 * ww + (ij & 1);
        }
#pragma unroll
        for (int j = 0; j < AREG; ++j) {
            const int row = rl0 + j * RSTEP;
            const unsigned rl = tile * TR + row, hh = rl / (unsigned)W, ww = rl - hh * (unsigned)W;
            const float in[4] = {ra[j].x, ra[j].y, ra[j].z, ra[j].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {                 // lanes hold consecutive c': coalesced stores, conflict-free LDS writes
                As[(e * TR + row) * LD + cq] = in[e];
                ai[(size_t)((2 * hh + (e >> 1)) * 2 * W + 2 * ww + (e & 1)) * CQ + cq] = gn_apply(in[e], mean[e], rstd[e], ga[e], be[e], p.relu);
            }
        }
        if (tile + (int)gridDim.x < p.tiles) fetch(tile + gridDim.x);
        for (int n0 = 0; n0 < p.K; n0 += 64) {
            if (n0) __syncthreads();                      // the previous filter slice is consumed
#pragma unroll
            for (int j = 0; j < WREG; ++j) {
                const int idx = tid + 256 * j;
                *reinterpret_cast<f32x4*>(&Ws[(idx / (CQ / 4)) * LD + (idx % (CQ / 4)) * 4]) = rw[j];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[j] = rb[j];
            fetch_w(n0 + 64 < p.K ? n0 + 64 : 0);         // the next slice (of the next tile) lands under this one's MFMAs
            __syncthreads();                              // As, s_row and Ws are written
            f32x16 acc[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
#pragma unroll 4
            for (int g = 0; g < CQ / 8; ++g) {
                const float4 a = *reinterpret_cast<const float4*>(&As[(arow + r) * LD + 8 * g + 4 * h]);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float4 b = *reinterpret_cast<const float4*>(&Ws[(fo + j * 32 + r) * LD + 8 * g + 4 * h]);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int f = n0 + fo + j * 32 + r;
#pragma unroll
                for (int v = 0; v < 16; ++v)              // this lane's rows: arow + 4h + (v & 3) + 8 * (v >> 2)
                    si[s_row[arow + 4 * h + (v & 3) + 8 * (v >> 2)] * p.K + f] = acc[j][v] + bv[j];
            }
        }
    }
}

template <int CQ, int TR>
static int launch_gn_shortcut(GsParams& p, int N, int per_cu, hipStream_t st) {
    p.tiles = p.HW / TR;                                  // HW is a multiple of 64
    int gx = 256 * per_cu / N;
    gx = gx < 1 ? 1 : (gx > p.tiles ? p.tiles : gx);
    const int walk = (p.tiles + gx - 1) / gx;             // tiles per workgroup; then no more workgroups than that needs
    gx = (p.tiles + walk - 1) / walk;
    note_kernel("gn_shortcut_kernel<%d>", CQ);
    hipLaunchKernelGGL((gn_shortcut_kernel<CQ, TR>), dim3((unsigned)gx, (unsigned)N), dim3(256), 0, st, p);
    return check_launch("gn_shortcut_kernel");
}

}  // namespace cslgan

using namespace cslgan;

extern "C" int cslgan_groupnorm_apply_parts_shortcut_f32(const float* x, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                                                         float eps, int relu, const float* part, int n_part, float* stats_ws, float* y,
                                                         int d2s_W, const float* wf, const float* bias, int K, float* s, void* stream) {
    CSLGAN_REQUIRE(x && gamma && beta && part && stats_ws && y && wf && s, "groupnorm_apply_parts_shortcut: null argument");
    CSLGAN_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 4 == 0, "groupnorm_apply_parts_shortcut: needs C %% 4 == 0 (C=%d)", C);
    CSLGAN_REQUIRE(groups > 0 && groups <= GS_MAX_GROUPS && C % groups == 0,
                   "groupnorm_apply_parts_shortcut: C=%d not divisible by groups=%d (at most %d groups)", C, groups, GS_MAX_GROUPS);
    CSLGAN_REQUIRE(C == 128 || C == 256 || C == 512, "groupnorm_apply_parts_shortcut: C / 4 must be 32, 64 or 128 (C=%d)", C);
    CSLGAN_REQUIRE(K >= 64 && K % 64 == 0, "groupnorm_apply_parts_shortcut: K=%d is not a multiple of 64", K);
    CSLGAN_REQUIRE(N <= 65535 && n_part >= 1 && n_part <= CSLGAN_NORM_PARTIAL_BLOCKS && HW == 64 * n_part,
                   "groupnorm_apply_parts_shortcut: needs HW == 64 * n_part <= %d * 64 (n_part=%d)", CSLGAN_NORM_PARTIAL_BLOCKS, n_part);
    CSLGAN_REQUIRE(d2s_W > 0 && HW % d2s_W == 0, "groupnorm_apply_parts_shortcut: d2s_W=%d does not divide the %d pixels of an image", d2s_W, HW);
    CSLGAN_REQUIRE(4ll * HW * K < (1ll << 31), "groupnorm_apply_parts_shortcut: image of %d x %d outputs too large", 4 * HW, K);
    CSLGAN_REQUIRE(aligned16(x) && aligned16(y) && aligned16(wf) && aligned16(s), "groupnorm_apply_parts_shortcut: misaligned pointer");
    GsParams p{};
    p.x = x; p.gamma = gamma; p.beta = beta; p.part = part; p.wf = wf; p.bias = bias; p.stats = stats_ws; p.a_ps = y; p.s = s;
    p.HW = HW; p.W = d2s_W; p.cpg = C / groups; p.n_groups = groups; p.n_part = n_part; p.K = K; p.relu = relu; p.eps = eps;
    hipStream_t st = (hipStream_t)stream;
    // workgroups per CU: LDS 30 / 54 / 68 KB and the register budget of the launch bounds
    if (C == 128) return launch_gn_shortcut<32, 32>(p, N, 4, st);
    if (C == 256) return launch_gn_shortcut<64, 32>(p, N, 2, st);
    return launch_gn_shortcut<128, 16>(p, N, 2, st);
}
