// 1x1 convolutions with few input channels (the generator's shortcut convs, DCResNet_models.py:22: C/4 = 32..128 shuffled channels ->
// 64..512 filters) as a stream: y[m][:] = act(x[m][:] W^T + b).  On the generic 128x64 implicit-GEMM tile the whole reduction is one
// K tile, so a launch was prologue + epilogue (24-45 TF, 2.3 TB/s on a layer that only moves bytes).  Here a workgroup walks 128-row
// tiles: the tile's rows sit in LDS (the next tile in registers while this one is multiplied), the filter comes through LDS 64 output
// channels at a time, each wavefront owns 32 rows x 64 outputs (two 32x32 fp32 MFMA tiles, k = 8g + 4h + e on both operands so a
// fragment is one ds_read_b128), bias / activation in the epilogue, 128-byte contiguous stores.  gfx950 only.
#include "common.h"
#include "device_prims.h"
#include "igemm.h"

namespace cslgan {

struct C1Params {
    const float* x;      // [M][C]
    const float* w;      // [K][C]
    const float* bias;   // [K] or null
    float* y;            // [M][K]
    long long M;
    int K, act, n_tiles;
};

template <int C>
__global__ __launch_bounds__(256, C == 32 ? 3 : (C == 64 ? 2 : 1)) void conv1x1_kernel(const C1Params p) {
    constexpr int LD = C + 4, C4 = C / 4;
    constexpr int AREG = 128 * C4 / 256;                 // float4 of a row tile per thread (4, 8 or 16)
    constexpr int WREG = 64 * C4 / 256;                  // float4 of a 64-filter slice per thread
    __shared__ __attribute__((aligned(16))) float As[128 * LD];
    __shared__ __attribute__((aligned(16))) float Ws[64 * LD];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    float4 ra[AREG];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int j = 0; j < AREG; ++j) {
            const int idx = tid + 256 * j;
            const long long row = (long long)tile * 128 + idx / C4;
            ra[j] = row < p.M ? *reinterpret_cast<const float4*>(p.x + row * C + (idx % C4) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    if ((int)blockIdx.x < p.n_tiles) fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        __syncthreads();                                  // the previous tile's reads are done
#pragma unroll
        for (int j = 0; j < AREG; ++j) {
            const int idx = tid + 256 * j;
            *reinterpret_cast<float4*>(&As[(idx / C4) * LD + (idx % C4) * 4]) = ra[j];
        }
        if (tile + (int)gridDim.x < p.n_tiles) fetch(tile + gridDim.x);
        for (int n0 = 0; n0 < p.K; n0 += 64) {
            __syncthreads();                              // As is written / the previous filter slice is consumed
#pragma unroll
            for (int j = 0; j < WREG; ++j) {
                const int idx = tid + 256 * j;
                const int n = idx / C4;
                *reinterpret_cast<float4*>(&Ws[n * LD + (idx % C4) * 4]) =
                    *reinterpret_cast<const float4*>(p.w + (long long)(n0 + n) * C + (idx % C4) * 4);
            }
            __syncthreads();
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
#pragma unroll 4
            for (int g = 0; g < C / 8; ++g) {
                const float4 a = *reinterpret_cast<const float4*>(&As[(wid * 32 + r) * LD + 8 * g + 4 * h]);
                const float4 b0 = *reinterpret_cast<const float4*>(&Ws[r * LD + 8 * g + 4 * h]);
                const float4 b1 = *reinterpret_cast<const float4*>(&Ws[(32 + r) * LD + 8 * g + 4 * h]);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc[0], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc[0], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc[0], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc[1], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc[1], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc[1], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc[1], 0, 0, 0);
            }
            const long long row0 = (long long)tile * 128 + wid * 32 + 4 * h;      // this lane's rows: row0 + (v & 3) + 8 * (v >> 2)
            const int rows_left = (int)(p.M - row0 < 32 ? p.M - row0 : 32);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + j * 32 + r;
                const float bv = p.bias ? p.bias[n] : 0.f;
                float* yj = p.y + row0 * p.K + n;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int ro = (v & 3) + 8 * (v >> 2);
                    if (ro >= rows_left) continue;
                    float val = acc[j][v] + bv;
                    val = apply_act(val, p.act);
                    yj[ro * p.K] = val;
                }
            }
        }
    }
}

bool conv1x1_eligible(const cslgan_conv_t* c, const float* x, const float* w, const float* residual) {
    return !residual && c->compute == CSLGAN_COMPUTE_F32 && c->R == 1 && c->S == 1 && c->stride == 1 && c->pad == 0 &&
           // measured at 128 images: 82 -> 60 us (C = 32, 64x64), 60 -> 49 us (C = 64, 32x32); 128 channels on <= 16x16 grids have too
           // few row tiles to stream (42 -> 48 us, 26 -> 82 us) and stay on the generic kernel
           (c->C == 32 || c->C == 64) && (c->K & 63) == 0 && c->K >= 64 && (long long)c->N * c->H * c->W >= 65536 &&
           aligned16(x) && aligned16(w);
}

int launch_conv1x1(const cslgan_conv_t* c, const float* x, const float* w, const float* bias, int act, float* y, hipStream_t st) {
    C1Params p{};
    p.x = x; p.w = w; p.bias = bias; p.y = y; p.act = act; p.K = c->K;
    p.M = (long long)c->N * c->H * c->W;
    const long long nt = (p.M + 127) / 128;
    CSLGAN_REQUIRE(nt < (1ll << 31), "conv2d_fwd (1x1): too many rows");
    p.n_tiles = (int)nt;
    const int per_cu = c->C == 128 ? 1 : (c->C == 64 ? 2 : 3);       // LDS 101 / 52 / 28 KB per workgroup; registers allow 1 / 2 / 3
    const long long cap = 256ll * per_cu;
    const unsigned grid = (unsigned)(nt < cap ? nt : cap);
    note_kernel("conv1x1_kernel<%d>", c->C);
    if (c->C == 32) hipLaunchKernelGGL(conv1x1_kernel<32>, dim3(grid), dim3(256), 0, st, p);
    else if (c->C == 64) hipLaunchKernelGGL(conv1x1_kernel<64>, dim3(grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(conv1x1_kernel<128>, dim3(grid), dim3(256), 0, st, p);
    return check_launch("conv1x1_kernel");
}

// ---- bf16-stored x, 1x1 convs with 16 / 32 / 64 input channels (the generator's shortcut convs on the shuffled C/4 channels, DCResNet_models.py:22) ----
// A stream over the pixels: the whole reduction is 1-4 MFMA k-steps, so the gather kernel's 64-k tile was mostly padding (C = 16: a
// quarter of it) and its LDS round trip pure overhead — 0.26 ms for a layer whose traffic (67 MB in, 268 MB out at 128x128) is 0.08 ms.
// Here a wavefront owns 32 pixels: its A operand is one 16-byte load per k-step straight from the bf16 rows (a pixel's channels are
// contiguous, 32 pixels = 512-2048 contiguous bytes), the filter lives in registers for the whole kernel, no LDS, no barriers.
template <int CK, int TN, bool OUT_BF16>
__global__ __launch_bounds__(256) void conv1x1s_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ wb, const float* __restrict__ bias,
                                                       long long M, int K, int act, void* __restrict__ y) {
    constexpr int C = CK * 16;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    bf16x8 bw[TN][CK];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int s = 0; s < CK; ++s) {
            const int n = 32 * j + r;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (n < K) v = *reinterpret_cast<const uint4*>(wb + (long long)n * C + 16 * s + 8 * h);
            bw[j][s] = __builtin_bit_cast(bf16x8, v);
        }
    float bv[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) bv[j] = (bias && 32 * j + r < K) ? bias[32 * j + r] : 0.f;
    const long long n_tiles = (M + 31) / 32;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * 4;
    for (long long t = wave0; t < n_tiles; t += n_waves) {
        const long long m = 32 * t + r;
        f32x16 acc[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
#pragma unroll
        for (int s = 0; s < CK; ++s) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (m < M) v = *reinterpret_cast<const uint4*>(x + m * C + 16 * s + 8 * h);
            const bf16x8 a = __builtin_bit_cast(bf16x8, v);
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bw[j][s], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = 32 * j + r;
            if (n >= K) continue;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const long long row = 32 * t + (v & 3) + 8 * (v >> 2) + 4 * h;
                if (row >= M) continue;
                float val = acc[j][v] + bv[j];
                val = apply_act(val, act);
                if (OUT_BF16) reinterpret_cast<unsigned short*>(y)[row * K + n] = bf16_rne(val);
                else reinterpret_cast<float*>(y)[row * K + n] = val;
            }
        }
    }
}

bool conv1x1s_eligible(const cslgan_conv_t* c, const void* residual) {
    return !residual && c->R == 1 && c->S == 1 && c->stride == 1 && c->pad == 0 && (c->C == 16 || c->C == 32 || c->C == 64) &&
           c->K % 32 == 0 && c->K >= 32 && c->K <= 128 && (long long)c->N * c->H * c->W >= 65536;
}

template <int CK>
static int launch_conv1x1s_ck(const cslgan_conv_t* c, const void* x, const void* wb, const float* bias, int act, void* y, int y_bf16, hipStream_t st) {
    const long long M = (long long)c->N * c->H * c->W;
    long long nb = (M / 32 + 3) / 4;
    nb = nb > 2048 ? 2048 : (nb < 1 ? 1 : nb);
    const dim3 grid((unsigned)nb), block(256);
    const unsigned short* xh = reinterpret_cast<const unsigned short*>(x);
    const unsigned short* wh = reinterpret_cast<const unsigned short*>(wb);
    note_kernel("conv1x1s_kernel<%d>", CK * 16);
#define CSL_C1S(TN)                                                                                                          \
    do {                                                                                                                     \
        if (y_bf16) hipLaunchKernelGGL((conv1x1s_kernel<CK, TN, true>), grid, block, 0, st, xh, wh, bias, M, c->K, act, y);   \
        else hipLaunchKernelGGL((conv1x1s_kernel<CK, TN, false>), grid, block, 0, st, xh, wh, bias, M, c->K, act, y);         \
    } while (0)
    const int tn = c->K / 32;
    if (tn == 1) CSL_C1S(1);
    else if (tn == 2) CSL_C1S(2);
    else if (tn == 3) CSL_C1S(3);
    else CSL_C1S(4);
#undef CSL_C1S
    return check_launch("conv1x1s_kernel");
}

int launch_conv1x1s(const cslgan_conv_t* c, const void* x, const void* wb, const float* bias, int act, void* y, int y_bf16, hipStream_t st) {
    if (c->C == 16) return launch_conv1x1s_ck<1>(c, x, wb, bias, act, y, y_bf16, st);
    if (c->C == 32) return launch_conv1x1s_ck<2>(c, x, wb, bias, act, y, y_bf16, st);
    return launch_conv1x1s_ck<4>(c, x, wb, bias, act, y, y_bf16, st);
}

}  // namespace cslgan
