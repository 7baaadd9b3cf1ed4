// Layout streams (HBM-bound, no arithmetic beyond a scale): depth-to-space and its inverse, the fold / unfold of four channel groups
// that goes with it, and the uint8 <-> fp32 image conversions of the input pipeline and the sample cache.  gfx950 only.
// Replaces (reference file:line): cat([x]*4) + pixel_shuffle(2) of UpsampleConv DCResNet_models.py:13-15; datasets.py:41-47.
#include "common.h"
#include "device_prims.h"

namespace cslgan {

// ps[n][2h+i][2w+j][c'] = x[n][h][w][4c'+2i+j]  (INVERSE: x from ps — the backward of the forward and vice versa)
template <bool INVERSE>
__global__ void depth_to_space_kernel(const float* __restrict__ in, long long rows, int H, int W, int C, float* __restrict__ out) {
    const int Cq = C >> 2;
    const long long n4 = rows * Cq;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / Cq;
        const int cq = (int)(i - r * Cq);
        if (INVERSE) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = in[d2s_offset(r, e, H, W, Cq) + cq];
            reinterpret_cast<float4*>(out)[i] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            const float4 v = reinterpret_cast<const float4*>(in)[i];
            const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) out[d2s_offset(r, e, H, W, Cq) + cq] = a[e];
        }
    }
}

// The conv after the depth-to-space sees four identical channel groups, so it equals a conv over C/4 channels with
//   wf[row][c'] = sum_q w[row][c' + q*C/4]      (row = (k, r, s) of a KRSC filter)
// UNFOLD is its transpose (the gradient of w from the gradient of wf): gw[row][c' + q*C/4] = gwf[row][c'].
template <bool UNFOLD>
__global__ void fold_channels4_kernel(const float* __restrict__ in, long long rows, int C, float* __restrict__ out) {
    const int Cq = C >> 2;
    const long long n = rows * Cq;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / Cq;
        const int cq = (int)(i - r * Cq);
        if (UNFOLD) {
            const float v = in[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) out[r * C + q * Cq + cq] = v;
        } else {
            const float* b = in + r * C + cq;
            out[i] = (b[0] + b[Cq]) + (b[2 * Cq] + b[3 * Cq]);
        }
    }
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

// ---- input pipeline (round 4): uint8 NHWC image rows -> normalised fp32 NHWC, with the per-image horizontal flip -------------------
// out[n][h][w][c] = src[n][h][flip[n] ? W-1-w : w][c] * scale + bias     (datasets.py:41-47: ToTensor, RandomHorizontalFlip, Normalize)
__global__ void u8_to_f32_nhwc_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ flip, int N, int H, int W, int C,
                                      float scale, float bias, float* __restrict__ out) {
    const long long total = (long long)N * H * W * C;
    const long long per_img = (long long)H * W * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / per_img;
        long long si = i;
        if (flip && flip[n]) {
            const long long r = i - n * per_img;
            const long long row = r / ((long long)W * C);
            const int wc = (int)(r - row * W * C);
            const int w = wc / C, c = wc - w * C;
            si = n * per_img + row * W * C + (long long)(W - 1 - w) * C + c;
        }
        out[i] = (float)src[si] * scale + bias;
    }
}

int cslgan_u8_to_f32_nhwc(const void* src_u8, const void* flip_u8, int N, int H, int W, int C, float scale, float bias, float* out, void* stream) {
    CSLGAN_REQUIRE(src_u8 && out, "u8_to_f32_nhwc: null argument");
    CSLGAN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "u8_to_f32_nhwc: non-positive dimension");
    const long long total = (long long)N * H * W * C;
    unsigned nb = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL(u8_to_f32_nhwc_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned char*>(src_u8),
                       reinterpret_cast<const unsigned char*>(flip_u8), N, H, W, C, scale, bias, out);
    return check_launch("u8_to_f32_nhwc_kernel");
}

// ---- the inverse: fp32 images -> uint8 rows of the cache (util.denorm_celeba + util.save_image's quantisation, elementwise) -----------
//   t = clamp(src * scale + bias, 0, 1);  dst = (uint8) clamp(t * 255 + 0.5, 0, 255)        truncation; NaN -> 0
// Bit-identical to the host's fp32 expression: every product and sum is rounded on its own (no contraction into an fma, which
// would skip the product's rounding and can move a value across a (k + 0.5) / 255 boundary), in the host's order.
__device__ __forceinline__ unsigned quantise_u8(float x, float scale, float bias) {
#pragma clang fp contract(off)
    float t = x * scale;
    t = t + bias;
    t = fminf(fmaxf(t, 0.f), 1.f);               // fmaxf(NaN, 0) = 0
    float u = t * 255.f;
    u = u + 0.5f;
    u = fminf(fmaxf(u, 0.f), 255.f);
    return (unsigned)u;
}

// vec: src 16-byte and dst 4-byte aligned — one float4 load and one packed 4-byte store per thread and step; the n % 4 tail and
// misaligned slices go element by element.
__global__ __launch_bounds__(256) void f32_to_u8_kernel(const float* __restrict__ src, long long n, float scale, float bias,
                                                        unsigned char* __restrict__ dst, int vec) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    long long done = 0;
    if (vec) {
        const long long n4 = n >> 2;
        for (long long i = tid; i < n4; i += nth) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            reinterpret_cast<unsigned*>(dst)[i] = quantise_u8(v.x, scale, bias) | (quantise_u8(v.y, scale, bias) << 8) |
                                                  (quantise_u8(v.z, scale, bias) << 16) | (quantise_u8(v.w, scale, bias) << 24);
        }
        done = n4 << 2;
    }
    for (long long i = done + tid; i < n; i += nth) dst[i] = (unsigned char)quantise_u8(src[i], scale, bias);
}

int cslgan_f32_to_u8(const float* src, int64_t n, float scale, float bias, void* dst_u8, void* stream) {
    CSLGAN_REQUIRE(src && dst_u8, "f32_to_u8: null argument");
    CSLGAN_REQUIRE(n > 0, "f32_to_u8: n=%lld must be positive", (long long)n);
    const int vec = (aligned16(src) && (reinterpret_cast<uintptr_t>(dst_u8) & 3u) == 0) ? 1 : 0;
    hipLaunchKernelGGL(f32_to_u8_kernel, dim3(grid_for(n, vec ? 4 : 1)), dim3(256), 0, (hipStream_t)stream, src, (long long)n, scale, bias,
                       reinterpret_cast<unsigned char*>(dst_u8), vec);
    return check_launch("f32_to_u8_kernel");
}

int cslgan_depth_to_space_f32(const float* x, int N, int H, int W, int C, int inverse, float* y, void* stream) {
    CSLGAN_REQUIRE(x && y, "depth_to_space: null argument");
    CSLGAN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "depth_to_space: needs C %% 4 == 0 (C=%d)", C);
    CSLGAN_REQUIRE(aligned16(inverse ? y : x), "depth_to_space: the [N,H,W,C] tensor must be 16-byte aligned");
    const long long rows = (long long)N * H * W;
    const dim3 g(grid_for(rows * (C / 4))), b(256);
    if (inverse) hipLaunchKernelGGL((depth_to_space_kernel<true>), g, b, 0, (hipStream_t)stream, x, rows, H, W, C, y);
    else hipLaunchKernelGGL((depth_to_space_kernel<false>), g, b, 0, (hipStream_t)stream, x, rows, H, W, C, y);
    return check_launch("depth_to_space_kernel");
}

int cslgan_fold_channels4_f32(const float* in, int64_t rows, int C, int unfold, float* out, void* stream) {
    CSLGAN_REQUIRE(in && out, "fold_channels4: null argument");
    CSLGAN_REQUIRE(rows > 0 && C > 0 && C % 4 == 0, "fold_channels4: needs C %% 4 == 0 (C=%d)", C);
    const dim3 g(grid_for((long long)rows * (C / 4))), b(256);
    if (unfold) hipLaunchKernelGGL((fold_channels4_kernel<true>), g, b, 0, (hipStream_t)stream, in, (long long)rows, C, out);
    else hipLaunchKernelGGL((fold_channels4_kernel<false>), g, b, 0, (hipStream_t)stream, in, (long long)rows, C, out);
    return check_launch("fold_channels4_kernel");
}

}  // extern "C"
