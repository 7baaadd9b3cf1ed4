// Casts and the activation backward.  Streams over bf16-stored tensors (the storage mode of igemm_bf16s.hip): fp32 <-> bfloat16 casts and
// round_bf16 (the fp32 master filter rounded once per parameter version for the bf16-stored convs, cached by the caller); the activation
// backward in its fp32 and its bf16 form.  gfx950 only.  Replaces (reference file:line): F.leaky_relu's backward DCResNet_models.py:132
// (autograd).
#include "common.h"
#include "device_prims.h"
#include "igemm.h"

namespace cslgan {

__global__ void round_bf16_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, long long n) {
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(in)[i];
        reinterpret_cast<uint2*>(out)[i] = make_uint2(pack_bf16(v.x, v.y), pack_bf16(v.z, v.w));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) out[(n4 << 2) + threadIdx.x] = bf16_rne(in[(n4 << 2) + threadIdx.x]);
}

__global__ void widen_bf16_kernel(const unsigned short* __restrict__ in, float* __restrict__ out, long long n) {
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const uint2 v = reinterpret_cast<const uint2*>(in)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) out[(n4 << 2) + threadIdx.x] = bf2f(in[(n4 << 2) + threadIdx.x]);
}

static unsigned stream_blocks(long long n_items) {
    long long nb = (n_items + 255) / 256;
    return (unsigned)(nb > 4096 ? 4096 : (nb < 1 ? 1 : nb));
}

__global__ void act_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y, long long n, float slope,
                               float* __restrict__ out, int vec) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    if (vec) {
        const long long n4 = n >> 2;
        const float4* g4 = reinterpret_cast<const float4*>(g);
        const float4* y4 = reinterpret_cast<const float4*>(y);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            const float4 a = g4[i], b = y4[i];
            o4[i] = make_float4(b.x > 0.f ? a.x : slope * a.x, b.y > 0.f ? a.y : slope * a.y,
                                b.z > 0.f ? a.z : slope * a.z, b.w > 0.f ? a.w : slope * a.w);
        }
        for (long long i = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            out[i] = y[i] > 0.f ? g[i] : slope * g[i];
    } else {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            out[i] = y[i] > 0.f ? g[i] : slope * g[i];
    }
}

// out = g * (y > 0 ? 1 : slope): LeakyReLU / ReLU backward from the OUTPUT's sign, 8 values per lane
__global__ __launch_bounds__(256) void act_bwd_bf16_kernel(const uint4* __restrict__ g, const uint4* __restrict__ y, long long n8, float slope,
                                                           uint4* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        const uint4 gv = g[i], yv = y[i];
        const unsigned gs[4] = {gv.x, gv.y, gv.z, gv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
        unsigned o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float g0 = bf_lo(gs[q]), g1 = bf_hi(gs[q]);
            const float y0 = bf_lo(ys[q]), y1 = bf_hi(ys[q]);
            o[q] = pack_bf16(y0 > 0.f ? g0 : slope * g0, y1 > 0.f ? g1 : slope * g1);
        }
        out[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

int round_bf16(const float* w, void* out, long long n, hipStream_t st) {
    hipLaunchKernelGGL(round_bf16_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, st, w, reinterpret_cast<unsigned short*>(out), n);
    return check_launch("round_bf16_kernel");
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_cast_f32_bf16(const float* in, void* out, int64_t n, void* stream) {
    CSLGAN_REQUIRE(in && out && n >= 0, "cast_f32_bf16: bad argument");
    CSLGAN_REQUIRE(aligned16(in) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0, "cast_f32_bf16: misaligned");
    if (n == 0) return CSLGAN_OK;
    return round_bf16(in, out, n, (hipStream_t)stream);
}

int cslgan_cast_bf16_f32(const void* in, float* out, int64_t n, void* stream) {
    CSLGAN_REQUIRE(in && out && n >= 0, "cast_bf16_f32: bad argument");
    CSLGAN_REQUIRE(aligned16(out) && (reinterpret_cast<uintptr_t>(in) & 7u) == 0, "cast_bf16_f32: misaligned");
    if (n == 0) return CSLGAN_OK;
    hipLaunchKernelGGL(widen_bf16_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned short*>(in), out, (long long)n);
    return check_launch("widen_bf16_kernel");
}

int cslgan_act_bwd_f32(const float* g, const float* y, int64_t n, float slope, float* out, void* stream) {
    CSLGAN_REQUIRE(g && y && out, "act_bwd: null argument");
    CSLGAN_REQUIRE(n >= 0, "act_bwd: n < 0");
    if (n == 0) return CSLGAN_OK;
    const int vec = aligned16(g) && aligned16(y) && aligned16(out);
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)stream, g, y, (long long)n, slope, out, vec);
    return check_launch("act_bwd_kernel");
}

int cslgan_act_bwd_bf16(const void* g, const void* y, int64_t n, float slope, void* out, void* stream) {
    CSLGAN_REQUIRE(g && y && out && n >= 0, "act_bwd_bf16: bad argument");
    CSLGAN_REQUIRE(n % 8 == 0 && aligned16(g) && aligned16(y) && aligned16(out), "act_bwd_bf16: needs a multiple of 8 elements, 16-byte aligned");
    if (n == 0) return CSLGAN_OK;
    hipLaunchKernelGGL(act_bwd_bf16_kernel, dim3(stream_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(g),
                       reinterpret_cast<const uint4*>(y), (long long)(n / 8), slope, reinterpret_cast<uint4*>(out));
    return check_launch("act_bwd_bf16_kernel");
}

}  // extern "C"
