// Linear layers with ONE output unit (the critic's head, DCResNet_models.py:145: 8192 -> 1, no bias): forward and data gradient as
// plain streams.  As an implicit GEMM with N = 1 they ran on a 128x32 MFMA tile that is 31/32 padding (14-29 us per launch for
// 4-13 MB); here a workgroup takes one row: y[n] = act(<x[n,:], w> + b) and gx[n,:] = gy[n] * w (* lrelu'(mask)).  gfx950 only.
// The linear_k1s_* kernels are the same streams on bf16-stored features, with the head's grouped weight gradient.
#include "common.h"
#include "device_prims.h"
#include "igemm.h"

namespace cslgan {

__global__ __launch_bounds__(256) void linear_k1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ res, long long C, int act, float* __restrict__ y) {
    __shared__ float s_red[4];
    const long long n = blockIdx.x;
    const float4* xr = reinterpret_cast<const float4*>(x + n * C);
    const float4* wr = reinterpret_cast<const float4*>(w);
    float acc = 0.f;
    for (long long i = threadIdx.x; i < (C >> 2); i += 256) {
        const float4 a = xr[i], b = wr[i];
        acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
    }
    const float tot = block_sum_256(acc, s_red);
    if (threadIdx.x == 0) {
        float val = tot + (bias ? bias[0] : 0.f) + (res ? res[n] : 0.f);
        val = apply_act(val, act);
        y[n] = val;
    }
}

__global__ __launch_bounds__(256) void linear_k1_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ w, const float* __restrict__ mask,
                                                              long long C4, float* __restrict__ gx) {
    const long long n = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= C4) return;
    const float g = gy[n];
    const float4 b = reinterpret_cast<const float4*>(w)[i];
    float4 o = make_float4(g * b.x, g * b.y, g * b.z, g * b.w);
    if (mask) {
        const float4 m = reinterpret_cast<const float4*>(mask + n * C4 * 4)[i];
        o.x = lrelu_mask(o.x, m.x); o.y = lrelu_mask(o.y, m.y); o.z = lrelu_mask(o.z, m.z); o.w = lrelu_mask(o.w, m.w);
    }
    reinterpret_cast<float4*>(gx + n * C4 * 4)[i] = o;
}

// a linear layer with one output and a long input: H = W = P = Q = R = S = 1, K = 1, C % 4 == 0
bool linear_k1_shape(const cslgan_conv_t* c) {
    return c->K == 1 && c->H == 1 && c->W == 1 && c->R == 1 && c->S == 1 && c->P == 1 && c->Q == 1 && c->stride == 1 && c->pad == 0 &&
           (c->C & 3) == 0 && c->C >= 256 && c->N <= 65535;
}

int launch_linear_k1_fwd(const cslgan_conv_t* c, const float* x, const float* w, const float* bias, const float* residual, int act,
                         float* y, hipStream_t st) {
    note_kernel("linear_k1_fwd_kernel");
    hipLaunchKernelGGL(linear_k1_fwd_kernel, dim3((unsigned)c->N), dim3(256), 0, st, x, w, bias, residual, (long long)c->C, act, y);
    return check_launch("linear_k1_fwd_kernel");
}

int launch_linear_k1_dgrad(const cslgan_conv_t* c, const float* gy, const float* w, const float* mask, float* gx, hipStream_t st) {
    const long long C4 = c->C >> 2;
    note_kernel("linear_k1_dgrad_kernel");
    hipLaunchKernelGGL(linear_k1_dgrad_kernel, dim3((unsigned)((C4 + 255) / 256), (unsigned)c->N), dim3(256), 0, st, gy, w, mask, C4, gx);
    return check_launch("linear_k1_dgrad_kernel");
}

// ---- the critic's head on bf16 features (nn.Linear(C, 1), DCResNet_models.py:145) as streams -------------------------------------
// y[n] = act(<x[n,:], bf16(w)> + b): one workgroup per row (as linear_k1_fwd_kernel, x bfloat16)
__global__ __launch_bounds__(256) void linear_k1s_fwd_kernel(const unsigned short* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             long long C, int act, float* __restrict__ y) {
    __shared__ float s_red[4];
    const long long n = blockIdx.x;
    const uint4* xr = reinterpret_cast<const uint4*>(x + n * C);
    float acc = 0.f;
    for (long long i = threadIdx.x; i < (C >> 3); i += 256) {
        const uint4 a = xr[i];
        const float4 b0 = reinterpret_cast<const float4*>(w)[2 * i], b1 = reinterpret_cast<const float4*>(w)[2 * i + 1];
        acc = fmaf(bf_lo(a.x), bf2f(bf16_rne(b0.x)), acc); acc = fmaf(bf_hi(a.x), bf2f(bf16_rne(b0.y)), acc);
        acc = fmaf(bf_lo(a.y), bf2f(bf16_rne(b0.z)), acc); acc = fmaf(bf_hi(a.y), bf2f(bf16_rne(b0.w)), acc);
        acc = fmaf(bf_lo(a.z), bf2f(bf16_rne(b1.x)), acc); acc = fmaf(bf_hi(a.z), bf2f(bf16_rne(b1.y)), acc);
        acc = fmaf(bf_lo(a.w), bf2f(bf16_rne(b1.z)), acc); acc = fmaf(bf_hi(a.w), bf2f(bf16_rne(b1.w)), acc);
    }
    const float tot = block_sum_256(acc, s_red);
    if (threadIdx.x == 0) {
        float val = tot + (bias ? bias[0] : 0.f);
        val = apply_act(val, act);
        y[n] = val;
    }
}

// gx[n,:] = bf16( gy[n] * bf16(w) (* lrelu'(mask[n,:])) ), 8 channels per lane
__global__ __launch_bounds__(256) void linear_k1s_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ w, const unsigned short* __restrict__ mask,
                                                               long long C8, unsigned short* __restrict__ gx) {
    const long long n = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= C8) return;
    const float g = gy[n];
    const float4 b0 = reinterpret_cast<const float4*>(w)[2 * i], b1 = reinterpret_cast<const float4*>(w)[2 * i + 1];
    float o[8] = {g * bf2f(bf16_rne(b0.x)), g * bf2f(bf16_rne(b0.y)), g * bf2f(bf16_rne(b0.z)), g * bf2f(bf16_rne(b0.w)),
                  g * bf2f(bf16_rne(b1.x)), g * bf2f(bf16_rne(b1.y)), g * bf2f(bf16_rne(b1.z)), g * bf2f(bf16_rne(b1.w))};
    if (mask) {
        const uint4 m = reinterpret_cast<const uint4*>(mask + n * C8 * 8)[i];
        const unsigned md[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o[2 * q] = lrelu_mask(o[2 * q], bf_lo(md[q]));
            o[2 * q + 1] = lrelu_mask(o[2 * q + 1], bf_hi(md[q]));
        }
    }
    reinterpret_cast<uint4*>(gx + n * C8 * 8)[i] = make_uint4(pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]), pack_bf16(o[4], o[5]), pack_bf16(o[6], o[7]));
}

// gw[g,:] = alpha * sum_{n in group g} gy[n] * x[n,:] (fp32), sq[g] += ||gw[g,:]||^2: the head's per-sample / grouped weight gradient
// is a scaled copy (a short weighted sum) of bf16 feature rows
__global__ __launch_bounds__(256) void linear_k1s_wgrad_kernel(const float* __restrict__ gy, const unsigned short* __restrict__ x, long long C8, int group,
                                                               float alpha, float* __restrict__ gw, float* __restrict__ sq, const float* __restrict__ row_scale) {
    __shared__ float s_red[4];
    const long long g = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    if (i < C8) {
        for (int r = 0; r < group; ++r) {
            const long long n = g * group + r;
            const float s = row_scale ? gy[n] * row_scale[n] : gy[n];        // clip-weighted sums: the weight meets the fp32 cotangent
            const uint4 a = reinterpret_cast<const uint4*>(x + n * C8 * 8)[i];
            const unsigned d[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[2 * q] = fmaf(s, bf_lo(d[q]), acc[2 * q]);
                acc[2 * q + 1] = fmaf(s, bf_hi(d[q]), acc[2 * q + 1]);
            }
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { acc[q] *= alpha; ss = fmaf(acc[q], acc[q], ss); }
    if (gw && i < C8) {
        float4* o = reinterpret_cast<float4*>(gw + g * C8 * 8) + 2 * i;
        o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    if (sq) {
        const float tot = block_sum_256(ss, s_red);
        if (threadIdx.x == 0) atomicAdd(sq + g, tot);
    }
}

int launch_linear_k1s_fwd(const cslgan_conv_t* c, const void* x, const float* w, const float* bias, int act, float* y, hipStream_t st) {
    note_kernel("linear_k1s_fwd_kernel");
    hipLaunchKernelGGL(linear_k1s_fwd_kernel, dim3((unsigned)c->N), dim3(256), 0, st, reinterpret_cast<const unsigned short*>(x), w, bias,
                       (long long)c->C, act, y);
    return check_launch("linear_k1s_fwd_kernel");
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

// The head nn.Linear(C, 1) on bf16 features x [N, C] (C % 8 == 0): data gradient gx[n,:] = bf16(gy[n] * bf16(w) (* lrelu'(mask)))
// with fp32 gy [N] and bf16 mask / gx [N, C] ...
int cslgan_linear_k1_dgrad_bf16s(const float* gy, const float* w, const void* mask, int N, int64_t C, void* gx, void* stream) {
    CSLGAN_REQUIRE(gy && w && gx && N > 0 && N <= 65535 && C > 0 && C % 8 == 0, "linear_k1_dgrad_bf16s: bad argument");
    CSLGAN_REQUIRE(aligned16(w) && aligned16(gx) && (!mask || aligned16(mask)), "linear_k1_dgrad_bf16s: misaligned");
    const long long C8 = C / 8;
    note_kernel("linear_k1s_dgrad_kernel");
    hipLaunchKernelGGL(linear_k1s_dgrad_kernel, dim3((unsigned)((C8 + 255) / 256), (unsigned)N), dim3(256), 0, (hipStream_t)stream, gy, w,
                       reinterpret_cast<const unsigned short*>(mask), C8, reinterpret_cast<unsigned short*>(gx));
    return check_launch("linear_k1s_dgrad_kernel");
}

// ... and its grouped weight gradient gw[N/group, C] = alpha * sum_{n in g} gy[n] x[n,:] (fp32; nullable) and / or
// sq[N/group] += ||gw_g||^2.
int cslgan_linear_k1_wgrad_bf16s(const float* gy, const void* x, const float* row_scale, int N, int64_t C, int group, float alpha, float* gw, float* sq,
                                 void* stream) {
    CSLGAN_REQUIRE(gy && x && (gw || sq) && N > 0 && C > 0 && C % 8 == 0 && group >= 1 && N % group == 0 && N / group <= 65535,
                   "linear_k1_wgrad_bf16s: bad argument");
    CSLGAN_REQUIRE(aligned16(x) && (!gw || aligned16(gw)), "linear_k1_wgrad_bf16s: misaligned");
    const long long C8 = C / 8;
    note_kernel("linear_k1s_wgrad_kernel");
    hipLaunchKernelGGL(linear_k1s_wgrad_kernel, dim3((unsigned)((C8 + 255) / 256), (unsigned)(N / group)), dim3(256), 0, (hipStream_t)stream, gy,
                       reinterpret_cast<const unsigned short*>(x), C8, group, alpha, gw, sq, row_scale);
    return check_launch("linear_k1s_wgrad_kernel");
}

}  // extern "C"
