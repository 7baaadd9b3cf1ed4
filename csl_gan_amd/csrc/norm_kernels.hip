// The normalisation family over NHWC data (HBM-bound, 16-byte accesses where alignment allows): GroupNorm / BatchNorm statistics, apply
// (+ReLU, + the depth-to-space output of UpsampleConv), eval-mode and running BatchNorm statistics, the consumers of the conv
// epilogue's partial statistics, and the backward.  gfx950 only.
// Replaces (reference file:line): nn.GroupNorm + F.relu DCResNet_models.py:55-57,63-67,101-102 and their autograd backward.
#include "common.h"
#include "device_prims.h"
#include "gn_apply.h"

namespace cslgan {

// ---- normalisation statistics over NHWC data ------------------------------------------------
// x is [R][C] (R = N*H*W rows).  A statistic s covers `rows_per_stat` consecutive rows and `cpg`
// consecutive channels:  s = (row / rows_per_stat) * n_groups + c / cpg.
//   GroupNorm(G): rows_per_stat = H*W, cpg = C/G, n_groups = G        (per image, per group)
//   BatchNorm   : rows_per_stat = R,   cpg = 1,   n_groups = C        (per channel over the batch)
// ONE pass over x accumulates shifted moments  S1 = sum(x - k_s),  S2 = sum((x - k_s)^2)  with the shift k_s = the
// statistic's first element (x[first row of s][first channel of s]): mean = k + S1/n, var = S2/n - (S1/n)^2.
// x is read once instead of twice, and the cancellation of raw E[x^2] - mean^2 (about (mean/sigma)^2) is replaced by that of
// S2 - S1^2/n about the shift: the rounding error of the variance grows with  1 + ((k_s - mean)/sigma)^2.  k_s is the FIRST pixel of
// the statistic, one sample: among the 64 statistics of a layer some sit 2-3 sigma off (a factor 5-10), and for a zero-padded conv's
// output k_s is the image's corner pixel, the least typical one.  Measured against float64 (tests/test_norm_kernels_gpu.py, 300
// values per channel, sigma 1): mean 8 with k = 2.9 (factor 29) — variance error 6.5e-6, output error 2.4e-5, 39x and 9x a float32
// two-pass; mean 30 with k = 10.8 (factor 178) — 1.2e-4 and 4.4e-4, 108x and 106x a two-pass; both are 0.04-0.16 of what the factor
// allows.  The one-pass form is kept where it pays, the partials route of the training step (launch_norm); the routes with global
// atomics run a second statistics pass about the first pass's mean, which takes the factor back to 1.  With a scratch buffer (the float entries)
// the mean reaches the apply kernels rounded once (k + S1/n, not sum * (1/n)): a group of constant values comes out as beta exactly.
// A tiny finalize kernel turns (S1, S2) into the (sum, centred sum of squares) pair the apply / backward kernels consume.
// Rows are read with 16-byte loads, coalesced along C; partial sums go thread -> LDS (per channel) -> one
// global atomic per channel per block.
constexpr int NS_ROWS_MIN = 64;   // rows per block, lower bound (the launch picks a multiple: ~1024 blocks in all)

// Element access for the normalisation kernels: fp32 tensors, or bfloat16-stored activations (csrc/igemm_bf16s.hip's storage mode;
// statistics and arithmetic are fp32 either way, a bf16 output is rounded to nearest even).
typedef unsigned short bf16_t;
__device__ __forceinline__ float ldf(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ float ldf(const bf16_t* p, long long i) { return bf2f(p[i]); }
__device__ __forceinline__ float4 ld4(const float* p, long long i) { return *reinterpret_cast<const float4*>(p + i); }
__device__ __forceinline__ float4 ld4(const bf16_t* p, long long i) {
    const uint2 v = *reinterpret_cast<const uint2*>(p + i);
    return make_float4(bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
}
__device__ __forceinline__ void st1(float* p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void st1(bf16_t* p, long long i, float v) { p[i] = (bf16_t)rne_bf16(v); }
__device__ __forceinline__ void st4(float* p, long long i, float a, float b, float c, float d) { *reinterpret_cast<float4*>(p + i) = make_float4(a, b, c, d); }
__device__ __forceinline__ void st4(bf16_t* p, long long i, float a, float b, float c, float d) {
    *reinterpret_cast<uint2*>(p + i) = make_uint2(rne_bf16(a) | (rne_bf16(b) << 16), rne_bf16(c) | (rne_bf16(d) << 16));
}

// PART: `final_stats` is the partials array [row group][workgroup of the row group][group][2] (see launch_norm): every workgroup
// leaves its own (S1, S2) pairs there and the apply kernel adds them — no zeroed accumulator, no atomics, no finalize launch.
// (Round 3's attempt to finish the statistics in the LAST workgroup of a row group behind a ticket needed a device-scope fence in
// every workgroup and made this kernel 5x slower; it is gone.)
template <bool VEC, bool PART, typename TX>
__global__ __launch_bounds__(256) void norm_stats_kernel(const TX* __restrict__ x, long long rows_per_stat, int C, int cpg,
                                                         int n_groups, int rows_per_block, float* __restrict__ stats,
                                                         float* __restrict__ final_stats, long long n_stats,
                                                         const float* __restrict__ shift) {
    // shift (nullable): k_s per statistic from a first pass (launch_norm's refined scalar route) instead of the first element
    extern __shared__ float s_acc[];   // [2*C]: S1, S2 per channel
    const int tid = threadIdx.x;
    for (int c = tid; c < 2 * C; c += 256) s_acc[c] = 0.f;
    __syncthreads();
    const long long sr = blockIdx.y;                      // which row-group of statistics
    const long long row_first = sr * rows_per_stat;
    const long long r0 = row_first + (long long)blockIdx.x * rows_per_block;
    long long r1 = r0 + rows_per_block;
    const long long rend = row_first + rows_per_stat;
    if (r1 > rend) r1 = rend;
    if (VEC) {
        const int c4n = C >> 2;
        const int c4 = tid % c4n, rl = tid / c4n, rstep = 256 / c4n;
        float k[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = shift ? shift[sr * n_groups + (4 * c4 + e) / cpg] : ldf(x, row_first * C + ((4 * c4 + e) / cpg) * cpg);
        float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
        long long r = r0 + rl;
        for (; r + 3 * rstep < r1; r += 4 * rstep) {      // four independent 16-byte loads in flight
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = ld4(x, (r + u * rstep) * C + 4 * c4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float d[4] = {v[u].x - k[0], v[u].y - k[1], v[u].z - k[2], v[u].w - k[3]};
#pragma unroll
                for (int e = 0; e < 4; ++e) { a1[e] += d[e]; a2[e] = fmaf(d[e], d[e], a2[e]); }
            }
        }
        for (; r < r1; r += rstep) {
            const float4 v = ld4(x, r * C + 4 * c4);
            const float d[4] = {v.x - k[0], v.y - k[1], v.z - k[2], v.w - k[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) { a1[e] += d[e]; a2[e] = fmaf(d[e], d[e], a2[e]); }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            atomicAdd(&s_acc[2 * (4 * c4 + e)], a1[e]);
            atomicAdd(&s_acc[2 * (4 * c4 + e) + 1], a2[e]);
        }
    } else {
        const long long n = (r1 - r0) * C;
        for (long long i = tid; i < n; i += 256) {
            const int c = (int)(i % C);
            const float d = ldf(x, r0 * C + i) - (shift ? shift[sr * n_groups + c / cpg] : ldf(x, row_first * C + (c / cpg) * cpg));
            atomicAdd(&s_acc[2 * c], d);
            atomicAdd(&s_acc[2 * c + 1], d * d);
        }
    }
    __syncthreads();
    // the channels of a group share the shift: fold them in LDS; then ONE value per (group, moment) leaves the workgroup —
    // PART: written to this workgroup's slot of the partials array (no atomics, no zeroed accumulator: the apply kernel adds the
    // <= 64 slots of a row group in its prologue); otherwise one global atomic into the zeroed statistics
    for (int i = tid; i < 2 * n_groups; i += 256) {
        const int g = i >> 1, which = i & 1;
        float t = 0.f;
        for (int j = 0; j < cpg; ++j) t += s_acc[2 * (g * cpg + j) + which];
        if (PART) final_stats[((sr * gridDim.x + blockIdx.x) * n_groups + g) * 2 + which] = t;
        else atomicAdd(&stats[2 * (sr * n_groups + g) + which], t);
    }
}

// (S1, S2) about the shift k  ->  (sum x, sum (x-mean)^2).  shift (nullable): the table the statistics kernel used.  mean_out (nullable,
// may be the same table): receives mean_s = k + S1/n, rounded once — the apply kernel reads it instead of sum * (1/n).  first_pass:
// that mean is the second pass's shift; zero the accumulators for it and leave.
template <typename TX>
__global__ void norm_stats_finalize_kernel(const TX* __restrict__ x, long long rows_per_stat, int C, int cpg, int n_groups,
                                           long long n_stats, float* __restrict__ stats, const float* shift, float* mean_out,
                                           int first_pass) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_stats) return;
    const long long sr = s / n_groups;
    const int g = (int)(s - sr * n_groups);
    const float k = shift ? shift[s] : ldf(x, sr * rows_per_stat * C + g * cpg);
    const float cnt = (float)rows_per_stat * (float)cpg;
    const float S1 = stats[2 * s], S2 = stats[2 * s + 1];
    const float m1 = S1 / cnt;
    if (mean_out) mean_out[s] = k + m1;
    if (first_pass) {
        stats[2 * s] = 0.f;
        stats[2 * s + 1] = 0.f;
        return;
    }
    float css = S2 - S1 * m1;           // sum (x-mean)^2 = S2 - S1^2/n
    if (css < 0.f) css = 0.f;
    stats[2 * s] = (k + m1) * cnt;      // sum x
    stats[2 * s + 1] = css;
}

// y = act((x - mean_s) * rstd_s * gamma[c] + beta[c])
// D2S: y (and xs, the raw input, when given) are written in the depth-to-space layout [N][2H][2W][C/4].
template <bool VEC, bool D2S, typename TX, typename TY>
__global__ void norm_apply_kernel(const TX* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                  const float* __restrict__ stats, long long total, long long rows_per_stat, int C, int cpg,
                                  int n_groups, float eps, int relu, TY* __restrict__ y, int H, int W, TY* __restrict__ xs,
                                  const float* __restrict__ mean_tab) {
    // mean_tab (nullable): mean_s rounded once (norm_stats_finalize_kernel) instead of sum * (1/n)
    const float inv_cnt = 1.f / ((float)rows_per_stat * (float)cpg);
    const long long per_stat_elems = rows_per_stat * C;
    const long long stride = (long long)gridDim.x * blockDim.x;
    if (VEC) {
        const long long n4 = total >> 2;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            const long long e0 = i << 2;
            const int c = (int)(e0 % C);
            const long long sr = e0 / per_stat_elems;
            const float4 v = ld4(x, e0);
            float in[4] = {v.x, v.y, v.z, v.w}, o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long s = sr * n_groups + (c + e) / cpg;
                const float mean = mean_tab ? mean_tab[s] : stats[2 * s] * inv_cnt;
                const float rstd = rsqrtf(stats[2 * s + 1] * inv_cnt + eps);
                float t = (in[e] - mean) * rstd * gamma[c + e] + beta[c + e];
                o[e] = (relu && t < 0.f) ? 0.f : t;
            }
            if (D2S) {
                const long long r = e0 / C;
                const int Cq = C >> 2, cq = c >> 2;
#pragma unroll
                for (int e = 0; e < 4; ++e) {          // lanes hold consecutive c': each of the four stores is coalesced
                    const long long off = d2s_offset(r, e, H, W, Cq) + cq;
                    st1(y, off, o[e]);
                    if (xs) st1(xs, off, in[e]);
                }
            } else {
                st4(y, e0, o[0], o[1], o[2], o[3]);
            }
        }
    } else {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const int c = (int)(i % C);
            const long long s = (i / per_stat_elems) * n_groups + c / cpg;
            const float mean = mean_tab ? mean_tab[s] : stats[2 * s] * inv_cnt;
            const float rstd = rsqrtf(stats[2 * s + 1] * inv_cnt + eps);
            const float xi = ldf(x, i);
            float t = (xi - mean) * rstd * gamma[c] + beta[c];
            t = (relu && t < 0.f) ? 0.f : t;
            if (D2S) {
                const long long off = d2s_offset(i / C, c & 3, H, W, C >> 2) + (c >> 2);
                st1(y, off, t);
                if (xs) st1(xs, off, xi);
            } else {
                st1(y, i, t);
            }
        }
    }
}

// The vector path of norm_apply_kernel with the index arithmetic taken out of the loop.  grid = (slices, statistic row groups): a
// workgroup walks a slice of ONE row group (an image for GroupNorm), and since 256 % (C/4) == 0 a thread keeps the same four
// channels for the whole walk — mean, rstd, gamma and beta are loop constants and an element costs a load, four fused operations
// and a store.  norm_apply_kernel<true, ...> spent two 64-bit divisions, four 32-bit ones, eight statistic loads and four rsqrt per
// four elements: 206 us for the generator's 128x128x64 bfloat16 tensors (537 MB, 2.6 TB/s) — arithmetic, not memory.
template <bool D2S, typename TX, typename TY>
__global__ __launch_bounds__(256) void norm_apply_rows_kernel(const TX* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ stats, long long rows_per_stat, int C, int cpg, int n_groups,
                                                              float eps, int relu, TY* __restrict__ y, int H, int W, TY* __restrict__ xs,
                                                              const float* __restrict__ part, int n_part, float* __restrict__ stats_out, int chan,
                                                              const float* __restrict__ mean_tab) {
    const int c4n = C >> 2;                           // a power of two (256 % c4n == 0)
    const int lg = __ffs(c4n) - 1;
    const int c = (threadIdx.x & (c4n - 1)) << 2;
    const long long sr = blockIdx.y;
    const float cnt = (float)rows_per_stat * (float)cpg;
    const float inv_cnt = 1.f / cnt;
    const long long base = sr * rows_per_stat * C;
    float mean[4], rstd[4], ga[4], be[4];
    if (part) {
        // Two-launch form (round 4): the statistics kernel left one (S1, S2) pair about the shift k per workgroup and group; add the
        // row group's n_part slots here (2 * n_groups threads, n_part loads each), finish them in LDS, and let the row group's first
        // workgroup publish the final (sum x, centred sum of squares) pairs for whoever reads the statistics later (the backward).
        extern __shared__ float s_st[];               // [2 * n_groups]: (mean, centred sum of squares)
        // chan: the partials come from a conv epilogue (cslgan_conv_t.gn_part) and are combined exactly (gn_apply.h)
        if (chan) gn_combine_chan(part, sr, n_part, n_groups, cnt, s_st, stats_out, blockIdx.x == 0);
        for (int i = threadIdx.x; !chan && i < n_groups; i += 256) {
            float S1 = 0.f, S2 = 0.f;
            for (int b = 0; b < n_part; ++b) {
                const float* q = part + ((sr * n_part + b) * n_groups + i) * 2;
                S1 += q[0];
                S2 += q[1];
            }
            const float k = ldf(x, base + (long long)i * cpg);
            const float m1 = S1 / cnt;
            float css = S2 - S1 * m1;
            css = css < 0.f ? 0.f : css;
            s_st[2 * i] = k + m1;
            s_st[2 * i + 1] = css;
            if (stats_out && blockIdx.x == 0) {
                stats_out[2 * (sr * n_groups + i)] = (k + m1) * cnt;
                stats_out[2 * (sr * n_groups + i) + 1] = css;
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            gn_group_stat(s_st, (c + e) / cpg, inv_cnt, eps, mean[e], rstd[e]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long s = sr * n_groups + (c + e) / cpg;
            mean[e] = mean_tab ? mean_tab[s] : stats[2 * s] * inv_cnt;
            rstd[e] = rsqrtf(stats[2 * s + 1] * inv_cnt + eps);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        ga[e] = gamma[c + e];
        be[e] = beta[c + e];
    }
    const unsigned n4 = (unsigned)((rows_per_stat * C) >> 2);          // launcher: rows_per_stat * C < 2^32
    const bool per_image = rows_per_stat == (long long)H * W;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        const long long e0 = base + ((long long)i << 2);
        const float4 v = ld4(x, e0);
        const float in[4] = {v.x, v.y, v.z, v.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = gn_apply(in[e], mean[e], rstd[e], ga[e], be[e], relu);
        if (D2S) {
            const unsigned rl = i >> lg;              // row within the group
            const int Cq = C >> 2, cq = c >> 2;
            long long off[4];
            if (per_image) {
                const unsigned h = rl / (unsigned)W, w = rl - h * (unsigned)W;
#pragma unroll
                for (int e = 0; e < 4; ++e) off[e] = (((sr * 2 * H + 2 * h + (e >> 1)) * 2 * W + 2 * w + (e & 1)) * Cq) + cq;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) off[e] = d2s_offset(sr * rows_per_stat + rl, e, H, W, Cq) + cq;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {             // lanes hold consecutive c': each of the four stores is coalesced
                st1(y, off[e], o[e]);
                if (xs) st1(xs, off[e], in[e]);
            }
        } else {
            st4(y, e0, o[0], o[1], o[2], o[3]);
        }
    }
}

// eval-mode BatchNorm: the (sum, centred sum of squares) pair norm_apply_kernel consumes, from the running statistics
__global__ void bn_eval_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, int C, float cnt,
                                     float* __restrict__ stats) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    stats[2 * c] = rm[c] * cnt;
    stats[2 * c + 1] = rv[c] * cnt;
}

// ---- normalisation backward (GroupNorm / BatchNorm + optional ReLU) -------------------------------
// With xh = (x-mean_s)*rstd_s, dy' = dy * [y > 0] (ReLU fused; y is the forward output):
//   per (row-group sr, channel c):  A = sum_rows dy',  Bq = sum_rows dy' * xh        -> ab[(sr*C + c)*2 + {0,1}]
//   d gamma[c] = sum_sr Bq,  d beta[c] = sum_sr A
//   per statistic s: s1 = sum_{c in s} gamma_c A, s2 = sum_{c in s} gamma_c Bq
//   dx = rstd_s * (gamma_c dy' - s1/cnt - xh * s2/cnt)
// xh is formed as fma(x, cnt, -sum_s) * (rstd_s / cnt): the statistics carry sum_s, and x - sum_s * (1/cnt) would give xh the absolute
// error of a rounded mean times rstd (up to 316 on a nearly constant group); the fused form rounds x * cnt - sum_s once, relative to itself.
template <bool VEC>
__global__ __launch_bounds__(256) void norm_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ y, const float* __restrict__ stats,
                                                             long long rows_per_stat, int C, int cpg, int n_groups, float eps,
                                                             int relu, int rows_per_block, float* __restrict__ ab) {
    extern __shared__ float s_acc[];   // [2*C]
    const int tid = threadIdx.x;
    for (int c = tid; c < 2 * C; c += 256) s_acc[c] = 0.f;
    __syncthreads();
    const long long sr = blockIdx.y;
    const long long r0 = sr * rows_per_stat + (long long)blockIdx.x * rows_per_block;
    long long r1 = r0 + rows_per_block;
    const long long rend = (sr + 1) * rows_per_stat;
    if (r1 > rend) r1 = rend;
    const float cnt = (float)rows_per_stat * (float)cpg;
    const float inv_cnt = 1.f / cnt;
    if (VEC) {
        const int c4n = C >> 2;
        const int c4 = tid % c4n, rl = tid / c4n, rstep = 256 / c4n;
        float sum[4], rn[4], a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long s = sr * n_groups + (4 * c4 + e) / cpg;
            sum[e] = stats[2 * s];
            rn[e] = rsqrtf(stats[2 * s + 1] * inv_cnt + eps) * inv_cnt;
        }
        for (long long r = r0 + rl; r < r1; r += rstep) {
            const float4 xv = *reinterpret_cast<const float4*>(x + r * C + 4 * c4);
            const float4 gv = *reinterpret_cast<const float4*>(dy + r * C + 4 * c4);
            float4 yv = make_float4(1.f, 1.f, 1.f, 1.f);
            if (relu) yv = *reinterpret_cast<const float4*>(y + r * C + 4 * c4);
            const float xi[4] = {xv.x, xv.y, xv.z, xv.w}, gi[4] = {gv.x, gv.y, gv.z, gv.w}, yi[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = yi[e] > 0.f ? gi[e] : 0.f;
                a[e] += g;
                b[e] = fmaf(g, fmaf(xi[e], cnt, -sum[e]) * rn[e], b[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            atomicAdd(&s_acc[2 * (4 * c4 + e)], a[e]);
            atomicAdd(&s_acc[2 * (4 * c4 + e) + 1], b[e]);
        }
    } else {
        const long long n = (r1 - r0) * C;
        for (long long i = tid; i < n; i += 256) {
            const int c = (int)(i % C);
            const long long s = sr * n_groups + c / cpg;
            const float rn = rsqrtf(stats[2 * s + 1] * inv_cnt + eps) * inv_cnt;
            const long long off = r0 * C + i;
            const float g = (!relu || y[off] > 0.f) ? dy[off] : 0.f;
            atomicAdd(&s_acc[2 * c], g);
            atomicAdd(&s_acc[2 * c + 1], g * (fmaf(x[off], cnt, -stats[2 * s]) * rn));
        }
    }
    __syncthreads();
    for (int c = tid; c < 2 * C; c += 256) atomicAdd(&ab[sr * 2 * C + c], s_acc[c]);
}

// gs[s] = (s1, s2);  dgamma/dbeta accumulate over row groups
__global__ void norm_bwd_finalize_kernel(const float* __restrict__ ab, const float* __restrict__ gamma, long long n_row_groups,
                                         int C, int cpg, int n_groups, float* __restrict__ gs, float* __restrict__ dgamma,
                                         float* __restrict__ dbeta) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n_stats = n_row_groups * n_groups;
    if (i < n_stats) {
        const long long sr = i / n_groups;
        const int g = (int)(i - sr * n_groups);
        float s1 = 0.f, s2 = 0.f;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            s1 = fmaf(gamma[c], ab[(sr * C + c) * 2], s1);
            s2 = fmaf(gamma[c], ab[(sr * C + c) * 2 + 1], s2);
        }
        gs[2 * i] = s1;
        gs[2 * i + 1] = s2;
    }
    if (i < C) {
        float da = 0.f, db = 0.f;
        for (long long sr = 0; sr < n_row_groups; ++sr) {
            da += ab[(sr * C + i) * 2];
            db += ab[(sr * C + i) * 2 + 1];
        }
        dbeta[i] = da;
        dgamma[i] = db;
    }
}

__global__ void norm_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
                                      const float* __restrict__ gamma, const float* __restrict__ stats, const float* __restrict__ gs,
                                      long long total, long long rows_per_stat, int C, int cpg, int n_groups, float eps, int relu,
                                      float* __restrict__ dx) {
    const float cnt = (float)rows_per_stat * (float)cpg;
    const float inv_cnt = 1.f / cnt;
    const long long per_stat_elems = rows_per_stat * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long s = (i / per_stat_elems) * n_groups + c / cpg;
        const float rstd = rsqrtf(stats[2 * s + 1] * inv_cnt + eps);
        const float xh = fmaf(x[i], cnt, -stats[2 * s]) * (rstd * inv_cnt);
        const float g = (!relu || y[i] > 0.f) ? dy[i] : 0.f;
        dx[i] = rstd * (gamma[c] * g - gs[2 * s] * inv_cnt - xh * gs[2 * s + 1] * inv_cnt);
    }
}

// BatchNorm running statistics (torch semantics: running_var uses the unbiased batch variance)
__global__ void bn_running_kernel(const float* __restrict__ stats, int C, float cnt, float momentum, float* __restrict__ rm,
                                  float* __restrict__ rv) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float mean = stats[2 * c] / cnt;
    const float var_unb = cnt > 1.f ? stats[2 * c + 1] / (cnt - 1.f) : 0.f;
    rm[c] = (1.f - momentum) * rm[c] + momentum * mean;
    rv[c] = (1.f - momentum) * rv[c] + momentum * var_unb;
}

// ---- host frame: one normalisation call as its entry describes it, filled once, read by launch_norm and launch_norm_apply -------------
template <typename TX, typename TY>
struct NormCall {
    const TX* x;
    const float *gamma, *beta;
    long long R, rows_per_stat;        // rows in all; rows of one statistic (divides R)
    int C, cpg, n_groups;
    float eps;
    int relu;
    float* stats;                      // [R / rows_per_stat][n_groups][2]
    TY* y;
    int d2s_H, d2s_W;                  // d2s_W > 0: y (and xs, the raw input, when given) in the depth-to-space layout; else both 0
    TY* xs;
    hipStream_t st;
};

// about 1024 workgroups in all, each with at least NS_ROWS_MIN rows: fewer, longer blocks mean fewer global atomics
static long long norm_rows_per_block(long long rows) {
    const long long rpb = (rows / 1024 + NS_ROWS_MIN - 1) / NS_ROWS_MIN * NS_ROWS_MIN;
    return rpb < NS_ROWS_MIN ? NS_ROWS_MIN : (rpb > 4096 ? 4096 : rpb);
}

// The channel half of "the 16-byte kernels are legal": a row is whole float4s and 256 threads hold whole rows of them.
static bool norm_vec_channels(int C) { return (C % 4 == 0) && ((C / 4) <= 256) && (256 % (C / 4) == 0); }

static bool norm_vec_ok(const void* x, const void* y, const void* xs, int C, int cpg) {
    return norm_vec_channels(C) && (cpg % 4 == 0 || 4 % cpg == 0) && aligned16(x) && aligned16(y) && (!xs || aligned16(xs));
}

template <typename TX, typename TY>
static int launch_norm_apply(const NormCall<TX, TY>& c, bool vec, const float* part = nullptr, int n_part = 0, int chan = 0, const float* mean_tab = nullptr) {
    const long long total = c.R * c.C;
    const long long n_rg = c.R / c.rows_per_stat;
    const bool d2s = c.d2s_W > 0;
    if (vec && c.rows_per_stat * c.C < (1ll << 32) && n_rg <= 65535) {
        long long bx = (c.rows_per_stat * c.C / 4 + 255) / 256;
        const long long cap = (4096 + n_rg - 1) / n_rg;                 // about 4096 workgroups in all
        bx = bx > cap ? cap : (bx < 1 ? 1 : bx);
        const size_t lds = part ? sizeof(float) * 2 * c.n_groups : 0;
        const auto k = d2s ? norm_apply_rows_kernel<true, TX, TY> : norm_apply_rows_kernel<false, TX, TY>;
        hipLaunchKernelGGL(k, dim3((unsigned)bx, (unsigned)n_rg), dim3(256), lds, c.st, c.x, c.gamma, c.beta, c.stats, c.rows_per_stat, c.C, c.cpg,
                           c.n_groups, c.eps, c.relu, c.y, c.d2s_H, c.d2s_W, c.xs, part, n_part, c.stats, chan, mean_tab);
        return check_launch("norm_apply_rows_kernel");
    }
    long long nb = (total / 4 + 255) / 256;
    nb = nb > 4096 ? 4096 : (nb < 1 ? 1 : nb);
    const auto k = d2s ? (vec ? norm_apply_kernel<true, true, TX, TY> : norm_apply_kernel<false, true, TX, TY>)
                       : (vec ? norm_apply_kernel<true, false, TX, TY> : norm_apply_kernel<false, false, TX, TY>);
    hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(256), 0, c.st, c.x, c.gamma, c.beta, c.stats, total, c.rows_per_stat, c.C, c.cpg, c.n_groups, c.eps, c.relu, c.y, c.d2s_H, c.d2s_W, c.xs, mean_tab);
    return check_launch("norm_apply_kernel");
}

template <typename TX, typename TY>
static int launch_norm(const NormCall<TX, TY>& c, float* scratch = nullptr) {
    const long long n_row_groups = c.R / c.rows_per_stat;
    const long long n_stats = n_row_groups * c.n_groups;
    const bool vec = norm_vec_ok(c.x, c.y, c.xs, c.C, c.cpg);
    const long long rpb = norm_rows_per_block(c.R);
    const dim3 grid((unsigned)((c.rows_per_stat + rpb - 1) / rpb), (unsigned)n_row_groups), block(256);
    const size_t lds = sizeof(float) * 2 * c.C;
    // Two-launch form (PART, above norm_stats_kernel): per-workgroup partial statistics into `scratch` (2 * n_stats * grid.x floats,
    // grid.x <= CSLGAN_NORM_PARTIAL_BLOCKS), summed by the apply kernel's prologue; round 3 took four launches per normalisation, 36 per D-step.
    if (scratch && vec && grid.x <= CSLGAN_NORM_PARTIAL_BLOCKS && c.rows_per_stat * c.C < (1ll << 32) && n_row_groups <= 65535 && 2 * (size_t)c.n_groups * sizeof(float) <= 32768) {
        hipLaunchKernelGGL((norm_stats_kernel<true, true, TX>), grid, block, lds, c.st, c.x, c.rows_per_stat, c.C, c.cpg, c.n_groups, (int)rpb, c.stats, scratch, n_stats, (const float*)nullptr);
        if (int rc = check_launch("norm_stats_kernel")) return rc;
        return launch_norm_apply(c, vec, scratch, (int)grid.x);
    }
    if (int rc = zero_floats(c.stats, (size_t)2 * n_stats, c.st)) return rc;
    // one pass of the statistics with global atomics about `shift` (nullptr: the statistic's first element); then the finalize kernel
    const auto stats_pass = [&](const float* shift) {
        const auto k = vec ? norm_stats_kernel<true, false, TX> : norm_stats_kernel<false, false, TX>;
        hipLaunchKernelGGL(k, grid, block, lds, c.st, c.x, c.rows_per_stat, c.C, c.cpg, c.n_groups, (int)rpb, c.stats, (float*)nullptr, n_stats, shift);
        return check_launch("norm_stats_kernel");
    };
    const auto finalize = [&](const float* shift, int first_pass) {
        hipLaunchKernelGGL(norm_stats_finalize_kernel<TX>, dim3((unsigned)((n_stats + 127) / 128)), dim3(128), 0, c.st, c.x, c.rows_per_stat, c.C,
                           c.cpg, c.n_groups, n_stats, c.stats, shift, scratch, first_pass);
        return check_launch("norm_stats_finalize_kernel");
    };
    if (int rc = stats_pass(nullptr)) return rc;
    if (scratch) {
        // The routes with global atomics (more than CSLGAN_NORM_PARTIAL_BLOCKS workgroups per statistic, or the scalar kernels; the
        // training step's GroupNorms take neither) buy the variance back with a second pass: the first pass's mean_s (n_stats floats
        // at the head of scratch) becomes the shift, so S2 - S1^2/n no longer cancels by 1 + ((k - mean)/sigma)^2.  One more read
        // of x: a quarter on top of the three passes (statistics, apply's read and write) the route costs anyway.
        if (int rc = finalize(nullptr, 1)) return rc;
        if (int rc = stats_pass(scratch)) return rc;
    }
    if (int rc = finalize(scratch, 0)) return rc;
    return launch_norm_apply(c, vec, nullptr, 0, 0, scratch);
}

// d2s_W > 0 asks for the depth-to-space output layout: rows are (n, h, w) with w fastest, H = rows_per_image / d2s_W
static int check_d2s(long long rows_per_image, int C, int d2s_W, const void* xs, int* H_out) {
    *H_out = 0;
    if (d2s_W <= 0) {
        CSLGAN_REQUIRE(d2s_W == 0 && !xs, "norm: x_shuffled needs d2s_W > 0");
        return CSLGAN_OK;
    }
    CSLGAN_REQUIRE(C % 4 == 0, "norm: depth-to-space output needs C %% 4 == 0 (C=%d)", C);
    CSLGAN_REQUIRE(rows_per_image % d2s_W == 0, "norm: d2s_W=%d does not divide the %lld pixels of an image", d2s_W, rows_per_image);
    *H_out = (int)(rows_per_image / d2s_W);
    return CSLGAN_OK;
}

// The argument checks of the GroupNorm entries under the entry's message prefix `who`; n_part (nullable): of an entry that consumes partials.
static int check_groupnorm(const char* who, bool pointers, int N, int HW, int C, int groups, const int* n_part, int d2s_W, const void* xs, int* H_out) {
    CSLGAN_REQUIRE(pointers, "%s: null argument", who);
    CSLGAN_REQUIRE(N > 0 && HW > 0 && C > 0 && groups > 0 && C % groups == 0, "%s: C=%d not divisible by groups=%d", who, C, groups);
    if (n_part)
        CSLGAN_REQUIRE(N <= 65535 && C <= 8192 && *n_part >= 1 && *n_part <= CSLGAN_NORM_PARTIAL_BLOCKS && HW == 64 * *n_part,
                       "%s: needs HW == 64 * n_part <= %d * 64", who, CSLGAN_NORM_PARTIAL_BLOCKS);
    else
        CSLGAN_REQUIRE(N <= 65535 && C <= 8192, "%s: N or C too large", who);
    return check_d2s(HW, C, d2s_W, xs, H_out);
}

// The same for the BatchNorm entries; running_pair: running_mean and running_var are both given or both absent.
static int check_batchnorm(const char* who, bool pointers, long long rows, int C, bool running_pair, long long rows_per_image, int d2s_W, const void* xs, int* H_out) {
    CSLGAN_REQUIRE(pointers, "%s: null argument", who);
    CSLGAN_REQUIRE(rows > 0 && C > 0 && C <= 8192, "%s: bad sizes", who);
    CSLGAN_REQUIRE(running_pair, "%s: running_mean/var must both be given or both null", who);
    CSLGAN_REQUIRE(d2s_W == 0 || (rows_per_image > 0 && rows % rows_per_image == 0), "%s: rows_per_image must divide rows", who);
    return check_d2s(rows_per_image, C, d2s_W, xs, H_out);
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_groupnorm_act_f32(const float* x, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                             float eps, int relu, float* stats_ws, float* y, int d2s_W, float* x_shuffled, float* scratch, void* stream) {
    int H = 0;
    if (int rc = check_groupnorm("groupnorm", x && gamma && beta && stats_ws && y, N, HW, C, groups, nullptr, d2s_W, x_shuffled, &H)) return rc;
    return launch_norm(NormCall<float, float>{x, gamma, beta, (long long)N * HW, HW, C, C / groups, groups, eps, relu, stats_ws, y, H, d2s_W, x_shuffled, (hipStream_t)stream}, scratch);
}

// (scale, shift) of every (image, channel) from the conv-epilogue partials: one workgroup per image.  The n_part (<= 64) pairs of
// a group are read by 256 / n_groups threads in parallel (a lone thread per channel walking all 64 slots took 23-33 us on the
// generator's last block: latency, not bytes), combined as in the apply kernel's prologue (Chan), in a fixed order.
__global__ __launch_bounds__(256) void gn_affine_parts_kernel(const float* __restrict__ part, int n_part, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int C, int cpg, float cnt, float eps,
                                                              float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ float s_red[256];
    __shared__ float s_mean[256], s_rstd[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int n_groups = C / cpg;                       // <= 256 (host)
    const int ways = 256 / n_groups;                    // threads per group
    const int g = tid % n_groups, k = tid / n_groups;
    const float* base = part + (long long)n * n_part * n_groups * 2;
    const float nb = cnt / (float)n_part;
    float sum = 0.f;
    if (k < ways) for (int b = k; b < n_part; b += ways) sum += base[(b * n_groups + g) * 2];
    s_red[tid] = sum;
    __syncthreads();
    if (tid < n_groups) {
        float t = 0.f;
        for (int j = 0; j < ways; ++j) t += s_red[j * n_groups + tid];
        s_mean[tid] = t / cnt;
    }
    __syncthreads();
    float css = 0.f;
    if (k < ways) {
        const float mean = s_mean[g];
        for (int b = k; b < n_part; b += ways) {
            const float* q = base + (b * n_groups + g) * 2;
            const float dm = q[0] / nb - mean;
            css += q[1] + nb * dm * dm;
        }
    }
    s_red[tid] = css;
    __syncthreads();
    if (tid < n_groups) {
        float t = 0.f;
        for (int j = 0; j < ways; ++j) t += s_red[j * n_groups + tid];
        s_rstd[tid] = rsqrtf(t / cnt + eps);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float a = gamma[c] * s_rstd[c / cpg];
        scale[(long long)n * C + c] = a;
        shift[(long long)n * C + c] = beta[c] - s_mean[c / cpg] * a;
    }
}

int cslgan_groupnorm_affine_parts_f32(const float* part, int n_part, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                                      float eps, float* scale, float* shift, void* stream) {
    CSLGAN_REQUIRE(part && gamma && beta && scale && shift, "groupnorm_affine_parts: null argument");
    CSLGAN_REQUIRE(N > 0 && HW > 0 && C > 0 && groups > 0 && groups <= 256 && C % groups == 0 && n_part >= 1 && HW == 64 * n_part,
                   "groupnorm_affine_parts: needs C %% groups == 0, groups <= 256 and HW == 64 * n_part");
    hipLaunchKernelGGL(gn_affine_parts_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, part, n_part,
                       gamma, beta, C, C / groups, (float)HW * (float)(C / groups), eps, scale, shift);
    return check_launch("gn_affine_parts_kernel");
}

// The apply half on statistics left by a conv epilogue (include/cslgan.h: cslgan_conv_t.gn_part).
int cslgan_groupnorm_apply_parts_f32(const float* x, const float* gamma, const float* beta, int N, int HW, int C, int groups, float eps, int relu,
                                     const float* part, int n_part, float* stats_ws, float* y, int d2s_W, float* x_shuffled, void* stream) {
    int H = 0;
    if (int rc = check_groupnorm("groupnorm_apply_parts", x && gamma && beta && stats_ws && y && part, N, HW, C, groups, &n_part, d2s_W, x_shuffled, &H)) return rc;
    CSLGAN_REQUIRE(norm_vec_ok(x, y, x_shuffled, C, C / groups) && (long long)HW * C < (1ll << 32) && 2 * (size_t)groups * sizeof(float) <= 32768,
                   "groupnorm_apply_parts: shape not taken by the row-walking apply kernel");
    return launch_norm_apply(NormCall<float, float>{x, gamma, beta, (long long)N * HW, HW, C, C / groups, groups, eps, relu, stats_ws, y, H, d2s_W,
                                                    x_shuffled, (hipStream_t)stream}, true, part, n_part, 1);
}

// GroupNorm (+ReLU) at the head of the bf16-stored chain (csrc/igemm_bf16s.hip): x fp32 or bfloat16, y (and x_shuffled) bfloat16;
// statistics and arithmetic in fp32 exactly as cslgan_groupnorm_act_f32.
int cslgan_groupnorm_act_bf16s(const void* x, int x_bf16, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                               float eps, int relu, float* stats_ws, void* y_bf16, int d2s_W, void* x_shuffled_bf16, void* stream) {
    int H = 0;
    if (int rc = check_groupnorm("groupnorm_bf16s", x && gamma && beta && stats_ws && y_bf16, N, HW, C, groups, nullptr, d2s_W, x_shuffled_bf16, &H)) return rc;
    const NormCall<float, bf16_t> c{reinterpret_cast<const float*>(x), gamma, beta, (long long)N * HW, HW, C, C / groups, groups, eps, relu, stats_ws,
                                    reinterpret_cast<bf16_t*>(y_bf16), H, d2s_W, reinterpret_cast<bf16_t*>(x_shuffled_bf16), (hipStream_t)stream};
    if (!x_bf16) return launch_norm(c);
    return launch_norm(NormCall<bf16_t, bf16_t>{reinterpret_cast<const bf16_t*>(x), c.gamma, c.beta, c.R, c.rows_per_stat, c.C, c.cpg, c.n_groups, c.eps,
                                                c.relu, c.stats, c.y, c.d2s_H, c.d2s_W, c.xs, c.st});
}

int cslgan_batchnorm_act_f32(const float* x, const float* gamma, const float* beta, int64_t rows, int C, float eps, int relu,
                             float momentum, float* running_mean, float* running_var, float* stats_ws, float* y,
                             int64_t rows_per_image, int d2s_W, float* x_shuffled, float* scratch, void* stream) {
    int H = 0;
    if (int rc = check_batchnorm("batchnorm", x && gamma && beta && stats_ws && y, rows, C, (running_mean == nullptr) == (running_var == nullptr), rows_per_image, d2s_W, x_shuffled, &H)) return rc;
    if (int rc = launch_norm(NormCall<float, float>{x, gamma, beta, rows, rows, C, 1, C, eps, relu, stats_ws, y, H, d2s_W, x_shuffled, (hipStream_t)stream}, scratch)) return rc;
    if (!running_mean) return CSLGAN_OK;
    hipLaunchKernelGGL(bn_running_kernel, dim3((unsigned)((C + 127) / 128)), dim3(128), 0, (hipStream_t)stream, stats_ws, C, (float)rows, momentum, running_mean, running_var);
    return check_launch("bn_running_kernel");
}

int cslgan_batchnorm_eval_act_f32(const float* x, const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, int64_t rows, int C, float eps, int relu, float* stats_ws, float* y,
                                  int64_t rows_per_image, int d2s_W, float* x_shuffled, void* stream) {
    int H = 0;
    if (int rc = check_batchnorm("batchnorm_eval", x && gamma && beta && running_mean && running_var && stats_ws && y, rows, C, true, rows_per_image, d2s_W, x_shuffled, &H)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((unsigned)((C + 127) / 128)), dim3(128), 0, st, running_mean, running_var, C, (float)rows, stats_ws);
    if (int rc = check_launch("bn_eval_stats_kernel")) return rc;
    return launch_norm_apply(NormCall<float, float>{x, gamma, beta, rows, rows, C, 1, C, eps, relu, stats_ws, y, H, d2s_W, x_shuffled, st}, norm_vec_ok(x, y, x_shuffled, C, 1));
}

int cslgan_norm_act_bwd_f32(const float* x, const float* dy, const float* y, const float* gamma, const float* stats,
                            int64_t rows, int64_t rows_per_stat, int C, int groups, float eps, int relu, float* ws, float* dx,
                            float* dgamma, float* dbeta, void* stream) {
    CSLGAN_REQUIRE(x && dy && gamma && stats && ws && dx && dgamma && dbeta, "norm_bwd: null argument");
    CSLGAN_REQUIRE(!relu || y, "norm_bwd: relu backward needs the forward output");
    CSLGAN_REQUIRE(rows > 0 && rows_per_stat > 0 && rows % rows_per_stat == 0 && C > 0 && groups > 0 && C % groups == 0 && C <= 4096, "norm_bwd: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const long long nrg = rows / rows_per_stat;
    CSLGAN_REQUIRE(nrg <= 65535, "norm_bwd: too many row groups");
    const int cpg = C / groups;
    float* ab = ws;                         // [nrg][C][2]
    float* gs = ws + nrg * C * 2;           // [nrg*groups][2]
    if (int rc = zero_floats(ab, (size_t)nrg * C * 2, st)) return rc;
    const bool vec = norm_vec_channels(C) && aligned16(x) && aligned16(dy) && (!relu || aligned16(y));
    const long long rpb = norm_rows_per_block(rows);
    const dim3 grid((unsigned)((rows_per_stat + rpb - 1) / rpb), (unsigned)nrg), block(256);
    hipLaunchKernelGGL(vec ? norm_bwd_stats_kernel<true> : norm_bwd_stats_kernel<false>, grid, block, sizeof(float) * 2 * C, st, x, dy, y, stats,
                       (long long)rows_per_stat, C, cpg, groups, eps, relu, (int)rpb, ab);
    if (int rc = check_launch("norm_bwd_stats_kernel")) return rc;
    const long long nfin = nrg * groups > C ? nrg * groups : C;
    hipLaunchKernelGGL(norm_bwd_finalize_kernel, dim3((unsigned)((nfin + 127) / 128)), dim3(128), 0, st, ab, gamma, nrg, C, cpg, groups, gs, dgamma, dbeta);
    if (int rc = check_launch("norm_bwd_finalize_kernel")) return rc;
    const long long total = rows * C;
    hipLaunchKernelGGL(norm_bwd_apply_kernel, dim3(grid_for(total)), dim3(256), 0, st, x, dy, y, gamma, stats, gs, total, (long long)rows_per_stat, C, cpg, groups, eps, relu, dx);
    return check_launch("norm_bwd_apply_kernel");
}

int64_t cslgan_norm_bwd_ws_floats(int64_t rows, int64_t rows_per_stat, int C, int groups) {
    const int64_t nrg = rows_per_stat > 0 ? rows / rows_per_stat : 0;
    return nrg * C * 2 + nrg * groups * 2;
}

}  // extern "C"
