// One-vs-rest logistic regression for gfx950 (csl_gan_amd.classify).
//
//   downstream.py:71-72, :87  OneVsRestClassifier(LogisticRegression(lbfgs, multinomial)).fit  -> ovr_logreg_eval_kernel + ovr_logreg_reduce_kernel
//                                                                (one loss-and-gradient evaluation of all K <= 16 binary problems)
//   downstream.py:87          .predict_proba(X_test)                                             -> ovr_logreg_proba_kernel
//
// Objective of class k (include/cslgan.h "Downstream classifier"): sum_i softplus(-s_ik z_ik) + ||u_k||^2 / 4 with z = X u_k + b_k.
// Both products, Z = X U and G = X^T (sigmoid(Z) - T), run on v_mfma_f32_16x16x4_f32 with the classes padded to the 16 columns of
// the instruction: the pass is bound by the read of X, and an optimiser wants the gradient as clean as fp32 gives it.
//
// Tiling of the evaluation.  A workgroup (4 wavefronts) walks row tiles of 16 rows, tile = blockIdx.x, + gridDim.x, ...  A tile is
// loaded from HBM ONCE into registers (one tile ahead of the arithmetic), stored to LDS as [16][Dp + 4] with the constant column
// x[D] = 1 of the intercept and zeros up to Dp = roundup(D + 1, 16), and read from LDS by both products.  The D axis is cut into
// tiles of 16; wavefront w owns D-tiles w, w + 4, ...: it keeps their rows of U as B fragments and their [16, 16] blocks of the
// gradient as accumulators in registers for the whole kernel.  Per row tile: every wavefront multiplies its D-tiles into a partial
// Z, the four partials meet in LDS and are added in a fixed order, 256 threads turn the 16 x 16 logits into loss terms and residuals,
// and every wavefront multiplies the residuals into its accumulators.  A workgroup writes ONE partial gradient and one partial
// loss; ovr_logreg_reduce_kernel adds the partials in index order in double and adds the penalty.  No atomics anywhere: the same
// inputs give the same bits.
#include "common.h"
#include "device_prims.h"

namespace cslgan {

constexpr int LR_THREADS = 256;
constexpr int LR_ROWS = 16;                       // rows of a tile = the M of the first product, the K of the second
constexpr int LR_MAX_K = 16;                      // classes: the N of the instruction
constexpr int LR_WAVE_DT = 14;                    // D-tiles of 16 per wavefront
constexpr int LR_MAX_DP = 4 * 16 * LR_WAVE_DT;    // 896 >= D + 1: tile, partial logits and residuals fit 64 KB of LDS
constexpr int LR_MAX_D = LR_MAX_DP - 1;
constexpr int LR_MAX_BLOCKS = 256;                // one workgroup per CU of an MI355X; also the number of partials
constexpr int LR_PAD = 4;                         // row stride Dp + 4 = 4 or 20 (mod 32) banks: the A reads of the first product hit every bank twice

static inline int lr_dp(int D) { return (D + 1 + 15) & ~15; }
static inline int lr_blocks(long long N) {
    const long long tiles = (N + LR_ROWS - 1) / LR_ROWS;
    return (int)(tiles < LR_MAX_BLOCKS ? tiles : LR_MAX_BLOCKS);
}

// softplus(-s z) and sigmoid(z) from one exponential of -|z|: no overflow for any finite z.
__device__ __forceinline__ void lr_terms(float z, bool positive, float& loss, float& resid) {
    const float e = expf(-fabsf(z));
    const float sz = positive ? z : -z;                          // s z
    loss = (sz < 0.f ? -sz : 0.f) + log1pf(e);                   // max(-s z, 0) + log(1 + exp(-|z|))
    const float sig = (z >= 0.f ? 1.f : e) / (1.f + e);
    resid = sig - (positive ? 1.f : 0.f);
}

// Column quad q (columns 4q .. 4q+3 < Dp) of the 16 rows from row0: X where it exists, 1 in column D, 0 elsewhere.
__device__ __forceinline__ void lr_fetch(const float* __restrict__ X, long long row0, long long N, int D, bool vec, int q, float4 (&pre)[LR_ROWS]) {
    const int c = 4 * q;
    const float o0 = c == D ? 1.f : 0.f, o1 = c + 1 == D ? 1.f : 0.f, o2 = c + 2 == D ? 1.f : 0.f, o3 = c + 3 == D ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < LR_ROWS; ++i) {
        const long long row = row0 + i;
        float4 v = make_float4(o0, o1, o2, o3);
        if (row < N) {
            const float* __restrict__ p = X + row * D + c;
            if (vec) {
                if (c < D) v = *reinterpret_cast<const float4*>(p);          // D % 4 == 0: a quad lies wholly inside or outside a row
            } else {
                if (c < D) v.x = p[0];
                if (c + 1 < D) v.y = p[1];
                if (c + 2 < D) v.z = p[2];
                if (c + 3 < D) v.w = p[3];
            }
        }
        pre[i] = v;
    }
}

__global__ __launch_bounds__(LR_THREADS) void ovr_logreg_eval_kernel(const float* __restrict__ X, const int* __restrict__ labels,
                                                                     const float* __restrict__ U, long long N, int D, int K, int Dp, int vec,
                                                                     float* __restrict__ gpart, double* __restrict__ lpart) {
    __shared__ __attribute__((aligned(16))) float tile[LR_ROWS * (LR_MAX_DP + LR_PAD)];
    __shared__ __attribute__((aligned(16))) float zpart[4 * LR_ROWS * LR_MAX_K];      // after the last tile: the loss terms, as doubles
    __shared__ float rs[LR_ROWS * LR_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4;
    const int ldw = Dp + LR_PAD, Q = Dp >> 2;
    const long long tiles = (N + LR_ROWS - 1) / LR_ROWS;

    // B fragments of the first product: step kk of D-tile j holds U[d0 + 4 kk + lg][l16], zero beyond row D and column K - 1
    float uf[LR_WAVE_DT][4];
    f32x4 acc[LR_WAVE_DT];
#pragma unroll
    for (int j = 0; j < LR_WAVE_DT; ++j) {
        const int d0 = 16 * (4 * j + w);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int d = d0 + 4 * kk + lg;
            uf[j][kk] = (d <= D && l16 < K) ? U[(long long)d * K + l16] : 0.f;
        }
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double lacc = 0.0;                                  // thread (row tid >> 4, class tid & 15) over this workgroup's tiles

    float4 pre[LR_ROWS];
    long long t = blockIdx.x;
    if (tid < Q && t < tiles) lr_fetch(X, t * LR_ROWS, N, D, vec != 0, tid, pre);
    for (; t < tiles; t += gridDim.x) {
        __syncthreads();                                // the second product of the tile before has read the LDS tile
        if (tid < Q) {
#pragma unroll
            for (int i = 0; i < LR_ROWS; ++i) *reinterpret_cast<float4*>(&tile[i * ldw + 4 * tid]) = pre[i];
        }
        __syncthreads();
        const long long tn = t + gridDim.x;
        if (tid < Q && tn < tiles) lr_fetch(X, tn * LR_ROWS, N, D, vec != 0, tid, pre);      // in flight during the arithmetic below

        // Z partial of this wavefront's D-tiles: A[row l16][d0 + 4 kk + lg]; two accumulators hide the dependent latency
        f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < LR_WAVE_DT; ++j) {
            const int d0 = 16 * (4 * j + w);
            if (d0 < Dp) {
                const float* __restrict__ a = &tile[l16 * ldw + d0 + lg];
                z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], uf[j][0], z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4], uf[j][1], z1, 0, 0, 0);
                z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[8], uf[j][2], z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[12], uf[j][3], z1, 0, 0, 0);
            }
        }
        // C layout: column (class) l16, row 4 lg + i
#pragma unroll
        for (int i = 0; i < 4; ++i) zpart[(w * LR_ROWS + 4 * lg + i) * LR_MAX_K + l16] = z0[i] + z1[i];
        __syncthreads();
        {
            const int r = tid >> 4, c = tid & 15;
            const long long row = t * LR_ROWS + r;
            const float z = ((zpart[tid] + zpart[256 + tid]) + zpart[512 + tid]) + zpart[768 + tid];
            float ls = 0.f, rd = 0.f;
            if (row < N && c < K) {
                lr_terms(z, labels[row] == c, ls, rd);
                lacc += (double)ls;
            }
            rs[r * LR_MAX_K + c] = rd;                 // rows >= N and columns >= K add nothing to the gradient
        }
        __syncthreads();
        // G[d][class] += sum_row X[row][d] resid[row][class]: A[d0 + l16][row 4 kk + lg], B[row 4 kk + lg][class l16]
        float rf[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) rf[kk] = rs[(4 * kk + lg) * LR_MAX_K + l16];
#pragma unroll
        for (int j = 0; j < LR_WAVE_DT; ++j) {
            const int d0 = 16 * (4 * j + w);
            if (d0 < Dp) {
                const float* __restrict__ a = &tile[lg * ldw + d0 + l16];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * kk * ldw], rf[kk], acc[j], 0, 0, 0);
            }
        }
    }

    // one partial per workgroup: gpart[block][Dp][16], lpart[block][16]
    float* __restrict__ gp = gpart + (long long)blockIdx.x * Dp * LR_MAX_K;
#pragma unroll
    for (int j = 0; j < LR_WAVE_DT; ++j) {
        const int d0 = 16 * (4 * j + w);
        if (d0 < Dp) {
#pragma unroll
            for (int i = 0; i < 4; ++i) gp[(d0 + 4 * lg + i) * LR_MAX_K + l16] = acc[j][i];
        }
    }
    __syncthreads();
    double* __restrict__ lred = reinterpret_cast<double*>(zpart);          // 256 doubles = 2 KB of the 4 KB
    lred[tid] = lacc;
    __syncthreads();
    if (tid < LR_MAX_K) {
        double s = 0.0;
        for (int r = 0; r < LR_ROWS; ++r) s += lred[r * LR_MAX_K + tid];
        lpart[blockIdx.x * LR_MAX_K + tid] = s;
    }
}

// Block d <= D: grad[d][0..K) = sum over the partials in index order (double) + u / 2 for d < D.  Block D + 1: the K losses, data
// term + ||u_k||^2 / 4.  256 threads = 16 slices of the partials x 16 classes; the slices meet in LDS and are added in order.
__global__ __launch_bounds__(LR_THREADS) void ovr_logreg_reduce_kernel(const float* __restrict__ gpart, const double* __restrict__ lpart,
                                                                       const float* __restrict__ U, int nb, int D, int K, int Dp,
                                                                       float* __restrict__ loss, float* __restrict__ grad) {
    __shared__ double red[LR_THREADS];
    const int tid = threadIdx.x, c = tid & 15, sl = tid >> 4;
    const int d = blockIdx.x;
    double s = 0.0;
    if (d <= D) {
        for (int b = sl; b < nb; b += 16) s += (double)gpart[((long long)b * Dp + d) * LR_MAX_K + c];
    } else if (c < K) {
        for (int b = sl; b < nb; b += 16) s += lpart[b * LR_MAX_K + c];
        for (int i = sl; i < D; i += 16) {
            const double u = (double)U[(long long)i * K + c];
            s += 0.25 * u * u;
        }
    }
    red[tid] = s;
    __syncthreads();
    if (tid < K) {
        double tot = 0.0;
        for (int i = 0; i < 16; ++i) tot += red[i * 16 + tid];
        if (d < D) grad[(long long)d * K + tid] = (float)(tot + 0.5 * (double)U[(long long)d * K + tid]);
        else if (d == D) grad[(long long)d * K + tid] = (float)tot;                  // the intercept carries no penalty
        else loss[tid] = (float)tot;
    }
}

// P[i][k] = sigmoid(z_ik) / sum_k' sigmoid(z_ik'), z = x_i . u_k + b_k.  One wavefront per 16 rows, operands straight from memory
// into fragments (the matrix is read once; U stays in L2): lane (l16, lg) holds X[row l16][d0 + 4 lg + e], e = 0..3, and issues the
// four steps of a D-tile with B = U[d0 + 4 lg + e][l16].  Bytes become floats times 1/255 in the load.
template <bool U8>
__global__ __launch_bounds__(LR_THREADS) void ovr_logreg_proba_kernel(const void* __restrict__ Xv, const float* __restrict__ U, long long M,
                                                                      int D, int K, int vec, float* __restrict__ P) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4;
    const long long row0 = ((long long)blockIdx.x * 4 + w) * LR_ROWS;
    if (row0 >= M) return;                              // no barrier below
    const long long row = row0 + l16;
    const bool rok = row < M;
    const bool cok = l16 < K;
    f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D; d0 += 16) {
        const int c = d0 + 4 * lg;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (rok && c < D) {
            if (U8) {
                const unsigned char* __restrict__ p = reinterpret_cast<const unsigned char*>(Xv) + row * D + c;
                if (vec) {
                    const uchar4 b = *reinterpret_cast<const uchar4*>(p);
                    x[0] = (float)b.x; x[1] = (float)b.y; x[2] = (float)b.z; x[3] = (float)b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = c + e < D ? (float)p[e] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] *= (1.0f / 255.0f);
            } else {
                const float* __restrict__ p = reinterpret_cast<const float*>(Xv) + row * D + c;
                if (vec) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = c + e < D ? p[e] : 0.f;
                }
            }
        }
        float u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = (cok && c + e < D) ? U[(long long)(c + e) * K + l16] : 0.f;
        z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[0], u[0], z0, 0, 0, 0);
        z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[1], u[1], z1, 0, 0, 0);
        z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[2], u[2], z0, 0, 0, 0);
        z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[3], u[3], z1, 0, 0, 0);
    }
    const float bias = cok ? U[(long long)D * K + l16] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                        // C layout: class l16, row 4 lg + i
        const float z = z0[i] + z1[i] + bias;
        const float e = expf(-fabsf(z));
        const float sig = cok ? (z >= 0.f ? 1.f : e) / (1.f + e) : 0.f;
        float tot = sig;                                 // butterfly over the 16 lanes of a row: partners hold equal sums at every level
        tot += __shfl_xor(tot, 1, 64);
        tot += __shfl_xor(tot, 2, 64);
        tot += __shfl_xor(tot, 4, 64);
        tot += __shfl_xor(tot, 8, 64);
        const long long r = row0 + 4 * lg + i;
        if (r < M && cok) P[r * K + l16] = sig / tot;
    }
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int64_t cslgan_ovr_logreg_ws_floats(int64_t N, int D) {
    if (N < 1 || D < 1 || D > LR_MAX_D) return 0;
    const int64_t nb = lr_blocks(N);
    return nb * (int64_t)lr_dp(D) * LR_MAX_K + 2 * nb * LR_MAX_K;      // partial gradients, then the partial losses as doubles
}

int cslgan_ovr_logreg_eval_f32(const float* X, const int32_t* labels, const float* U, int64_t N, int D, int K, float* loss, float* grad,
                               float* ws, int64_t ws_floats, void* stream) {
    CSLGAN_REQUIRE(X && labels && U && loss && grad && ws, "ovr_logreg_eval: null argument");
    CSLGAN_REQUIRE(K >= 2 && K <= LR_MAX_K, "ovr_logreg_eval: K=%d must lie in 2 .. %d", K, LR_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= LR_MAX_D, "ovr_logreg_eval: D=%d must lie in 1 .. %d", D, LR_MAX_D);
    CSLGAN_REQUIRE(N >= 1 && N < (1ll << 31), "ovr_logreg_eval: N=%lld out of range", (long long)N);
    const int64_t need = cslgan_ovr_logreg_ws_floats(N, D);
    CSLGAN_REQUIRE(ws_floats >= need, "ovr_logreg_eval: workspace of %lld floats, need %lld", (long long)ws_floats, (long long)need);
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "ovr_logreg_eval: workspace misaligned (8 bytes)");
    const int nb = lr_blocks(N), Dp = lr_dp(D);
    float* gpart = ws;
    double* lpart = reinterpret_cast<double*>(ws + (int64_t)nb * Dp * LR_MAX_K);          // an even number of floats precedes it
    const int vec = (D % 4 == 0 && aligned16(X)) ? 1 : 0;
    note_kernel("ovr_logreg_eval_kernel");
    hipLaunchKernelGGL(ovr_logreg_eval_kernel, dim3((unsigned)nb), dim3(LR_THREADS), 0, (hipStream_t)stream, X, labels, U, (long long)N, D, K, Dp,
                       vec, gpart, lpart);
    int rc = check_launch("ovr_logreg_eval_kernel");
    if (rc != CSLGAN_OK) return rc;
    hipLaunchKernelGGL(ovr_logreg_reduce_kernel, dim3((unsigned)(D + 2)), dim3(LR_THREADS), 0, (hipStream_t)stream, gpart, lpart, U, nb, D, K, Dp,
                       loss, grad);
    return check_launch("ovr_logreg_reduce_kernel");
}

int cslgan_ovr_logreg_proba_f32(const void* Xtest, int is_u8, const float* U, int64_t M, int D, int K, float* P, void* stream) {
    CSLGAN_REQUIRE(Xtest && U && P, "ovr_logreg_proba: null argument");
    CSLGAN_REQUIRE(is_u8 == 0 || is_u8 == 1, "ovr_logreg_proba: is_u8=%d must be 0 (fp32) or 1 (bytes)", is_u8);
    CSLGAN_REQUIRE(K >= 2 && K <= LR_MAX_K, "ovr_logreg_proba: K=%d must lie in 2 .. %d", K, LR_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= LR_MAX_D, "ovr_logreg_proba: D=%d must lie in 1 .. %d", D, LR_MAX_D);
    CSLGAN_REQUIRE(M >= 1 && M < (1ll << 31), "ovr_logreg_proba: M=%lld out of range", (long long)M);
    const unsigned blocks = (unsigned)((M + 4 * LR_ROWS - 1) / (4 * LR_ROWS));
    if (is_u8) {
        const int vec = (D % 4 == 0 && (reinterpret_cast<uintptr_t>(Xtest) & 3u) == 0) ? 1 : 0;
        note_kernel("ovr_logreg_proba_kernel<u8>");
        hipLaunchKernelGGL(ovr_logreg_proba_kernel<true>, dim3(blocks), dim3(LR_THREADS), 0, (hipStream_t)stream, Xtest, U, (long long)M, D, K, vec, P);
    } else {
        CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(Xtest) & 3u) == 0, "ovr_logreg_proba: fp32 matrix misaligned");
        const int vec = (D % 4 == 0 && aligned16(Xtest)) ? 1 : 0;
        note_kernel("ovr_logreg_proba_kernel<f32>");
        hipLaunchKernelGGL(ovr_logreg_proba_kernel<false>, dim3(blocks), dim3(LR_THREADS), 0, (hipStream_t)stream, Xtest, U, (long long)M, D, K, vec, P);
    }
    return check_launch("ovr_logreg_proba_kernel");
}

}  // extern "C"
