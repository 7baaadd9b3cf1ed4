// One-vs-rest logistic regression for gfx950 (csl_gan_amd.classify).
//
//   downstream.py:71-72, :87  OneVsRestClassifier(LogisticRegression(lbfgs, multinomial)).fit  -> ovr_logreg_eval_kernel + ovr_logreg_reduce_kernel
//                                                                (one loss-and-gradient evaluation of all K <= 16 binary problems)
//   downstream.py:87          .predict_proba(X_test)                                             -> ovr_logreg_proba_kernel
//   (no counterpart)          the same evaluation and probabilities on uint8 cache rows of any size  -> ovr_logreg_u8_fwd_kernel + ovr_logreg_u8_grad_kernel
//                                                                (csl_gan_amd.tstr; second half of this file)   + ovr_logreg_u8_reduce_kernel
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
#include "ovr_rows.h"

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

// ---- the same objective on cache BYTES, any row size (csl_gan_amd.tstr) ------------------------------------------------
// x = byte / 255, 1 <= D <= 65536: a 16-row tile no longer fits in LDS, so an evaluation is two passes over X with the residuals
// R = sigmoid(Z) - T [N, 16] kept in the workspace between them.  Bytes enter the matrix instruction as the exact floats 0 .. 255
// and 1 / 255 is applied once to each sum.
//
//   ovr_logreg_u8_fwd_kernel    Z = X U, loss terms, R, the intercept gradient (or P when PROBA).  A workgroup walks blocks of
//                               LRB_RT x 16 rows.  Wavefront w owns the 64-column groups w, w + 4, ...: lane (l16, lg) loads the
//                               16 bytes [64 g + 16 lg, + 16) of row l16 of each of the LRB_RT row tiles and the 16 matching rows
//                               of U, and issues 16 steps per row tile with ONE B fragment set for all LRB_RT tiles (U is
//                               D x 16 floats, four times a 16-row tile of X: shared over 64 rows it costs what X costs, from
//                               L2).  The k order inside a group is permuted the same way on both operands.  The four partial Z
//                               meet in LDS and are added in a fixed order.
//   ovr_logreg_u8_grad_kernel   G = X^T R.  Workgroup (slab, chunk) owns 256 columns and a chunk of rows; its four wavefronts
//                               take the 4-row steps w, w + 4, ... of the chunk.  Lane (l16, lg) loads the 16 bytes
//                               [d0 + 16 l16, + 16) of row lg of the step — a wave instruction reads four runs of 256 contiguous
//                               bytes, so the transposed operand needs no LDS — and byte j is the A element of output block j,
//                               whose row m = l16 stands for column d0 + 16 m + j.  16 [16, 16] accumulators per wavefront; the
//                               four wavefronts meet in LDS in a fixed order and the workgroup writes ONE partial [256, 16].
//   ovr_logreg_u8_reduce_kernel adds the partials in index order in double, scales by 1 / 255, adds u / 2 and ||u||^2 / 4.
constexpr int LRB_MAX_D = 65536;
constexpr int LRB_RT = 4;                         // row tiles of 16 per forward row block: 64 rows share one read of U
constexpr int LRB_ROWS = 16 * LRB_RT;
constexpr int LRB_FWD_BLOCKS = 1024;              // forward workgroups (4 per CU of an MI355X); also the number of loss partials
constexpr int LRB_SLAB = 256;                     // columns of a gradient workgroup: 16 bytes x 16 lanes
constexpr int LRB_GRAD_WGS = 768;                 // slabs x chunks aimed at: 3 workgroups per CU
constexpr int LRB_MAX_CHUNKS = 64;                // bounds the workspace: chunks x Dp x 16 floats
constexpr int LRB_BATCH = 4;                      // 4-row steps in flight per wavefront of the gradient pass

static inline long long lrb_row_blocks(long long N) { return (N + LRB_ROWS - 1) / LRB_ROWS; }
static inline int lrb_fwd_blocks(long long N) {
    const long long rb = lrb_row_blocks(N);
    return (int)(rb < LRB_FWD_BLOCKS ? rb : LRB_FWD_BLOCKS);
}
static inline int lrb_dp(int D) { return (D + LRB_SLAB - 1) / LRB_SLAB * LRB_SLAB; }
// rows per chunk (a multiple of 16) and the number of chunks: slabs x chunks near LRB_GRAD_WGS, at most LRB_MAX_CHUNKS chunks
static inline void lrb_chunks(long long N, int D, long long& rows_per_chunk, int& chunks) {
    const long long slabs = lrb_dp(D) / LRB_SLAB;
    long long want = (LRB_GRAD_WGS + slabs - 1) / slabs;
    want = want > LRB_MAX_CHUNKS ? LRB_MAX_CHUNKS : want;
    rows_per_chunk = ((N + want - 1) / want + 15) / 16 * 16;
    chunks = (int)((N + rows_per_chunk - 1) / rows_per_chunk);
}

template <bool PROBA, bool AL>
__global__ __launch_bounds__(LR_THREADS) void ovr_logreg_u8_fwd_kernel(const unsigned char* __restrict__ X, const int* __restrict__ labels,
                                                                       const float* __restrict__ U, long long N, int D, int K,
                                                                       float* __restrict__ R, double* __restrict__ lpart, float* __restrict__ P) {
    __shared__ __attribute__((aligned(16))) float zpart[4 * LRB_RT * LR_ROWS * LR_MAX_K];      // 16 KB
    __shared__ double lred[3 * LR_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    const int groups = (D + 63) >> 6;
    const long long row_blocks = (N + LRB_ROWS - 1) / LRB_ROWS;
    const int c = tid & 15, r = tid >> 4;
    const float bias = c < K ? U[(long long)D * K + c] : 0.f;
    const bool cok = l16 < K;
    double lacc = 0.0, bacc = 0.0;                      // thread (row r of every tile, class c) over this workgroup's row blocks

    for (long long rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
        const long long row0 = rb * LRB_ROWS;
        unsigned long long start[LRB_RT];
        bool rok[LRB_RT];
#pragma unroll
        for (int rt = 0; rt < LRB_RT; ++rt) {
            const long long row = row0 + 16 * rt + l16;
            rok[rt] = row < N;
            start[rt] = (unsigned long long)row * (unsigned long long)D;
        }
        f32x4 acc[LRB_RT];
#pragma unroll
        for (int rt = 0; rt < LRB_RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        u32x4 xn[LRB_RT];
        float un[16];
        // group g: columns 64 g + 16 lg + e, e = 0 .. 15, on this lane
        auto fetch = [&](int g) {
            const int col = 64 * g + 16 * lg;
#pragma unroll
            for (int rt = 0; rt < LRB_RT; ++rt) xn[rt] = lrb_load16<AL>(X, total, whole, start[rt], col, D, rok[rt]);
#pragma unroll
            for (int e = 0; e < 16; ++e) {                // unconditional loads (U[0] where there is nothing to read), then a select
                const bool in = cok && col + e < D;
                const float u = U[in ? (long long)(col + e) * K + l16 : 0ll];
                un[e] = in ? u : 0.f;
            }
        };
        fetch(w);
        for (int g = w; g < groups; g += 4) {
            u32x4 xc[LRB_RT];
            float uc[16];
#pragma unroll
            for (int rt = 0; rt < LRB_RT; ++rt) xc[rt] = xn[rt];
#pragma unroll
            for (int e = 0; e < 16; ++e) uc[e] = un[e];
            fetch(g + 4);                                // in flight during the 64 instructions below; zeros past the last group
#pragma unroll
            for (int e = 0; e < 16; ++e) {
#pragma unroll
                for (int rt = 0; rt < LRB_RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(lrb_byte(xc[rt], e), uc[e], acc[rt], 0, 0, 0);
            }
        }
        // C layout: column (class) l16, row 4 lg + i
#pragma unroll
        for (int rt = 0; rt < LRB_RT; ++rt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) zpart[((w * LRB_RT + rt) * LR_ROWS + 4 * lg + i) * LR_MAX_K + l16] = acc[rt][i];
        }
        __syncthreads();
#pragma unroll
        for (int rt = 0; rt < LRB_RT; ++rt) {
            const int o = rt * 256 + tid;
            const float sum = ((zpart[o] + zpart[LRB_RT * 256 + o]) + zpart[2 * LRB_RT * 256 + o]) + zpart[3 * LRB_RT * 256 + o];
            const float z = sum * (1.0f / 255.0f) + bias;
            const long long row = row0 + 16 * rt + r;
            if (PROBA) {
                const float e = expf(-fabsf(z));
                const float sig = c < K ? (z >= 0.f ? 1.f : e) / (1.f + e) : 0.f;
                float tot = sig;                         // butterfly over the 16 lanes of a row: partners hold equal sums at every level
                tot += __shfl_xor(tot, 1, 64);
                tot += __shfl_xor(tot, 2, 64);
                tot += __shfl_xor(tot, 4, 64);
                tot += __shfl_xor(tot, 8, 64);
                if (row < N && c < K) P[row * K + c] = sig / tot;
            } else if (row < N) {
                float ls = 0.f, rd = 0.f;
                if (c < K) {
                    lr_terms(z, labels[row] == c, ls, rd);
                    lacc += (double)ls;
                    bacc += (double)rd;
                }
                R[row * LR_MAX_K + c] = rd;              // columns >= K add nothing to the gradient
            }
        }
        __syncthreads();                                // the next row block overwrites zpart
    }
    if (!PROBA) {
        // the penalty ||u_k||^2 / 4 of rows [b per, (b + 1) per) of U, per = ceil(D / workgroups): D is up to 65536 rows, too long
        // a chain of dependent loads for the one block that ends the reduction
        double pacc = 0.0;
        if (c < K) {
            const int per = (D + (int)gridDim.x - 1) / (int)gridDim.x;
            const int dlo = (int)blockIdx.x * per, dhi = dlo + per < D ? dlo + per : D;
            for (int d = dlo + r; d < dhi; d += 8 * LR_ROWS) {
                float u[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) u[j] = d + LR_ROWS * j < dhi ? U[(long long)(d + LR_ROWS * j) * K + c] : 0.f;      // 8 loads in flight
#pragma unroll
                for (int j = 0; j < 8; ++j) pacc += 0.25 * (double)u[j] * (double)u[j];
            }
        }
        lred[tid] = lacc;
        lred[LR_THREADS + tid] = bacc;
        lred[2 * LR_THREADS + tid] = pacc;
        __syncthreads();
        if (tid < 3 * LR_MAX_K) {                       // threads 0 .. 15: the losses, 16 .. 31: the intercept gradients, 32 .. 47: the penalties
            const int k = tid & 15, which = tid >> 4;
            double s = 0.0;
            for (int i = 0; i < LR_ROWS; ++i) s += lred[which * LR_THREADS + i * LR_MAX_K + k];
            lpart[((long long)blockIdx.x * 3 + which) * LR_MAX_K + k] = s;
        }
    }
}

template <bool AL>
__global__ __launch_bounds__(LR_THREADS) void ovr_logreg_u8_grad_kernel(const unsigned char* __restrict__ X, const float* __restrict__ R, long long N,
                                                                        int D, int Dp, long long rows_per_chunk, float* __restrict__ gpart) {
    __shared__ __attribute__((aligned(16))) float part[3 * 64 * 64];        // wavefronts 1 .. 3: [block j][i][lane], 48 KB
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    const int d0 = blockIdx.x * LRB_SLAB, col = d0 + 16 * l16;
    const long long cs = (long long)blockIdx.y * rows_per_chunk;
    const long long ce = cs + rows_per_chunk < N ? cs + rows_per_chunk : N;
    const int steps = (int)((ce - cs + 3) >> 2);                            // 4-row steps of this chunk; wavefront w takes w, w + 4, ...
    const int batches = (steps + 4 * LRB_BATCH - 1) / (4 * LRB_BATCH);      // the same for the four wavefronts

    f32x4 acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 xn[LRB_BATCH];
    float rn[LRB_BATCH];
    // step t: A[column d0 + 16 l16 + j][row cs + 4 t + lg] for block j, B[row cs + 4 t + lg][class l16]
    auto fetch = [&](int b) {
#pragma unroll
        for (int q = 0; q < LRB_BATCH; ++q) {
            const long long row = cs + 4ll * (w + 4 * (LRB_BATCH * b + q)) + lg;
            const bool ok = row < ce;
            xn[q] = lrb_load16<AL>(X, total, whole, (unsigned long long)row * (unsigned long long)D, col, D, ok);
            const float rv = R[ok ? row * LR_MAX_K + l16 : 0ll];          // unconditional, then a select
            rn[q] = ok ? rv : 0.f;
        }
    };
    fetch(0);
    for (int b = 0; b < batches; ++b) {
        u32x4 xc[LRB_BATCH];
        float rc[LRB_BATCH];
#pragma unroll
        for (int q = 0; q < LRB_BATCH; ++q) { xc[q] = xn[q]; rc[q] = rn[q]; }
        fetch(b + 1);                                    // in flight during the 64 instructions below; zeros past the chunk's end
#pragma unroll
        for (int q = 0; q < LRB_BATCH; ++q) {
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(lrb_byte(xc[q], j), rc[q], acc[j], 0, 0, 0);
        }
    }
    if (w > 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) part[((w - 1) * 64 + 4 * j + i) * 64 + lane] = acc[j][i];
        }
    }
    __syncthreads();
    if (w == 0) {
        // C layout of block j: class l16, row m = 4 lg + i, which stands for column d0 + 16 m + j < Dp
        float* __restrict__ gp = gpart + ((long long)blockIdx.y * Dp + d0) * LR_MAX_K;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = (4 * j + i) * 64 + lane;
                const float v = ((acc[j][i] + part[o]) + part[64 * 64 + o]) + part[2 * 64 * 64 + o];
                gp[(16 * (4 * lg + i) + j) * LR_MAX_K + l16] = v;
            }
        }
    }
}

// Blocks 0 .. ceil(D / 16) - 1: 16 rows d of the gradient each, thread (d, class): the chunk partials in index order (double), times
// 1 / 255, + u / 2.  The last block: 16 slices of the forward partials (data term, intercept gradient, a slice of ||u_k||^2 / 4 each)
// x 16 classes for the intercept gradients and the K losses, the slices added in order.
__global__ __launch_bounds__(LR_THREADS) void ovr_logreg_u8_reduce_kernel(const float* __restrict__ gpart, const double* __restrict__ lpart,
                                                                          const float* __restrict__ U, int chunks, int fwd_blocks, int D, int K,
                                                                          int Dp, float* __restrict__ loss, float* __restrict__ grad) {
    __shared__ double red[2 * LR_THREADS];
    const int tid = threadIdx.x, c = tid & 15, sl = tid >> 4;
    const int dblocks = (D + 15) >> 4;
    if ((int)blockIdx.x < dblocks) {
        const int d = blockIdx.x * 16 + sl;
        if (d < D && c < K) {
            double s = 0.0;
#pragma unroll 4
            for (int ch = 0; ch < chunks; ++ch) s += (double)gpart[((long long)ch * Dp + d) * LR_MAX_K + c];
            grad[(long long)d * K + c] = (float)(s / 255.0 + 0.5 * (double)U[(long long)d * K + c]);
        }
        return;                                          // no barrier in this branch
    }
    double sl_loss = 0.0, sl_b = 0.0;
    if (c < K) {
#pragma unroll 4
        for (int b = sl; b < fwd_blocks; b += 16) {
            sl_loss += lpart[((long long)b * 3) * LR_MAX_K + c] + lpart[((long long)b * 3 + 2) * LR_MAX_K + c];
            sl_b += lpart[((long long)b * 3 + 1) * LR_MAX_K + c];
        }
    }
    red[tid] = sl_loss;
    red[LR_THREADS + tid] = sl_b;
    __syncthreads();
    if (tid < K) {
        double tl = 0.0, tb = 0.0;
        for (int i = 0; i < 16; ++i) {
            tl += red[i * 16 + tid];
            tb += red[LR_THREADS + i * 16 + tid];
        }
        loss[tid] = (float)tl;
        grad[(long long)D * K + tid] = (float)tb;        // the intercept carries no penalty
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

int64_t cslgan_ovr_logreg_u8_ws_floats(int64_t N, int D) {
    if (N < 1 || N >= (1ll << 31) || D < 1 || D > LRB_MAX_D) return 0;
    long long rpc;
    int chunks;
    lrb_chunks(N, D, rpc, chunks);
    // the forward partials as doubles (loss, intercept gradient and a slice of the penalty per workgroup), the residuals, the
    // partial gradients
    return 6 * (int64_t)lrb_fwd_blocks(N) * LR_MAX_K + N * LR_MAX_K + (int64_t)chunks * lrb_dp(D) * LR_MAX_K;
}

int cslgan_ovr_logreg_eval_u8(const void* X, const int32_t* labels, const float* U, int64_t N, int D, int K, float* loss, float* grad, float* ws,
                              int64_t ws_floats, void* stream) {
    CSLGAN_REQUIRE(X && labels && U && loss && grad && ws, "ovr_logreg_eval_u8: null argument");
    CSLGAN_REQUIRE(K >= 2 && K <= LR_MAX_K, "ovr_logreg_eval_u8: K=%d must lie in 2 .. %d", K, LR_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= LRB_MAX_D, "ovr_logreg_eval_u8: D=%d must lie in 1 .. %d", D, LRB_MAX_D);
    CSLGAN_REQUIRE(N >= 1 && N < (1ll << 31), "ovr_logreg_eval_u8: N=%lld out of range", (long long)N);
    const int64_t need = cslgan_ovr_logreg_u8_ws_floats(N, D);
    CSLGAN_REQUIRE(ws_floats >= need, "ovr_logreg_eval_u8: workspace of %lld floats, need %lld", (long long)ws_floats, (long long)need);
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "ovr_logreg_eval_u8: workspace misaligned (8 bytes)");
    CSLGAN_REQUIRE(aligned16(X), "ovr_logreg_eval_u8: X misaligned (16 bytes)");
    const int nb = lrb_fwd_blocks(N), Dp = lrb_dp(D);
    const bool al = D % 16 == 0;
    long long rpc;
    int chunks;
    lrb_chunks(N, D, rpc, chunks);
    double* lpart = reinterpret_cast<double*>(ws);
    float* R = ws + 6 * (int64_t)nb * LR_MAX_K;
    float* gpart = R + N * LR_MAX_K;
    const hipStream_t st = (hipStream_t)stream;
    note_kernel("ovr_logreg_u8_fwd_kernel<eval>");
    const auto fwd = al ? ovr_logreg_u8_fwd_kernel<false, true> : ovr_logreg_u8_fwd_kernel<false, false>;
    hipLaunchKernelGGL(fwd, dim3((unsigned)nb), dim3(LR_THREADS), 0, st, (const unsigned char*)X, labels, U, (long long)N, D, K, R, lpart, (float*)nullptr);
    int rc = check_launch("ovr_logreg_u8_fwd_kernel");
    if (rc != CSLGAN_OK) return rc;
    note_kernel("ovr_logreg_u8_grad_kernel");
    const auto bwd = al ? ovr_logreg_u8_grad_kernel<true> : ovr_logreg_u8_grad_kernel<false>;
    hipLaunchKernelGGL(bwd, dim3((unsigned)(Dp / LRB_SLAB), (unsigned)chunks), dim3(LR_THREADS), 0, st, (const unsigned char*)X, (const float*)R, (long long)N, D, Dp, rpc, gpart);
    rc = check_launch("ovr_logreg_u8_grad_kernel");
    if (rc != CSLGAN_OK) return rc;
    hipLaunchKernelGGL(ovr_logreg_u8_reduce_kernel, dim3((unsigned)((D + 15) / 16 + 1)), dim3(LR_THREADS), 0, st, (const float*)gpart,
                       (const double*)lpart, U, chunks, nb, D, K, Dp, loss, grad);
    return check_launch("ovr_logreg_u8_reduce_kernel");
}

int cslgan_ovr_logreg_proba_u8(const void* Xtest, const float* U, int64_t M, int D, int K, float* P, void* stream) {
    CSLGAN_REQUIRE(Xtest && U && P, "ovr_logreg_proba_u8: null argument");
    CSLGAN_REQUIRE(K >= 2 && K <= LR_MAX_K, "ovr_logreg_proba_u8: K=%d must lie in 2 .. %d", K, LR_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= LRB_MAX_D, "ovr_logreg_proba_u8: D=%d must lie in 1 .. %d", D, LRB_MAX_D);
    CSLGAN_REQUIRE(M >= 1 && M < (1ll << 31), "ovr_logreg_proba_u8: M=%lld out of range", (long long)M);
    CSLGAN_REQUIRE(aligned16(Xtest), "ovr_logreg_proba_u8: Xtest misaligned (16 bytes)");
    note_kernel("ovr_logreg_u8_fwd_kernel<proba>");
    const auto fwd = D % 16 == 0 ? ovr_logreg_u8_fwd_kernel<true, true> : ovr_logreg_u8_fwd_kernel<true, false>;
    hipLaunchKernelGGL(fwd, dim3((unsigned)lrb_fwd_blocks(M)), dim3(LR_THREADS), 0, (hipStream_t)stream, (const unsigned char*)Xtest, (const int*)nullptr, U, (long long)M, D, K, (float*)nullptr,
                       (double*)nullptr, P);
    return check_launch("ovr_logreg_u8_fwd_kernel");
}

}  // extern "C"
