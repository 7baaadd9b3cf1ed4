// One-vs-rest MLP on cache bytes for gfx950 (csl_gan_amd.classify.OvrMlp, csl_gan_amd.tstr --classifier mlp).
//
//   downstream.py:82  OneVsRestClassifier(MLPClassifier(alpha=1)).fit   -> ovr_mlp_fwd_kernel<eval> + ovr_mlp_grad_kernel + ovr_mlp_reduce_kernel
//                                                     (one loss-and-gradient evaluation of all K <= 16 one-hidden-layer networks)
//   downstream.py:87  .predict_proba(X_test)                             -> ovr_mlp_fwd_kernel<proba>
//
// Class k owns H ReLU units; U [P, K], P = (D + 2) H + 1 (include/cslgan.h "One-vs-rest MLP").  With C = H K and c = h K + k the
// first layer of all classes is ONE matrix W1 [D, C], the first D C floats of U, followed by b1 [C], w2 [C] and b2 [K].  Both
// products, Z1 = X W1 and dW1 = X^T dZ1, run on v_mfma_f32_16x16x4_f32 with the bytes as the exact floats 0 .. 255 and 1 / 255
// applied once to each sum.  Every tile is 64 x 64 with a reduction step of 64, staged through LDS from registers that were
// loaded one step ahead; the four wavefronts of a workgroup own a 2 x 2 arrangement of 32 x 32 quadrants (2 x 2 accumulators).
//
//   ovr_mlp_fwd_kernel    A workgroup walks blocks of 64 rows.  Per block it visits the column tiles of C in order: the product over
//                         D, then the tile of A = relu(Z1 / 255 + b1) meets in LDS, thread (row, k mod 4) adds A w2 into its
//                         logits in column order, and A goes to the workspace.  After the last tile the logits give the loss terms
//                         and R = sigmoid(z) - T (or P when PROBA); then thread c walks column c of the block's rows of the
//                         workspace in row order: dw2 += A R, dZ1 = [A > 0] w2 R replaces A, db1 += dZ1.  One partial of the
//                         loss, db2, dw2, db1 and a slice of the penalty per workgroup.
//   ovr_mlp_grad_kernel   Workgroup (d tile, c tile, chunk of rows): dW1 tile = X^T dZ1 over the chunk, one partial per chunk.
//   ovr_mlp_reduce_kernel adds the partials in index order in double, scales by 1 / 255, adds alpha times the weights.
// No atomics and no memset: the same inputs give the same bits.
#include "common.h"
#include "device_prims.h"
#include "ovr_rows.h"

namespace cslgan {

constexpr int ML_THREADS = 256;
constexpr int ML_T = 64;                          // tile edge: rows, columns and the reduction step
constexpr int ML_LDA = ML_T + 4;                  // [row][k] image of the forward X tile: 16-byte rows, A reads at most 2-way on a bank
constexpr int ML_LDB = ML_T + 16;                 // [k][column] images: the B reads (and the transposed A reads) hit 32 banks once
constexpr int ML_MAX_K = 16;
constexpr int ML_MAX_H = 128;
constexpr int ML_MAX_C = ML_MAX_K * ML_MAX_H;     // 2048
constexpr int ML_CPT = ML_MAX_C / ML_THREADS;     // columns per thread in the sweep over dZ1
constexpr int ML_MAX_D = 65536;
constexpr int ML_FWD_BLOCKS = 1024;               // forward workgroups (4 per CU of an MI355X); also the number of forward partials
constexpr int ML_GRAD_WGS = 768;                  // tiles x chunks aimed at: 3 workgroups per CU
constexpr int ML_MAX_CHUNKS = 64;                 // bounds the workspace: chunks x D x C floats

static inline long long ml_row_blocks(long long N) { return (N + ML_T - 1) / ML_T; }
static inline int ml_fwd_blocks(long long N) {
    const long long rb = ml_row_blocks(N);
    return (int)(rb < ML_FWD_BLOCKS ? rb : ML_FWD_BLOCKS);
}
static inline int ml_tiles(int n) { return (n + ML_T - 1) / ML_T; }
// rows per chunk (a multiple of 64) and the number of chunks: tiles x chunks near ML_GRAD_WGS, at most ML_MAX_CHUNKS chunks
static inline void ml_chunks(long long N, int D, int C, long long& rows_per_chunk, int& chunks) {
    const long long tiles = (long long)ml_tiles(D) * ml_tiles(C);
    long long want = (ML_GRAD_WGS + tiles - 1) / tiles;
    want = want > ML_MAX_CHUNKS ? ML_MAX_CHUNKS : want;
    rows_per_chunk = ((N + want - 1) / want + ML_T - 1) / ML_T * ML_T;
    chunks = (int)((N + rows_per_chunk - 1) / rows_per_chunk);
}

// The 16 bytes of a staged row piece as floats into an LDS image, 16-byte aligned
__device__ __forceinline__ void ml_store16(float* __restrict__ dst, const u32x4& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(dst + 4 * q) = make_float4(lrb_byte(v, 4 * q), lrb_byte(v, 4 * q + 1), lrb_byte(v, 4 * q + 2), lrb_byte(v, 4 * q + 3));
}

// 64 x 64 floats from row-major M (row pitch `pitch`), rows r0 .. and columns c0 ..: element (idx >> 6, idx & 63), idx = 256 j + tid,
// zero from row `rows` and column `cols` on.  Unconditional loads (M[0] where there is nothing to read), then a select.
__device__ __forceinline__ void ml_fetch_tile(const float* __restrict__ M, long long r0, long long rows, int c0, int cols, int pitch, int tid,
                                              float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int idx = ML_THREADS * j + tid;
        const long long r = r0 + (idx >> 6);
        const int c = c0 + (idx & 63);
        const bool in = r < rows && c < cols;
        const float x = M[in ? r * pitch + c : 0ll];
        v[j] = in ? x : 0.f;
    }
}
__device__ __forceinline__ void ml_store_tile(float* __restrict__ img, int tid, const float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int idx = ML_THREADS * j + tid;
        img[(idx >> 6) * ML_LDB + (idx & 63)] = v[j];
    }
}

template <bool PROBA, bool AL>
__global__ __launch_bounds__(ML_THREADS) void ovr_mlp_fwd_kernel(const unsigned char* __restrict__ X, const int* __restrict__ labels,
                                                                 const float* __restrict__ U, long long N, int D, int K, int H,
                                                                 float* __restrict__ dZ, double* __restrict__ cpart, double* __restrict__ lpart,
                                                                 float* __restrict__ P) {
    __shared__ __attribute__((aligned(16))) float xs[ML_T * ML_LDA];          // the X tile [row][d]; then the A tile [row][65]
    __shared__ __attribute__((aligned(16))) float wm[ML_T * ML_LDB];          // the W1 tile [d][c]; at the end the loss terms, as doubles
    __shared__ float rs[ML_T * ML_MAX_K];                                     // R (or sigmoid) of the row block
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4;
    const int rw = (w >> 1) * 32, cw = (w & 1) * 32;                         // this wavefront's quadrant of the tile
    const int C = H * K;
    const long long DC = (long long)D * C;
    const float* __restrict__ b1 = U + DC;
    const float* __restrict__ w2 = b1 + C;
    const float* __restrict__ b2 = w2 + C;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    const long long row_blocks = (N + ML_T - 1) / ML_T;
    const int ctiles = (C + ML_T - 1) / ML_T;
    const int zr = tid & 63, kk = tid >> 6;                                   // logits: thread (row zr, classes kk, kk + 4, kk + 8, kk + 12)
    const int xr = tid >> 2, xc = (tid & 3) * 16;                             // staging of X: 16 bytes at column xc of row xr
    double lacc[4] = {0.0, 0.0, 0.0, 0.0}, bacc[4] = {0.0, 0.0, 0.0, 0.0};
    double cwacc[ML_CPT], cbacc[ML_CPT];                                      // dw2 and db1 of columns tid + 256 j
#pragma unroll
    for (int j = 0; j < ML_CPT; ++j) cwacc[j] = cbacc[j] = 0.0;

    for (long long rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
        const long long row0 = rb * ML_T;
        const long long xrow = row0 + xr;
        const bool xok = xrow < N;
        const unsigned long long xstart = (unsigned long long)xrow * (unsigned long long)D;
        float zacc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ct = 0; ct < ctiles; ++ct) {
            const int c0 = ct * ML_T;
            f32x4 acc[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            u32x4 xn = lrb_load16<AL>(X, total, whole, xstart, xc, D, xok);
            float wn[16];
            ml_fetch_tile(U, 0, D, c0, C, C, tid, wn);
            for (int d0 = 0; d0 < D; d0 += ML_T) {
                __syncthreads();                                             // the images are free: everything before has read them
                ml_store16(&xs[xr * ML_LDA + xc], xn);
                ml_store_tile(wm, tid, wn);
                __syncthreads();
                if (d0 + ML_T < D) {                                         // in flight during the 64 instructions below
                    xn = lrb_load16<AL>(X, total, whole, xstart, d0 + ML_T + xc, D, xok);
                    ml_fetch_tile(U, d0 + ML_T, D, c0, C, C, tid, wn);
                }
                // A[row rw + 16 a + l16][d 4 s + lg], B[d 4 s + lg][column cw + 16 b + l16]
#pragma unroll
                for (int s = 0; s < ML_T / 4; ++s) {
                    const int k = 4 * s + lg;
                    const float a0 = xs[(rw + l16) * ML_LDA + k], a1 = xs[(rw + 16 + l16) * ML_LDA + k];
                    const float v0 = wm[k * ML_LDB + cw + l16], v1 = wm[k * ML_LDB + cw + 16 + l16];
                    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, v0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, v1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v1, acc[1][1], 0, 0, 0);
                }
            }
            __syncthreads();                                                 // the X image becomes the A tile [row][65]
            // C layout: column l16, row 4 lg + i
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int col = cw + 16 * b + l16;
                const bool cok = c0 + col < C;
                const float bias = cok ? b1[c0 + col] : 0.f;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float z1 = acc[a][b][i] / 255.0f + bias;
                        xs[(rw + 16 * a + 4 * lg + i) * (ML_T + 1) + col] = (cok && z1 > 0.f) ? z1 : 0.f;
                    }
                }
            }
            __syncthreads();
            const int cend = c0 + ML_T < C ? c0 + ML_T : C;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kk + 4 * j;
                if (k < K) {
                    int c = c0 + (k - c0 % K + K) % K;                       // the first column of the tile that belongs to class k
                    float z = zacc[j];
                    for (; c < cend; c += K) z += xs[zr * (ML_T + 1) + (c - c0)] * w2[c];
                    zacc[j] = z;
                }
            }
            if (!PROBA) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int idx = ML_THREADS * j + tid;
                    const long long row = row0 + (idx >> 6);
                    const int c = c0 + (idx & 63);
                    if (row < N && c < C) dZ[row * C + c] = xs[(idx >> 6) * (ML_T + 1) + (idx & 63)];
                }
            }
        }
        // the logits are complete
        const long long row = row0 + zr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kk + 4 * j;
            if (k < K) {
                const float z = zacc[j] + b2[k];
                float out = 0.f;
                if (PROBA) {
                    const float e = expf(-fabsf(z));
                    out = (z >= 0.f ? 1.f : e) / (1.f + e);
                } else if (row < N) {
                    float ls;
                    lr_terms(z, labels[row] == k, ls, out);
                    lacc[j] += (double)ls;
                    bacc[j] += (double)out;
                }
                rs[zr * ML_MAX_K + k] = out;
            }
        }
        __syncthreads();                                                     // rs is complete, and so are this workgroup's stores of A
        if (PROBA) {
            if (tid < ML_T && row < N) {
                float tot = 0.f;
                for (int k = 0; k < K; ++k) tot += rs[tid * ML_MAX_K + k];
                for (int k = 0; k < K; ++k) P[row * K + k] = rs[tid * ML_MAX_K + k] / tot;
            }
        } else {
            const int rows = (int)(N - row0 < ML_T ? N - row0 : ML_T);
#pragma unroll
            for (int j = 0; j < ML_CPT; ++j) {
                const int c = ML_THREADS * j + tid;
                if (c < C) {
                    const int k = c % K;
                    const float w2c = w2[c];
                    float sw = 0.f, sb = 0.f;
                    float* __restrict__ p = dZ + row0 * C + c;
                    for (int r = 0; r < rows; ++r) {
                        const float a = p[(long long)r * C];
                        const float rr = rs[r * ML_MAX_K + k];
                        const float dz = a > 0.f ? w2c * rr : 0.f;
                        sw += a * rr;
                        sb += dz;
                        p[(long long)r * C] = dz;
                    }
                    cwacc[j] += (double)sw;
                    cbacc[j] += (double)sb;
                }
            }
        }
        __syncthreads();                                                     // the next row block overwrites rs
    }
    if (!PROBA) {
#pragma unroll
        for (int j = 0; j < ML_CPT; ++j) {
            const int c = ML_THREADS * j + tid;
            if (c < C) {
                cpart[((long long)blockIdx.x * 2) * C + c] = cwacc[j];
                cpart[((long long)blockIdx.x * 2 + 1) * C + c] = cbacc[j];
            }
        }
        // sum of squares of rows [b per, (b + 1) per) of W1 as rows of U [D H, K], per = ceil(D H / workgroups)
        const int pc = tid & 15, pr = tid >> 4;
        double pacc = 0.0;
        if (pc < K) {
            const int DH = D * H;
            const int per = (DH + (int)gridDim.x - 1) / (int)gridDim.x;
            const long long lo = (long long)blockIdx.x * per;
            const long long hi = lo + per < DH ? lo + per : DH;
            for (long long e = lo + pr; e < hi; e += 16) {
                const double u = (double)U[e * K + pc];
                pacc += u * u;
            }
        }
        double* __restrict__ lred = reinterpret_cast<double*>(wm);           // [2][16][64] doubles = 16 KB of the 20 KB
        double* __restrict__ pred = reinterpret_cast<double*>(xs);           // [256] doubles
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lred[(kk + 4 * j) * ML_T + zr] = lacc[j];
            lred[(ML_MAX_K + kk + 4 * j) * ML_T + zr] = bacc[j];
        }
        pred[tid] = pacc;
        __syncthreads();
        if (tid < 3 * ML_MAX_K) {                       // threads 0 .. 15: the losses, 16 .. 31: db2, 32 .. 47: the sums of squares
            const int k = tid & 15, which = tid >> 4;
            double s = 0.0;
            if (which < 2) {
                for (int i = 0; i < ML_T; ++i) s += lred[(which * ML_MAX_K + k) * ML_T + i];
            } else {
                for (int i = 0; i < 16; ++i) s += pred[i * 16 + k];
            }
            lpart[((long long)blockIdx.x * 3 + which) * ML_MAX_K + k] = s;
        }
    }
}

template <bool AL>
__global__ __launch_bounds__(ML_THREADS) void ovr_mlp_grad_kernel(const unsigned char* __restrict__ X, const float* __restrict__ dZ, long long N, int D,
                                                                  int C, long long rows_per_chunk, float* __restrict__ gpart) {
    __shared__ __attribute__((aligned(16))) float xs[ML_T * ML_LDB];          // the X tile [row][d]
    __shared__ __attribute__((aligned(16))) float zs[ML_T * ML_LDB];          // the dZ1 tile [row][c]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4;
    const int dw = (w >> 1) * 32, cw = (w & 1) * 32;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    const int d0 = blockIdx.x * ML_T, c0 = blockIdx.y * ML_T;
    const long long cs = (long long)blockIdx.z * rows_per_chunk;
    const long long ce = cs + rows_per_chunk < N ? cs + rows_per_chunk : N;
    const int xr = tid >> 2, xc = (tid & 3) * 16;

    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 xn = lrb_load16<AL>(X, total, whole, (unsigned long long)(cs + xr) * (unsigned long long)D, d0 + xc, D, cs + xr < ce);
    float zn[16];
    ml_fetch_tile(dZ, cs, ce, c0, C, C, tid, zn);
    for (long long n0 = cs; n0 < ce; n0 += ML_T) {
        __syncthreads();
        ml_store16(&xs[xr * ML_LDB + xc], xn);
        ml_store_tile(zs, tid, zn);
        __syncthreads();
        if (n0 + ML_T < ce) {
            const long long row = n0 + ML_T + xr;
            xn = lrb_load16<AL>(X, total, whole, (unsigned long long)row * (unsigned long long)D, d0 + xc, D, row < ce);
            ml_fetch_tile(dZ, n0 + ML_T, ce, c0, C, C, tid, zn);
        }
        // A[d dw + 16 a + l16][row 4 s + lg], B[row 4 s + lg][column cw + 16 b + l16]
#pragma unroll
        for (int s = 0; s < ML_T / 4; ++s) {
            const int k = 4 * s + lg;
            const float a0 = xs[k * ML_LDB + dw + l16], a1 = xs[k * ML_LDB + dw + 16 + l16];
            const float v0 = zs[k * ML_LDB + cw + l16], v1 = zs[k * ML_LDB + cw + 16 + l16];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, v0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, v1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v1, acc[1][1], 0, 0, 0);
        }
    }
    // C layout: column l16, row 4 lg + i
    float* __restrict__ gp = gpart + (long long)blockIdx.z * D * C;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int c = c0 + cw + 16 * b + l16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = d0 + dw + 16 * a + 4 * lg + i;
                if (d < D && c < C) gp[(long long)d * C + c] = acc[a][b][i];
            }
        }
    }
}

// Blocks 0 .. gridDim.x - 2: one entry of the gradient per thread, in the order of U: dW1 (the chunk partials in index order in
// double, times 1 / 255, + alpha W1), db1, dw2 (+ alpha w2), db2 (the forward partials in index order).  The last block: 16 slices
// of the forward partials x 16 classes for the K losses, the slices added in order, + alpha / 2 times the sums of squares.
__global__ __launch_bounds__(ML_THREADS) void ovr_mlp_reduce_kernel(const float* __restrict__ gpart, const double* __restrict__ cpart,
                                                                    const double* __restrict__ lpart, const float* __restrict__ U, int chunks,
                                                                    int fwd_blocks, int D, int K, int H, float alpha, float* __restrict__ loss,
                                                                    float* __restrict__ grad) {
    __shared__ double red[ML_THREADS];
    const int tid = threadIdx.x;
    const int C = H * K;
    const long long DC = (long long)D * C;
    if (blockIdx.x + 1 < gridDim.x) {
        const long long e = (long long)blockIdx.x * ML_THREADS + tid;
        if (e >= DC + 2 * C + K) return;                 // no barrier in this branch
        double s = 0.0;
        if (e < DC) {
#pragma unroll 4
            for (int ch = 0; ch < chunks; ++ch) s += (double)gpart[(long long)ch * DC + e];
            s = s / 255.0 + (double)alpha * (double)U[e];
        } else if (e < DC + C) {
            const int c = (int)(e - DC);
#pragma unroll 4
            for (int b = 0; b < fwd_blocks; ++b) s += cpart[((long long)b * 2 + 1) * C + c];
        } else if (e < DC + 2 * C) {
            const int c = (int)(e - DC - C);
#pragma unroll 4
            for (int b = 0; b < fwd_blocks; ++b) s += cpart[((long long)b * 2) * C + c];
            s += (double)alpha * (double)U[e];
        } else {
            const int k = (int)(e - DC - 2 * C);
#pragma unroll 4
            for (int b = 0; b < fwd_blocks; ++b) s += lpart[((long long)b * 3 + 1) * ML_MAX_K + k];
        }
        grad[e] = (float)s;
        return;
    }
    const int k = tid & 15, sl = tid >> 4;
    double s = 0.0;
    if (k < K) {
#pragma unroll 4
        for (int b = sl; b < fwd_blocks; b += 16)
            s += lpart[((long long)b * 3) * ML_MAX_K + k] + 0.5 * (double)alpha * lpart[((long long)b * 3 + 2) * ML_MAX_K + k];
    }
    red[tid] = s;
    __syncthreads();
    if (tid < K) {
        double tot = 0.0;
        for (int i = 0; i < 16; ++i) tot += red[i * 16 + tid];
        double sq = 0.0;
        for (int h = 0; h < H; ++h) {
            const double v = (double)U[DC + C + (long long)h * K + tid];
            sq += v * v;
        }
        loss[tid] = (float)(tot + 0.5 * (double)alpha * sq);
    }
}

static int ml_check_shape(const char* what, long long N, int D, int K, int H) {
    CSLGAN_REQUIRE(K >= 2 && K <= ML_MAX_K, "%s: K=%d must lie in 2 .. %d", what, K, ML_MAX_K);
    CSLGAN_REQUIRE(H >= 1 && H <= ML_MAX_H, "%s: H=%d must lie in 1 .. %d", what, H, ML_MAX_H);
    CSLGAN_REQUIRE(D >= 1 && D <= ML_MAX_D, "%s: D=%d must lie in 1 .. %d", what, D, ML_MAX_D);
    CSLGAN_REQUIRE(N >= 1 && N < (1ll << 31), "%s: N=%lld out of range", what, N);
    return CSLGAN_OK;
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int64_t cslgan_ovr_mlp_u8_ws_floats(int64_t N, int D, int K, int H) {
    if (N < 1 || N >= (1ll << 31) || D < 1 || D > ML_MAX_D || K < 2 || K > ML_MAX_K || H < 1 || H > ML_MAX_H) return 0;
    const int C = H * K;
    long long rpc;
    int chunks;
    ml_chunks(N, D, C, rpc, chunks);
    // the forward partials as doubles (loss, db2 and a slice of the sums of squares; dw2 and db1), dZ1, the partial gradients
    const int64_t nb = ml_fwd_blocks(N);
    return 2 * nb * (3 * ML_MAX_K + 2 * (int64_t)C) + N * C + (int64_t)chunks * D * C;
}

int cslgan_ovr_mlp_eval_u8(const void* X, const int32_t* labels, const float* U, int64_t N, int D, int K, int H, float alpha, float* loss,
                           float* grad, float* ws, void* stream) {
    CSLGAN_REQUIRE(X && labels && U && loss && grad && ws, "ovr_mlp_eval_u8: null argument");
    const int rc0 = ml_check_shape("ovr_mlp_eval_u8", (long long)N, D, K, H);
    if (rc0 != CSLGAN_OK) return rc0;
    CSLGAN_REQUIRE(alpha >= 0.f && alpha <= 3.0e38f, "ovr_mlp_eval_u8: alpha=%g must be a finite number >= 0", (double)alpha);
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "ovr_mlp_eval_u8: workspace misaligned (8 bytes)");
    CSLGAN_REQUIRE(aligned16(X), "ovr_mlp_eval_u8: X misaligned (16 bytes)");
    const int C = H * K, nb = ml_fwd_blocks(N);
    const bool al = D % 16 == 0;
    long long rpc;
    int chunks;
    ml_chunks(N, D, C, rpc, chunks);
    double* lpart = reinterpret_cast<double*>(ws);
    double* cpart = lpart + (int64_t)nb * 3 * ML_MAX_K;
    float* dZ = ws + 2 * (int64_t)nb * (3 * ML_MAX_K + 2 * (int64_t)C);
    float* gpart = dZ + N * C;
    const hipStream_t st = (hipStream_t)stream;
    note_kernel("ovr_mlp_fwd_kernel<eval>");
    const auto fwd = al ? ovr_mlp_fwd_kernel<false, true> : ovr_mlp_fwd_kernel<false, false>;
    hipLaunchKernelGGL(fwd, dim3((unsigned)nb), dim3(ML_THREADS), 0, st, (const unsigned char*)X, labels, U, (long long)N, D, K, H, dZ, cpart, lpart,
                       (float*)nullptr);
    int rc = check_launch("ovr_mlp_fwd_kernel");
    if (rc != CSLGAN_OK) return rc;
    note_kernel("ovr_mlp_grad_kernel");
    const auto bwd = al ? ovr_mlp_grad_kernel<true> : ovr_mlp_grad_kernel<false>;
    hipLaunchKernelGGL(bwd, dim3((unsigned)ml_tiles(D), (unsigned)ml_tiles(C), (unsigned)chunks), dim3(ML_THREADS), 0, st, (const unsigned char*)X,
                       (const float*)dZ, (long long)N, D, C, rpc, gpart);
    rc = check_launch("ovr_mlp_grad_kernel");
    if (rc != CSLGAN_OK) return rc;
    const long long entries = (long long)D * C + 2 * C + K;
    note_kernel("ovr_mlp_reduce_kernel");
    hipLaunchKernelGGL(ovr_mlp_reduce_kernel, dim3((unsigned)((entries + ML_THREADS - 1) / ML_THREADS + 1)), dim3(ML_THREADS), 0, st,
                       (const float*)gpart, (const double*)cpart, (const double*)lpart, U, chunks, nb, D, K, H, alpha, loss, grad);
    return check_launch("ovr_mlp_reduce_kernel");
}

int cslgan_ovr_mlp_proba_u8(const void* Xtest, const float* U, int64_t M, int D, int K, int H, float* P, void* stream) {
    CSLGAN_REQUIRE(Xtest && U && P, "ovr_mlp_proba_u8: null argument");
    const int rc0 = ml_check_shape("ovr_mlp_proba_u8", (long long)M, D, K, H);
    if (rc0 != CSLGAN_OK) return rc0;
    CSLGAN_REQUIRE(aligned16(Xtest), "ovr_mlp_proba_u8: Xtest misaligned (16 bytes)");
    note_kernel("ovr_mlp_fwd_kernel<proba>");
    const auto fwd = D % 16 == 0 ? ovr_mlp_fwd_kernel<true, true> : ovr_mlp_fwd_kernel<true, false>;
    hipLaunchKernelGGL(fwd, dim3((unsigned)ml_fwd_blocks(M)), dim3(ML_THREADS), 0, (hipStream_t)stream, (const unsigned char*)Xtest, (const int*)nullptr, U,
                       (long long)M, D, K, H, (float*)nullptr, (double*)nullptr, (double*)nullptr, P);
    return check_launch("ovr_mlp_fwd_kernel");
}

}  // extern "C"
