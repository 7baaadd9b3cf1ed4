// Linear support-vector kernels for gfx950 (csl_gan_amd.svm; DESIGN.md §6p, include/cslgan.h "linear SVC").
//
// gram_d2_u8_kernel stores what the nearest-neighbour kernels throw away: the exact uint32 squared distance of every pair of cache
// rows, out of nn_tile_loop (nn_tile.h) with a storing epilogue.  svc_smo_f64_kernel solves up to 96 dual problems over that one
// matrix, a workgroup per problem, LIBSVM's SMO with second-order working-set selection in float64.  Every floating-point operation
// of the solver is elementwise or an exact (value, index) minimum with ties to the lowest index, written in the order of
// csl_gan_amd.svm.smo_host, so the two agree bit for bit: nothing in this file may be contracted into a fused multiply-add.
#include <math.h>

#include "nn_tile.h"

#pragma clang fp contract(off)

namespace cslgan {

constexpr long long SVM_MAX_ROWS = 65536;                      // a 16 GiB matrix
constexpr int SVM_MAX_PROBLEMS = 96;                           // 16 classes x (1 + 5 folds)
constexpr int SMO_THREADS = 1024;                              // 16 waves: a row of the matrix is one or a few loads per thread
constexpr int SMO_WAVES = SMO_THREADS / WAVE;
constexpr int SMO_LDS_ROWS = 3072;                             // alpha and the gradient of so many rows stay in LDS: 48 KiB + 6 KiB
constexpr int SMO_NONE = 0x7fffffff;                           // index of "no candidate"
constexpr double SMO_TAU = 1e-12;                              // replaces a curvature that is not positive
constexpr double SMO_SCALE = 65025.0;                          // K = <b_i, b_j> / 255^2

// ---- the stored matrix -------------------------------------------------------------------------------------------------------------
// out[row, col] = d2(row, col) for col < pitch: per accumulator register the 32 lanes of a row half hold 32 consecutive columns of one
// row, one 128-byte store.  pitch is a multiple of 32, so a 32-column group lies inside the row or outside it as a whole; the columns
// n .. pitch - 1 receive the distance to a row of zeros, which nobody reads.
__global__ __launch_bounds__(NN_THREADS) void gram_d2_u8_kernel(const signed char* __restrict__ xs, const int* __restrict__ sq, int n, int Dp,
                                                                int tiles_per, int n_col_tiles, uint32_t* __restrict__ out, long long pitch) {
    const NNLane ln(threadIdx.x);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    nn_tile_loop(xs, sq, n, xs, sq, n, Dp, tiles_per, n_col_tiles, NNNoColumn(), [&](int mt, int i, bool, long long col, uint32_t d2) {
        const long long row = row0 + ln.row(mt, i);
        if (row < n && col < pitch) out[row * pitch + col] = d2;
    });
}

// ---- the solver ----------------------------------------------------------------------------------------------------------------------
// (value, index) minimum, ties to the lowest index; `none` is (+inf, SMO_NONE).
struct SmoBest {
    double v;
    int idx;
};

__device__ __forceinline__ SmoBest smo_better(SmoBest a, SmoBest b) { return (b.v < a.v || (b.v == a.v && b.idx < a.idx)) ? b : a; }

__device__ __forceinline__ SmoBest smo_shfl_xor(SmoBest a, int o) {
    SmoBest b;
    b.v = __shfl_xor(a.v, o, 64);
    b.idx = __shfl_xor(a.idx, o, 64);
    return b;
}

// Over the workgroup: every thread returns the same record.  A wave reduces by lane shuffles, the 16 leaders leave their records in
// `slot`, and behind ONE barrier every wave reduces those 16 again.  `low` carries a plain minimum along (the solver's M(alpha)).
// The caller alternates between two slots, so a slot is rewritten only two barriers after its last read.
struct SmoSlot {
    double v[SMO_WAVES], low[SMO_WAVES];
    int idx[SMO_WAVES];
};

__device__ __forceinline__ SmoBest smo_block_min(SmoBest b, double& low, SmoSlot& slot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        b = smo_better(b, smo_shfl_xor(b, o));
        low = fmin(low, __shfl_xor(low, o, 64));
    }
    if (lane == 0) {
        slot.v[w] = b.v;
        slot.idx[w] = b.idx;
        slot.low[w] = low;
    }
    __syncthreads();
    b.v = slot.v[lane & (SMO_WAVES - 1)];
    b.idx = slot.idx[lane & (SMO_WAVES - 1)];
    low = slot.low[lane & (SMO_WAVES - 1)];
#pragma unroll
    for (int o = SMO_WAVES / 2; o > 0; o >>= 1) {
        b = smo_better(b, smo_shfl_xor(b, o));
        low = fmin(low, __shfl_xor(low, o, 64));
    }
    return b;
}

// K_it of the byte rows i and t from their squared norms and their squared distance: an exact integer, one conversion, one division.
__device__ __forceinline__ double smo_kernel_value(long long si, long long st, uint32_t d2) {
    return (double)((si + st - (long long)d2) >> 1) / SMO_SCALE;
}

// One workgroup per problem p: labels y[p] (+1 / -1), mask active[p] (a row outside it is never selected; its gradient entry is kept
// like every other), state alpha[p], grad[p], iters[p], done[p] in global memory between launches.  A launch runs at most `chunk`
// iterations and stops at max_iter in total.  Thread t owns the rows t, t + 1024, ...: it alone reads and writes their alpha and
// gradient entries outside the two-variable update, whose four inputs every thread reads between the barriers B and C.
// IN_LDS (n <= SMO_LDS_ROWS): alpha, the gradient, y and the mask are copied into LDS for the launch and written back at its end.
template <bool IN_LDS>
__global__ __launch_bounds__(SMO_THREADS) void svc_smo_f64_kernel(const uint32_t* __restrict__ d2, long long pitch, const long long* __restrict__ s,
                                                                  int n, const signed char* __restrict__ y_all,
                                                                  const unsigned char* __restrict__ active_all, double C, double tol,
                                                                  long long chunk, long long max_iter, double* alpha_all,
                                                                  double* grad_all, long long* __restrict__ iters,
                                                                  int* __restrict__ done) {
    __shared__ double sG[IN_LDS ? SMO_LDS_ROWS : 1], sA[IN_LDS ? SMO_LDS_ROWS : 1];
    __shared__ signed char sY[IN_LDS ? SMO_LDS_ROWS : 1];
    __shared__ unsigned char sM[IN_LDS ? SMO_LDS_ROWS : 1];
    __shared__ SmoSlot slot[2];

    const int p = blockIdx.x, tid = threadIdx.x;
    if (done[p] != 0) return;                                  // uniform: the flag is written by thread 0 at the END of a launch only
    const long long base = (long long)p * n;
    double* gG = grad_all + base;
    double* gA = alpha_all + base;
    const signed char* gY = y_all + base;
    const unsigned char* gM = active_all + base;
    double* G = IN_LDS ? sG : gG;
    double* A = IN_LDS ? sA : gA;
    const signed char* Y = IN_LDS ? sY : gY;
    const unsigned char* M = IN_LDS ? sM : gM;
    if (IN_LDS) {
        for (int t = tid; t < n; t += SMO_THREADS) {
            sG[t] = gG[t];
            sA[t] = gA[t];
            sY[t] = gY[t];
            sM[t] = gM[t];
        }
    }
    __syncthreads();

    long long it = iters[p];
    long long budget = max_iter - it;
    budget = budget < chunk ? budget : chunk;
    int finished = 0;
    const double inf = (double)INFINITY;
    for (long long step = 0; step < budget; ++step) {
        // i: the largest -y G over I_up, as the smallest y G
        SmoBest bi = {inf, SMO_NONE};
        double unused = inf;
        for (int t = tid; t < n; t += SMO_THREADS) {
            const double a = A[t];
            const bool pos = Y[t] > 0;
            if (M[t] != 0 && (pos ? a < C : a > 0.0)) {
                const double g = G[t];
                bi = smo_better(bi, SmoBest{pos ? g : -g, t});
            }
        }
        bi = smo_block_min(bi, unused, slot[0]);               // barrier A
        if (bi.idx == SMO_NONE) {                              // I_up is empty
            finished = 1;
            break;
        }
        const int i = bi.idx;
        const double gmax = -bi.v;
        const long long si = s[i];
        const double kii = (double)si / SMO_SCALE;
        const uint32_t* row_i = d2 + (long long)i * pitch;

        // j: the smallest -b^2 / a over the rows of I_low with b = gmax + y G > 0; gmin: the smallest -y G over I_low
        SmoBest bj = {inf, SMO_NONE};
        double gmin = inf;
        for (int t = tid; t < n; t += SMO_THREADS) {
            const double a = A[t];
            const bool pos = Y[t] > 0;
            if (M[t] != 0 && (pos ? a > 0.0 : a < C)) {
                const double g = G[t];
                const double val = pos ? -g : g;
                gmin = fmin(gmin, val);
                const double b = gmax - val;
                if (b > 0.0) {
                    const long long st = s[t];
                    double quad = (kii + (double)st / SMO_SCALE) - 2.0 * smo_kernel_value(si, st, row_i[t]);
                    if (!(quad > 0.0)) quad = SMO_TAU;
                    bj = smo_better(bj, SmoBest{-(b * b) / quad, t});
                }
            }
        }
        bj = smo_block_min(bj, gmin, slot[1]);                 // barrier B
        if (bj.idx == SMO_NONE || gmax - gmin < tol) {
            finished = 1;
            break;
        }
        const int j = bj.idx;

        // the two-variable update with LIBSVM's clipping, by every thread on the same four values
        const long long sj = s[j];
        const uint32_t* row_j = d2 + (long long)j * pitch;
        const int yi = Y[i], yj = Y[j];
        const double gi = G[i], gj = G[j], ai_old = A[i], aj_old = A[j];
        double quad = (kii + (double)sj / SMO_SCALE) - 2.0 * smo_kernel_value(si, sj, row_i[j]);
        if (!(quad > 0.0)) quad = SMO_TAU;
        double ai = ai_old, aj = aj_old;
        if (yi != yj) {
            const double delta = (-gi - gj) / quad;
            const double diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) {
                if (aj < 0.0) { aj = 0.0; ai = diff; }
            } else {
                if (ai < 0.0) { ai = 0.0; aj = -diff; }
            }
            if (diff > 0.0) {
                if (ai > C) { ai = C; aj = C - diff; }
            } else {
                if (aj > C) { aj = C; ai = C + diff; }
            }
        } else {
            const double delta = (gi - gj) / quad;
            const double sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > C) {
                if (ai > C) { ai = C; aj = sum - C; }
            } else {
                if (aj < 0.0) { aj = 0.0; ai = sum; }
            }
            if (sum > C) {
                if (aj > C) { aj = C; ai = sum - C; }
            } else {
                if (ai < 0.0) { ai = 0.0; aj = sum; }
            }
        }
        const double dai = ai - ai_old, daj = aj - aj_old;
        __syncthreads();                                       // barrier C: everyone holds the four values; their owners may write

        // G += (Q_i * dai) + (Q_j * daj), Q_it = y_i y_t K_it, over ALL rows
        for (int t = tid; t < n; t += SMO_THREADS) {
            const long long st = s[t];
            const int yt = Y[t];
            const double kit = smo_kernel_value(si, st, row_i[t]), kjt = smo_kernel_value(sj, st, row_j[t]);
            const double qit = yi == yt ? kit : -kit, qjt = yj == yt ? kjt : -kjt;
            G[t] = G[t] + ((qit * dai) + (qjt * daj));
            if (t == i) A[t] = ai;
            if (t == j) A[t] = aj;
        }
        ++it;
    }

    __syncthreads();
    if (IN_LDS) {
        for (int t = tid; t < n; t += SMO_THREADS) {
            gG[t] = sG[t];
            gA[t] = sA[t];
        }
    }
    if (tid == 0) {
        iters[p] = it;
        done[p] = finished;
    }
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_gram_d2_u8(const void* xs, const int32_t* sqnorm, int64_t n, int Dp, uint32_t* out, int64_t pitch, void* stream) {
    CSLGAN_REQUIRE(xs && sqnorm && out, "gram_d2_u8: null argument");
    CSLGAN_REQUIRE(n >= 1 && n <= SVM_MAX_ROWS,
                   "gram_d2_u8: n=%lld rows; the stored matrix takes 1 .. %lld (16 GiB), a larger set needs a kernel-row cache", (long long)n,
                   SVM_MAX_ROWS);
    CSLGAN_REQUIRE(Dp >= NN_KT && Dp <= NN_MAX_D && Dp % NN_KT == 0, "gram_d2_u8: Dp=%d must be a multiple of %d in %d .. %d", Dp, NN_KT, NN_KT,
                   NN_MAX_D);
    CSLGAN_REQUIRE(pitch >= n && pitch % 32 == 0 && pitch <= SVM_MAX_ROWS, "gram_d2_u8: pitch=%lld must be a multiple of 32 in n .. %lld",
                   (long long)pitch, SVM_MAX_ROWS);
    CSLGAN_REQUIRE(aligned16(xs) && aligned_to(sqnorm, 4) && aligned_to(out, 128), "gram_d2_u8: misaligned pointer");
    long long tiles_per = 0;
    const long long gy = nn_column_ranges(n, n, NN_ANY_TILES, &tiles_per);
    CSLGAN_REQUIRE(gy >= 1 && gy <= 65535, "gram_d2_u8: n=%lld needs %lld column ranges", (long long)n, gy);
    const long long col_tiles = (n + NN_TN - 1) / NN_TN;
    note_kernel("gram_d2_u8_kernel");
    hipLaunchKernelGGL(gram_d2_u8_kernel, dim3((unsigned)((n + NN_TM - 1) / NN_TM), (unsigned)gy), dim3(NN_THREADS), 0, (hipStream_t)stream,
                       (const signed char*)xs, (const int*)sqnorm, (int)n, Dp, (int)tiles_per, (int)col_tiles, out, (long long)pitch);
    return check_launch("gram_d2_u8_kernel");
}

int cslgan_svc_smo_f64(const uint32_t* d2, int64_t pitch, const int64_t* s, int64_t n, const int8_t* y, const uint8_t* active, int n_problems,
                       double C, double tol, int64_t chunk, int64_t max_iter, double* alpha, double* grad, int64_t* iters, int32_t* done,
                       void* stream) {
    CSLGAN_REQUIRE(d2 && s && y && active && alpha && grad && iters && done, "svc_smo_f64: null argument");
    CSLGAN_REQUIRE(n >= 2 && n <= SVM_MAX_ROWS, "svc_smo_f64: n=%lld must lie in 2 .. %lld", (long long)n, SVM_MAX_ROWS);
    CSLGAN_REQUIRE(pitch >= n && pitch % 32 == 0 && pitch <= SVM_MAX_ROWS, "svc_smo_f64: pitch=%lld must be a multiple of 32 in n .. %lld",
                   (long long)pitch, SVM_MAX_ROWS);
    CSLGAN_REQUIRE(n_problems >= 1 && n_problems <= SVM_MAX_PROBLEMS, "svc_smo_f64: n_problems=%d must lie in 1 .. %d", n_problems,
                   SVM_MAX_PROBLEMS);
    CSLGAN_REQUIRE(C > 0.0 && C < (double)INFINITY, "svc_smo_f64: C=%g must be a finite number > 0", C);
    CSLGAN_REQUIRE(tol > 0.0 && tol < (double)INFINITY, "svc_smo_f64: tol=%g must be a finite number > 0", tol);
    CSLGAN_REQUIRE(chunk >= 1, "svc_smo_f64: chunk=%lld must be >= 1", (long long)chunk);
    CSLGAN_REQUIRE(max_iter >= 0, "svc_smo_f64: max_iter=%lld must be >= 0", (long long)max_iter);
    CSLGAN_REQUIRE(aligned_to(d2, 128) && aligned_to(s, 8) && aligned_to(alpha, 8) && aligned_to(grad, 8) && aligned_to(iters, 8) &&
                       aligned_to(done, 4),
                   "svc_smo_f64: misaligned pointer");
    const bool in_lds = n <= SMO_LDS_ROWS;
    note_kernel("svc_smo_f64_kernel");
    hipLaunchKernelGGL(in_lds ? svc_smo_f64_kernel<true> : svc_smo_f64_kernel<false>, dim3((unsigned)n_problems), dim3(SMO_THREADS), 0,
                       (hipStream_t)stream, d2, (long long)pitch, (const long long*)s, (int)n, (const signed char*)y, (const unsigned char*)active,
                       C, tol, (long long)chunk, (long long)max_iter, alpha, grad, (long long*)iters, (int*)done);
    return check_launch("svc_smo_f64_kernel");
}

}  // extern "C"
