// Naive Bayes on cache bytes (include/cslgan.h "naive Bayes"; csl_gan_amd.classify.NaiveBayes): the exact per-class
// byte moments of a training cache in one pass, and the two score sums of a test cache in one pass.
//
// cslgan_class_moments_u8 — nb_moments_kernel.  One WAVE per workgroup.  A workgroup owns a chunk of at most NBM_MAX_ROWS rows
// (blockIdx.x), a slab of 1024 columns (blockIdx.y: lane l owns the 16 columns [16 l, 16 l + 16) of it, one 16-byte load per row) and
// a group of four classes (blockIdx.z).  It reads the chunk's labels 64 at a time, and of those rows only the ones of its own classes
// (a row of another group is never loaded: over the groups every byte of X is read once).  A row's label is uniform across the wave,
// so the lane adds its 16 bytes to ITS entries of an LDS table [class][column] with plain read-modify-write: no LDS atomics, no
// barrier in the row loop — no other lane touches those entries before the flush.  NBM_UNROLL rows are in flight per lane.  Two
// 32-bit partials per (class, column): sum b^2, and sum b in bits 0 .. 19 with the count of b > binarize in bits 20 .. 31.
//   Where the partials are flushed: once, at the end of the chunk, and a chunk has at most NBM_MAX_ROWS = 2048 rows, so
//   sum b^2 <= 2048 * 65025 < 2^28, sum b <= 2048 * 255 < 2^20 and the count <= 2048 < 2^12: nothing wraps, whatever N is (a 32-bit
//   sum of squares would wrap after 66 051 rows of 255).  The flush adds each nonzero partial to the int64 outputs with a 64-bit
//   integer vector atomic (global_atomic_add_x2): integer addition is associative, so the result is the exact sum in every
//   schedule.  The outputs are zeroed before the launch by cslgan::zero_floats.
//
// cslgan_nb_score_gauss_u8 / _bern_u8 — nb_score_kernel<AL, GAUSS, KP>.  256 threads own 64 rows and walk the row in slabs of 256
// columns: thread t holds the 16 bytes [16 (t % 16), +16) of the slab of rows 4 (t / 16) .. + 3 (four 16-byte loads), the slab of the
// tables ([KP][256] of m and w, or of delta) is staged in LDS once per workgroup and every element read from there serves the
// thread's four rows (and, as an LDS broadcast, the 16 threads of a wave that share its columns).  The bytes and the table column of
// the next slab are loaded into registers while the current one is computed, where the registers allow it (PF).  KP >= K is a
// template parameter: the accumulators [4][KP] are registers, and K = 2 keeps four waves per SIMD where 16 classes leave two.
//   The chain of fp32 additions of one (row, class) sum, s: the 16 terms of a slab are added in order into a fresh partial (15), the
//   partial is added to the thread's accumulator (at most 65536 / 256 = 256 slabs), and the 16 accumulators of a row are added in a
//   butterfly (4): s = 15 + 256 + 4 = 275 <= 320.  A term takes three roundings (b - m, its square, times w), so
//   |S_dev - S_host| <= (s + 3) 2^-24 T = 1.66e-5 T <= 2e-5 T with T the float64 sum of the absolute terms.  The subtraction comes
//   first; the expanded quadratic is never formed.  No atomics: the order is fixed, the same inputs return the same bits.
#include "ovr_rows.h"

namespace cslgan {

constexpr int NB_MAX_K = 16;
constexpr int NB_MAX_D = 65536;
constexpr int NBM_SLAB = 1024;           // columns of a moments workgroup: 64 lanes x 16 bytes
constexpr int NBM_GROUP = 4;             // classes of a moments workgroup
constexpr int NBM_MAX_ROWS = 2048;       // rows of a chunk: the bound that keeps the packed 32-bit partials from wrapping
constexpr int NBM_MIN_ROWS = 128;
constexpr int NBM_UNROLL = 8;            // rows in flight per lane
constexpr unsigned NBM_CNT_ONE = 1u << 20;
constexpr int NBS_THREADS = 256;
constexpr int NBS_RR = 4;                // rows of a score thread: every table element read from LDS serves them
constexpr int NBS_ROWS = 16 * NBS_RR;    // rows of a score workgroup: 16 row groups
constexpr int NBS_SLAB = 256;            // columns of a slab: 16 column lanes x 16 bytes

__device__ __forceinline__ unsigned nb_word(const u32x4& v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }

template <bool AL>
__global__ __launch_bounds__(64) void nb_moments_kernel(const unsigned char* __restrict__ x, const int* __restrict__ labels, long long N, int D,
                                                        int K, int binarize, int rpc, unsigned long long* __restrict__ n_out,
                                                        unsigned long long* __restrict__ s1, unsigned long long* __restrict__ s2,
                                                        unsigned long long* __restrict__ cnt) {
    // [table: 0 = sum b | count << 20, 1 = sum b^2][class of the group, G = min(K, NBM_GROUP) of them][16-byte piece of the lane's 16
    // columns][lane]: a wave's 16-byte accesses are 1 KiB contiguous.  8 KiB per class: K = 2 leaves room for 10 workgroups per CU
    extern __shared__ u32x4 nbm_tab[];
    const int G = K < NBM_GROUP ? K : NBM_GROUP;
    u32x4* const tab0 = nbm_tab;
    u32x4* const tab1 = nbm_tab + G * 256;
    const int lane = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * rpc;
    const long long r1 = r0 + rpc < N ? r0 + rpc : N;
    const int col0 = blockIdx.y * NBM_SLAB, col = col0 + lane * 16;
    const int k0 = blockIdx.z * NBM_GROUP;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    const unsigned thr = (unsigned)binarize;
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < NBM_GROUP; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c < G) { tab0[(c * 4 + j) * 64 + lane] = zero; tab1[(c * 4 + j) * 64 + lane] = zero; }
    int rows_of[NBM_GROUP] = {0, 0, 0, 0};

    for (long long base = r0; base < r1; base += 64) {
        const long long row = base + lane;
        const int lab = row < r1 ? labels[row] : -1;
        const int rel = lab - k0;
        const bool mine = lab >= 0 && lab < K && rel >= 0 && rel < NBM_GROUP;
        unsigned long long todo = __ballot(mine);
#pragma unroll
        for (int c = 0; c < NBM_GROUP; ++c) rows_of[c] += __popcll(__ballot(mine && rel == c));
        while (todo) {                                               // wave-uniform: up to NBM_UNROLL rows of this group per turn
            int at[NBM_UNROLL], cls[NBM_UNROLL];
            bool has[NBM_UNROLL];
            u32x4 v[NBM_UNROLL];
#pragma unroll
            for (int u = 0; u < NBM_UNROLL; ++u) {
                has[u] = todo != 0ull;
                at[u] = has[u] ? __builtin_ctzll(todo) : 0;
                todo &= todo - 1ull;                                 // 0 stays 0
                cls[u] = __builtin_amdgcn_readfirstlane(__shfl(rel, at[u], 64));
                cls[u] = has[u] ? cls[u] : 0;
            }
#pragma unroll
            for (int u = 0; u < NBM_UNROLL; ++u)
                v[u] = lrb_load16<AL>(x, total, whole, (unsigned long long)(base + at[u]) * (unsigned long long)D, col, D, has[u]);
#pragma unroll
            for (int u = 0; u < NBM_UNROLL; ++u) {
                if (!has[u]) continue;                               // uniform
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned w = nb_word(v[u], j);
                    const int at_tab = (cls[u] * 4 + j) * 64 + lane;
                    u32x4 a = tab0[at_tab], q = tab1[at_tab];
                    const unsigned b0 = w & 0xffu, b1 = (w >> 8) & 0xffu, b2 = (w >> 16) & 0xffu, b3 = w >> 24;
                    a.x += b0 + (b0 > thr ? NBM_CNT_ONE : 0u); q.x += b0 * b0;
                    a.y += b1 + (b1 > thr ? NBM_CNT_ONE : 0u); q.y += b1 * b1;
                    a.z += b2 + (b2 > thr ? NBM_CNT_ONE : 0u); q.z += b2 * b2;
                    a.w += b3 + (b3 > thr ? NBM_CNT_ONE : 0u); q.w += b3 * b3;
                    tab0[at_tab] = a;
                    tab1[at_tab] = q;
                }
            }
        }
    }
    __syncthreads();                                                 // the flush reads other lanes' entries
    const unsigned* t1 = reinterpret_cast<const unsigned*>(tab0);
    const unsigned* t2 = reinterpret_cast<const unsigned*>(tab1);
    for (int c = 0; c < NBM_GROUP; ++c) {
        const int k = k0 + c;
        if (k >= K) break;
        if (blockIdx.y == 0 && lane == 0 && rows_of[c] > 0) atomicAdd(&n_out[k], (unsigned long long)rows_of[c]);
        if (rows_of[c] == 0) continue;                               // uniform: nothing of this class in the chunk
        for (int cc = lane; cc < NBM_SLAB; cc += 64) {               // consecutive lanes, consecutive columns
            const int column = col0 + cc;
            if (column >= D) break;
            const int idx = ((c * 4 + ((cc & 15) >> 2)) * 64 + (cc >> 4)) * 4 + (cc & 3);
            const unsigned a = t1[idx], q = t2[idx];
            const size_t o = (size_t)k * (size_t)D + (size_t)column;
            if (a & (NBM_CNT_ONE - 1u)) atomicAdd(&s1[o], (unsigned long long)(a & (NBM_CNT_ONE - 1u)));
            if (a >> 20) atomicAdd(&cnt[o], (unsigned long long)(a >> 20));
            if (q) atomicAdd(&s2[o], (unsigned long long)q);
        }
    }
}

// byte e (0 .. 3) of a 32-bit word as the exact float 0 .. 255
__device__ __forceinline__ float nb_bytef(unsigned w, int e) { return (float)((w >> (8 * e)) & 0xffu); }

template <bool AL, bool GAUSS, int KP>
__global__ __launch_bounds__(NBS_THREADS) void nb_score_kernel(const unsigned char* __restrict__ x, const float* __restrict__ ta,
                                                               const float* __restrict__ tb, long long M, int D, int K, int binarize,
                                                               float* __restrict__ S) {
    // [table: m / delta, w][class][16-byte piece j of a thread's 16 columns][column lane]: the 16 column lanes of a wave read 256
    // contiguous bytes, its four row groups the same ones
    __shared__ f32x4 tab[GAUSS ? 2 : 1][KP][4][16];
    constexpr int NT = GAUSS ? 2 : 1;
    const int tid = threadIdx.x, cl = tid & 15, rg = tid >> 4;
    const long long row0 = (long long)blockIdx.x * NBS_ROWS + rg * NBS_RR;
    const unsigned long long total = (unsigned long long)M * (unsigned long long)D, whole = total & ~15ull;
    const float thr = (float)binarize;
    const int at = (((tid & 15) >> 2) * 16 + (tid >> 4)) * 4 + (tid & 3);   // where column tid of a slab sits in a class's 256 floats
    float* const ma = reinterpret_cast<float*>(&tab[0][0][0][0]);
    float acc[NBS_RR][KP];                                         // KP >= K (nb_score picks it); the classes K .. KP-1 are zeros
#pragma unroll
    for (int r = 0; r < NBS_RR; ++r)
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[r][k] = 0.f;

    // fetch: the bytes (v) and this thread's column of the tables (tn; NBS_SLAB == NBS_THREADS, a thread stages one column) of a slab,
    // into registers.  PF — one slab ahead: slab s + 1 is fetched after slab s's tables are in LDS and is in flight while slab s is
    // computed.  Only where the registers allow it: few classes and aligned rows (the unaligned loader is register-hungry); elsewhere
    // the second set of registers would cost the second wave per SIMD, and the slab is fetched at the top of its own turn.
    constexpr bool PF = AL && KP <= 4;
    u32x4 v[NBS_RR];
    float tn[NT][KP];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int r = 0; r < NBS_RR; ++r)
            v[r] = lrb_load16<AL>(x, total, whole, (unsigned long long)(row0 + r) * (unsigned long long)D, c0 + cl * 16, D, row0 + r < M);
        const int column = c0 + tid;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool in = k < K && column < D;
            const size_t o = in ? (size_t)k * (size_t)D + (size_t)column : 0;       // always a load, from entry 0 where there is none
            const float a = ta[o];
            tn[0][k] = in ? a : 0.f;
            if (GAUSS) { const float w = tb[o]; tn[NT - 1][k] = in ? w : 0.f; }      // w = 0 beyond D and K: the zero bytes there add 0
        }
    };
    if (PF) fetch(0);
    for (int c0 = 0; c0 < D; c0 += NBS_SLAB) {
        if (!PF) fetch(c0);
        __syncthreads();                                             // the previous slab's tables have been read
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            ma[k * 256 + at] = tn[0][k];
            if (GAUSS) ma[KP * 256 + k * 256 + at] = tn[NT - 1][k];
        }
        float xb[NBS_RR][16];
#pragma unroll
        for (int r = 0; r < NBS_RR; ++r)
#pragma unroll
            for (int e = 0; e < 16; ++e) xb[r][e] = nb_bytef(nb_word(v[r], e >> 2), e & 3);
        __syncthreads();
        if (PF && c0 + NBS_SLAB < D) fetch(c0 + NBS_SLAB);           // uniform
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            float part[NBS_RR];
#pragma unroll
            for (int r = 0; r < NBS_RR; ++r) part[r] = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 a = tab[0][k][j][cl];
                f32x4 w = a;
                if (GAUSS) w = tab[NT - 1][k][j][cl];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int r = 0; r < NBS_RR; ++r) {
                        const float b = xb[r][4 * j + e];
                        if (GAUSS) {
                            const float d = b - a[e];
                            part[r] += w[e] * (d * d);
                        } else {
                            part[r] += b > thr ? a[e] : 0.f;
                        }
                    }
            }
#pragma unroll
            for (int r = 0; r < NBS_RR; ++r) acc[r][k] += part[r];
        }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (k >= K) continue;                                        // a guard, not a break: the loop unrolls, acc stays in registers
#pragma unroll
        for (int r = 0; r < NBS_RR; ++r) {
            float s = acc[r][k];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);           // the 16 column lanes of a row sit in one wave
            if (cl == 0 && row0 + r < M) S[(size_t)(row0 + r) * (size_t)K + (size_t)k] = s;
        }
    }
}

static int nb_score(const char* what, bool gauss, const void* X, const float* ta, const float* tb, int64_t M, int D, int K, int binarize, float* S,
                    void* stream) {
    CSLGAN_REQUIRE(X && ta && (tb || !gauss) && S, "%s: null argument", what);
    CSLGAN_REQUIRE(K >= 2 && K <= NB_MAX_K, "%s: K=%d must lie in 2 .. %d", what, K, NB_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= NB_MAX_D, "%s: D=%d must lie in 1 .. %d", what, D, NB_MAX_D);
    CSLGAN_REQUIRE(M >= 1 && M < (1ll << 31), "%s: M=%lld out of range", what, (long long)M);
    CSLGAN_REQUIRE(binarize >= 0 && binarize <= 254, "%s: binarize=%d must lie in 0 .. 254", what, binarize);
    CSLGAN_REQUIRE(aligned16(X), "%s: X misaligned (16 bytes)", what);
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(ta) & 3u) == 0 && (reinterpret_cast<uintptr_t>(tb) & 3u) == 0 && (reinterpret_cast<uintptr_t>(S) & 3u) == 0,
                   "%s: table or output misaligned (4 bytes)", what);
    const bool al = D % 16 == 0;
    const dim3 grid((unsigned)((M + NBS_ROWS - 1) / NBS_ROWS)), block(NBS_THREADS);
    const unsigned char* x = (const unsigned char*)X;
    hipStream_t st = (hipStream_t)stream;
    // the class count is a template parameter (the accumulators are registers): K itself where a dataset is likely to have it (2, 3, 4,
    // MNIST's 10), else the next of 6, 8, 12, 16 with the classes K .. KP-1 as zeros
    const int kp = K <= 4 ? K : (K <= 6 ? 6 : (K <= 8 ? 8 : (K <= 10 ? 10 : (K <= 12 ? 12 : 16))));
    note_kernel("nb_score_kernel<%s, %d>", gauss ? "gauss" : "bern", kp);
    void (*kern)(const unsigned char*, const float*, const float*, long long, int, int, int, float*) = nullptr;
#define NB_PICK(KP)                                                                                                              \
    kern = gauss ? (al ? nb_score_kernel<true, true, KP> : nb_score_kernel<false, true, KP>)                                      \
                 : (al ? nb_score_kernel<true, false, KP> : nb_score_kernel<false, false, KP>)
    switch (kp) {
        case 2: NB_PICK(2); break;
        case 3: NB_PICK(3); break;
        case 4: NB_PICK(4); break;
        case 6: NB_PICK(6); break;
        case 8: NB_PICK(8); break;
        case 10: NB_PICK(10); break;
        case 12: NB_PICK(12); break;
        default: NB_PICK(16); break;
    }
#undef NB_PICK
    hipLaunchKernelGGL(kern, grid, block, 0, st, x, ta, tb, (long long)M, D, K, binarize, S);
    return check_launch("nb_score_kernel");
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_class_moments_u8(const void* X, const int32_t* labels, int64_t N, int D, int K, int binarize, int64_t* n, int64_t* s1, int64_t* s2,
                            int64_t* cnt, void* ws, void* stream) {
    (void)ws;                                                        // the atomic flush needs no workspace
    CSLGAN_REQUIRE(X && labels && n && s1 && s2 && cnt, "class_moments_u8: null argument");
    CSLGAN_REQUIRE(K >= 2 && K <= NB_MAX_K, "class_moments_u8: K=%d must lie in 2 .. %d", K, NB_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= NB_MAX_D, "class_moments_u8: D=%d must lie in 1 .. %d", D, NB_MAX_D);
    CSLGAN_REQUIRE(N >= 1 && N < (1ll << 31), "class_moments_u8: N=%lld out of range", (long long)N);
    CSLGAN_REQUIRE(binarize >= 0 && binarize <= 254, "class_moments_u8: binarize=%d must lie in 0 .. 254", binarize);
    CSLGAN_REQUIRE(aligned16(X), "class_moments_u8: X misaligned (16 bytes)");
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 3u) == 0, "class_moments_u8: labels misaligned (4 bytes)");
    CSLGAN_REQUIRE(((reinterpret_cast<uintptr_t>(n) | reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(cnt)) & 7u) == 0,
                   "class_moments_u8: output misaligned (8 bytes)");
    hipStream_t st = (hipStream_t)stream;
    const size_t kd2 = 2 * (size_t)K * (size_t)D;                    // an int64 zero is two float zeros
    if (int rc = zero_floats((float*)n, 2 * (size_t)K, st)) return rc;
    if (int rc = zero_floats((float*)s1, kd2, st)) return rc;
    if (int rc = zero_floats((float*)s2, kd2, st)) return rc;
    if (int rc = zero_floats((float*)cnt, kd2, st)) return rc;
    // rows per chunk: about 1024 workgroups where N allows it, never more than NBM_MAX_ROWS rows (the wrap bound), a multiple of 64
    const int slabs = (D + NBM_SLAB - 1) / NBM_SLAB, groups = (K + NBM_GROUP - 1) / NBM_GROUP;
    const long long chunks_wanted = (1024 + slabs * groups - 1) / (slabs * groups);
    long long rpc = (N + chunks_wanted - 1) / chunks_wanted;
    rpc = (rpc + 63) / 64 * 64;
    rpc = rpc < NBM_MIN_ROWS ? NBM_MIN_ROWS : (rpc > NBM_MAX_ROWS ? NBM_MAX_ROWS : rpc);
    const dim3 grid((unsigned)((N + rpc - 1) / rpc), (unsigned)slabs, (unsigned)groups);
    const size_t lds = (size_t)(K < NBM_GROUP ? K : NBM_GROUP) * 2 * 256 * sizeof(u32x4);       // at most 32 KiB
    note_kernel("nb_moments_kernel");
    if (D % 16 == 0)
        hipLaunchKernelGGL(nb_moments_kernel<true>, grid, dim3(64), lds, st, (const unsigned char*)X, labels, (long long)N, D, K, binarize, (int)rpc,
                           (unsigned long long*)n, (unsigned long long*)s1, (unsigned long long*)s2, (unsigned long long*)cnt);
    else
        hipLaunchKernelGGL(nb_moments_kernel<false>, grid, dim3(64), lds, st, (const unsigned char*)X, labels, (long long)N, D, K, binarize, (int)rpc,
                           (unsigned long long*)n, (unsigned long long*)s1, (unsigned long long*)s2, (unsigned long long*)cnt);
    return check_launch("nb_moments_kernel");
}

int cslgan_nb_score_gauss_u8(const void* X, const float* m, const float* w, int64_t M, int D, int K, float* S, void* stream) {
    return nb_score("nb_score_gauss_u8", true, X, m, w, M, D, K, 0, S, stream);
}

int cslgan_nb_score_bern_u8(const void* X, const float* delta, int64_t M, int D, int K, int binarize, float* S, void* stream) {
    return nb_score("nb_score_bern_u8", false, X, delta, nullptr, M, D, K, binarize, S, stream);
}

}  // extern "C"
