// Membership-inference audit kernels for gfx950 (csl_gan_amd.audit).
//
// Integer / compare work on score arrays that already live in HBM:
//   mem_inf_attack.py:29-66  attack() + _get_random_subset()          -> attack_trials_kernel   (one workgroup = one trial)
//   (addition of this build)  exact rank counts for AUC / TPR at FPR   -> rank_counts_kernel
//   mem_inf_attack.py:80      softmax(logits, 1).max(1)[0]             -> softmax_max_rows_kernel
// The subsets of a trial come from a keyed permutation (swap-or-not shuffle on Philox4x32-10, include/cslgan.h "Audit
// sampler"): every lane evaluates pi(j) on its own, so a trial needs no sort, no rejection loop and no state between trials.
#include "common.h"
#include "device_prims.h"

namespace cslgan {

constexpr int AT_THREADS = 256;
constexpr int AT_MAX_POOL = 4096;                 // n + m: 16 KB of LDS, eight workgroups per CU
constexpr int AT_MAX_ROUNDS = 8 * 31;             // N < 2^31
constexpr uint32_t AT_ROUND_KEY_TAG = 0xFFFFFFFFu;   // word 0 of the counter of K_r (no element index: x < 2^31)
constexpr uint32_t AT_SIDE_TRAIN = 0x7472616Eu, AT_SIDE_NONTRAIN = 0x6E6F6E74u;

// pi(x) of the swap-or-not shuffle over [0, N): round r pairs x with x' = (K_r - x) mod N and moves to x' when the round bit of
// the pair (named by its larger member) is set.  An involution per round, hence a permutation for every N.
__device__ __forceinline__ uint32_t swap_or_not(uint32_t x, uint32_t N, int rounds, const uint32_t* __restrict__ kr, uint32_t t_lo,
                                                uint32_t t_hi_tag, uint32_t k0, uint32_t k1) {
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        uint32_t xp = kr[r] + N - x;              // K_r < N, x < N: 1 .. 2N - 1, no wrap below 2^32
        xp = xp >= N ? xp - N : xp;
        const uint32_t xh = x > xp ? x : xp;
        uint32_t w[4];
        philox4x32_10(xh, (uint32_t)r, t_lo, t_hi_tag, k0, k1, w);
        x = (w[0] & 1u) ? xp : x;
    }
    return x;
}

__global__ __launch_bounds__(AT_THREADS) void attack_trials_kernel(const float* __restrict__ vt, const float* __restrict__ vn, uint32_t N,
                                                                   uint32_t M, int n, int m, int rounds_t, int rounds_n,
                                                                   unsigned long long key, unsigned long long first_trial,
                                                                   uint32_t* __restrict__ hits) {
    __shared__ __attribute__((aligned(16))) float pool[AT_MAX_POOL];
    __shared__ uint32_t kt[AT_MAX_ROUNDS], kn[AT_MAX_ROUNDS];
    __shared__ float red[4];
    const unsigned long long trial = first_trial + (unsigned long long)blockIdx.x;
    const uint32_t t_lo = (uint32_t)trial, t_hi = (uint32_t)(trial >> 32);
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const int tid = threadIdx.x;
    // the round keys, once per workgroup
    for (int r = tid; r < rounds_t + rounds_n; r += AT_THREADS) {
        const bool tr = r < rounds_t;
        const int rr = tr ? r : r - rounds_t;
        uint32_t w[4];
        philox4x32_10(AT_ROUND_KEY_TAG, (uint32_t)rr, t_lo, t_hi ^ (tr ? AT_SIDE_TRAIN : AT_SIDE_NONTRAIN), k0, k1, w);
        const uint32_t K = __umulhi(w[0], tr ? N : M);
        if (tr) kt[rr] = K; else kn[rr] = K;
    }
    __syncthreads();
    // the pool: n train values, then m non-train values
    const int total = n + m;
    for (int i = tid; i < total; i += AT_THREADS) {
        float v;
        if (i < n) v = vt[swap_or_not((uint32_t)i, N, rounds_t, kt, t_lo, t_hi ^ AT_SIDE_TRAIN, k0, k1)];
        else v = vn[swap_or_not((uint32_t)(i - n), M, rounds_n, kn, t_lo, t_hi ^ AT_SIDE_NONTRAIN, k0, k1)];
        pool[i] = v;
    }
    __syncthreads();
    // rank(i) = #{j : v[j] > v[i]} + #{j < i : v[j] == v[i]} for the train rows; every lane reads the same pool address (broadcast)
    int cnt = 0;
    const int quads = total >> 2;
    const float4* __restrict__ pool4 = reinterpret_cast<const float4*>(pool);
    for (int i = tid; i < n; i += AT_THREADS) {
        const float vi = pool[i];
        int rank = 0;
        for (int q = 0; q < quads; ++q) {
            const float4 v = pool4[q];
            const int j = q << 2;
            rank += (v.x > vi || (v.x == vi && j < i)) ? 1 : 0;
            rank += (v.y > vi || (v.y == vi && j + 1 < i)) ? 1 : 0;
            rank += (v.z > vi || (v.z == vi && j + 2 < i)) ? 1 : 0;
            rank += (v.w > vi || (v.w == vi && j + 3 < i)) ? 1 : 0;
        }
        for (int j = quads << 2; j < total; ++j) {
            const float vj = pool[j];
            rank += (vj > vi || (vj == vi && j < i)) ? 1 : 0;
        }
        cnt += rank < n ? 1 : 0;
    }
    const float tot = block_sum_256((float)cnt, red);           // at most 4096: exact in fp32
    if (tid == 0) hits[blockIdx.x] = (uint32_t)(tot + 0.5f);
}

constexpr int RC_THREADS = 256;
constexpr int RC_TILE = 2048;                     // floats of b per LDS tile

__global__ __launch_bounds__(RC_THREADS) void rank_counts_kernel(const float* __restrict__ a, long long na, const float* __restrict__ b,
                                                                 long long nb, uint32_t* __restrict__ gt, uint32_t* __restrict__ eq) {
    __shared__ __attribute__((aligned(16))) float tile[RC_TILE];
    const long long i = (long long)blockIdx.x * RC_THREADS + threadIdx.x;
    const float ai = i < na ? a[i] : 0.f;
    uint32_t g = 0, e = 0;
    for (long long base = 0; base < nb; base += RC_TILE) {
        const int len = (int)(nb - base < RC_TILE ? nb - base : RC_TILE);
        for (int j = threadIdx.x; j < len; j += RC_THREADS) tile[j] = b[base + j];
        __syncthreads();
        const int quads = len >> 2;
        const float4* __restrict__ t4 = reinterpret_cast<const float4*>(tile);
        for (int q = 0; q < quads; ++q) {
            const float4 v = t4[q];
            g += (ai > v.x ? 1u : 0u) + (ai > v.y ? 1u : 0u) + (ai > v.z ? 1u : 0u) + (ai > v.w ? 1u : 0u);
            e += (ai == v.x ? 1u : 0u) + (ai == v.y ? 1u : 0u) + (ai == v.z ? 1u : 0u) + (ai == v.w ? 1u : 0u);
        }
        for (int j = quads << 2; j < len; ++j) {
            const float v = tile[j];
            g += ai > v ? 1u : 0u;
            e += ai == v ? 1u : 0u;
        }
        __syncthreads();
    }
    if (i < na) { gt[i] = g; eq[i] = e; }
}

// One thread per row.  The sum runs in fp64 (B x n_classes <= a few 10^4 exponentials per batch): the result is the correctly
// rounded fp32 of the formula on the fp32 logits, whatever their range.
__global__ void softmax_max_rows_kernel(const float* __restrict__ logits, long long B, int C, float* __restrict__ out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    const float* __restrict__ l = logits + r * C;
    float mx = l[0];
    for (int j = 1; j < C; ++j) mx = l[j] > mx ? l[j] : mx;
    double s = 0.0;
    for (int j = 0; j < C; ++j) s += exp((double)l[j] - (double)mx);
    out[r] = (float)(1.0 / s);
}

static int ceil_log2(long long N) {
    int b = 0;
    while ((1ll << b) < N) ++b;
    return b;
}
static int shuffle_rounds(long long N) {
    const int b = ceil_log2(N);
    return 8 * (b > 1 ? b : 1);
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_attack_trials(const float* vt, int64_t N, const float* vn, int64_t M, int n, int m, uint64_t seed, uint64_t first_trial,
                         int64_t trials, uint32_t* hits, void* stream) {
    CSLGAN_REQUIRE(vt && hits, "attack_trials: null argument");
    CSLGAN_REQUIRE(N >= 1 && N < (1ll << 31), "attack_trials: N=%lld out of range", (long long)N);
    CSLGAN_REQUIRE(M >= 0 && M < (1ll << 31), "attack_trials: M=%lld out of range", (long long)M);
    CSLGAN_REQUIRE(n >= 1 && n <= N, "attack_trials: n=%d must lie in 1 .. N=%lld", n, (long long)N);
    CSLGAN_REQUIRE(m >= 0 && m <= M, "attack_trials: m=%d must lie in 0 .. M=%lld", m, (long long)M);
    CSLGAN_REQUIRE((long long)n + m <= AT_MAX_POOL, "attack_trials: n + m = %lld exceeds the pool of %d", (long long)n + m, AT_MAX_POOL);
    CSLGAN_REQUIRE(vn || m == 0, "attack_trials: null non-train scores with m=%d", m);
    CSLGAN_REQUIRE(trials >= 0 && trials < (1ll << 31), "attack_trials: trials=%lld out of range", (long long)trials);
    if (trials == 0) return CSLGAN_OK;
    note_kernel("attack_trials_kernel");
    hipLaunchKernelGGL(attack_trials_kernel, dim3((unsigned)trials), dim3(AT_THREADS), 0, (hipStream_t)stream, vt, vn, (uint32_t)N, (uint32_t)M, n,
                       m, shuffle_rounds(N), m > 0 ? shuffle_rounds(M) : 0, (unsigned long long)(seed ^ 0x6D656D696E666174ull),
                       (unsigned long long)first_trial, hits);
    return check_launch("attack_trials_kernel");
}

int cslgan_rank_counts(const float* a, int64_t na, const float* b, int64_t nb, uint32_t* gt, uint32_t* eq, void* stream) {
    CSLGAN_REQUIRE(a && gt && eq, "rank_counts: null argument");
    CSLGAN_REQUIRE(na >= 0 && na < (1ll << 31), "rank_counts: na=%lld out of range", (long long)na);
    CSLGAN_REQUIRE(nb >= 0 && nb < (1ll << 31), "rank_counts: nb=%lld out of range", (long long)nb);
    CSLGAN_REQUIRE(b || nb == 0, "rank_counts: null b with nb=%lld", (long long)nb);
    if (na == 0) return CSLGAN_OK;
    note_kernel("rank_counts_kernel");
    hipLaunchKernelGGL(rank_counts_kernel, dim3((unsigned)((na + RC_THREADS - 1) / RC_THREADS)), dim3(RC_THREADS), 0, (hipStream_t)stream, a,
                       (long long)na, b, (long long)nb, gt, eq);
    return check_launch("rank_counts_kernel");
}

int cslgan_softmax_max_rows_f32(const float* logits, int64_t B, int n_classes, float* out, void* stream) {
    CSLGAN_REQUIRE(logits && out, "softmax_max_rows: null argument");
    CSLGAN_REQUIRE(B >= 0 && B < (1ll << 31), "softmax_max_rows: B=%lld out of range", (long long)B);
    CSLGAN_REQUIRE(n_classes >= 1 && n_classes <= 64, "softmax_max_rows: n_classes=%d must lie in 1 .. 64", n_classes);
    if (B == 0) return CSLGAN_OK;
    note_kernel("softmax_max_rows_kernel");
    hipLaunchKernelGGL(softmax_max_rows_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, (hipStream_t)stream, logits, (long long)B, n_classes,
                       out);
    return check_launch("softmax_max_rows_kernel");
}

}  // extern "C"
