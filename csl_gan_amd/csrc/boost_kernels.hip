// Boosted stumps on cache bytes (include/cslgan.h "boosted stumps"; csl_gan_amd.classify.AdaBoost): the stump search of
// one boosting round — the K one-vs-rest classes over all N rows in one launch — under fixed-point row weights 0 .. 2^28.
//
// cslgan_boost_stump_u8 — boost_stump_tile_kernel, then boost_stump_reduce_kernel.  The frame is tree_split_tile_kernel's
// (tree_kernels.hip): a workgroup of 256 threads owns one (class, 16-feature tile) pair, a row's sixteen features are one 16-byte load
// (lrb_load16: rows need not be aligned, D may be below 16, no byte beyond X is read), a feature's histogram has a pitch of 257
// entries and lane l starts at feature l % 16, so that lanes holding the same byte hit different bank pairs.  What differs:
//   Rows: all N, contiguous; no row-index array, no segments, no feature mask.  Workgroup b is tile b / K, class b % K: the K
//   workgroups of a tile are neighbours and the tile's bytes come from HBM once and from L2 for the other K - 1.
//   Counters: sum w may reach 2^24 2^28 = 2^52, so a bin cannot hold n and p in the halves of one entry.  A feature has two
//   histograms of 64-bit entries, one of the negative rows and one of the positive rows; a row adds its weight to the one its target
//   names: still ONE 64-bit LDS atomic per byte.  2 x 16 x 257 x 8 bytes = 64.25 KiB leave two workgroups per CU of the 160 KiB.
//   A weight is clamped into 0 .. 2^28 before it is added: no counter can wrap, whatever the caller hands over.
//   Scan: a wave takes a feature; lane l owns the bins 4 l .. 4 l + 3; 64-bit wave prefix sums give (nL, pL) at every bin, a suffix
//   minimum the next larger byte present.  The score is (a a) / fl(nL) + (c c) / fl(nR) with a = fl(pL), c = fl(p - pL): every integer
//   is below 2^53, so the four conversions are exact, and the five operations are __dmul_rn, __ddiv_rn, __dadd_rn — each rounded once,
//   and no product feeds an addition, so nothing can be contracted.
//   The tile's best candidate — tree_better: largest score, smallest feature, smallest byte — goes to the workspace with the totals
//   (n, p), which every tile has from its first feature; boost_stump_reduce_kernel (a wave per class) reduces the tiles.
#include "ovr_rows.h"
#include "tree_best.h"

namespace cslgan {

constexpr int BS_MAX_K = 16;
constexpr int BS_MAX_D = 65536;
constexpr long long BS_MAX_N = 1ll << 24;
constexpr int BS_W1 = 1 << 28;           // the largest weight
constexpr int BS_TILE = 16;              // features of a workgroup: one 16-byte load per row
constexpr int BS_THREADS = 256;
constexpr int BS_PITCH = 257;            // entries of a feature's histogram: 256 bins and one of padding
constexpr int BS_PLANE = BS_TILE * BS_PITCH;     // entries of the negative rows' histograms; the positive rows' follow
constexpr int BS_REC = 8;                // int64 words of a tile record: score bits, j, v, v_hi, nL, pL, n, p

using BoostBest = TreeBestT<unsigned long long>;

template <bool AL>
__global__ __launch_bounds__(BS_THREADS) void boost_stump_tile_kernel(const unsigned char* __restrict__ x, const int* __restrict__ labels,
                                                                      const int* __restrict__ weights, long long N, int D, int K,
                                                                      long long* __restrict__ tile_rec) {
    __shared__ unsigned long long hist[2 * BS_PLANE];
    __shared__ unsigned long long s_tot[2];
    __shared__ BoostBest s_best[BS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = (int)(blockIdx.x / (unsigned)K), cls = (int)(blockIdx.x % (unsigned)K);
    const int j0 = tile * BS_TILE;

    for (int i = tid; i < 2 * BS_PLANE; i += BS_THREADS) hist[i] = 0ull;
    __syncthreads();

    const int* const wp = weights + (size_t)cls * (size_t)N;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    for (long long i = tid; i < N; i += BS_THREADS) {
        int wi = wp[i];
        wi = wi < 0 ? 0 : (wi > BS_W1 ? BS_W1 : wi);
        if (wi == 0) continue;                                       // a row of weight 0 is not there
        unsigned long long* const h = hist + (labels[i] == cls ? BS_PLANE : 0);
        const unsigned long long inc = (unsigned long long)wi;
        const u32x4 v = lrb_load16<AL>(x, total, whole, (unsigned long long)i * (unsigned long long)D, j0, D, true);
#pragma unroll
        for (int e = 0; e < BS_TILE; ++e) {
            const int f = (e + tid) & (BS_TILE - 1);
            const unsigned word = (f >> 2) == 0 ? v.x : ((f >> 2) == 1 ? v.y : ((f >> 2) == 2 ? v.z : v.w));
            const unsigned b = (word >> (8 * (f & 3))) & 0xffu;
            atomicAdd(&h[f * BS_PITCH + (int)b], inc);               // the bytes of the features from D on are zeros; nobody scans them
        }
    }
    __syncthreads();

    BoostBest wbest = {-1.0, -1, -1, -1, 0ull, 0ull};
    for (int f = wv; f < BS_TILE && j0 + f < D; f += BS_THREADS / 64) {      // wave-uniform
        const unsigned long long* const hn = hist + f * BS_PITCH + lane * 4;
        unsigned long long nb[4], pb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { pb[q] = hn[BS_PLANE + q]; nb[q] = hn[q] + pb[q]; }
        const unsigned long long sn = nb[0] + nb[1] + nb[2] + nb[3], sp = pb[0] + pb[1] + pb[2] + pb[3];
        unsigned long long cn = sn, cp = sp;                         // inclusive prefix sums over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long a = __shfl_up(cn, o, 64), b = __shfl_up(cp, o, 64);
            if (lane >= o) { cn += a; cp += b; }
        }
        const unsigned long long ntot = __shfl(cn, 63, 64), ptot = __shfl(cp, 63, 64);
        if (f == 0 && lane == 0) { s_tot[0] = ntot; s_tot[1] = ptot; }
        int first = 256;                                             // the smallest byte present among this lane's four
#pragma unroll
        for (int q = 3; q >= 0; --q) if (nb[q]) first = lane * 4 + q;
        int sfx = first;                                             // inclusive suffix minimum over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int a = __shfl_down(sfx, o, 64);
            if (lane + o < 64) sfx = a < sfx ? a : sfx;
        }
        int nxt = __shfl_down(sfx, 1, 64);
        if (lane == 63) nxt = 256;
        int hi[4];
#pragma unroll
        for (int q = 3; q >= 0; --q) { hi[q] = nxt; if (nb[q]) nxt = lane * 4 + q; }
        BoostBest best = {-1.0, -1, -1, -1, 0ull, 0ull};
        unsigned long long bn = cn - sn, bp = cp - sp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bn += nb[q]; bp += pb[q];
            if (nb[q] && bn < ntot) {                                // the byte is present and a row lies to its right
                const double a = (double)bp, c = (double)(ptot - bp);
                const double s = __dadd_rn(__ddiv_rn(__dmul_rn(a, a), (double)bn), __ddiv_rn(__dmul_rn(c, c), (double)(ntot - bn)));
                if (s > best.s) { best.s = s; best.j = j0 + f; best.v = lane * 4 + q; best.vh = hi[q]; best.nL = bn; best.pL = bp; }
            }
        }
        tree_wave_best(best);
        if (tree_better(best.s, best.j, best.v, wbest.s, wbest.j, wbest.v)) wbest = best;
    }
    if (lane == 0) s_best[wv] = wbest;
    __syncthreads();
    if (tid == 0) {
        BoostBest b = s_best[0];
        for (int w = 1; w < BS_THREADS / 64; ++w)
            if (tree_better(s_best[w].s, s_best[w].j, s_best[w].v, b.s, b.j, b.v)) b = s_best[w];
        long long* const rec = tile_rec + (size_t)blockIdx.x * BS_REC;
        rec[0] = __double_as_longlong(b.s); rec[1] = b.j; rec[2] = b.v; rec[3] = b.vh;
        rec[4] = (long long)b.nL; rec[5] = (long long)b.pL; rec[6] = (long long)s_tot[0]; rec[7] = (long long)s_tot[1];
    }
}

// A wave per class: the best of its tiles' candidates, the totals from tile 0.
__global__ __launch_bounds__(BS_THREADS) void boost_stump_reduce_kernel(const long long* __restrict__ tile_rec, int K, int tiles,
                                                                        long long* __restrict__ out, long long* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int cls = (int)blockIdx.x * (BS_THREADS / 64) + (int)(threadIdx.x >> 6);
    if (cls >= K) return;                                            // wave-uniform
    BoostBest best = {-1.0, -1, -1, -1, 0ull, 0ull};
    for (int t = lane; t < tiles; t += 64) {
        const long long* const rec = tile_rec + ((size_t)t * (size_t)K + (size_t)cls) * BS_REC;
        const double s = __longlong_as_double(rec[0]);
        if (tree_better(s, (int)rec[1], (int)rec[2], best.s, best.j, best.v)) {
            best.s = s; best.j = (int)rec[1]; best.v = (int)rec[2]; best.vh = (int)rec[3];
            best.nL = (unsigned long long)rec[4]; best.pL = (unsigned long long)rec[5];
        }
    }
    tree_wave_best(best);
    if (lane == 0) {
        const long long* const rec0 = tile_rec + (size_t)cls * BS_REC;
        long long* const o = out + (size_t)cls * 7;
        const bool found = best.s >= 0.0 && best.j >= 0;
        o[0] = found ? best.j : -1; o[1] = found ? best.v : -1; o[2] = found ? best.vh : -1;
        o[3] = found ? (long long)best.nL : 0ll; o[4] = found ? (long long)best.pL : 0ll; o[5] = rec0[6]; o[6] = rec0[7];
        score[cls] = found ? __double_as_longlong(best.s) : 0ll;
    }
}

static inline bool bs_aligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int64_t cslgan_boost_stump_ws_bytes(int K, int D) {
    if (K < 2 || K > BS_MAX_K || D < 1 || D > BS_MAX_D) return 0;
    return (int64_t)K * ((D + BS_TILE - 1) / BS_TILE) * (int64_t)(BS_REC * sizeof(long long));
}

int cslgan_boost_stump_u8(const void* X, const int32_t* labels, const int32_t* weights, int64_t N, int D, int K, int64_t* out, int64_t* score,
                          void* ws, int64_t ws_bytes, void* stream) {
    CSLGAN_REQUIRE(X && labels && weights && out && score && ws, "boost_stump_u8: null argument");
    CSLGAN_REQUIRE(K >= 2 && K <= BS_MAX_K, "boost_stump_u8: K=%d must lie in 2 .. %d", K, BS_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= BS_MAX_D, "boost_stump_u8: D=%d must lie in 1 .. %d", D, BS_MAX_D);
    CSLGAN_REQUIRE(N >= 1 && N < BS_MAX_N, "boost_stump_u8: N=%lld must lie in 1 .. 2^24 - 1", (long long)N);
    const int64_t need = cslgan_boost_stump_ws_bytes(K, D);
    CSLGAN_REQUIRE(ws_bytes >= need, "boost_stump_u8: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
    CSLGAN_REQUIRE(aligned16(X), "boost_stump_u8: X misaligned (16 bytes)");
    CSLGAN_REQUIRE(bs_aligned(labels, 3u) && bs_aligned(weights, 3u), "boost_stump_u8: int32 array misaligned (4 bytes)");
    CSLGAN_REQUIRE(bs_aligned(out, 7u) && bs_aligned(score, 7u) && bs_aligned(ws, 7u), "boost_stump_u8: out, score or workspace misaligned (8 bytes)");
    const int tiles = (D + BS_TILE - 1) / BS_TILE;
    hipStream_t st = (hipStream_t)stream;
    long long* const tile_rec = (long long*)ws;
    const dim3 grid((unsigned)(tiles * K)), block(BS_THREADS);
    note_kernel("boost_stump_tile_kernel");
    if (D % 16 == 0)
        hipLaunchKernelGGL(boost_stump_tile_kernel<true>, grid, block, 0, st, (const unsigned char*)X, labels, weights, (long long)N, D, K, tile_rec);
    else
        hipLaunchKernelGGL(boost_stump_tile_kernel<false>, grid, block, 0, st, (const unsigned char*)X, labels, weights, (long long)N, D, K, tile_rec);
    if (int rc = check_launch("boost_stump_tile_kernel")) return rc;
    hipLaunchKernelGGL(boost_stump_reduce_kernel, dim3((unsigned)((K + BS_THREADS / 64 - 1) / (BS_THREADS / 64))), block, 0, st, tile_rec, K, tiles,
                       (long long*)out, (long long*)score);
    return check_launch("boost_stump_reduce_kernel");
}

}  // extern "C"
