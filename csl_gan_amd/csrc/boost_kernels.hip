// Boosted stumps on cache bytes (include/cslgan.h "boosted stumps"; csl_gan_amd.classify.AdaBoost): the stump search of
// one boosting round — the K one-vs-rest classes over all N rows in one launch — under fixed-point row weights 0 .. 2^28.
//
// cslgan_boost_stump_u8 — boost_stump_tile_kernel, then boost_stump_reduce_kernel, on the frame of byte_split.h (the histograms in LDS,
// the scan, the one score routine, the tie rule and the reductions, shared with tree_kernels.hip).  What is boosting's own:
//   Rows: all N, contiguous; no row-index array, no segments, no feature mask.  Workgroup b is tile b / K, class b % K: the K
//   workgroups of a tile are neighbours and the tile's bytes come from HBM once and from L2 for the other K - 1.
//   Counters: sum w may reach 2^24 2^28 = 2^52, so a bin cannot hold n and p in the halves of one entry.  A feature has two
//   histograms of 64-bit entries, one of the negative rows and one of the positive rows; a row adds its weight to the one its target
//   names: still ONE 64-bit LDS atomic per byte.  2 x 16 x 257 x 8 bytes = 64.25 KiB leave two workgroups per CU of the 160 KiB.
//   A weight is clamped into 0 .. 2^28 before it is added: no counter can wrap, whatever the caller hands over.
//   Record: eight int64 words per tile, the score bits first and the totals (n, p), which every tile has from its first feature, last.
#include "byte_split.h"

namespace cslgan {

constexpr int BS_W1 = 1 << 28;           // the largest weight
constexpr int BS_PLANE = SPLIT_TILE * SPLIT_PITCH;       // entries of the negative rows' histograms; the positive rows' follow
constexpr int BS_REC = 8;                // int64 words of a tile record: score bits, j, v, v_hi, nL, pL, n, p

using BoostBest = SplitBest<unsigned long long>;

template <bool AL>
__global__ __launch_bounds__(SPLIT_THREADS) void boost_stump_tile_kernel(const unsigned char* __restrict__ x, const int* __restrict__ labels,
                                                                         const int* __restrict__ weights, long long N, int D, int K,
                                                                         long long* __restrict__ tile_rec) {
    __shared__ unsigned long long hist[2 * BS_PLANE];
    __shared__ unsigned long long s_tot[2];
    __shared__ BoostBest s_best[SPLIT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = (int)(blockIdx.x / (unsigned)K), cls = (int)(blockIdx.x % (unsigned)K);
    const int j0 = tile * SPLIT_TILE;

    for (int i = tid; i < 2 * BS_PLANE; i += SPLIT_THREADS) hist[i] = 0ull;
    __syncthreads();

    const int* const wp = weights + (size_t)cls * (size_t)N;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    for (long long i = tid; i < N; i += SPLIT_THREADS) {
        int wi = wp[i];
        wi = wi < 0 ? 0 : (wi > BS_W1 ? BS_W1 : wi);
        if (wi == 0) continue;                                       // a row of weight 0 is not there
        split_scatter16(hist + (labels[i] == cls ? BS_PLANE : 0), lrb_load16<AL>(x, total, whole, (unsigned long long)i * (unsigned long long)D, j0, D, true),
                        tid, (unsigned long long)wi);
    }
    __syncthreads();

    const unsigned inside = D - j0 >= SPLIT_TILE ? 0xffffu : (1u << (D - j0)) - 1u;      // every feature below D is a candidate
    BoostBest b = split_scan_tile<unsigned long long>(inside, j0, lane, wv, s_tot, [&](int f, unsigned long long (&nb)[4], unsigned long long (&pb)[4]) {
        const unsigned long long* const hn = hist + f * SPLIT_PITCH + lane * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) { pb[q] = hn[BS_PLANE + q]; nb[q] = hn[q] + pb[q]; }
    });
    if (split_block_best(s_best, tid, b)) {
        long long* const rec = tile_rec + (size_t)blockIdx.x * BS_REC;
        rec[0] = __double_as_longlong(b.s); rec[1] = b.j; rec[2] = b.v; rec[3] = b.vh;
        rec[4] = (long long)b.nL; rec[5] = (long long)b.pL; rec[6] = (long long)s_tot[0]; rec[7] = (long long)s_tot[1];
    }
}

// A wave per class: the best of its tiles' candidates, the totals from tile 0.
__global__ __launch_bounds__(SPLIT_THREADS) void boost_stump_reduce_kernel(const long long* __restrict__ tile_rec, int K, int tiles,
                                                                           long long* __restrict__ out, long long* __restrict__ score) {
    const int cls = (int)blockIdx.x * SPLIT_WAVES + (int)(threadIdx.x >> 6);
    if (cls >= K) return;                                            // wave-uniform
    split_reduce_tiles<unsigned long long>(tiles, threadIdx.x & 63, [&](int t) {
        const long long* const rec = tile_rec + ((size_t)t * (size_t)K + (size_t)cls) * BS_REC;
        return BoostBest{__longlong_as_double(rec[0]), (int)rec[1], (int)rec[2], (int)rec[3], (unsigned long long)rec[4], (unsigned long long)rec[5]};
    }, tile_rec + (size_t)cls * BS_REC + 6, out + (size_t)cls * 7, score + cls);
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int64_t cslgan_boost_stump_ws_bytes(int K, int D) {
    if (K < 2 || K > SPLIT_MAX_K || D < 1 || D > SPLIT_MAX_D) return 0;
    return (int64_t)K * ((D + SPLIT_TILE - 1) / SPLIT_TILE) * (int64_t)(BS_REC * sizeof(long long));
}

int cslgan_boost_stump_u8(const void* X, const int32_t* labels, const int32_t* weights, int64_t N, int D, int K, int64_t* out, int64_t* score,
                          void* ws, int64_t ws_bytes, void* stream) {
    CSLGAN_REQUIRE(X && labels && weights && out && score && ws, "boost_stump_u8: null argument");
    CSLGAN_REQUIRE(K >= 2 && K <= SPLIT_MAX_K, "boost_stump_u8: K=%d must lie in 2 .. %d", K, SPLIT_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= SPLIT_MAX_D, "boost_stump_u8: D=%d must lie in 1 .. %d", D, SPLIT_MAX_D);
    CSLGAN_REQUIRE(N >= 1 && N < SPLIT_MAX_N, "boost_stump_u8: N=%lld must lie in 1 .. 2^24 - 1", (long long)N);
    const int64_t need = cslgan_boost_stump_ws_bytes(K, D);
    CSLGAN_REQUIRE(ws_bytes >= need, "boost_stump_u8: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
    CSLGAN_REQUIRE(aligned16(X), "boost_stump_u8: X misaligned (16 bytes)");
    CSLGAN_REQUIRE(aligned_to(labels, 4) && aligned_to(weights, 4), "boost_stump_u8: int32 array misaligned (4 bytes)");
    CSLGAN_REQUIRE(aligned_to(out, 8) && aligned_to(score, 8) && aligned_to(ws, 8), "boost_stump_u8: out, score or workspace misaligned (8 bytes)");
    const int tiles = (D + SPLIT_TILE - 1) / SPLIT_TILE;
    hipStream_t st = (hipStream_t)stream;
    long long* const tile_rec = (long long*)ws;
    const dim3 grid((unsigned)(tiles * K)), block(SPLIT_THREADS);
    note_kernel("boost_stump_tile_kernel");
    if (D % 16 == 0)
        hipLaunchKernelGGL(boost_stump_tile_kernel<true>, grid, block, 0, st, (const unsigned char*)X, labels, weights, (long long)N, D, K, tile_rec);
    else
        hipLaunchKernelGGL(boost_stump_tile_kernel<false>, grid, block, 0, st, (const unsigned char*)X, labels, weights, (long long)N, D, K, tile_rec);
    if (int rc = check_launch("boost_stump_tile_kernel")) return rc;
    hipLaunchKernelGGL(boost_stump_reduce_kernel, dim3((unsigned)((K + SPLIT_WAVES - 1) / (SPLIT_WAVES))), block, 0, st, tile_rec, K, tiles,
                       (long long*)out, (long long*)score);
    return check_launch("boost_stump_reduce_kernel");
}

}  // extern "C"
