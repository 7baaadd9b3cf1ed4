// Decision trees on cache bytes (include/cslgan.h "decision trees"; csl_gan_amd.classify.Trees): the split search of
// one tree level — every open node of every tree in one launch — and the leaf numbers of test rows under fitted trees.
//
// cslgan_tree_best_split_u8 — tree_split_tile_kernel, then tree_split_reduce_kernel, on the frame of byte_split.h (the histograms in
// LDS, the scan, the one score routine, the tie rule and the reductions, shared with boost_kernels.hip).  What is the trees' own:
//   Rows: a workgroup owns one (segment, feature tile) pair: the rows of one open node, named by row indices that are range-checked.
//   The tiles of a segment are consecutive workgroups, so the 64-byte sectors that a row's neighbouring tiles share are fetched from
//   HBM once and served to the other three from L2.  A wider tile would fetch fewer partial sectors, but the histograms are what LDS
//   holds: 16 features x 256 bins x 8 bytes = 32 KiB (+ the pad) leaves four workgroups per CU of the 160 KiB; 64 features would
//   leave one.  A segment's weight row is optional; one that does not exist counts nothing.
//   Counters: one 64-bit LDS entry per (feature, byte) — n = sum w in bits 0 .. 31, p = sum w [label == class] in bits 32 .. 63 — so
//   a row costs ONE 64-bit LDS atomic per byte, not two.  The contract keeps sum w of a segment below 2^31: the low half never
//   carries into the high half and neither wraps, even when one bin holds the whole segment (p <= n).
//   Mask: a feature that the Philox mask of an rf node leaves out is scanned by nobody, and a tile without a candidate feature skips
//   its rows (tile 0 never does: it owns the node's totals n and p).
//   Record: a tile's score in a float64 array, (j, v, v_hi, nL, pL, n, p) as int32 behind it.
//
// cslgan_tree_apply_u8 — tree_apply_kernel: a thread per (tree, row) walks the flat node tables from the root; every index it reads
// is range-checked against the tree's node count and the walk is bounded by that count, so a malformed table ends in leaf -1, not
// in a stray read or an endless loop.
#include "byte_split.h"

namespace cslgan {

constexpr uint32_t TR_COUNTER_TAG = 0x74726565u;          // word 3 of every counter of the feature-mask stream ("tree")
constexpr unsigned long long TR_SEED_TAG = 0x7472656573706C74ull;      // xor-ed into the seed ("treesplt")
constexpr int TR_REC = 8;                // int32 words of a tile record: j, v, v_hi, nL, pL, n, p, unused

using TreeBest = SplitBest<unsigned>;

template <bool AL>
__global__ __launch_bounds__(SPLIT_THREADS) void tree_split_tile_kernel(
    const unsigned char* __restrict__ x, const int* __restrict__ labels, const int* __restrict__ weights, int n_wrows, long long N, int D,
    const int* __restrict__ rows, long long R, const int* __restrict__ seg_off, const int* __restrict__ seg_class, const int* __restrict__ seg_wrow,
    const int* __restrict__ seg_tree, const int* __restrict__ seg_node, unsigned mask_thr, uint32_t k0, uint32_t k1, int tiles,
    double* __restrict__ tile_score, int* __restrict__ tile_rec) {
    __shared__ unsigned long long hist[SPLIT_TILE * SPLIT_PITCH];
    __shared__ unsigned s_cand;
    __shared__ unsigned s_tot[2];
    __shared__ TreeBest s_best[SPLIT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int seg = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int j0 = tile * SPLIT_TILE;

    bool cand = false;
    if (tid < SPLIT_TILE && j0 + tid < D) {
        cand = true;
        if (mask_thr != 0u) {
            uint32_t w[4];
            philox4x32_10((uint32_t)(j0 + tid), (uint32_t)seg_node[seg], (uint32_t)seg_tree[seg], TR_COUNTER_TAG, k0, k1, w);
            cand = w[0] < mask_thr;
        }
    }
    const unsigned long long bal = __ballot(cand);
    if (tid == 0) s_cand = (unsigned)bal & 0xffffu;
    for (int i = tid; i < SPLIT_TILE * SPLIT_PITCH; i += SPLIT_THREADS) hist[i] = 0ull;
    __syncthreads();
    const unsigned candbits = s_cand;
    int* const rec = tile_rec + (size_t)blockIdx.x * TR_REC;
    if (candbits == 0u && tile != 0) {                               // uniform: nothing to find here, and the totals are tile 0's
        if (tid == 0) {
            tile_score[blockIdx.x] = -1.0;
            rec[0] = -1; rec[1] = -1; rec[2] = -1; rec[3] = 0; rec[4] = 0; rec[5] = 0; rec[6] = 0; rec[7] = 0;
        }
        return;
    }

    const int r0 = seg_off[seg] > 0 ? seg_off[seg] : 0;
    const int r1 = (long long)seg_off[seg + 1] < R ? seg_off[seg + 1] : (int)R;         // never a read outside rows
    const int cls = seg_class[seg];
    const int wrow = (weights && seg_wrow) ? seg_wrow[seg] : -1;
    const bool no_rows = wrow >= n_wrows;                            // a weight row that does not exist: the segment counts nothing
    const int* const wp = wrow >= 0 && !no_rows ? weights + (size_t)wrow * (size_t)N : nullptr;
    const unsigned long long total = (unsigned long long)N * (unsigned long long)D, whole = total & ~15ull;
    for (long long i = (long long)r0 + tid; i < r1 && !no_rows; i += SPLIT_THREADS) {
        const int r = rows[i];
        if (r < 0 || (long long)r >= N) continue;                    // never a read outside X, labels or the weight row
        const int wi = wp ? wp[r] : 1;
        if (wi <= 0) continue;
        const unsigned long long inc = (unsigned long long)(unsigned)wi | (labels[r] == cls ? (unsigned long long)(unsigned)wi << 32 : 0ull);
        split_scatter16(hist, lrb_load16<AL>(x, total, whole, (unsigned long long)r * (unsigned long long)D, j0, D, true), tid, inc);
    }
    __syncthreads();

    TreeBest b = split_scan_tile<unsigned>(candbits, j0, lane, wv, s_tot, [&](int f, unsigned (&nb)[4], unsigned (&pb)[4]) {
        const unsigned long long* const h = hist + f * SPLIT_PITCH + lane * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const unsigned long long e = h[q]; nb[q] = (unsigned)e; pb[q] = (unsigned)(e >> 32); }
    });
    if (split_block_best(s_best, tid, b)) {
        tile_score[blockIdx.x] = b.s;
        rec[0] = b.j; rec[1] = b.v; rec[2] = b.vh; rec[3] = (int)b.nL; rec[4] = (int)b.pL; rec[5] = (int)s_tot[0]; rec[6] = (int)s_tot[1]; rec[7] = 0;
    }
}

// A wave per segment: the best of its tiles' candidates, the totals from tile 0.
__global__ __launch_bounds__(SPLIT_THREADS) void tree_split_reduce_kernel(const double* __restrict__ tile_score, const int* __restrict__ tile_rec,
                                                                       long long S, int tiles, int* __restrict__ out, long long* __restrict__ score) {
    const long long seg = (long long)blockIdx.x * SPLIT_WAVES + (threadIdx.x >> 6);
    if (seg >= S) return;                                            // wave-uniform
    const size_t at0 = (size_t)seg * (size_t)tiles;
    split_reduce_tiles<unsigned>(tiles, threadIdx.x & 63, [&](int t) {
        const int* const rec = tile_rec + (at0 + (size_t)t) * TR_REC;
        return TreeBest{tile_score[at0 + (size_t)t], rec[0], rec[1], rec[2], (unsigned)rec[3], (unsigned)rec[4]};
    }, tile_rec + at0 * TR_REC + 5, out + seg * 7, score + seg);
}

__global__ __launch_bounds__(SPLIT_THREADS) void tree_apply_kernel(const unsigned char* __restrict__ x, long long M, int D, const int* __restrict__ feature,
                                                                const int* __restrict__ threshold, const int* __restrict__ child,
                                                                const int* __restrict__ tree_off, long long Q, int* __restrict__ leaf) {
    const long long row = (long long)blockIdx.x * SPLIT_THREADS + threadIdx.x;
    const int t = blockIdx.y;
    if (row >= M) return;
    const long long q0 = tree_off[t], q1 = tree_off[t + 1];
    int result = -1;
    if (q0 >= 0 && q1 <= Q && q0 < q1) {
        const int nq = (int)(q1 - q0);
        int node = 0;
        for (int step = 0; step < nq; ++step) {                      // a walk visits a node at most once: children lie behind their parent
            const int f = feature[q0 + node];
            if (f < 0) { result = node; break; }
            const int c = child[q0 + node];
            if (f >= D || c <= node || c + 1 >= nq) break;           // a malformed table: leaf -1
            const int b = (int)x[(size_t)row * (size_t)D + (size_t)f];
            node = c + (b > threshold[q0 + node] ? 1 : 0);
        }
    }
    leaf[(size_t)t * (size_t)M + (size_t)row] = result;
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int64_t cslgan_tree_best_split_ws_bytes(int64_t S, int D) {
    if (S < 1 || D < 1 || D > SPLIT_MAX_D) return 0;
    const int64_t tiles = (D + SPLIT_TILE - 1) / SPLIT_TILE;
    if (S > ((1ll << 31) - 1) / tiles) return 0;
    return S * tiles * (int64_t)(sizeof(double) + TR_REC * sizeof(int));
}

int cslgan_tree_best_split_u8(const void* X, const int32_t* labels, const int32_t* weights, int n_wrows, int64_t N, int D, int K, const int32_t* rows,
                              int64_t R, const int32_t* seg_off, const int32_t* seg_class, const int32_t* seg_wrow, const int32_t* seg_tree,
                              const int32_t* seg_node, int64_t S, uint32_t mask_thr, uint64_t seed, int32_t* out, int64_t* score, void* ws,
                              int64_t ws_bytes, void* stream) {
    CSLGAN_REQUIRE(X && labels && rows && seg_off && seg_class && out && score && ws, "tree_best_split_u8: null argument");
    CSLGAN_REQUIRE(K >= 2 && K <= SPLIT_MAX_K, "tree_best_split_u8: K=%d must lie in 2 .. %d", K, SPLIT_MAX_K);
    CSLGAN_REQUIRE(D >= 1 && D <= SPLIT_MAX_D, "tree_best_split_u8: D=%d must lie in 1 .. %d", D, SPLIT_MAX_D);
    CSLGAN_REQUIRE(N >= 1 && N < SPLIT_MAX_N, "tree_best_split_u8: N=%lld must lie in 1 .. 2^24 - 1", (long long)N);
    CSLGAN_REQUIRE(R >= 0 && R < (1ll << 31), "tree_best_split_u8: R=%lld row indices out of range", (long long)R);
    const int64_t need = cslgan_tree_best_split_ws_bytes(S, D);
    CSLGAN_REQUIRE(need > 0, "tree_best_split_u8: S=%lld segments of %d features: need 1 <= S and S * ceil(D / 16) < 2^31", (long long)S, D);
    CSLGAN_REQUIRE(ws_bytes >= need, "tree_best_split_u8: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
    CSLGAN_REQUIRE(!weights || (seg_wrow && n_wrows >= 1), "tree_best_split_u8: weights need seg_wrow and n_wrows >= 1, got n_wrows=%d", n_wrows);
    CSLGAN_REQUIRE(mask_thr == 0u || (seg_tree && seg_node), "tree_best_split_u8: a feature mask needs the keys seg_tree and seg_node");
    CSLGAN_REQUIRE(aligned16(X), "tree_best_split_u8: X misaligned (16 bytes)");
    CSLGAN_REQUIRE(aligned_to(labels, 4) && aligned_to(weights, 4) && aligned_to(rows, 4) && aligned_to(seg_off, 4) && aligned_to(seg_class, 4) &&
                       aligned_to(seg_wrow, 4) && aligned_to(seg_tree, 4) && aligned_to(seg_node, 4) && aligned_to(out, 4),
                   "tree_best_split_u8: int32 array misaligned (4 bytes)");
    CSLGAN_REQUIRE(aligned_to(score, 8) && aligned_to(ws, 8), "tree_best_split_u8: score or workspace misaligned (8 bytes)");
    const int tiles = (D + SPLIT_TILE - 1) / SPLIT_TILE;
    hipStream_t st = (hipStream_t)stream;
    double* const tile_score = (double*)ws;
    int* const tile_rec = (int*)(tile_score + (size_t)S * (size_t)tiles);
    const unsigned long long key = (unsigned long long)seed ^ TR_SEED_TAG;
    const dim3 grid((unsigned)(S * tiles)), block(SPLIT_THREADS);
    note_kernel("tree_split_tile_kernel");
    if (D % 16 == 0)
        hipLaunchKernelGGL(tree_split_tile_kernel<true>, grid, block, 0, st, (const unsigned char*)X, labels, weights, n_wrows, (long long)N, D, rows, (long long)R, seg_off,
                           seg_class, seg_wrow, seg_tree, seg_node, mask_thr, (uint32_t)key, (uint32_t)(key >> 32), tiles, tile_score, tile_rec);
    else
        hipLaunchKernelGGL(tree_split_tile_kernel<false>, grid, block, 0, st, (const unsigned char*)X, labels, weights, n_wrows, (long long)N, D, rows, (long long)R, seg_off,
                           seg_class, seg_wrow, seg_tree, seg_node, mask_thr, (uint32_t)key, (uint32_t)(key >> 32), tiles, tile_score, tile_rec);
    if (int rc = check_launch("tree_split_tile_kernel")) return rc;
    hipLaunchKernelGGL(tree_split_reduce_kernel, dim3((unsigned)((S + SPLIT_WAVES - 1) / SPLIT_WAVES)), block, 0, st, tile_score, tile_rec,
                       (long long)S, tiles, out, (long long*)score);
    return check_launch("tree_split_reduce_kernel");
}

int cslgan_tree_apply_u8(const void* Xtest, int64_t M, int D, const int32_t* feature, const int32_t* threshold, const int32_t* child,
                         const int32_t* tree_off, int T, int64_t Q, int32_t* leaf, void* stream) {
    CSLGAN_REQUIRE(Xtest && feature && threshold && child && tree_off && leaf, "tree_apply_u8: null argument");
    CSLGAN_REQUIRE(D >= 1 && D <= SPLIT_MAX_D, "tree_apply_u8: D=%d must lie in 1 .. %d", D, SPLIT_MAX_D);
    CSLGAN_REQUIRE(M >= 1 && M < (1ll << 31), "tree_apply_u8: M=%lld out of range", (long long)M);
    CSLGAN_REQUIRE(T >= 1 && T <= 65535, "tree_apply_u8: T=%d trees must lie in 1 .. 65535", T);
    CSLGAN_REQUIRE(Q >= T && Q < (1ll << 31), "tree_apply_u8: Q=%lld nodes for %d trees: every tree has a root", (long long)Q, T);
    CSLGAN_REQUIRE(aligned_to(feature, 4) && aligned_to(threshold, 4) && aligned_to(child, 4) && aligned_to(tree_off, 4) && aligned_to(leaf, 4),
                   "tree_apply_u8: int32 array misaligned (4 bytes)");
    note_kernel("tree_apply_kernel");
    hipLaunchKernelGGL(tree_apply_kernel, dim3((unsigned)((M + SPLIT_THREADS - 1) / SPLIT_THREADS), (unsigned)T), dim3(SPLIT_THREADS), 0, (hipStream_t)stream,
                       (const unsigned char*)Xtest, (long long)M, D, feature, threshold, child, tree_off, (long long)Q, leaf);
    return check_launch("tree_apply_kernel");
}

}  // extern "C"
