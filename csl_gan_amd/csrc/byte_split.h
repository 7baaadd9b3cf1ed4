// The split search on cache bytes that tree_kernels.hip (counts C = unsigned) and boost_kernels.hip (C = unsigned long long) share:
// a workgroup of 256 threads owns 16 consecutive features — one 16-byte load per row — and builds their 256-bin histograms in LDS;
// a wave then scans a feature; the tile's best candidate goes to the workspace and a wave per segment or class reduces the tiles.
//   Banks: a feature's 256 entries are followed by one entry of padding (pitch 257 entries = 514 dwords), and lane l starts at
//   feature l % 16 and walks the 16 features round from there.  Lanes that all hold the same byte (the constant background of an
//   image) then hit 16 different addresses on 16 different bank pairs per instruction instead of one address 64 times.
//   Scan: lane l owns the bins 4 l .. 4 l + 3; a wave prefix sum gives (nL, pL) at every bin and a suffix minimum the next larger
//   byte present (v_hi).
//   Score: (a a) / fl(nL) + (c c) / fl(nR) with a = fl(pL), c = fl(p - pL).  Every integer is below 2^53, so the four conversions are
//   exact; the five operations are __dmul_rn, __ddiv_rn, __dadd_rn — each rounded once, and no product feeds an addition, so nothing
//   can be contracted.  For counts below 2^32 this is also fl(pL pL as an exact 64-bit integer) / fl(nL) + ..., the form in which
//   the trees were first defined: the conversion of the exact integer product and the multiplication of the exact factors both
//   round the same real number once, to nearest even.
//   Ties: the largest score, then the smallest feature, then the smallest byte, at every level of the reduction.
// What a caller keeps: which rows it counts and with which weight, the layout of a bin's (n, p), and its tile record.
#pragma once
#include "ovr_rows.h"

namespace cslgan {

constexpr int SPLIT_MAX_K = 16;
constexpr int SPLIT_MAX_D = 65536;
constexpr long long SPLIT_MAX_N = 1ll << 24;
constexpr int SPLIT_TILE = 16;           // features of a workgroup: one 16-byte load per row
constexpr int SPLIT_THREADS = 256;
constexpr int SPLIT_WAVES = SPLIT_THREADS / 64;
constexpr int SPLIT_PITCH = 257;         // entries of a feature's histogram: 256 bins and one of padding

template <typename C>
struct SplitBest {
    double s;                            // -1: no candidate (a score is >= 0)
    int j, v, vh;
    C nL, pL;
};

template <typename C>
__device__ __forceinline__ SplitBest<C> split_none() { return {-1.0, -1, -1, -1, (C)0, (C)0}; }

// a before b: the larger score, then the smaller feature, then the smaller byte
template <typename C>
__device__ __forceinline__ bool split_better(const SplitBest<C>& a, const SplitBest<C>& b) {
    return a.s > b.s || (a.s == b.s && (a.j < b.j || (a.j == b.j && a.v < b.v)));
}

template <typename C>
__device__ __forceinline__ void split_wave_best(SplitBest<C>& b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        SplitBest<C> t;
        t.s = __shfl_xor(b.s, o, 64);
        t.j = __shfl_xor(b.j, o, 64);
        t.v = __shfl_xor(b.v, o, 64);
        t.vh = __shfl_xor(b.vh, o, 64);
        t.nL = __shfl_xor(b.nL, o, 64);
        t.pL = __shfl_xor(b.pL, o, 64);
        if (split_better(t, b)) b = t;
    }
}

template <typename C>
__device__ __forceinline__ double split_score(C pL, C nL, C pR, C nR) {
    const double a = (double)pL, c = (double)pR;
    return __dadd_rn(__ddiv_rn(__dmul_rn(a, a), (double)nL), __ddiv_rn(__dmul_rn(c, c), (double)nR));
}

// One row's sixteen bytes v into sixteen histograms a pitch apart from h on: one 64-bit LDS atomic of `inc` per byte.  The bytes of
// the features from D on are zeros; nobody scans them.  v by value: taken by reference, the word select below compiled into a branch
// per atomic and the tile kernels took 1.6 to 2 times as long (profiles/split_frame_bench.txt).
__device__ __forceinline__ void split_scatter16(unsigned long long* h, const u32x4 v, int tid, unsigned long long inc) {
#pragma unroll
    for (int e = 0; e < SPLIT_TILE; ++e) {
        const int f = (e + tid) & (SPLIT_TILE - 1);
        const unsigned word = (f >> 2) == 0 ? v.x : ((f >> 2) == 1 ? v.y : ((f >> 2) == 2 ? v.z : v.w));
        atomicAdd(&h[f * SPLIT_PITCH + (int)((word >> (8 * (f & 3))) & 0xffu)], inc);
    }
}

// A wave scans feature j from the counts (nb, pb) of the four bins that each lane holds: the totals (ntot, ptot) in every lane and,
// when the feature is a candidate (wave-uniform), the wave's best split of it in every lane; else none.
template <typename C>
__device__ __forceinline__ SplitBest<C> split_scan_feature(const C (&nb)[4], const C (&pb)[4], int lane, int j, bool is_cand, C& ntot, C& ptot) {
    const C sn = nb[0] + nb[1] + nb[2] + nb[3], sp = pb[0] + pb[1] + pb[2] + pb[3];
    C cn = sn, cp = sp;                                              // inclusive prefix sums over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const C a = __shfl_up(cn, o, 64), b = __shfl_up(cp, o, 64);
        if (lane >= o) { cn += a; cp += b; }
    }
    ntot = __shfl(cn, 63, 64); ptot = __shfl(cp, 63, 64);
    SplitBest<C> best = split_none<C>();
    if (!is_cand) return best;                                       // summed for its totals only
    int first = 256;                                                 // the smallest byte present among this lane's four
#pragma unroll
    for (int q = 3; q >= 0; --q) if (nb[q]) first = lane * 4 + q;
    int sfx = first;                                                 // inclusive suffix minimum over the lanes
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
    C bn = cn - sn, bp = cp - sp;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bn += nb[q]; bp += pb[q];
        if (nb[q] && bn < ntot) {                                    // the byte is present and a row lies to its right
            const double s = split_score(bp, bn, ptot - bp, ntot - bn);
            if (s > best.s) { best.s = s; best.j = j; best.v = lane * 4 + q; best.vh = hi[q]; best.nL = bn; best.pL = bp; }
        }
    }
    split_wave_best(best);
    return best;
}

// The waves scan the tile's features f = 0 .. 15 (global j0 + f) whose bit of candbits is set, and feature 0 in any case for the
// totals, which go to s_tot[0 .. 1].  bins(f, nb, pb) fills the lane's four bin counts of feature f.  The wave's best is returned.
template <typename C, typename Bins>
__device__ __forceinline__ SplitBest<C> split_scan_tile(unsigned candbits, int j0, int lane, int wv, C* s_tot, Bins bins) {
    SplitBest<C> wbest = split_none<C>();
    for (int f = wv; f < SPLIT_TILE; f += SPLIT_WAVES) {             // wave-uniform
        const bool is_cand = (candbits >> f) & 1u;
        if (!is_cand && f != 0) continue;
        C nb[4], pb[4], ntot, ptot;
        bins(f, nb, pb);
        const SplitBest<C> best = split_scan_feature(nb, pb, lane, j0 + f, is_cand, ntot, ptot);
        if (f == 0 && lane == 0) { s_tot[0] = ntot; s_tot[1] = ptot; }
        if (split_better(best, wbest)) wbest = best;
    }
    return wbest;
}

// The waves' bests to the workgroup's: true in thread 0 alone, whose b then holds it (and s_tot is visible to it).
template <typename C>
__device__ __forceinline__ bool split_block_best(SplitBest<C>* s_best, int tid, SplitBest<C>& b) {
    if ((tid & 63) == 0) s_best[tid >> 6] = b;
    __syncthreads();
    if (tid != 0) return false;
    b = s_best[0];
    for (int w = 1; w < SPLIT_WAVES; ++w)
        if (split_better(s_best[w], b)) b = s_best[w];
    return true;
}

// A wave reduces the `tiles` records of one segment or class — load(t) gives tile t's — and lane 0 writes the seven outputs and the
// score bits: (-1, -1, -1, 0, 0) and score 0 when no tile found a candidate; tot points at tile 0's totals (n, p).
template <typename C, typename O, typename Load>
__device__ __forceinline__ void split_reduce_tiles(int tiles, int lane, Load load, const O* tot, O* o, long long* score) {
    SplitBest<C> best = split_none<C>();
    for (int t = lane; t < tiles; t += 64) {
        const SplitBest<C> r = load(t);
        if (split_better(r, best)) best = r;
    }
    split_wave_best(best);
    if (lane == 0) {
        const bool found = best.s >= 0.0 && best.j >= 0;
        o[0] = found ? best.j : -1; o[1] = found ? best.v : -1; o[2] = found ? best.vh : -1;
        o[3] = found ? (O)best.nL : (O)0; o[4] = found ? (O)best.pL : (O)0; o[5] = tot[0]; o[6] = tot[1];
        *score = found ? __double_as_longlong(best.s) : 0ll;
    }
}

}  // namespace cslgan
