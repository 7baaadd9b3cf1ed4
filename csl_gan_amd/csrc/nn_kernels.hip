// Nearest-neighbour audit kernels for gfx950 (csl_gan_amd.neighbours; DESIGN.md §6g, §6h, include/cslgan.h "Nearest-neighbour audit").
//
// Exact integer arithmetic on uint8 image caches: for every query row the smallest squared Euclidean distance to a reference row
// and the index of that row, as one uint64 key (d2 << 32 | index).  The bytes are shifted to int8 (x - 128) once by
// nn_prepare_u8_kernel, which also leaves |row|^2; nn_min_i8_kernel is then an nq x nr x Dp dot-product GEMM on the int8 matrix
// instruction whose epilogue forms d2 = |a|^2 + |b|^2 - 2 a.b and keeps a running minimum per row: the nq x nr matrix never
// reaches memory.  nn_count_i8_kernel (csl_gan_amd.blackbox) runs the same tile loop with a counting epilogue: per row
// the number of reference rows with d2 <= each of up to four thresholds.
#include "common.h"
#include "device_prims.h"
#include "nn_tile.h"

namespace cslgan {

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- prepare: uint8 [rows, D] -> int8 [rows, Dp] (x - 128, zero padding) and |row|^2 ------------------------------------------
// One wave per row, one 16-byte store per lane and step.  A row starts at x + row * D, which is 16-byte aligned only when D is a
// multiple of 16: a chunk is assembled from the two ALIGNED 16-byte words that hold it (v_alignbyte), so every access is 16 bytes
// wide and aligned whatever D is.  Words that reach beyond the last byte of x are never touched: those chunks read byte by byte.
__device__ __forceinline__ u32x4 nn_shift_bytes(const u32x4& lo, const u32x4& hi, int s) {
    const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const int ds = s >> 2, bs = s & 3;
    u32x4 o;
    // ds is uniform over the wave (one row): four straight-line variants keep w[] in registers
#define NN_PICK(d)                                                                                         \
    o.x = __builtin_amdgcn_alignbyte(w[d + 1], w[d], bs); o.y = __builtin_amdgcn_alignbyte(w[d + 2], w[d + 1], bs); \
    o.z = __builtin_amdgcn_alignbyte(w[d + 3], w[d + 2], bs); o.w = __builtin_amdgcn_alignbyte(w[d + 4], w[d + 3], bs);
    if (ds == 0) { NN_PICK(0) } else if (ds == 1) { NN_PICK(1) } else if (ds == 2) { NN_PICK(2) } else { NN_PICK(3) }
#undef NN_PICK
    return o;
}

__device__ __forceinline__ int nn_sq4(unsigned v) {           // sum of the squares of the four int8 of v
    const int a = (int)(signed char)(v & 0xffu), b = (int)(signed char)((v >> 8) & 0xffu), c = (int)(signed char)((v >> 16) & 0xffu),
              d = (int)(signed char)(v >> 24);
    return a * a + b * b + c * c + d * d;
}

__global__ __launch_bounds__(NN_THREADS) void nn_prepare_u8_kernel(const unsigned char* __restrict__ x, long long rows, int D, int Dp,
                                                                   signed char* __restrict__ xs, int* __restrict__ sqnorm) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (NN_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // whole waves leave: no barrier follows
    const unsigned long long total = (unsigned long long)rows * (unsigned long long)D;      // bytes of x
    const unsigned long long start = (unsigned long long)row * (unsigned long long)D;       // first byte of this row
    const int s = (int)(start & 15u);                          // x is 16-byte aligned (checked by the host)
    const unsigned long long start_al = start - (unsigned long long)s;
    const unsigned long long whole = total & ~15ull;           // the aligned 16-byte words below this offset lie inside x
    u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(xs + row * (long long)Dp);
    int sq = 0;
    for (int c = lane; c < Dp / 16; c += WAVE) {
        const int valid = D - 16 * c;                          // bytes of this chunk that exist in the row (<= 0: padding only)
        u32x4 v = {0u, 0u, 0u, 0u};
        if (valid > 0) {
            const unsigned long long g = start_al + 16ull * (unsigned long long)c;          // aligned; the chunk is bytes g + s .. g + s + 15
            if (g + 32ull <= whole) {
                const u32x4 lo = *reinterpret_cast<const u32x4*>(x + g);
                const u32x4 hi = *reinterpret_cast<const u32x4*>(x + g + 16);
                v = nn_shift_bytes(lo, hi, s);
            } else {                                           // the last words of x: byte by byte, nothing beyond total is read
                unsigned b[4] = {0u, 0u, 0u, 0u};
                for (int j = 0; j < 16; ++j) {
                    const unsigned long long a = g + (unsigned long long)(s + j);
                    const unsigned byte = a < total ? (unsigned)x[a] : 0u;
                    b[j >> 2] |= byte << (8 * (j & 3));
                }
                v.x = b[0]; v.y = b[1]; v.z = b[2]; v.w = b[3];
            }
            v ^= 0x80808080u;                                  // byte - 128 as int8
            if (valid < 16) {                                  // zero the bytes past the row's end (they hold the next row or nothing)
                unsigned m[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int nb = valid - 4 * j;              // valid bytes of dword j
                    m[j] = nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u));
                }
                v.x &= m[0]; v.y &= m[1]; v.z &= m[2]; v.w &= m[3];
            }
            sq += nn_sq4(v.x) + nn_sq4(v.y) + nn_sq4(v.z) + nn_sq4(v.w);
        }
        dst[c] = v;
    }
    sq = wave_sum_i32(sq);                                     // <= 2^14 D <= 2^30
    if (lane == 0) sqnorm[row] = sq;
}

// ---- the search ------------------------------------------------------------------------------------------------------------------
// Epilogue: key = d2 << 32 | index, running minimum per row in registers.

__global__ __launch_bounds__(NN_THREADS) void nn_min_i8_kernel(const signed char* __restrict__ q, const int* __restrict__ qn, int nq,
                                                               const signed char* __restrict__ r, const int* __restrict__ rn, int nr, int Dp,
                                                               uint32_t index_base, int tiles_per, int n_col_tiles,
                                                               unsigned long long* __restrict__ best) {
    __shared__ unsigned long long red[2][NN_TM];

    unsigned long long bk[2][16];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) bk[mt][i] = NN_NONE;
    nn_tile_loop(q, qn, nq, r, rn, nr, Dp, tiles_per, n_col_tiles, NNNoColumn(), [&](int mt, int i, bool live, long long col, uint32_t d2) {
        const uint32_t idx = index_base + (uint32_t)col;
        const unsigned long long key = live ? (((unsigned long long)d2 << 32) | (unsigned long long)idx) : NN_NONE;
        bk[mt][i] = key < bk[mt][i] ? key : bk[mt][i];
    });

    // per-row minimum over the 32 lanes that share a row, then over the two waves of a row half, then ONE atomicMin per row
    const int tid = threadIdx.x;
    const NNLane ln(tid);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    const int rows_here = (int)(nq - row0 < NN_TM ? nq - row0 : NN_TM);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            unsigned long long v = bk[mt][i];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                const unsigned long long u = __shfl_xor(v, o, 64);
                v = u < v ? u : v;
            }
            if (ln.l31 == 0) red[ln.wn][ln.row(mt, i)] = v;
        }
    __syncthreads();
    if (tid < rows_here) {
        const unsigned long long v0 = red[0][tid], v1 = red[1][tid];
        const unsigned long long v = v0 < v1 ? v0 : v1;
        if (v != NN_NONE) atomicMin(&best[row0 + tid], v);
    }
}

// ---- the count ---------------------------------------------------------------------------------------------------------------------
// counts[q][j] += #{r : d2(q, r) <= thr[j]}, compared as unsigned values.  The four running counters of a row are the four bytes of
// ONE register: a lane meets two columns per row and tile, so a byte grows by at most 2 per tile and holds NN_COUNT_TILES tiles
// (the host caps tiles_per there); no byte ever carries into its neighbour.  A column past nr adds nothing, whatever its bytes
// are (zero padding has d2 = |a|^2, which a threshold may well reach).  All four compares always run: a threshold past n_thr is
// zero on entry and its byte is never written out.
constexpr int NN_COUNT_TILES = 127;                            // 2 * 127 = 254 <= 255
constexpr int NN_MAX_THR = 4;

struct NNThresholds { uint32_t t[NN_MAX_THR]; };

__global__ __launch_bounds__(NN_THREADS) void nn_count_i8_kernel(const signed char* __restrict__ q, const int* __restrict__ qn, int nq,
                                                                 const signed char* __restrict__ r, const int* __restrict__ rn, int nr, int Dp,
                                                                 NNThresholds thr, int n_thr, int tiles_per, int n_col_tiles,
                                                                 uint32_t* __restrict__ counts) {
    __shared__ uint32_t red[2][NN_TM][2];                      // [column half][row][thresholds 0 2 | 1 3 as 16-bit pairs]

    uint32_t cnt[2][16];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) cnt[mt][i] = 0u;
    nn_tile_loop(q, qn, nq, r, rn, nr, Dp, tiles_per, n_col_tiles, NNNoColumn(), [&](int mt, int i, bool live, long long, uint32_t d2) {
        const uint32_t one = live ? 1u : 0u;                   // the column mask, applied to every increment
        uint32_t inc = 0u;
#pragma unroll
        for (int j = 0; j < NN_MAX_THR; ++j) inc |= (d2 <= thr.t[j] ? one : 0u) << (8 * j);
        cnt[mt][i] += inc;
    });

    // unpack once: the bytes 0 2 and 1 3 of a register as two pairs of 16-bit fields, each summed over the 32 lanes that share a
    // row (32 * 254 < 2^16), then over the two waves of a row half through LDS, then ONE atomicAdd per (row, threshold)
    const int tid = threadIdx.x;
    const NNLane ln(tid);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    const int rows_here = (int)(nq - row0 < NN_TM ? nq - row0 : NN_TM);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t even = cnt[mt][i] & 0x00ff00ffu, odd = (cnt[mt][i] >> 8) & 0x00ff00ffu;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                even += (uint32_t)__shfl_xor((int)even, o, 64);
                odd += (uint32_t)__shfl_xor((int)odd, o, 64);
            }
            if (ln.l31 == 0) {
                red[ln.wn][ln.row(mt, i)][0] = even;
                red[ln.wn][ln.row(mt, i)][1] = odd;
            }
        }
    __syncthreads();
    if (tid < rows_here) {                                     // rows past nq issue nothing
        const uint32_t even = red[0][tid][0] + red[1][tid][0], odd = red[0][tid][1] + red[1][tid][1];       // 64 * 254 < 2^16 per field
        const uint32_t c[NN_MAX_THR] = {even & 0xffffu, odd & 0xffffu, even >> 16, odd >> 16};
#pragma unroll
        for (int j = 0; j < NN_MAX_THR; ++j)
            if (j < n_thr && c[j] != 0u) atomicAdd(&counts[(row0 + tid) * n_thr + j], c[j]);
    }
}

// ---- the k smallest keys (csl_gan_amd.manifold) -----------------------------------------------------------------------
// Per row the k <= 8 smallest keys over the live columns, minus the one column whose index is the row's own (self search).  A
// wave keeps ONE uint32 per row in LDS: the d2 of the k-th key that it holds for the row so far (seeded with the k-th d2 of the
// in/out `best`, which no later key above it can displace, and rewritten only once the list is full; the bound only falls, so
// a stale read admits too much, never too little — the write by lane k - 1 and the later reads by the other lanes of the wave
// are ordered by program order within the wave alone, no fence, and correctness does not rest on it: either value is a valid
// bound).  A candidate above the bound costs one LDS read and one compare.  The others are taken one at a time by the whole
// wave: a ballot, then a uniform loop over its set bits that inserts the key into the WAVE's own sorted list of the row in LDS —
// lane j < k holds entry j, the position is a ballot, the shift a lane shuffle, so a lane reads and writes only its own LDS word
// and no order between lanes is assumed.  Nothing waits for another wave.  After the last tile the two waves of a row merge
// their lists and the workgroup writes k keys per row to its own slice of the workspace; every slice is written in full, so the
// workspace needs no clearing.
constexpr int NN_MAX_K = 8;

// (amdgpu_waves_per_eu: the allocator otherwise stops a few registers above the two-waves-per-SIMD budget of the other kernels)
__global__ __launch_bounds__(NN_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void nn_kth_i8_kernel(
    const signed char* __restrict__ q, const int* __restrict__ qn, int nq, const signed char* __restrict__ r, const int* __restrict__ rn, int nr,
    int Dp, uint32_t index_base, long long self_first, int k, int tiles_per, int n_col_tiles, const unsigned long long* __restrict__ best,
    unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long lists[2][NN_TM][NN_MAX_K];   // [column half = wave of the row][row][entry], sorted ascending
    __shared__ uint32_t bound[2][NN_TM];                       // [wave of the row][row]: d2 of the k-th entry of its list, seeded from best

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const NNLane ln(tid);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    const int rows_here = (int)(nq - row0 < NN_TM ? nq - row0 : NN_TM);
    for (int e = tid; e < 2 * NN_TM * NN_MAX_K; e += NN_THREADS) (&lists[0][0][0])[e] = NN_NONE;
    // a row past nq is never written out: bound 0 keeps (nearly) everything of it off the insert path
    bound[tid >> 7][tid & 127] = (tid & 127) < rows_here ? (uint32_t)(best[(row0 + (tid & 127)) * k + (k - 1)] >> 32) : 0u;
    // the column that row row0 + t must skip has index_base + col = self_first + row0 + t; without a self search no column has
    const long long self0 = self_first < 0 ? (1ll << 62) : self_first + row0;

    nn_tile_loop(q, qn, nq, r, rn, nr, Dp, tiles_per, n_col_tiles, NNNoColumn(), [&](int mt, int i, bool live, long long col, uint32_t d2) {
        const uint32_t idx = index_base + (uint32_t)col;
        const bool own = (long long)index_base + col - self0 == (long long)ln.row(mt, i);
        unsigned long long m = __ballot(live && !own && d2 <= bound[ln.wn][ln.row(mt, i)]);
        while (m != 0ull) {                                    // uniform over the wave
            const int src = __builtin_ctzll(m);
            m &= m - 1ull;
            const unsigned long long key = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)d2, src) << 32) |
                                           (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)idx, src);
            const int srow = ln.wm * 64 + mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * (src >> 5);        // ln.row(mt, i) of lane src
            unsigned long long* lst = &lists[ln.wn][srow][0];
            const unsigned long long cur = lane < k ? lst[lane] : NN_NONE;
            const int pos = __popcll(__ballot(cur < key));     // entries below the key: a prefix of the sorted list
            if (pos < k) {
                const unsigned long long up = __shfl_up(cur, 1, 64);
                const unsigned long long nv = lane < pos ? cur : (lane == pos ? key : up);
                if (lane >= pos && lane < k) lst[lane] = nv;
                // while the list is not full its k-th entry is all-ones: the seed stays, so the bound only ever falls
                if (lane == k - 1 && nv != NN_NONE) bound[ln.wn][srow] = (uint32_t)(nv >> 32);
            }
        }
    });

    // the loop ended behind a barrier: merge the two sorted lists of a row, k steps, and write the row's slice
    if (tid < rows_here) {
        unsigned long long* out = partial + ((long long)blockIdx.y * nq + row0 + tid) * k;
        int ia = 0, ib = 0;
        for (int j = 0; j < k; ++j) {
            const unsigned long long a = lists[0][tid][ia], b = lists[1][tid][ib];     // ia, ib <= j < k <= NN_MAX_K
            const bool ta = a <= b;
            out[j] = ta ? a : b;
            ia += ta ? 1 : 0;
            ib += ta ? 0 : 1;
        }
    }
}

// best[row] = the k smallest of best[row] and the n_ranges slices of the row, ascending.  One thread per row; the running list is
// eight registers (entries past k start all-ones and only ever take keys that k larger ones displaced), inserted into by an
// unrolled compare-and-shift from the top.
__global__ __launch_bounds__(NN_THREADS) void nn_kth_merge_kernel(const unsigned long long* __restrict__ partial, int n_ranges, int nq, int k,
                                                                  unsigned long long* __restrict__ best) {
    const long long row = (long long)blockIdx.x * NN_THREADS + threadIdx.x;
    if (row >= nq) return;
    unsigned long long cur[NN_MAX_K];
#pragma unroll
    for (int t = 0; t < NN_MAX_K; ++t) cur[t] = t < k ? best[row * k + t] : NN_NONE;
    unsigned long long kth = best[row * k + (k - 1)];           // cur[k - 1]: what a key must beat to enter
    for (int g = 0; g < n_ranges; ++g) {
        const unsigned long long* src = partial + ((long long)g * nq + row) * k;
        for (int j = 0; j < k; ++j) {
            const unsigned long long key = src[j];
            if (key >= kth) break;                             // the slice is sorted: nothing after it gets in either
#pragma unroll
            for (int t = NN_MAX_K - 1; t >= 0; --t)
                if (key < cur[t]) {
                    if (t + 1 < NN_MAX_K) cur[t + 1] = cur[t];
                    cur[t] = key;
                }
#pragma unroll
            for (int t = 0; t < NN_MAX_K; ++t) kth = t == k - 1 ? cur[t] : kth;
        }
    }
#pragma unroll
    for (int t = 0; t < NN_MAX_K; ++t)
        if (t < k) best[row * k + t] = cur[t];
}

// ---- the count inside per-column radii ------------------------------------------------------------------------------
// counts[q] += #{r : d2(q, r) <= radius[r]}, compared as unsigned values: the counting epilogue with the threshold of the column,
// read once per column and tile beside rn[col], and one plain uint32 counter per row and
// lane, so no cap on the tiles of a workgroup.  A column past nr adds nothing, whatever radius would lie behind it.
__global__ __launch_bounds__(NN_THREADS) void nn_count_radius_i8_kernel(const signed char* __restrict__ q, const int* __restrict__ qn, int nq,
                                                                        const signed char* __restrict__ r, const int* __restrict__ rn, int nr,
                                                                        int Dp, const uint32_t* __restrict__ radius, int tiles_per,
                                                                        int n_col_tiles, uint32_t* __restrict__ counts) {
    __shared__ uint32_t red[2][NN_TM];

    uint32_t cnt[2][16];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) cnt[mt][i] = 0u;
    uint32_t rad = 0u;                                         // of the column whose elements come next
    nn_tile_loop(q, qn, nq, r, rn, nr, Dp, tiles_per, n_col_tiles, [&](bool live, long long col) { rad = live ? radius[col] : 0u; },
                 [&](int mt, int i, bool live, long long, uint32_t d2) {
                     cnt[mt][i] += (live && d2 <= rad) ? 1u : 0u;      // the column mask, applied to every increment
                 });

    const int tid = threadIdx.x;
    const NNLane ln(tid);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    const int rows_here = (int)(nq - row0 < NN_TM ? nq - row0 : NN_TM);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t v = cnt[mt][i];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
            if (ln.l31 == 0) red[ln.wn][ln.row(mt, i)] = v;
        }
    __syncthreads();
    if (tid < rows_here) {                                     // rows past nq issue nothing
        const uint32_t c = red[0][tid] + red[1][tid];
        if (c != 0u) atomicAdd(&counts[row0 + tid], c);
    }
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_nn_padded_dim(int D) {
    if (D < 1 || D > NN_MAX_D) return 0;
    return (D + NN_KT - 1) / NN_KT * NN_KT;
}

int cslgan_nn_prepare_u8(const void* x, int64_t rows, int D, int Dp, void* xs, int32_t* sqnorm, void* stream) {
    CSLGAN_REQUIRE(x && xs && sqnorm, "nn_prepare_u8: null argument");
    CSLGAN_REQUIRE(D >= 1 && D <= NN_MAX_D, "nn_prepare_u8: D=%d must lie in 1 .. %d", D, NN_MAX_D);
    CSLGAN_REQUIRE(Dp == cslgan_nn_padded_dim(D), "nn_prepare_u8: Dp=%d is not the padded width %d of D=%d", Dp, cslgan_nn_padded_dim(D), D);
    CSLGAN_REQUIRE(rows >= 1 && rows < (1ll << 31), "nn_prepare_u8: rows=%lld out of range", (long long)rows);
    CSLGAN_REQUIRE(aligned16(x) && aligned16(xs) && (reinterpret_cast<uintptr_t>(sqnorm) & 3u) == 0, "nn_prepare_u8: misaligned pointer");
    note_kernel("nn_prepare_u8_kernel");
    const int rows_per_wg = NN_THREADS / WAVE;
    hipLaunchKernelGGL(nn_prepare_u8_kernel, dim3((unsigned)((rows + rows_per_wg - 1) / rows_per_wg)), dim3(NN_THREADS), 0, (hipStream_t)stream,
                       (const unsigned char*)x, (long long)rows, D, Dp, (signed char*)xs, (int*)sqnorm);
    return check_launch("nn_prepare_u8_kernel");
}

// What a valid pair of prepared operands is, for the four entries below: q / r non-null and 16-byte aligned, their norms qn / rn
// non-null and 4-byte aligned, a row pitch Dp that nn_prepare_u8 can have produced, and row counts that fit an int.  `entry`
// prefixes the message.  An entry checks its own arguments itself.
static int nn_check_operands(const char* entry, const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp) {
    CSLGAN_REQUIRE(q && qn && r && rn, "%s: null argument", entry);
    CSLGAN_REQUIRE(Dp >= NN_KT && Dp <= NN_MAX_D && Dp % NN_KT == 0, "%s: Dp=%d must be a multiple of %d in %d .. %d", entry, Dp, NN_KT, NN_KT,
                   NN_MAX_D);
    CSLGAN_REQUIRE(nq >= 1 && nq < (1ll << 31), "%s: nq=%lld out of range", entry, (long long)nq);
    CSLGAN_REQUIRE(nr >= 1 && nr < (1ll << 31), "%s: nr=%lld out of range", entry, (long long)nr);
    CSLGAN_REQUIRE(aligned16(q) && aligned16(r) && (reinterpret_cast<uintptr_t>(qn) & 3u) == 0 && (reinterpret_cast<uintptr_t>(rn) & 3u) == 0,
                   "%s: misaligned pointer", entry);
    return CSLGAN_OK;
}

int cslgan_nn_min_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp, int64_t index_base,
                     uint64_t* best, void* stream) {
    CSLGAN_REQUIRE(best, "nn_min_i8: null argument");
    if (int rc = nn_check_operands("nn_min_i8", q, qn, nq, r, rn, nr, Dp)) return rc;
    CSLGAN_REQUIRE(index_base >= 0 && index_base + nr <= 0xFFFFFFFFll, "nn_min_i8: index_base + nr = %lld exceeds 2^32 - 1",
                   (long long)(index_base + nr));
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(best) & 7u) == 0, "nn_min_i8: misaligned pointer");
    long long tiles_per = 0;
    const long long gy = nn_column_ranges(nq, nr, NN_ANY_TILES, &tiles_per);
    CSLGAN_REQUIRE(gy <= 65535, "nn_min_i8: nr=%lld needs %lld column ranges", (long long)nr, gy);
    const long long col_tiles = (nr + NN_TN - 1) / NN_TN;
    note_kernel("nn_min_i8_kernel");
    hipLaunchKernelGGL(nn_min_i8_kernel, dim3((unsigned)((nq + NN_TM - 1) / NN_TM), (unsigned)gy), dim3(NN_THREADS), 0, (hipStream_t)stream,
                       (const signed char*)q, (const int*)qn, (int)nq, (const signed char*)r, (const int*)rn, (int)nr, Dp, (uint32_t)index_base,
                       (int)tiles_per, (int)col_tiles, (unsigned long long*)best);
    return check_launch("nn_min_i8_kernel");
}

int cslgan_nn_count_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp,
                       const uint32_t* thresholds, int n_thr, uint32_t* counts, void* stream) {
    CSLGAN_REQUIRE(thresholds && counts, "nn_count_i8: null argument");
    CSLGAN_REQUIRE(n_thr >= 1 && n_thr <= NN_MAX_THR, "nn_count_i8: n_thr=%d must lie in 1 .. %d", n_thr, NN_MAX_THR);
    if (int rc = nn_check_operands("nn_count_i8", q, qn, nq, r, rn, nr, Dp)) return rc;
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 3u) == 0 && (reinterpret_cast<uintptr_t>(thresholds) & 3u) == 0,
                   "nn_count_i8: misaligned pointer");
    long long tiles_per = 0;                                   // no more tiles per workgroup than a byte counter holds
    const long long gy = nn_column_ranges(nq, nr, NN_COUNT_TILES, &tiles_per);
    CSLGAN_REQUIRE(gy <= 65535, "nn_count_i8: nr=%lld needs %lld column ranges", (long long)nr, gy);
    const long long col_tiles = (nr + NN_TN - 1) / NN_TN;
    NNThresholds thr = {{0u, 0u, 0u, 0u}};
    for (int j = 0; j < n_thr; ++j) thr.t[j] = thresholds[j];  // read now: the caller's array may go when this returns
    note_kernel("nn_count_i8_kernel");
    hipLaunchKernelGGL(nn_count_i8_kernel, dim3((unsigned)((nq + NN_TM - 1) / NN_TM), (unsigned)gy), dim3(NN_THREADS), 0, (hipStream_t)stream,
                       (const signed char*)q, (const int*)qn, (int)nq, (const signed char*)r, (const int*)rn, (int)nr, Dp, thr, n_thr, (int)tiles_per,
                       (int)col_tiles, (uint32_t*)counts);
    return check_launch("nn_count_i8_kernel");
}

int64_t cslgan_nn_kth_workspace_bytes(int64_t nq, int64_t nr, int k) {
    if (k < 1 || k > NN_MAX_K) return 0;
    const long long gy = nn_column_ranges(nq, nr, NN_ANY_TILES, nullptr);
    if (gy < 1 || gy > 65535) return 0;
    return (int64_t)(gy * nq * k * 8);
}

int cslgan_nn_kth_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp, int64_t index_base,
                     int64_t self_base, int k, uint64_t* best, void* workspace, int64_t workspace_bytes, void* stream) {
    CSLGAN_REQUIRE(best && workspace, "nn_kth_i8: null argument");
    CSLGAN_REQUIRE(k >= 1 && k <= NN_MAX_K, "nn_kth_i8: k=%d must lie in 1 .. %d", k, NN_MAX_K);
    if (int rc = nn_check_operands("nn_kth_i8", q, qn, nq, r, rn, nr, Dp)) return rc;
    CSLGAN_REQUIRE(index_base >= 0 && index_base + nr <= 0xFFFFFFFFll, "nn_kth_i8: index_base + nr = %lld exceeds 2^32 - 1",
                   (long long)(index_base + nr));
    CSLGAN_REQUIRE(self_base >= -1 && self_base + nq <= 0xFFFFFFFFll, "nn_kth_i8: self_base=%lld must be -1 or keep self_base + nq <= 2^32 - 1",
                   (long long)self_base);
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(best) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
                   "nn_kth_i8: misaligned pointer");
    long long tiles_per = 0;
    const long long gy = nn_column_ranges(nq, nr, NN_ANY_TILES, &tiles_per);
    CSLGAN_REQUIRE(gy >= 1 && gy <= 65535, "nn_kth_i8: nr=%lld needs %lld column ranges", (long long)nr, gy);
    CSLGAN_REQUIRE(workspace_bytes >= gy * nq * k * 8, "nn_kth_i8: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                   (long long)(gy * nq * k * 8));
    const long long col_tiles = (nr + NN_TN - 1) / NN_TN;
    note_kernel("nn_kth_i8_kernel");
    hipLaunchKernelGGL(nn_kth_i8_kernel, dim3((unsigned)((nq + NN_TM - 1) / NN_TM), (unsigned)gy), dim3(NN_THREADS), 0, (hipStream_t)stream,
                       (const signed char*)q, (const int*)qn, (int)nq, (const signed char*)r, (const int*)rn, (int)nr, Dp, (uint32_t)index_base,
                       (long long)self_base, k, (int)tiles_per, (int)col_tiles, (const unsigned long long*)best, (unsigned long long*)workspace);
    if (int rc = check_launch("nn_kth_i8_kernel")) return rc;
    note_kernel("nn_kth_merge_kernel");
    hipLaunchKernelGGL(nn_kth_merge_kernel, dim3((unsigned)((nq + NN_THREADS - 1) / NN_THREADS)), dim3(NN_THREADS), 0, (hipStream_t)stream,
                       (const unsigned long long*)workspace, (int)gy, (int)nq, k, (unsigned long long*)best);
    return check_launch("nn_kth_merge_kernel");
}

int cslgan_nn_count_radius_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp,
                              const uint32_t* radius, uint32_t* counts, void* stream) {
    CSLGAN_REQUIRE(radius && counts, "nn_count_radius_i8: null argument");
    if (int rc = nn_check_operands("nn_count_radius_i8", q, qn, nq, r, rn, nr, Dp)) return rc;
    CSLGAN_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 3u) == 0 && (reinterpret_cast<uintptr_t>(radius) & 3u) == 0,
                   "nn_count_radius_i8: misaligned pointer");
    long long tiles_per = 0;
    const long long gy = nn_column_ranges(nq, nr, NN_ANY_TILES, &tiles_per);
    CSLGAN_REQUIRE(gy >= 1 && gy <= 65535, "nn_count_radius_i8: nr=%lld needs %lld column ranges", (long long)nr, gy);
    const long long col_tiles = (nr + NN_TN - 1) / NN_TN;
    note_kernel("nn_count_radius_i8_kernel");
    hipLaunchKernelGGL(nn_count_radius_i8_kernel, dim3((unsigned)((nq + NN_TM - 1) / NN_TM), (unsigned)gy), dim3(NN_THREADS), 0,
                       (hipStream_t)stream, (const signed char*)q, (const int*)qn, (int)nq, (const signed char*)r, (const int*)rn, (int)nr, Dp,
                       radius, (int)tiles_per, (int)col_tiles, (uint32_t*)counts);
    return check_launch("nn_count_radius_i8_kernel");
}

}  // extern "C"
