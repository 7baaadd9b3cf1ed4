// Sliced-Wasserstein audit kernels for gfx950 (csl_gan_amd.sliced; DESIGN.md §6q, include/cslgan.h "Sliced Wasserstein audit").
//
// Exact integer arithmetic on uint8 image caches: P Rademacher directions from an indexed Philox stream, the projection of every
// cache row on every direction as an int32 matrix (the tile loop of nn_tile.h with an epilogue that KEEPS the product), a segmented
// LSD radix sort of the rows of that matrix, and the one-dimensional W1 numerator of two sorted rows as one int64.  Nothing in this
// file waits for another workgroup: every pass of the sort is a launch of its own.
#include "common.h"
#include "device_prims.h"
#include "nn_tile.h"

namespace cslgan {

constexpr uint32_t SWD_COUNTER_TAG = 0x73776464u;                        // word 3 of every counter of the direction stream ("swdd")
constexpr unsigned long long SWD_SEED_TAG = 0x7377647369676E73ull;       // xor-ed into the seed ("swdsigns")

// ---- directions ----------------------------------------------------------------------------------------------------------------------
// One thread per (direction p, 128-column group b): one Philox call, eight 16-byte stores.  Bit t of the call (word t >> 5, bit
// t & 31) is the sign of column 128 b + t: set +1, clear -1; a column >= D is zero.
__global__ __launch_bounds__(256) void swd_directions_i8_kernel(unsigned long long key, long long P, int D, int Dp, int groups,
                                                                signed char* __restrict__ dirs) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= P * groups) return;
    const long long p = id / groups;
    const int b = (int)(id % groups);
    uint32_t w[4];
    philox4x32_10((uint32_t)b, (uint32_t)p, 0u, SWD_COUNTER_TAG, (uint32_t)key, (uint32_t)(key >> 32), w);
    u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(dirs + p * (long long)Dp + 128ll * b);
#pragma unroll
    for (int c = 0; c < 8; ++c) {                              // chunk c: columns 128 b + 16 c .. + 15, bits 16 c .. of the call
        const int col0 = 128 * b + 16 * c;
        if (col0 >= Dp) break;                                 // Dp is a multiple of 64: the last group may be half a group
        const uint32_t bits = (w[c >> 1] >> (16 * (c & 1))) & 0xffffu;
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t v = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = 4 * q + k;
                const uint32_t byte = col0 + t < D ? (((bits >> t) & 1u) ? 0x01u : 0xffu) : 0u;
                v |= byte << (8 * k);
            }
            o[q] = v;
        }
        u32x4 out = {o[0], o[1], o[2], o[3]};
        dst[c] = out;
    }
}

// ---- projection ------------------------------------------------------------------------------------------------------------------------
// Y[p, col0 + i] = dirs[p] . xs[i]: the directions are the row operand of the tile loop and the data rows its column operand, so per
// accumulator register the 32 lanes of a row half hold 32 consecutive columns of one Y row, one 128-byte store where col0 allows.
// Every element has exactly one writer: the column ranges of the launch are disjoint.
__global__ __launch_bounds__(NN_THREADS) void swd_project_i8_kernel(const signed char* __restrict__ dirs, int P, const signed char* __restrict__ xs,
                                                                    int n, int Dp, int tiles_per, int n_col_tiles, int* __restrict__ Y,
                                                                    long long ldy, long long col0) {
    const NNLane ln(threadIdx.x);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    nn_tile_loop<true>(dirs, nullptr, P, xs, nullptr, n, Dp, tiles_per, n_col_tiles, NNNoColumn(),
                       [&](int mt, int i, bool live, long long col, uint32_t dot) {
                           const long long row = row0 + ln.row(mt, i);
                           if (live && row < P) Y[row * ldy + col0 + col] = (int)dot;
                       });
}

// ---- segmented LSD radix sort ------------------------------------------------------------------------------------------------------------
// Rows of an int32 matrix, ascending and signed: the key is value + 2^(key_bits - 1) as uint32 (for 32 bits the flipped sign bit),
// eight bits per pass from the lowest.  A pass is three launches: the digit histogram of every (row, tile) in LDS, an exclusive scan
// per row over (digit, tile), and the scatter of every tile from the pass's source to its destination.  The scatter ranks a tile in
// 16 rounds of 256 consecutive entries: inside a wave by ballots (the lanes that hold the same digit and come earlier), across
// the four waves and the earlier rounds by counters in LDS, so equal digits keep their order and the pass is stable.  Tail tiles and
// short rows are masked by the entry's index; nothing is read or written beyond entry n - 1 of a row.
constexpr int SORT_THREADS = 256;
constexpr int SORT_ITEMS = 16;
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;           // 4096 entries
constexpr int SORT_RADIX = 256;

__device__ __forceinline__ unsigned sort_digit(int v, unsigned bias, int shift) { return (((unsigned)v + bias) >> shift) & (SORT_RADIX - 1); }

// counts[(p T + t) 256 + d] = entries of tile t of row p whose digit is d
__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(const int* __restrict__ src, long long ld, int n, int T, int shift, unsigned bias,
                                                                 unsigned* __restrict__ counts) {
    __shared__ unsigned h[SORT_RADIX];
    const int tid = threadIdx.x;
    const long long p = blockIdx.x / (unsigned)T;
    const int t = (int)(blockIdx.x % (unsigned)T);
    h[tid] = 0u;
    __syncthreads();
    const int* __restrict__ row = src + p * ld;
    const long long e0 = (long long)t * SORT_TILE;
#pragma unroll 4
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long long e = e0 + r * SORT_THREADS + tid;
        if (e < n) atomicAdd(&h[sort_digit(row[e], bias, shift)], 1u);
    }
    __syncthreads();
    counts[(long long)blockIdx.x * SORT_RADIX + tid] = h[tid];
}

// per row: counts -> the first destination index of every (tile, digit): digits ascending, inside a digit the tiles ascending.
// Thread d owns digit d: its loads and stores run along the tiles, 256 consecutive words per tile over the workgroup.
__global__ __launch_bounds__(SORT_THREADS) void sort_scan_kernel(unsigned* __restrict__ counts, int T) {
    __shared__ unsigned tot[SORT_RADIX];
    const int d = threadIdx.x;
    unsigned* __restrict__ c = counts + (long long)blockIdx.x * T * SORT_RADIX;
    unsigned sum = 0u;
    for (int t = 0; t < T; ++t) sum += c[(long long)t * SORT_RADIX + d];
    tot[d] = sum;
    __syncthreads();
    unsigned run = 0u;
    for (int j = 0; j < d; ++j) run += tot[j];
    for (int t = 0; t < T; ++t) {
        const unsigned v = c[(long long)t * SORT_RADIX + d];
        c[(long long)t * SORT_RADIX + d] = run;
        run += v;
    }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(const int* __restrict__ src, long long ld_src, int* __restrict__ dst,
                                                                    long long ld_dst, int n, int T, int shift, unsigned bias,
                                                                    const unsigned* __restrict__ offsets) {
    __shared__ unsigned run[SORT_RADIX];                       // next destination index of every digit for this tile
    __shared__ unsigned wcnt[SORT_THREADS / WAVE][SORT_RADIX]; // this round's entries per wave and digit
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long p = blockIdx.x / (unsigned)T;
    const int t = (int)(blockIdx.x % (unsigned)T);
    run[tid] = offsets[(long long)blockIdx.x * SORT_RADIX + tid];
#pragma unroll
    for (int k = 0; k < SORT_THREADS / WAVE; ++k) wcnt[k][tid] = 0u;
    __syncthreads();
    const int* __restrict__ srow = src + p * ld_src;
    int* __restrict__ drow = dst + p * ld_dst;
    const long long e0 = (long long)t * SORT_TILE;
    for (int r = 0; r < SORT_ITEMS; ++r) {
        if (e0 + (long long)r * SORT_THREADS >= n) break;      // uniform over the workgroup
        const long long e = e0 + r * SORT_THREADS + tid;
        const bool valid = e < n;
        const int v = valid ? srow[e] : 0;
        const unsigned d = sort_digit(v, bias, shift);
        unsigned long long peers = __ballot(valid);            // the valid lanes of the wave with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(valid && bit);
            peers &= bit ? bal : ~bal;
        }
        const unsigned rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wcnt[w][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (valid) {
            unsigned pos = run[d] + rank;
#pragma unroll
            for (int k = 0; k < SORT_THREADS / WAVE - 1; ++k) pos += k < w ? wcnt[k][d] : 0u;
            if (pos < (unsigned)n) drow[pos] = v;              // always true for counts of this source; never a store beyond the row
        }
        __syncthreads();
        unsigned s = 0u;
#pragma unroll
        for (int k = 0; k < SORT_THREADS / WAVE; ++k) {
            s += wcnt[k][tid];
            wcnt[k][tid] = 0u;
        }
        run[tid] += s;
        __syncthreads();
    }
}

// an odd number of passes leaves the result in the workspace
__global__ __launch_bounds__(SORT_THREADS) void sort_copy_rows_kernel(const int* __restrict__ src, long long ld_src, int* __restrict__ dst,
                                                                      long long ld_dst, int n, int T) {
    const long long p = blockIdx.x / (unsigned)T;
    const long long e0 = (long long)(blockIdx.x % (unsigned)T) * SORT_TILE;
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long long e = e0 + r * SORT_THREADS + threadIdx.x;
        if (e < n) dst[p * ld_dst + e] = src[p * ld_src + e];
    }
}

static long long sort_tiles(int64_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }
static long long sort_pitch(int64_t n) { return (n + 3) / 4 * 4; }      // of the ping-pong rows: 16-byte aligned row starts

// ---- W1 numerator ----------------------------------------------------------------------------------------------------------------------
// num[p] = sum_i sum_j |l[i] - s[j]| * |[i Ns, (i + 1) Ns) n [j Nl, (j + 1) Nl)| for the longer row l (Nl entries) and the shorter s
// (Ns <= Nl): entry i of l meets the entries floor(i Ns / Nl) .. floor(((i + 1) Ns - 1) / Nl) of s, at most two.  One workgroup per
// direction, a strided share of i per thread, int64 throughout, one plain store.
constexpr int W1_THREADS = 256;

__global__ __launch_bounds__(W1_THREADS) void swd_w1_i64_kernel(const int* __restrict__ L, long long ldl, long long Nl, const int* __restrict__ S,
                                                                long long lds, long long Ns, long long* __restrict__ num) {
    __shared__ long long red[W1_THREADS / WAVE];
    const long long p = blockIdx.x;
    const int* __restrict__ l = L + p * ldl;
    const int* __restrict__ s = S + p * lds;
    long long acc = 0;
    for (long long i = threadIdx.x; i < Nl; i += W1_THREADS) {
        const long long lo = i * Ns, hi = lo + Ns;
        const long long j0 = lo / Nl, j1 = (hi - 1) / Nl;      // j1 <= (Nl Ns - 1) / Nl = Ns - 1
        const long long li = l[i];
        for (long long j = j0; j <= j1; ++j) {
            const long long s_lo = j * Nl, s_hi = s_lo + Nl;
            const long long ov = (hi < s_hi ? hi : s_hi) - (lo > s_lo ? lo : s_lo);
            const long long d = li - (long long)s[j];
            acc += (d < 0 ? -d : d) * ov;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
#pragma unroll
        for (int k = 0; k < W1_THREADS / WAVE; ++k) t += red[k];
        num[p] = t;
    }
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_swd_directions_i8(uint64_t seed, int64_t P, int D, int Dp, void* dirs, void* stream) {
    CSLGAN_REQUIRE(dirs, "swd_directions_i8: null argument");
    CSLGAN_REQUIRE(D >= 1 && D <= NN_MAX_D, "swd_directions_i8: D=%d must lie in 1 .. %d", D, NN_MAX_D);
    CSLGAN_REQUIRE(Dp == (D + NN_KT - 1) / NN_KT * NN_KT, "swd_directions_i8: Dp=%d is not the padded width %d of D=%d", Dp,
                   (D + NN_KT - 1) / NN_KT * NN_KT, D);
    CSLGAN_REQUIRE(P >= 1 && P < (1ll << 31), "swd_directions_i8: P=%lld out of range", (long long)P);
    CSLGAN_REQUIRE(aligned16(dirs), "swd_directions_i8: misaligned pointer");
    const int groups = (Dp + 127) / 128;
    const long long blocks = (P * groups + 255) / 256;
    CSLGAN_REQUIRE(blocks < (1ll << 31), "swd_directions_i8: P=%lld directions of Dp=%d need %lld workgroups", (long long)P, Dp, blocks);
    note_kernel("swd_directions_i8_kernel");
    hipLaunchKernelGGL(swd_directions_i8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long)(seed ^ SWD_SEED_TAG), (long long)P, D, Dp, groups, (signed char*)dirs);
    return check_launch("swd_directions_i8_kernel");
}

int cslgan_swd_project_i8(const void* dirs, int64_t P, const void* xs, int64_t n, int Dp, int32_t* Y, int64_t ldy, int64_t col0, void* stream) {
    CSLGAN_REQUIRE(dirs && xs && Y, "swd_project_i8: null argument");
    CSLGAN_REQUIRE(Dp >= NN_KT && Dp <= NN_MAX_D && Dp % NN_KT == 0, "swd_project_i8: Dp=%d must be a multiple of %d in %d .. %d", Dp, NN_KT,
                   NN_KT, NN_MAX_D);
    CSLGAN_REQUIRE(P >= 1 && P < (1ll << 31), "swd_project_i8: P=%lld out of range", (long long)P);
    CSLGAN_REQUIRE(n >= 1 && n < (1ll << 31), "swd_project_i8: n=%lld out of range", (long long)n);
    CSLGAN_REQUIRE(col0 >= 0 && col0 < (1ll << 40) && ldy < (1ll << 40) && ldy >= col0 + n,
                   "swd_project_i8: ldy=%lld is smaller than col0 + n = %lld + %lld (or out of range)", (long long)ldy, (long long)col0,
                   (long long)n);
    CSLGAN_REQUIRE(aligned16(dirs) && aligned16(xs) && aligned_to(Y, 4), "swd_project_i8: misaligned pointer");
    long long tiles_per = 0;
    const long long gy = nn_column_ranges(P, n, NN_ANY_TILES, &tiles_per);
    CSLGAN_REQUIRE(gy >= 1 && gy <= 65535, "swd_project_i8: n=%lld needs %lld column ranges", (long long)n, gy);
    const long long col_tiles = (n + NN_TN - 1) / NN_TN;
    note_kernel("swd_project_i8_kernel");
    hipLaunchKernelGGL(swd_project_i8_kernel, dim3((unsigned)((P + NN_TM - 1) / NN_TM), (unsigned)gy), dim3(NN_THREADS), 0, (hipStream_t)stream,
                       (const signed char*)dirs, (int)P, (const signed char*)xs, (int)n, Dp, (int)tiles_per, (int)col_tiles, (int*)Y,
                       (long long)ldy, (long long)col0);
    return check_launch("swd_project_i8_kernel");
}

int64_t cslgan_sort_rows_ws_bytes(int64_t P, int64_t n) {
    if (P < 1 || n < 1 || P >= (1ll << 31) || n >= (1ll << 31)) return 0;
    if (P * sort_tiles(n) >= (1ll << 31)) return 0;
    return (int64_t)(P * sort_pitch(n) * 4 + P * sort_tiles(n) * SORT_RADIX * 4);
}

int cslgan_sort_rows_i32(int32_t* x, int64_t P, int64_t n, int64_t ld, int key_bits, void* ws, int64_t ws_bytes, void* stream) {
    CSLGAN_REQUIRE(x && ws, "sort_rows_i32: null argument");
    CSLGAN_REQUIRE(P >= 1 && P < (1ll << 31), "sort_rows_i32: P=%lld out of range", (long long)P);
    CSLGAN_REQUIRE(n >= 1 && n < (1ll << 31), "sort_rows_i32: n=%lld out of range", (long long)n);
    CSLGAN_REQUIRE(ld >= n && ld < (1ll << 40), "sort_rows_i32: ld=%lld is smaller than n=%lld (or out of range)", (long long)ld, (long long)n);
    CSLGAN_REQUIRE(key_bits >= 1 && key_bits <= 32, "sort_rows_i32: key_bits=%d must lie in 1 .. 32", key_bits);
    const long long T = sort_tiles(n), pitch = sort_pitch(n);
    CSLGAN_REQUIRE(P * T < (1ll << 31), "sort_rows_i32: P=%lld rows of n=%lld entries need %lld workgroups", (long long)P, (long long)n, P * T);
    CSLGAN_REQUIRE(ws_bytes >= cslgan_sort_rows_ws_bytes(P, n), "sort_rows_i32: workspace of %lld bytes, need %lld", (long long)ws_bytes,
                   (long long)cslgan_sort_rows_ws_bytes(P, n));
    CSLGAN_REQUIRE(aligned_to(x, 4) && aligned16(ws), "sort_rows_i32: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    int* other = (int*)ws;
    unsigned* counts = (unsigned*)(other + P * pitch);
    const unsigned bias = 1u << (key_bits - 1);
    const int passes = (key_bits + 7) / 8;
    const int* src = x;
    long long ld_src = ld;
    int* dst = other;
    long long ld_dst = pitch;
    for (int pass = 0; pass < passes; ++pass) {
        const int shift = 8 * pass;
        note_kernel("sort_hist_kernel");
        hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)(P * T)), dim3(SORT_THREADS), 0, st, src, ld_src, (int)n, (int)T, shift, bias, counts);
        if (int rc = check_launch("sort_hist_kernel")) return rc;
        note_kernel("sort_scan_kernel");
        hipLaunchKernelGGL(sort_scan_kernel, dim3((unsigned)P), dim3(SORT_THREADS), 0, st, counts, (int)T);
        if (int rc = check_launch("sort_scan_kernel")) return rc;
        note_kernel("sort_scatter_kernel");
        hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)(P * T)), dim3(SORT_THREADS), 0, st, src, ld_src, dst, ld_dst, (int)n, (int)T, shift,
                           bias, (const unsigned*)counts);
        if (int rc = check_launch("sort_scatter_kernel")) return rc;
        int* const was = const_cast<int*>(src);
        const long long ld_was = ld_src;
        src = dst;
        ld_src = ld_dst;
        dst = was;
        ld_dst = ld_was;
    }
    if (src != x) {
        note_kernel("sort_copy_rows_kernel");
        hipLaunchKernelGGL(sort_copy_rows_kernel, dim3((unsigned)(P * T)), dim3(SORT_THREADS), 0, st, src, ld_src, (int*)x, (long long)ld, (int)n,
                           (int)T);
        return check_launch("sort_copy_rows_kernel");
    }
    return CSLGAN_OK;
}

int cslgan_swd_w1_i64(const int32_t* a, int64_t lda, int64_t Na, const int32_t* b, int64_t ldb, int64_t Nb, int64_t P, int64_t* num,
                      void* stream) {
    CSLGAN_REQUIRE(a && b && num, "swd_w1_i64: null argument");
    CSLGAN_REQUIRE(P >= 1 && P < (1ll << 31), "swd_w1_i64: P=%lld out of range", (long long)P);
    CSLGAN_REQUIRE(Na >= 1 && Na < (1ll << 31) && Nb >= 1 && Nb < (1ll << 31), "swd_w1_i64: Na=%lld, Nb=%lld out of range", (long long)Na,
                   (long long)Nb);
    CSLGAN_REQUIRE(Na * Nb < (1ll << 38), "swd_w1_i64: Na * Nb * 2^25 = %lld * %lld * 2^25 >= 2^63 overflows the int64 numerator",
                   (long long)Na, (long long)Nb);
    CSLGAN_REQUIRE(lda >= Na && ldb >= Nb && lda < (1ll << 40) && ldb < (1ll << 40), "swd_w1_i64: lda=%lld / ldb=%lld smaller than Na=%lld / Nb=%lld",
                   (long long)lda, (long long)ldb, (long long)Na, (long long)Nb);
    CSLGAN_REQUIRE(aligned_to(a, 4) && aligned_to(b, 4) && aligned_to(num, 8), "swd_w1_i64: misaligned pointer");
    const bool a_long = Na >= Nb;
    note_kernel("swd_w1_i64_kernel");
    hipLaunchKernelGGL(swd_w1_i64_kernel, dim3((unsigned)P), dim3(W1_THREADS), 0, (hipStream_t)stream, (const int*)(a_long ? a : b),
                       (long long)(a_long ? lda : ldb), (long long)(a_long ? Na : Nb), (const int*)(a_long ? b : a), (long long)(a_long ? ldb : lda),
                       (long long)(a_long ? Nb : Na), (long long*)num);
    return check_launch("swd_w1_i64_kernel");
}

}  // extern "C"
