// The 128 x 128 int8 tile loop of the exact squared-distance kernels (nn_kernels.hip: search, counts, k-th keys; svm_kernels.hip: the
// stored matrix; swd_kernels.hip: the stored projection) and the launch rule of its entries.  Operands are those of
// nn_prepare_u8_kernel (nn_kernels.hip): int8 rows of pitch Dp, a multiple of NN_KT, with their squared norms.
#pragma once
#include "common.h"
#include "device_prims.h"

namespace cslgan {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int NN_KT = 64;                         // bytes of K per LDS stage = the row pitch granule of the prepared operands
constexpr int NN_TM = 128, NN_TN = 128;           // rows of Q x rows of R per workgroup tile: 2 x 2 waves of 64 x 64
constexpr int NN_PITCH = NN_KT + 16;              // LDS row pitch: 20 dwords, so 16 consecutive rows of a 16-byte read cover all 64 banks
constexpr int NN_THREADS = 256;
constexpr int NN_MAX_D = 65536;                   // 255^2 D < 2^32
constexpr unsigned long long NN_NONE = ~0ull;     // "nothing seen yet"

// ---- the tile loop that the search and the count share ---------------------------------------------------------------------------
// Workgroup (bx, by): rows bx * 128 .. of Q against column tiles by * tiles_per .. of R.  The K loop runs flattened over
// (column tile, K stage): stage i + 1 is fetched from HBM/L2 into registers while stage i is multiplied out of LDS, and stored to
// the other LDS buffer before the single barrier of the iteration.  Both operands are K-contiguous and read with the same
// lane -> k assignment (lane half h: 16 consecutive bytes), so the sums do not depend on the instruction's k order; the
// row/column maps are those of every 32x32 form: operand row = lane & 31, C/D col = lane & 31, row = (reg & 3) + 8 (reg >> 2) +
// 4 (lane >> 5); tests/test_nearest_gpu.py checks them with asymmetric exact-integer data.
struct NNLane {                                                // where a lane sits in the 128 x 128 tile
    int wm, wn, l31, lh;                                       // the wave's 64 x 64 quadrant; column and row half inside a 32 x 32 block
    __device__ __forceinline__ explicit NNLane(int tid) : wm(tid >> 7), wn((tid >> 6) & 1), l31(tid & 31), lh((tid >> 5) & 1) {}
    __device__ __forceinline__ int row(int mt, int i) const { return wm * 64 + mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh; }      // of accumulator register i
    __device__ __forceinline__ long long col(int ct, int nt) const { return (long long)ct * NN_TN + wn * 64 + nt * 32 + l31; }   // in R
};

// After the last K stage of a column tile the loop forms d2 = |a|^2 + |b|^2 - 2 a.b in uint32 (the true value is below 2^32, so
// arithmetic mod 2^32 returns it exactly; int32 would not hold it) and hands every element to the epilogue:
// `epi(int mt, int i, bool live, long long col, uint32_t d2)` for row ln.row(mt, i) and column col of R, live = col < nr (a column
// past nr has a d2 that means nothing).  The epilogue is a lambda over the kernel's own running values, which stay locals of the
// kernel so that they are promoted to registers.  The loop ends behind a barrier, every call done.
// A kernel that needs a value per COLUMN (nn_count_radius_i8_kernel: the column's radius) passes `per_col(bool live, long long col)`
// as well, which runs once per column and tile ahead of that column's 32 epilogue calls.
// RAW = true (swd_kernels.hip: the stored projection) hands the epilogue the accumulator itself, the dot product a.b as the bits of
// an int32, in place of d2; qn and rn are then never read and may be null.  The default is the loop of the distance kernels.
struct NNNoColumn {
    __device__ __forceinline__ void operator()(bool, long long) const {}
};

template <bool RAW = false, class PerColumn, class Epilogue>
__device__ __forceinline__ void nn_tile_loop(const signed char* __restrict__ q, const int* __restrict__ qn, int nq, const signed char* __restrict__ r,
                                             const int* __restrict__ rn, int nr, int Dp, int tiles_per, int n_col_tiles, PerColumn per_col,
                                             Epilogue epi) {
    __shared__ __attribute__((aligned(16))) unsigned char sA[2][NN_TM * NN_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char sB[2][NN_TN * NN_PITCH];
    __shared__ int qn_s[NN_TM];

    const int tid = threadIdx.x;
    const NNLane ln(tid);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    const int rows_here = (int)(nq - row0 < NN_TM ? nq - row0 : NN_TM);
    const int tile_first = blockIdx.y * tiles_per;
    const int tile_end = tile_first + tiles_per < n_col_tiles ? tile_first + tiles_per : n_col_tiles;
    const int nk = Dp / NN_KT;
    const int n_iter = (tile_end - tile_first) * nk;

    if (!RAW && tid < NN_TM) qn_s[tid] = tid < rows_here ? qn[row0 + tid] : 0;

    // range-checked descriptors over the rows that exist: a row past nq / nr reads as zeros (and is masked in the epilogue anyway)
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(q + row0 * (long long)Dp, (unsigned)rows_here * (unsigned)Dp);
    const int ld_row = tid >> 2, ld_chunk = (tid & 3) * 16;    // this thread's two 16-byte pieces of a stage: rows ld_row, ld_row + 64
    const unsigned ld_off = (unsigned)ld_row * (unsigned)Dp + (unsigned)ld_chunk;
    const unsigned ld_off2 = ld_off + 64u * (unsigned)Dp;
    const int st_off = ld_row * NN_PITCH + ld_chunk;

    u32x4 ga0, ga1, gb0, gb1;
    int f_kt = 0, f_ct = tile_first;                           // the (column tile, K stage) of the next fetch
    auto fetch = [&]() {
        const unsigned k0 = (unsigned)f_kt * NN_KT;
        const long long c0 = (long long)f_ct * NN_TN;
        const int cols_here = (int)(nr - c0 < NN_TN ? nr - c0 : NN_TN);
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(r + c0 * (long long)Dp, (unsigned)cols_here * (unsigned)Dp);
        ga0 = buf_load4_raw(rq, ld_off + k0);
        ga1 = buf_load4_raw(rq, ld_off2 + k0);
        gb0 = buf_load4_raw(rr, ld_off + k0);
        gb1 = buf_load4_raw(rr, ld_off2 + k0);
        if (++f_kt == nk) { f_kt = 0; ++f_ct; }
    };
    auto stash = [&](int buf) {
        *reinterpret_cast<u32x4*>(&sA[buf][st_off]) = ga0;
        *reinterpret_cast<u32x4*>(&sA[buf][st_off + 64 * NN_PITCH]) = ga1;
        *reinterpret_cast<u32x4*>(&sB[buf][st_off]) = gb0;
        *reinterpret_cast<u32x4*>(&sB[buf][st_off + 64 * NN_PITCH]) = gb1;
    };

    i32x16 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0;

    if (n_iter > 0) {
        fetch();
        stash(0);
    }
    __syncthreads();                                           // also publishes qn_s

    const int a_off = (ln.wm * 64 + ln.l31) * NN_PITCH + 16 * ln.lh;
    const int b_off = (ln.wn * 64 + ln.l31) * NN_PITCH + 16 * ln.lh;
    int kt = 0, ct = tile_first;
    for (int it = 0; it < n_iter; ++it) {
        const int buf = it & 1;
        if (it + 1 < n_iter) fetch();
#pragma unroll
        for (int ks = 0; ks < NN_KT / 32; ++ks) {
            i32x4 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const i32x4*>(&sA[buf][a_off + t * 32 * NN_PITCH + ks * 32]);
                b[t] = *reinterpret_cast<const i32x4*>(&sB[buf][b_off + t * 32 * NN_PITCH + ks * 32]);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
        if (++kt == nk) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const long long col = ln.col(ct, nt);
                const bool live = col < nr;
                const uint32_t bn = (!RAW && live) ? (uint32_t)rn[col] : 0u;
                per_col(live, col);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        if (RAW)
                            epi(mt, i, live, col, (uint32_t)acc[mt][nt][i]);
                        else
                            epi(mt, i, live, col, (uint32_t)qn_s[ln.row(mt, i)] + bn - 2u * (uint32_t)acc[mt][nt][i]);
                        acc[mt][nt][i] = 0;
                    }
            }
            kt = 0;
            ++ct;
        }
        if (it + 1 < n_iter) stash(buf ^ 1);                   // last read in iteration it - 1, which every wave has left
        __syncthreads();
    }
}

constexpr long long NN_ANY_TILES = 1ll << 31;                  // no cap on the tiles of a workgroup: more than any nr has

// The launch rule of the four entries: the column tiles are cut into ranges of tiles_per tiles, one workgroup per row tile and
// range — enough workgroups (about 1024) for every CU a few times over, and as few ranges, hence atomics or partial lists per row,
// as that allows; never more than max_tiles tiles per workgroup.  Returns the number of ranges, 0 for sizes out of range.
static long long nn_column_ranges(int64_t nq, int64_t nr, long long max_tiles, long long* tiles_per_out) {
    if (nq < 1 || nq >= (1ll << 31) || nr < 1 || nr >= (1ll << 31)) return 0;
    const long long row_tiles = (nq + NN_TM - 1) / NN_TM, col_tiles = (nr + NN_TN - 1) / NN_TN;
    long long splits = (1024 + row_tiles - 1) / row_tiles;
    splits = splits < 1 ? 1 : (splits > col_tiles ? col_tiles : splits);
    long long tiles_per = (col_tiles + splits - 1) / splits;
    tiles_per = tiles_per > max_tiles ? max_tiles : tiles_per;
    if (tiles_per_out) *tiles_per_out = tiles_per;
    return (col_tiles + tiles_per - 1) / tiles_per;
}

}  // namespace cslgan
