// Byte-moment kernels for gfx950 (csl_gan_amd.moments; DESIGN.md §6r, include/cslgan.h "Byte moments").
//
// Exact integer first and second moments of the columns of a uint8 image cache: the TRANSPOSED operand image xt = (x - 128)^T as int8
// with zero padding along the rows of the cache, its row sums as int64, and the Gram matrix xt xt^T — a product that sums over the ROWS of
// the cache — on the int8 matrix instruction through the tile loop of nn_tile.h, xt as both operands, the tiles on and below the diagonal
// only.  Nothing in this file waits for another workgroup and every output element has one writer per launch.
#include "common.h"
#include "device_prims.h"
#include "nn_tile.h"

namespace cslgan {

constexpr int MOM_MAX_N = 65536;                   // rows per call: the reduction length of the Gram product, |acc| <= 65536 * 2^14 = 2^30
constexpr int MOM_TI = 256, MOM_TJ = 64;           // rows x columns of x per transpose workgroup
constexpr int MOM_PITCH = MOM_TI / 4 + 1;          // LDS row pitch in dwords: odd, so the 32 lanes of a store group (32 columns) hit 32 banks

// ---- transpose: uint8 [n, D] -> int8 [D, np], xt[j][i] = x[i][j] - 128, zero for n <= i < np ---------------------------------------------
// Workgroup (bx, by): rows 256 bx .. of x, columns 64 by ...  A thread owns one column and packs the bytes of four consecutive rows
// into a dword (a wave reads 64 consecutive bytes of one row per load: rows of x start at any byte, so the loads are single bytes),
// stores it to the LDS tile [column][row / 4], and the tile leaves as 16-byte stores, 16 lanes per 256-byte run of an xt row.  A byte
// of a row >= n reads as 128 (zero after the shift); a row >= np or a column >= D is neither read nor written.
__global__ __launch_bounds__(256) void mom_transpose_u8_kernel(const unsigned char* __restrict__ x, int n, int D, int np,
                                                               signed char* __restrict__ xt) {
    __shared__ unsigned tile[MOM_TJ * MOM_PITCH];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * MOM_TI, j0 = blockIdx.y * MOM_TJ;
    const int tj = tid & 63, q = tid >> 6;
    const int j = j0 + tj;
#pragma unroll 4
    for (int r = 0; r < MOM_TI / 16; ++r) {                    // rows i0 + 64 q + 4 r .. + 3
        const int i = i0 + 64 * q + 4 * r;
        unsigned v = 0x80808080u;
        if (j < D) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < n) v = (v & ~(0xffu << (8 * k))) | ((unsigned)x[(long long)(i + k) * D + j] << (8 * k));
        }
        tile[tj * MOM_PITCH + 16 * q + r] = v ^ 0x80808080u;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MOM_TJ * (MOM_TI / 16) / 256; ++s) {   // 1024 chunks of 16 bytes
        const int id = tid + 256 * s;
        const int row = id >> 4, c = id & 15;
        const int i = i0 + 16 * c;
        if (j0 + row < D && i < np) {                          // np is a multiple of 64: a chunk lies inside a row of xt or behind it
            const unsigned* t = &tile[row * MOM_PITCH + 4 * c];
            const u32x4 out = {t[0], t[1], t[2], t[3]};
            *reinterpret_cast<u32x4*>(xt + (long long)(j0 + row) * np + i) = out;
        }
    }
}

// ---- column sums: s1[j] += sum_i xt[j][i] ----------------------------------------------------------------------------------------------
// One wave per row of xt, 16 bytes per lane and step, int32 per lane (at most 65536 / 64 * 128 < 2^31), reduced over the wave; lane 0
// is the ONE writer of s1[j]: a plain 8-byte load / add / store.
__global__ __launch_bounds__(256) void mom_colsum_i64_kernel(const signed char* __restrict__ xt, int D, int np, long long* __restrict__ s1) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
    if (j >= D) return;                                        // whole waves leave: no barrier follows
    const u32x4* __restrict__ row = reinterpret_cast<const u32x4*>(xt + (long long)j * np);
    int acc = 0;
    for (int c = lane; c < np / 16; c += WAVE) {
        const u32x4 v = row[c];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            acc += ((int)(w[k] << 24) >> 24) + ((int)(w[k] << 16) >> 24) + ((int)(w[k] << 8) >> 24) + ((int)w[k] >> 24);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) s1[j] += (long long)acc;
}

// ---- Gram: S2[i][j] += xt[i] . xt[j] for the 128 x 128 tiles on and below the diagonal ----------------------------------------------------
// Workgroup (bx, by) of row tile bx sees bx + 1 column tiles and nr = min(D, 128 (bx + 1)) columns: the triangle.  A workgroup whose range
// of column tiles starts behind the diagonal runs no iteration.  Every element of the triangle has one writer per launch, and the launches
// of one stream are ordered: the int32 accumulator (|acc| <= 2^30) is added by a plain 8-byte load / add / store.  The loop hands the
// epilogue the 16 registers of a 32 x 32 block one after the other, all of one column: the 16 old values are loaded at the first of them,
// so a block costs one trip to memory, not sixteen in a row (a store followed by the next load of the same array cannot be reordered).
// Two workgroups per CU as for the other kernels of the tile loop: unbounded, the 16 values and their addresses take the kernel past 256
// registers and to one workgroup per CU.
__global__ __launch_bounds__(NN_THREADS, 2) void mom_gram_i64_kernel(const signed char* __restrict__ xt, int D, int np, int tiles_per,
                                                                  long long* __restrict__ S2, long long ld) {
    const NNLane ln(threadIdx.x);
    const long long row0 = (long long)blockIdx.x * NN_TM;
    const int n_col_tiles = (int)blockIdx.x + 1;
    const int nr = D < NN_TN * n_col_tiles ? D : NN_TN * n_col_tiles;
    long long old[16];
    nn_tile_loop<true>(xt, nullptr, D, xt, nullptr, nr, np, tiles_per, n_col_tiles, NNNoColumn(),
                       [&](int mt, int i, bool live, long long col, uint32_t dot) {
                           if (i == 0) {
#pragma unroll
                               for (int k = 0; k < 16; ++k) {
                                   const long long r = row0 + ln.row(mt, k);
                                   old[k] = (live && r < D) ? S2[r * ld + col] : 0;
                               }
                           }
                           const long long row = row0 + ln.row(mt, i);
                           if (live && row < D) S2[row * ld + col] = old[i] + (long long)(int)dot;
                       });
}

// ---- mirror: S2[i][j] = S2[j][i] for the tiles strictly above the diagonal ---------------------------------------------------------------
// Workgroup (bx, by): the 32 x 32 block of rows 32 by .., columns 32 bx .. of S2, which lies inside ONE 128 x 128 tile; it is filled from
// its transposed block when its tile is above the diagonal.  The source tiles (below the diagonal) are never written here.
__global__ __launch_bounds__(256) void mom_mirror_i64_kernel(long long* __restrict__ S2, int D, long long ld) {
    __shared__ long long t[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;
    if ((bx >> 2) <= (by >> 2)) return;                        // uniform over the workgroup
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 32 * bx + ty + 8 * k, c = 32 * by + tx;  // the source: row in the column range of the destination
        if (r < D && c < D) t[ty + 8 * k][tx] = S2[(long long)r * ld + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 32 * by + ty + 8 * k, c = 32 * bx + tx;
        if (r < D && c < D) S2[(long long)r * ld + c] = t[tx][ty + 8 * k];
    }
}

static long long mom_padded_rows(int64_t n) { return (n + NN_KT - 1) / NN_KT * NN_KT; }

static int mom_check_image(const char* entry, const void* xt, int D, int64_t np) {
    CSLGAN_REQUIRE(D >= 1 && D <= NN_MAX_D, "%s: D=%d must lie in 1 .. %d", entry, D, NN_MAX_D);
    CSLGAN_REQUIRE(np >= NN_KT && np <= MOM_MAX_N && np % NN_KT == 0, "%s: np=%lld must be a multiple of %d in %d .. %d", entry, (long long)np,
                   NN_KT, NN_KT, MOM_MAX_N);
    CSLGAN_REQUIRE(aligned16(xt), "%s: misaligned pointer", entry);
    return CSLGAN_OK;
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_mom_transpose_u8(const void* x, int64_t n, int D, int64_t np, void* xt, void* stream) {
    CSLGAN_REQUIRE(x && xt, "mom_transpose_u8: null argument");
    CSLGAN_REQUIRE(D >= 1 && D <= NN_MAX_D, "mom_transpose_u8: D=%d must lie in 1 .. %d", D, NN_MAX_D);
    CSLGAN_REQUIRE(n >= 1 && n <= MOM_MAX_N, "mom_transpose_u8: n=%lld must lie in 1 .. %d", (long long)n, MOM_MAX_N);
    CSLGAN_REQUIRE(np == mom_padded_rows(n), "mom_transpose_u8: np=%lld is not the padded width %lld of n=%lld", (long long)np,
                   mom_padded_rows(n), (long long)n);
    CSLGAN_REQUIRE(aligned16(xt), "mom_transpose_u8: misaligned pointer");
    note_kernel("mom_transpose_u8_kernel");
    hipLaunchKernelGGL(mom_transpose_u8_kernel, dim3((unsigned)((np + MOM_TI - 1) / MOM_TI), (unsigned)((D + MOM_TJ - 1) / MOM_TJ)), dim3(256), 0,
                       (hipStream_t)stream, (const unsigned char*)x, (int)n, D, (int)np, (signed char*)xt);
    return check_launch("mom_transpose_u8_kernel");
}

int cslgan_mom_colsum_i64(const void* xt, int D, int64_t np, int64_t* s1, void* stream) {
    CSLGAN_REQUIRE(xt && s1, "mom_colsum_i64: null argument");
    if (int rc = mom_check_image("mom_colsum_i64", xt, D, np)) return rc;
    CSLGAN_REQUIRE(aligned_to(s1, 8), "mom_colsum_i64: misaligned pointer");
    note_kernel("mom_colsum_i64_kernel");
    const int rows_per_wg = 256 / WAVE;
    hipLaunchKernelGGL(mom_colsum_i64_kernel, dim3((unsigned)((D + rows_per_wg - 1) / rows_per_wg)), dim3(256), 0, (hipStream_t)stream,
                       (const signed char*)xt, D, (int)np, (long long*)s1);
    return check_launch("mom_colsum_i64_kernel");
}

int cslgan_mom_gram_i64(const void* xt, int D, int64_t np, int64_t* S2, int64_t ld, void* stream) {
    CSLGAN_REQUIRE(xt && S2, "mom_gram_i64: null argument");
    if (int rc = mom_check_image("mom_gram_i64", xt, D, np)) return rc;
    CSLGAN_REQUIRE(ld >= D && ld < (1ll << 40), "mom_gram_i64: ld=%lld is smaller than D=%d (or out of range)", (long long)ld, D);
    CSLGAN_REQUIRE(aligned_to(S2, 8), "mom_gram_i64: misaligned pointer");
    // one column tile per workgroup, T x T workgroups of which those above the diagonal leave at once: the loop fetches both operands
    // for every tile, so a range of tiles would save no traffic, and single tiles balance the rows of the triangle (1 .. T tiles) best
    const long long T = (D + NN_TM - 1) / NN_TM;
    const long long tiles_per = 1;
    const long long gy = T;
    note_kernel("mom_gram_i64_kernel");
    hipLaunchKernelGGL(mom_gram_i64_kernel, dim3((unsigned)T, (unsigned)gy), dim3(NN_THREADS), 0, (hipStream_t)stream, (const signed char*)xt, D,
                       (int)np, (int)tiles_per, (long long*)S2, (long long)ld);
    return check_launch("mom_gram_i64_kernel");
}

int cslgan_mom_mirror_i64(int64_t* S2, int D, int64_t ld, void* stream) {
    CSLGAN_REQUIRE(S2, "mom_mirror_i64: null argument");
    CSLGAN_REQUIRE(D >= 1 && D <= NN_MAX_D, "mom_mirror_i64: D=%d must lie in 1 .. %d", D, NN_MAX_D);
    CSLGAN_REQUIRE(ld >= D && ld < (1ll << 40), "mom_mirror_i64: ld=%lld is smaller than D=%d (or out of range)", (long long)ld, D);
    CSLGAN_REQUIRE(aligned_to(S2, 8), "mom_mirror_i64: misaligned pointer");
    const unsigned g = (unsigned)((D + 31) / 32);
    note_kernel("mom_mirror_i64_kernel");
    hipLaunchKernelGGL(mom_mirror_i64_kernel, dim3(g, g), dim3(256), 0, (hipStream_t)stream, (long long*)S2, D, (long long)ld);
    return check_launch("mom_mirror_i64_kernel");
}

}  // extern "C"
