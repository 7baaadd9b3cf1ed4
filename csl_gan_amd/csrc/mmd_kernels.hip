// Kernel two-sample test kernels for gfx950 (csl_gan_amd.kernel_test; DESIGN.md §6s, include/cslgan.h "Kernel two-sample test").
//
// Three passes over the stored squared-distance matrix of gram_d2_u8_kernel (svm_kernels.hip): a radix histogram of the entries above the
// diagonal (the median in four calls), the fixed-point Gaussian kernel matrix Kq written over it, and the sums of Kq over the two sides
// of P partitions at once — r = Kq member^T on the int8 matrix instruction, Kq cut into four byte limbs while it is staged.  Every
// figure is an exact integer; the one floating-point expression (a float64 product, a power-of-two scale, round-half-even) has no sum in
// it: nothing in this file may be contracted into a fused multiply-add.
#include "nn_tile.h"

#pragma clang fp contract(off)

namespace cslgan {

constexpr long long MMD_MAX_ROWS = 65536;                      // the stored matrix of gram_d2_u8: a 16 GiB matrix
constexpr int MMD_MAX_B = 7;                                   // 7 * 2^28 < 2^31
constexpr long long MMD_MAX_P = 1ll << 20;                     // partitions of one launch
constexpr int MMD_TABLE = 65536;                               // entries of one exp table
constexpr int MMD_TM = 64, MMD_TN = 128;                       // rows of Kq x partitions per workgroup tile: 2 x 2 waves of 32 x 64
constexpr int MMD_LIMBS = 4;                                   // bytes of an entry, each shifted by 128 into int8

// ---- the histogram of one radix digit above the diagonal ---------------------------------------------------------------------------
// One wave per row and pass of the grid-stride loop: 16 bytes per lane from the 16-byte group that holds column i + 1 on, entries with
// i < j < n only.  The digits of one row are mostly equal (the top byte of a squared distance in the first call): when the whole wave
// agrees on one bin its first lane adds the count, otherwise every lane adds 1 in LDS.  The 256 counters of the workgroup (below 2^32:
// the whole triangle has fewer than 2^31 entries) leave as one 64-bit atomic add each.
__device__ __forceinline__ void mmd_hist_add(unsigned* h, bool on, unsigned bin, int lane) {
    const unsigned key = on ? bin : 256u;
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
    const unsigned long long same = __ballot(key == first);
    if (same == ~0ull) {                                       // the loop's trip count is uniform: all 64 lanes are here
        if (lane == 0 && first < 256u) atomicAdd(&h[first], 64u);
    } else if (on) {
        atomicAdd(&h[bin], 1u);
    }
}

__global__ __launch_bounds__(256) void tri_hist_u32_kernel(const uint32_t* __restrict__ d2, long long pitch, int n, uint32_t prefix, int prefix_bits,
                                                           unsigned long long* __restrict__ hist) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    h[tid] = 0;
    __syncthreads();
    const int hi_shift = 32 - prefix_bits;                     // 32 with no prefix: the comparison is then skipped
    const int bin_shift = 24 - prefix_bits;
    const uint32_t want = prefix_bits ? prefix >> hi_shift : 0u;
    for (long long i = (long long)blockIdx.x * 4 + w; i < n - 1; i += (long long)gridDim.x * 4) {
        const uint32_t* __restrict__ row = d2 + i * pitch;
        const int j_first = (int)((i + 1) & ~3ll);
        for (int j0 = j_first; j0 < n; j0 += 256) {            // uniform over the wave
            const int j = j0 + 4 * lane;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (j < n) v = *reinterpret_cast<const u32x4*>(row + j);       // j + 3 < pitch: pitch is a multiple of 4, not below n
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool on = j + k > i && j + k < n && (prefix_bits == 0 || (e[k] >> hi_shift) == want);
                mmd_hist_add(h, on, (e[k] >> bin_shift) & 255u, lane);
            }
        }
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&hist[tid], (unsigned long long)h[tid]);
}

// ---- Kq over d2 ----------------------------------------------------------------------------------------------------------------------
// Kq = sum_b rint(2^28 (hi_b[d2 >> 16] lo_b[d2 & 65535])) off the diagonal, 0 on it: per bandwidth one float64 product, one exact
// scaling and v_rndne_f64, then integers.  Elementwise and in place, four columns per thread, the columns up to the pitch included
// (whatever they hold indexes the tables in range, and nobody reads the result).
__global__ __launch_bounds__(256) void mmd_kernel_u32_kernel(uint32_t* __restrict__ d2, long long pitch, int n, const double* __restrict__ hi,
                                                            const double* __restrict__ lo, int B) {
    const long long groups = pitch / 4;
    const long long total = (long long)n * groups;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const long long i = g / groups;
        const long long j = (g - i * groups) * 4;
        u32x4* p = reinterpret_cast<u32x4*>(d2 + i * pitch + j);
        const u32x4 v = *p;
        const uint32_t e[4] = {v.x, v.y, v.z, v.w};
        uint32_t out[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t s = 0;
            for (int b = 0; b < B; ++b) {
                const double prod = hi[(long long)b * MMD_TABLE + (e[k] >> 16)] * lo[(long long)b * MMD_TABLE + (e[k] & 65535u)];
                s += (uint32_t)rint(prod * 268435456.0);
            }
            out[k] = (j + k == i) ? 0u : s;
        }
        const u32x4 o = {out[0], out[1], out[2], out[3]};
        *p = o;
    }
}

// ---- the partition sums --------------------------------------------------------------------------------------------------------------
// r[i, p] = sum_j Kq[i, j] member[p, j].  Workgroup (bx, by): partitions 128 bx .., rows 64 by .. of Kq, the whole K range of
// ceil(n / 64) stages of 64 columns.  The partition tile is the FAST grid index, so the workgroups that share 64 rows of Kq run side by
// side and the matrix comes from HBM once; member (P x ldm bytes) is re-read per row tile out of the caches.
//
// Kq's bytes b_l (entry = sum_l b_l 256^l) become int8 as a_l = b_l - 128 while a stage goes from registers to LDS: a 16-byte load
// holds four entries of one row, whose l-th bytes make one dword of limb plane l.  An entry of a column >= n or a row >= n is staged
// as 0.  The four planes are the A operand and member, K-contiguous as stored, the B operand, read with one lane -> k assignment
// (nn_tile.h), so with cnt_p = sum_j member[p, j] over the staged columns
//     r = sum_l 256^l (acc_l + 128 cnt_p) = sum_l 256^l acc_l + 0x80808080 cnt_p,     |acc_l| <= 65536 * 128 * 128 = 2^30.
// cnt_p costs no matrix instruction: the thread that stages 16 bytes of member row p in every stage sums them (v_sad_u8 on the bytes
// xor 0x80), and the four threads of a row meet in LDS after the loop.  The epilogue recombines the limbs to int64 once, adds each lane's
// 16 rows into the side that member[p, i] names, folds the two row halves of a wave by a lane shuffle and the two waves of a column
// through LDS, and leaves with two 64-bit atomic adds per partition: exact, so their order does not matter.
__global__ __launch_bounds__(NN_THREADS, 2) void mmd_partition_sums_i64_kernel(const uint32_t* __restrict__ kq, long long pitch, int n,
                                                                             const signed char* __restrict__ member, long long ldm,
                                                                             long long P, unsigned long long* __restrict__ sxx2,
                                                                             unsigned long long* __restrict__ sxy) {
    __shared__ __attribute__((aligned(16))) unsigned char sA[2][MMD_LIMBS][MMD_TM * NN_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char sB[2][MMD_TN * NN_PITCH];
    __shared__ int cnt_s[MMD_TN];
    __shared__ long long fold_s[2][MMD_TN];

    const int tid = threadIdx.x;
    const int lane31 = tid & 31, lh = (tid >> 5) & 1, wn = (tid >> 6) & 1, wm = tid >> 7;
    const long long p0 = (long long)blockIdx.x * MMD_TN;
    const long long row0 = (long long)blockIdx.y * MMD_TM;
    const int nk = (n + NN_KT - 1) / NN_KT;

    // A: four 16-byte loads per thread and stage, (row, 4 columns) = (id >> 4, id & 15) of id = tid + 256 s
    const int a_row = tid >> 4, a_c4 = (tid & 15) * 4;
    // B: the staging of nn_tile_loop: rows tid >> 2 and + 64, 16 bytes each, behind a range-checked descriptor over the rows < P
    const int rows_here = (int)(P - p0 < MMD_TN ? P - p0 : MMD_TN);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(member + p0 * ldm, (unsigned)rows_here * (unsigned)ldm);
    const int b_row = tid >> 2, b_chunk = (tid & 3) * 16;
    const unsigned b_off = (unsigned)b_row * (unsigned)ldm + (unsigned)b_chunk;
    const unsigned b_off2 = b_off + 64u * (unsigned)ldm;
    const int b_st = b_row * NN_PITCH + b_chunk;

    u32x4 ga[4], gb0, gb1;
    int cnt0 = 0, cnt1 = 0;                                    // of member rows b_row and b_row + 64, this thread's 16 bytes per stage
    auto fetch = [&](int kt) {
        const int k0 = kt * NN_KT;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long long r = row0 + a_row + 16 * s;
            const int j = k0 + a_c4;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (r < n && j < n) v = *reinterpret_cast<const u32x4*>(kq + r * pitch + j);      // j + 3 < pitch
            if (j + 1 >= n) v.y = 0u;
            if (j + 2 >= n) v.z = 0u;
            if (j + 3 >= n) v.w = 0u;
            ga[s] = v;
        }
        gb0 = buf_load4_raw(rb, b_off + (unsigned)k0);
        gb1 = buf_load4_raw(rb, b_off2 + (unsigned)k0);
    };
    auto byte_sum = [](const u32x4& v) {                       // of 16 signed bytes
        unsigned s = __builtin_amdgcn_sad_u8(v.x ^ 0x80808080u, 0u, 0u);
        s = __builtin_amdgcn_sad_u8(v.y ^ 0x80808080u, 0u, s);
        s = __builtin_amdgcn_sad_u8(v.z ^ 0x80808080u, 0u, s);
        s = __builtin_amdgcn_sad_u8(v.w ^ 0x80808080u, 0u, s);
        return (int)s - 16 * 128;
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t w0 = ga[s].x, w1 = ga[s].y, w2 = ga[s].z, w3 = ga[s].w;
            const int off = (a_row + 16 * s) * NN_PITCH + a_c4;
#pragma unroll
            for (int l = 0; l < MMD_LIMBS; ++l) {
                const uint32_t plane = ((w0 >> (8 * l)) & 0xffu) | (((w1 >> (8 * l)) & 0xffu) << 8) | (((w2 >> (8 * l)) & 0xffu) << 16) |
                                       (((w3 >> (8 * l)) & 0xffu) << 24);
                *reinterpret_cast<uint32_t*>(&sA[buf][l][off]) = plane ^ 0x80808080u;
            }
        }
        *reinterpret_cast<u32x4*>(&sB[buf][b_st]) = gb0;
        *reinterpret_cast<u32x4*>(&sB[buf][b_st + 64 * NN_PITCH]) = gb1;
        cnt0 += byte_sum(gb0);
        cnt1 += byte_sum(gb1);
    };

    i32x16 acc[MMD_LIMBS][2];
#pragma unroll
    for (int l = 0; l < MMD_LIMBS; ++l)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[l][nt][i] = 0;

    fetch(0);                                                  // nk >= 1: n >= 1
    stash(0);
    __syncthreads();

    const int a_off = (wm * 32 + lane31) * NN_PITCH + 16 * lh;
    const int bb_off = (wn * 64 + lane31) * NN_PITCH + 16 * lh;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
        for (int ks = 0; ks < NN_KT / 32; ++ks) {
            i32x4 b[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) b[nt] = *reinterpret_cast<const i32x4*>(&sB[buf][bb_off + nt * 32 * NN_PITCH + ks * 32]);
#pragma unroll
            for (int l = 0; l < MMD_LIMBS; ++l) {
                const i32x4 a = *reinterpret_cast<const i32x4*>(&sA[buf][l][a_off + ks * 32]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[l][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[nt], acc[l][nt], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) stash(buf ^ 1);                       // last read in iteration kt - 1, which every wave has left
        __syncthreads();
    }

    // cnt_p: the four threads of a member row are neighbours in one wave
    cnt0 += __shfl_xor(cnt0, 1, 64);
    cnt0 += __shfl_xor(cnt0, 2, 64);
    cnt1 += __shfl_xor(cnt1, 1, 64);
    cnt1 += __shfl_xor(cnt1, 2, 64);
    if ((tid & 3) == 0) {
        cnt_s[b_row] = cnt0;
        cnt_s[b_row + 64] = cnt1;
    }
    __syncthreads();

#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int pc = wn * 64 + nt * 32 + lane31;             // column of the tile
        const long long p = p0 + pc;
        const bool live = p < P;
        const long long bias = (long long)cnt_s[pc] * 0x80808080ll;
        long long xx = 0, xy = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {                          // registers 4 g .. 4 g + 3: rows 8 g + 4 lh + 0 .. 3, four bytes of member row p;
                                                               // a row >= n was staged as zeros: its r is 0 whatever member holds there
            const long long i0 = row0 + wm * 32 + 8 * g + 4 * lh;          // < 64 ceil(n / 64) <= ldm
            const uint32_t m4 = live ? *reinterpret_cast<const uint32_t*>(member + p * ldm + i0) : 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = 4 * g + k;
                long long r = bias;
#pragma unroll
                for (int l = 0; l < MMD_LIMBS; ++l) r += (long long)acc[l][nt][i] * (1ll << (8 * l));
                if ((m4 >> (8 * k)) & 0xffu)
                    xx += r;
                else
                    xy += r;
            }
        }
        xx += __shfl_xor(xx, 32, 64);                          // the two row halves of the 32 x 32 block
        xy += __shfl_xor(xy, 32, 64);
        if (wm == 1 && lh == 0) {
            fold_s[0][pc] = xx;
            fold_s[1][pc] = xy;
        }
        __syncthreads();                                       // uniform: nt is
        if (wm == 0 && lh == 0 && live) {
            xx += fold_s[0][pc];
            xy += fold_s[1][pc];
            if (xx) atomicAdd(&sxx2[p], (unsigned long long)xx);
            if (xy) atomicAdd(&sxy[p], (unsigned long long)xy);
        }
        __syncthreads();
    }
}

static int mmd_check_matrix(const char* entry, const void* m, int64_t pitch, int64_t n) {
    CSLGAN_REQUIRE(n >= 1 && n <= MMD_MAX_ROWS, "%s: n=%lld rows; the stored matrix takes 1 .. %lld (16 GiB)", entry, (long long)n, MMD_MAX_ROWS);
    CSLGAN_REQUIRE(pitch >= n && pitch % 32 == 0 && pitch <= MMD_MAX_ROWS, "%s: pitch=%lld must be a multiple of 32 in n .. %lld", entry,
                   (long long)pitch, MMD_MAX_ROWS);
    CSLGAN_REQUIRE(aligned_to(m, 128), "%s: misaligned pointer", entry);
    return CSLGAN_OK;
}

}  // namespace cslgan

using namespace cslgan;

extern "C" {

int cslgan_tri_hist_u32(const uint32_t* d2, int64_t pitch, int64_t n, uint32_t prefix, int prefix_bits, int64_t* hist, void* stream) {
    CSLGAN_REQUIRE(d2 && hist, "tri_hist_u32: null argument");
    if (int rc = mmd_check_matrix("tri_hist_u32", d2, pitch, n)) return rc;
    CSLGAN_REQUIRE(prefix_bits == 0 || prefix_bits == 8 || prefix_bits == 16 || prefix_bits == 24,
                   "tri_hist_u32: prefix_bits=%d must be 0, 8, 16 or 24", prefix_bits);
    CSLGAN_REQUIRE(aligned_to(hist, 8), "tri_hist_u32: misaligned pointer");
    long long blocks = (n + 3) / 4;
    blocks = blocks > 4096 ? 4096 : blocks;
    note_kernel("tri_hist_u32_kernel");
    hipLaunchKernelGGL(tri_hist_u32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d2, (long long)pitch, (int)n, prefix,
                       prefix_bits, (unsigned long long*)hist);
    return check_launch("tri_hist_u32_kernel");
}

int cslgan_mmd_kernel_u32(uint32_t* d2, int64_t pitch, int64_t n, const double* hi, const double* lo, int B, void* stream) {
    CSLGAN_REQUIRE(d2 && hi && lo, "mmd_kernel_u32: null argument");
    if (int rc = mmd_check_matrix("mmd_kernel_u32", d2, pitch, n)) return rc;
    CSLGAN_REQUIRE(B >= 1 && B <= MMD_MAX_B, "mmd_kernel_u32: B=%d bandwidths; 1 .. %d keep the sum below 2^31", B, MMD_MAX_B);
    CSLGAN_REQUIRE(aligned_to(hi, 8) && aligned_to(lo, 8), "mmd_kernel_u32: misaligned pointer");
    note_kernel("mmd_kernel_u32_kernel");
    hipLaunchKernelGGL(mmd_kernel_u32_kernel, dim3(grid_for((long long)n * (pitch / 4)) * 4), dim3(256), 0, (hipStream_t)stream, d2,
                       (long long)pitch, (int)n, hi, lo, B);
    return check_launch("mmd_kernel_u32_kernel");
}

int cslgan_mmd_partition_sums_i64(const uint32_t* kq, int64_t pitch, int64_t n, const int8_t* member, int64_t ldm, int64_t P, int64_t* sxx2,
                                  int64_t* sxy, void* stream) {
    CSLGAN_REQUIRE(kq && member && sxx2 && sxy, "mmd_partition_sums_i64: null argument");
    if (int rc = mmd_check_matrix("mmd_partition_sums_i64", kq, pitch, n)) return rc;
    CSLGAN_REQUIRE(ldm >= n && ldm % NN_KT == 0 && ldm <= MMD_MAX_ROWS, "mmd_partition_sums_i64: ldm=%lld must be a multiple of %d in n .. %lld",
                   (long long)ldm, NN_KT, MMD_MAX_ROWS);
    CSLGAN_REQUIRE(P >= 1 && P <= MMD_MAX_P, "mmd_partition_sums_i64: P=%lld partitions; a launch takes 1 .. %lld", (long long)P, MMD_MAX_P);
    CSLGAN_REQUIRE(aligned16(member) && aligned_to(sxx2, 8) && aligned_to(sxy, 8), "mmd_partition_sums_i64: misaligned pointer");
    note_kernel("mmd_partition_sums_i64_kernel");
    hipLaunchKernelGGL(mmd_partition_sums_i64_kernel, dim3((unsigned)((P + MMD_TN - 1) / MMD_TN), (unsigned)((n + MMD_TM - 1) / MMD_TM)),
                       dim3(NN_THREADS), 0, (hipStream_t)stream, kq, (long long)pitch, (int)n, (const signed char*)member, (long long)ldm,
                       (long long)P, (unsigned long long*)sxx2, (unsigned long long*)sxy);
    return check_launch("mmd_partition_sums_i64_kernel");
}

}  // extern "C"
