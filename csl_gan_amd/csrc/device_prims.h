// Device primitives shared by every HIP kernel of libcslgan_hip.so (gfx950 only): vector types, range-checked buffer
// loads, the two bfloat16 rounding forms, the three-piece fp32 split, depth-to-space addressing and the epilogue pieces.  Included after common.h.
// One definition each: a fix made here reaches every kernel.
#pragma once
#include "common.h"

namespace cslgan {

// ---- vector types -----------------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;      // operand of the transposing LDS reads (ds_read_b64_tr_b16)

// ---- range-checked buffer access --------------------------------------------------------------------------------------------
// A byte offset at or beyond the descriptor's byte count returns 0, so padding taps, ragged rows and the K tail need neither
// a branch nor a select — the loader is straight-line code that the scheduler can interleave with MFMAs.  32-bit byte
// offsets (tensors are < 4 GB; the hosts check their operand sizes against BUF_OOB).  BUF_OOB is the offset that is out of
// range for every such tensor; its low four bits are clear, so OR-ing it into a 16-byte aligned offset keeps the alignment.
constexpr unsigned BUF_OOB = 0xFFFFFFF0u;

// Raw buffer descriptor over [base, base + bytes).  0x00020000 is the descriptor's fourth word: DATA_FORMAT = 32-bit (the gfx9
// encoding, bits 15..18 = 4) and every other field zero — no swizzle, no index stride, no added TID.  With stride 0 the
// hardware range-checks the byte offset against NUM_RECORDS (= bytes) and a read that fails returns zero instead of faulting.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ u32x4 buf_load4_raw(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0);
}
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    const u32x4 v = buf_load4_raw(r, byte_off);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}

// ---- bfloat16 conversion ----------------------------------------------------------------------------------------------------
// Two round-to-nearest-even forms exist and both stay: results agree on finite inputs, the instruction streams do not.
// Convert-instruction form (v_cvt_pk_bf16_f32; lo in bits 0..15):
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ unsigned short bf16_rne(float x) { return (unsigned short)(pack_bf16(x, 0.f) & 0xffffu); }
__device__ __forceinline__ uint2 pack4_bf16(const float4& v) { return make_uint2(pack_bf16(v.x, v.y), pack_bf16(v.z, v.w)); }
// Integer-arithmetic form: the float's bits with the rounding increment added; the bfloat16 is the upper half.
__device__ __forceinline__ unsigned rne_bf16_bits(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u;
}
__device__ __forceinline__ unsigned rne_bf16(float f) { return rne_bf16_bits(f) >> 16; }

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }             // low / high half of a packed pair
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float bf2f(unsigned short u) { return __uint_as_float((unsigned)u << 16); }

// ---- fp32 from three bfloat16 pieces ---------------------------------------------------------------------------------------
// x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): three 8-bit mantissas cover fp32's 24 bits
// (|x - hi - mid - lo| <= 2^-24 |x|).  A product a*b is then the sum of 9 piece products, each EXACT in fp32 (8 x 8 bits);
// dropping the three smallest (mid*lo, lo*mid, lo*lo: <= 2^-23 |a||b| together) leaves SIX bf16 MFMAs per fp32 MFMA step:
//     a*b ~= hi*hi + (hi*mid + mid*hi) + (hi*lo + lo*hi + mid*mid)
// at 16x the fp32 MFMA rate each — 2.67x the fp32 matrix rate for a per-product error of about one fp32 ulp
// (CSLGAN_COMPUTE_BF16X3; the same construction vendor BLAS libraries ship as "fp32 emulation").  Small terms are added first.
struct bf16x3_t { uint2 hi, mid, lo; };
__device__ __forceinline__ bf16x3_t split4_bf16(const float4& v) {
    bf16x3_t r;
    r.hi = make_uint2(pack_bf16(v.x, v.y), pack_bf16(v.z, v.w));
    const float r0 = v.x - bf_lo(r.hi.x), r1 = v.y - bf_hi(r.hi.x), r2 = v.z - bf_lo(r.hi.y), r3 = v.w - bf_hi(r.hi.y);   // exact
    r.mid = make_uint2(pack_bf16(r0, r1), pack_bf16(r2, r3));
    r.lo = make_uint2(pack_bf16(r0 - bf_lo(r.mid.x), r1 - bf_hi(r.mid.x)), pack_bf16(r2 - bf_lo(r.mid.y), r3 - bf_hi(r.mid.y)));
    return r;
}

// ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------------
// The counter-based generator of every device random stream (include/cslgan.h "Device random streams"): Random123's
// philox4x32_R(10, ...), counter (c0..c3), key (k0, k1), four 32-bit words out.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- depth-to-space addressing ----------------------------------------------------------------------------------------------
// Depth-to-space addressing of UpsampleConv (DCResNet_models.py:13-15): cat([x]*4, dim=1) + pixel_shuffle(2) gives
// up[c][2h+i][2w+j] = x[(4c+2i+j) mod C][h][w], i.e. for C % 4 == 0 the C output channels are the C/4 channels of the
// plain depth-to-space tensor  ps[n][2h+i][2w+j][c'] = x[n][h][w][4c'+2i+j]  repeated four times (the conv that follows
// runs on ps with its filter summed over the four channel groups, cslgan_fold_channels4_f32).  Element (row r, channel
// 4c'+p) of x[N*H*W][C] lands at ps offset d2s_offset(r, p) + c'.
__device__ __forceinline__ long long d2s_offset(long long r, int p, int H, int W, int Cq) {
    const int w = (int)(r % W);
    const long long t = r / W;
    const int h = (int)(t % H);
    const long long n = t / H;
    return ((n * 2 * H + 2 * h + (p >> 1)) * 2 * W + 2 * w + (p & 1)) * Cq;
}

// ---- epilogue pieces --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == CSLGAN_ACT_LRELU02) v = v > 0.f ? v : 0.2f * v;
    else if (act == CSLGAN_ACT_RELU) v = v > 0.f ? v : 0.f;
    else if (act == CSLGAN_ACT_TANH) v = tanhf(v);
    return v;
}
// The float4 form tests the activation once per vector (the shape of the LDS-halo kernels' epilogues).
__device__ __forceinline__ void apply_act4(float4& v, int act) {
    if (act == CSLGAN_ACT_LRELU02) {
        v.x = v.x > 0.f ? v.x : 0.2f * v.x; v.y = v.y > 0.f ? v.y : 0.2f * v.y; v.z = v.z > 0.f ? v.z : 0.2f * v.z; v.w = v.w > 0.f ? v.w : 0.2f * v.w;
    } else if (act == CSLGAN_ACT_RELU) {
        v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
    } else if (act == CSLGAN_ACT_TANH) {
        v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w);
    }
}
// Data gradient of LeakyReLU(0.2) applied from the saved forward output m: v where m > 0, 0.2 v elsewhere.
__device__ __forceinline__ float lrelu_mask(float v, float m) { return v * (m > 0.f ? 1.f : 0.2f); }

}  // namespace cslgan
