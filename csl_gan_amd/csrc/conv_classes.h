// Host-side geometry shared by the conv entry points: their argument check and how a cslgan_conv_t becomes tap tables and tap classes
// (igemm.h: KcClass).
// Plain functions over the existing structs; nothing here runs on the device.
#pragma once
#include "common.h"
#include "igemm.h"

namespace cslgan {

// Argument check of every conv entry; `who` prefixes the messages.  check_compute: cslgan_conv_t.compute must name a compute mode
// (the bf16-stored entries never read it and accept any value).
inline int check_conv(const cslgan_conv_t* c, const char* who, bool check_compute) {
    CSLGAN_REQUIRE(c->N > 0 && c->H > 0 && c->W > 0 && c->C > 0 && c->K > 0 && c->R > 0 && c->S > 0 && c->stride > 0 && c->pad >= 0,
                   "%s: non-positive dimension", who);
    CSLGAN_REQUIRE(c->R * c->S <= IG_MAX_TAPS, "%s: %dx%d filter has more than %d taps", who, c->R, c->S, IG_MAX_TAPS);
    CSLGAN_REQUIRE(!check_compute || (c->compute >= CSLGAN_COMPUTE_F32 && c->compute <= CSLGAN_COMPUTE_BF16X3), "%s: unknown cslgan_conv_t.compute %d", who, c->compute);
    const int P = (c->H + 2 * c->pad - c->R) / c->stride + 1, Q = (c->W + 2 * c->pad - c->S) / c->stride + 1;
    CSLGAN_REQUIRE(P == c->P && Q == c->Q, "%s: output %dx%d does not match P,Q=%d,%d", who, P, Q, c->P, c->Q);
    CSLGAN_REQUIRE((long long)c->N * c->P * c->Q * c->K < (1ll << 31) && (long long)c->N * c->H * c->W * c->C < (1ll << 31) &&
                   (long long)c->K * c->R * c->S * c->C < (1ll << 31), "%s: tensor too large for 32-bit offsets", who);
    return CSLGAN_OK;
}

// Tap table of a forward conv (and of a weight gradient, which walks the same window): tap t = kh*S + kw reads the input
// at offset (kh - pad, kw - pad).  Writes R*S entries; the tables sit in zero-initialised parameter structs.
inline void fill_forward_taps(signed char* ty, signed char* tx, int R, int S, int pad) {
    for (int kh = 0; kh < R; ++kh)
        for (int kw = 0; kw < S; ++kw) { ty[kh * S + kw] = (signed char)(kh - pad); tx[kh * S + kw] = (signed char)(kw - pad); }
}

// Filter tap (kh, kw) behind tap t of each data-gradient class, for the entry's filter repack.
struct ClassTaps {
    signed char kh[IG_MAX_CLS][IG_MAX_TAPS], kw[IG_MAX_CLS][IG_MAX_TAPS];
};

// Output-parity classes of a stride-s data gradient (s = 1, 2): class (py, px) owns the input pixels (s*i + py, s*j + px) and reads
// gy at offset ((py + pad - kh) / s, (px + pad - kw) / s) for every filter tap with kh == (py + pad) mod s, kw == (px + pad) mod s.
// Fills M, OHc, OWc, T, Kdim, w_off, oy0, ox0, ty, tx of cls[0..n) — w_off counts the elements of the consecutive [C][T][K] class
// matrices — and src with each tap's filter tap.  Returns n, or -1 when a class has no tap (filter smaller than the stride).
inline int build_dgrad_classes(const cslgan_conv_t* c, KcClass* cls, ClassTaps& src) {
    const int s = c->stride;
    int off = 0, n = 0;
    for (int py = 0; py < s; ++py)
        for (int px = 0; px < s; ++px) {
            const int OHc = (c->H - py + s - 1) / s, OWc = (c->W - px + s - 1) / s;
            if (OHc <= 0 || OWc <= 0) continue;
            KcClass& k = cls[n];
            int T = 0;
            for (int kh = 0; kh < c->R; ++kh) {
                if (((py + c->pad - kh) % s + s) % s != 0) continue;
                for (int kw = 0; kw < c->S; ++kw) {
                    if (((px + c->pad - kw) % s + s) % s != 0) continue;
                    src.kh[n][T] = (signed char)kh; src.kw[n][T] = (signed char)kw;
                    k.ty[T] = (signed char)((py + c->pad - kh) / s);
                    k.tx[T] = (signed char)((px + c->pad - kw) / s);
                    ++T;
                }
            }
            if (T == 0) return -1;
            k.M = c->N * OHc * OWc; k.OHc = OHc; k.OWc = OWc; k.T = T; k.Kdim = T * c->K; k.w_off = off; k.oy0 = py; k.ox0 = px;
            off += T * c->K * c->C;
            ++n;
        }
    return n;
}

// Split-K factor of a weight-gradient launch (McParams, or the bf16-stored MsParams of igemm_mcs.hip; tiles_m / tiles_n set): few
// workgroups with a long pixel loop (the 3-channel first layer: one 64x75 tile per sample, 1024+ pixels) split the pixels over
// workgroups that atomically add into the fp32 output, which is zeroed here.  bk: pixels per K tile; only from min_nk K tiles on, and
// at least tiles_per_split of them per workgroup.
template <typename P>
inline int wgrad_plan_split(P& p, int bk, int min_nk, int tiles_per_split, hipStream_t st) {
    const long long base = (long long)p.n_groups * p.tiles_m * p.tiles_n;
    const int nk_all = (p.group * p.P * p.Q + bk - 1) / bk;
    p.ksplit = 1;
    if (!p.gw || p.out_bf16 || base >= 192 || nk_all < min_nk) return CSLGAN_OK;
    const long long want = (512 + base - 1) / base, cap = nk_all / tiles_per_split;
    p.ksplit = (int)(want < cap ? want : cap);
    if (p.ksplit <= 1) { p.ksplit = 1; return CSLGAN_OK; }
    return zero_floats((float*)p.gw, (size_t)p.n_groups * p.Kc * p.Ndim, st);
}

// After a split launch the per-group norms need the completed sums: one pass of the contract norm kernel over the (small) result.
template <typename P>
inline int wgrad_split_norms(const P& p, hipStream_t st) {
    if (p.ksplit <= 1 || !p.sq) return CSLGAN_OK;
    return sqnorm_rows_accumulate((const float*)p.gw, p.n_groups, (long long)p.Kc * p.Ndim, p.sq, st);
}

// Range of a class's tap offsets: the halo of a patch is its side plus (max - min) in each direction.
inline void tap_range(const KcClass& k, int& ymin, int& ymax, int& xmin, int& xmax) {
    ymin = 127; ymax = -128; xmin = 127; xmax = -128;
    for (int t = 0; t < k.T; ++t) {
        ymin = k.ty[t] < ymin ? k.ty[t] : ymin; ymax = k.ty[t] > ymax ? k.ty[t] : ymax;
        xmin = k.tx[t] < xmin ? k.tx[t] : xmin; xmax = k.tx[t] > xmax ? k.tx[t] : xmax;
    }
}

// Four classes of equal row count and unequal tap count (9/6/6/4 taps of a 5x5 stride-2 data gradient): the heaviest class runs with
// the lightest in ONE workgroup (9+4, 6+6 K steps), so every workgroup carries the same number of K steps — as long as the halved
// grid (2 * tiles per class * n-tiles) still has pair_min workgroups.  Sets pair_mode, pair_cls, tiles_per_cls and tiles_m.
inline void pair_unequal_classes(KcParams& p, bool wide, int pair_min) {
    p.pair_mode = 0;
    if (p.acc_classes || p.n_cls != 4) return;
    bool same_m = true, same_t = true;
    for (int c = 1; c < p.n_cls; ++c) { same_m = same_m && p.cls[c].M == p.cls[0].M; same_t = same_t && p.cls[c].T == p.cls[0].T; }
    if (!same_m || same_t) return;
    const int tpc = (p.cls[0].M + 127) / 128;
    const long long paired = 2ll * tpc * (wide ? (p.Nn + 127) / 128 : (p.Nn + 63) / 64);
    if (paired < pair_min) return;
    int o[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (p.cls[o[j]].T > p.cls[o[i]].T) { const int t = o[i]; o[i] = o[j]; o[j] = t; }
    p.pair_mode = 1;
    p.pair_cls[0][0] = o[0]; p.pair_cls[0][1] = o[3];
    p.pair_cls[1][0] = o[1]; p.pair_cls[1][1] = o[2];
    p.tiles_per_cls = tpc;
    p.tiles_m = 2 * tpc;
}

}  // namespace cslgan
