// Host-side geometry shared by the conv entry points: how a cslgan_conv_t becomes tap tables and tap classes (igemm.h: KcClass).
// Plain functions over the existing structs; nothing here runs on the device.
#pragma once
#include "igemm.h"

namespace cslgan {

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
