"""Kernel two-sample test of two image caches (include/cslgan.h "Kernel two-sample test"): the unbiased squared maximum
mean discrepancy (Gretton et al. 2012) of the cache BYTES under a mean of Gaussian kernels, with a permutation p-value.

Z is the pool of n synthetic rows followed by m real rows, N = n + m <= 65536, and d2 its exact squared-distance matrix (svm.gram_d2_host
/ ops.gram_d2).  Everything below is an integer or built from integers:

    med      the lower median of the N (N - 1) / 2 entries d2[i, j], i < j: rank (N (N - 1) / 2 - 1) // 2 ascending
    den_b    2 med c_b for the scales c_1 .. c_B (B <= 7), so k_b(d2) = exp(-d2 / den_b)
    hi_b[h]  exp(-(65536 h) / den_b),  lo_b[l] = exp(-l / den_b): float64 tables of 65536 entries from numpy, on both paths
    Kq[i, j] sum_b rint(2^28 (hi_b[d2 >> 16] lo_b[d2 & 65535])) for i != j, 0 on the diagonal: one float64 product, one exact scaling,
             round-half-even — no transcendental and no fused operation after the tables, so Kq is the same on the CPU and a device
    member   int8 [P + 1, ld], ld = N rounded up to 64: row 0 marks the synthetic rows, row p >= 1 the n columns
             audit.subset_indices(seed, p, 0, N, n): relabelling p
    r[i, p]  sum_j Kq[i, j] member[p, j];  sxx2[p] = sum_{i in p} r[i, p];  sxy[p] = sum_{i not in p} r[i, p];  tot2 = sum Kq;
             syy2 = tot2 - sxx2 - 2 sxy: exact int64, N (N - 1) 2^31 < 2^63
    T[p]     sxx2[p] m (m - 1) + syy2[p] n (n - 1) - 2 sxy[p] (n - 1) (m - 1), a Python integer: the unbiased MMD^2 of relabelling p
             over the common denominator 2^28 B n (n - 1) m (m - 1)

and p_value = (1 + #{p >= 1 : T[p] >= T[0]}) / (P + 1), compared on the integers.  A relabelling is a function of (seed, p, N, n) alone,
so the figures do not depend on how the P relabellings are cut into chunks, and the device (ops.tri_hist / mmd_kernel /
mmd_partition_sums) is held to the host functions of this file by equality.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import audit, svm

MAX_POOL = 65536                               # rows of the stored matrix
MAX_SCALES = 7                                 # 7 * 2^28 < 2^31
TABLE = 65536
ONE = 1 << 28                                  # the fixed-point unit of one kernel
DEFAULT_SCALES = (0.25, 1.0, 4.0)
_HOST_ROWS = 256                               # rows of one block of the host model


def padded_cols(N):
    return (int(N) + 63) // 64 * 64


def check_sizes(n, m):
    n, m = int(n), int(m)
    if n + m > MAX_POOL:
        raise ValueError("a pool of %d + %d = %d rows: the stored matrix takes at most %d (16 GiB); give fewer rows with --n_real or a "
                         "smaller synthetic cache" % (n, m, n + m, MAX_POOL))
    if n < 2 or m < 2:
        raise ValueError("sets of %d and %d rows: the unbiased estimate needs at least 2 of each" % (n, m))
    return n, m


# ---- the median ---------------------------------------------------------------------------------------------------------------------------

def tri_hist_host(d2, n, prefix=0, prefix_bits=0):
    """int64 [256]: the definition of cslgan_tri_hist_u32 on d2 uint32 [>= n, >= n]."""
    n, pb = int(n), int(prefix_bits)
    if pb not in (0, 8, 16, 24):
        raise ValueError("prefix_bits = %d must be 0, 8, 16 or 24" % pb)
    hist = np.zeros(256, dtype=np.int64)
    for i in range(n - 1):
        v = np.asarray(d2[i, i + 1:n], dtype=np.uint32)
        if pb:
            v = v[(v >> np.uint32(32 - pb)) == np.uint32((int(prefix) & 0xFFFFFFFF) >> (32 - pb))]
        hist += np.bincount((v >> np.uint32(24 - pb)) & np.uint32(255), minlength=256)
    return hist


def median_rank(n):
    """The rank, from 0 and ascending, of the lower median of the n (n - 1) / 2 entries above the diagonal."""
    return (int(n) * (int(n) - 1) // 2 - 1) // 2


def median_d2(d2, n, device="cpu"):
    """The lower median of d2[i, j], i < j < n, as a Python integer: an exact radix select in four histograms of 8 bits, tri_hist_host on
    the CPU (d2: numpy uint32) and ops.tri_hist on a device (d2: the matrix of ops.gram_d2)."""
    n = int(n)
    if n < 2:
        raise ValueError("a pool of %d rows has no pair" % n)
    on_device = torch.device(device).type == "cuda"
    if on_device:
        from . import ops
        if d2.shape[0] != n:
            raise ValueError("the device matrix has %d rows, the pool %d" % (d2.shape[0], n))
    rank, prefix = median_rank(n), 0
    for pb in (0, 8, 16, 24):
        hist = ops.tri_hist(d2, prefix, pb).cpu().numpy() if on_device else tri_hist_host(d2, n, prefix, pb)
        below = np.cumsum(hist) - hist
        v = int(np.searchsorted(np.cumsum(hist), rank, side="right"))
        rank -= int(below[v])
        prefix |= v << (24 - pb)
    return prefix


# ---- the kernel matrix --------------------------------------------------------------------------------------------------------------------

def kernel_tables(med, scales=DEFAULT_SCALES):
    """(hi, lo) float64 [B, 65536]: hi[b, h] = exp(-(65536 h) / den_b) and lo[b, l] = exp(-l / den_b), den_b = 2 med c_b."""
    med, scales = int(med), [float(c) for c in scales]
    if med < 1:
        raise ValueError("the median squared distance is %d: more than half of the pairs coincide, no bandwidth follows" % med)
    if not 1 <= len(scales) <= MAX_SCALES or any(not (c > 0.0 and math.isfinite(c)) for c in scales):
        raise ValueError("need 1 .. %d finite scales > 0, got %s" % (MAX_SCALES, scales))
    t = np.arange(TABLE, dtype=np.float64)
    den = np.array([2.0 * med * c for c in scales], dtype=np.float64)[:, None]
    return np.exp(-(65536.0 * t)[None, :] / den), np.exp(-t[None, :] / den)


def kernel_matrix_host(d2, n, hi, lo):
    """Kq uint32 [n, n]: the definition of cslgan_mmd_kernel_u32 on d2 uint32 [>= n, >= n]."""
    n = int(n)
    kq = np.empty((n, n), dtype=np.uint32)
    for r0 in range(0, n, _HOST_ROWS):
        v = np.asarray(d2[r0:r0 + _HOST_ROWS, :n], dtype=np.uint32)
        h, l = (v >> np.uint32(16)).astype(np.intp), (v & np.uint32(65535)).astype(np.intp)
        s = np.zeros(v.shape, dtype=np.uint32)
        for b in range(len(hi)):
            s += np.rint((hi[b][h] * lo[b][l]) * float(ONE)).astype(np.uint32)
        kq[r0:r0 + len(v)] = s
    kq[np.arange(n), np.arange(n)] = 0
    return kq


# ---- the partitions and their sums --------------------------------------------------------------------------------------------------------

def partitions(seed, first, count, N, n):
    """int8 [count, padded_cols(N)]: the rows first .. first + count - 1 of `member`.  Row 0 marks the columns 0 .. n - 1."""
    first, count, N, n = int(first), int(count), int(N), int(n)
    member = np.zeros((count, padded_cols(N)), dtype=np.int8)
    ps = np.arange(first, first + count)
    if count and ps[0] == 0:
        member[0, :n] = 1
    perm = ps[ps > 0]
    if len(perm):
        idx = audit.subset_indices(seed, perm, 0, N, n)
        member[(np.arange(len(perm)) + (count - len(perm)))[:, None], idx] = 1
    return member


def partition_sums_host(kq, member, n=None):
    """(sxx2, sxy) int64 [P]: the definition of cslgan_mmd_partition_sums_i64 on kq uint32 [>= n, >= n] (entries < 2^31) and member int8
    [P, >= n] of marks 0 / 1.  The product runs in float64: every partial sum is an integer below 65536 * 2^31 = 2^47, so it is exact."""
    kq, member = np.asarray(kq), np.asarray(member)
    n = kq.shape[0] if n is None else int(n)
    mt = member[:, :n].astype(np.float64).T
    marked = member[:, :n].T != 0
    sxx2, sxy = np.zeros(member.shape[0], dtype=np.int64), np.zeros(member.shape[0], dtype=np.int64)
    for r0 in range(0, n, _HOST_ROWS):
        r = (kq[r0:r0 + _HOST_ROWS, :n].astype(np.float64) @ mt).astype(np.int64)
        mk = marked[r0:r0 + _HOST_ROWS]
        sxx2 += np.where(mk, r, 0).sum(0)
        sxy += np.where(mk, 0, r).sum(0)
    return sxx2, sxy


def statistics(sxx2, sxy, tot2, n, m):
    """[T[p]] as Python integers."""
    n, m, tot2 = int(n), int(m), int(tot2)
    out = []
    for xx, xy in zip((int(v) for v in sxx2), (int(v) for v in sxy)):
        yy = tot2 - xx - 2 * xy
        out.append(xx * m * (m - 1) + yy * n * (n - 1) - 2 * xy * (n - 1) * (m - 1))
    return out


def figures(T, n, m, n_scales, med, seed=0):
    """The report from T[0 .. P]: the comparisons on the integers, one division per figure."""
    n, m = int(n), int(m)
    den = ONE * int(n_scales) * n * (n - 1) * m * (m - 1)
    t0, perm = T[0], T[1:]
    n_ge, n_eq = sum(1 for t in perm if t >= t0), sum(1 for t in perm if t == t0)
    out = {"mmd2": t0 / den, "p_value": (1 + n_ge) / (len(perm) + 1), "n_ge": n_ge, "n_eq": n_eq, "n_perms": len(perm), "n_syn": n, "n_real": m,
           "median_d2": int(med), "n_scales": int(n_scales), "seed": int(seed)}
    if perm:
        vals = np.array([t / den for t in perm], dtype=np.float64)
        mean, std = float(vals.mean()), float(vals.std(ddof=1)) if len(perm) > 1 else 0.0
        out.update(perm_mean=mean, perm_std=std, z_score=(t0 / den - mean) / std if std > 0.0 else 0.0)
    else:
        out.update(perm_mean=0.0, perm_std=0.0, z_score=0.0)
    return out


def _member_chunk(N, chunk):
    """Partitions per launch: `chunk`, or as many as keep member (ld bytes each) at 64 MiB."""
    return int(chunk) if chunk else max(1, (64 << 20) // padded_cols(N))


def pool_sums(Z, n, n_perms=1000, scales=DEFAULT_SCALES, seed=0, device="cpu", chunk=None):
    """{"sxx2", "sxy": int64 [P + 1], "tot2", "median_d2"} of the pool Z (uint8 [N, D]: n synthetic rows, then the real ones)."""
    Z = np.ascontiguousarray(np.asarray(Z, dtype=np.uint8).reshape(len(Z), -1))
    N, n, P1 = len(Z), int(n), int(n_perms) + 1
    check_sizes(n, N - n)
    if n_perms < 0:
        raise ValueError("n_perms = %d" % n_perms)
    chunk = _member_chunk(N, chunk)
    dev = torch.device(device)
    sxx2, sxy = np.empty(P1, dtype=np.int64), np.empty(P1, dtype=np.int64)
    ones = np.zeros((1, padded_cols(N)), dtype=np.int8)
    ones[0, :N] = 1
    if dev.type != "cuda":
        d2, _ = svm.gram_d2_host(Z)
        med = median_d2(d2, N)
        hi, lo = kernel_tables(med, scales)
        kq = kernel_matrix_host(d2, N, hi, lo)
        tot2 = int(partition_sums_host(kq, ones)[0][0])
        for p0 in range(0, P1, chunk):
            cnt = min(chunk, P1 - p0)
            sxx2[p0:p0 + cnt], sxy[p0:p0 + cnt] = partition_sums_host(kq, partitions(seed, p0, cnt, N, n))
    else:
        from . import ops
        with torch.cuda.device(dev):
            xs, sq = ops.nn_prepare(torch.from_numpy(Z).to(dev))
            d2 = ops.gram_d2(xs, sq)
            del xs, sq
            med = median_d2(d2, N, dev)
            hi, lo = kernel_tables(med, scales)
            kq = ops.mmd_kernel(d2, torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev))
            tot2 = int(ops.mmd_partition_sums(kq, torch.from_numpy(ones).to(dev))[0].cpu()[0])
            for p0 in range(0, P1, chunk):
                cnt = min(chunk, P1 - p0)
                xx, xy = ops.mmd_partition_sums(kq, torch.from_numpy(partitions(seed, p0, cnt, N, n)).to(dev))
                sxx2[p0:p0 + cnt], sxy[p0:p0 + cnt] = xx.cpu().numpy(), xy.cpu().numpy()
    return {"sxx2": sxx2, "sxy": sxy, "tot2": tot2, "median_d2": med}


def mmd_rows(syn, real, n_perms=1000, scales=DEFAULT_SCALES, seed=0, device="cpu", chunk=None):
    """(figures, values) of synthetic rows against real rows, uint8 [n, ...] and [m, ...]; values: the sums of pool_sums and "T"."""
    syn, real = np.asarray(syn, dtype=np.uint8), np.asarray(real, dtype=np.uint8)
    n, m = check_sizes(len(syn), len(real))
    vals = pool_sums(np.concatenate([syn.reshape(n, -1), real.reshape(m, -1)]), n, n_perms, scales, seed, device, chunk)
    vals["T"] = statistics(vals["sxx2"], vals["sxy"], vals["tot2"], n, m)
    return figures(vals["T"], n, m, len(scales), vals["median_d2"], seed), vals


# ---- caches -------------------------------------------------------------------------------------------------------------------------------

class RealSide:
    """The reference cache and which of its rows enter a pool: `rows(m)` are the rows audit.subset_indices(seed, 0, 1, len, m), in that
    order, or all rows in index order when the cache has at most m; gathered once per m."""

    def __init__(self, cache, seed=0, n_real=None):
        self.cache, self.seed, self.n_real = cache, int(seed), None if n_real is None else int(n_real)
        self._rows = {}

    def count(self, n):
        """m for a synthetic set of n rows: n_real as asked for, or by default n capped so that the pool keeps to 65536 rows; never more
        than the cache holds."""
        want = max(0, min(int(n), MAX_POOL - int(n))) if self.n_real is None else self.n_real
        return min(want, len(self.cache))

    def rows(self, m):
        m = int(m)
        if m not in self._rows:
            total = len(self.cache)
            idx = np.arange(total) if total <= m else audit.subset_indices(self.seed, 0, 1, total, m)
            out = np.empty((len(idx), self.cache.H, self.cache.W, self.cache.C), dtype=np.uint8)
            self._rows = {m: self.cache.gather(idx, out).reshape(len(idx), -1)}
        return self._rows[m]


def real_side(train, seed=0, n_real=None):
    return RealSide(train, seed, n_real)


def run_mmd(real, cache, n_perms=1000, scales=DEFAULT_SCALES, device="cpu", chunk=None):
    """(figures, values) of one cache against real_side()'s reference.  They do not depend on the device or on `chunk`."""
    if (cache.H, cache.W, cache.C) != (real.cache.H, real.cache.W, real.cache.C):
        raise ValueError("the caches hold %dx%dx%d and %dx%dx%d images: both must have one geometry"
                         % (real.cache.H, real.cache.W, real.cache.C, cache.H, cache.W, cache.C))
    n = len(cache)
    m = real.count(n)
    check_sizes(n, m)
    syn = np.array(cache.x, dtype=np.uint8).reshape(n, -1)
    return mmd_rows(syn, real.rows(m), n_perms, scales, real.seed, device, chunk)
