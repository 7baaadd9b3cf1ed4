"""Exact byte moments of an image cache and the Fréchet distance of two caches from them (include/cslgan.h "Byte moments").

A cache of N rows of D = H W C bytes, y = x - 128 (the shift of ops.nn_prepare):

    s1[j]    = sum_n y[n][j]                       int64
    s2[i][j] = sum_n y[n][i] y[n][j]               int64, |s2| <= N 2^14
    M        = N s2 - s1 (x) s1                    exact int64 for N < 2^24: N^2 2^14 < 2^62 for either term
    C        = M / (N (N - 1))                     float64: the unbiased covariance, np.cov's and pytorch_fid's
    dmu      = (s1A NB - s1B NA) / (NA NB)         from the integers: a set shifted by 3 per byte gives 3 exactly

    FD(A, B) = |dmu|^2 + tr CA + tr CB - 2 tr (CA^1/2 CB CA^1/2)^1/2

with CA^1/2 from eigh(CA), eigenvalues clipped at 0, the inner matrix symmetrised and the trace of its root taken as the sum of
sqrt(max(lambda, 0)) over eigvalsh; no eps I is added and nothing is clamped, so FD(A, A) is a rounding error of either sign.  The
integers are the same on the CPU (`byte_moments_host`: THE definition) and on a device (ops.mom_transpose / mom_colsum / mom_gram /
mom_mirror), which is held to them by equality; the float step runs on the host in float64 on both paths, in `frechet_from_moments`.
"""
from __future__ import annotations

import numpy as np
import torch

MAX_D = 65536
MAX_N = 2 ** 24                                # N^2 2^14 must stay below 2^62
MAX_CHUNK = 65536                              # rows of one Gram launch: |acc| <= 65536 * 2^14 = 2^30 in int32
HOST_BLOCK = 4096                              # rows of one float64 product of the host model
MAX_HOST_BLOCK = 2 ** 38                       # block * 2^14 < 2^53: every partial sum of the float64 product is an exact integer


def padded_rows(n):
    return (int(n) + 63) // 64 * 64


def workspace_bytes(D, block_rows, chunk_rows=MAX_CHUNK):
    """What a walk keeps beside the D x D int64 matrix: one block of bytes and the transposed image of one chunk."""
    D, block_rows = int(D), int(block_rows)
    return block_rows * D + D * padded_rows(min(block_rows, int(chunk_rows), MAX_CHUNK))


def check_sizes(n, D, block_rows=16384, resident_gb=8.0, chunk_rows=MAX_CHUNK):
    """2 <= N < 2^24 (the covariance divides by N - 1; M must fit int64), 1 <= D <= 65536, and the matrix with its workspace fits."""
    n, D, block_rows, chunk_rows = int(n), int(D), int(block_rows), int(chunk_rows)
    if n < 2:
        raise ValueError("a set of %d rows: the unbiased covariance needs at least 2" % n)
    if n >= MAX_N:
        raise ValueError("a set of %d rows: N^2 * 2^14 must stay below 2^62, so N < 2^24 = %d" % (n, MAX_N))
    if not 1 <= D <= MAX_D or block_rows < 1 or chunk_rows < 1:
        raise ValueError("%d images of %d bytes in blocks of %d rows, chunks of %d; need 1 <= D <= %d" % (n, D, block_rows, chunk_rows, MAX_D))
    need = 8 * D * D + workspace_bytes(D, min(block_rows, n), chunk_rows)
    if need > float(resident_gb) * 2 ** 30:
        raise ValueError("the second moments of %d bytes per image take D * D * 8 = %d bytes and the workspace %d: %.3f GB above "
                         "--resident_gb %g" % (D, 8 * D * D, need - 8 * D * D, need / 2 ** 30, float(resident_gb)))
    return n, D


# ---- the integers ---------------------------------------------------------------------------------------------------------------------------

def _add_rows_host(s1, s2, rows, block):
    """s1, s2 += the moments of uint8 rows [m, D].  The product runs in float64 over at most `block` rows: its entries and every partial
    sum are integers of magnitude <= block * 2^14 < 2^53, so the BLAS result is exact in any summation order."""
    for r0 in range(0, len(rows), block):
        y = rows[r0:r0 + block].astype(np.float64) - 128.0
        s1 += y.sum(0).astype(np.int64)                        # |sum| <= block * 2^7
        s2 += (y.T @ y).astype(np.int64)


def byte_moments_host(Xu8, block=HOST_BLOCK):
    """{"n", "s1": int64 [D], "s2": int64 [D, D]} of uint8 rows [n, ...]: the host model."""
    X = np.asarray(Xu8, dtype=np.uint8)
    n = len(X)
    X = X.reshape(n, -1)
    block = int(block)
    if not 1 <= block < MAX_HOST_BLOCK:
        raise ValueError("blocks of %d rows; an exact float64 product needs 1 <= block < 2^38" % block)
    D = X.shape[1]
    s1, s2 = np.zeros(D, dtype=np.int64), np.zeros((D, D), dtype=np.int64)
    _add_rows_host(s1, s2, X, block)
    return {"n": n, "s1": s1, "s2": s2}


def byte_moments(cache, device="cpu", block_rows=16384, chunk_rows=MAX_CHUNK):
    """{"n", "s1", "s2"} of a pipeline.CachedImages as int64 numpy arrays, walked in blocks of block_rows images.  On a device every
    block goes through ops.mom_transpose / mom_colsum / mom_gram in chunks of at most chunk_rows (<= 65536) rows, and the tiles above the
    diagonal are mirrored once at the end.  The result does not depend on the device, block_rows or chunk_rows."""
    dev = torch.device(device)
    n, D = len(cache), cache.H * cache.W * cache.C
    block_rows, chunk_rows = int(block_rows), int(chunk_rows)
    if n < 1 or not 1 <= D <= MAX_D or block_rows < 1 or not 1 <= chunk_rows <= MAX_CHUNK:
        raise ValueError("%d images of %d bytes in blocks of %d rows, chunks of %d; need 1 <= D <= %d and chunks of 1 .. %d rows"
                         % (n, D, block_rows, chunk_rows, MAX_D, MAX_CHUNK))
    if dev.type != "cuda":
        s1, s2 = np.zeros(D, dtype=np.int64), np.zeros((D, D), dtype=np.int64)
        for r0 in range(0, n, block_rows):
            _add_rows_host(s1, s2, np.asarray(cache.x[r0:r0 + block_rows], dtype=np.uint8).reshape(-1, D), HOST_BLOCK)
        return {"n": n, "s1": s1, "s2": s2}
    from . import ops
    with torch.cuda.device(dev):
        s1 = torch.zeros(D, device=dev, dtype=torch.int64)
        s2 = torch.zeros((D, D), device=dev, dtype=torch.int64)
        stage = torch.empty((min(block_rows, n), cache.H, cache.W, cache.C), dtype=torch.uint8, pin_memory=True)
        for r0 in range(0, n, block_rows):
            cnt = min(block_rows, n - r0)
            cache.gather(np.arange(r0, r0 + cnt), stage[:cnt])
            x = stage[:cnt].to(dev)
            for c0 in range(0, cnt, chunk_rows):
                xt = ops.mom_transpose(x[c0:c0 + chunk_rows])
                ops.mom_colsum(xt, s1)
                ops.mom_gram(xt, s2)
        ops.mom_mirror(s2)
        return {"n": n, "s1": s1.cpu().numpy(), "s2": s2.cpu().numpy()}


# ---- the float step: the host, float64, both paths -------------------------------------------------------------------------------------------

def centred(s1, s2, n):
    """M = N s2 - s1 (x) s1 as int64: N times the sum of squares about the mean, exact for N < 2^24."""
    n = int(n)
    if not 2 <= n < MAX_N:
        raise ValueError("a set of %d rows; need 2 <= N < 2^24" % n)
    s1, s2 = np.asarray(s1, dtype=np.int64), np.asarray(s2, dtype=np.int64)
    if s1.ndim != 1 or s2.shape != (len(s1), len(s1)):
        raise ValueError("need s1 [D] and s2 [D, D], got %s and %s" % (s1.shape, s2.shape))
    return np.int64(n) * s2 - np.multiply.outer(s1, s1)


def covariance(s1, s2, n):
    """float64 [D, D]: the unbiased covariance M / (N (N - 1)) of the bytes."""
    return centred(s1, s2, n).astype(np.float64) / float(int(n) * (int(n) - 1))


def sqrt_psd(C):
    """The symmetric root of a covariance: eigh, eigenvalues clipped at 0."""
    w, V = np.linalg.eigh(C)
    return (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T


def frechet_from_moments(ma, mb, sqrt_a=None, cov_a=None):
    """The figures of one pair of sets from their integer moments ({"n", "s1", "s2"} each); sqrt_a / cov_a: CA^1/2 and CA when the caller
    has them (real_side).  fd is reported as computed: a value below zero is a rounding error of FD(A, A) and is not clamped."""
    na, nb = int(ma["n"]), int(mb["n"])
    s1a, s1b = np.asarray(ma["s1"], dtype=np.int64), np.asarray(mb["s1"], dtype=np.int64)
    if s1a.shape != s1b.shape:
        raise ValueError("the sets hold rows of %d and %d bytes" % (len(s1a), len(s1b)))
    D = len(s1a)
    ca = covariance(s1a, ma["s2"], na) if cov_a is None else cov_a
    cb = covariance(s1b, mb["s2"], nb)
    if sqrt_a is None:
        sqrt_a = sqrt_psd(ca)
    delta = (s1a * np.int64(nb) - s1b * np.int64(na)).astype(np.float64) / float(na * nb)        # |s1 N| < 2^31 * 2^24
    mean_term = float(np.dot(delta, delta))
    trace_term = float(np.trace(ca) + np.trace(cb))
    inner = sqrt_a @ cb @ sqrt_a
    lam = np.linalg.eigvalsh((inner + inner.T) * 0.5)
    sqrt_term = float(np.sqrt(np.clip(lam, 0.0, None)).sum())
    fd = mean_term + trace_term - 2.0 * sqrt_term
    return {"fd": fd, "fd_unit": fd / 255.0 ** 2, "fd_per_dim": fd / D, "mean_term": mean_term, "trace_term": trace_term,
            "sqrt_term": sqrt_term, "n_a": na, "n_b": nb, "dim": D}


class RealSide:
    """The moments of the reference cache with its covariance and the root of it, computed once."""

    def __init__(self, cache, moments):
        self.cache, self.moments = cache, moments
        self.cov = covariance(moments["s1"], moments["s2"], moments["n"])
        self.sqrt = sqrt_psd(self.cov)


def real_side(train, device="cpu", block_rows=16384, resident_gb=8.0, chunk_rows=MAX_CHUNK):
    """The training set's moments and CA^1/2 once for all synthetic caches."""
    check_sizes(len(train), train.H * train.W * train.C, block_rows, resident_gb, chunk_rows)
    return RealSide(train, byte_moments(train, device, block_rows, chunk_rows))


def run_frechet(real, cache, device="cpu", block_rows=16384, resident_gb=8.0, chunk_rows=MAX_CHUNK):
    """(figures, moments) of one cache against real_side()'s reference."""
    if (cache.H, cache.W, cache.C) != (real.cache.H, real.cache.W, real.cache.C):
        raise ValueError("the caches hold %dx%dx%d and %dx%dx%d images: both must have one geometry"
                         % (real.cache.H, real.cache.W, real.cache.C, cache.H, cache.W, cache.C))
    check_sizes(len(cache), cache.H * cache.W * cache.C, block_rows, resident_gb, chunk_rows)
    m = byte_moments(cache, device, block_rows, chunk_rows)
    return frechet_from_moments(real.moments, m, sqrt_a=real.sqrt, cov_a=real.cov), m
