"""Sliced Wasserstein distance of two image caches (include/cslgan.h "Sliced Wasserstein audit").

How far the mass of one set has to move to become the other, without a borrowed network: the cache BYTES of A (Na rows) and B (Nb
rows), D = H W C each, are projected on P Rademacher directions s_p in {-1, +1}^D,

    y_p(x) = sum_j s_p[j] (x[j] - 128)                           an exact integer, |y| <= 128 D <= 2^23

and per direction the one-dimensional Wasserstein-1 distance of the two projected samples is taken in its quantile form on the common
grid of Na Nb cells, with a, b the ascending sorted projections:

    num_p = sum_i sum_j |a[i] - b[j]| * |[i Nb, (i + 1) Nb) n [j Na, (j + 1) Na)|,      W1_p = num_p / (Na Nb).

Every direction has the norm sqrt(D) exactly, so swd = mean_p W1_p / sqrt(D), in bytes.  The shift by 128 moves both sets alike and W1
is translation invariant.  The P numerators are exact int64 and the same on the CPU (`directions_host`, `project_host`, np.sort,
`w1_numerators_host`: THE definitions) and on a device (ops.swd_directions / swd_project / sort_rows / swd_w1), which is held to them by
equality; the float figures follow from them on the host in float64 on both paths.

The direction stream: one Philox4x32-10 call gives the 128 signs of the columns 128 b .. 128 b + 127 of direction p, counter
(b, p, 0, SWD_COUNTER_TAG), key seed ^ SWD_SEED_TAG; bit t is bit t & 31 of word t >> 5, set +1, clear -1.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .generate import _philox4x32_10

SWD_SEED_TAG = 0x7377647369676E73              # include/cslgan.h: xor-ed into the seed ("swdsigns"; apart from every other stream)
SWD_COUNTER_TAG = 0x73776464                   # word 3 of every counter of the stream ("swdd")
MAX_D = 65536
MAX_CELLS = 2 ** 38                            # Na Nb 2^25 must stay below 2^63
KEY_BITS = 25                                  # |y| <= 2^23: the sort's keys
_M64 = 0xFFFFFFFFFFFFFFFF


def check_sizes(na, nb):
    """Na Nb 2^25 < 2^63: |a - b| <= 2^24 on at most Na Nb cells cannot overflow the int64 numerator."""
    na, nb = int(na), int(nb)
    if na < 1 or nb < 1:
        raise ValueError("sets of %d and %d rows: both need at least one" % (na, nb))
    if na * nb >= MAX_CELLS:
        raise ValueError("Na * Nb * 2^25 = %d * %d * 2^25 >= 2^63 overflows the int64 numerator" % (na, nb))
    return na, nb


# ---- host models ------------------------------------------------------------------------------------------------------------------------

def directions_host(P, D, seed, first=0):
    """int8 [P, D] of +1 / -1: the directions first .. first + P - 1 of the stream of `seed`.  Entry (p, j) depends on (seed, p, j) only."""
    P, D, first = int(P), int(D), int(first)
    if P < 1 or not 1 <= D <= MAX_D or first < 0:
        raise ValueError("P = %d directions from %d of D = %d columns; need P >= 1, 1 <= D <= %d" % (P, first, D, MAX_D))
    key = (int(seed) ^ SWD_SEED_TAG) & _M64
    b = np.arange((D + 127) // 128, dtype=np.uint64)[None, :]
    p = (np.arange(P, dtype=np.uint64) + np.uint64(first))[:, None]
    w = np.stack(_philox4x32_10(b, p, 0, SWD_COUNTER_TAG, key & 0xFFFFFFFF, key >> 32), axis=-1)          # [P, groups, 4] words
    bits = (w[..., None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)                                 # [P, groups, 4, 32]
    return (2 * bits.reshape(P, -1)[:, :D].astype(np.int8) - 1).astype(np.int8)


def project_host(dirs, x, block=4096):
    """int32 [P, n]: y_p of every row of x (uint8 [n, ...], D bytes each) on dirs int8 [P, D], in float64 — exact: every partial sum is
    an integer below 2^53."""
    dirs = np.asarray(dirs)
    n = len(x)
    D = dirs.shape[1]
    s = dirs.astype(np.float64).T
    out = np.empty((dirs.shape[0], n), dtype=np.int32)
    for r0 in range(0, n, block):
        rows = np.asarray(x[r0:r0 + block], dtype=np.uint8).reshape(-1, D).astype(np.float64) - 128.0
        out[:, r0:r0 + len(rows)] = (rows @ s).T.astype(np.int32)
    return out


def w1_numerators_host(a_sorted, b_sorted, block=64):
    """int64 [P]: num_p of the ascending rows a [P, Na] and b [P, Nb].  The common grid is cut where either index changes: at the
    multiples of Nb (of a) and of Na (of b), Na + Nb - 1 pieces at most; a piece that starts at cell c lies in a[c // Nb] and b[c // Na]."""
    a, b = np.asarray(a_sorted), np.asarray(b_sorted)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("need a [P, Na] and b [P, Nb], got %s and %s" % (a.shape, b.shape))
    na, nb = check_sizes(a.shape[1], b.shape[1])
    cuts = np.union1d(np.arange(na + 1, dtype=np.int64) * nb, np.arange(nb + 1, dtype=np.int64) * na)
    length, ia, ib = np.diff(cuts), cuts[:-1] // nb, cuts[:-1] // na
    out = np.empty(a.shape[0], dtype=np.int64)
    for p0 in range(0, a.shape[0], block):
        d = np.abs(a[p0:p0 + block, ia].astype(np.int64) - b[p0:p0 + block, ib].astype(np.int64))
        out[p0:p0 + block] = (d * length[None, :]).sum(1)
    return out


def swd_metrics(num, na, nb, D, seed=0):
    """The figures of one pair of sets from its numerators: one division per direction, then float64 on the host."""
    num = np.asarray(num, dtype=np.int64).reshape(-1)
    na, nb = check_sizes(na, nb)
    P = len(num)
    if P < 1:
        raise ValueError("no directions")
    w1 = num.astype(np.float64) / float(na * nb) / math.sqrt(float(D))
    swd = float(w1.mean())
    return {"swd": swd, "swd_unit": swd / 255.0, "max_sliced": float(w1.max()),
            "stderr": float(w1.std(ddof=1) / math.sqrt(P)) if P > 1 else 0.0, "n_a": na, "n_b": nb, "n_dirs": P, "seed": int(seed)}


# ---- the sorted projections of one cache, direction block by direction block ---------------------------------------------------------------

def _labels_of(cache):
    return np.asarray(cache.labels, dtype=np.int64).reshape(-1)


def _dir_block(P, n, n_other, resident_gb):
    """Directions per block: the projections, their sort's workspace, a class's copy and the other side's rows fit resident_gb."""
    per_dir = 16 * int(n) + 8 * int(n_other) + 4096
    return int(max(1, min(int(P), int(float(resident_gb) * 2 ** 30) // per_dir)))


def sorted_blocks(cache, P, seed, device="cpu", block_rows=16384, resident_gb=8.0, per_class=False, n_other=0):
    """Yields (p0, p1, all, {label: rows}) for consecutive direction blocks [p0, p1): `all` is int32 [p1 - p0, len(cache)], the ascending
    projections of the whole cache, and `rows` the same over the images of one label (per_class only: the label's columns of the
    projected matrix are gathered before the sort).  numpy arrays on the CPU, device tensors on a device, valid until the next block."""
    dev = torch.device(device)
    n, D = len(cache), cache.H * cache.W * cache.C
    P, block_rows = int(P), int(block_rows)
    if P < 1 or block_rows < 1 or not 1 <= D <= MAX_D or n < 1:
        raise ValueError("P = %d directions, blocks of %d rows, %d images of %d bytes" % (P, block_rows, n, D))
    labels = _labels_of(cache)
    groups = {int(l): np.nonzero(labels == l)[0] for l in np.unique(labels)} if per_class else {}
    pb = _dir_block(P, n, n_other, resident_gb)
    if dev.type != "cuda":
        for p0 in range(0, P, pb):
            p1 = min(P, p0 + pb)
            y = project_host(directions_host(p1 - p0, D, seed, first=p0), cache.x)
            yield p0, p1, np.sort(y, axis=1), {l: np.sort(y[:, idx], axis=1) for l, idx in groups.items()}
        return
    from . import ops
    with torch.cuda.device(dev):
        dirs = ops.swd_directions(P, D, seed, dev)                    # all of them: P Dp bytes
        stage = torch.empty((min(block_rows, n), cache.H, cache.W, cache.C), dtype=torch.uint8, pin_memory=True)
        idx_dev = {l: torch.from_numpy(idx).to(dev) for l, idx in groups.items()}
        ws = torch.empty(ops.sort_rows_ws_bytes(min(pb, P), n), device=dev, dtype=torch.uint8)
        for p0 in range(0, P, pb):
            p1 = min(P, p0 + pb)
            y = torch.empty((p1 - p0, n), device=dev, dtype=torch.int32)
            for r0 in range(0, n, block_rows):
                cnt = min(block_rows, n - r0)
                cache.gather(np.arange(r0, r0 + cnt), stage[:cnt])
                xs, _ = ops.nn_prepare(stage[:cnt].to(dev))
                ops.swd_project(dirs[p0:p1], xs, y, r0)
            per = {l: ops.sort_rows(y[:, idx].contiguous(), key_bits=KEY_BITS, ws=ws) for l, idx in idx_dev.items()}
            yield p0, p1, ops.sort_rows(y, key_bits=KEY_BITS, ws=ws), per
        torch.cuda.synchronize(dev)


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else t


class RealSide:
    """The sorted projections of the reference cache on all P directions, on the host: int32 [P, Na], and per label with per_class."""

    def __init__(self, cache, P, seed, rows, per_label):
        self.cache, self.P, self.seed, self.rows, self.per_label = cache, int(P), int(seed), rows, per_label
        self.D = cache.H * cache.W * cache.C


def real_side(train, P, seed=0, device="cpu", block_rows=16384, resident_gb=8.0, per_class=False):
    """Projects and sorts the training cache once for all synthetic caches."""
    P = int(P)
    if P < 1:
        raise ValueError("P = %d directions; need at least one" % P)
    labels, counts = np.unique(_labels_of(train), return_counts=True)
    rows = np.empty((P, len(train)), dtype=np.int32)
    per = {int(l): np.empty((P, int(c)), dtype=np.int32) for l, c in zip(labels, counts)} if per_class else {}
    for p0, p1, y, cls in sorted_blocks(train, P, seed, device, block_rows, resident_gb, per_class):
        rows[p0:p1] = _host(y)
        for l, v in cls.items():
            per[l][p0:p1] = _host(v)
    return RealSide(train, P, seed, rows, per)


def _numerators(a, b, dev):
    """num of one direction block: a from the host (the real side), b as sorted_blocks left it."""
    if dev.type != "cuda":
        return w1_numerators_host(a, b)
    from . import ops
    a_dev = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ops.swd_w1(a_dev, a_dev.shape[1], b, b.shape[1]).cpu().numpy()


def run_swd(real, cache, device="cpu", block_rows=16384, resident_gb=8.0, per_class=False):
    """The numerators of one cache against real_side()'s reference: {"num": int64 [P]} and, with per_class, "per_class": {label:
    (int64 [P], n_a, n_b)} for every label that both sets hold.  They do not depend on the device or the blocking."""
    if (cache.H, cache.W, cache.C) != (real.cache.H, real.cache.W, real.cache.C):
        raise ValueError("the caches hold %dx%dx%d and %dx%dx%d images: both must have one geometry"
                         % (real.cache.H, real.cache.W, real.cache.C, cache.H, cache.W, cache.C))
    if per_class and not real.per_label:
        raise ValueError("per_class needs a real_side(..., per_class=True)")
    na, nb = check_sizes(len(real.cache), len(cache))
    dev = torch.device(device)
    num = np.empty(real.P, dtype=np.int64)
    shared = sorted(set(real.per_label) & {int(l) for l in np.unique(_labels_of(cache))}) if per_class else []
    per = {l: np.empty(real.P, dtype=np.int64) for l in shared}
    for p0, p1, y, cls in sorted_blocks(cache, real.P, real.seed, device, block_rows, resident_gb, per_class, n_other=na):
        num[p0:p1] = _numerators(real.rows[p0:p1], y, dev)
        for l in shared:
            per[l][p0:p1] = _numerators(real.per_label[l][p0:p1], cls[l], dev)
    out = {"num": num}
    if per_class:
        out["per_class"] = {l: (per[l], real.per_label[l].shape[1], int((_labels_of(cache) == l).sum())) for l in shared}
    return out
