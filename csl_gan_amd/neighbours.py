"""Exact nearest-neighbour audit of a synthetic image cache (include/cslgan.h "Nearest-neighbour audit").

For every query image the nearest reference image under the squared Euclidean distance on the cache BYTES, as one uint64 key:

    d2(q, r) = sum_i (Q[q, i] - R[r, i])^2                       an integer in [0, 65025 D],  D = H W C <= 65536
    key(q)   = min over r of (d2(q, r) << 32 | (index_base + r))

The neighbour is the low word, its squared distance the high word, and ties go to the smallest index.  The key is a minimum over a
set, so it does not depend on how the reference is cut into blocks.  Everything is integer arithmetic: `nearest_host` is the
definition, and the device path (`ops.nn_prepare` + `ops.nn_min`) is held to it by equality.

`kth_host` is the definition of the k smallest keys per row, with an optional self-excluding search of a set in itself (DESIGN.md
§6i; csl_gan_amd.manifold builds precision / recall / density / coverage on it).  `count_within_host` (§6h) and
`count_within_radii_host` (§6i) are the definitions of the two counts.  All four reduce the distances of one host walk, `_d2_blocks`.

`NearestSearch` drives the device over a pipeline.CachedImages reference of any size; `dcr_metrics` turns keys into the
"distance to closest record" figures and the share of samples that lie closer to the training set than to a held-out set — 0.5 for
a generator that has not memorised.
"""
from __future__ import annotations

import math

import numpy as np
import torch

MAX_D = 65536
NONE_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_INDEX = 2 ** 32 - 1


def split_keys(keys):
    """(d2, index) of uint64 keys, both as int64 arrays."""
    k = np.asarray(keys, dtype=np.uint64)
    return (k >> np.uint64(32)).astype(np.int64), (k & np.uint64(0xFFFFFFFF)).astype(np.int64)


def _rows_u8(a):
    a = np.asarray(a) if not isinstance(a, np.ndarray) else a
    if a.dtype != np.uint8 or a.ndim < 2:
        raise ValueError("need a uint8 array [n, ...], got %s %s" % (a.dtype, a.shape))
    return a.reshape(a.shape[0], -1)


def _d2_blocks(Q, R, block):
    """(nq, nr, blocks) for the rows of Q [nq, ...] and R [nr, ...] (uint8, same row size D, 1 <= D <= 65536): `blocks` yields
    (q0, r0, d2) with d2[i, j] = d2(Q[q0 + i], R[r0 + j]) as float64, for every pair of blocks of `block` rows, the reference
    blocks outermost — the ONE place where the host forms d2, which every definition below reduces.  The shifted bytes (x - 128)
    go through a float64 matmul: every product sum is below 2^30 and every d2 below 2^32, far under 2^53, so the floats are the
    integers.  The operands are checked here, before the first block is asked for."""
    Q, R = _rows_u8(Q), _rows_u8(R)
    nq, D = Q.shape
    nr = R.shape[0]
    if R.shape[1] != D or not 1 <= D <= MAX_D:
        raise ValueError("rows of %d and %d bytes; need equal sizes in 1 .. %d" % (D, R.shape[1], MAX_D))
    block = max(1, int(block))

    def shifted(rows):
        return np.asarray(rows).astype(np.float64) - 128.0

    def blocks():
        for r0 in range(0, nr, block):
            b = shifted(R[r0:r0 + block])
            bn = (b * b).sum(1)
            for q0 in range(0, nq, block):
                a = shifted(Q[q0:q0 + block])
                yield q0, r0, (a * a).sum(1)[:, None] + bn[None, :] - 2.0 * (a @ b.T)
    return nq, nr, blocks()


def _block_keys(d2, first_index):
    """(uint64 keys d2 << 32 | index, the uint64 indices first_index + column) of one block of distances."""
    idx = np.arange(first_index, first_index + d2.shape[1], dtype=np.uint64)
    return (d2.astype(np.uint64) << np.uint64(32)) | idx[None, :], idx


def nearest_host(Q, R, index_base=0, best=None, block=1024):
    """key(q) for every row of Q [nq, ...] over the rows of R [nr, ...] (uint8, same row size), merged into `best` (uint64 [nq], the
    running minimum of earlier calls; all-ones when absent) — THE definition, a minimum over the blocks of `_d2_blocks`."""
    nq, nr, blocks = _d2_blocks(Q, R, block)
    if index_base < 0 or index_base + nr > MAX_INDEX:
        raise ValueError("index_base + nr = %d exceeds 2^32 - 1" % (index_base + nr))
    out = np.full(nq, NONE_KEY, dtype=np.uint64) if best is None else np.array(best, dtype=np.uint64, copy=True)
    if out.shape != (nq,):
        raise ValueError("best has shape %s, expected (%d,)" % (out.shape, nq))
    for q0, r0, d2 in blocks:
        rows = slice(q0, q0 + d2.shape[0])
        out[rows] = np.minimum(out[rows], _block_keys(d2, index_base + r0)[0].min(1))
    return out


MAX_K = 8                               # the device keeps a list of at most eight keys per row (csrc/nn_kernels.hip)


def kth_host(Q, R, k, index_base=0, self_base=-1, best=None, block=1024):
    """uint64 [nq, k]: per row of Q the k smallest keys d2(q, r) << 32 | (index_base + r) over the rows of R, ascending, merged with
    `best` (the lists of earlier calls; all-ones when absent) — THE definition of the k-nearest-neighbour lists, 1 <= k <= 8.  With
    self_base >= 0 row q leaves out the ONE column with index_base + r == self_base + q: the row is excluded by its index, never
    by its distance, so a different row with the same bytes stays in at d2 = 0.  Keys carry the index and are distinct, so ties in
    d2 are ordered by index and the list is a function of the candidate set alone.  All-ones entries stay last while fewer than k
    candidates have been seen.  PRECONDITION (the device entry has the same): successive calls bring disjoint index ranges — a key
    presented twice would be kept twice.  The distances are those of `_d2_blocks`."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d; the lists hold 1 .. %d neighbours" % (k, MAX_K))
    nq, nr, blocks = _d2_blocks(Q, R, block)
    if index_base < 0 or index_base + nr > MAX_INDEX:
        raise ValueError("index_base + nr = %d exceeds 2^32 - 1" % (index_base + nr))
    if self_base < -1 or self_base + nq > MAX_INDEX:
        raise ValueError("self_base = %d must be -1 or keep self_base + nq <= 2^32 - 1" % self_base)
    out = np.full((nq, k), NONE_KEY, dtype=np.uint64) if best is None else np.array(best, dtype=np.uint64, copy=True)
    if out.shape != (nq, k):
        raise ValueError("best has shape %s, expected (%d, %d)" % (out.shape, nq, k))
    for q0, r0, d2 in blocks:
        rows = slice(q0, q0 + d2.shape[0])
        keys, idx = _block_keys(d2, index_base + r0)
        if self_base >= 0:
            own = np.arange(self_base + q0, self_base + q0 + d2.shape[0], dtype=np.uint64)
            keys[own[:, None] == idx[None, :]] = NONE_KEY
        out[rows] = np.sort(np.concatenate([out[rows], keys], axis=1), axis=1)[:, :k]
    return out


MAX_THRESHOLDS = 4                      # the counters of a row are the four bytes of one register (csrc/nn_kernels.hip)
MAX_THRESHOLD = 2 ** 32 - 1
MAX_RADIUS = 2 ** 32 - 1


def check_thresholds(thresholds):
    """The thresholds as a list of 1 .. 4 Python integers in [0, 2^32 - 1]."""
    thr = [int(t) for t in np.asarray(thresholds, dtype=object).reshape(-1)]
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("need 1 .. %d thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    if any(t < 0 or t > MAX_THRESHOLD for t in thr):
        raise ValueError("thresholds must lie in [0, 2^32 - 1], got %s" % (thr,))
    return thr


def count_within_host(Q, R, thresholds, counts=None, block=1024):
    """counts[q, j] += #{r : d2(q, r) <= thresholds[j]} as int64 [nq, J] for the rows of Q [nq, ...] and R [nr, ...] (uint8, same row
    size D, 1 <= D <= 65536) and 1 <= J <= 4 integer thresholds in [0, 2^32 - 1], in any order — THE definition (DESIGN.md §6h;
    csl_gan_amd.blackbox builds the Monte-Carlo attack on it).  `counts` holds the sums of earlier calls (zeros when absent) and is
    not written.  The distances are those of `_d2_blocks`: they and the thresholds are integers below 2^32 held in float64."""
    nq, nr, blocks = _d2_blocks(Q, R, block)
    thr = np.array(check_thresholds(thresholds), dtype=np.float64)
    out = np.zeros((nq, len(thr)), dtype=np.int64) if counts is None else np.array(counts, dtype=np.int64, copy=True)
    if out.shape != (nq, len(thr)):
        raise ValueError("counts has shape %s, expected (%d, %d)" % (out.shape, nq, len(thr)))
    for q0, r0, d2 in blocks:
        for j, t in enumerate(thr):
            out[q0:q0 + d2.shape[0], j] += (d2 <= t).sum(1)
    return out


def check_radii(radii, n):
    """The radii as an int64 array [n] of integers in [0, 2^32 - 1]."""
    rad = np.asarray(radii)
    if rad.dtype.kind not in "iu" or rad.shape != (n,):
        raise ValueError("need %d integer radii, one per reference row, got %s %s" % (n, rad.dtype, rad.shape))
    if rad.dtype == np.uint64 and len(rad) and int(rad.max()) > MAX_RADIUS:
        raise ValueError("radii must lie in [0, 2^32 - 1]")
    rad = rad.astype(np.int64)
    if len(rad) and (int(rad.min()) < 0 or int(rad.max()) > MAX_RADIUS):
        raise ValueError("radii must lie in [0, 2^32 - 1]")
    return rad


def count_within_radii_host(Q, R, radii, counts=None, block=1024):
    """counts[q] += #{r : d2(q, r) <= radii[r]} as int64 [nq] for the rows of Q [nq, ...] and R [nr, ...] (uint8, same row size D,
    1 <= D <= 65536) and one integer radius in [0, 2^32 - 1] per row of R — THE definition (csl_gan_amd.manifold
    builds precision / recall / density / coverage on it).  `counts` holds the sums of earlier calls (zeros when absent) and is not
    written.  The distances are those of `_d2_blocks`: they and the radii are integers below 2^32 held in float64."""
    nq, nr, blocks = _d2_blocks(Q, R, block)
    rad = check_radii(radii, nr).astype(np.float64)
    out = np.zeros(nq, dtype=np.int64) if counts is None else np.array(counts, dtype=np.int64, copy=True)
    if out.shape != (nq,):
        raise ValueError("counts has shape %s, expected (%d,)" % (out.shape, nq))
    for q0, r0, d2 in blocks:
        out[q0:q0 + d2.shape[0]] += (d2 <= rad[None, r0:r0 + d2.shape[1]]).sum(1)
    return out


class NearestSearch:
    """`fit(reference cache)`, then `query(cache) -> uint64 keys[len(cache)]` and `count_within(cache, thresholds) -> int64
    counts[len(cache), J]`, any number of times; `kth` and `count_within_radii` walk the same way.

    On a HIP device the reference is walked in blocks of `block_rows` images: pinned uint8 gather -> H2D on a side stream ->
    ops.nn_prepare -> ops.nn_min with index_base = the block's first row.  Two pinned and two device staging buffers alternate, so
    block k + 1 is gathered and uploaded while the kernel of block k runs.  Prepared blocks (int8 rows + norms) stay on the device
    for later queries while they fit `resident_gb`; the rest is streamed again.  The query side goes up in chunks of `query_rows`.
    On the CPU `nearest_host` / `count_within_host` run.  Keys and counts do not depend on block_rows, query_rows or the
    device."""

    def __init__(self, device, block_rows=16384, resident_gb=8.0, query_rows=16384):
        self.device = torch.device(device)
        self.on_gpu = self.device.type == "cuda"
        self.block_rows, self.query_rows = int(block_rows), int(query_rows)
        if self.block_rows < 1 or self.query_rows < 1:
            raise ValueError("block_rows and query_rows must be positive")
        self.budget = int(float(resident_gb) * 2 ** 30)
        self.ref = None
        self._resident, self._resident_bytes, self._copy = {}, 0, None

    def fit(self, cache):
        if not 1 <= cache.H * cache.W * cache.C <= MAX_D:
            raise ValueError("images of %d bytes; the search takes 1 .. %d" % (cache.H * cache.W * cache.C, MAX_D))
        if not 1 <= len(cache) <= MAX_INDEX:
            raise ValueError("a reference of %d images" % len(cache))
        self.ref = cache
        self._resident, self._resident_bytes = {}, 0
        return self

    def resident_rows(self):
        return sum(xs.shape[0] for xs, _ in self._resident.values())

    def query(self, cache):
        self._check_query(cache)
        if not self.on_gpu:
            return nearest_host(cache.x, self.ref.x)
        from . import ops
        return self._pass(cache, np.empty(len(cache), dtype=np.uint64),
                          lambda n: torch.full((n,), -1, device=self.device, dtype=torch.int64),      # all ones: nothing seen yet
                          lambda q, qn, r, rn, s, start, best: ops.nn_min(q, qn, r, rn, start, best), _key_rows)

    def _check_query(self, cache):
        if self.ref is None:
            raise RuntimeError("fit() a reference cache first")
        if (cache.H, cache.W, cache.C) != (self.ref.H, self.ref.W, self.ref.C):
            raise ValueError("the query images are %dx%dx%d and the reference images %dx%dx%d: both caches must have one geometry"
                             % (cache.H, cache.W, cache.C, self.ref.H, self.ref.W, self.ref.C))

    def count_within(self, cache, thresholds):
        """int64 [len(cache), J]: for every query image the number of reference images with d2 <= thresholds[j] (1 <= J <= 4
        integers in [0, 2^32 - 1], any order) — count_within_host on the CPU, ops.nn_count over the same walk of the reference as
        `query` on a device.  The device counts in 32 bits, so a reference of 2^31 images or more is refused."""
        self._check_query(cache)
        thr = check_thresholds(thresholds)
        if len(self.ref) >= 2 ** 31:
            raise ValueError("a reference of %d images: counts are held below 2^31" % len(self.ref))
        if not self.on_gpu:
            return count_within_host(cache.x, self.ref.x, thr)
        from . import ops
        return self._pass(cache, np.empty((len(cache), len(thr)), dtype=np.int64),
                          lambda n: torch.zeros((n, len(thr)), device=self.device, dtype=torch.int32),
                          lambda q, qn, r, rn, s, start, counts: ops.nn_count(q, qn, r, rn, thr, counts), _count_rows)

    def kth(self, cache, k, exclude_self=False):
        """uint64 [len(cache), k]: for every query image the k smallest keys over the reference, ascending (`kth_host`; 1 <= k <= 8).
        exclude_self=True is the search of the reference in itself — `cache` must be the fitted reference — and leaves every
        image's own index out of its list.  kth_host on the CPU, ops.nn_kth over the walk of `query` on a device: query chunk
        start s and reference block start give self_base = s and index_base = start."""
        self._check_query(cache)
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k = %d; the lists hold 1 .. %d neighbours" % (k, MAX_K))
        if exclude_self and cache is not self.ref:
            raise ValueError("exclude_self searches the fitted reference in itself: pass the cache that fit() was given")
        if not self.on_gpu:
            return kth_host(cache.x, self.ref.x, k, self_base=0 if exclude_self else -1)
        from . import ops
        return self._pass(cache, np.empty((len(cache), k), dtype=np.uint64),
                          lambda n: torch.full((n, k), -1, device=self.device, dtype=torch.int64),
                          lambda q, qn, r, rn, s, start, best: ops.nn_kth(q, qn, r, rn, start, best, s if exclude_self else -1), _key_rows)

    def count_within_radii(self, cache, radii):
        """int64 [len(cache)]: for every query image the number of reference images r with d2 <= radii[r]; `radii` holds one
        integer in [0, 2^32 - 1] per reference image — count_within_radii_host on the CPU, ops.nn_count_radius over the walk of
        `query` on a device, where the radii stay on the device and are sliced per block."""
        self._check_query(cache)
        rad = check_radii(radii, len(self.ref))
        if len(self.ref) >= 2 ** 31:
            raise ValueError("a reference of %d images: counts are held below 2^31" % len(self.ref))
        if not self.on_gpu:
            return count_within_radii_host(cache.x, self.ref.x, rad)
        from . import ops
        rad_dev = torch.from_numpy(rad.astype(np.uint32).view(np.int32)).to(self.device)
        return self._pass(cache, np.empty(len(cache), dtype=np.int64),
                          lambda n: torch.zeros(n, device=self.device, dtype=torch.int32),
                          lambda q, qn, r, rn, s, start, counts: ops.nn_count_radius(q, qn, r, rn, rad_dev[start:start + r.shape[0]], counts),
                          _count_rows)

    # ---- device path -------------------------------------------------------------------------------------------------------------
    def _pass(self, cache, out, make, step, rows):
        """One pass of the query cache over the reference on the device, the frame of all four searches: per query chunk (first row
        s, prepared q / qn) acc = make(rows of the chunk) is its device accumulator, step(q, qn, r, rn, s, start, acc) is issued for
        every reference block (first row start, prepared r / rn), and rows(acc) are the chunk's numpy rows of `out`."""
        with torch.cuda.device(self.device):
            first = [0]                                                                  # first row of the next chunk: they come in order

            def chunk(q, qn):
                s, first[0] = first[0], first[0] + q.shape[0]
                acc = make(q.shape[0])
                self._walk_reference(lambda start, r, rn: step(q, qn, r, rn, s, start, acc))
                return rows(acc)
            return self._query_chunks(cache, out, chunk)

    def _query_chunks(self, cache, out, fn):
        """out[s : s + cnt] = fn(prepared int8 chunk, its norms) for the query side in chunks of query_rows."""
        from . import ops
        n = len(cache)
        shape = (cache.H, cache.W, cache.C)
        stage = torch.empty((min(self.query_rows, n),) + shape, dtype=torch.uint8, pin_memory=True)
        for s in range(0, n, self.query_rows):
            cnt = min(self.query_rows, n - s)
            cache.gather(np.arange(s, s + cnt), stage[:cnt])
            q, qn = ops.nn_prepare(stage[:cnt].to(self.device, non_blocking=True))
            out[s:s + cnt] = fn(q, qn)                                                   # its .cpu(): the stage buffer is free again
        torch.cuda.synchronize(self.device)
        return out

    def _walk_reference(self, fn):
        """fn(first row, prepared int8 block, its norms) for every block of the reference, in order, on the current stream."""
        from . import ops
        ref, B, dev = self.ref, self.block_rows, self.device
        n = len(ref)
        starts = list(range(0, n, B))
        shape = (min(B, n), ref.H, ref.W, ref.C)
        main = torch.cuda.current_stream(dev)
        if self._copy is None:
            self._copy = torch.cuda.Stream(device=dev)
        slots = [dict(host=None, dev=None, sent=None, used=None) for _ in range(2)]

        def upload(k):
            s = starts[k]
            if s in self._resident:
                return
            cnt, sl = min(B, n - s), slots[k % 2]
            if sl["host"] is None:
                sl["host"] = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
                sl["dev"] = torch.empty(shape, dtype=torch.uint8, device=dev)
            if sl["sent"] is not None:
                sl["sent"].synchronize()                        # the upload of block k - 2 has left this pinned buffer
            ref.gather(np.arange(s, s + cnt), sl["host"][:cnt])
            with torch.cuda.stream(self._copy):
                if sl["used"] is not None:
                    self._copy.wait_event(sl["used"])           # nn_prepare of block k - 2 has read the device buffer
                sl["dev"][:cnt].copy_(sl["host"][:cnt], non_blocking=True)
                sl["sent"] = torch.cuda.Event()
                sl["sent"].record(self._copy)

        upload(0)
        for k, s in enumerate(starts):
            cnt, sl = min(B, n - s), slots[k % 2]
            if s in self._resident:
                r, rn = self._resident[s]
            else:
                main.wait_event(sl["sent"])
                r, rn = ops.nn_prepare(sl["dev"][:cnt])
                sl["used"] = torch.cuda.Event()
                sl["used"].record(main)
                nbytes = r.numel() + 4 * rn.numel()
                if self._resident_bytes + nbytes <= self.budget:
                    self._resident[s] = (r, rn)
                    self._resident_bytes += nbytes
            fn(s, r, rn)
            if k + 1 < len(starts):
                upload(k + 1)                                   # gathered and sent while the kernel of block k runs
        main.wait_stream(self._copy)
        torch.cuda.synchronize(dev)                             # the staging buffers go out of scope below


def _key_rows(best):
    """The uint64 keys of an int64 device accumulator, on the host."""
    return best.cpu().numpy().view(np.uint64)


def _count_rows(counts):
    """The int64 counts of an int32 device accumulator, on the host."""
    return counts.cpu().numpy().astype(np.int64)


def fitted_search(ref, device, block_rows=16384, resident_gb=8.0, query_rows=16384):
    """A NearestSearch on `device`, fitted to the reference cache."""
    return NearestSearch(device, block_rows=block_rows, resident_gb=resident_gb, query_rows=query_rows).fit(ref)


# ---- metrics -------------------------------------------------------------------------------------------------------------------------

QUANTILES = (("min", 0.0), ("p01", 0.01), ("p05", 0.05), ("p50", 0.5))


def _order_stats(d2):
    """Order statistics of the integer distances: the p-quantile is element floor(p (n - 1)) of the sorted array (no
    interpolation, so it is one of the integers); dcr = sqrt(d2) / 255 is the Euclidean distance in [0, 1]-pixel units."""
    s = np.sort(np.asarray(d2, dtype=np.int64))
    n = len(s)
    out = {}
    for name, p in QUANTILES:
        v = int(s[int(math.floor(p * (n - 1)))])
        out["d2_" + name] = v
        out["dcr_" + name] = math.sqrt(v) / 255.0
    return out


def dcr_metrics(key_train, key_heldout=None):
    """Figures of one query set from its keys against the training set (and a held-out set): exact up to the final divisions.
    duplicates = #{d2 == 0}; closer_to_train_share = (#{d2_t < d2_h} + #{d2_t == d2_h} / 2) / n with its binomial standard error
    sqrt(s (1 - s) / n)."""
    dt, _ = split_keys(key_train)
    n = len(dt)
    if n < 1:
        raise ValueError("no keys")
    out = {"n": n, "duplicates": int((dt == 0).sum())}
    out.update(_order_stats(dt))
    if key_heldout is not None:
        dh, _ = split_keys(key_heldout)
        if len(dh) != n:
            raise ValueError("%d train keys and %d held-out keys" % (n, len(dh)))
        closer, ties = int((dt < dh).sum()), int((dt == dh).sum())
        share = (closer + 0.5 * ties) / n
        out.update(closer_to_train=closer, ties=ties, closer_to_train_share=share,
                   closer_to_train_stderr=math.sqrt(share * (1.0 - share) / n), heldout_duplicates=int((dh == 0).sum()))
        out.update({"heldout_" + k: v for k, v in _order_stats(dh).items()})
    return out
