"""Precision, recall, density and coverage of a synthetic image cache (include/cslgan.h "Nearest-neighbour audit").

The k-nearest-neighbour manifold figures that need no borrowed network: improved precision and recall (Kynkäänniemi et al., NeurIPS
2019) and density and coverage (Naeem et al., ICML 2020), on the cache BYTES under d2 of csl_gan_amd.neighbours.  N real rows X, M
synthetic rows S, 1 <= k <= 8:

    rad_X[x] = d2 of the k-th nearest OTHER row of X (the row is left out by its index; a twin with the same bytes counts, at 0)
    rad_S[s] = the same inside S
    c[s]     = #{x : d2(s, x) <= rad_X[x]}

    precision = #{s : c[s] > 0} / M                               density  = sum_s c[s] / (k M)
    recall    = #{x : #{s : d2(x, s) <= rad_S[s]} > 0} / N        coverage = #{x : min_s d2(x, s) <= rad_X[x]} / N

The compare is `<=`, as in Kynkäänniemi et al. and as in cslgan_nn_count_i8.  The `prdc` PyPI package uses `<`; the two differ on
exact ties only, which integer distances do produce.  Every numerator is an integer and is reported, so the figures are
bit-identical on the CPU (`neighbours.kth_host`, `neighbours.count_within_radii_host`: THE definitions) and on a device
(ops.nn_kth / ops.nn_count_radius through NearestSearch), which is held to them by equality.
"""
from __future__ import annotations

import numpy as np

from . import neighbours
from .neighbours import MAX_K, MAX_RADIUS, NONE_KEY, check_radii, count_within_radii_host  # noqa: F401  (the names stay reachable here)

def knn_radii(keys):
    """int64 [n]: the k-NN radius of every row from its list of a self-excluding search (uint64 [n, k]): the d2 of the last entry.
    A list with an all-ones entry comes from a set of fewer than k + 1 rows and is refused."""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.ndim != 2 or not 1 <= keys.shape[1] <= MAX_K or keys.shape[0] < 1:
        raise ValueError("need keys [n, k] with k in 1 .. %d, got %s" % (MAX_K, keys.shape))
    if (keys[:, -1] == NONE_KEY).any():
        raise ValueError("a list of %d neighbours is not full: the set needs at least %d rows" % (keys.shape[1], keys.shape[1] + 1))
    return (keys[:, -1] >> np.uint64(32)).astype(np.int64)


def prdc_metrics(counts_syn, counts_real, d2min_real, rad_real, k):
    """The figures of one synthetic cache from its integers: counts_syn[s] = #{x : d2(s, x) <= rad_X[x]} (M entries),
    counts_real[x] = #{s : d2(x, s) <= rad_S[s]}, d2min_real[x] = min_s d2(x, s) and rad_real = rad_X (N entries each).  The four
    numerators are exact; each ratio is one division."""
    cs, cr = np.asarray(counts_syn, dtype=np.int64).reshape(-1), np.asarray(counts_real, dtype=np.int64).reshape(-1)
    dm, rx = np.asarray(d2min_real, dtype=np.int64).reshape(-1), np.asarray(rad_real, dtype=np.int64).reshape(-1)
    k = int(k)
    M, N = len(cs), len(cr)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d; need 1 .. %d" % (k, MAX_K))
    if M < 1 or N < 1 or len(dm) != N or len(rx) != N:
        raise ValueError("%d synthetic counts; %d / %d / %d real counts / distances / radii" % (M, N, len(dm), len(rx)))
    p, d, r, c = int((cs > 0).sum()), int(cs.sum()), int((cr > 0).sum()), int((dm <= rx).sum())
    return {"n_real": N, "n_syn": M, "k": k, "precision_hits": p, "density_sum": d, "recall_hits": r, "coverage_hits": c,
            "precision": p / M, "density": d / (k * M), "recall": r / N, "coverage": c / N}


def check_sizes(k, **sets):
    """k in 1 .. 8 and every named cache with more than k rows (its k-NN radius needs k other rows)."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d; need 1 .. %d" % (k, MAX_K))
    for name, c in sets.items():
        if len(c) <= k:
            raise ValueError("%s holds %d images; the radius of the %d-th neighbour needs at least %d" % (name, len(c), k, k + 1))
    return k


def real_side(real, k, device="cpu", block_rows=16384, resident_gb=8.0, query_rows=16384):
    """(the fitted search of the real cache, rad_X): the self-search that all synthetic caches of one run share."""
    k = check_sizes(k, real=real)
    s = neighbours.fitted_search(real, device, block_rows, resident_gb, query_rows)
    return s, knn_radii(s.kth(real, k, exclude_self=True))


def run_prdc(real, syn, k, real_search=None, rad_real=None, device="cpu", block_rows=16384, resident_gb=8.0, query_rows=16384):
    """The integers of one synthetic cache (pipeline.CachedImages both), four passes: its own self-search, synthetic -> real counts,
    real -> synthetic counts, real -> synthetic nearest.  `real_search` / `rad_real` are real_side()'s and are computed when
    absent.  Returns dict(rad_real, rad_syn, counts_syn, counts_real, d2min_real)."""
    k = check_sizes(k, real=real, syn=syn)
    if real_search is None or rad_real is None:
        real_search, rad_real = real_side(real, k, device, block_rows, resident_gb, query_rows)
    out = {"rad_real": rad_real, "counts_syn": real_search.count_within_radii(syn, rad_real)}
    s = neighbours.fitted_search(syn, device, block_rows, resident_gb, query_rows)
    out["rad_syn"] = knn_radii(s.kth(syn, k, exclude_self=True))
    out["counts_real"] = s.count_within_radii(real, out["rad_syn"])
    out["d2min_real"] = neighbours.split_keys(s.query(real))[0]
    return out
