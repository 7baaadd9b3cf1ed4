"""Black-box membership audit of a synthetic image cache (include/cslgan.h "Nearest-neighbour audit").

The adversary holds only the samples S that a generator released and asks of a record x whether it was trained on.  Every score
is an integer function of the cache BYTES under d2 of csl_gan_amd.neighbours, and a larger score means "member":

    d2min(x)   = min over s in S of d2(x, s)                      the high word of NearestSearch.query's key
    s_fbb(x)   = -d2min(x)                                        full black-box attack of GAN-Leaks (Chen et al., CCS 2020)
    s_cal(x)   = d2min_ref(x) - d2min(x)                          the same, calibrated with the samples of a reference generator
    s_mc,p(x)  = #{s in S : d2(x, s) <= eps2_p}                   Monte-Carlo attack of Hilprecht et al. (PoPETs 2019)

eps2_p is element floor(p (n - 1)) of the sorted pooled d2min over train and held-out together — the order-statistic rule of
neighbours.dcr_metrics, no interpolation, no membership label.  `neighbours.count_within_host` is THE definition of the counts, and the
device path (ops.nn_count through NearestSearch.count_within) is held to it by equality.  Scores reach 2^32 and audit's rank
kernels take float32, so `dense_ranks` maps the pooled scores to their rank among the pooled distinct values first: order and ties
survive exactly, and audit.attack_metrics turns them into ASR, AUC and TPR at a fixed FPR, the same integers on every device.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from . import audit, neighbours
from .neighbours import MAX_THRESHOLD, MAX_THRESHOLDS, check_thresholds, count_within_host  # noqa: F401  (the names stay reachable here)

MAX_DISTINCT = 2 ** 24                  # float32 holds every integer up to here
DEFAULT_PERCENTILES = (50.0, 10.0, 1.0, 0.1)


def epsilon2(d2_pooled, percentiles=DEFAULT_PERCENTILES):
    """eps2_p for every percentile p (in percent): element floor(p / 100 (n - 1)) of the sorted pooled d2min, as Python integers.
    The product is formed in exact decimal arithmetic, so 0.1 % of 1000 is element 0 of 1000 values and element 1 of 1001."""
    pct = [float(p) for p in np.asarray(percentiles, dtype=np.float64).reshape(-1)]
    if not 1 <= len(pct) <= MAX_THRESHOLDS:
        raise ValueError("need 1 .. %d percentiles, got %d" % (MAX_THRESHOLDS, len(pct)))
    if any(not 0.0 <= p <= 100.0 for p in pct):
        raise ValueError("percentiles must lie in [0, 100], got %s" % (pct,))
    s = np.sort(np.asarray(d2_pooled, dtype=np.int64).reshape(-1))
    if len(s) < 1:
        raise ValueError("no distances")
    return [int(s[int(math.floor(Fraction(repr(p)) * (len(s) - 1) / 100))]) for p in pct]


def dense_ranks(st, sn):
    """(float32 [len(st)], float32 [len(sn)]): every integer score replaced by its index among the sorted distinct values of both
    sides together.  a < b, a == b and a > b hold for the ranks exactly as for the scores, on and across both sides, which is all
    that audit.attack_metrics reads.  More than 2^24 distinct values do not fit float32 and are refused."""
    st, sn = np.asarray(st, dtype=np.int64).reshape(-1), np.asarray(sn, dtype=np.int64).reshape(-1)
    uniq, inv = np.unique(np.concatenate([st, sn]), return_inverse=True)
    if len(uniq) > MAX_DISTINCT:
        raise ValueError("%d distinct scores; float32 ranks are exact up to %d" % (len(uniq), MAX_DISTINCT))
    inv = inv.reshape(-1).astype(np.float32)
    return inv[:len(st)], inv[len(st):]


def percentile_name(p):
    return "mc_p%g" % p


def attack_scores(d2_train, d2_heldout, counts_train=None, counts_heldout=None, percentiles=(), d2ref_train=None, d2ref_heldout=None):
    """{name: (train scores, held-out scores)} as int64: "fbb", "cal" when the reference distances are given, and one
    "mc_p<percentile>" per column of the counts."""
    dt, dh = np.asarray(d2_train, dtype=np.int64).reshape(-1), np.asarray(d2_heldout, dtype=np.int64).reshape(-1)
    out = {"fbb": (-dt, -dh)}
    if d2ref_train is not None:
        rt, rh = np.asarray(d2ref_train, dtype=np.int64).reshape(-1), np.asarray(d2ref_heldout, dtype=np.int64).reshape(-1)
        if len(rt) != len(dt) or len(rh) != len(dh):
            raise ValueError("calibration distances of %d / %d records for %d / %d" % (len(rt), len(rh), len(dt), len(dh)))
        out["cal"] = (rt - dt, rh - dh)
    if counts_train is not None:
        ct, ch = np.asarray(counts_train, dtype=np.int64), np.asarray(counts_heldout, dtype=np.int64)
        if ct.shape != (len(dt), len(percentiles)) or ch.shape != (len(dh), len(percentiles)):
            raise ValueError("counts of shape %s / %s for %d / %d records and %d percentiles" % (ct.shape, ch.shape, len(dt), len(dh), len(percentiles)))
        for j, p in enumerate(percentiles):
            out[percentile_name(p)] = (ct[:, j], ch[:, j])
    return out


def sample_attack_metrics(d2_train, d2_heldout, counts_train, counts_heldout, percentiles, eps2, n_syn, d2ref_train=None, d2ref_heldout=None,
                          data_prop=0.1, pool=1000, asr_iters=10000, seed=0, device="cpu"):
    """The figures of one synthetic cache: per score of attack_scores the dict of audit.attack_metrics on its dense ranks, plus
    the percentiles with their eps2, the order statistics of the pooled d2min and the sizes."""
    pct = [float(p) for p in percentiles]
    scores = attack_scores(d2_train, d2_heldout, counts_train, counts_heldout, pct, d2ref_train, d2ref_heldout)
    pooled = np.concatenate([np.asarray(d2_train, dtype=np.int64).reshape(-1), np.asarray(d2_heldout, dtype=np.int64).reshape(-1)])
    out = {"n_train": int(len(scores["fbb"][0])), "n_heldout": int(len(scores["fbb"][1])), "n_syn": int(n_syn), "percentiles": pct,
           "eps2": [int(e) for e in eps2], "d2min_pooled": neighbours._order_stats(pooled)}
    for name, (st, sn) in scores.items():
        rt, rn = dense_ranks(st, sn)
        out[name] = audit.attack_metrics(rt, rn, data_prop=data_prop, pool=pool, asr_iters=asr_iters, seed=seed, device=device)
    return out


def d2min_to(ref, caches, device="cpu", block_rows=16384, resident_gb=8.0, query_rows=16384):
    """[d2min of every image of c to the images of `ref`, int64, for c in caches]: the reference is fitted once."""
    s = neighbours.fitted_search(ref, device, block_rows, resident_gb, query_rows)
    return [neighbours.split_keys(s.query(c))[0] for c in caches]


def run_attack(syn, train, heldout, percentiles=DEFAULT_PERCENTILES, device="cpu", block_rows=16384, resident_gb=8.0, query_rows=16384):
    """The integers of the attack on one synthetic cache (pipeline.CachedImages all): S is fitted once, train and held-out are
    queried for d2min, eps2 comes from the pooled d2min, and one counting walk per side gives the Monte-Carlo scores.  Returns
    dict(d2_train, d2_heldout, eps2, counts_train, counts_heldout)."""
    s = neighbours.fitted_search(syn, device, block_rows, resident_gb, query_rows)
    out = {"d2_train": neighbours.split_keys(s.query(train))[0], "d2_heldout": neighbours.split_keys(s.query(heldout))[0]}
    out["eps2"] = epsilon2(np.concatenate([out["d2_train"], out["d2_heldout"]]), percentiles)
    out["counts_train"], out["counts_heldout"] = s.count_within(train, out["eps2"]), s.count_within(heldout, out["eps2"])
    return out
