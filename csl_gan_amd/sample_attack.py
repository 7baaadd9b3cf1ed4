"""Black-box membership audit of a synthetic dataset: `python -m csl_gan_amd.sample_attack --syn_cache out/syn [more ...]
--train_cache out/train --nontrain_cache out/heldout [--calib_cache out/ref_syn] [--percentiles 50 10 1 0.1] [--pool 1000
--data_prop 0.1 --asr_iters 10000 --seed 0] [-d cuda:0 --block_rows N --resident_gb G] [--values_dir DIR] [--save --outputs_dir
outputs/ --name NAME]`.

Given only the samples of a generator, can an adversary tell a training record from a held-out one?  For every synthetic cache
(what `gensamples --cache` wrote) the scores of csl_gan_amd.blackbox — full black-box (distance to the nearest sample), the same
calibrated with the samples of a reference generator (--calib_cache), and Monte-Carlo (samples inside an eps-ball, eps^2 a
percentile of the pooled nearest-sample distances) — and for each of them the figures of audit.attack_metrics: ASR with its
standard error, AUC, and TPR at 1 % and 0.1 % FPR.  `nearest` asks of every sample how close it lies to a record; this asks of
every record how close the samples come, which is the membership question a privacy review puts next to epsilon.

The synthetic cache is fitted once; train and held-out are queried for the nearest sample, and one counting walk per side gives
the Monte-Carlo scores.  --values_dir keeps the distances and counts (int64) as .npy.  With --save the figures are merged into
`<outputs_dir>/<name>.json`.  Every integer printed is exact and the same on `-d cpu` (the host model) and on a device.
"""
import argparse
import sys

import numpy as np

from . import audit, blackbox, cache_cli, pipeline


def build_parser():
    ap = argparse.ArgumentParser(description="Black-box membership audit of a synthetic image cache")
    cache_cli.add_common_arguments(ap, "sample_attack", "uint8 image cache(s) of synthetic samples", "keep the distances and counts as .npy here")
    cache_cli.add_search_arguments(ap, "synthetic images per device block", "device memory for prepared blocks kept between queries")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, required=True, help="uint8 image cache of the held-out set")
    ap.add_argument("--calib_cache", type=str, default=None, help="uint8 image cache of a reference generator's samples (calibrated attack)")
    ap.add_argument("--percentiles", type=float, nargs="+", default=list(blackbox.DEFAULT_PERCENTILES),
                    help="percentiles of the pooled nearest-sample distance that serve as eps^2 of the Monte-Carlo attack (at most 4)")
    ap.add_argument("--pool", type=int, default=1000, help="size of the adversary's pool")
    ap.add_argument("--data_prop", type=float, default=0.1, help="share of training data in the adversary's pool")
    ap.add_argument("--asr_iters", type=int, default=10000, help="subset pairs drawn for the attack success rate")
    ap.add_argument("--seed", type=int, default=0, help="seed of the subset stream")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if not 1 <= len(a.percentiles) <= blackbox.MAX_THRESHOLDS:
        raise SystemExit("--percentiles takes 1 .. %d values, got %d" % (blackbox.MAX_THRESHOLDS, len(a.percentiles)))
    if any(not 0.0 <= p <= 100.0 for p in a.percentiles) or len(set(a.percentiles)) != len(a.percentiles):
        raise SystemExit("--percentiles must be distinct values in [0, 100], got %s" % a.percentiles)
    train, heldout = pipeline.CachedImages(a.train_cache), pipeline.CachedImages(a.nontrain_cache)
    calib = pipeline.CachedImages(a.calib_cache) if a.calib_cache else None
    syns = cache_cli.open_syn_caches(a.syn_cache, train, a.train_cache,
                                     [(a.nontrain_cache, heldout)] + ([(a.calib_cache, calib)] if calib is not None else []))
    n, m = int(a.pool * a.data_prop), int(a.pool * (1 - a.data_prop))
    try:
        audit.check_sizes(len(train), len(heldout), n, m)
    except ValueError as e:
        raise SystemExit("the pool of %d does not fit the caches: %s" % (a.pool, e))

    kw = cache_cli.search_kw(a)
    ref = dict(zip(("d2ref_train", "d2ref_heldout"), blackbox.d2min_to(calib, (train, heldout), **kw))) if calib is not None else {}
    stats, values = {}, {}
    for lab, _, c in syns:
        v = dict(blackbox.run_attack(c, train, heldout, a.percentiles, **kw), **ref)
        values[lab] = v
        m_ = blackbox.sample_attack_metrics(v["d2_train"], v["d2_heldout"], v["counts_train"], v["counts_heldout"], a.percentiles, v["eps2"],
                                            len(c), v.get("d2ref_train"), v.get("d2ref_heldout"), data_prop=a.data_prop, pool=a.pool,
                                            asr_iters=a.asr_iters, seed=a.seed, device=a.device)
        stats[lab] = m_
        print("%s: %d samples against %d train / %d held-out records, eps^2 = %s" % (lab, len(c), len(train), len(heldout), m_["eps2"]))
        for name in [k for k in m_ if isinstance(m_[k], dict) and "auc" in m_[k]]:
            s = m_[name]
            print("  %-8s ASR %.4f (+- %.4f)  AUC %.4f  TPR at 1 %% / 0.1 %% FPR %.4f / %.4f"
                  % (name, s["asr"], s["asr_stderr"], s["auc"], s["tpr_at_fpr_0.01"], s["tpr_at_fpr_0.001"]))
    cache_cli.save_values(a.values_dir, {"%s_%s" % (lab, k): np.asarray(arr, dtype=np.int64)
                                         for lab, v in values.items() for k, arr in v.items() if k != "eps2"})
    return cache_cli.report(a, stats)


if __name__ == "__main__":
    main(sys.argv[1:])
