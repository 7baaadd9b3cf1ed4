"""How far are the samples from the data?  `python -m csl_gan_amd.swd --syn_cache out/syn [more ...] --train_cache out/train
[--nontrain_cache out/heldout --baseline] [--n_dirs 1024] [--seed 0] [--per_class] [-d cuda:0] [--block_rows N] [--resident_gb G]
[--values_dir DIR] [--save --outputs_dir outputs/ --name swd]`.

The sliced Wasserstein distance (csl_gan_amd.sliced) of every synthetic cache (what `gensamples --cache` wrote) to the training cache, on
the cache bytes: the distance between the two distributions that needs no borrowed network, so it also covers CelebA.  The training set
is projected and sorted once for all synthetic caches.  --baseline reports the held-out set as if it were the samples: the real-vs-real
line, the sampling floor without which an SWD cannot be read.  --per_class adds the distance inside every label that both sets hold.
--values_dir keeps the numerators as int64 .npy; with --save the figures are merged into `<outputs_dir>/<name>.json`.  The numerators
are exact and the same on `-d cpu` (the host models) and on a device, and so are the figures computed from them.
"""
import argparse
import sys

import numpy as np

from . import cache_cli, pipeline, sliced


def build_parser():
    ap = argparse.ArgumentParser(description="Sliced Wasserstein distance of a synthetic image cache to the training cache")
    cache_cli.add_common_arguments(ap, "swd", "uint8 image cache(s) of synthetic samples", "keep the numerators as int64 .npy here")
    cache_cli.add_search_arguments(ap, "images per device block", "device memory for the projections and the workspace of their sort")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, default=None, help="uint8 image cache of the held-out set")
    ap.add_argument("--baseline", default=False, action="store_true", help="also report the held-out set as if it were the samples")
    ap.add_argument("--n_dirs", type=int, default=1024, help="Rademacher directions")
    ap.add_argument("--seed", type=int, default=0, help="seed of the direction stream")
    ap.add_argument("--per_class", default=False, action="store_true", help="also report every label that both sets hold")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.baseline and not a.nontrain_cache:
        raise SystemExit("--baseline reports the held-out set against the training set: give --nontrain_cache")
    if a.n_dirs < 1:
        raise SystemExit("--n_dirs %d: the distance needs at least one direction" % a.n_dirs)
    train = pipeline.CachedImages(a.train_cache)
    extra = [("baseline_heldout", a.nontrain_cache, pipeline.CachedImages(a.nontrain_cache))] if a.baseline else []
    sets = cache_cli.open_syn_caches(a.syn_cache, train, a.train_cache, [(p, c) for _, p, c in extra]) + extra
    try:
        for _, _, c in sets:
            sliced.check_sizes(len(train), len(c))
    except ValueError as e:
        raise SystemExit(str(e))

    kw = cache_cli.search_kw(a)
    D = train.H * train.W * train.C
    real = sliced.real_side(train, a.n_dirs, a.seed, per_class=a.per_class, **kw)           # once for all synthetic caches
    stats, values = {}, {}
    for lab, _, c in sets:
        v = sliced.run_swd(real, c, per_class=a.per_class, **kw)
        m = stats[lab] = sliced.swd_metrics(v["num"], len(train), len(c), D, a.seed)
        values["%s_num" % lab] = v["num"]
        if a.per_class:
            m["per_class"] = {}
            for l, (num, na, nb) in v["per_class"].items():
                m["per_class"][str(l)] = sliced.swd_metrics(num, na, nb, D, a.seed)
                values["%s_num_class%d" % (lab, l)] = num
        print("%s: %d samples against %d images, %d directions: swd %.4f bytes (%.6f of the range), max sliced %.4f, stderr %.4f"
              % (lab, m["n_b"], m["n_a"], m["n_dirs"], m["swd"], m["swd_unit"], m["max_sliced"], m["stderr"]))
    cache_cli.save_values(a.values_dir, {name: np.asarray(arr, dtype=np.int64) for name, arr in values.items()})
    return cache_cli.report(a, stats)


if __name__ == "__main__":
    main(sys.argv[1:])
