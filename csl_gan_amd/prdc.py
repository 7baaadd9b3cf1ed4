"""Are the samples good and varied?  `python -m csl_gan_amd.prdc --syn_cache out/syn [more ...] --train_cache out/train
[--nontrain_cache out/heldout --baseline] [-k 5] [-d cuda:0] [--block_rows N] [--resident_gb G] [--values_dir DIR]
[--save --outputs_dir outputs/ --name prdc]`.

Precision, recall, density and coverage (csl_gan_amd.manifold) of every synthetic cache (what `gensamples --cache` wrote) against
the training cache, on the cache bytes: the quality and diversity figures that need no borrowed network, so they also cover
CelebA.  The self-search of the training set runs once for all synthetic caches; per synthetic cache there are four passes: its own
self-search, synthetic -> real counts, real -> synthetic counts, real -> synthetic nearest.  --baseline reports the held-out set as
if it were the samples, the real-vs-real line that puts the synthetic ones in context.  --values_dir keeps the radii, counts and
distances as int64 .npy; with --save the figures are merged into `<outputs_dir>/<name>.json`.  Every integer printed is exact and
the same on `-d cpu` (the host models) and on a device, and so are the four ratios.
"""
import argparse
import sys

import numpy as np

from . import cache_cli, manifold, pipeline


def build_parser():
    ap = argparse.ArgumentParser(description="Precision, recall, density and coverage of a synthetic image cache")
    cache_cli.add_common_arguments(ap, "prdc", "uint8 image cache(s) of synthetic samples", "keep radii, counts and distances as .npy here")
    cache_cli.add_search_arguments(ap, "reference images per device block", "device memory for prepared reference blocks kept between queries")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, default=None, help="uint8 image cache of the held-out set")
    ap.add_argument("--baseline", default=False, action="store_true", help="also report the held-out set as if it were the samples")
    ap.add_argument("-k", type=int, default=5, help="neighbours of the radius, 1 .. 8")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.baseline and not a.nontrain_cache:
        raise SystemExit("--baseline reports the held-out set against the training set: give --nontrain_cache")
    if not 1 <= a.k <= manifold.MAX_K:
        raise SystemExit("-k %d: the radius is that of neighbour 1 .. %d" % (a.k, manifold.MAX_K))
    train = pipeline.CachedImages(a.train_cache)
    extra = [("baseline_heldout", a.nontrain_cache, pipeline.CachedImages(a.nontrain_cache))] if a.baseline else []
    sets = cache_cli.open_syn_caches(a.syn_cache, train, a.train_cache, [(p, c) for _, p, c in extra]) + extra
    try:
        manifold.check_sizes(a.k, **dict([(a.train_cache, train)] + [(p, c) for _, p, c in sets]))
    except ValueError as e:
        raise SystemExit(str(e))

    kw = cache_cli.search_kw(a)
    search, rad_real = manifold.real_side(train, a.k, **kw)              # once for all synthetic caches
    stats, values = {}, {"rad_real": rad_real}
    for lab, _, c in sets:
        v = manifold.run_prdc(train, c, a.k, search, rad_real, **kw)
        del v["rad_real"]
        m = stats[lab] = manifold.prdc_metrics(v["counts_syn"], v["counts_real"], v["d2min_real"], rad_real, a.k)
        values.update({"%s_%s" % (lab, name): arr for name, arr in v.items()})
        print("%s: %d samples against %d images, k = %d: precision %.4f, recall %.4f, density %.4f, coverage %.4f"
              % (lab, m["n_syn"], m["n_real"], m["k"], m["precision"], m["recall"], m["density"], m["coverage"]))
    cache_cli.save_values(a.values_dir, {name: np.asarray(arr, dtype=np.int64) for name, arr in values.items()})
    return cache_cli.report(a, stats)


if __name__ == "__main__":
    main(sys.argv[1:])
