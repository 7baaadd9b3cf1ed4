"""Can a test tell the samples from the data?  `python -m csl_gan_amd.mmd --syn_cache out/syn [more ...] --train_cache out/train
[--nontrain_cache out/heldout --baseline] [--n_real M] [--n_perms 1000] [--scales 0.25 1 4] [--seed 0] [-d cuda:0] [--values_dir DIR]
[--save --outputs_dir outputs/ --name mmd]`.

The kernel two-sample test (csl_gan_amd.kernel_test) between the cache BYTES of every synthetic cache (what `gensamples --cache` wrote)
and --n_real rows of the training cache (default: as many as the synthetic cache holds, capped so that the pool keeps to 65536 rows):
the unbiased MMD^2 under the mean of Gaussian kernels at --scales times the median squared distance, and the p-value of a permutation
test over --n_perms relabellings of the pool.  No borrowed network, so it also covers CelebA.  --baseline reports the held-out set as if
it were the samples: the real-vs-real line, whose p-value is uniform.  --values_dir keeps the integer sums as int64 .npy and the
statistics T as decimal strings; with --save the figures are merged into `<outputs_dir>/<name>.json`.  Every figure follows from exact
integers and is the same on `-d cpu` (the host model) and on a device.
"""
import argparse
import sys

import numpy as np

from . import cache_cli, kernel_test, pipeline


def build_parser():
    ap = argparse.ArgumentParser(description="Kernel two-sample test (MMD) of a synthetic image cache against the training cache, on the cache bytes")
    cache_cli.add_common_arguments(ap, "mmd", "uint8 image cache(s) of synthetic samples",
                                   "keep <set>_sxx2.npy, <set>_sxy.npy, <set>_tot2.npy (int64) and <set>_T.npy (decimal strings) here")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, default=None, help="uint8 image cache of the held-out set")
    ap.add_argument("--baseline", default=False, action="store_true", help="also report the held-out set as if it were the samples")
    ap.add_argument("--n_real", type=int, default=None, help="rows of the training cache in the pool (default: as many as the synthetic cache "
                    "holds, capped so that the pool keeps to %d rows)" % kernel_test.MAX_POOL)
    ap.add_argument("--n_perms", type=int, default=1000, help="relabellings of the permutation test")
    ap.add_argument("--scales", type=float, nargs="+", default=list(kernel_test.DEFAULT_SCALES),
                    help="bandwidths as multiples of the median squared distance, at most %d" % kernel_test.MAX_SCALES)
    ap.add_argument("--seed", type=int, default=0, help="of the real rows and the relabellings")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.baseline and not a.nontrain_cache:
        raise SystemExit("--baseline reports the held-out set against the training set: give --nontrain_cache")
    if a.n_perms < 1 or (a.n_real is not None and a.n_real < 2):
        raise SystemExit("--n_perms %d, --n_real %s: need at least one relabelling and two real rows" % (a.n_perms, a.n_real))
    train = pipeline.CachedImages(a.train_cache)
    extra = [("baseline_heldout", a.nontrain_cache, pipeline.CachedImages(a.nontrain_cache))] if a.baseline else []
    sets = cache_cli.open_syn_caches(a.syn_cache, train, a.train_cache, [(p, c) for _, p, c in extra]) + extra
    real = kernel_test.real_side(train, a.seed, a.n_real)
    try:
        for _, _, c in sets:
            kernel_test.check_sizes(len(c), real.count(len(c)))
        kernel_test.kernel_tables(1, a.scales)
    except ValueError as e:
        raise SystemExit(str(e))

    stats = {}
    for lab, _, c in sets:
        try:
            m, vals = kernel_test.run_mmd(real, c, a.n_perms, a.scales, a.device)
        except ValueError as e:                                # a median of zero: the pool is mostly copies of one row
            raise SystemExit("%s: %s" % (lab, e))
        stats[lab] = m
        cache_cli.save_values(a.values_dir, {"%s_sxx2" % lab: vals["sxx2"], "%s_sxy" % lab: vals["sxy"],
                                             "%s_tot2" % lab: np.array([vals["tot2"]], dtype=np.int64),
                                             "%s_T" % lab: np.array([str(t) for t in vals["T"]])})
        print("%s: %d samples against %d images: mmd2 %.6e, p %.4f (%d of %d relabellings at or above it, %d equal), z %.2f, median d2 %d"
              % (lab, m["n_syn"], m["n_real"], m["mmd2"], m["p_value"], m["n_ge"], m["n_perms"], m["n_eq"], m["z_score"], m["median_d2"]))
    return cache_cli.report(a, stats)


if __name__ == "__main__":
    main(sys.argv[1:])
