"""Do the samples have the data's second-order structure?  `python -m csl_gan_amd.frechet --syn_cache out/syn [more ...] --train_cache
out/train [--nontrain_cache out/heldout --baseline] [-d cuda:0] [--block_rows N] [--resident_gb G] [--values_dir DIR] [--save
--outputs_dir outputs/ --name frechet]`.

The Fréchet distance (csl_gan_amd.moments) between the Gaussians fitted to the cache BYTES of every synthetic cache (what `gensamples
--cache` wrote) and of the training cache: the formula of FID without its borrowed network, so it also covers CelebA.  The training set's
moments and the root of its covariance are computed once for all synthetic caches.  --baseline reports the held-out set as if it were
the samples: the distance is biased upward at small N, so it cannot be read without that real-vs-real line.  --values_dir keeps the
integer moments as int64 .npy; with --save the figures are merged into `<outputs_dir>/<name>.json`.  The moments are exact and the same
on `-d cpu` (the host model) and on a device; the float step runs on the host in float64 from them on both paths.
"""
import argparse
import sys

from . import cache_cli, moments, pipeline


def build_parser():
    ap = argparse.ArgumentParser(description="Fréchet distance of a synthetic image cache to the training cache, on the cache bytes")
    cache_cli.add_common_arguments(ap, "frechet", "uint8 image cache(s) of synthetic samples",
                                   "keep <set>_s1.npy and <set>_s2.npy, the integer moments as int64, here; s2 is 8 * D * D bytes per set")
    cache_cli.add_search_arguments(ap, "images per device block", "memory for the D x D int64 second moments and the workspace of a block")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, default=None, help="uint8 image cache of the held-out set")
    ap.add_argument("--baseline", default=False, action="store_true", help="also report the held-out set as if it were the samples")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.baseline and not a.nontrain_cache:
        raise SystemExit("--baseline reports the held-out set against the training set: give --nontrain_cache")
    train = pipeline.CachedImages(a.train_cache)
    extra = [("baseline_heldout", a.nontrain_cache, pipeline.CachedImages(a.nontrain_cache))] if a.baseline else []
    sets = cache_cli.open_syn_caches(a.syn_cache, train, a.train_cache, [(p, c) for _, p, c in extra]) + extra
    kw = cache_cli.search_kw(a)
    D = train.H * train.W * train.C
    try:
        for c in [train] + [c for _, _, c in sets]:
            moments.check_sizes(len(c), D, a.block_rows, a.resident_gb)
    except ValueError as e:
        raise SystemExit(str(e))

    real = moments.real_side(train, **kw)                      # once for all synthetic caches
    stats = {}
    for lab, _, c in sets:
        m, mom = moments.run_frechet(real, c, **kw)
        stats[lab] = m
        cache_cli.save_values(a.values_dir, {"%s_s1" % lab: mom["s1"], "%s_s2" % lab: mom["s2"]})       # set by set: s2 is large
        print("%s: %d samples against %d images of %d bytes: fd %.4f bytes^2 (%.6f of the range squared, %.4f per byte), mean %.4f, "
              "traces %.4f, root %.4f" % (lab, m["n_b"], m["n_a"], m["dim"], m["fd"], m["fd_unit"], m["fd_per_dim"], m["mean_term"],
                                          m["trace_term"], m["sqrt_term"]))
    return cache_cli.report(a, stats)


if __name__ == "__main__":
    main(sys.argv[1:])
