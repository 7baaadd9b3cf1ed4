"""Nearest-neighbour audit of a synthetic dataset: `python -m csl_gan_amd.nearest --syn_cache out/syn [more ...] --train_cache
out/train [--nontrain_cache out/heldout] [-d cuda:0] [--block_rows N] [--resident_gb G] [--baseline] [--grid K] [--values_dir DIR]
[--save --outputs_dir outputs/ --name NAME]`.

For every image of a synthetic cache (what `gensamples --cache` wrote) the exact nearest training image and nearest held-out image
under the squared Euclidean distance on the cache bytes (csl_gan_amd.neighbours), and from the two distances the figures of
neighbours.dcr_metrics: duplicates, the low order statistics of the distance to the closest training record, and the share of
samples that are closer to the training set than to the held-out set (0.5 for a generator that has not memorised).  It audits what
a DP-GAN releases — the samples — where mem_inf_attack audits the critic, and needs no borrowed network, so it also covers CelebA.

Several --syn_cache (one per checkpoint) share one prepared reference.  --baseline adds held-out -> train, the real-to-real
distances that put the synthetic ones in context.  --values_dir keeps the uint64 keys (d2 << 32 | index) as .npy; --grid K writes
`<outputs_dir>/<name>_<syn>_nearest.png`, the K synthetic samples closest to the training set, one per row: synthetic | nearest
train | nearest held-out.  With --save the figures are merged into `<outputs_dir>/<name>.json`.  Every integer printed is exact and
the same on `-d cpu` (the host model) and on a device.
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import cache_cli, neighbours, pipeline, util


def build_parser():
    ap = argparse.ArgumentParser(description="Exact nearest-neighbour audit of a synthetic image cache")
    cache_cli.add_common_arguments(ap, "nearest", "uint8 image cache(s) of synthetic samples", "keep the key arrays as .npy here")
    cache_cli.add_search_arguments(ap, "reference images per device block", "device memory for prepared reference blocks kept between queries")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, default=None, help="uint8 image cache of the held-out set")
    ap.add_argument("--baseline", default=False, action="store_true", help="also report held-out -> train")
    ap.add_argument("--grid", type=int, default=0, help="picture grid of the K samples closest to the training set")
    return ap


def _rows(cache, idx):
    """float [len(idx), C, H, W] in [0, 1] of the cache rows idx: bytes / 255."""
    out = np.empty((len(idx), cache.H, cache.W, cache.C), dtype=np.uint8)
    cache.gather(np.asarray(idx, dtype=np.int64), out)
    return torch.from_numpy(out).float().div(255.0).permute(0, 3, 1, 2)


def write_grid(path, K, syn, train, key_train, heldout=None, key_heldout=None):
    """Rows of synthetic | nearest train | nearest held-out for the K samples with the smallest training key."""
    pick = np.argsort(np.asarray(key_train, dtype=np.uint64), kind="stable")[:K]
    cols = [_rows(syn, pick), _rows(train, neighbours.split_keys(key_train)[1][pick])]
    if heldout is not None:
        cols.append(_rows(heldout, neighbours.split_keys(key_heldout)[1][pick]))
    imgs = torch.stack(cols, 1).reshape((-1,) + tuple(cols[0].shape[1:]))
    util.save_image(imgs, path, nrow=len(cols))
    return len(pick)


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.baseline and not a.nontrain_cache:
        raise SystemExit("--baseline compares the held-out set with the training set: give --nontrain_cache")
    train = pipeline.CachedImages(a.train_cache)
    heldout = pipeline.CachedImages(a.nontrain_cache) if a.nontrain_cache else None
    syns = cache_cli.open_syn_caches(a.syn_cache, train, a.train_cache, [(a.nontrain_cache, heldout)] if heldout is not None else [])

    # one reference at a time on the device: all queries against the training set, then all against the held-out set
    keys = {}
    s = neighbours.fitted_search(train, **cache_cli.search_kw(a))
    for lab, _, c in syns:
        keys[lab, "train"] = s.query(c)
    if a.baseline:
        keys["baseline", "train"] = s.query(heldout)
    if heldout is not None:
        s = neighbours.fitted_search(heldout, **cache_cli.search_kw(a))
        for lab, _, c in syns:
            keys[lab, "heldout"] = s.query(c)
    del s

    stats = {}
    for lab, _, c in syns:
        stats[lab] = neighbours.dcr_metrics(keys[lab, "train"], keys.get((lab, "heldout")))
        m = stats[lab]
        print("%s: %d samples, %d duplicates of a training image, d2 min / 1%% / 50%% = %d / %d / %d" % (lab, m["n"], m["duplicates"], m["d2_min"],
                                                                                                       m["d2_p01"], m["d2_p50"])
              + ("" if heldout is None else ", closer to train: %.4f (+- %.4f)" % (m["closer_to_train_share"], m["closer_to_train_stderr"])))
    if a.baseline:
        stats["baseline_heldout_to_train"] = neighbours.dcr_metrics(keys["baseline", "train"])
    cache_cli.save_values(a.values_dir, {"%s_keys_%s" % (lab, side): k for (lab, side), k in keys.items()})
    if a.grid > 0:
        os.makedirs(a.outputs_dir, exist_ok=True)
        for lab, _, c in syns:
            png = os.path.join(a.outputs_dir, "%s_%s_nearest.png" % (a.name, lab))
            write_grid(png, a.grid, c, train, keys[lab, "train"], heldout, keys.get((lab, "heldout")))
            print("saved %s" % png)
    return cache_cli.report(a, stats)


if __name__ == "__main__":
    main(sys.argv[1:])
