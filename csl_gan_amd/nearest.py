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
import json
import os
import sys

import numpy as np
import torch

from . import neighbours, pipeline, util


def build_parser():
    ap = argparse.ArgumentParser(description="Exact nearest-neighbour audit of a synthetic image cache")
    ap.add_argument("--syn_cache", type=str, nargs="+", required=True, help="uint8 image cache(s) of synthetic samples")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, default=None, help="uint8 image cache of the held-out set")
    ap.add_argument("-d", "--device", type=str, default="cpu")
    ap.add_argument("--block_rows", type=int, default=16384, help="reference images per device block")
    ap.add_argument("--resident_gb", type=float, default=8.0, help="device memory for prepared reference blocks kept between queries")
    ap.add_argument("--baseline", default=False, action="store_true", help="also report held-out -> train")
    ap.add_argument("--grid", type=int, default=0, help="picture grid of the K samples closest to the training set")
    ap.add_argument("--values_dir", type=str, default=None, help="keep the key arrays as .npy here")
    ap.add_argument("--outputs_dir", type=str, default="outputs/")
    ap.add_argument("--name", type=str, default="nearest")
    ap.add_argument("--save", default=False, action="store_true", help="merge the figures into <outputs_dir>/<name>.json")
    return ap


def _label(path):
    return os.path.basename(os.path.normpath(path))


def _same_geometry(a, pa, b, pb):
    if (a.H, a.W, a.C) != (b.H, b.W, b.C):
        raise SystemExit("%s holds %dx%dx%d images and %s %dx%dx%d images: the caches of one audit must have one geometry"
                         % (pa, a.H, a.W, a.C, pb, b.H, b.W, b.C))


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
    syns = [(p, pipeline.CachedImages(p)) for p in a.syn_cache]
    if heldout is not None:
        _same_geometry(train, a.train_cache, heldout, a.nontrain_cache)
    for p, c in syns:
        _same_geometry(train, a.train_cache, c, p)
    if len({_label(p) for p, _ in syns}) != len(syns):
        raise SystemExit("two --syn_cache share the name %s" % ", ".join(sorted(_label(p) for p, _ in syns)))

    def search(ref):
        return neighbours.NearestSearch(a.device, block_rows=a.block_rows, resident_gb=a.resident_gb).fit(ref)

    # one reference at a time on the device: all queries against the training set, then all against the held-out set
    keys = {}
    s = search(train)
    for p, c in syns:
        keys[_label(p), "train"] = s.query(c)
    if a.baseline:
        keys["baseline", "train"] = s.query(heldout)
    if heldout is not None:
        s = search(heldout)
        for p, c in syns:
            keys[_label(p), "heldout"] = s.query(c)
    del s

    stats = {}
    for p, c in syns:
        lab = _label(p)
        stats[lab] = neighbours.dcr_metrics(keys[lab, "train"], keys.get((lab, "heldout")))
        m = stats[lab]
        print("%s: %d samples, %d duplicates of a training image, d2 min / 1%% / 50%% = %d / %d / %d" % (lab, m["n"], m["duplicates"], m["d2_min"],
                                                                                                       m["d2_p01"], m["d2_p50"])
              + ("" if heldout is None else ", closer to train: %.4f (+- %.4f)" % (m["closer_to_train_share"], m["closer_to_train_stderr"])))
    if a.baseline:
        stats["baseline_heldout_to_train"] = neighbours.dcr_metrics(keys["baseline", "train"])
    if a.values_dir:
        os.makedirs(a.values_dir, exist_ok=True)
        for (lab, side), k in keys.items():
            np.save(os.path.join(a.values_dir, "%s_keys_%s.npy" % (lab, side)), k)
    if a.grid > 0:
        os.makedirs(a.outputs_dir, exist_ok=True)
        for p, c in syns:
            lab = _label(p)
            png = os.path.join(a.outputs_dir, "%s_%s_nearest.png" % (a.name, lab))
            write_grid(png, a.grid, c, train, keys[lab, "train"], heldout, keys.get((lab, "heldout")))
            print("saved %s" % png)
    print(json.dumps(stats, indent=4))
    if a.save:
        os.makedirs(a.outputs_dir, exist_ok=True)
        json_path = os.path.join(a.outputs_dir, a.name + ".json")
        merged = {}
        if os.path.exists(json_path):
            with open(json_path) as f:
                merged = json.load(f)
        merged.update(stats)
        with open(json_path, "w") as f:
            json.dump(merged, f)
        print("saved %s" % json_path)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
