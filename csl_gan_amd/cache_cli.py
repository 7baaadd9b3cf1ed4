"""What the command lines over image caches share (csl_gan_amd.nearest, sample_attack, prdc, swd, frechet, mmd, tstr): the arguments every one of them
takes, how the synthetic caches are opened, named and checked, and how values and figures are written.  A tool decides what it
computes and under which names and dtypes it keeps it; how a set gets its name and where the results go is decided here.
"""
import json
import os

import numpy as np

from . import pipeline


def add_common_arguments(ap, name, syn_help, values_help):
    """--syn_cache, -d, --values_dir, --outputs_dir, --name (default: the tool's `name`) and --save."""
    ap.add_argument("--syn_cache", type=str, nargs="+", required=True, help=syn_help)
    ap.add_argument("-d", "--device", type=str, default="cpu")
    ap.add_argument("--values_dir", type=str, default=None, help=values_help)
    ap.add_argument("--outputs_dir", type=str, default="outputs/")
    ap.add_argument("--name", type=str, default=name)
    ap.add_argument("--save", default=False, action="store_true", help="merge the figures into <outputs_dir>/<name>.json")


def add_search_arguments(ap, block_help, resident_help):
    """--block_rows and --resident_gb of the tools that walk a reference with neighbours.NearestSearch."""
    ap.add_argument("--block_rows", type=int, default=16384, help=block_help)
    ap.add_argument("--resident_gb", type=float, default=8.0, help=resident_help)


def search_kw(a):
    """The parsed search arguments as the keywords of neighbours.fitted_search, blackbox.run_attack and manifold.run_prdc."""
    return dict(device=a.device, block_rows=a.block_rows, resident_gb=a.resident_gb)


def label_of(path):
    """The name of a set in the figures and the file names: the last component of its cache's path."""
    return os.path.basename(os.path.normpath(path))


def open_syn_caches(paths, anchor, anchor_path, others=()):
    """[(label, path, cache)] of the --syn_cache paths.  The tool exits when one of `others` (its further (path, cache)) or of the
    synthetic caches, in that order, holds images of another height, width or channel count than the anchor cache, and when two
    synthetic paths give one label."""
    sets = [(label_of(p), p, pipeline.CachedImages(p)) for p in paths]
    a = anchor
    for p, b in list(others) + [(p, c) for _, p, c in sets]:
        if (a.H, a.W, a.C) != (b.H, b.W, b.C):
            raise SystemExit("%s holds %dx%dx%d images and %s %dx%dx%d images: the caches of one audit must have one geometry"
                             % (anchor_path, a.H, a.W, a.C, p, b.H, b.W, b.C))
    if len({lab for lab, _, _ in sets}) != len(sets):
        raise SystemExit("two --syn_cache share the name %s" % ", ".join(sorted(lab for lab, _, _ in sets)))
    return sets


def cache_rows(cache):
    """(bytes [n, H*W*C] uint8, a copy in memory; labels [n] int64) of a pipeline.CachedImages."""
    return np.array(cache.x, dtype=np.uint8).reshape(len(cache), -1), np.asarray(cache.labels, dtype=np.int64).reshape(-1)


def save_values(values_dir, arrays):
    """<values_dir>/<name>.npy for every (name, array) of the dict, as the caller typed them; nothing without --values_dir."""
    if not values_dir:
        return
    os.makedirs(values_dir, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(values_dir, name + ".npy"), arr)


def report(a, stats):
    """Print the figures as JSON and, with --save, merge them into <outputs_dir>/<name>.json (sets of earlier runs stay)."""
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
