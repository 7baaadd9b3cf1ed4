"""What `python -m csl_gan_amd.tstr --classifier dt / rf` costs on one MI355X, in ONE process:

  (1) cslgan_tree_best_split_u8 at the root (K segments, each all N rows) and at a deep level (the rows cut into nodes of 8, for every
      class: N K / 8 segments), and cslgan_tree_apply_u8 (100 random trees of 255 nodes), at 10000 x 12288 bytes (K = 2) and
      60000 x 784 (K = 10), random bytes and labels.  HIP events around each call, warm-up calls thrown away, every repetition
      printed, the median quoted.  The yardstick: a device-to-device copy of the same bytes timed the same way in the same process;
  (2) tstr.main --classifier dt and --classifier rf end to end (host clock, cache reading and the copies to the device included) on
      caches of a ten-class blob problem, 10000 synthetic and 2000 test images of 28 x 28 x 1, beside
      scikit-learn's OneVsRestClassifier(DecisionTreeClassifier()) / (RandomForestClassifier(n_estimators)) on the same bytes / 255
      on the host when scikit-learn is importable.  (-d cpu is not timed: the host model is the definition the device is held to, a
      numpy sort per node, and takes minutes at this size.)

    python scripts/tree_bench.py [--reps 5] [--warmup 2] [--cli true] [--n_trees 100] [--out FILE]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import classify, ops, options, pipeline, tstr  # noqa: E402
from tstr_bench import HBM_BYTES_PER_S, event_times  # noqa: E402

SHAPES = [(10000, 12288, 2), (60000, 784, 10)]


def blobs(n, K, seed, side=28):
    """A blob per class on a noisy background, 10 % of the labels redrawn: uint8 [n, side, side, 1] and int64 labels."""
    rng = np.random.default_rng(seed)
    y = np.arange(n) % K
    x = rng.integers(0, 60, (n, side, side, 1))
    for k in range(K):
        r, c = 2 + 5 * (k // 2), 3 + 12 * (k % 2)
        x[y == k, r:r + 6, c:c + 9] += rng.integers(60, 190, (int((y == k).sum()), 6, 9, 1))
    y = np.where(rng.random(n) < 0.10, rng.integers(0, K, n), y)
    return x.astype(np.uint8), y.astype(np.int64)


def write_cache(path, x, y):
    u8p, labp, hdrp = pipeline.cache_paths(path)
    np.save(open(u8p, "wb"), x)
    np.save(labp, y)
    with open(hdrp, "w") as f:
        json.dump({"version": pipeline.CACHE_VERSION, "n": len(x), "H": x.shape[1], "W": x.shape[2], "C": x.shape[3], "signed": False,
                   "dtype": "uint8", "layout": "NHWC"}, f)
    return path


def random_trees(rng, T, D, nodes):
    """T complete trees of `nodes` (2^d - 1) nodes as flat tables."""
    inner = nodes // 2
    feature = np.concatenate([rng.integers(0, D, inner), np.full(nodes - inner, -1)])
    child = np.concatenate([1 + 2 * np.arange(inner), np.full(nodes - inner, -1)])
    f = np.concatenate([np.where(feature >= 0, rng.integers(0, D, nodes), -1) for _ in range(T)])
    return f, rng.integers(0, 255, T * nodes), np.tile(child, T), np.arange(T + 1) * nodes


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cli", type=options.str2bool, default=True)
    ap.add_argument("--n_trees", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tree_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    i32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    rng = np.random.default_rng(5)
    say("tree_bench: %s, random bytes; %d warm-up + %d timed calls (HIP events), all values then the median"
        % (torch.cuda.get_device_name(0), a.warmup, a.reps))
    for N, D, K in SHAPES:
        X = torch.randint(0, 256, (N, D), device=dev, dtype=torch.uint8, generator=g)
        y = torch.randint(0, K, (N,), device=dev, generator=g).to(torch.int32)
        Y = torch.empty_like(X)
        t_read = N * D / HBM_BYTES_PER_S * 1e6
        t_copy = float(np.median(event_times(lambda i: Y.copy_(X), a.warmup, a.reps)))
        say("(1) %d x %d, K = %d (%.0f MB): device-to-device copy median %.1f us (%.2f TB/s read + written); one read at 6.29 TB/s: %.1f us"
            % (N, D, K, N * D / 1e6, t_copy, 2 * N * D / t_copy / 1e6, t_read))
        del Y
        deep = N // 8
        cases = (("root: %d segments of %d rows" % (K, N), np.tile(np.arange(N), K), np.arange(K + 1) * N, np.arange(K)),
                 ("deep level: %d segments of 8 rows" % (deep * K), np.concatenate([rng.permutation(N)[:deep * 8] for _ in range(K)]),
                  np.arange(deep * K + 1) * 8, np.repeat(np.arange(K), deep)))
        for name, rows, off, cls in cases:
            rows, off, cls = i32(rows), i32(off), i32(cls)
            S = cls.numel()
            ws = torch.empty(ops.tree_best_split_ws_bytes(S, D), device=dev, dtype=torch.uint8)
            out = ops.tree_best_split_u8(X, y, K, rows, off, cls, ws=ws)
            t = event_times(lambda i: ops.tree_best_split_u8(X, y, K, rows, off, cls, out=out, ws=ws), a.warmup, a.reps)
            med = float(np.median(t))
            say("    cslgan_tree_best_split_u8, %s (%d row visits x %d bytes): %s us, median %.1f us = %.2fx the copy, %.2f TB/s of bytes"
                % (name, rows.numel(), D, " / ".join("%.1f" % v for v in t), med, med / t_copy, rows.numel() * D / med / 1e6))
            del ws, out
        tabs = [i32(t) for t in random_trees(rng, 100, D, 255)]
        leaf = ops.tree_apply_u8(X, *tabs)
        t = event_times(lambda i: ops.tree_apply_u8(X, *tabs, out=leaf), a.warmup, a.reps)
        say("    cslgan_tree_apply_u8, 100 trees of 255 nodes (depth 7): %s us, median %.1f us = %.2fx the copy"
            % (" / ".join("%.1f" % v for v in t), float(np.median(t)), float(np.median(t)) / t_copy))
        del X, leaf
        torch.cuda.empty_cache()

    if a.cli:
        tmp = tempfile.mkdtemp(prefix="tree_bench_")
        (x, yy), (xt, yt) = blobs(10000, 10, 1), blobs(2000, 10, 2)
        syn, test = write_cache(os.path.join(tmp, "syn"), x, yy), write_cache(os.path.join(tmp, "test"), xt, yt)
        say("(2) ten-class blobs, 10000 synthetic and 2000 test images of 28 x 28 x 1 (784 bytes), 10 % of the labels redrawn")
        for flags in (["--classifier", "dt"], ["--classifier", "dt"], ["--classifier", "rf", "--n_trees", str(a.n_trees)]):
            t0 = time.perf_counter()
            res = tstr.main(["--syn_cache", syn, "--test_cache", test, "-d", "cuda:0"] + flags)["syn"]
            torch.cuda.synchronize()
            f = res["fit"]
            say("    tstr.main %s -d cuda:0: %.2f s (host clock); %d trees, %d nodes, depth <= %d, %d levels; AUROC %.4f, accuracy %d / %d"
                % (" ".join(flags), time.perf_counter() - t0, len(f["nodes"]), sum(f["nodes"]), max(f["depth"]), f["levels"],
                   res["auroc_micro"], res["accuracy_hits"], res["n_test"]))
        try:
            from sklearn.ensemble import RandomForestClassifier
            from sklearn.multiclass import OneVsRestClassifier
            from sklearn.tree import DecisionTreeClassifier
        except ImportError:
            say("    scikit-learn is not importable here: no host reference times")
        else:
            xs, xts = x.reshape(len(x), -1) / 255.0, xt.reshape(len(xt), -1) / 255.0
            for name, est in (("DecisionTreeClassifier()", DecisionTreeClassifier(random_state=0)),
                              ("RandomForestClassifier(n_estimators=%d)" % a.n_trees, RandomForestClassifier(n_estimators=a.n_trees, random_state=0))):
                t0 = time.perf_counter()
                P = OneVsRestClassifier(est).fit(xs, yy).predict_proba(xts)
                dt = time.perf_counter() - t0
                acc = classify.accuracy(P, yt)
                say("    scikit-learn OneVsRestClassifier(%s), one thread, fit + predict_proba: %.2f s; AUROC %.4f, accuracy %d / %d"
                    % (name, dt, classify.auroc(P, yt)["micro"], acc["hits"], acc["n"]))
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
