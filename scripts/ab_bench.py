"""What `python -m csl_gan_amd.tstr --classifier ab` costs on one MI355X, in ONE process:

  (1) cslgan_boost_stump_u8, the stump search of one boosting round for all K classes, at 10000 x 12288 bytes (K = 2) and 60000 x 784
      (K = 10), random bytes and labels, under unit weights and under random weights in 0 .. 2^28 with a fifth of the rows at 0.  HIP
      events around each call, warm-up calls thrown away, every repetition printed, the median quoted.  Two yardsticks timed the same
      way in the same process: a device-to-device copy of the same bytes, and cslgan_tree_best_split_u8 at the root (K segments, each
      all N rows) — the same histograms with 32-bit counts packed into one 64-bit entry;
  (2) tstr.main --classifier ab end to end (host clock, cache reading and the copies to the device included) on caches of a ten-class
      blob problem, 10000 synthetic and 2000 test images of 28 x 28 x 1, beside scikit-learn's AdaBoostClassifier() per class (what
      OneVsRestClassifier fits, one class after the other, one thread) on the same bytes / 255 on the host when scikit-learn is
      importable.

    python scripts/ab_bench.py [--reps 5] [--warmup 2] [--cli true] [--n_rounds 50] [--out FILE]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import classify, ops, options, tstr  # noqa: E402
from tree_bench import SHAPES, blobs, write_cache  # noqa: E402
from tstr_bench import HBM_BYTES_PER_S, event_times  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cli", type=options.str2bool, default=True)
    ap.add_argument("--n_rounds", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ab_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    i32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    say("ab_bench: %s, random bytes; %d warm-up + %d timed calls (HIP events), all values then the median"
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
        ws = torch.empty(ops.boost_stump_ws_bytes(K, D), device=dev, dtype=torch.uint8)
        unit = torch.full((K, N), classify.BOOST_W1, device=dev, dtype=torch.int32)
        rand = torch.randint(0, classify.BOOST_W1 + 1, (K, N), device=dev, generator=g).to(torch.int32)
        rand = rand * (torch.rand((K, N), device=dev, generator=g) < 0.8).to(torch.int32)
        for name, W in (("unit weights", unit), ("random weights, a fifth of the rows at 0", rand)):
            out = ops.boost_stump_u8(X, y, K, W, ws=ws)
            t = event_times(lambda i: ops.boost_stump_u8(X, y, K, W, out=out, ws=ws), a.warmup, a.reps)
            med = float(np.median(t))
            say("    cslgan_boost_stump_u8, %s (%d row visits x %d bytes): %s us, median %.1f us = %.2fx the copy, %.2f TB/s of bytes"
                % (name, N * K, D, " / ".join("%.1f" % v for v in t), med, med / t_copy, N * K * D / med / 1e6))
        del ws, unit, rand
        rows, off, cls = i32(np.tile(np.arange(N), K)), i32(np.arange(K + 1) * N), i32(np.arange(K))
        tws = torch.empty(ops.tree_best_split_ws_bytes(K, D), device=dev, dtype=torch.uint8)
        out = ops.tree_best_split_u8(X, y, K, rows, off, cls, ws=tws)
        t = event_times(lambda i: ops.tree_best_split_u8(X, y, K, rows, off, cls, out=out, ws=tws), a.warmup, a.reps)
        med = float(np.median(t))
        say("    cslgan_tree_best_split_u8, root: %d segments of %d rows: %s us, median %.1f us = %.2fx the copy"
            % (K, N, " / ".join("%.1f" % v for v in t), med, med / t_copy))
        del X, tws, out
        torch.cuda.empty_cache()

    if a.cli:
        tmp = tempfile.mkdtemp(prefix="ab_bench_")
        (x, yy), (xt, yt) = blobs(10000, 10, 1), blobs(2000, 10, 2)
        syn, test = write_cache(os.path.join(tmp, "syn"), x, yy), write_cache(os.path.join(tmp, "test"), xt, yt)
        say("(2) ten-class blobs, 10000 synthetic and 2000 test images of 28 x 28 x 1 (784 bytes), 10 % of the labels redrawn")
        flags = ["--classifier", "ab", "--n_rounds", str(a.n_rounds)]
        for _ in range(2):
            t0 = time.perf_counter()
            res = tstr.main(["--syn_cache", syn, "--test_cache", test, "-d", "cuda:0", "--values_dir", os.path.join(tmp, "vals")] + flags)["syn"]
            torch.cuda.synchronize()
            say("    tstr.main %s -d cuda:0: %.2f s (host clock); rounds per class %s; AUROC %.4f, accuracy %d / %d"
                % (" ".join(flags), time.perf_counter() - t0, res["fit"]["rounds"], res["auroc_micro"], res["accuracy_hits"], res["n_test"]))
        try:
            from sklearn.ensemble import AdaBoostClassifier
        except ImportError:
            say("    scikit-learn is not importable here: no host reference time")
        else:
            xs, xts = x.reshape(len(x), -1) / 255.0, xt.reshape(len(xt), -1) / 255.0
            P = np.zeros((len(xts), 10))
            t0 = time.perf_counter()
            for k in range(10):
                est = AdaBoostClassifier(n_estimators=a.n_rounds, random_state=0).fit(xs, (yy == k).astype(np.int64))
                P[:, k] = est.predict_proba(xts)[:, 1]
                print("    ... class %d after %.1f s" % (k, time.perf_counter() - t0), flush=True)
            dt = time.perf_counter() - t0
            acc = classify.accuracy(P, yt)
            say("    scikit-learn AdaBoostClassifier(n_estimators=%d) per class, one thread, fit + predict_proba: %.2f s; AUROC %.4f, accuracy %d / %d; "
                "max |P - P_tstr| = %.3g" % (a.n_rounds, dt, classify.auroc(P, yt)["micro"], acc["hits"], acc["n"], float(np.abs(P - np.load(os.path.join(tmp, "vals", "syn_P.npy"))).max())))
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
