"""What `python -m csl_gan_amd.tstr_svm` costs on one MI355X, in ONE process:

  (1) cslgan_gram_d2_u8, the stored matrix of squared distances, at 10000 x 784 and 10000 x 12288 random bytes, beside cslgan_nn_min_i8 on
      the same prepared operands against themselves (the same tile loop with the epilogue that keeps a minimum instead of storing).  HIP
      events around each call, warm-up calls thrown away, every repetition printed, the median quoted;
  (2) cslgan_svc_smo_f64 on the matrices of (1): iterations per second and per problem, 12 problems (K = 2, five folds) and 96 (K = 16) of
      random labels in one launch of --chunk iterations each (random labels keep every problem far from its end), HIP events around a
      launch;
  (3) tstr_svm.main end to end (host clock, cache reading and the copies included) on caches of a ten-class blob problem, --rows synthetic
      and 2000 test images of 28 x 28 x 1, beside scikit-learn's SVC(kernel='linear', probability=True) per class (what
      OneVsRestClassifier fits, one class after the other, one thread) on the same bytes / 255 on the host when scikit-learn is importable
      and --sklearn is true.

    python scripts/svm_bench.py [--reps 5] [--warmup 2] [--chunk 512] [--cli true] [--rows 2000 10000] [--sklearn true] [--out FILE]
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
from csl_gan_amd import classify, ops, options, svm, tstr_svm  # noqa: E402
from tree_bench import blobs, write_cache  # noqa: E402
from tstr_bench import event_times  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--cli", type=options.str2bool, default=True)
    ap.add_argument("--rows", type=int, nargs="+", default=[2000, 10000])
    ap.add_argument("--sklearn", type=options.str2bool, default=True)
    ap.add_argument("--sklearn_rows", type=int, default=2000, help="scikit-learn is timed on sets of at most this many rows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("svm_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    say("svm_bench: %s, random bytes; %d warm-up + %d timed calls (HIP events), all values then the median"
        % (torch.cuda.get_device_name(0), a.warmup, a.reps))
    n = 10000
    for D in (784, 12288):
        X = torch.randint(0, 256, (n, D), device=dev, dtype=torch.uint8, generator=g)
        xs, sq = ops.nn_prepare(X)
        d2 = ops.gram_d2(xs, sq)
        t = event_times(lambda i: ops.gram_d2(xs, sq, out=d2), a.warmup, a.reps)
        med = float(np.median(t))
        macs = n * n * xs.shape[1]
        say("(1) %d x %d (Dp = %d): cslgan_gram_d2_u8 %s us, median %.1f us = %.0f int8 TOP/s, %.0f MB stored at %.2f TB/s"
            % (n, D, xs.shape[1], " / ".join("%.1f" % v for v in t), med, 2 * macs / med / 1e6, d2.numel() * 4 / 1e6, d2.numel() * 4 / med / 1e6))
        best = torch.full((n,), -1, dtype=torch.int64, device=dev)
        t = event_times(lambda i: ops.nn_min(xs, sq, xs, sq, 0, best), a.warmup, a.reps)
        say("    cslgan_nn_min_i8 on the same operands: %s us, median %.1f us; the store costs %.2fx"
            % (" / ".join("%.1f" % v for v in t), float(np.median(t)), med / float(np.median(t))))
        s = svm._byte_sqnorms_device(X)
        del xs, best
        for P in (12, 96):
            Y = (torch.randint(0, 2, (P, n), device=dev, generator=g) * 2 - 1).to(torch.int8)
            act = torch.ones((P, n), dtype=torch.uint8, device=dev)
            alpha = torch.zeros((P, n), dtype=torch.float64, device=dev)
            grad = torch.full((P, n), -1.0, dtype=torch.float64, device=dev)
            iters, done = torch.zeros(P, dtype=torch.int64, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
            t = event_times(lambda i: ops.svc_smo(d2, s, Y, act, 1.0, 1e-3, a.chunk, 10 ** 9, alpha, grad, iters, done), a.warmup, a.reps)
            med = float(np.median(t))
            ran = int(iters.min()), int(iters.max())
            say("(2) %d x %d, %d problems, launches of %d iterations: %s us, median %.1f us = %.1f us per iteration, %.0f iterations / s per problem, "
                "%.0f / s over all; iterations run %d .. %d, done %d"
                % (n, D, P, a.chunk, " / ".join("%.1f" % v for v in t), med, med / a.chunk, a.chunk / med * 1e6, P * a.chunk / med * 1e6, ran[0], ran[1],
                   int(done.sum())))
        del X, d2, s
        torch.cuda.empty_cache()

    if a.cli:
        tmp = tempfile.mkdtemp(prefix="svm_bench_")
        xt, yt = blobs(2000, 10, 2)
        test = write_cache(os.path.join(tmp, "test"), xt, yt)
        for rows in a.rows:
            x, yy = blobs(rows, 10, 1)
            syn = write_cache(os.path.join(tmp, "syn%d" % rows), x, yy)
            say("(3) ten-class blobs, %d synthetic and 2000 test images of 28 x 28 x 1 (784 bytes), 10 %% of the labels redrawn" % rows)
            for _ in range(2):
                t0 = time.perf_counter()
                res = tstr_svm.main(["--syn_cache", syn, "--test_cache", test, "-d", "cuda:0", "--values_dir", os.path.join(tmp, "vals")])["syn%d" % rows]
                torch.cuda.synchronize()
                f = res["fit"]
                say("    tstr_svm.main -d cuda:0: %.2f s (host clock); iterations per class %s, all 60 problems %d; support vectors %s; AUROC %.4f, "
                    "accuracy %d / %d" % (time.perf_counter() - t0, f["iterations"], f["iterations_total"], f["n_sv"], res["auroc_micro"],
                                          res["accuracy_hits"], res["n_test"]))
            if not a.sklearn or rows > a.sklearn_rows:
                continue
            try:
                from sklearn.svm import SVC
            except ImportError:
                say("    scikit-learn is not importable here: no host reference time")
                continue
            xs_, xts = x.reshape(len(x), -1) / 255.0, xt.reshape(len(xt), -1) / 255.0
            Pm = np.zeros((len(xts), 10))
            t0 = time.perf_counter()
            for k in range(10):
                est = SVC(kernel="linear", probability=True, random_state=0).fit(xs_, (yy == k).astype(np.int64))
                Pm[:, k] = est.predict_proba(xts)[:, 1]
                print("    ... class %d after %.1f s" % (k, time.perf_counter() - t0), flush=True)
            dt = time.perf_counter() - t0
            Pm /= Pm.sum(1, keepdims=True)
            acc = classify.accuracy(Pm, yt)
            say("    scikit-learn SVC(kernel='linear', probability=True) per class, one thread, fit + predict_proba: %.2f s; AUROC %.4f, accuracy %d / %d; "
                "max |P - P_tstr_svm| = %.3g (other folds, shrinking, float32 kernel rows)"
                % (dt, classify.auroc(Pm, yt)["micro"], acc["hits"], acc["n"],
                   float(np.abs(Pm - np.load(os.path.join(tmp, "vals", "syn%d_P.npy" % rows))).max())))
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
