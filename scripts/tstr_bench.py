"""What `python -m csl_gan_amd.tstr` costs on one MI355X, in ONE process:

  (1) one cslgan_ovr_logreg_eval_u8 call (forward, gradient and reduce kernels, launch gaps included) at 10000 x 12288 bytes, K = 2
      and K = 10, on one X (123 MB: its second read comes from the Infinity Cache) and rotating over enough copies that every
      read comes from HBM; and at 162770 x 12288, K = 2 (2 GB: always HBM).  HIP events around each call, warm-up calls thrown
      away, every repetition printed, the median quoted.  Beside each: the time to read X twice at the 6.29 TB/s the project has
      measured, and the time of 2 x 2 N D 16 FLOP at the 155 TF of the fp32 matrix instruction, and which of the two is larger;
  (2) tstr.main end to end on caches of random bytes of CelebA's sizes (162770 train, 19962 test, 10000 synthetic images of
      64 x 64 x 3) with random labels, K = 2, --baseline included (host clock);
  (3) the float64 host path on the 10000-row fit (--host_max_iter bounds it; the time per evaluation is what scales);
  (4) scikit-learn's LogisticRegression on the same rows, if it imports.

    python scripts/tstr_bench.py [--reps 7] [--warmup 3] [--cli_max_iter N] [--host_max_iter N] [--out FILE]
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

HBM_BYTES_PER_S = 6.29e12
MFMA_F32_FLOPS = 155e12
D = 12288


def event_times(fn, warmup, reps):
    out = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)          # us
    return out


def write_cache(path, n, K, seed):
    rng = np.random.default_rng(seed)
    u8p, labp, hdrp = pipeline.cache_paths(path)
    mm = np.lib.format.open_memmap(u8p, mode="w+", dtype=np.uint8, shape=(n, 64, 64, 3))
    for s in range(0, n, 16384):
        k = min(16384, n - s)
        mm[s:s + k] = rng.integers(0, 256, (k, 64, 64, 3), dtype=np.uint8)
    mm.flush()
    del mm
    np.save(labp, (np.arange(n) % K).astype(np.int64) if seed == 0 else rng.integers(0, K, n).astype(np.int64))
    with open(hdrp, "w") as f:
        json.dump({"version": pipeline.CACHE_VERSION, "n": n, "H": 64, "W": 64, "C": 3, "signed": False, "dtype": "uint8", "layout": "NHWC"}, f)
    return path


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cli", type=options.str2bool, default=True)
    ap.add_argument("--host", type=options.str2bool, default=True)
    ap.add_argument("--cli_max_iter", type=int, default=2000, help="--max_iter of the tstr.main runs")
    ap.add_argument("--host_max_iter", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tstr_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    say("tstr_bench: %s, rows of %d bytes, random bytes; %d warm-up + %d timed calls (HIP events), all values then the median"
        % (torch.cuda.get_device_name(0), D, a.warmup, a.reps))

    def bounds(N):
        t_mem, t_mma = 2.0 * N * D / HBM_BYTES_PER_S * 1e6, 2 * 2.0 * N * D * 16 / MFMA_F32_FLOPS * 1e6
        return "X twice at 6.29 TB/s: %.1f us; 2 x 2 N D 16 FLOP at 155 TF: %.1f us; the larger bound: %s" % (
            t_mem, t_mma, "memory" if t_mem >= t_mma else "matrix instruction"), max(t_mem, t_mma)

    def one_eval(N, K, rotate):
        copies = max(2, int(2 * 256e6 / (N * D)) + 1) if rotate else 1                 # twice the Infinity Cache
        Xs = [torch.randint(0, 256, (N, D), device=dev, dtype=torch.uint8, generator=g) for _ in range(copies)]
        y = torch.randint(0, K, (N,), device=dev, generator=g).to(torch.int32)
        U = (torch.randn(D + 1, K, device=dev, generator=g) * 0.002)
        ws = torch.empty(ops.ovr_logreg_u8_ws_floats(N, D), device=dev, dtype=torch.float32)
        loss, grad = ops.ovr_logreg_eval_u8(Xs[0], y, U, ws=ws)
        t = event_times(lambda i: ops.ovr_logreg_eval_u8(Xs[i % copies], y, U, out_loss=loss, out_grad=grad, ws=ws), a.warmup, a.reps)
        text, bound = bounds(N)
        say("(1) cslgan_ovr_logreg_eval_u8, %d x %d, K = %d, %s (workspace %.1f MB): %s us, median %.1f us = %.2fx the larger bound"
            % (N, D, K, "%d copies of X in turn" % copies if rotate else "one X", ws.numel() * 4 / 1e6, " / ".join("%.1f" % v for v in t),
               np.median(t), np.median(t) / bound))
        say("    " + text)

    for K in (2, 10):
        for rotate in (False, True):
            one_eval(10000, K, rotate)
    one_eval(162770, 2, False)
    torch.cuda.empty_cache()

    tmp = tempfile.mkdtemp(prefix="tstr_bench_")
    t0 = time.perf_counter()
    syn, test = write_cache(os.path.join(tmp, "syn"), 10000, 2, 0), write_cache(os.path.join(tmp, "test"), 19962, 2, 2)
    if a.cli:
        train = write_cache(os.path.join(tmp, "train"), 162770, 2, 1)
        say("(2) caches of random bytes written in %.1f s: 162770 train, 19962 test, 10000 synthetic images of %d bytes, random labels, K = 2"
            % (time.perf_counter() - t0, D))
        for _ in range(2):
            t0 = time.perf_counter()
            res = tstr.main(["--syn_cache", syn, "--test_cache", test, "--train_cache", train, "--baseline", "-d", "cuda:0", "--max_iter",
                            str(a.cli_max_iter)])
            torch.cuda.synchronize()
            say("    tstr.main --baseline -d cuda:0 --max_iter %d: %.2f s (host clock)" % (a.cli_max_iter, time.perf_counter() - t0))
        for lab, m in res.items():
            s = m["solver"]
            say("    %s: %d rows, iterations %s, evaluations %s, stalled %s, converged %s; AUROC %.4f, accuracy %d / %d"
                % (lab, m["n_train"], s["iterations"], s["evaluations"], s["stalled"], s["converged"], m["auroc_micro"], m["accuracy_hits"], m["n_test"]))
    if a.host:
        c = pipeline.CachedImages(syn)
        x, y = tstr.cache_rows(c)
        clf = classify.OvrLogReg(2, max_iter=a.host_max_iter)
        t0 = time.perf_counter()
        rep = clf.fit_bytes(x, y)
        t = time.perf_counter() - t0
        say("(3) float64 host path, fit_bytes on 10000 x %d, %d threads, max_iter %d: %.1f s, iterations %s, evaluations %s = %.3f s per evaluation"
            % (D, torch.get_num_threads(), a.host_max_iter, t, rep["iterations"], rep["evaluations"], t / max(rep["evaluations"])))
        try:
            from sklearn.linear_model import LogisticRegression
        except ImportError:
            LogisticRegression = None
        if LogisticRegression is not None:
            t0 = time.perf_counter()
            est = LogisticRegression(C=2.0, solver="lbfgs", max_iter=a.host_max_iter).fit(x.astype(np.float64) / 255.0, y)
            say("(4) scikit-learn LogisticRegression(C=2, lbfgs, max_iter %d) on the same rows: %.1f s, %s iterations"
                % (a.host_max_iter, time.perf_counter() - t0, est.n_iter_.tolist()))
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
