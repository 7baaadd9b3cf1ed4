"""What `python -m csl_gan_amd.tstr --classifier gnb / bnb` costs on one MI355X, in ONE process:

  (1) cslgan_class_moments_u8, cslgan_nb_score_gauss_u8 and cslgan_nb_score_bern_u8, one call each, at 10000 x 12288 bytes (K = 2),
      162770 x 12288 (K = 2) and 60000 x 784 (K = 10), random bytes and labels.  HIP events around each call, warm-up calls thrown
      away, every repetition printed, the median quoted.  The yardstick: a device-to-device copy of the same bytes timed the same
      way in the same process (it reads AND writes them, so a kernel that only reads could take half of it), and the time to read
      the bytes once at the 6.29 TB/s the project has measured for HBM.  The 123 MB and 47 MB matrices fit the 256 MB Infinity
      Cache: their repeated reads are not HBM reads, for the kernels and for the copy alike; the 2 GB one is always HBM;
  (2) tstr.main --classifier gnb --baseline end to end on caches of random bytes of CelebA's sizes (162770 train, 19962 test, 10000
      synthetic images of 64 x 64 x 3), random labels, K = 2 (host clock, cache reading and the copies to the device included).

    python scripts/nb_bench.py [--reps 7] [--warmup 3] [--cli true] [--out FILE]
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
from csl_gan_amd import ops, options, tstr  # noqa: E402
from tstr_bench import HBM_BYTES_PER_S, event_times, write_cache  # noqa: E402

SHAPES = [(10000, 12288, 2), (162770, 12288, 2), (60000, 784, 10)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cli", type=options.str2bool, default=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("nb_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    say("nb_bench: %s, random bytes; %d warm-up + %d timed calls (HIP events), all values then the median"
        % (torch.cuda.get_device_name(0), a.warmup, a.reps))
    for N, D, K in SHAPES:
        X = torch.randint(0, 256, (N, D), device=dev, dtype=torch.uint8, generator=g)
        y = torch.randint(0, K, (N,), device=dev, generator=g).to(torch.int32)
        m = torch.rand((K, D), device=dev, generator=g) * 255
        w = torch.exp(torch.rand((K, D), device=dev, generator=g) * 9.2 - 11.5)           # 1e-5 .. 1e-1
        delta = torch.randn((K, D), device=dev, generator=g) * 3
        Y = torch.empty_like(X)
        mom = ops.class_moments_u8(X, y, K)
        S = ops.nb_score_gauss_u8(X, m, w)
        t_read = N * D / HBM_BYTES_PER_S * 1e6
        t_copy = float(np.median(event_times(lambda i: Y.copy_(X), a.warmup, a.reps)))
        say("(1) %d x %d, K = %d (%.0f MB): device-to-device copy median %.1f us (%.2f TB/s read + written); one read at 6.29 TB/s: %.1f us"
            % (N, D, K, N * D / 1e6, t_copy, 2 * N * D / t_copy / 1e6, t_read))
        for name, fn in (("cslgan_class_moments_u8", lambda i: ops.class_moments_u8(X, y, K, 0, out=mom)),
                         ("cslgan_nb_score_gauss_u8", lambda i: ops.nb_score_gauss_u8(X, m, w, out=S)),
                         ("cslgan_nb_score_bern_u8", lambda i: ops.nb_score_bern_u8(X, delta, 127, out=S))):
            t = event_times(fn, a.warmup, a.reps)
            med = float(np.median(t))
            say("    %s: %s us, median %.1f us = %.2fx the copy, %.2fx one read at 6.29 TB/s (%.2f TB/s of bytes)"
                % (name, " / ".join("%.1f" % v for v in t), med, med / t_copy, med / t_read, N * D / med / 1e6))
        del X, Y, mom, S
        torch.cuda.empty_cache()

    if a.cli:
        tmp = tempfile.mkdtemp(prefix="nb_bench_")
        t0 = time.perf_counter()
        syn, test = write_cache(os.path.join(tmp, "syn"), 10000, 2, 0), write_cache(os.path.join(tmp, "test"), 19962, 2, 2)
        train = write_cache(os.path.join(tmp, "train"), 162770, 2, 1)
        say("(2) caches of random bytes written in %.1f s: 162770 train, 19962 test, 10000 synthetic images of 12288 bytes, random labels, K = 2"
            % (time.perf_counter() - t0))
        for kind in ("gnb", "gnb", "bnb"):
            t0 = time.perf_counter()
            res = tstr.main(["--syn_cache", syn, "--test_cache", test, "--train_cache", train, "--baseline", "-d", "cuda:0", "--classifier", kind])
            torch.cuda.synchronize()
            say("    tstr.main --classifier %s --baseline -d cuda:0: %.2f s (host clock)" % (kind, time.perf_counter() - t0))
        for lab, r in res.items():
            say("    %s: %d rows, rows per class %s; AUROC %.4f, accuracy %d / %d" % (lab, r["n_train"], r["fit"]["n_per_class"], r["auroc_micro"],
                                                                                     r["accuracy_hits"], r["n_test"]))
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
