"""What `python -m csl_gan_amd.tstr --classifier mlp` costs on one MI355X, in ONE process:

  (1) one cslgan_ovr_mlp_eval_u8 call (forward, gradient and reduce kernels, launch gaps included) at 10000 x 12288 bytes with
      K = 2, H = 100 and at 60000 x 784 with K = 10, H = 100.  HIP events around each call, warm-up calls thrown away, every
      repetition printed, the median quoted.  Beside each: the time of 2 x 2 N D C FLOP (C = H K) at the 155 TF of the fp32 matrix
      instruction, and the time to move the bytes the evaluation cannot avoid (X twice, A and dZ1 written once and read once each,
      W1 read and its gradient written) at the 6.29 TB/s the project has measured, and which of the two is larger;
  (2) tstr.main --classifier mlp end to end on caches of random bytes (64 x 64 x 3 images, random labels, K = 2), --baseline
      included (host clock);
  (3) scikit-learn's OneVsRestClassifier(MLPClassifier(solver="lbfgs", alpha=1)) on the synthetic cache's rows on the host, if it
      imports, with the same iteration bound — context, not a competitor: another initial point, another line search.

    python scripts/mlp_bench.py [--reps 7] [--warmup 3] [--rows 10000] [--max_iter 20] [--out profiles/mlp_bench.txt]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import ops, options, pipeline, tstr  # noqa: E402
from tstr_bench import HBM_BYTES_PER_S, MFMA_F32_FLOPS, event_times, write_cache  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cli", type=options.str2bool, default=True)
    ap.add_argument("--host", type=options.str2bool, default=True)
    ap.add_argument("--rows", type=int, default=10000, help="rows of the training and synthetic caches of (2); the test cache has a fifth")
    ap.add_argument("--max_iter", type=int, default=20, help="--max_iter of the tstr.main runs and of scikit-learn")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mlp_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    say("mlp_bench: %s, random bytes; %d warm-up + %d timed calls (HIP events), all values then the median"
        % (torch.cuda.get_device_name(0), a.warmup, a.reps))

    def one_eval(N, D, K, H):
        C = H * K
        X = torch.randint(0, 256, (N, D), device=dev, dtype=torch.uint8, generator=g)
        y = torch.randint(0, K, (N,), device=dev, generator=g).to(torch.int32)
        U = torch.randn((D + 2) * H + 1, K, device=dev, generator=g) * (1.0 / np.sqrt(D))
        ws = torch.empty(ops.ovr_mlp_u8_ws_floats(N, D, K, H), device=dev, dtype=torch.float32)
        loss, grad = ops.ovr_mlp_eval_u8(X, y, U, H, 1.0, ws=ws)
        t = event_times(lambda i: ops.ovr_mlp_eval_u8(X, y, U, H, 1.0, out_loss=loss, out_grad=grad, ws=ws), a.warmup, a.reps)
        t_mma = 2 * 2.0 * N * D * C / MFMA_F32_FLOPS * 1e6
        t_mem = (2.0 * N * D + 16.0 * N * C + 8.0 * D * C) / HBM_BYTES_PER_S * 1e6
        say("(1) cslgan_ovr_mlp_eval_u8, %d x %d, K = %d, H = %d (C = %d, workspace %.1f MB): %s us, median %.1f us = %.2fx the larger bound"
            % (N, D, K, H, C, ws.numel() * 4 / 1e6, " / ".join("%.1f" % v for v in t), np.median(t), np.median(t) / max(t_mma, t_mem)))
        say("    2 x 2 N D C FLOP at 155 TF: %.1f us (the median is %.1f TFLOP/s); 2 N D + 16 N C + 8 D C bytes at 6.29 TB/s: %.1f us; "
            "the larger bound: %s" % (t_mma, 4.0 * N * D * C / np.median(t) / 1e6, t_mem, "matrix instruction" if t_mma >= t_mem else "memory"))

    one_eval(10000, 12288, 2, 100)
    one_eval(60000, 784, 10, 100)
    torch.cuda.empty_cache()

    tmp = tempfile.mkdtemp(prefix="mlp_bench_")
    t0 = time.perf_counter()
    syn = write_cache(os.path.join(tmp, "syn"), a.rows, 2, 0)
    test = write_cache(os.path.join(tmp, "test"), max(a.rows // 5, 2), 2, 2)
    if a.cli:
        train = write_cache(os.path.join(tmp, "train"), a.rows, 2, 1)
        say("(2) caches of random bytes written in %.1f s: %d train, %d test, %d synthetic images of 12288 bytes, random labels, K = 2"
            % (time.perf_counter() - t0, a.rows, max(a.rows // 5, 2), a.rows))
        for _ in range(2):
            t0 = time.perf_counter()
            res = tstr.main(["--syn_cache", syn, "--test_cache", test, "--train_cache", train, "--baseline", "-d", "cuda:0", "--classifier", "mlp",
                             "--max_iter", str(a.max_iter)])
            torch.cuda.synchronize()
            say("    tstr.main --classifier mlp --baseline -d cuda:0 --max_iter %d: %.2f s (host clock)" % (a.max_iter, time.perf_counter() - t0))
        for lab, m in res.items():
            s = m["solver"]
            say("    %s: %d rows, hidden %d, iterations %s, evaluations %s, stalled %s; AUROC %.4f, accuracy %d / %d"
                % (lab, m["n_train"], m["hidden"], s["iterations"], s["evaluations"], s["stalled"], m["auroc_micro"], m["accuracy_hits"], m["n_test"]))
    if a.host:
        try:
            from sklearn.multiclass import OneVsRestClassifier
            from sklearn.neural_network import MLPClassifier
        except ImportError:
            OneVsRestClassifier = None
        if OneVsRestClassifier is None:
            say("(3) scikit-learn does not import: not measured")
        else:
            import warnings
            x, y = tstr.cache_rows(pipeline.CachedImages(syn))
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                            # the iteration bound is the point
                est = OneVsRestClassifier(MLPClassifier(hidden_layer_sizes=(100,), solver="lbfgs", alpha=1, max_iter=a.max_iter, random_state=0))
                est.fit(x.astype(np.float64) / 255.0, y)
            say("(3) scikit-learn OneVsRestClassifier(MLPClassifier(100, lbfgs, alpha=1, max_iter %d)) on the %d synthetic rows, host: %.1f s, "
                "%s iterations" % (a.max_iter, len(y), time.perf_counter() - t0, [int(e.n_iter_) for e in est.estimators_]))
    shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
