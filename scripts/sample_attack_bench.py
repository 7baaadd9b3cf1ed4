"""What the counting kernel of `python -m csl_gan_amd.sample_attack` costs beside the search kernel it shares its tile loop with, and
what the command costs end to end, on one MI355X.  Random bytes stand in for the images (the arithmetic does not depend on the
values; no dataset is needed).  In ONE process:

  (1) cslgan_nn_min_i8, --nq queries against one prepared block of --block_rows images of --d bytes: HIP events around each call —
      the yardstick (profiles/nearest_bench.txt (2)), measured again here;
  (2) cslgan_nn_count_i8 on the same operands with J = 1 and with J = 4 thresholds (the median of a sample of the d2 matrix and
      values around it, so that the compares go both ways): HIP events around each call, and the count / min ratio of the medians;
  (3) `sample_attack.main` end to end (host clock, in this process: cache opening, both d2min queries, both counting walks, the
      rank metrics and the JSON) on caches of random bytes of CelebA's sizes, written to a temporary directory first.

Each kernel timing: --warmup calls that are thrown away, then --reps calls; all values are printed and the median is the figure.

    python scripts/sample_attack_bench.py [--nq 10000] [--block_rows 16384] [--d 12288] [--n_train 162770] [--n_heldout 19962]
                                          [--n_syn 10000] [--reps 5] [--out FILE]
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
from csl_gan_amd import ops, sample_attack  # noqa: E402
from csl_gan_amd.generate import CacheWriter  # noqa: E402
from nearest_bench import event_times, fmt  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--block_rows", type=int, default=16384)
    ap.add_argument("--d", type=int, default=12288, help="bytes per image; written as a [d / 3, 1, 3] image")
    ap.add_argument("--n_train", type=int, default=162770)
    ap.add_argument("--n_heldout", type=int, default=19962)
    ap.add_argument("--n_syn", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli_runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sample_attack_bench.py measures on an MI355X; no device is visible")
    if a.d % 3:
        raise SystemExit("--d must be a multiple of 3")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    shape = (a.d // 3, 1, 3)
    rand = lambda n: torch.randint(0, 256, (n,) + shape, device=dev, dtype=torch.uint8, generator=g)
    Dp = ops.nn_padded_dim(a.d)
    nq, nb = a.nq, a.block_rows
    say("sample_attack_bench: %s, %d queries x %d reference images x %d bytes (Dp = %d), random bytes; %d warm-up + %d timed calls, all values "
        "then the median" % (torch.cuda.get_device_name(0), nq, nb, a.d, Dp, a.warmup, a.reps))

    # ---- (1) the search kernel, (2) the counting kernel on the same operands -----------------------------------------------------------
    Qd, Rd = rand(nq), rand(nb)
    q, qn = ops.nn_prepare(Qd)
    r, rn = ops.nn_prepare(Rd)
    ns = min(256, nq, nb)                                  # the thresholds: from the exact d2 of a 256 x 256 corner
    qa, ra = Qd[:ns].reshape(ns, -1).cpu().double(), Rd[:ns].reshape(ns, -1).cpu().double()
    d2 = ((qa * qa).sum(1)[:, None] + (ra * ra).sum(1)[None, :] - 2.0 * (qa @ ra.T)).round().long().reshape(-1).sort().values
    med = int(d2[len(d2) // 2])
    thr4 = [med, int(d2[len(d2) // 10]), int(d2[len(d2) // 100]), int(d2[(9 * len(d2)) // 10])]
    del Qd, Rd, qa, ra
    best = torch.full((nq,), -1, device=dev, dtype=torch.int64)
    t_min = event_times(lambda: ops.nn_min(q, qn, r, rn, 0, best), a.warmup, a.reps)
    work = 2.0 * nq * nb * Dp
    say("(1) cslgan_nn_min_i8, %d x %d x %d: %s ms, median %.2f ms; %.3g int8 ops = %.0f TOP/s achieved"
        % (nq, nb, Dp, fmt(t_min), 1e3 * np.median(t_min), work, work / np.median(t_min) / 1e12))
    for J, thr in ((1, thr4[:1]), (4, thr4)):
        counts = torch.zeros((nq, J), device=dev, dtype=torch.int32)
        t = event_times(lambda: ops.nn_count(q, qn, r, rn, thr, counts), a.warmup, a.reps)      # (warmup + reps) * nb stays far below 2^31
        calls = a.warmup + a.reps
        say("(2) cslgan_nn_count_i8, J = %d, thresholds %s: %s ms, median %.2f ms = %.0f TOP/s; count / min = %.3f; share of pairs counted per "
            "threshold: %s" % (J, thr, fmt(t), 1e3 * np.median(t), work / np.median(t) / 1e12, np.median(t) / np.median(t_min),
                               " / ".join("%.3f" % (float(c) / calls / nb / nq) for c in counts.sum(0, dtype=torch.int64).tolist())))
    t_min2 = event_times(lambda: ops.nn_min(q, qn, r, rn, 0, best), 1, a.reps)
    say("    cslgan_nn_min_i8 again, after the counts: %s ms, median %.2f ms" % (fmt(t_min2), 1e3 * np.median(t_min2)))
    del q, qn, r, rn, best, counts
    torch.cuda.empty_cache()

    # ---- (3) the command end to end ---------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="sample_attack_bench_")
    try:
        t0 = time.perf_counter()
        for name, n in (("train", a.n_train), ("heldout", a.n_heldout), ("syn", a.n_syn)):
            w = CacheWriter(os.path.join(tmp, name), n, shape[0], shape[1], shape[2], True, {"note": "random bytes"})
            for s in range(0, n, 16384):
                k = min(16384, n - s)
                w(s, rand(k).cpu().numpy(), np.zeros(k, dtype=np.int64))
            w.close()
        say("(3) caches of random bytes written in %.1f s: %d train, %d held-out, %d synthetic images of %d bytes"
            % (time.perf_counter() - t0, a.n_train, a.n_heldout, a.n_syn, a.d))
        argv3 = ["--syn_cache", os.path.join(tmp, "syn"), "--train_cache", os.path.join(tmp, "train"), "--nontrain_cache", os.path.join(tmp, "heldout"),
                 "-d", "cuda:0", "--block_rows", str(a.block_rows)]
        ts = []
        for _ in range(a.cli_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with open(os.devnull, "w") as null:
                old, sys.stdout = sys.stdout, null
                try:
                    stats = sample_attack.main(argv3)
                finally:
                    sys.stdout = old
            ts.append(time.perf_counter() - t0)
        m = stats["syn"]
        say("    sample_attack.main %s (4 percentiles, pool 1000, 10000 ASR trials): %s s (first run first; host clock)"
            % (" ".join(argv3[6:]), fmt(ts, 1.0)))
        say("    eps^2 = %s; fbb AUC %.4f, ASR %.4f (+- %.4f); mc_p50 AUC %.4f" % (m["eps2"], m["fbb"]["auc"], m["fbb"]["asr"], m["fbb"]["asr_stderr"],
                                                                                    m["mc_p50"]["auc"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
