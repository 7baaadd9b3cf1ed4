"""What the k-smallest-keys kernel and the per-column-radius count of `python -m csl_gan_amd.prdc` cost beside the search kernel they
share their tile loop with, and what the command costs end to end, on one MI355X.  Random bytes stand in for the images (no
dataset is needed; on random order the insert path of the k-list is rare, which is what the design relies on).  In ONE process:

  (1) cslgan_nn_min_i8, --nq queries against one prepared block of --block_rows images of --d bytes: HIP events around each call —
      the yardstick (profiles/nearest_bench.txt (2)), measured again here and once more at the end;
  (2) cslgan_nn_kth_i8 (search + merge kernel) on the same operands at k = 1, 5, 8, `best` refilled with all-ones before every
      call outside the timed region, so every call starts without a bound; and at k = 5 with the `best` that a first block left,
      which is what every later block of a walk meets;
  (3) cslgan_nn_count_radius_i8 on the same operands, radii around the median of a sample of the d2 matrix;
  (4) `prdc.main` end to end (host clock, in this process) on caches of random bytes of CelebA's sizes, with --baseline.

Each kernel timing: --warmup calls that are thrown away, then --reps calls; all values are printed and the median is the figure.

    python scripts/prdc_bench.py [--nq 10000] [--block_rows 16384] [--d 12288] [--n_train 162770] [--n_heldout 19962]
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
from csl_gan_amd import ops, prdc  # noqa: E402
from csl_gan_amd.generate import CacheWriter  # noqa: E402
from nearest_bench import event_times, fmt  # noqa: E402


def event_times_with_setup(setup, fn, warmup, reps):
    """event_times with `setup()` ahead of every call, outside the events."""
    out = []
    for i in range(warmup + reps):
        setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) * 1e-3)
    return out


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
        raise SystemExit("prdc_bench.py measures on an MI355X; no device is visible")
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
    say("prdc_bench: %s, %d queries x %d reference images x %d bytes (Dp = %d), random bytes; %d warm-up + %d timed calls, all values then "
        "the median" % (torch.cuda.get_device_name(0), nq, nb, a.d, Dp, a.warmup, a.reps))

    # ---- (1) the search kernel, (2) the k-list kernel and (3) the radius count on the same operands ---------------------------------------
    Qd, Rd = rand(nq), rand(nb)
    q, qn = ops.nn_prepare(Qd)
    r, rn = ops.nn_prepare(Rd)
    ns = min(256, nq, nb)                                  # the radii: around the median of the exact d2 of a 256 x 256 corner
    qa, ra = Qd[:ns].reshape(ns, -1).cpu().double(), Rd[:ns].reshape(ns, -1).cpu().double()
    d2 = ((qa * qa).sum(1)[:, None] + (ra * ra).sum(1)[None, :] - 2.0 * (qa @ ra.T)).round().long().reshape(-1).sort().values
    lo, hi = int(d2[len(d2) // 4]), int(d2[(3 * len(d2)) // 4])
    del Qd, Rd, qa, ra
    best1 = torch.full((nq,), -1, device=dev, dtype=torch.int64)
    t_min = event_times(lambda: ops.nn_min(q, qn, r, rn, 0, best1), a.warmup, a.reps)
    work = 2.0 * nq * nb * Dp
    med_min = np.median(t_min)
    say("(1) cslgan_nn_min_i8, %d x %d x %d: %s ms, median %.2f ms; %.3g int8 ops = %.0f TOP/s achieved"
        % (nq, nb, Dp, fmt(t_min), 1e3 * med_min, work, work / med_min / 1e12))
    for k in (1, 5, 8):
        best = torch.empty((nq, k), device=dev, dtype=torch.int64)
        t = event_times_with_setup(lambda: best.fill_(-1), lambda: ops.nn_kth(q, qn, r, rn, 0, best), a.warmup, a.reps)
        say("(2) cslgan_nn_kth_i8, k = %d, best all-ones before every call (workspace %.1f MB): %s ms, median %.2f ms = %.0f TOP/s; "
            "kth / min = %.3f" % (k, ops.nn_kth_workspace_bytes(nq, nb, k) / 1e6, fmt(t), 1e3 * np.median(t), work / np.median(t) / 1e12,
                                  np.median(t) / med_min))
        if k == 1:
            same = bool((best[:, 0] == best1).all())
            say("    its keys equal those of cslgan_nn_min_i8: %s" % same)
        if k == 5:
            first = best.clone()                           # what the first block left: the bound that a later block starts from
            t = event_times_with_setup(lambda: best.copy_(first), lambda: ops.nn_kth(q, qn, r, rn, nb, best), a.warmup, a.reps)
            say("    k = 5 as a LATER block of a walk (best holds a first block's lists, index_base = %d): %s ms, median %.2f ms; "
                "kth / min = %.3f" % (nb, fmt(t), 1e3 * np.median(t), np.median(t) / med_min))
    radius = torch.randint(lo, hi + 1, (nb,), device=dev, dtype=torch.int64, generator=g).to(torch.int32)     # below 2^31 at this d
    counts = torch.zeros(nq, device=dev, dtype=torch.int32)
    t = event_times(lambda: ops.nn_count_radius(q, qn, r, rn, radius, counts), a.warmup, a.reps)
    calls = a.warmup + a.reps
    say("(3) cslgan_nn_count_radius_i8, radii in [%d, %d]: %s ms, median %.2f ms = %.0f TOP/s; count_radius / min = %.3f; share of pairs "
        "counted: %.3f" % (lo, hi, fmt(t), 1e3 * np.median(t), work / np.median(t) / 1e12, np.median(t) / med_min,
                           float(counts.sum(dtype=torch.int64)) / calls / nb / nq))
    t_min2 = event_times(lambda: ops.nn_min(q, qn, r, rn, 0, best1), 1, a.reps)
    say("    cslgan_nn_min_i8 again, at the end: %s ms, median %.2f ms" % (fmt(t_min2), 1e3 * np.median(t_min2)))
    del q, qn, r, rn, best, best1, first, counts, radius
    torch.cuda.empty_cache()

    # ---- (4) the command end to end -----------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="prdc_bench_")
    try:
        t0 = time.perf_counter()
        for name, n in (("train", a.n_train), ("heldout", a.n_heldout), ("syn", a.n_syn)):
            w = CacheWriter(os.path.join(tmp, name), n, shape[0], shape[1], shape[2], True, {"note": "random bytes"})
            for s in range(0, n, 16384):
                c = min(16384, n - s)
                w(s, rand(c).cpu().numpy(), np.zeros(c, dtype=np.int64))
            w.close()
        say("(4) caches of random bytes written in %.1f s: %d train, %d held-out, %d synthetic images of %d bytes"
            % (time.perf_counter() - t0, a.n_train, a.n_heldout, a.n_syn, a.d))
        argv4 = ["--syn_cache", os.path.join(tmp, "syn"), "--train_cache", os.path.join(tmp, "train"), "--nontrain_cache", os.path.join(tmp, "heldout"),
                 "--baseline", "-k", "5", "-d", "cuda:0", "--block_rows", str(a.block_rows)]
        ts = []
        for _ in range(a.cli_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with open(os.devnull, "w") as null:
                old, sys.stdout = sys.stdout, null
                try:
                    stats = prdc.main(argv4)
                finally:
                    sys.stdout = old
            ts.append(time.perf_counter() - t0)
        say("    prdc.main %s: %s s (first run first; host clock)" % (" ".join(argv4[6:]), fmt(ts, 1.0)))
        for lab, m in stats.items():
            say("    %s: precision %d / %d, density sum %d, recall %d / %d, coverage %d / %d" % (lab, m["precision_hits"], m["n_syn"], m["density_sum"],
                                                                                             m["recall_hits"], m["n_real"], m["coverage_hits"], m["n_real"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
