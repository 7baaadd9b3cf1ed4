"""What the kernels of `python -m csl_gan_amd.mmd` cost on one MI355X, each beside its yardstick, and what the test costs end to end beside
the numpy host model.  Random bytes stand in for the images (no dataset is needed).  In ONE process, per pool size N of --sizes:

  (1) cslgan_gram_d2_u8 on N rows of --d bytes: the matrix the other three read, and the like-for-like memory line — it WRITES the
      4 N^2 bytes that the partition sums READ;
  (2) cslgan_tri_hist_u32, one call without a prefix (half the matrix read, every digit in few bins) and the four-call select of the
      median with its three trips to the host;
  (3) cslgan_mmd_kernel_u32 with --scales bandwidths: 4 N^2 bytes read and written, 2 B table gathers per entry; it rewrites its input,
      so the distances are stored afresh before every timed call;
  (4) cslgan_mmd_partition_sums_i64 with --p partitions of random halves: N x P x N on four int8 limbs, 8 N N P integer operations of
      matrix work, beside gram_d2's time on the same matrix and beside the int8 matrix rate of the MI355X (twice the dense bf16 rate,
      about 5 POP/s).

Then (5) kernel_test.mmd_rows end to end (host clock) on `-d cuda:0` and on `-d cpu` over --host_rows + --host_rows rows with
--host_perms relabellings; the dictionaries are compared.

Each kernel timing: --warmup calls that are thrown away, then --reps calls; all values are printed and the median is the figure.

    python scripts/mmd_bench.py [--sizes 20000 65536] [--d 784] [--p 1024] [--scales 0.25 1 4] [--host_rows 1024] [--host_perms 200]
                                [--reps 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import kernel_test, ops  # noqa: E402
from nearest_bench import event_times, fmt  # noqa: E402

INT8_PEAK = 5.0e15          # dense int8 matrix operations per second of the MI355X: twice the bf16 rate


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 65536], help="rows of the pool")
    ap.add_argument("--d", type=int, default=784, help="bytes per image")
    ap.add_argument("--p", type=int, default=1024, help="partitions of one launch")
    ap.add_argument("--scales", type=float, nargs="+", default=list(kernel_test.DEFAULT_SCALES))
    ap.add_argument("--host_rows", type=int, default=1024, help="rows of each side of the end-to-end run (0: skip it)")
    ap.add_argument("--host_perms", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mmd_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    B = len(a.scales)
    say("mmd_bench: %s, pools of %s rows x %d random bytes, %d partitions, %d bandwidths; %d warm-up + %d timed calls, all values then the "
        "median" % (torch.cuda.get_device_name(0), " and ".join(str(n) for n in a.sizes), a.d, a.p, B, a.warmup, a.reps))

    for N in a.sizes:
        x = torch.randint(0, 256, (N, a.d), device=dev, dtype=torch.uint8, generator=g)
        xs, sq = ops.nn_prepare(x)
        d2 = torch.empty((N, ops.gram_pitch(N)), device=dev, dtype=torch.int32)
        mat = 4.0 * N * N
        say("N = %d: a matrix of %.2f GB" % (N, 1e-9 * mat))
        t_gr = event_times(lambda: ops.gram_d2(xs, sq, out=d2), a.warmup, a.reps)
        say("(1) cslgan_gram_d2_u8, D = %d: %s ms, median %.2f ms = %.2f TB/s written"
            % (a.d, fmt(t_gr), 1e3 * np.median(t_gr), mat / np.median(t_gr) / 1e12))
        hist = torch.zeros(256, device=dev, dtype=torch.int64)
        t_h = event_times(lambda: ops.tri_hist(d2, 0, 0, hist=hist), a.warmup, a.reps)
        t0 = time.perf_counter()
        med = kernel_test.median_d2(d2, N, dev)
        t_sel = time.perf_counter() - t0
        say("(2) cslgan_tri_hist_u32 without a prefix: %s ms, median %.2f ms = %.2f TB/s of the triangle read; the four-call select (host "
            "clock): %.1f ms, median d2 = %d" % (fmt(t_h), 1e3 * np.median(t_h), mat / 2 / np.median(t_h) / 1e12, 1e3 * t_sel, med))
        hi, lo = (torch.from_numpy(t).to(dev) for t in kernel_test.kernel_tables(med, a.scales))
        t_k = []
        for rep in range(a.warmup + a.reps):                    # the kernel rewrites its input: every call gets the distances afresh
            ops.gram_d2(xs, sq, out=d2)
            t = event_times(lambda: ops.mmd_kernel(d2, hi, lo), 0, 1)
            if rep >= a.warmup:
                t_k += t
        say("(3) cslgan_mmd_kernel_u32, B = %d: %s ms, median %.2f ms = %.2f TB/s read + written, %.1f G entries/s"
            % (B, fmt(t_k), 1e3 * np.median(t_k), 2 * mat / np.median(t_k) / 1e12, N * N / np.median(t_k) / 1e9))
        member = torch.zeros((a.p, ops.mmd_padded_cols(N)), device=dev, dtype=torch.int8)
        member[:, :N] = (torch.rand((a.p, N), device=dev, generator=g) < 0.5).to(torch.int8)
        sxx2, sxy = torch.zeros(a.p, device=dev, dtype=torch.int64), torch.zeros(a.p, device=dev, dtype=torch.int64)
        t_p = event_times(lambda: ops.mmd_partition_sums(d2, member, sxx2, sxy), a.warmup, a.reps)
        work = 8.0 * N * N * a.p
        md = np.median(t_p)
        say("(4) cslgan_mmd_partition_sums_i64, P = %d: %s ms, median %.2f ms = %.0f TOP/s on four limbs (%.1f %% of the %.0f POP/s int8 "
            "rate), the matrix read at %.2f TB/s if once; partition sums / gram_d2 = %.2f"
            % (a.p, fmt(t_p), 1e3 * md, work / md / 1e12, 100.0 * work / md / INT8_PEAK, INT8_PEAK / 1e15, mat / md / 1e12, md / np.median(t_gr)))
        calls = a.warmup + a.reps
        mi = member[:2, :N].to(torch.int64)                     # two partitions again: r as a float64 product (below 2^47: exact), then int64
        mf = mi.to(torch.float64)
        xx, xy = torch.zeros(2, device=dev, dtype=torch.int64), torch.zeros(2, device=dev, dtype=torch.int64)
        for r0 in range(0, N, 4096):
            r = (d2[r0:r0 + 4096, :N].to(torch.float64) @ mf.T).to(torch.int64)
            xx += (r * mi[:, r0:r0 + 4096].T).sum(0)
            xy += (r * (1 - mi[:, r0:r0 + 4096].T)).sum(0)
        ok = bool((sxx2[:2] == calls * xx).all()) and bool((sxy[:2] == calls * xy).all())
        say("    after %d calls the sums of the first two partitions are %d times a float64 product's (sxx2[0] = %d): %s; the histogram "
            "holds %d x N (N - 1) / 2 entries: %s" % (calls, calls, int(xx[0]), ok, calls, int(hist.sum()) == calls * (N * (N - 1) // 2)))
        del x, xs, sq, d2, member, hi, lo
        torch.cuda.empty_cache()

    if a.host_rows > 0:
        h = a.host_rows
        rng = np.random.default_rng(3)
        X, Y = rng.integers(0, 256, (h, a.d)).astype(np.uint8), rng.integers(16, 240, (h, a.d)).astype(np.uint8)

        def clock(device):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = kernel_test.mmd_rows(X, Y, n_perms=a.host_perms, scales=a.scales, seed=0, device=device)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        clock("cuda:0")
        t_dev, (f_dev, v_dev) = clock("cuda:0")
        t_cpu, (f_cpu, v_cpu) = clock("cpu")
        say("(5) kernel_test.mmd_rows, %d + %d rows, %d relabellings (host clock, the partitions drawn on the host on both paths): -d cuda:0 "
            "%.2f s, -d cpu (the numpy host model) %.2f s; figures and integers equal: %s; mmd2 %.6e, p %.4f"
            % (h, h, a.host_perms, t_dev, t_cpu, f_dev == f_cpu and v_dev["T"] == v_cpu["T"], f_dev["mmd2"], f_dev["p_value"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
