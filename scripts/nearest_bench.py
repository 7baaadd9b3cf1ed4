"""What `python -m csl_gan_amd.nearest` costs at the CelebA workload's size on one MI355X: 10 000 synthetic x 162 770 training images of
64 x 64 x 3 = 12 288 bytes, i.e. 2.0e13 multiply-adds per query cache.  Random bytes stand in for the images (the arithmetic does not
depend on the values; no dataset is needed).  In ONE process:

  (1) cslgan_nn_prepare_u8 on one block of --block_rows images: HIP events around each call, set against the bytes it moves (reads
      D, writes Dp + 4 per row) at the 6.29 TB/s a float4 copy reaches (MI355X_MICROARCH.md);
  (2) cslgan_nn_min_i8, the 10 000 queries against one prepared block: HIP events around each call; achieved int8 TOP/s =
      2 nq nr Dp / t, beside the dense int8 matrix rate.  MI355X_MICROARCH.md "Matrix cores" gives BF16 as ~2.5 PF dense and the I8 forms
      (32x32x32 / 16x16x64) as "the cycles of the BF16 form of the same M x N at 2x the K, so 2x BF16 per clock": ~5.0 POP/s dense is the
      figure used.  No counter run is made here, so nothing is said about whether the clock or the memory limits the kernel;
  (3) NearestSearch.query end to end (host clock, synchronised): the first query streams the reference (pinned gather, upload,
      prepare, search), the later ones run against the prepared blocks that stayed on the device;
  (4) neighbours.nearest_host (float64 BLAS, the threads the process is given) on a --host_q x --host_r slice on the same machine,
      SCALED linearly to the full size: an estimate, labelled as such.

Each timing: --warmup calls that are thrown away, then --reps calls; all values are printed and the median is the figure.

    python scripts/nearest_bench.py [--nq 10000] [--nr 162770] [--d 12288] [--block_rows 16384] [--reps 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import neighbours, ops  # noqa: E402
from csl_gan_amd.pipeline import CachedImages  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
INT8_DENSE_OPS_PER_S = 5.0e15


def event_times(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def fmt(ts, unit=1e3, f="%.2f"):
    return " / ".join(f % (t * unit) for t in ts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--nr", type=int, default=162770)
    ap.add_argument("--d", type=int, default=12288, help="bytes per image; written as a [d / 3, 1, 3] image")
    ap.add_argument("--block_rows", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host_q", type=int, default=512)
    ap.add_argument("--host_r", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("nearest_bench.py measures on an MI355X; no device is visible")
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
    Rd = rand(a.nr)
    ref = CachedImages.from_arrays(Rd.cpu().numpy(), np.zeros(a.nr), True)
    Qd = rand(a.nq)
    qry = CachedImages.from_arrays(Qd.cpu().numpy(), np.zeros(a.nq), True)
    Dp = ops.nn_padded_dim(a.d)
    say("nearest_bench: %s, %d queries x %d reference images x %d bytes (Dp = %d), random bytes, block_rows %d; %d warm-up + %d timed calls, "
        "all values then the median" % (torch.cuda.get_device_name(0), a.nq, a.nr, a.d, Dp, a.block_rows, a.warmup, a.reps))

    # ---- (1) prepare -----------------------------------------------------------------------------------------------------------------
    nb = min(a.block_rows, a.nr)
    blk = Rd[:nb]
    r = torch.empty((nb, Dp), device=dev, dtype=torch.int8)
    rn = torch.empty(nb, device=dev, dtype=torch.int32)
    t = event_times(lambda: ops.nn_prepare(blk, out=r, out_sqnorm=rn), a.warmup, a.reps)
    moved = nb * (a.d + Dp + 4)
    say("(1) cslgan_nn_prepare_u8, %d rows: %s ms, median %.3f ms; %.1f MB moved = %.2f TB/s (%.0f %% of the 6.29 TB/s of a float4 copy)"
        % (nb, fmt(t, f="%.3f"), 1e3 * np.median(t), moved / 1e6, moved / np.median(t) / 1e12, 100 * moved / np.median(t) / HBM_BYTES_PER_S))
    del Rd

    # ---- (2) the search kernel -------------------------------------------------------------------------------------------------------
    q, qn = ops.nn_prepare(Qd)
    best = torch.full((a.nq,), -1, device=dev, dtype=torch.int64)
    t = event_times(lambda: ops.nn_min(q, qn, r, rn, 0, best), a.warmup, a.reps)
    work = 2.0 * a.nq * nb * Dp
    rate = work / np.median(t)
    say("(2) cslgan_nn_min_i8, %d x %d x %d: %s ms, median %.2f ms; %.3g int8 ops = %.0f TOP/s achieved, %.1f %% of the ~%.1f POP/s dense int8 "
        "matrix rate (2x the ~2.5 PF BF16 rate per clock, MI355X_MICROARCH.md 'Matrix cores'); no counter run: not said whether clock- or "
        "memory-limited" % (a.nq, nb, Dp, fmt(t), 1e3 * np.median(t), work, rate / 1e12, 100 * rate / INT8_DENSE_OPS_PER_S, INT8_DENSE_OPS_PER_S / 1e15))
    say("    the whole reference at that rate: %.2f s of kernel time per query cache" % (2.0 * a.nq * a.nr * Dp / rate))
    del q, qn, r, rn, best, Qd, blk

    # ---- (3) end to end ---------------------------------------------------------------------------------------------------------------
    s = neighbours.NearestSearch(dev, block_rows=a.block_rows, resident_gb=8.0).fit(ref)
    t_all = []
    for _ in range(1 + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keys = s.query(qry)
        t_all.append(time.perf_counter() - t0)
    say("(3) NearestSearch.query end to end (host clock): first query, reference streamed (gather + upload + prepare + search) %.2f s; "
        "later queries, %d of %d reference rows resident: %s s, median %.2f s" % (t_all[0], s.resident_rows(), a.nr, fmt(t_all[1:], 1.0), np.median(t_all[1:])))
    d2, _ = neighbours.split_keys(keys)
    say("    keys of the last query: d2 min / median / max = %d / %d / %d" % (d2.min(), np.median(d2), d2.max()))
    del s

    # ---- (4) the host model on a slice ------------------------------------------------------------------------------------------------
    hq, hr = min(a.host_q, a.nq), min(a.host_r, a.nr)
    Qh, Rh = qry.x[:hq], ref.x[:hr]
    neighbours.nearest_host(Qh[:64], Rh[:1024])
    th = []
    for _ in range(3):
        t0 = time.perf_counter()
        hk = neighbours.nearest_host(Qh, Rh)
        th.append(time.perf_counter() - t0)
    scale = (a.nq / hq) * (a.nr / hr)
    say("(4) neighbours.nearest_host (float64 BLAS, OMP_NUM_THREADS = %s) on a %d x %d slice: %s s, median %.2f s; SCALED linearly x %.1f to the full size: "
        "%.0f s (an estimate, not a measurement)" % (os.environ.get("OMP_NUM_THREADS", "unset"), hq, hr, fmt(th, 1.0), np.median(th), scale, np.median(th) * scale))
    dev_slice = neighbours.NearestSearch(dev, block_rows=4096).fit(CachedImages.from_arrays(Rh, np.zeros(hr), True)).query(
        CachedImages.from_arrays(Qh, np.zeros(hq), True))
    say("    device keys == host keys on that slice: %s" % bool(np.array_equal(dev_slice, hk)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
