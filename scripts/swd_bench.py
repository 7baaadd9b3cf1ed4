"""What the kernels of `python -m csl_gan_amd.swd` cost on one MI355X, each beside its yardstick, and what the command costs end to end
beside the numpy host model.  Random bytes stand in for the images (no dataset is needed).  In ONE process:

  (1) cslgan_swd_project_i8, --n_dirs directions against one prepared block of --block_rows images of --d bytes, beside
      cslgan_nn_min_i8 on the SAME operands (the directions as its queries): the same tile loop, a store in place of a running minimum;
  (2) cslgan_sort_rows_i32 (key_bits = 25, the projections' range) beside torch.sort(dim=1) of the same matrix on the device, at
      --n_dirs x 10 000 and --n_dirs x --n_train; the matrix is restored from a copy before every call, outside the timed region;
  (3) cslgan_swd_w1_i64 at --n_dirs x --n_train against --n_dirs x --n_syn;
  (4) `swd.main` end to end (host clock, in this process) on caches of random bytes of CelebA's sizes with --baseline, on the device and
      — with --host_dirs directions — on `-d cpu`, the numpy host model; the numerators of the shared directions are compared.

Each kernel timing: --warmup calls that are thrown away, then --reps calls; all values are printed and the median is the figure.

    python scripts/swd_bench.py [--n_dirs 1024] [--block_rows 16384] [--d 12288] [--n_train 162770] [--n_heldout 19962] [--n_syn 10000]
                                [--host_dirs 64] [--reps 5] [--out FILE]
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
from csl_gan_amd import ops, swd  # noqa: E402
from csl_gan_amd.generate import CacheWriter  # noqa: E402
from nearest_bench import event_times, fmt  # noqa: E402
from prdc_bench import event_times_with_setup  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_dirs", type=int, default=1024)
    ap.add_argument("--block_rows", type=int, default=16384)
    ap.add_argument("--d", type=int, default=12288, help="bytes per image; written as a [d / 3, 1, 3] image")
    ap.add_argument("--n_train", type=int, default=162770)
    ap.add_argument("--n_heldout", type=int, default=19962)
    ap.add_argument("--n_syn", type=int, default=10000)
    ap.add_argument("--host_dirs", type=int, default=64, help="directions of the -d cpu run (0: skip it)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("swd_bench.py measures on an MI355X; no device is visible")
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
    P, nb, Dp = a.n_dirs, a.block_rows, ops.nn_padded_dim(a.d)
    say("swd_bench: %s, %d directions, blocks of %d images x %d bytes (Dp = %d), random bytes; %d warm-up + %d timed calls, all values then "
        "the median" % (torch.cuda.get_device_name(0), P, nb, a.d, Dp, a.warmup, a.reps))

    # ---- (1) the projection beside the search kernel on the same operands --------------------------------------------------------------------
    dirs = ops.swd_directions(P, a.d, 0, dev)
    dn = torch.full((P,), a.d, device=dev, dtype=torch.int32)
    r, rn = ops.nn_prepare(rand(nb))
    Y = torch.empty((P, nb), device=dev, dtype=torch.int32)
    best = torch.full((P,), -1, device=dev, dtype=torch.int64)
    work = 2.0 * P * nb * Dp
    t_min = event_times(lambda: ops.nn_min(dirs, dn, r, rn, 0, best), a.warmup, a.reps)
    t_prj = event_times(lambda: ops.swd_project(dirs, r, Y), a.warmup, a.reps)
    t_min2 = event_times(lambda: ops.nn_min(dirs, dn, r, rn, 0, best), 1, a.reps)
    say("(1) cslgan_nn_min_i8, %d x %d x %d: %s ms, median %.2f ms = %.0f TOP/s; again at the end: %s ms, median %.2f ms"
        % (P, nb, Dp, fmt(t_min), 1e3 * np.median(t_min), work / np.median(t_min) / 1e12, fmt(t_min2), 1e3 * np.median(t_min2)))
    say("    cslgan_swd_project_i8 on the same operands (%.0f MB stored): %s ms, median %.2f ms = %.0f TOP/s; project / min = %.3f"
        % (4e-6 * P * nb, fmt(t_prj), 1e3 * np.median(t_prj), work / np.median(t_prj) / 1e12, np.median(t_prj) / np.median(t_min)))
    del dirs, dn, r, rn, Y, best
    torch.cuda.empty_cache()

    # ---- (2) the sort beside torch.sort ------------------------------------------------------------------------------------------------------
    for n in (10000, a.n_train):
        src = torch.randint(-128 * a.d, 128 * a.d + 1, (P, n), device=dev, dtype=torch.int32, generator=g)
        x = torch.empty_like(src)
        ws = torch.empty(ops.sort_rows_ws_bytes(P, n), device=dev, dtype=torch.uint8)
        t_own = event_times_with_setup(lambda: x.copy_(src), lambda: ops.sort_rows(x, key_bits=25, ws=ws), a.warmup, a.reps)
        own = x.clone()
        t_32 = event_times_with_setup(lambda: x.copy_(src), lambda: ops.sort_rows(x, key_bits=32, ws=ws), a.warmup, a.reps)
        del ws
        out = []
        t_torch = event_times(lambda: out.__setitem__(slice(None), [torch.sort(src, dim=1).values]), a.warmup, a.reps)
        same = bool((own == out[0]).all())
        say("(2) %d x %d int32: cslgan_sort_rows_i32 key_bits 25 (4 passes): %s ms, median %.2f ms; key_bits 32: median %.2f ms; "
            "torch.sort(dim=1): %s ms, median %.2f ms; sort_rows / torch.sort = %.3f; equal: %s"
            % (P, n, fmt(t_own), 1e3 * np.median(t_own), 1e3 * np.median(t_32), fmt(t_torch), 1e3 * np.median(t_torch),
               np.median(t_own) / np.median(t_torch), same))
        if n == a.n_train:                                                                  # (3) on the sorted matrix
            b = torch.sort(torch.randint(-128 * a.d, 128 * a.d + 1, (P, a.n_syn), device=dev, dtype=torch.int32, generator=g), dim=1).values
            num = torch.empty(P, device=dev, dtype=torch.int64)
            t_w1 = event_times(lambda: ops.swd_w1(own, n, b, a.n_syn, out=num), a.warmup, a.reps)
            say("(3) cslgan_swd_w1_i64, %d directions, %d against %d entries: %s ms, median %.2f ms" % (P, n, a.n_syn, fmt(t_w1), 1e3 * np.median(t_w1)))
            del b, num
        del src, x, own, out
        torch.cuda.empty_cache()

    # ---- (4) the command end to end ------------------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="swd_bench_")
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
        base = ["--syn_cache", os.path.join(tmp, "syn"), "--train_cache", os.path.join(tmp, "train"), "--nontrain_cache", os.path.join(tmp, "heldout"),
                "--baseline", "--block_rows", str(a.block_rows)]

        def run(extra, vals):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with open(os.devnull, "w") as null:
                old, sys.stdout = sys.stdout, null
                try:
                    stats = swd.main(base + extra + ["--values_dir", os.path.join(tmp, vals)])
                finally:
                    sys.stdout = old
            return time.perf_counter() - t0, stats, np.load(os.path.join(tmp, vals, "syn_num.npy"))

        ts = []
        for _ in range(2):
            t, stats, num_dev = run(["-d", "cuda:0", "--n_dirs", str(P)], "dev")
            ts.append(t)
        say("    swd.main -d cuda:0 --n_dirs %d --baseline: %s s (first run first; host clock)" % (P, fmt(ts, 1.0)))
        for lab, m in stats.items():
            say("    %s: swd %.4f bytes, max sliced %.4f, stderr %.4f (%d against %d images)" % (lab, m["swd"], m["max_sliced"], m["stderr"], m["n_b"], m["n_a"]))
        if a.host_dirs > 0:
            h = min(a.host_dirs, P)
            t, _, num_host = run(["-d", "cpu", "--n_dirs", str(h)], "host")
            say("    swd.main -d cpu --n_dirs %d --baseline (the numpy host model; host clock): %.1f s; its numerators equal the device's first %d: %s"
                % (h, t, h, bool(np.array_equal(num_host, num_dev[:h]))))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
