"""What the kernels of `python -m csl_gan_amd.frechet` cost on one MI355X, each beside its yardstick, and what the figure costs end to end:
the integer moments on the device and the float64 eigen step on the host, timed SEPARATELY, beside the numpy host model.  Random bytes stand
in for the images (no dataset is needed).  In ONE process:

  (1) cslgan_swd_project_i8 on the transposed image of --chunk_rows images of --d bytes against ITSELF (the full D x D square through the
      tile loop, int32 stored) and cslgan_mom_gram_i64 on the same operand (the tiles on and below the diagonal, added to int64): with T
      row tiles the triangle can give (T + 1) / (2 T) of the square's time; the yardstick is read again at the end;
  (2) cslgan_mom_transpose_u8 of that chunk beside a device copy of the same bytes, then cslgan_mom_colsum_i64 and cslgan_mom_mirror_i64;
  (3) the command's work on caches of random bytes of CelebA's sizes with --baseline, in its parts (host clock): moments.byte_moments on
      the device per set, then the host step — the covariance and its root once (one eigh), and per set frechet_from_moments (the
      covariance, two D x D x D products, one eigvalsh);
  (4) moments.byte_moments on `-d cpu` (the numpy host model) over the first --host_rows rows of the synthetic cache, beside the device on
      the same rows; the integers are compared.

Each kernel timing: --warmup calls that are thrown away, then --reps calls; all values are printed and the median is the figure.

    python scripts/frechet_bench.py [--chunk_rows 16384] [--d 12288] [--n_train 162770] [--n_heldout 19962] [--n_syn 10000]
                                    [--host_rows 2048] [--reps 5] [--out FILE]
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
from csl_gan_amd import moments, ops, pipeline  # noqa: E402
from csl_gan_amd.generate import CacheWriter  # noqa: E402
from nearest_bench import event_times, fmt  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk_rows", type=int, default=16384, help="images of the kernel timings and of one device block end to end")
    ap.add_argument("--d", type=int, default=12288, help="bytes per image; written as a [d / 3, 1, 3] image")
    ap.add_argument("--n_train", type=int, default=162770)
    ap.add_argument("--n_heldout", type=int, default=19962)
    ap.add_argument("--n_syn", type=int, default=10000)
    ap.add_argument("--host_rows", type=int, default=2048, help="rows of the -d cpu run (0: skip it)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("frechet_bench.py measures on an MI355X; no device is visible")
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
    D, n = a.d, a.chunk_rows
    np_ = ops.mom_padded_rows(n)
    T = (D + 127) // 128
    say("frechet_bench: %s, a chunk of %d images x %d bytes (np = %d, %d row tiles), random bytes; %d warm-up + %d timed calls, all values "
        "then the median" % (torch.cuda.get_device_name(0), n, D, np_, T, a.warmup, a.reps))

    # ---- (1) the Gram beside the full square of the projection kernel on the same operand --------------------------------------------------------
    x = rand(n)
    xt = ops.mom_transpose(x)
    Y = torch.empty((D, D), device=dev, dtype=torch.int32)
    S2 = torch.zeros((D, D), device=dev, dtype=torch.int64)
    work = 2.0 * D * D * np_
    t_sq = event_times(lambda: ops.swd_project(xt, xt, Y), a.warmup, a.reps)
    t_gr = event_times(lambda: ops.mom_gram(xt, S2), a.warmup, a.reps)
    t_sq2 = event_times(lambda: ops.swd_project(xt, xt, Y), 1, a.reps)
    say("(1) cslgan_swd_project_i8, xt against xt, %d x %d x %d: %s ms, median %.2f ms = %.0f TOP/s; again at the end: %s ms, median %.2f ms"
        % (D, D, np_, fmt(t_sq), 1e3 * np.median(t_sq), work / np.median(t_sq) / 1e12, fmt(t_sq2), 1e3 * np.median(t_sq2)))
    say("    cslgan_mom_gram_i64 on the same operand (%d of %d tiles): %s ms, median %.2f ms = %.0f TOP/s of the triangle; gram / square = %.3f, "
        "(T + 1) / (2 T) = %.3f" % (T * (T + 1) // 2, T * T, fmt(t_gr), 1e3 * np.median(t_gr),
                                    work * (T + 1) / (2.0 * T) / np.median(t_gr) / 1e12, np.median(t_gr) / np.median(t_sq), (T + 1) / (2.0 * T)))
    calls = a.warmup + a.reps
    ops.mom_mirror(S2)
    lower = bool((torch.tril(S2) == calls * torch.tril(Y.to(torch.int64))).all())
    say("    after %d calls and the mirror the int64 matrix is symmetric: %s, and %d times the square's lower triangle: %s"
        % (calls, bool((S2 == S2.T).all()), calls, lower))
    del Y
    torch.cuda.empty_cache()

    # ---- (2) the transpose beside a device copy, the column sums, the mirror -------------------------------------------------------------------
    xc = torch.empty_like(x)
    s1 = torch.zeros(D, device=dev, dtype=torch.int64)
    t_cp = event_times(lambda: xc.copy_(x), a.warmup, a.reps)
    t_tr = event_times(lambda: ops.mom_transpose(x, out=xt), a.warmup, a.reps)
    t_cs = event_times(lambda: ops.mom_colsum(xt, s1), a.warmup, a.reps)
    t_mi = event_times(lambda: ops.mom_mirror(S2), a.warmup, a.reps)
    say("(2) device copy of %.0f MB: %s ms, median %.3f ms; cslgan_mom_transpose_u8 of the same bytes: %s ms, median %.3f ms; transpose / copy "
        "= %.2f" % (1e-6 * n * D, fmt(t_cp, f="%.3f"), 1e3 * np.median(t_cp), fmt(t_tr, f="%.3f"), 1e3 * np.median(t_tr),
                    np.median(t_tr) / np.median(t_cp)))
    say("    cslgan_mom_colsum_i64: %s ms, median %.3f ms; cslgan_mom_mirror_i64 of %d x %d int64: %s ms, median %.3f ms"
        % (fmt(t_cs, f="%.3f"), 1e3 * np.median(t_cs), D, D, fmt(t_mi, f="%.3f"), 1e3 * np.median(t_mi)))
    del x, xc, xt, S2, s1
    torch.cuda.empty_cache()

    # ---- (3) the command's work in its parts -----------------------------------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="frechet_bench_")
    try:
        t0 = time.perf_counter()
        for name, rows in (("train", a.n_train), ("heldout", a.n_heldout), ("syn", a.n_syn)):
            w = CacheWriter(os.path.join(tmp, name), rows, shape[0], shape[1], shape[2], True, {"note": "random bytes"})
            for s in range(0, rows, 16384):
                c = min(16384, rows - s)
                w(s, rand(c).cpu().numpy(), np.zeros(c, dtype=np.int64))
            w.close()
        say("(3) caches of random bytes written in %.1f s: %d train, %d held-out, %d synthetic images of %d bytes"
            % (time.perf_counter() - t0, a.n_train, a.n_heldout, a.n_syn, D))
        caches = {name: pipeline.CachedImages(os.path.join(tmp, name)) for name in ("train", "heldout", "syn")}

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        mom, t_mom = {}, {}
        for name, c in caches.items():
            for _ in range(2):
                t, mom[name] = clock(lambda: moments.byte_moments(c, "cuda:0", block_rows=a.chunk_rows))
                t_mom.setdefault(name, []).append(t)
        say("    moments.byte_moments -d cuda:0, blocks of %d (host clock, first run first; cache read, copies and the %.1f GB matrix back "
            "included): train %s s, held-out %s s, synthetic %s s" % (a.chunk_rows, 8e-9 * D * D, fmt(t_mom["train"], 1.0),
                                                                     fmt(t_mom["heldout"], 1.0), fmt(t_mom["syn"], 1.0)))
        t_real, real = clock(lambda: moments.RealSide(caches["train"], mom["train"]))
        say("    host step, float64, OMP_NUM_THREADS=%s: covariance and root of the training set (one eigh of %d x %d): %.1f s"
            % (os.environ.get("OMP_NUM_THREADS", "unset"), D, D, t_real))
        t_fd = []
        for name in ("syn", "heldout"):
            t, m = clock(lambda: moments.frechet_from_moments(real.moments, mom[name], sqrt_a=real.sqrt, cov_a=real.cov))
            t_fd.append(t)
            say("    host step per set (covariance, two %d^3 products, one eigvalsh): %s %.1f s; fd %.4f bytes^2 = mean %.4f + traces %.4f - 2 x "
                "root %.4f (%d against %d images)" % (D, name, t, m["fd"], m["mean_term"], m["trace_term"], m["sqrt_term"], m["n_b"], m["n_a"]))
        dev_s = sum(t[1] for t in t_mom.values())
        say("    end to end with --baseline: moments %.1f s + host step %.1f s; the host step is %.0f %% of the sum"
            % (dev_s, t_real + sum(t_fd), 100.0 * (t_real + sum(t_fd)) / (dev_s + t_real + sum(t_fd))))

        # ---- (4) the host model on a fraction ------------------------------------------------------------------------------------------------------
        if a.host_rows > 0:
            h = min(a.host_rows, a.n_syn)
            part = pipeline.CachedImages.from_arrays(np.array(caches["syn"].x[:h]), np.zeros(h), True)
            t_host, mh = clock(lambda: moments.byte_moments(part, "cpu", block_rows=a.chunk_rows))
            t_dev, md = clock(lambda: moments.byte_moments(part, "cuda:0", block_rows=a.chunk_rows))
            same = bool(np.array_equal(mh["s1"], md["s1"]) and np.array_equal(mh["s2"], md["s2"]))
            say("(4) moments.byte_moments -d cpu (the numpy host model; host clock) over %d rows, %.4f of the three sets: %.1f s, so about %.0f s "
                "for all of them; the device on the same rows: %.2f s; integers equal: %s"
                % (h, h / float(a.n_train + a.n_heldout + a.n_syn), t_host, t_host * (a.n_train + a.n_heldout + a.n_syn) / h, t_dev, same))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
