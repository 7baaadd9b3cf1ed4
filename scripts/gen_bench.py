"""Images/s of synthetic-dataset generation from a CelebA-64 GroupNorm generator, two paths alternated in ONE process (A/B/A/B):

  (A) csl_gan_amd.generate.SampleGenerator: latent kernel -> frozen G -> cslgan_f32_to_u8 replayed from a HIP graph, bytes leave
      through two pinned buffers on a side stream, a writer thread fills a uint8 memmap (the cache format);
  (B) what the tree could do per batch before: eager G(z) on torch-drawn z, .to("cpu"), util.denorm_celeba, the host quantisation
      of util.save_image, the same memmap.

End to end is a host clock around a window that ends in a device synchronise and, for (A), the writer thread's join.  "device" is the
time HIP events see for the same number of batches with nothing leaving the device (graph replays / eager forwards back to back):
launch gaps of the eager path are inside it, so it is an upper bound of kernel time, not kernel time; a kernel-only figure comes from
a `rocprofv3 --kernel-trace --stats -- python scripts/gen_bench.py --only A|B ...` run of its own (--only keeps one path).

    python scripts/gen_bench.py [--bs 128 512] [--images 16384] [--rounds 2] [--only A|B] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import generate, init_util, options, util  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="*", default=[128, 512])
    ap.add_argument("--images", type=int, default=16384, help="images per timed window")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=["A", "B"], default=None)
    ap.add_argument("--compute_dtype", default="fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gen_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = tempfile.mkdtemp(prefix="gen_bench_") + "/"
    opt = options.parse(["CelebA", "-dpm", "gc", "-gcm", "adaptive-pl", "-nms", "4", "-gd", "cuda:0", "-dd", "cuda:0", "-o", tmp, "--manual_seed", "1",
                         "--synthetic", "--compute_dtype", a.compute_dtype])
    G, _ = init_util.init_models(opt, init_D=False)
    G.eval()
    dev = torch.device("cuda:0")
    say("gen_bench: CelebA-64 GroupNorm generator (%.1f M parameters), compute_dtype %s, %d images per window, %d rounds, %s"
        % (sum(p.numel() for p in G.parameters()) / 1e6, a.compute_dtype, a.images, a.rounds, torch.cuda.get_device_name(0)))

    for bs in a.bs:
        nb = max(a.images // bs, 4)
        n = nb * bs
        mm = np.lib.format.open_memmap(tmp + "bench_%d.u8" % bs, mode="w+", dtype=np.uint8, shape=(n, 64, 64, 3))
        gen = generate.SampleGenerator(G, opt, dev, 1, bs, hip_graph=True, compute_dtype=a.compute_dtype)

        def sink(start, rows, labels):
            mm[start:start + len(rows)] = rows

        def run_a(nb):
            gen.generate(0, nb * bs, sink)

        def dev_a(nb):
            for k in range(nb):
                gen.device_batch(k * bs)

        @torch.no_grad()
        def batch_b(z):
            return G(z.normal_(0.0, 1.0))

        @torch.no_grad()
        def run_b(nb):
            z = torch.empty((bs, opt.g_latent_dim), device=dev)
            for k in range(nb):
                fake = util.denorm_celeba(batch_b(z).to("cpu"))
                mm[k * bs:(k + 1) * bs] = fake.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
            torch.cuda.synchronize()

        @torch.no_grad()
        def dev_b(nb):
            z = torch.empty((bs, opt.g_latent_dim), device=dev)
            for k in range(nb):
                batch_b(z)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(nb)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def events(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn(nb)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        paths = [p for p in (("A", run_a, dev_a), ("B", run_b, dev_b)) if a.only in (None, p[0])]
        for _, run, devfn in paths:               # warm-up: every shape of the timed windows, the graph recording included
            run(3)
            devfn(3)
        res = {p[0]: {"e2e": [], "dev": []} for p in paths}
        for r in range(a.rounds):
            for name, run, devfn in paths:
                res[name]["e2e"].append(n / wall(run))
                res[name]["dev"].append(n / events(devfn))
        say("-bs %d, %d batches (%d images) per window" % (bs, nb, n))
        for name, _, _ in paths:
            e, d = res[name]["e2e"], res[name]["dev"]
            say("  (%s) end to end %s images/s (mean %.0f)   device only %s images/s (mean %.0f, %.3f ms per batch)"
                % (name, " / ".join("%.0f" % v for v in e), np.mean(e), " / ".join("%.0f" % v for v in d), np.mean(d), 1e3 * bs / np.mean(d)))
        if len(paths) == 2:
            say("  (A) / (B): end to end %.2fx, device only %.2fx" % (np.mean(res["A"]["e2e"]) / np.mean(res["B"]["e2e"]),
                                                                   np.mean(res["A"]["dev"]) / np.mean(res["B"]["dev"])))
        gen.release()
        del mm
        os.remove(tmp + "bench_%d.u8" % bs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
