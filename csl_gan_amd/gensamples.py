"""Samples of a saved generator: `python -m csl_gan_amd.gensamples path [-e EPOCHS] [-n NUM] [-bs BS] [-d DEVICE]` — the reference's
gensamples.py (flags and defaults of gensamples.py:9-13, output folder of :19, model loading of :26-32).

Reads `path/opt.txt`, builds only G on the requested device, loads `path/saves/G-<EPOCHS>` with the no-code loader and writes

  without --cache   one PNG per sample, `path/G-<EPOCHS>-samples/<k>.png`, k 1-based over the whole index range (gensamples.py:40-41);
  with --cache OUT  the uint8 NHWC cache of csl_gan_amd.pipeline (`OUT.u8`, `OUT.labels.npy`, `OUT.json`) that CachedImages and
                    `train --data_cache OUT` read as it is, and PNGs only for the first --png K samples.

Additions: --seed (default: the run's recorded manual_seed; printed), --first_index, --cache, --png, --label, --hip_graph,
--compute_dtype.  The work is csl_gan_amd.generate.SampleGenerator's.

Deliberate differences from the reference:
  * exactly -n samples are written — the reference drops the num_samples % batch_size tail (gensamples.py:35);
  * z comes from the indexed stream of csl_gan_amd.generate, not from the process RNG: sample k is the same image whatever -bs,
    --first_index / -n split or device count produced it (the reference's output changes with -bs);
  * a conditional generator gets class-balanced labels (index mod n_classes, or --label K for one class) — the reference calls
    G(z) without y and fails on it.
"""
import argparse
import sys

from . import generate, init_util, options, util


def build_parser():
    ap = argparse.ArgumentParser(description="Generate samples / a synthetic dataset from a saved generator")
    ap.add_argument("path", type=str, help="Path to the output folder containing the generator save")
    ap.add_argument("-e", "--epochs", type=int, default=-1, help="Epochs trained for the generator save")
    ap.add_argument("-n", "--num_samples", type=int, default=100)
    ap.add_argument("-bs", "--batch_size", type=int, default=50)
    ap.add_argument("-d", "--device", type=str, default="cpu")
    # ---- additions of this build ----
    ap.add_argument("--seed", type=int, default=None, help="seed of the latent stream (default: the run's manual_seed)")
    ap.add_argument("--first_index", type=int, default=0, help="index of the first sample (shard a range by hand: the outputs concatenate)")
    ap.add_argument("--cache", type=str, default=None, help="write the uint8 NHWC cache OUT.u8 / OUT.labels.npy / OUT.json")
    ap.add_argument("--png", type=int, default=None, help="with --cache: also write PNGs of the first K samples")
    ap.add_argument("--label", type=int, default=-1, help="conditional generators: one class for every sample (default: index mod n_classes)")
    ap.add_argument("--hip_graph", type=options.str2bool, default=True, help="record full batches in a HIP graph (device runs)")
    ap.add_argument("--compute_dtype", type=str, choices=["fp32", "bf16", "bf16x3", "fp32_auto"], default=None,
                    help="arithmetic of the conv kernels (default: the training run's)")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    path = util.add_slash(a.path)
    train_opt = options.load_opt(path + "opt.txt")
    seed = int(train_opt.manual_seed) if a.seed is None else a.seed
    if a.first_index < 0 or a.num_samples < 0:
        raise SystemExit("--first_index and -n must not be negative")
    if a.label >= 0 and not train_opt.conditional:
        raise SystemExit("--label needs a conditional generator")
    print("latent seed: %d   samples %d .. %d" % (seed, a.first_index, a.first_index + a.num_samples - 1))

    train_opt.g_device = a.device
    G, _ = init_util.init_models(train_opt, init_D=False)
    ckpt = path + "saves/G-" + str(a.epochs)
    util.load_model(ckpt, G, device=a.device)
    gen = generate.SampleGenerator(G, train_opt, a.device, seed, a.batch_size, hip_graph=a.hip_graph, compute_dtype=a.compute_dtype,
                                   fixed_label=a.label)

    png_dir = path + "G-" + str(a.epochs) + "-samples/"
    cache = pngs = None
    if a.cache is None:
        pngs = generate.PngWriter(png_dir, number_from=a.first_index + 1)
    else:
        info = {"checkpoint": ckpt, "epochs": a.epochs, "seed": seed, "first_index": a.first_index,
                "label_mode": ("fixed:%d" % a.label) if a.label >= 0 else ("index mod %d" % gen.n_classes if gen.conditional else "none"),
                "compute_dtype": gen.compute_dtype if gen.on_gpu else "torch-cpu"}
        cache = generate.CacheWriter(a.cache, a.num_samples, gen.H, gen.W, gen.C, gen.signed, info)
        if a.png:
            pngs = generate.PngWriter(png_dir, number_from=a.first_index + 1, limit=a.png)
    try:
        gen.generate(a.first_index, a.num_samples, generate.tee(cache, pngs))
    finally:
        gen.release()
        hdr = cache.close() if cache is not None else None
    if cache is not None:
        print("wrote %s.u8 (%d x %d x %d x %d uint8, signed=%s), .labels.npy, .json" % (a.cache, hdr["n"], hdr["H"], hdr["W"], hdr["C"], hdr["signed"]))
    if pngs is not None:
        print("wrote PNGs to %s" % png_dir)
    return gen


if __name__ == "__main__":
    main(sys.argv[1:])
