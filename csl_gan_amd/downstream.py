"""Downstream utility of a saved conditional MNIST generator: `python -m csl_gan_amd.downstream RUN [-e E | -ei 100] [-bs 50]
[-d cuda:0] [-c lr]` — the reference's downstream.py.  Per checkpoint `RUN/saves/G-<epoch>` it generates -n labelled images, fits a
one-vs-rest logistic regression on them (csl_gan_amd.classify.OvrLogReg), scores the real MNIST test set and appends the
micro-averaged AUROC to `RUN/downstream_log.csv` (header `Epoch,lr AUROC`, one row per checkpoint; downstream.py:112-145).

Kept from downstream.py:26-35, :43-46, :118-150: the flags and their defaults, the MNIST-only refusal, the loop from
--epoch_interval (or the single --epochs) in steps of --epoch_interval until a save is missing, the printed line and the csv.
Additions: -n (the reference's literal 10000), --seed, --hip_graph, --compute_dtype, --gtol_rel, --max_iter, and --test_cache (a
labelled uint8 cache of csl_gan_amd.pipeline instead of the t10k idx files under the run's data_path).

Deliberate differences from the reference:
  * the figure is that of the MINIMISER of the estimator's objective, which is unique (strictly convex).  The reference stops
    scikit-learn's L-BFGS at tol=1e-4 / max_iter=100 with the convergence warning silenced (downstream.py:64), so its figure depends
    on where SciPy happened to stop: the same estimator, stopped early (DESIGN.md §6f has the measured gap);
  * -c accepts the reference's eight names but builds only `lr`: downstream.py:139 passes the literal "lr" to classify() whatever was
    asked (the other branches name classes it never imports).  Any other name exits with that explanation instead of logging a
    logistic-regression figure under another classifier's column;
  * z and the labels come from the indexed streams of csl_gan_amd.generate (sample k is a function of (checkpoint, seed, k); labels
    are k mod 10, balanced) instead of the process RNG's normal_ / random_(0, 10) (downstream.py:94-95): a rerun, another -bs or
    another device prints the same number;
  * a class without a generated sample raises instead of failing on a shape mismatch in predict_proba; an unconditional run is
    refused up front (the reference fails inside G(z, y));
  * the per-class AUROCs, which the reference computes and drops (:53-56), and the solver's report are printed too.
"""
import argparse
import csv
import os
import sys

import numpy as np
import torch

from . import cache_cli, classify, datasets, generate, init_util, options, pipeline, util

CLASSIFIERS = ["svm", "dt", "lr", "rf", "gnb", "bnb", "ab", "mlp"]


def build_parser():
    ap = argparse.ArgumentParser(description="Classifier AUROC of a saved conditional MNIST generator")
    ap.add_argument("path", type=str, help="Path to the output folder containing the generator save")
    ap.add_argument("-e", "--epochs", type=int, default=None, help="Epochs trained for the generator save")
    ap.add_argument("-ei", "--epoch_interval", type=int, default=100, help="Alternative to --epochs, runs on all saves with an interval of epoch_interval")
    ap.add_argument("-bs", "--batch_size", type=int, default=50)
    ap.add_argument("-d", "--device", type=str, default=None)
    ap.add_argument("-c", "--classifiers", type=str, default=["lr"], nargs="*", choices=CLASSIFIERS)
    # ---- additions of this build ----
    ap.add_argument("-n", "--num_samples", type=int, default=10000, help="generated training samples per checkpoint")
    ap.add_argument("--seed", type=int, default=None, help="seed of the latent stream (default: the run's manual_seed)")
    ap.add_argument("--test_cache", type=str, default=None, help="labelled uint8 image cache to score (default: the t10k idx files under data_path)")
    ap.add_argument("--hip_graph", type=options.str2bool, default=True, help="record full batches in a HIP graph (device runs)")
    ap.add_argument("--compute_dtype", type=str, choices=["fp32", "bf16", "bf16x3", "fp32_auto"], default=None,
                    help="arithmetic of the generator's conv kernels (default: the training run's)")
    ap.add_argument("--gtol_rel", type=float, default=None, help="a class has converged when max|gradient| <= gtol_rel * n")
    ap.add_argument("--max_iter", type=int, default=2000, help="L-BFGS iterations per class")
    return ap


def load_test_set(train_opt, test_cache):
    """(bytes [M, H*W*C] uint8, labels [M] int64).  The features are bytes / 255 whatever scale a cache records."""
    if test_cache is not None:
        return cache_cli.cache_rows(pipeline.CachedImages(test_cache))
    root = train_opt.data_path
    for d in (os.path.join(root, "MNIST", "raw"), root):                  # downstream.py:103-105 reads <data_path>MNIST/raw/
        for suf in ("", ".gz"):
            if os.path.exists(os.path.join(d, "t10k-images-idx3-ubyte" + suf)):
                x = datasets._read_idx(os.path.join(d, "t10k-images-idx3-ubyte" + suf))
                y = datasets._read_idx(os.path.join(d, "t10k-labels-idx1-ubyte" + suf))
                return np.array(x, dtype=np.uint8).reshape(len(x), -1), y.astype(np.int64)
    raise SystemExit("MNIST t10k idx files not found under %s: give --test_cache" % root)


def generated_features(gen, n):
    """(X [n, H*W*C] float32 on gen.device, labels [n] int64 ndarray): the generator's own floats of samples 0 .. n-1, never
    quantised, and the labels of the indexed label stream.  On a device the floats never leave it."""
    labels = generate.labels_host(0, n, gen.n_classes, gen.fixed_label)
    feat = gen.H * gen.W * gen.C
    X = torch.empty((n, feat), device=gen.device, dtype=torch.float32)
    if gen.on_gpu:
        with torch.cuda.device(gen.device):
            for s in range(0, n, gen.B):
                k = min(gen.B, n - s)
                X[s:s + k].copy_(gen.device_batch(s, k)["f32"].reshape(k, feat))
            torch.cuda.synchronize(gen.device)
    else:
        def keep(s, rows):
            X[s:s + len(rows)] = torch.from_numpy(rows).reshape(len(rows), feat)
        gen.generate(0, n, lambda s, rows, lab: None, float_sink=keep)
    return X, labels


def evaluate_checkpoint(G, train_opt, a, seed, device, test_x, test_y):
    """Generate, fit, predict and score one loaded generator: the dict of one csv row."""
    gen = generate.SampleGenerator(G, train_opt, device, seed, a.batch_size, hip_graph=a.hip_graph, compute_dtype=a.compute_dtype,
                                   keep_float=True)
    try:
        X, labels = generated_features(gen, a.num_samples)
    finally:
        gen.release()
    clf = classify.OvrLogReg(gen.n_classes, gtol_rel=a.gtol_rel, max_iter=a.max_iter)
    report = clf.fit(X, torch.from_numpy(labels))
    P = clf.predict_proba(test_x)
    out = classify.auroc(P, test_y)
    out["solver"] = report
    return out


def main(argv=None):
    a = build_parser().parse_args(argv)
    other = [c for c in a.classifiers if c != "lr"]
    if other or not a.classifiers:
        raise SystemExit("only the logistic regression is built (-c lr): the reference runs `lr` whatever -c names (downstream.py:139 "
                         "passes the literal \"lr\"), so %s would log a logistic-regression figure under another name" % (other or "an empty list"))
    path = util.add_slash(a.path)
    train_opt = options.load_opt(path + "opt.txt")
    if train_opt.dataset != "MNIST":
        raise SystemExit("Downstream evaluation only implemented for MNIST.")
    if not train_opt.conditional:
        raise SystemExit("Downstream evaluation needs a conditional generator: the classifier is fitted on (G(z, y), y).")
    if a.num_samples < 1:
        raise SystemExit("-n must be positive")
    if a.device is not None:
        train_opt.g_device = a.device
    device = torch.device(train_opt.g_device)
    seed = int(train_opt.manual_seed) if a.seed is None else a.seed
    print("latent seed: %d   %d samples per checkpoint" % (seed, a.num_samples))

    test_bytes, test_labels = load_test_set(train_opt, a.test_cache)
    test_x = torch.from_numpy(test_bytes).to(device)
    test_y = torch.from_numpy(test_labels)
    G, _ = init_util.init_models(train_opt, init_D=False)

    results = {}
    with open(path + "downstream_log.csv", "a", newline="") as log:
        logger = csv.writer(log)
        logger.writerow(["Epoch"] + [c + " AUROC" for c in a.classifiers])
        log.flush()
        epoch = a.epoch_interval if a.epochs is None else a.epochs
        while os.path.isfile(path + "saves/G-" + str(epoch)):
            util.load_model(path + "saves/G-" + str(epoch), G, device=device)
            res = evaluate_checkpoint(G, train_opt, a, seed, device, test_x, test_y)
            print("lr AUROC ({}):  {}".format(epoch, res["micro"]))
            print("   per class: %s" % " ".join("%.4f" % v for v in res["per_class"]))
            print(classify.solver_line(res["solver"]))
            logger.writerow([epoch, res["micro"]])
            log.flush()
            results[epoch] = res
            if a.epochs is not None:
                break
            epoch += a.epoch_interval
    return results


if __name__ == "__main__":
    main(sys.argv[1:])
