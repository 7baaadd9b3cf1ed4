"""Membership-inference audit of a saved critic: `python -m csl_gan_amd.mem_inf_attack RUN --train_cache A --nontrain_cache B
[--checkpoints E ...] [-bs 1000] [-d cuda:0]` — the reference's mem_inf_attack.py (the white-box attack of Hayes et al.: score the
training set and a held-out set with D, and measure how often the best-scored images are training images).

Reads `RUN/opt.txt`, builds only D on the requested device, and per checkpoint E loads `RUN/saves/D-<E>` with the no-code loader,
scores both caches with csl_gan_amd.audit.CriticScorer and prints / saves csl_gan_amd.audit.attack_metrics: asr (the reference's
figure, mem_inf_attack.py:29-59, :347-350), its standard error, auc, and the TPR at 1 % and 0.1 % FPR.  Flags and defaults of
mem_inf_attack.py:170-217 are kept for --asr_iters, --batch_size, --data_prop, --checkpoints, --checkpoint_min/_max/_step,
--outputs_dir, --values_dir and --save; --pool, --seed, --hip_graph and --compute_dtype are additions.  The attack values of a
checkpoint are kept as `<values_dir>/<run>/checkpoint-<E>/attack_values_{train,nontrain}.npy` and reused when present (the
reference's commented-out behaviour, :319-344); with --save the figures are merged into `<outputs_dir>/<run>.json` and checkpoints
already there are skipped (:300-309).

Deliberate differences from the reference:
  * FID is not built (--compute_fid, --fid_dir, --real_samples_dir): it needs Inception weights, which no machine of this project has;
  * --generate_samples / --num_generated_samples / --samples_dir are `python -m csl_gan_amd.gensamples`' job;
  * the data come from uint8 caches (what `train --data_cache` or `gensamples --cache` wrote) instead of init_data: the audit scores
    exactly the rows of the two files, in index order, so --data_dir, --labels_dir, --public_set_size and --train_set_size are gone,
    and RUN is a path, not --model_dir + --model_name;
  * the figures are exact functions of (score arrays, seed, pool, data_prop, asr_iters): the subsets come from an indexed Philox
    stream (include/cslgan.h "Audit sampler"), not from the process RNG, so a rerun, another device or another split of the trials
    prints the same numbers.  The reference's own estimate is a different draw of the same estimator.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import audit, init_util, options, pipeline, util


def build_parser():
    ap = argparse.ArgumentParser(description="Membership-inference audit of a saved critic")
    ap.add_argument("path", type=str, help="Path to the output folder of the training run (opt.txt, saves/D-<E>)")
    ap.add_argument("--train_cache", type=str, required=True, help="uint8 image cache of the training set")
    ap.add_argument("--nontrain_cache", type=str, required=True, help="uint8 image cache of the held-out set")
    ap.add_argument("--asr_iters", type=int, default=10000, help="subset pairs drawn for the attack success rate")
    ap.add_argument("-bs", "--batch_size", type=int, default=1000, help="batch size of the critic")
    ap.add_argument("--data_prop", type=float, default=0.1, help="share of training data in the adversary's pool")
    ap.add_argument("--checkpoint_max", type=int, default=None)
    ap.add_argument("--checkpoint_min", type=int, default=None)
    ap.add_argument("--checkpoint_step", type=int, default=None)
    ap.add_argument("--checkpoints", type=int, nargs="+", default=None, help="epochs of the D saves to audit")
    ap.add_argument("--outputs_dir", type=str, default="outputs/")
    ap.add_argument("--values_dir", type=str, default="values/")
    ap.add_argument("--save", default=False, action="store_true", help="merge the figures into <outputs_dir>/<run>.json")
    ap.add_argument("-d", "--device", type=str, default="cpu")
    # ---- additions of this build ----
    ap.add_argument("--pool", type=int, default=1000, help="size of the adversary's pool (the reference's literal 1000)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the subset stream (default: the run's manual_seed)")
    ap.add_argument("--hip_graph", type=options.str2bool, default=True, help="record full batches in a HIP graph (device runs)")
    ap.add_argument("--compute_dtype", type=str, choices=["fp32", "bf16", "bf16x3", "fp32_auto"], default=None,
                    help="arithmetic of the conv kernels (default: the training run's)")
    return ap


def _values(path, scorer, cache, what):
    if os.path.exists(path):
        v = np.load(path)
        if v.shape != (len(cache),):
            raise SystemExit("%s holds %s values, the cache %d rows" % (path, v.shape, len(cache)))
        print("%d %s attack values loaded from %s" % (len(v), what, path))
        return v.astype(np.float32)
    v = scorer.score(cache)
    np.save(path, v)
    print("%d %s attack values computed and saved to %s" % (len(v), what, path))
    return v


def main(argv=None):
    a = build_parser().parse_args(argv)
    path = util.add_slash(a.path)
    run = os.path.basename(os.path.normpath(path))
    if None not in (a.checkpoint_max, a.checkpoint_min, a.checkpoint_step) and a.checkpoint_max > a.checkpoint_min > 0:
        a.checkpoints = list(range(a.checkpoint_min, a.checkpoint_max + a.checkpoint_step, a.checkpoint_step))      # mem_inf_attack.py:221-223
    if not a.checkpoints:
        raise SystemExit("give --checkpoints, or --checkpoint_min/_max/_step")
    for e in a.checkpoints:
        if not os.path.exists(path + "saves/D-%d" % e):
            raise SystemExit("D-%d is not in %ssaves/" % (e, path))
    train_opt = options.load_opt(path + "opt.txt")
    seed = int(train_opt.manual_seed) if a.seed is None else a.seed
    print("subset seed: %d   pool %d   data_prop %g   asr_iters %d" % (seed, a.pool, a.data_prop, a.asr_iters))
    train, nontrain = pipeline.CachedImages(a.train_cache), pipeline.CachedImages(a.nontrain_cache)

    json_path = os.path.join(a.outputs_dir, run + ".json")
    stats = {}
    if os.path.exists(json_path):
        with open(json_path) as f:
            stats = json.load(f)
    todo = [e for e in a.checkpoints if str(e) not in stats]

    if todo:
        train_opt.d_device = a.device
        _, D = init_util.init_models(train_opt, init_G=False)
        scorer = audit.CriticScorer(D, train_opt, a.device, a.batch_size, hip_graph=a.hip_graph, compute_dtype=a.compute_dtype)
        try:
            for e in todo:
                util.load_model(path + "saves/D-%d" % e, D, device=a.device)
                scorer.weights_changed()
                vdir = os.path.join(a.values_dir, run, "checkpoint-%d" % e)
                os.makedirs(vdir, exist_ok=True)
                vt = _values(os.path.join(vdir, "attack_values_train.npy"), scorer, train, "training")
                vn = _values(os.path.join(vdir, "attack_values_nontrain.npy"), scorer, nontrain, "non-training")
                stats[str(e)] = audit.attack_metrics(vt, vn, a.data_prop, a.pool, a.asr_iters, seed, a.device)
                print("ASR on %s-%d: %.2f%% (+- %.2f%%)   AUC %.4f" % (run, e, 100 * stats[str(e)]["asr"], 100 * stats[str(e)]["asr_stderr"],
                                                                       stats[str(e)]["auc"]))
        finally:
            scorer.release()
    print(json.dumps(stats, indent=4))
    if a.save:
        os.makedirs(a.outputs_dir, exist_ok=True)
        with open(json_path, "w") as f:
            json.dump(stats, f)
        print("saved %s" % json_path)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
