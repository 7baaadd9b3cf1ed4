"""Are the samples any use?  `python -m csl_gan_amd.tstr --syn_cache out/syn [more ...] --test_cache out/test
[--train_cache out/train --baseline] [-d cuda:0] [--gtol_rel G] [--max_iter 2000] [--values_dir DIR]
[--classifier {lr,mlp,gnb,bnb,dt,rf,ab} --hidden 100 --alpha 1.0 --seed 0 --var_smoothing 1e-9 --nb_alpha 0.01 --binarize 0
--n_trees 100 --max_features 0 --max_depth 0 --min_samples_split 2 --n_rounds 50 --learning_rate 1.0]
[--save --outputs_dir outputs/ --name tstr]`.

Train on synthetic, test on real: per labelled synthetic cache (what `gensamples --cache` of a conditional generator
wrote: images and the labels `index mod n_classes`) a one-vs-rest logistic regression (csl_gan_amd.classify.OvrLogReg.fit_bytes) is
fitted on the cache BYTES / 255 and scores the real test cache: micro and per-class AUROC (exact rank counts), accuracy with its
integer numerator, the solver's report.  K = 1 + the largest synthetic label.  The utility figure of `downstream`, for any dataset
whose rows are at most 65536 bytes — CelebA with `--label_attr Male` (K = 2) included.  --baseline fits on --train_cache instead and
reports it as `baseline_train`: the real-data line that puts the synthetic figures in context.  The test cache goes to the device
once, for all fits.  --values_dir keeps P (test probabilities) and U (coefficients, intercepts in the last row) per cache as .npy;
with --save the figures are merged into `<outputs_dir>/<name>.json`.  `-d cpu` runs the host model (float64), the definition the
device (fp32 kernels on the bytes) is held to.

--classifier mlp fits the reference's other classifier instead, a one-vs-rest MLP with --hidden ReLU units per class
and L2 penalty --alpha (csl_gan_amd.classify.OvrMlp, started from --seed; --max_iter then defaults to 200): the figures carry
"classifier", "hidden", "alpha" and "seed" as well, and U is kept in OvrMlp's layout [(D + 2) hidden + 1, K].

--classifier gnb / bnb fit the reference's two naive-Bayes classifiers (csl_gan_amd.classify.NaiveBayes): GaussianNB
with --var_smoothing, BernoulliNB with --nb_alpha on the features [byte > --binarize].  No solver: one pass over the training bytes
gives exact integer moments and the model follows in closed form, the same bits with -d cpu and on a device.  The figures carry
"classifier", "fit" (the class counts; eps for gnb) and the parameters used instead of "solver"; AUROC ranks the log-odds (the
posteriors saturate to exactly 0 and 1), accuracy is the argmax of the joint log-likelihood; --values_dir keeps P (float64
posteriors), J (the joint log-likelihood) and U (NaiveBayes.coef).  A flag of another classifier is ignored.

--classifier dt / rf fit the reference's two tree classifiers (csl_gan_amd.classify.Trees): per class a fully grown
decision tree, or a forest of --n_trees trees on bootstrap weights with about --max_features candidate features per node (0: sqrt of
the row size), both drawn from --seed; --max_depth (0: unlimited) and --min_samples_split bound the growth.  The splits are exact
integer histograms of the bytes: the trees, hence every figure, are the same bits with -d cpu and on a device.  The figures carry
"classifier", "fit" (class counts; nodes, leaves and depth per tree; levels) and the parameters; P is the mean leaf frequency over the
class's trees; --values_dir keeps P and U (the node tables, Trees.coef).

--classifier ab fits the reference's AdaBoost classifier (csl_gan_amd.classify.AdaBoost): per class up to --n_rounds
stumps, SAMME with --learning_rate, under fixed-point row weights, so every sum of a round is an exact integer and the stumps, hence
every figure, are the same bits with -d cpu and on a device.  The figures carry "classifier", "fit" (class counts; rounds kept, the sum
of the stump weights and the first round's error per class), "n_rounds" and "learning_rate"; P is 1 / (1 + exp(-2 F)) of the
normalised vote F; --values_dir keeps P and U (the stump table, AdaBoost.coef).

The panel's eighth classifier, the linear support-vector machine, has its own command over the same machinery: csl_gan_amd.tstr_svm
(DESIGN.md §6p), which calls `run` below with its own Estimator.
"""
import argparse
import collections
import sys

import numpy as np
import torch

from . import cache_cli, classify, pipeline
from .cache_cli import cache_rows  # noqa: F401  (scripts/tstr_bench.py and scripts/mlp_bench.py reach it as tstr.cache_rows)


def _proba_scores(clf, test_x):
    """(what AUROC ranks, what accuracy takes the argmax of, the values kept besides U) of an estimator with predict_proba_bytes.  Where P
    comes back on the host (dt, rf, ab) it is moved to the test rows' device for the ranks: on a device the rank counts are the device's."""
    P = clf.predict_proba_bytes(test_x)
    return P.to(test_x.device), P, {"P": P}


def _nb_scores(clf, test_x):
    """Naive Bayes: AUROC ranks the log-odds (the posteriors saturate to exactly 0 and 1), accuracy is the argmax of J."""
    J = clf.jll_bytes(test_x)
    return classify.log_odds(J).to(test_x.device), J, {"P": torch.softmax(J, 1), "J": J}


def _max_iter(a, default):
    return a.max_iter if a.max_iter is not None else default


def _trees(K, a):
    return classify.Trees(K, kind=a.classifier, n_trees=a.n_trees, max_features=a.max_features or None, max_depth=a.max_depth,
                          min_samples_split=a.min_samples_split, seed=a.seed)


def _tree_stats(clf, a, rep, D):
    return {"classifier": a.classifier, "fit": rep, "max_depth": clf.max_depth, "min_samples_split": clf.min_samples_split}


def _nb_line(m):
    return "   fit: rows per class %s%s" % (m["fit"]["n_per_class"], "  eps %.6g" % m["fit"]["eps"] if "eps" in m["fit"] else "")


def _tree_line(m):
    f = m["fit"]
    return "   fit: rows per class %s  trees %d  nodes %d  leaves %d  depth <= %d  levels %d" % (
        f["n_per_class"], len(f["nodes"]), sum(f["nodes"]), sum(f["leaves"]), max(f["depth"]), f["levels"])


# One entry per --classifier choice.  build(K, a): the estimator of csl_gan_amd.classify from the parsed arguments a (fit_bytes(X, y)
# returns its report); scores(clf, test_x): see _proba_scores; stats(clf, a, report, D): the keys the figures carry besides the scores,
# the report among them, in the order they are written; fit_line(figures): the line printed under the scores.  DESIGN.md §6o.
Estimator = collections.namedtuple("Estimator", "build scores stats fit_line")
ESTIMATORS = {
    "lr": Estimator(lambda K, a: classify.OvrLogReg(K, gtol_rel=a.gtol_rel, max_iter=_max_iter(a, 2000)), _proba_scores,
                    lambda clf, a, rep, D: {"solver": rep}, lambda m: classify.solver_line(m["solver"])),
    "mlp": Estimator(lambda K, a: classify.OvrMlp(K, gtol_rel=a.gtol_rel, max_iter=_max_iter(a, 200), hidden=a.hidden, alpha=a.alpha, seed=a.seed),
                     _proba_scores,
                     lambda clf, a, rep, D: {"solver": rep, "classifier": "mlp", "hidden": int(a.hidden), "alpha": float(a.alpha), "seed": int(a.seed)},
                     lambda m: classify.solver_line(m["solver"])),
    "gnb": Estimator(lambda K, a: classify.NaiveBayes(K, kind="gnb", var_smoothing=a.var_smoothing), _nb_scores,
                     lambda clf, a, rep, D: {"classifier": "gnb", "fit": rep, "var_smoothing": a.var_smoothing}, _nb_line),
    "bnb": Estimator(lambda K, a: classify.NaiveBayes(K, kind="bnb", alpha=a.nb_alpha, binarize=a.binarize), _nb_scores,
                     lambda clf, a, rep, D: {"classifier": "bnb", "fit": rep, "alpha": a.nb_alpha, "binarize": a.binarize}, _nb_line),
    "dt": Estimator(_trees, _proba_scores, _tree_stats, _tree_line),
    "rf": Estimator(_trees, _proba_scores,
                    lambda clf, a, rep, D: dict(_tree_stats(clf, a, rep, D), n_trees=clf.B, max_features=clf.max_features or max(1, int(np.sqrt(D))),
                                                seed=clf.seed), _tree_line),
    "ab": Estimator(lambda K, a: classify.AdaBoost(K, n_rounds=a.n_rounds, learning_rate=a.learning_rate), _proba_scores,
                    lambda clf, a, rep, D: {"classifier": "ab", "fit": rep, "n_rounds": clf.n_rounds, "learning_rate": clf.learning_rate},
                    lambda m: "   fit: rows per class %s  rounds per class %s  stumps %d" % (
                        m["fit"]["n_per_class"], m["fit"]["rounds"], sum(m["fit"]["rounds"]))),
}


def add_cache_arguments(ap, name):
    """The arguments of every train-on-synthetic command line (this one and csl_gan_amd.tstr_svm): the common ones under the tool's `name`,
    --test_cache, --train_cache and --baseline."""
    cache_cli.add_common_arguments(ap, name, "labelled uint8 image cache(s) of synthetic samples",
                                   "keep the test probabilities and the coefficients as .npy here")
    ap.add_argument("--test_cache", type=str, required=True, help="labelled uint8 image cache of real test images")
    ap.add_argument("--train_cache", type=str, default=None, help="labelled uint8 image cache of the training set (for --baseline)")
    ap.add_argument("--baseline", default=False, action="store_true", help="also fit on the training set itself")


def check_cache_arguments(a):
    if a.baseline and not a.train_cache:
        raise SystemExit("--baseline fits on the training set: give --train_cache")


def build_parser():
    ap = argparse.ArgumentParser(description="Train-on-synthetic, test-on-real classifier utility of labelled image caches")
    add_cache_arguments(ap, "tstr")
    ap.add_argument("--gtol_rel", type=float, default=None, help="a class has converged when max|gradient| <= gtol_rel * n")
    ap.add_argument("--max_iter", type=int, default=None, help="L-BFGS iterations per class (default: 2000 for lr, 200 for mlp)")
    ap.add_argument("--classifier", type=str, default="lr", choices=list(ESTIMATORS),
                    help="one-vs-rest logistic regression or MLP, Gaussian or Bernoulli naive Bayes, decision tree or random forest, AdaBoost of stumps")
    ap.add_argument("--hidden", type=int, default=100, help="mlp: hidden ReLU units per class, 1 .. %d" % classify.MAX_HIDDEN)
    ap.add_argument("--alpha", type=float, default=1.0, help="mlp: L2 penalty on the weights, >= 0")
    ap.add_argument("--seed", type=int, default=0, help="mlp: seed of the initial point; rf: seed of the bootstrap draws and feature masks")
    ap.add_argument("--var_smoothing", type=float, default=1e-9, help="gnb: share of the largest feature variance added to every variance, >= 0")
    ap.add_argument("--nb_alpha", type=float, default=0.01, help="bnb: additive smoothing of the counts, > 0")
    ap.add_argument("--binarize", type=int, default=0, help="bnb: the feature is [byte > binarize], 0 .. 254")
    ap.add_argument("--n_trees", type=int, default=100, help="rf: trees per class, 1 .. 4095")
    ap.add_argument("--max_features", type=int, default=0, help="rf: expected number of candidate features per node (0: sqrt of the row size)")
    ap.add_argument("--max_depth", type=int, default=0, help="dt, rf: depth at which every node is a leaf (0: unlimited)")
    ap.add_argument("--min_samples_split", type=int, default=2, help="dt, rf: a node of fewer (weighted) rows is a leaf, >= 2")
    ap.add_argument("--n_rounds", type=int, default=50, help="ab: boosting rounds (stumps) per class, 1 .. %d" % classify.BOOST_MAX_ROUNDS)
    ap.add_argument("--learning_rate", type=float, default=1.0, help="ab: the factor on every stump's weight, > 0")
    return ap


def n_classes_of(labels, path):
    """K = 1 + the largest label, refused outside 2 .. 16 and when a class of 0 .. K-1 has no row."""
    if len(labels) < 1 or int(labels.min()) < 0:
        raise SystemExit("%s: needs rows with labels >= 0" % path)
    K = 1 + int(labels.max())
    if not 2 <= K <= classify.MAX_CLASSES:
        raise SystemExit("%s: labels 0 .. %d give K = %d classes; the classifier takes 2 .. %d (an unconditional generator leaves an "
                         "unlabelled or single-class cache: train one with -cond)" % (path, K - 1, K, classify.MAX_CLASSES))
    counts = np.bincount(labels, minlength=K)
    if (counts == 0).any():
        raise SystemExit("%s: every class 0 .. %d needs a row; counts: %s" % (path, K - 1, counts.tolist()))
    return K


def fit_and_score(est, a, train_x, train_y, K, test_x, test_y, device):
    """One fit of the estimator est (an entry of ESTIMATORS, built from the parsed arguments a) on bytes train_x [n, D] (numpy) and its
    figures on test_x (a uint8 tensor already on `device`): (stats, values), values the arrays --values_dir keeps ("P", "U"; "J" as
    well for naive Bayes).  The parameters are part of the stats."""
    stats = {"n_train": int(len(train_y)), "n_test": int(len(test_y)), "classes": int(K)}
    clf = est.build(K, a)
    report = clf.fit_bytes(torch.from_numpy(train_x).to(device), torch.from_numpy(train_y))
    rank, top, values = est.scores(clf, test_x)
    au, acc = classify.auroc(rank, test_y), classify.accuracy(top, test_y)
    stats.update({"auroc_micro": au["micro"], "auroc_per_class": au["per_class"], "accuracy": acc["accuracy"], "accuracy_hits": acc["hits"]})
    stats.update(est.stats(clf, a, report, train_x.shape[1]))
    return stats, {k: v.cpu().numpy() for k, v in dict(values, U=clf.coef).items()}


def main(argv=None):
    a = build_parser().parse_args(argv)
    check_cache_arguments(a)
    inf = float("inf")
    for flag, ok, msg in (          # every flag is checked whichever classifier is chosen; only --seed is the trees' alone
            ("hidden", 1 <= a.hidden <= classify.MAX_HIDDEN, "--hidden %%d: the MLP takes 1 .. %d hidden units per class" % classify.MAX_HIDDEN),
            ("alpha", 0 <= a.alpha < inf, "--alpha %r: the penalty must be a finite number >= 0"),
            ("var_smoothing", 0 <= a.var_smoothing < inf, "--var_smoothing %r: must be a finite number >= 0"),
            ("nb_alpha", 0 < a.nb_alpha < inf, "--nb_alpha %r: the smoothing must be a finite number > 0"),
            ("binarize", 0 <= a.binarize <= 254, "--binarize %d: a byte threshold, 0 .. 254"),
            ("n_trees", 1 <= a.n_trees <= 4095, "--n_trees %d: a forest takes 1 .. 4095 trees per class"),
            ("max_features", a.max_features >= 0, "--max_features %d: the expected number of candidate features, >= 1 (0: sqrt of the row size)"),
            ("max_depth", a.max_depth >= 0, "--max_depth %d: must be >= 0 (0: unlimited)"),
            ("min_samples_split", a.min_samples_split >= 2, "--min_samples_split %d: must be >= 2"),
            ("seed", a.classifier not in ("dt", "rf") or 0 <= a.seed < 2 ** 63, "--seed %d: the trees take 0 .. 2^63 - 1"),
            ("n_rounds", 1 <= a.n_rounds <= classify.BOOST_MAX_ROUNDS, "--n_rounds %%d: boosting takes 1 .. %d rounds per class" % classify.BOOST_MAX_ROUNDS),
            ("learning_rate", 0 < a.learning_rate < inf, "--learning_rate %r: must be a finite number > 0")):
        if not ok:
            raise SystemExit(msg % getattr(a, flag))
    return run(a, ESTIMATORS[a.classifier])


def run(a, est, check_set=None):
    """What a train-on-synthetic command line does once its arguments are parsed and checked: open and check the caches, fit the estimator
    `est` (an Estimator) on every set, score the test cache, print, keep the values and report the figures.  check_set(labels, K, path):
    the estimator's own refusals of a training set, raised before the first fit."""
    test = pipeline.CachedImages(a.test_cache)
    extra = [("baseline_train", a.train_cache, pipeline.CachedImages(a.train_cache))] if a.baseline else []
    sets = cache_cli.open_syn_caches(a.syn_cache, test, a.test_cache, [(p, c) for _, p, c in extra]) + extra
    D = test.H * test.W * test.C
    if not 1 <= D <= 65536:
        raise SystemExit("%s: rows of %d bytes; the classifier takes 1 .. 65536" % (a.test_cache, D))
    test_bytes, test_y = cache_rows(test)
    if len(test_y) < 1:
        raise SystemExit("%s holds no image" % a.test_cache)
    classes = {}
    for lab, p, c in sets:
        K = classes[lab] = n_classes_of(np.asarray(c.labels, dtype=np.int64).reshape(-1), p)
        if int(test_y.min()) < 0 or int(test_y.max()) >= K:
            raise SystemExit("%s: test labels span %d .. %d; %s has the classes 0 .. %d" % (a.test_cache, int(test_y.min()), int(test_y.max()), p, K - 1))
        if check_set is not None:
            check_set(np.asarray(c.labels, dtype=np.int64).reshape(-1), K, p)

    device = torch.device(a.device)
    test_x = torch.from_numpy(test_bytes).to(device)       # once, for all fits
    test_yt = torch.from_numpy(test_y)
    stats, values = {}, {}
    for lab, _, c in sets:
        x, y = cache_rows(c)
        m, vals = fit_and_score(est, a, x, y, classes[lab], test_x, test_yt, device)
        stats[lab] = m
        values.update({lab + "_" + k: v for k, v in vals.items()})
        print("%s: fitted on %d rows, scored %d: AUROC %.6f, accuracy %.4f (%d / %d)" % (
            lab, m["n_train"], m["n_test"], m["auroc_micro"], m["accuracy"], m["accuracy_hits"], m["n_test"]))
        print("   per class: %s" % " ".join("%.4f" % v for v in m["auroc_per_class"]))
        print(est.fit_line(m))
    cache_cli.save_values(a.values_dir, values)
    return cache_cli.report(a, stats)


if __name__ == "__main__":
    main(sys.argv[1:])
