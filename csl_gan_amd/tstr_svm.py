"""The support-vector line of the classifier panel: `python -m csl_gan_amd.tstr_svm --syn_cache out/syn [more ...] --test_cache out/test
[--train_cache out/train --baseline] [-d cuda:0] [--C 1.0] [--tol 1e-3] [--folds 5] [--seed 0] [--svm_max_iter N] [--values_dir DIR]
[--save --outputs_dir outputs/ --name tstr_svm]`.

Train on synthetic, test on real with `OneVsRestClassifier(SVC(kernel='linear', probability=True))` of the reference's downstream.py:67
(csl_gan_amd.svm.OvrSvc): the caches, the refusals, the printed lines and the score keys of csl_gan_amd.tstr, whose
machinery this command runs (tstr.run).  Per class the dual problem is solved by SMO at penalty --C to the gap --tol, and --folds further
problems on the same rows give the held-out decision values of Platt's sigmoid; the fold assignment follows --seed.  The solve is the same
bits with -d cpu and on a device, so the reports agree exactly.  The figures carry "classifier": "svm", "fit" (per class the iterations,
convergence, support vectors, rho, A and B; the iteration total of all problems), "C", "tol", "folds" and "seed"; --values_dir keeps P and U
(OvrSvc.coef, the sigmoids as a logistic model).  Two refusals of its own: a training set above 65536 rows (the kernel matrix is stored:
16 GiB there), and a class with fewer than 2 rows on either side.  A problem that reaches --svm_max_iter is reported "converged": false.
"""
import argparse
import sys

import numpy as np

from . import svm, tstr

ESTIMATOR = tstr.Estimator(
    lambda K, a: svm.OvrSvc(K, C=a.C, tol=a.tol, folds=a.folds, seed=a.seed, max_iter=a.svm_max_iter), tstr._proba_scores,
    lambda clf, a, rep, D: {"classifier": "svm", "fit": rep, "C": clf.C, "tol": clf.tol, "folds": clf.folds, "seed": clf.seed},
    lambda m: "   fit: rows per class %s  iterations %s (all problems %d)  support vectors %s  at the bound %s  converged %s" % (
        m["fit"]["n_per_class"], m["fit"]["iterations"], m["fit"]["iterations_total"], m["fit"]["n_sv"], m["fit"]["n_bsv"],
        "all" if all(m["fit"]["converged"]) else m["fit"]["converged"]))


def build_parser():
    ap = argparse.ArgumentParser(description="Train-on-synthetic, test-on-real utility of labelled image caches under a linear support-vector classifier")
    tstr.add_cache_arguments(ap, "tstr_svm")
    ap.add_argument("--C", type=float, default=1.0, help="the penalty of the dual's box, > 0")
    ap.add_argument("--tol", type=float, default=1e-3, help="a problem has converged when m(alpha) - M(alpha) < tol")
    ap.add_argument("--folds", type=int, default=5, help="folds of the held-out decision values behind Platt's sigmoid, >= 2")
    ap.add_argument("--seed", type=int, default=0, help="seed of the fold assignment")
    ap.add_argument("--svm_max_iter", type=int, default=10_000_000, help="SMO iterations per problem; a problem that gets there is reported unconverged")
    return ap


def check_set(labels, K, path, folds=5):
    """What the support-vector fit refuses beyond tstr's own rules."""
    if K * (1 + folds) > svm.MAX_PROBLEMS:
        raise SystemExit("%s: %d classes x (1 + %d folds) problems; one solve takes %d" % (path, K, folds, svm.MAX_PROBLEMS))
    if len(labels) > svm.MAX_ROWS:
        raise SystemExit("%s: %d rows; the stored kernel matrix takes at most %d (16 GiB): a larger set needs shrinking and a kernel-row cache"
                         % (path, len(labels), svm.MAX_ROWS))
    counts = np.bincount(labels, minlength=K)
    if (counts < 2).any() or (len(labels) - counts < 2).any():
        raise SystemExit("%s: every class needs at least 2 rows and 2 rows outside it (the folds of Platt's sigmoid); counts: %s" % (path, counts.tolist()))


def main(argv=None):
    a = build_parser().parse_args(argv)
    tstr.check_cache_arguments(a)
    inf = float("inf")
    for flag, ok, msg in (("C", 0 < a.C < inf, "--C %r: the penalty must be a finite number > 0"),
                          ("tol", 0 < a.tol < inf, "--tol %r: must be a finite number > 0"),
                          ("folds", 2 <= a.folds <= svm.MAX_PROBLEMS // 2 - 1, "--folds %%d: Platt's sigmoid takes 2 .. %d folds" % (svm.MAX_PROBLEMS // 2 - 1)),
                          ("seed", 0 <= a.seed < 2 ** 63, "--seed %d: the fold assignment takes 0 .. 2^63 - 1"),
                          ("svm_max_iter", a.svm_max_iter >= 0, "--svm_max_iter %d: must be >= 0")):
        if not ok:
            raise SystemExit(msg % getattr(a, flag))
    return tstr.run(a, ESTIMATOR, lambda labels, K, path: check_set(labels, K, path, a.folds))


if __name__ == "__main__":
    main(sys.argv[1:])
