"""Writes tests/golden/downstream_lr.npz and downstream_ties.npz: what scikit-learn's own classes compute for the estimator of the
reference's downstream.py (:71-72, :87, :48-62), on small synthetic data.  Needs scikit-learn (made with the version recorded in the
file); the tests read the fixtures and need only numpy.

    python tests/golden/make_downstream_golden.py

The estimator is built with the reference's arguments, except tol=1e-12 and a max_iter at which every column converges: the golden
is the minimiser, not the point where the default tol=1e-4 / max_iter=100 stops (recorded as auroc_micro_default_stop).  The script
asserts what the tests lean on and fails otherwise:
  * OneVsRest over the 'multinomial' form equals one binary logistic regression with C = 2 per class, to 1e-4 in probability;
  * the golden micro-AUROC lies in (0.85, 0.995): classes overlap, so a wrong fit moves the figure;
  * auroc_slack <= 0.01: the share of positive-negative pairs of P_gold closer than 2e-3, the only pairs whose order can change
    when every probability moves by at most 1e-3.
"""
import os
import warnings

import numpy as np
import sklearn
from sklearn.linear_model import LogisticRegression
from sklearn.metrics import auc, roc_curve
from sklearn.multiclass import OneVsRestClassifier
from sklearn.preprocessing import label_binarize

HERE = os.path.dirname(os.path.abspath(__file__))
N_TRAIN, N_TEST, D, K, N_ZERO = 600, 400, 64, 10, 6


def make_data():
    """K overlapping classes in [0, 1]^D: smooth class templates plus noise; 6 feature columns are zero everywhere (as the border
    pixels of MNIST are).  Test rows are bytes, as the idx file's."""
    rng = np.random.RandomState(20240607)
    templates = rng.rand(K, D)
    zero_cols = rng.choice(D, N_ZERO, replace=False)

    def draw(n, labels):
        x = 0.5 + 0.22 * (templates[labels] - 0.5) + 0.25 * rng.randn(n, D)
        x = np.clip(x, 0.0, 1.0)
        x[:, zero_cols] = 0.0
        return x

    y_train = np.concatenate([np.arange(K), rng.randint(0, K, N_TRAIN - K)])           # every class present
    rng.shuffle(y_train)
    y_test = rng.randint(0, K, N_TEST)
    x_train = draw(N_TRAIN, y_train).astype(np.float32)
    x_test = np.rint(draw(N_TEST, y_test) * 255.0).astype(np.uint8)
    return x_train, y_train.astype(np.int64), x_test, y_test.astype(np.int64), np.sort(zero_cols)


def reference_estimator(**over):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = dict(solver="lbfgs", multi_class="multinomial", random_state=30)
        kw.update(over)
        return OneVsRestClassifier(LogisticRegression(**kw))


def fit_proba(est, x_train, y_train, x_test):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return est.fit(x_train, y_train).predict_proba(x_test)


def aurocs(y_onehot, score):
    """compute_fpr_tpr_roc of the reference: auc(roc_curve(...)) on the ravelled matrices and per column."""
    fpr, tpr, _ = roc_curve(y_onehot.ravel(), score.ravel())
    per = []
    for k in range(score.shape[1]):
        f, t, _ = roc_curve(y_onehot[:, k], score[:, k])
        per.append(auc(f, t))
    return float(auc(fpr, tpr)), np.array(per)


def close_pair_share(pos, neg, gap):
    """Share of (positive, negative) pairs with |p - n| < gap."""
    sn = np.sort(neg)
    lo, hi = np.searchsorted(sn, pos - gap, side="right"), np.searchsorted(sn, pos + gap, side="left")
    return float((hi - lo).sum()) / (len(pos) * len(neg))


def main():
    x_train, y_train, x_test, y_test, zero_cols = make_data()
    xt = x_test.astype(np.float64) / 255.0
    hot = label_binarize(y_test, classes=list(range(K)))

    gold = reference_estimator(tol=1e-12, max_iter=20000)
    P = fit_proba(gold, x_train.astype(np.float64), y_train, xt)
    n_iter = [int(e.n_iter_[0]) for e in gold.estimators_]
    assert max(n_iter) < 20000, n_iter
    # 'multinomial' on a binary target: coef_ is the class-1 row of a symmetric two-class softmax, logit = 2 (x . coef_ + intercept_)
    U = np.stack([np.concatenate([2.0 * e.coef_[0], 2.0 * e.intercept_]) for e in gold.estimators_], axis=1)          # [D + 1, K]

    # the C = 2 equivalence
    S = np.zeros_like(P)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(K):
            b = LogisticRegression(solver="lbfgs", C=2.0, tol=1e-12, max_iter=20000).fit(x_train.astype(np.float64), (y_train == k).astype(int))
            S[:, k] = b.predict_proba(xt)[:, 1]
    P_c2 = S / S.sum(1, keepdims=True)
    c2_gap = float(np.abs(P_c2 - P).max())
    assert c2_gap <= 1e-4, c2_gap
    z = xt @ U[:D] + U[D]
    sg = 1.0 / (1.0 + np.exp(-z))
    coef_gap = float(np.abs(sg / sg.sum(1, keepdims=True) - P).max())
    assert coef_gap <= 1e-9, coef_gap

    P32 = P.astype(np.float32)
    micro, per = aurocs(hot, P32)
    assert 0.85 < micro < 0.995, micro
    P_def = fit_proba(reference_estimator(), x_train.astype(np.float64), y_train, xt)
    micro_def, _ = aurocs(hot, P_def.astype(np.float32))

    mask = hot.astype(bool)
    slack = close_pair_share(P[mask], P[~mask], 2e-3)
    slack_per = np.array([close_pair_share(P[mask[:, k], k], P[~mask[:, k], k], 2e-3) for k in range(K)])
    assert slack <= 0.01, slack

    np.savez_compressed(os.path.join(HERE, "downstream_lr.npz"), x_train=x_train, y_train=y_train, x_test=x_test, y_test=y_test,
                        zero_cols=zero_cols, P_gold=P, coef=U, n_iter=np.array(n_iter), auroc_micro=micro, auroc_per_class=per,
                        auroc_micro_default_stop=micro_def, default_stop_max_dp=float(np.abs(P_def - P).max()), auroc_slack=slack,
                        auroc_slack_per_class=slack_per, c2_gap=c2_gap, sklearn_version=sklearn.__version__)

    # scores with many exact ties: a coarse grid of float32 values
    rng = np.random.RandomState(7)
    y_t = rng.randint(0, 5, 300)
    raw = rng.rand(300, 5) + 0.6 * np.eye(5)[y_t]
    scores = (np.floor(raw * 8) / 8).astype(np.float32)
    hot_t = label_binarize(y_t, classes=list(range(5)))
    micro_t, per_t = aurocs(hot_t, scores)
    n_tied = int(300 * 5 - len(np.unique(scores)))
    assert n_tied > 1000
    np.savez_compressed(os.path.join(HERE, "downstream_ties.npz"), scores=scores, y=y_t.astype(np.int64), auroc_micro=micro_t,
                        auroc_per_class=per_t, sklearn_version=sklearn.__version__)
    for name in ("downstream_lr.npz", "downstream_ties.npz"):
        size = os.path.getsize(os.path.join(HERE, name))
        assert size < 256 * 1024, (name, size)
        print("%s: %d bytes" % (name, size))
    print("micro AUROC %.6f (default stop %.6f, max dP %.3f)  per class %s" % (micro, micro_def, float(np.abs(P_def - P).max()), np.round(per, 4)))
    print("iterations %s  C=2 gap %.2e  slack %.2e  per-class slack max %.2e" % (n_iter, c2_gap, slack, slack_per.max()))


if __name__ == "__main__":
    main()
