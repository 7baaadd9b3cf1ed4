"""The device path of csl_gan_amd.classify.NaiveBayes (-m gpu): cslgan_class_moments_u8 against the host model integer
for integer, cslgan_nb_score_gauss_u8 / _bern_u8 against float64 numpy on the same float32 tables within the bound of the header, the
device fit and scores against the host's on the three problems of tests/test_tstr.py, and the command line on cuda:0 against -d cpu."""
import functools
import os

import numpy as np
import pytest
import torch

from test_tstr import PROBLEMS, make, make_caches
from test_tstr_gpu import _close_pair_share, _problem

pytestmark = pytest.mark.gpu

# the smallest of each | D below one 16-byte load, ragged rows | rows not 16-byte aligned, D no multiple of 4 | a slab plus a remainder |
# CelebA's row | the largest D, all 16 classes
SHAPES = [(1, 1, 2), (17, 5, 3), (257, 930, 10), (300, 1040, 2), (100, 12288, 2), (20, 65536, 16)]
WRAP = (70000, 8, 2)                # every byte of class 0 is 255: a 32-bit sum of squares would wrap at 66 052 rows
MANY_ROWS = (65637, 12, 3)          # 1026 row tiles of the score kernels, the last one ragged
OUTSIDE = (257, 930, 10)            # the shape that also runs with labels in -2 .. K + 1
BOUND = 2e-5                        # |S_dev - S_host| <= BOUND * T: (275 + 3) 2^-24 = 1.66e-5 (include/cslgan.h "naive Bayes")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the moments --------------------------------------------------------------------------------------------------------------------------

def _check_moments(X, y, K, binarize):
    from csl_gan_amd import classify, ops
    N, D = X.shape
    ref = classify.class_moments_host_bytes(X, y, K, binarize)
    dX, dy = _dev(X), _dev(y.astype(np.int32))
    out = {"n": torch.full((K,), -1, dtype=torch.int64, device="cuda")}
    out.update({k: torch.full((K, D), -1, dtype=torch.int64, device="cuda") for k in ("s1", "s2", "cnt")})
    got = ops.class_moments_u8(dX, dy, K, binarize, out=out)
    again = ops.class_moments_u8(dX, dy, K, binarize)
    for name in ("n", "s1", "s2", "cnt"):
        assert got[name] is out[name] and got[name].dtype == torch.int64
        assert np.array_equal(got[name].cpu().numpy(), ref[name].numpy()), name
        assert torch.equal(again[name], got[name]), name
    return ref


@pytest.mark.parametrize("binarize", [0, 127])
@pytest.mark.parametrize("N,D,K", SHAPES)
def test_moments_equal_the_host_model(N, D, K, binarize):
    """np.array_equal on all four tables; the outputs are handed over filled with -1; a second call returns equal integers."""
    X, y, _ = _problem(N, D, K, False)
    _check_moments(X, y, K, binarize)


def test_moments_with_labels_outside_the_classes():
    X, y, _ = _problem(*OUTSIDE, False, True)
    assert (y < 0).any() and (y >= OUTSIDE[2]).any()
    ref = _check_moments(X, y, OUTSIDE[2], 254)
    assert int(ref["n"].sum()) < OUTSIDE[0]


def test_moments_do_not_wrap_32_bits():
    """70 000 rows of 8 bytes, ~68 000 of them in class 0 and all 255: sum b^2 = 65025 n_0 > 2^32."""
    N, D, K = WRAP
    rng = np.random.default_rng(7)
    y = (rng.random(N) < 0.03).astype(np.int64)
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    X[y == 0] = 255
    ref = _check_moments(X, y, K, 0)
    assert int(ref["n"][0]) > 66051 and int(ref["s2"][0, 0]) == 65025 * int(ref["n"][0]) > 2 ** 32


# ---- the scores ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tables(D, K):
    """m uniform in [0, 255], w log-uniform over 1e-5 .. 1e-1 with one column at 1e9 (the dead pixel of var_smoothing), delta normal
    with scale 3; float32."""
    rng = np.random.default_rng(100 * D + K)
    m = rng.uniform(0, 255, (K, D)).astype(np.float32)
    w = np.exp(rng.uniform(np.log(1e-5), np.log(1e-1), (K, D))).astype(np.float32)
    w[:, D // 2] = 1e9
    delta = (3.0 * rng.standard_normal((K, D))).astype(np.float32)
    return m, w, delta


def _check_scores(name, got, again, S, T):
    got, again = got.cpu().numpy(), again.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == S.shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - S)
    ratio = float((err[T > 0] / T[T > 0]).max()) if (T > 0).any() else 0.0
    print("%s: max |S_dev - S_host| / T = %.3g" % (name, ratio))
    assert (err <= BOUND * T).all()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("N,D,K", SHAPES + [MANY_ROWS])
def test_scores_within_the_bound_of_the_float64_sums(N, D, K):
    """|S_dev - S_host| <= 2e-5 T per entry, S_host and T in float64 numpy on the same float32 tables (gauss: T = S; bern, at binarize 0
    and 127: T = sum of the |delta| that count).  S is handed over full of NaN; a second call returns the same bits.  Measured on an MI355X: the
    largest ratio to T is 2.3e-6, gauss at (20, 65536, 16), where the w = 1e9 column holds all of T and 128 slab partials are added
    after it; elsewhere 1e-8 .. 4.4e-7 for gauss and at most 1.2e-7 for bern."""
    from csl_gan_amd import ops
    X, _, _ = _problem(N, D, K, False)
    m, w, delta = _tables(D, K)
    dX = _dev(X)
    nan = lambda: torch.full((N, K), float("nan"), device="cuda")
    Xd = X.astype(np.float64)
    S = np.stack([(w[k].astype(np.float64) * (Xd - m[k].astype(np.float64)) ** 2).sum(1) for k in range(K)], 1)
    dm, dw, dd = _dev(m), _dev(w), _dev(delta)
    out = nan()
    got = ops.nb_score_gauss_u8(dX, dm, dw, out=out)
    assert got is out
    _check_scores("gauss (%d, %d, %d)" % (N, D, K), got, ops.nb_score_gauss_u8(dX, dm, dw), S, S)
    for thr in (0, 127):
        F = (X > thr).astype(np.float64)
        S, T = F @ delta.astype(np.float64).T, F @ np.abs(delta).astype(np.float64).T
        got = ops.nb_score_bern_u8(dX, dd, thr, out=nan())
        _check_scores("bern binarize %d (%d, %d, %d)" % (thr, N, D, K), got, ops.nb_score_bern_u8(dX, dd, thr), S, T)


@pytest.mark.parametrize("D", [300, 304])
def test_scores_for_every_class_count(D):
    """K = 2 .. 16 at (70, D): the score kernels are compiled per class count (a K without its own build runs the next larger one with
    classes of zeros), for rows that are 16-byte aligned (304) and rows that are not (300).  The same bound."""
    from csl_gan_amd import ops
    X, _, _ = _problem(70, D, 2, False)
    dX, Xd = _dev(X), X.astype(np.float64)
    F = (X > 127).astype(np.float64)
    for K in range(2, 17):
        m, w, delta = _tables(D, K)
        S = np.stack([(w[k].astype(np.float64) * (Xd - m[k].astype(np.float64)) ** 2).sum(1) for k in range(K)], 1)
        dm, dw, dd = _dev(m), _dev(w), _dev(delta)
        _check_scores("gauss (70, %d, %d)" % (D, K), ops.nb_score_gauss_u8(dX, dm, dw), ops.nb_score_gauss_u8(dX, dm, dw), S, S)
        _check_scores("bern (70, %d, %d)" % (D, K), ops.nb_score_bern_u8(dX, dd, 127), ops.nb_score_bern_u8(dX, dd, 127),
                      F @ delta.astype(np.float64).T, F @ np.abs(delta).astype(np.float64).T)


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------

def _sum_of_absolute_terms(clf, xt):
    """T [M, K] of a fitted estimator in float64: gnb the score sum itself, bnb the sum of the |delta| that count."""
    if clf.kind == "gnb":
        m, w = (t.astype(np.float64) for t in clf.tables)
        Xd = xt.astype(np.float64)
        return np.stack([(w[k] * (Xd - m[k]) ** 2).sum(1) for k in range(clf.K)], 1)
    return (xt > clf.binarize).astype(np.float64) @ np.abs(clf.tables[0]).astype(np.float64).T


def _agree_nb(name, Jh, Jd, T, yt, K, auc_h, auc_d, hits_h, hits_d):
    """The slacks of DESIGN.md §6l, all from the HOST's scores: jll within 2e-5 T per entry; hit counts within the number of close
    rows (two largest host jll nearer than 2 * 2e-5 max_k T), which stays below 2 % of the rows; micro-AUROC within the share of
    positive-negative pairs of the host log-odds closer than 2 E, E = 2 * 2e-5 max T, which stays below 1e-3."""
    from csl_gan_amd import classify
    err = np.abs(Jh - Jd)
    assert (err <= BOUND * T).all()
    top = np.sort(Jh, 1)
    close = int((top[:, -1] - top[:, -2] < 2 * BOUND * T.max(1)).sum())
    E = 2 * BOUND * float(T.max())
    L = classify.log_odds(Jh).numpy()
    hot = yt[:, None] == np.arange(K)[None]
    slack = _close_pair_share(L[hot], L[~hot], 2 * E)
    print("%s: max |J_dev - J_host| / T = %.3g  AUROC host %.6f dev %.6f (slack %.3g)  hits host %d dev %d (close rows %d of %d)" % (
        name, float((err[T > 0] / T[T > 0]).max()), auc_h, auc_d, slack, hits_h, hits_d, close, len(yt)))
    assert close < 0.02 * len(yt) and abs(hits_h - hits_d) <= close
    assert slack < 1e-3 and abs(auc_h - auc_d) <= slack


@pytest.mark.parametrize("kind,kw", [("gnb", {}), ("bnb", {"binarize": 127})])
@pytest.mark.parametrize("i", range(len(PROBLEMS)))
def test_device_fit_and_scores_equal_the_host(i, kind, kw):
    """The tables are bit-equal (exact moments, one derivation); jll, accuracy and AUROC within the slacks of _agree_nb; a second
    device fit and score return the same bits.  Measured on an MI355X: jll within 1.7e-7 T, equal hit counts (544 / 371 / 190), no close
    row, AUROCs within 1e-6 under slacks of 5e-5 .. 3e-4."""
    from csl_gan_amd import classify
    N, H, W, C, K, M = PROBLEMS[i]
    x, y = make(N, H, W, C, K, 1)
    xt, yt = make(M, H, W, C, K, 2)
    host, dev = classify.NaiveBayes(K, kind, **kw), classify.NaiveBayes(K, kind, **kw)
    rep_h, rep_d = host.fit_bytes(x, y), dev.fit_bytes(_dev(x), _dev(y))
    assert rep_d == rep_h
    assert np.array_equal(dev.coef.numpy().view(np.uint64), host.coef.numpy().view(np.uint64))
    Jh, Jd = host.jll_bytes(xt), dev.jll_bytes(_dev(xt))
    assert Jd.dtype == torch.float64 and not Jd.is_cuda
    auc = lambda J, on_dev: classify.auroc(classify.log_odds(J).cuda() if on_dev else classify.log_odds(J), yt)["micro"]
    _agree_nb("%s problem %d" % (kind, i), Jh.numpy(), Jd.numpy(), _sum_of_absolute_terms(host, xt), yt, K, auc(Jh, False), auc(Jd, True),
              classify.accuracy(Jh, yt)["hits"], classify.accuracy(Jd, yt)["hits"])
    assert np.array_equal(dev.jll_bytes(_dev(xt)).numpy().view(np.uint64), Jd.numpy().view(np.uint64))
    P = dev.predict_proba_bytes(_dev(xt)).numpy()
    assert np.abs(P.sum(1) - 1).max() <= 1e-12


def test_default_binarize_on_the_device():
    """bnb at the default binarize 0 — on these blobs nearly every byte is positive and the classes are close, so only the plumbing
    is held: the same report and the same tables as the host."""
    from csl_gan_amd import classify
    N, H, W, C, K, M = PROBLEMS[1]
    x, y = make(N, H, W, C, K, 1)
    host, dev = classify.NaiveBayes(K, "bnb"), classify.NaiveBayes(K, "bnb")
    assert dev.fit_bytes(_dev(x), _dev(y)) == host.fit_bytes(x, y) == {"kind": "bnb", "n_per_class": np.bincount(y).tolist(), "binarize": 0}
    assert np.array_equal(dev.coef.numpy().view(np.uint64), host.coef.numpy().view(np.uint64))


# ---- the command line --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [["--classifier", "gnb"], ["--classifier", "bnb", "--binarize", "127"]])
def test_cli_on_the_device_agrees_with_the_cpu(tmp_path, flags):
    from csl_gan_amd import classify, tstr
    c = make_caches(tmp_path)
    xt, yt = c["test"][1], c["test"][2]
    args = ["--syn_cache", c["syn"][0], "--test_cache", c["test"][0], "--train_cache", c["train"][0], "--baseline"] + flags
    dev = tstr.main(args + ["-d", "cuda:0", "--values_dir", str(tmp_path / "dev")])
    cpu = tstr.main(args + ["-d", "cpu", "--values_dir", str(tmp_path / "cpu")])
    assert list(dev) == list(cpu) == ["syn", "baseline_train"]
    load = lambda where, lab, n: np.load(os.path.join(str(tmp_path / where), "%s_%s.npy" % (lab, n)))
    for lab, (tx, ty) in (("syn", c["syn"][1:]), ("baseline_train", c["train"][1:])):
        d, h = dev[lab], cpu[lab]
        assert {k: v for k, v in d.items() if not k.startswith(("auroc", "accuracy"))} == {k: v for k, v in h.items() if not k.startswith(("auroc", "accuracy"))}
        assert d["fit"]["n_per_class"] == np.bincount(ty, minlength=3).tolist()
        assert np.array_equal(load("dev", lab, "U").view(np.uint64), load("cpu", lab, "U").view(np.uint64))
        clf = classify.NaiveBayes(3, flags[1], **({"binarize": 127} if flags[1] == "bnb" else {}))
        clf.fit_bytes(tx, ty)
        Jh, Jd = load("cpu", lab, "J"), load("dev", lab, "J")
        assert load("dev", lab, "P").shape == (200, 3) and np.abs(load("dev", lab, "P").sum(1) - 1).max() <= 1e-12
        _agree_nb("%s %s" % (flags[1], lab), Jh, Jd, _sum_of_absolute_terms(clf, xt), yt, 3, h["auroc_micro"], d["auroc_micro"], h["accuracy_hits"],
                  d["accuracy_hits"])
