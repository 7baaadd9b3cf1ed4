"""csl_gan_amd.classify.NaiveBayes and `tstr --classifier gnb / bnb` on the CPU: the integer moments against a direct
numpy computation, the joint log-likelihoods against the textbook formulas on x = byte / 255 written out here in float64 numpy (with
the float32-rounded tables the library scores with), a case worked by hand, posteriors and log-odds, the refusals, the command line
on the blob caches of tests/test_tstr.py, and the host-side argument checks of the three C-ABI entries (no launch, no device)."""
import json
import os

import numpy as np
import pytest
import torch

from test_tstr import PROBLEMS, make, make_caches


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    return make_caches(tmp_path_factory.mktemp("nb_caches"))


def _bytes(N, D, K, seed, lo=-2, hi=2):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    X[:, ::7] = 0
    X[0, :] = 255
    y = rng.integers(lo, K + hi, N)
    return X, y


def _moments_numpy(X, y, K, thr):
    X = X.astype(np.int64)
    T = (y[None, :] == np.arange(K)[:, None]).astype(np.int64)
    return {"n": T.sum(1), "s1": T @ X, "s2": T @ (X * X), "cnt": T @ (X > thr).astype(np.int64)}


# ---- the moments --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("binarize", [0, 127, 254])
def test_moments_equal_a_direct_integer_computation(binarize):
    """Row blocks of 1, 7 and >= N, labels -2 .. K + 1 (outside the classes: no class), binarize 0, 127, 254."""
    from csl_gan_amd import classify
    N, D, K = 50, 93, 5
    X, y = _bytes(N, D, K, 11)
    assert (y < 0).any() and (y >= K).any()
    ref = _moments_numpy(X, y, K, binarize)
    for block in (1, 7, 50, 4096):
        got = classify.class_moments_host_bytes(X, y, K, binarize, block=block)
        assert sorted(got) == ["cnt", "n", "s1", "s2"]
        for name in ref:
            assert got[name].dtype == torch.int64 and np.array_equal(got[name].numpy(), ref[name]), (name, block)
    assert int(got["n"].sum()) == int(((y >= 0) & (y < K)).sum()) < N


def test_moments_refusals():
    from csl_gan_amd import classify
    X, y = _bytes(20, 9, 3, 2, 0, 0)
    for b in (-1, 255, 0.5):
        with pytest.raises(ValueError, match="binarize"):
            classify.class_moments_host_bytes(X, y, 3, b)
    for k in (1, 17):
        with pytest.raises(ValueError, match="n_classes"):
            classify.class_moments_host_bytes(X, y, k)
    with pytest.raises(ValueError, match="uint8"):
        classify.class_moments_host_bytes(X.astype(np.float32), y, 3)
    with pytest.raises(ValueError, match="labels"):
        classify.class_moments_host_bytes(X, y[:-1], 3)
    wide = np.zeros((3, 65537), dtype=np.uint8)
    for bad in (wide, wide[:, :0]):
        with pytest.raises(ValueError, match="1 .. 65536 bytes"):
            classify.class_moments_host_bytes(bad, [0, 1, 2], 3)
        with pytest.raises(ValueError, match="1 .. 65536 bytes"):
            classify.NaiveBayes(3, "gnb").fit_bytes(bad, [0, 1, 2])


def test_variance_numerator_is_exact_beyond_int64():
    """n s2 - s1^2 at n = 2^31 - 1 rows (the products pass 2^63): Python integers, the same value as the int64 route where that fits."""
    from csl_gan_amd import classify
    n = 2 ** 31 - 1
    s1, s2 = np.array([[255 * n, 7 * n + 3]]), np.array([[65025 * n, 49 * n + 1000]])
    got = classify._variance_times_n2(np.array([[n]]), s1, s2)
    exp = [float(n * int(b) - int(a) ** 2) for a, b in zip(s1[0], s2[0])]
    assert got.dtype == np.float64 and got[0].tolist() == exp and exp[0] == 0.0
    small = classify._variance_times_n2(np.array([[1000]]), np.array([[5000, 17]]), np.array([[26000, 289]]))
    assert small[0].tolist() == [1000.0 * 26000 - 5000.0 ** 2, 1000.0 * 289 - 289.0]


# ---- the joint log-likelihoods --------------------------------------------------------------------------------------------------------

def _gnb_textbook(x, y, xt, K, var_smoothing, m32, w32):
    """sum_j log N(x_j; theta, sigma^2 + eps) + log prior on x = b / 255, float64: scikit-learn's GaussianNB written out.  The mean and
    the precision are the library's float32-rounded tables mapped back to x units (theta = m / 255, 1 / (2 var) = 255^2 w); the
    normalising constant uses the float64 variances of this function, as the library's c does."""
    X, Xt = x.astype(np.float64) / 255.0, xt.astype(np.float64) / 255.0
    eps = var_smoothing * X.var(0).max()
    out = np.empty((len(Xt), K))
    for k in range(K):
        Xk = X[y == k]
        var = Xk.var(0) + eps
        theta, prec2 = m32[k].astype(np.float64) / 255.0, w32[k].astype(np.float64) * 65025.0      # prec2 = 1 / (2 var)
        out[:, k] = np.log(len(Xk) / len(X)) - 0.5 * np.log(2.0 * np.pi * var).sum() - (prec2 * (Xt - theta) ** 2).sum(1)
    return out, eps * 65025.0


def _bnb_textbook(x, y, xt, K, alpha, thr, d32):
    """log prior + sum_j [f_j log p_j + (1 - f_j) log(1 - p_j)] on f = [b > thr], float64: BernoulliNB written out, with
    log p - log(1 - p) taken from the library's float32 table and log(1 - p) in float64."""
    F, Ft = (x > thr).astype(np.float64), (xt > thr).astype(np.float64)
    out = np.empty((len(Ft), K))
    for k in range(K):
        Fk = F[y == k]
        p = (Fk.sum(0) + alpha) / (len(Fk) + 2.0 * alpha)
        out[:, k] = np.log(len(Fk) / len(F)) + np.log1p(-p).sum() + Ft @ d32[k].astype(np.float64)
    return out


@pytest.mark.parametrize("i", range(len(PROBLEMS)))
def test_jll_equals_the_textbook_formulas(i):
    """gnb, and bnb at binarize 0 and 127, on the three problems of tests/test_tstr.py: 1e-9 of the largest |jll|; the float32
    tables themselves within float32 rounding of the float64 moments of x."""
    from csl_gan_amd import classify
    N, H, W, C, K, M = PROBLEMS[i]
    x, y = make(N, H, W, C, K, 1)
    xt, yt = make(M, H, W, C, K, 2)
    g = classify.NaiveBayes(K, "gnb")
    rep = g.fit_bytes(x, y)
    m32, w32 = g.tables
    X = x.astype(np.float64)
    for k in range(K):
        assert np.abs(m32[k] - X[y == k].mean(0)).max() <= 255 * 2.0 ** -24
        var = X[y == k].var(0) + rep["eps"]
        assert np.abs(w32[k] * (2.0 * var) - 1.0).max() <= 1e-6
    J = g.jll_bytes(xt).numpy()
    ref, eps = _gnb_textbook(x, y, xt, K, 1e-9, m32, w32)
    err = np.abs(J - ref).max() / np.abs(ref).max()
    print("problem %d gnb: eps %.6g (textbook %.6g), jll err %.2e of %.3g" % (i, rep["eps"], eps, err, np.abs(ref).max()))
    assert abs(rep["eps"] - eps) <= 1e-12 * eps and err <= 1e-9
    assert rep["kind"] == "gnb" and rep["n_per_class"] == np.bincount(y, minlength=K).tolist() and "binarize" not in rep
    assert g.coef.dtype == torch.float64 and tuple(g.coef.shape) == (2 * x.shape[1] + 1, K)
    for thr in (0, 127):
        b = classify.NaiveBayes(K, "bnb", binarize=thr)
        rep = b.fit_bytes(x, y)
        d32, = b.tables
        p = ((x[y == 0] > thr).sum(0) + 0.01) / ((y == 0).sum() + 0.02)
        assert np.abs(d32[0] - (np.log(p) - np.log1p(-p))).max() <= 1e-6 * np.abs(d32[0]).max()
        J = b.jll_bytes(xt).numpy()
        ref = _bnb_textbook(x, y, xt, K, 0.01, thr, d32)
        err = np.abs(J - ref).max() / np.abs(ref).max()
        print("problem %d bnb binarize %d: jll err %.2e of %.3g" % (i, thr, err, np.abs(ref).max()))
        assert err <= 1e-9
        assert rep == {"kind": "bnb", "n_per_class": np.bincount(y, minlength=K).tolist(), "binarize": thr}
        assert tuple(b.coef.shape) == (x.shape[1] + 1, K)


def test_two_rows_two_features_by_hand():
    """Class 0 holds (0, 10) and (2, 10), class 1 holds (255, 20) and (255, 40), var_smoothing 0.5.
    gnb in byte units: m = [[1, 10], [255, 30]], v = [[1, 0], [0, 100]]; pooled: feature 0 has mean 128, variance
    (128^2 + 126^2 + 2 127^2) / 4 = 16129.5, feature 1 has mean 20, variance 150: eps = 0.5 * 16129.5 = 8064.75.
    bnb at binarize 15, alpha 1: cnt = [[0, 0], [2, 2]], p = (cnt + 1) / 4 = [[1/4, 1/4], [3/4, 3/4]]."""
    from csl_gan_amd import classify
    X = np.array([[0, 10], [2, 10], [255, 20], [255, 40]], dtype=np.uint8)
    y = np.array([0, 0, 1, 1])
    mom = classify.class_moments_host_bytes(X, y, 2, 15)
    assert mom["n"].tolist() == [2, 2] and mom["s1"].tolist() == [[2, 20], [510, 60]]
    assert mom["s2"].tolist() == [[4, 200], [130050, 2000]] and mom["cnt"].tolist() == [[0, 0], [2, 2]]
    g = classify.NaiveBayes(2, "gnb", var_smoothing=0.5)
    rep = g.fit_bytes(X, y)
    assert rep["eps"] == 8064.75 and rep["n_per_class"] == [2, 2]
    m, w = g.tables
    assert m.tolist() == [[1.0, 10.0], [255.0, 30.0]]
    v = np.array([[1.0, 0.0], [0.0, 100.0]]) + 8064.75
    assert np.array_equal(w, (1.0 / (2.0 * v)).astype(np.float32))
    c = np.log(0.5) - 0.5 * np.log(2.0 * np.pi * v / 65025.0).sum(1)
    t = np.array([[3, 12]], dtype=np.uint8)
    J = g.jll_bytes(t).numpy()[0]
    exp = c - (w.astype(np.float64) * (np.array([3.0, 12.0]) - m) ** 2).sum(1)
    assert np.abs(J - exp).max() <= 1e-12 * np.abs(exp).max()
    by_hand = [c[0] - (4.0 / (2 * 8065.75) + 4.0 / (2 * 8064.75)), c[1] - (252.0 ** 2 / (2 * 8064.75) + 18.0 ** 2 / (2 * 8164.75))]
    assert np.abs(J - by_hand).max() <= 1e-6                       # the float32 rounding of w
    assert np.array_equal(g.coef.numpy(), np.concatenate([m.astype(np.float64).T, w.astype(np.float64).T, c[None]], 0))
    b = classify.NaiveBayes(2, "bnb", alpha=1.0, binarize=15)
    b.fit_bytes(X, y)
    d, = b.tables
    assert np.allclose(d, [[np.log(1 / 3)] * 2, [np.log(3.0)] * 2], rtol=1e-6, atol=0)
    J = b.jll_bytes(np.array([[16, 15], [0, 0]], dtype=np.uint8)).numpy()
    # row 0: feature 0 on, feature 1 off; row 1: both off
    exp = [[np.log(0.5) + np.log(0.25) + np.log(0.75), np.log(0.5) + np.log(0.75) + np.log(0.25)],
           [np.log(0.5) + 2 * np.log(0.75), np.log(0.5) + 2 * np.log(0.25)]]
    assert np.abs(J - np.array(exp)).max() <= 1e-6


# ---- posteriors, log-odds, determinism, refusals ------------------------------------------------------------------------------------------

def test_posteriors_log_odds_and_a_second_fit():
    from csl_gan_amd import classify
    N, H, W, C, K, M = PROBLEMS[0]
    x, y = make(N, H, W, C, K, 1)
    xt, yt = make(M, H, W, C, K, 2)
    for kind, kw in (("gnb", {}), ("bnb", {"binarize": 127})):
        clf = classify.NaiveBayes(K, kind, **kw)
        clf.fit_bytes(x, y)
        J, P, L = clf.jll_bytes(xt), clf.predict_proba_bytes(xt), clf.log_odds_bytes(xt)
        assert P.dtype == J.dtype == L.dtype == torch.float64 and tuple(P.shape) == tuple(L.shape) == (M, K)
        P, L, Jn = P.numpy(), L.numpy(), J.numpy()
        assert np.abs(P.sum(1) - 1).max() <= 1e-12
        assert np.array_equal(P, torch.softmax(J, 1).numpy())
        for k in range(K):                                           # L orders as P does wherever the posteriors are distinct
            order = np.argsort(L[:, k], kind="stable")
            p = P[order, k]
            assert (np.diff(p) >= -1e-15).all()
            l = np.sort(L[:, k])
            others = np.delete(Jn, k, 1)
            exp = Jn[:, k] - (others.max(1) + np.log(np.exp(others - others.max(1, keepdims=True)).sum(1)))
            assert np.abs(L[:, k] - exp).max() <= 1e-9 * np.abs(exp).max() and np.isfinite(l).all()
        sat = int(((P == 0) | (P == 1)).sum())
        acc = classify.accuracy(J, yt)
        a = classify.auroc(L, yt)
        print("%s: accuracy %.4f  micro-AUROC %.4f  saturated posteriors %d of %d" % (kind, acc["accuracy"], a["micro"], sat, P.size))
        assert acc["accuracy"] > 0.7 and a["micro"] > 0.8            # it has learnt the blobs
        again = classify.NaiveBayes(K, kind, **kw)
        assert again.fit_bytes(x, y) == clf.report
        assert np.array_equal(again.coef.numpy().view(np.uint64), clf.coef.numpy().view(np.uint64))
        assert np.array_equal(again.jll_bytes(xt).numpy().view(np.uint64), Jn.view(np.uint64))


def test_estimator_refusals():
    from csl_gan_amd import classify
    x, y = make(60, 8, 8, 1, 3, 1)
    NB = classify.NaiveBayes
    with pytest.raises(ValueError, match="kind"):
        NB(3, "mnb")
    for k in (1, 17):
        with pytest.raises(ValueError, match="n_classes"):
            NB(k, "gnb")
    for a in (0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            NB(3, "bnb", alpha=a)
    with pytest.raises(ValueError, match="var_smoothing"):
        NB(3, "gnb", var_smoothing=-1e-9)
    for b in (-1, 255):
        with pytest.raises(ValueError, match="binarize"):
            NB(3, "bnb", binarize=b)
    for kind in ("gnb", "bnb"):
        with pytest.raises(ValueError, match="every class"):
            NB(4, kind).fit_bytes(x, y)
        with pytest.raises(ValueError, match="every class"):
            NB(2, kind).fit_bytes(x, y)                              # labels beyond the classes
        with pytest.raises(ValueError, match="uint8"):
            NB(3, kind).fit_bytes(x.astype(np.float32), y)
        with pytest.raises(RuntimeError, match="fit first"):
            NB(3, kind).jll_bytes(x)
    with pytest.raises(ValueError, match="every feature is constant"):
        NB(3, "gnb").fit_bytes(np.full((60, 5), 9, dtype=np.uint8), y)
    with pytest.raises(ValueError, match="every feature is constant"):
        NB(3, "gnb", var_smoothing=0.0).fit_bytes(x, y)                # eps == 0
    clf = NB(3, "gnb")
    clf.fit_bytes(x, y)
    with pytest.raises(ValueError, match="rows"):
        clf.jll_bytes(x[:, :10])


# ---- the command line ---------------------------------------------------------------------------------------------------------------

LR_KEYS = {"n_train", "n_test", "classes", "auroc_micro", "auroc_per_class", "accuracy", "accuracy_hits", "solver"}


@pytest.mark.parametrize("flags,extra", [(["--classifier", "gnb"], {"var_smoothing": 1e-9}),
                                         (["--classifier", "bnb", "--binarize", "127"], {"alpha": 0.01, "binarize": 127})])
def test_cli_on_the_cpu(caches, tmp_path, capsys, flags, extra):
    from csl_gan_amd import classify, tstr
    kind = flags[1]
    syn, x, y = caches["syn"]
    syn2 = caches["syn2"]
    test, xt, yt = caches["test"]
    train = caches["train"]
    vals = str(tmp_path / "vals")
    res = tstr.main(["--syn_cache", syn, syn2[0], "--test_cache", test, "--train_cache", train[0], "--baseline", "-d", "cpu", "--values_dir", vals,
                     "--hidden", "7", "--alpha", "0.5", "--max_iter", "3"] + flags)                # the other classifiers' flags mean nothing
    assert list(res) == ["syn", "syn2", "baseline_train"]            # two --syn_cache arguments keep their labels
    out = capsys.readouterr().out
    for lab, (tx, ty) in (("syn", (x, y)), ("syn2", syn2[1:]), ("baseline_train", train[1:])):
        m = res[lab]
        assert set(m) == (LR_KEYS - {"solver"}) | {"classifier", "fit"} | set(extra)
        assert m["classifier"] == kind and all(m[k] == v for k, v in extra.items())
        assert (m["n_train"], m["n_test"], m["classes"]) == (len(ty), 200, 3)
        clf = classify.NaiveBayes(3, kind, **({"binarize": 127} if kind == "bnb" else {}))
        rep = clf.fit_bytes(tx, ty)
        assert m["fit"] == rep and m["fit"]["n_per_class"] == np.bincount(ty, minlength=3).tolist()
        P, J, U = (np.load(os.path.join(vals, "%s_%s.npy" % (lab, n))) for n in "PJU")
        assert P.dtype == J.dtype == U.dtype == np.float64
        assert P.shape == J.shape == (200, 3) and U.shape == ((2 * 1024 + 1, 3) if kind == "gnb" else (1025, 3))
        assert np.array_equal(J, clf.jll_bytes(xt).numpy()) and np.array_equal(U, clf.coef.numpy())
        assert np.abs(P.sum(1) - 1).max() <= 1e-12 and np.array_equal(P, clf.predict_proba_bytes(xt).numpy())
        acc = classify.accuracy(J, yt)
        assert m["accuracy_hits"] == acc["hits"] and m["accuracy"] == acc["hits"] / 200
        a = classify.auroc(clf.log_odds_bytes(xt), yt)
        assert m["auroc_micro"] == a["micro"] and m["auroc_per_class"] == a["per_class"] and 0.8 < a["micro"] <= 1.0
        assert "%s: fitted on %d rows, scored 200: AUROC %.6f" % (lab, len(ty), a["micro"]) in out
    assert out.count("fit: rows per class") == 3 and "solver:" not in out and (out.count("  eps ") == 3) == (kind == "gnb")
    json.dumps(res)                                                  # the figures are plain JSON


def test_cli_default_binarize_and_lr_unchanged(caches, tmp_path):
    """bnb at the default binarize 0: the plumbing (fields present, moments behind them exact).  --classifier lr: the dict it
    returned before, whatever naive-Bayes flags are given."""
    from csl_gan_amd import classify, tstr
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    args = ["--syn_cache", syn, "--test_cache", test, "-d", "cpu"]
    m = tstr.main(args + ["--classifier", "bnb", "--nb_alpha", "0.5"])["syn"]
    assert m["binarize"] == 0 and m["alpha"] == 0.5 and m["fit"] == {"kind": "bnb", "n_per_class": np.bincount(y, minlength=3).tolist(), "binarize": 0}
    lr = tstr.main(args + ["--var_smoothing", "0.1", "--nb_alpha", "3", "--binarize", "9"])["syn"]
    assert set(lr) == LR_KEYS
    clf = classify.OvrLogReg(3)
    rep = clf.fit_bytes(x, y)
    P = clf.predict_proba_bytes(xt)
    a, acc = classify.auroc(P, yt), classify.accuracy(P, yt)
    assert lr == {"n_train": 300, "n_test": 200, "classes": 3, "auroc_micro": a["micro"], "auroc_per_class": a["per_class"],
                  "accuracy": acc["accuracy"], "accuracy_hits": acc["hits"], "solver": rep}


def test_cli_refusals(caches):
    from csl_gan_amd import tstr
    args = ["--syn_cache", caches["syn"][0], "--test_cache", caches["test"][0], "-d", "cpu", "--classifier"]
    for flags, msg in ((["bnb", "--binarize", "255"], "--binarize 255"), (["bnb", "--binarize", "-1"], "--binarize -1"),
                       (["bnb", "--nb_alpha", "0"], "--nb_alpha"), (["gnb", "--var_smoothing", "-1"], "--var_smoothing"),
                       (["lr", "--binarize", "300"], "--binarize 300")):
        with pytest.raises(SystemExit, match=msg):
            tstr.main(args + flags)
    with pytest.raises(SystemExit):
        tstr.main(args + ["mnb"])                                      # argparse: not one of lr, mlp, gnb, bnb


# ---- the C-ABI entries validate on the host -----------------------------------------------------------------------------------------

def test_abi_entries_reject_bad_arguments_without_a_device():
    from csl_gan_amd import _lib, build
    build.build()
    L = _lib.lib()
    err = lambda: L.cslgan_last_error()

    def mo(X=16, lab=16, N=100, D=930, K=10, b=0, n=16, s1=16, s2=16, cnt=16):
        return L.cslgan_class_moments_u8(X, lab, N, D, K, b, n, s1, s2, cnt, None, None)

    def ga(X=16, m=16, w=16, M=10, D=930, K=10, S=16):
        return L.cslgan_nb_score_gauss_u8(X, m, w, M, D, K, S, None)

    def be(X=16, d=16, M=10, D=930, K=10, b=0, S=16):
        return L.cslgan_nb_score_bern_u8(X, d, M, D, K, b, S, None)

    for fn, ptrs, rows in ((mo, ("X", "lab", "n", "s1", "s2", "cnt"), "N"), (ga, ("X", "m", "w", "S"), "M"), (be, ("X", "d", "S"), "M")):
        for name in ptrs:
            assert fn(**{name: None}) == -1 and b"null" in err(), (fn, name)
        for k in (1, 17):
            assert fn(K=k) == -1 and b"K=" in err()
        for d in (0, -1, 65537):
            assert fn(D=d) == -1 and b"D=" in err()
        for r in (0, -1, 2 ** 31):
            assert fn(**{rows: r}) == -1 and (rows + "=").encode() in err()
        assert fn(X=17) == -1 and b"misaligned" in err()
    for fn in (mo, be):
        for b in (-1, 255):
            assert fn(b=b) == -1 and b"binarize=" in err()
    assert mo(s2=20) == -1 and b"misaligned" in err()


def test_ops_have_no_cpu_path():
    from csl_gan_amd import ops
    X, t = torch.zeros((8, 20), dtype=torch.uint8), torch.zeros(3, 20)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.class_moments_u8(X, torch.zeros(8, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.nb_score_gauss_u8(X, t, t)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.nb_score_bern_u8(X, t)
