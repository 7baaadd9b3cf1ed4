"""csl_gan_amd.svm and csl_gan_amd.tstr_svm on the CPU: the host model's solutions against the optimality conditions of
the dual, recomputed from the exact integer Gram matrix; against scikit-learn's SVC; LIBSVM's sigmoid fit, the folds, the chunked driver,
the probabilities; the command line with its refusals, tstr's own output across the refactor; and the host-side argument checks of the two
C-ABI entries (no launch, no device)."""
import functools
import os

import numpy as np
import pytest
import torch

from test_trees import sklearn_problem
from test_tstr import make_caches, write_cache

_SCORES = {"n_train", "n_test", "classes", "auroc_micro", "auroc_per_class", "accuracy", "accuracy_hits"}
SVM_KEYS = _SCORES | {"classifier", "fit", "C", "tol", "folds", "seed"}
PAIR = (3, 5)                       # the identical rows of the ragged problem, of classes 0 and 2


def ragged_problem():
    """(257, 930), K = 3: n off the 128-row tile, D off the 16-byte chunk; a band of brighter bytes per class over uniform noise; rows 3 and 5
    are identical and carry the labels 0 and 2: zero curvature for that pair (the TAU branch) and both at the bound C."""
    rng = np.random.default_rng(7)
    n, D, K = 257, 930, 3
    y = np.arange(n) % K
    X = rng.integers(0, 256, (n, D))
    for k in range(K):
        X[y == k, k * 40:(k + 1) * 40] += 60
    X = np.clip(X, 0, 255).astype(np.uint8)
    X[PAIR[1]] = X[PAIR[0]]
    return X, y, K


def problem(name):
    """(X, y, K) of "ragged" or "base0" .. "base2" (test_trees.sklearn_problem: 200 x 30, K = 2)."""
    if name == "ragged":
        return ragged_problem()
    X, y = sklearn_problem(int(name[4:]))
    return X, y, 2


NAMES = ["base0", "base1", "base2", "ragged"]


@functools.lru_cache(maxsize=None)
def host_fit(name):
    """The OvrSvc fitted on the host with the defaults (C = 1, tol = 1e-3, 5 folds, seed 0); computed once and left unchanged."""
    from csl_gan_amd import svm
    X, y, K = problem(name)
    clf = svm.OvrSvc(K)
    clf.fit_bytes(X, y)
    return clf


@functools.lru_cache(maxsize=None)
def exact_kernel(name):
    """K in float64 from numpy's integer dot products: no code of the package."""
    X = problem(name)[0].astype(np.int64)
    return (X @ X.T).astype(np.float64) / 65025.0


def gap(alpha, G, y, active, C):
    val = -y * G
    up = active & np.where(y > 0, alpha < C, alpha > 0)
    low = active & np.where(y > 0, alpha > 0, alpha < C)
    return val[up].max() - val[low].min()


# ---- the model -----------------------------------------------------------------------------------------------------------------------------

def test_gram_d2_host_is_the_squared_distance():
    from csl_gan_amd import svm
    X = problem("ragged")[0]
    d2, s = svm.gram_d2_host(X, block=100)
    Xi = X.astype(np.int64)
    assert d2.dtype == np.uint32 and np.array_equal(s, (Xi * Xi).sum(1))
    assert np.array_equal(d2.astype(np.int64), ((Xi[:, None, :60] - Xi[None, :, :60]) ** 2).sum(2) + ((Xi[:, None, 60:] - Xi[None, :, 60:]) ** 2).sum(2))
    assert np.array_equal(svm.kernel_rows(d2, s, np.arange(len(X))), exact_kernel("ragged"))
    big = np.full((2, 65536), 255, dtype=np.uint8)                           # the largest distance and norm: 65025 * 65536 < 2^32
    big[1] = 0
    d2, s = svm.gram_d2_host(big)
    assert d2.tolist() == [[0, 65025 * 65536], [65025 * 65536, 0]] and s.tolist() == [65025 * 65536, 0]


def test_the_ragged_problem_has_a_zero_curvature_pair_at_the_bound():
    """The two conditions the ragged problem is there for, on the host model: the identical rows are taken as a working pair whose curvature
    is replaced by TAU, and they end as support vectors at the bound."""
    from csl_gan_amd import svm
    X, y, K = ragged_problem()
    assert np.array_equal(X[PAIR[0]], X[PAIR[1]]) and (y[PAIR[0]], y[PAIR[1]]) == (0, 2)
    d2, s = svm.gram_d2_host(X)
    assert d2[PAIR] == 0
    for k in (0, 2):
        pairs = []
        st = svm.smo_host(d2, s, np.where(y == k, 1, -1), np.ones(len(y), bool), on_pair=lambda i, j, q: pairs.append((i, j, q)))
        assert st["done"] and st["iterations"] == len(pairs)
        hit = [q for i, j, q in pairs if {i, j} == set(PAIR)]
        assert hit and all(q == svm.TAU for q in hit), k
        assert all(q > svm.TAU for i, j, q in pairs if {i, j} != set(PAIR))
        assert st["alpha"][PAIR[0]] == 1.0 and st["alpha"][PAIR[1]] == 1.0
    rep = host_fit("ragged").report
    assert rep["n_bsv"][0] >= 2 and rep["n_bsv"][2] >= 2 and all(rep["converged"])


@pytest.mark.parametrize("name", NAMES)
def test_every_solution_is_optimal_from_first_principles(name):
    """All K (1 + folds) problems: 0 <= alpha <= C exactly, alpha = 0 outside the active rows, |sum y alpha| <= 1e-12 n, and the gap
    m - M of the gradient RECOMPUTED from alpha and the exact Gram matrix below tol + 1e-9.  w is unique, so this is sufficient.  The
    iterated gradient is within 1e-10 of the recomputed one (the prototype's drift was 7e-13)."""
    clf = host_fit(name)
    sol, Kx = clf.solution, exact_kernel(name)
    n = Kx.shape[0]
    assert sol["alpha"].shape == (clf.K * 6, n) and sol["done"].all()
    worst = 0.0
    for p in range(clf.K * 6):
        a, y, act = sol["alpha"][p], sol["Y"][p].astype(np.float64), sol["active"][p]
        assert (a >= 0).all() and (a <= clf.C).all() and (a[~act] == 0).all()
        assert abs((y * a).sum()) <= 1e-12 * n
        G = y * (Kx @ (y * a)) - 1.0
        worst = max(worst, np.abs(G - sol["grad"][p]).max())
        assert gap(a, G, y, act, clf.C) < clf.tol + 1e-9, p
    print("%s: max |iterated - recomputed gradient| = %.3g" % (name, worst))
    assert worst <= 1e-10


@pytest.mark.parametrize("seed", range(3))
def test_against_scikit_learn(seed):
    """SVC(kernel='linear', C=1, tol=1e-6, shrinking=False) on X / 255 against smo_host at tol = 1e-6: identical support sets, decision
    values on the training rows within 6.9e-5.  The bound is 10 x the largest difference observed on these three seeds against scikit-learn
    1.7.2 (4.0e-6, 5.4e-6, 6.9e-6): LIBSVM keeps its kernel rows in float32, so the two solves stop at slightly different points."""
    sksvm = pytest.importorskip("sklearn.svm")
    from csl_gan_amd import svm
    X, y = sklearn_problem(seed)
    ypm, act = np.where(y == 1, 1, -1), np.ones(len(y), bool)
    d2, s = svm.gram_d2_host(X)
    st = svm.smo_host(d2, s, ypm, act, 1.0, 1e-6)
    assert st["done"]
    f = ypm * (st["grad"] + 1.0) - svm.rho_host(st["alpha"], st["grad"], ypm, act, 1.0)
    ref = sksvm.SVC(kernel="linear", C=1.0, tol=1e-6, shrinking=False).fit(X / 255.0, y)
    err = float(np.abs(f - ref.decision_function(X / 255.0)).max())
    print("seed %d: %d iterations, %d support vectors, max |f - f_sklearn| = %.3g" % (seed, st["iterations"], len(ref.support_), err))
    assert np.array_equal(np.nonzero(st["alpha"] > 0)[0], np.sort(ref.support_))
    assert err <= 6.9e-5


def test_rho_is_the_free_mean_or_the_midpoint():
    from csl_gan_amd import svm
    y, act = np.array([1, -1, 1, -1, 1]), np.array([True, True, True, True, False])
    G = np.array([-0.5, 0.25, -2.0, 3.0, 100.0])
    assert svm.rho_host(np.array([0.5, 0.25, 0.0, 1.0, 0.5]), G, y, act, 1.0) == (-0.5 + -0.25) / 2
    # nothing free: y G = -0.5 (y +, at 0: ub), -0.25 (y -, at 0: lb), -2 (y +, at C: lb), -3 (y -, at C: ub)
    assert svm.rho_host(np.array([0.0, 0.0, 1.0, 1.0, 0.5]), G, y, act, 1.0) == (-3.0 + -0.25) / 2


# ---- Platt ---------------------------------------------------------------------------------------------------------------------------------

def test_sigmoid_train_reaches_a_stationary_point():
    """Targets (N+ + 1) / (N+ + 2) and 1 / (N- + 2), start (0, log((N- + 1) / (N+ + 1))); at the returned (A, B) the gradient of the
    regularised cross-entropy, written out here in float64, has max-norm <= 1e-5 (LIBSVM's stopping rule)."""
    from csl_gan_amd import svm
    rng = np.random.default_rng(5)
    for n_pos, n_neg, shift in ((30, 50, 1.0), (2, 2, 0.5), (100, 7, 2.0)):
        y = np.array([1] * n_pos + [-1] * n_neg)
        f = rng.normal(shift * y, 1.0)
        t, A0, B0 = svm.platt_targets(y)
        assert set(np.unique(t)) == {(n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0)} and (t[y > 0] == (n_pos + 1.0) / (n_pos + 2.0)).all()
        assert A0 == 0.0 and B0 == np.log((n_neg + 1.0) / (n_pos + 1.0))
        A, B = svm.sigmoid_train(f, y)
        p = 1.0 / (1.0 + np.exp(A * f + B))
        gA, gB = (f * (t - p)).sum(), (t - p).sum()
        print("(%d, %d): A %.6f B %.6f gradient (%.2e, %.2e)" % (n_pos, n_neg, A, B, gA, gB))
        assert A < 0 and max(abs(gA), abs(gB)) <= 1e-5
    for name in NAMES:
        clf = host_fit(name)
        assert all(a < 0 for a in clf.report["A"]), name


# ---- folds -----------------------------------------------------------------------------------------------------------------------------------

def test_folds():
    from csl_gan_amd import svm
    rng = np.random.default_rng(0)
    labels = np.concatenate([rng.integers(0, 3, 95), [3, 3]])               # class 3 has 2 rows
    Y, active, fold = svm.problems_of(labels, 4, 5, seed=0)
    assert Y.shape == active.shape == (24, 97) and Y.dtype == np.int8 and fold.shape == (4, 97)
    for k in range(4):
        p0 = 6 * k
        assert active[p0].all() and (Y[p0:p0 + 6] == np.where(labels == k, 1, -1)).all()
        held = ~active[p0 + 1:p0 + 6]
        assert (held.sum(0) == 1).all()                                       # every row is held out exactly once
        for f in range(5):
            assert np.array_equal(held[f], fold[k] == f)
            assert (Y[p0][active[p0 + 1 + f]] > 0).sum() >= 1 and (Y[p0][active[p0 + 1 + f]] < 0).sum() >= 1
        counts = np.bincount(fold[k][labels == k], minlength=5)
        assert counts.max() - counts.min() <= 1                               # dealt round-robin within the positives
    again = svm.problems_of(labels, 4, 5, seed=0)
    assert np.array_equal(again[2], fold) and np.array_equal(again[1], active)
    assert not np.array_equal(svm.problems_of(labels, 4, 5, seed=1)[2], fold)
    with pytest.raises(ValueError, match="class 3 has 1 rows"):
        svm.problems_of(labels[:-1], 4, 5, seed=0)
    with pytest.raises(ValueError, match="class 0 has 4 rows against 1"):
        svm.problems_of(np.array([0, 0, 0, 0, 1]), 2, 5, seed=0)


# ---- the chunked driver ----------------------------------------------------------------------------------------------------------------------

def test_chunks_do_not_change_the_solution():
    """chunk = 1, 7 and 4096 against one uncut run: the same bits in alpha and the gradient, the same iteration count; a run cut at max_iter
    is not done, and continuing it with a larger max_iter ends where the uncut run ends."""
    from csl_gan_amd import svm
    X, y, K = ragged_problem()
    d2, s = svm.gram_d2_host(X)
    clf = host_fit("ragged")
    Y, act = clf.solution["Y"][2], clf.solution["active"][2]                  # class 0 without its fold 1
    want = svm.smo_host(d2, s, Y, act)
    assert np.array_equal(want["alpha"], clf.solution["alpha"][2]) and want["iterations"] == clf.solution["iterations"][2] > 100
    for chunk in (1, 7, 4096):
        st, calls = svm.smo_start(len(y)), 0
        while not st["done"]:
            before = st["iterations"]
            svm.smo_host(d2, s, Y, act, state=st, chunk=chunk)
            assert st["iterations"] - before <= chunk
            calls += 1
        assert st["iterations"] == want["iterations"] and calls >= want["iterations"] // chunk
        assert np.array_equal(st["alpha"], want["alpha"]) and np.array_equal(st["grad"], want["grad"])
    cut = svm.smo_host(d2, s, Y, act, max_iter=50)
    assert cut["iterations"] == 50 and not cut["done"]
    svm.smo_host(d2, s, Y, act, state=cut)
    assert cut["done"] and np.array_equal(cut["alpha"], want["alpha"])


def test_max_iter_is_reported_not_raised():
    from csl_gan_amd import svm
    X, y, K = problem("base0")
    clf = svm.OvrSvc(K, max_iter=20)
    rep = clf.fit_bytes(X, y)
    assert rep["converged"] == [False, False] and rep["iterations"] == [20, 20] and rep["iterations_total"] == 20 * 12
    assert np.isfinite(clf.coef.numpy()).all()


# ---- probabilities -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_probabilities_are_the_normalised_sigmoids(name):
    """predict_proba_bytes (the logistic form U) against 1 / (1 + exp(A f + B)) with f = sum_i alpha_i y_i K(x_i, x) - rho evaluated directly,
    normalised over the classes: 1e-12; rows sum to 1; the report's counts are the solution's."""
    clf = host_fit(name)
    X, y, K = problem(name)
    rng = np.random.default_rng(11)
    Xt = np.clip(X[rng.integers(0, len(X), 64)].astype(np.int64) + rng.integers(-20, 21, (64, X.shape[1])), 0, 255).astype(np.uint8)
    P = clf.predict_proba_bytes(Xt)
    assert P.dtype == torch.float64 and tuple(P.shape) == (64, K)
    Kt = (Xt.astype(np.int64) @ X.astype(np.int64).T).astype(np.float64) / 65025.0
    S = np.empty((64, K))
    rep = clf.report
    for k in range(K):
        a, yk = clf.solution["alpha"][6 * k], clf.solution["Y"][6 * k].astype(np.float64)
        f = Kt @ (a * yk) - rep["rho"][k]
        S[:, k] = 1.0 / (1.0 + np.exp(rep["A"][k] * f + rep["B"][k]))
        assert rep["n_sv"][k] == int((a > 0).sum()) and rep["n_bsv"][k] == int((a == clf.C).sum())
        assert rep["iterations"][k] == clf.solution["iterations"][6 * k]
    err = float(np.abs(P.numpy() - S / S.sum(1, keepdims=True)).max())
    print("%s: max |P - direct| = %.3g" % (name, err))
    assert err <= 1e-12 and np.abs(P.numpy().sum(1) - 1.0).max() <= 1e-12
    assert rep["n_per_class"] == np.bincount(y, minlength=K).tolist() and rep["iterations_total"] == int(clf.solution["iterations"].sum())
    assert tuple(clf.coef.shape) == (X.shape[1] + 1, K) and clf.coef.dtype == torch.float64


def test_estimator_refusals():
    from csl_gan_amd import svm
    X, y, K = problem("base0")
    for kw in ({"C": 0.0}, {"tol": 0.0}, {"C": float("inf")}, {"folds": 1}, {"max_iter": -1}):
        with pytest.raises(ValueError):
            svm.OvrSvc(2, **kw)
    with pytest.raises(ValueError, match="folds"):
        svm.OvrSvc(16, folds=6)
    with pytest.raises(ValueError, match="at least 2 on each side"):
        svm.OvrSvc(2).fit_bytes(X[:10], np.array([0] * 9 + [1]))
    with pytest.raises(ValueError):
        svm.OvrSvc(3).fit_bytes(X, y)                                         # class 2 has no row
    with pytest.raises(RuntimeError, match="fit first"):
        svm.OvrSvc(2).predict_proba_bytes(X)


# ---- the command line --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    return make_caches(tmp_path_factory.mktemp("svm_caches"))


def test_cli_on_the_cpu(caches, tmp_path, capsys):
    from csl_gan_amd import classify, svm, tstr_svm
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    vals = str(tmp_path / "vals")
    res = tstr_svm.main(["--syn_cache", syn, "--test_cache", test, "--train_cache", caches["train"][0], "--baseline", "-d", "cpu", "--values_dir", vals,
                         "--seed", "3"])
    assert list(res) == ["syn", "baseline_train"]
    m = res["syn"]
    assert set(m) == SVM_KEYS and set(res["baseline_train"]) == SVM_KEYS
    assert m["classifier"] == "svm" and (m["C"], m["tol"], m["folds"], m["seed"]) == (1.0, 1e-3, 5, 3)
    clf = svm.OvrSvc(3, seed=3)
    rep = clf.fit_bytes(x, y)
    P = clf.predict_proba_bytes(xt)
    assert m["fit"] == rep and all(rep["converged"]) and set(rep) == {"n_per_class", "iterations", "converged", "n_sv", "n_bsv", "rho", "A", "B",
                                                                      "iterations_total"}
    a, acc = classify.auroc(P, torch.from_numpy(yt)), classify.accuracy(P, torch.from_numpy(yt))
    assert m["auroc_micro"] == a["micro"] and m["accuracy_hits"] == acc["hits"] and 0.8 < a["micro"] < 1.0
    assert (m["n_train"], m["n_test"], m["classes"]) == (300, 200, 3) and res["baseline_train"]["n_train"] == 240
    assert np.array_equal(np.load(os.path.join(vals, "syn_P.npy")), P.numpy())
    assert np.array_equal(np.load(os.path.join(vals, "syn_U.npy")), clf.coef.numpy())
    assert np.load(os.path.join(vals, "baseline_train_U.npy")).shape == (1025, 3)
    out = capsys.readouterr().out
    assert "syn: fitted on 300 rows, scored 200: AUROC %.6f" % a["micro"] in out and "   fit: rows per class %s  iterations %s" % (rep["n_per_class"], rep["iterations"]) in out


def test_cli_refusals(caches, tmp_path):
    from csl_gan_amd import tstr_svm
    syn, x, y = caches["syn"]
    test = caches["test"][0]
    d = str(tmp_path)
    with pytest.raises(SystemExit, match="give --train_cache"):
        tstr_svm.main(["--syn_cache", syn, "--test_cache", test, "--baseline"])
    lone = np.array(y)
    lone[lone == 1] = 0
    lone[0] = 1                                                               # class 1 keeps one row
    p = write_cache(os.path.join(d, "lone"), x, lone, 32, 32, 1)
    with pytest.raises(SystemExit, match="at least 2 rows"):
        tstr_svm.main(["--syn_cache", p, "--test_cache", test])
    geo = write_cache(os.path.join(d, "geo"), x, y, 16, 64, 1)
    with pytest.raises(SystemExit, match="one geometry"):
        tstr_svm.main(["--syn_cache", geo, "--test_cache", test])
    two = write_cache(os.path.join(d, "two"), x, y % 2, 32, 32, 1)
    with pytest.raises(SystemExit, match="test labels span 0 .. 2"):
        tstr_svm.main(["--syn_cache", two, "--test_cache", test])
    for flags, msg in ((["--C", "0"], "--C 0"), (["--tol", "0"], "--tol 0"), (["--folds", "1"], "--folds 1"), (["--svm_max_iter", "-1"], "--svm_max_iter -1")):
        with pytest.raises(SystemExit, match=msg):
            tstr_svm.main(["--syn_cache", syn, "--test_cache", test] + flags)
    with pytest.raises(SystemExit, match="65537 rows"):                        # the rule itself: no cache of that size is written
        tstr_svm.check_set(np.arange(65537) % 3, 3, "big")
    tstr_svm.check_set(np.arange(65536) % 3, 3, "big")


def test_tstr_is_unchanged_by_the_shared_frame(caches, capsys):
    """tstr.main for --classifier lr --max_iter 3 against a direct tstr.fit_and_score call on the same caches: the same keys in the same
    order and the same values; the parser's arguments in the order they had."""
    from csl_gan_amd import tstr
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    argv = ["--syn_cache", syn, "--test_cache", test, "-d", "cpu", "--classifier", "lr", "--max_iter", "3"]
    res = tstr.main(argv)
    a = tstr.build_parser().parse_args(argv)
    want, _ = tstr.fit_and_score(tstr.ESTIMATORS["lr"], a, x, y, 3, torch.from_numpy(xt), torch.from_numpy(yt), torch.device("cpu"))
    assert list(res) == ["syn"] and list(res["syn"]) == list(want) and res["syn"] == want
    assert list(want) == ["n_train", "n_test", "classes", "auroc_micro", "auroc_per_class", "accuracy", "accuracy_hits", "solver"]
    assert "   solver: iterations" in capsys.readouterr().out
    dests = [act.dest for act in tstr.build_parser()._actions]
    assert dests[:12] == ["help", "syn_cache", "device", "values_dir", "outputs_dir", "name", "save", "test_cache", "train_cache", "baseline",
                          "gtol_rel", "max_iter"]
    assert tstr.build_parser().parse_args(argv).name == "tstr"


# ---- the C-ABI entries validate on the host -------------------------------------------------------------------------------------------------

def test_abi_entries_reject_bad_arguments_without_a_device():
    from csl_gan_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert {"cslgan_gram_d2_u8", "cslgan_svc_smo_f64"} <= set(_lib.EXPORTS) and L.cslgan_version() == 7
    err = lambda: L.cslgan_last_error()
    ok = dict(xs=128, sq=128, n=257, Dp=960, out=128, pitch=288)

    def gram(**kw):
        a = dict(ok, **kw)
        return L.cslgan_gram_d2_u8(a["xs"], a["sq"], a["n"], a["Dp"], a["out"], a["pitch"], None)

    for name in ("xs", "sq", "out"):
        assert gram(**{name: None}) == -1 and b"null" in err(), name
    for n in (0, -1):
        assert gram(n=n) == -1 and b"n=" in err()
    assert gram(n=65537, pitch=65568) == -1 and b"65537 rows" in err() and b"16 GiB" in err()     # refused before anything is allocated
    for dp in (0, 930, 65600):
        assert gram(Dp=dp) == -1 and b"Dp=" in err()
    for pitch in (256, 257, 290, 65568):
        assert gram(pitch=pitch) == -1 and b"pitch=" in err()
    for name, v in (("xs", 136), ("sq", 130), ("out", 192), ("out", 144)):
        assert gram(**{name: v}) == -1 and b"misaligned" in err(), (name, v)

    ok2 = dict(d2=128, pitch=288, s=128, n=257, y=128, act=128, P=18, C=1.0, tol=1e-3, chunk=64, max_iter=100, alpha=128, grad=128, iters=128, done=128)

    def smo(**kw):
        a = dict(ok2, **kw)
        return L.cslgan_svc_smo_f64(a["d2"], a["pitch"], a["s"], a["n"], a["y"], a["act"], a["P"], a["C"], a["tol"], a["chunk"], a["max_iter"],
                                    a["alpha"], a["grad"], a["iters"], a["done"], None)

    for name in ("d2", "s", "y", "act", "alpha", "grad", "iters", "done"):
        assert smo(**{name: None}) == -1 and b"null" in err(), name
    for n in (0, 1, 65537):
        assert smo(n=n, pitch=65536) == -1 and b"n=" in err()
    for pitch in (256, 260, 65568):
        assert smo(pitch=pitch) == -1 and b"pitch=" in err()
    for P in (0, 97):
        assert smo(P=P) == -1 and b"n_problems=" in err()
    for c in (0.0, -1.0, float("inf"), float("nan")):
        assert smo(C=c) == -1 and b"C=" in err()
    for tol in (0.0, float("inf")):
        assert smo(tol=tol) == -1 and b"tol=" in err()
    assert smo(chunk=0) == -1 and b"chunk=" in err()
    assert smo(max_iter=-1) == -1 and b"max_iter=" in err()
    for name, v in (("d2", 192), ("s", 132), ("alpha", 132), ("grad", 132), ("iters", 132), ("done", 130)):
        assert smo(**{name: v}) == -1 and b"misaligned" in err(), (name, v)
