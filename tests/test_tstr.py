"""csl_gan_amd.tstr and the byte paths of csl_gan_amd.classify on the CPU: objective_host_bytes against objective_host, the host
fit on bytes against the host fit on bytes / 255 as floats, the accuracy's tie rule, the command line end to end on small caches
with its refusals, and the host-side argument checks of the three C-ABI entries behind the device path (no launch, no device)."""
import functools
import json
import os

import numpy as np
import pytest
import torch


def make(N, H, W, C, K, seed, noise=60):
    """The labelled blob problem of DESIGN.md §6j: a blob per class, pixel noise, 15 % label noise (the classes overlap)."""
    rng = np.random.default_rng(seed)
    y = np.arange(N) % K
    x = np.zeros((N, H, W, C), dtype=np.int64)
    for i, k in enumerate(y):                                   # a blob per class, then noise
        r, c = (H // 4) * (k // 2) + 2, (W // 3) * (k % 2) + 3
        x[i, r:r + H // 3, c:c + W // 3, :] = rng.integers(60, 200, (H // 3, W // 3, C))
    x = np.clip(x + rng.integers(0, noise, x.shape), 0, 255).astype(np.uint8)
    y = np.where(rng.random(N) < 0.15, rng.integers(0, K, N), y)   # label noise: the classes overlap
    return x.reshape(N, -1), y.astype(np.int64)


# (N, H, W, C, K, held-out rows): the three fit problems
PROBLEMS = [(1200, 32, 32, 1, 3, 600), (256, 32, 32, 3, 2, 400), (96, 64, 64, 3, 2, 200)]


@functools.lru_cache(maxsize=None)
def host_fit(i):
    """(classifier fitted on the host, report, P on the held-out rows as float64 numpy, train (x, y), held-out (x, y)) of
    PROBLEMS[i]; computed once and left unchanged."""
    from csl_gan_amd import classify
    N, H, W, C, K, M = PROBLEMS[i]
    x, y = make(N, H, W, C, K, 1)
    xt, yt = make(M, H, W, C, K, 2)
    clf = classify.OvrLogReg(K)
    rep = clf.fit_bytes(x, y)
    return clf, rep, clf.predict_proba_bytes(xt).numpy(), (x, y), (xt, yt)


def write_cache(path, x, y, H, W, C):
    from csl_gan_amd import pipeline
    u8p, labp, hdrp = pipeline.cache_paths(path)
    np.save(open(u8p, "wb"), np.ascontiguousarray(x).reshape(len(x), H, W, C))
    np.save(labp, np.asarray(y, dtype=np.int64))
    with open(hdrp, "w") as f:
        json.dump({"version": pipeline.CACHE_VERSION, "n": len(x), "H": H, "W": W, "C": C, "signed": False, "dtype": "uint8", "layout": "NHWC"}, f)
    return path


def make_caches(root):
    """syn (300), syn2 (300, another seed), test (200), train (240): 32x32x1, K = 3."""
    out = {}
    for name, n, seed in (("syn", 300, 1), ("syn2", 300, 3), ("test", 200, 2), ("train", 240, 4)):
        x, y = make(n, 32, 32, 1, 3, seed)
        out[name] = (write_cache(os.path.join(str(root), name), x, y, 32, 32, 1), x, y)
    return out


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    return make_caches(tmp_path_factory.mktemp("tstr_caches"))


# ---- the library ------------------------------------------------------------------------------------------------------------------------

def test_objective_host_bytes_equals_objective_host():
    """Row blocks of 1, 7 and >= N against the one-matrix form on bytes / 255: 1e-12 of the largest entry (float64 sums in another
    order); then the loss by its formula in numpy and four gradient entries by central differences of it."""
    from csl_gan_amd import classify
    rng = np.random.default_rng(5)
    N, D, K = 50, 930, 10
    Xb = rng.integers(0, 256, (N, D)).astype(np.uint8)
    Xb[:, ::7] = 0
    y = rng.integers(0, K, N)
    U = rng.standard_normal((D + 1, K)) * (0.5 / np.sqrt(D))
    l0, g0 = classify.objective_host(torch.from_numpy(Xb).double() / 255, y, U)
    for block in (1, 7, 50, 4096):
        l, g = classify.objective_host_bytes(Xb, y, U, block=block)
        assert l.dtype == torch.float64 and g.dtype == torch.float64 and l.shape == (K,) and g.shape == (D + 1, K)
        assert float((l - l0).abs().max()) <= 1e-12 * float(l0.abs().max()), block
        assert float((g - g0).abs().max()) <= 1e-12 * float(g0.abs().max()), block
    X = Xb.astype(np.float64) / 255

    def f(U):
        z = X @ U[:D] + U[D]
        s = 2.0 * (y[:, None] == np.arange(K)[None]) - 1
        return np.logaddexp(0, -s * z).sum(0) + (U[:D] ** 2).sum(0) / 4

    l, g = classify.objective_host_bytes(Xb, y, U)
    assert np.abs(l.numpy() - f(U)).max() < 1e-10
    for d, k in ((1, 0), (17, 3), (929, 9), (930, 5)):
        E = np.zeros_like(U)
        E[d, k] = 1e-5
        assert abs((f(U + E)[k] - f(U - E)[k]) / 2e-5 - float(g[d, k])) < 1e-5
    with pytest.raises(ValueError, match="uint8"):
        classify.objective_host_bytes(X, y, U)


def test_fit_bytes_on_the_host():
    """1200 x 1024, K = 3: converges without a stall; the probabilities equal those of `fit` on the float64 bytes / 255 matrix to 1e-9
    (the same objective summed in another order, both stopped at max|g| <= 1e-8 N); a second fit returns the same bits."""
    from csl_gan_amd import classify
    clf, rep, P, (x, y), (xt, yt) = host_fit(0)
    assert all(rep["converged"]) and not any(rep["stalled"]) and rep["gtol_rel"] == classify.GTOL_REL_HOST
    assert P.dtype == np.float64 and P.shape == (600, 3) and np.abs(P.sum(1) - 1).max() < 1e-12
    ref = classify.OvrLogReg(3)
    rep_f = ref.fit(x.astype(np.float64) / 255, y)
    assert all(rep_f["converged"])
    Pf = ref.predict_proba(xt.astype(np.float64) / 255).numpy()
    err = float(np.abs(P - Pf).max())
    print("max|P_bytes - P_float| = %.3g  iterations %s" % (err, rep["iterations"]))
    assert err <= 1e-9
    again = classify.OvrLogReg(3)
    rep2 = again.fit_bytes(x, y)
    assert np.array_equal(again.coef.numpy().view(np.uint64), clf.coef.numpy().view(np.uint64)) and rep2 == rep
    a = classify.auroc(P, yt)
    acc = classify.accuracy(P, yt)
    print("micro-AUROC %.4f  accuracy %.4f" % (a["micro"], acc["accuracy"]))
    assert 0.85 < a["micro"] < 0.99 and 0.8 < acc["accuracy"] < 0.99          # neither trivial nor saturated


def test_fit_bytes_refusals():
    from csl_gan_amd import classify
    x, y = make(60, 8, 8, 1, 3, 1)
    with pytest.raises(ValueError, match="every class"):
        classify.OvrLogReg(4).fit_bytes(x, y)
    with pytest.raises(ValueError, match="every class"):
        classify.OvrLogReg(2).fit_bytes(x, y)                             # labels beyond the classes
    with pytest.raises(ValueError, match="uint8"):
        classify.OvrLogReg(3).fit_bytes(x.astype(np.float32), y)
    with pytest.raises(RuntimeError, match="fit first"):
        classify.OvrLogReg(3).predict_proba_bytes(x)


def test_accuracy_counts_argmax_hits_with_ties_to_the_smallest_class():
    from csl_gan_amd import classify
    P = np.array([[0.5, 0.5, 0.0],        # tie 0 / 1 -> 0
                  [0.2, 0.4, 0.4],        # tie 1 / 2 -> 1
                  [0.1, 0.2, 0.7],
                  [1 / 3, 1 / 3, 1 / 3],  # all equal -> 0
                  [0.6, 0.3, 0.1]])
    y = np.array([0, 2, 2, 1, 0])
    a = classify.accuracy(P, y)
    assert a == {"hits": 3, "n": 5, "accuracy": 0.6}
    assert classify.accuracy(torch.from_numpy(P).float(), torch.from_numpy(y)) == a
    assert classify.accuracy(P, np.array([1, 1, 2, 0, 0]))["hits"] == 4
    with pytest.raises(ValueError):
        classify.accuracy(P, y[:4])


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_cli_on_the_cpu(caches, tmp_path, capsys):
    from csl_gan_amd import classify, tstr
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    vals, outs = str(tmp_path / "vals"), str(tmp_path / "outs")
    res = tstr.main(["--syn_cache", syn, "--test_cache", test, "-d", "cpu", "--values_dir", vals, "--save", "--outputs_dir", outs])
    assert list(res) == ["syn"]
    m = res["syn"]
    clf = classify.OvrLogReg(3)
    rep = clf.fit_bytes(x, y)
    P = clf.predict_proba_bytes(xt)
    a, acc = classify.auroc(P, yt), classify.accuracy(P, yt)
    assert m["n_train"] == 300 and m["n_test"] == 200 and m["classes"] == 3
    assert m["auroc_micro"] == a["micro"] and m["auroc_per_class"] == a["per_class"]
    assert m["accuracy_hits"] == acc["hits"] and m["accuracy"] == acc["hits"] / 200 and m["solver"] == rep
    assert all(rep["converged"]) and 0.8 < a["micro"] < 1.0
    assert np.array_equal(np.load(os.path.join(vals, "syn_P.npy")), P.numpy())
    assert np.array_equal(np.load(os.path.join(vals, "syn_U.npy")), clf.coef.numpy())
    assert "syn: fitted on 300 rows, scored 200: AUROC %.6f" % a["micro"] in capsys.readouterr().out
    with open(os.path.join(outs, "tstr.json")) as f:
        assert json.load(f) == json.loads(json.dumps(res))

    # two synthetic caches and the baseline; --save merges into the same file
    syn2, train = caches["syn2"][0], caches["train"]
    res2 = tstr.main(["--syn_cache", syn, syn2, "--test_cache", test, "--train_cache", train[0], "--baseline", "--save", "--outputs_dir", outs,
                      "--name", "tstr"])
    assert list(res2) == ["syn", "syn2", "baseline_train"]
    assert res2["syn"] == m and res2["syn2"]["auroc_micro"] != m["auroc_micro"]
    assert res2["baseline_train"]["n_train"] == 240
    base = classify.OvrLogReg(3)
    base.fit_bytes(train[1], train[2])
    assert res2["baseline_train"]["accuracy_hits"] == classify.accuracy(base.predict_proba_bytes(xt), yt)["hits"]
    res3 = tstr.main(["--syn_cache", syn2, "--test_cache", test, "--save", "--outputs_dir", outs, "--max_iter", "3"])
    with open(os.path.join(outs, "tstr.json")) as f:
        merged = json.load(f)
    assert sorted(merged) == ["baseline_train", "syn", "syn2"]
    assert merged["syn"]["auroc_micro"] == m["auroc_micro"] and merged["syn2"]["solver"]["iterations"] == res3["syn2"]["solver"]["iterations"]
    assert max(res3["syn2"]["solver"]["iterations"]) <= 3


def test_cli_refusals(caches, tmp_path):
    from csl_gan_amd import tstr
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    d = str(tmp_path)
    with pytest.raises(SystemExit, match="give --train_cache"):
        tstr.main(["--syn_cache", syn, "--test_cache", test, "--baseline"])
    os.makedirs(os.path.join(d, "other"))
    twin = write_cache(os.path.join(d, "other", "syn"), x, y, 32, 32, 1)
    with pytest.raises(SystemExit, match="share the name"):
        tstr.main(["--syn_cache", syn, twin, "--test_cache", test])
    geo = write_cache(os.path.join(d, "geo"), x, y, 16, 64, 1)
    with pytest.raises(SystemExit, match="one geometry"):
        tstr.main(["--syn_cache", geo, "--test_cache", test])
    for name, labels, msg in (("uncond", np.zeros(300, dtype=np.int64), "K = 1 classes"),
                              ("many", np.arange(300) % 17, "K = 17 classes"),
                              ("gap", np.where(y == 1, 2, y), "every class 0 .. 2 needs a row")):
        p = write_cache(os.path.join(d, name), x, labels, 32, 32, 1)
        with pytest.raises(SystemExit, match=msg):
            tstr.main(["--syn_cache", p, "--test_cache", test])
    two = write_cache(os.path.join(d, "two"), x, y % 2, 32, 32, 1)
    with pytest.raises(SystemExit, match="test labels span 0 .. 2"):
        tstr.main(["--syn_cache", two, "--test_cache", test])
    with pytest.raises(SystemExit, match="K = 1 classes"):                # the baseline's cache is held to the same rules
        tstr.main(["--syn_cache", syn, "--test_cache", test, "--baseline", "--train_cache", os.path.join(d, "uncond")])


_SCORES = {"n_train", "n_test", "classes", "auroc_micro", "auroc_per_class", "accuracy", "accuracy_hits"}
STATS_KEYS = {"lr": _SCORES | {"solver"},
              "mlp": _SCORES | {"solver", "classifier", "hidden", "alpha", "seed"},
              "gnb": _SCORES | {"classifier", "fit", "var_smoothing"},
              "bnb": _SCORES | {"classifier", "fit", "alpha", "binarize"},
              "dt": _SCORES | {"classifier", "fit", "max_depth", "min_samples_split"},
              "rf": _SCORES | {"classifier", "fit", "max_depth", "min_samples_split", "n_trees", "max_features", "seed"},
              "ab": _SCORES | {"classifier", "fit", "n_rounds", "learning_rate"}}


def test_every_classifier_runs_through_the_table(caches):
    """The parser offers the table's keys, and every choice runs end to end and reports exactly the keys written down above."""
    from csl_gan_amd import tstr
    choices = [act.choices for act in tstr.build_parser()._actions if act.dest == "classifier"][0]
    assert list(choices) == list(tstr.ESTIMATORS) == list(STATS_KEYS)
    for k, keys in STATS_KEYS.items():
        res = tstr.main(["--syn_cache", caches["syn"][0], "--test_cache", caches["test"][0], "-d", "cpu", "--classifier", k, "--max_iter", "3",
                         "--hidden", "4", "--n_trees", "2", "--n_rounds", "3"])
        assert list(res) == ["syn"] and set(res["syn"]) == keys, k
        assert res["syn"].get("classifier", "lr") == k


# ---- the C-ABI entries validate on the host -----------------------------------------------------------------------------------------

def test_abi_entries_reject_bad_arguments_without_a_device():
    from csl_gan_amd import _lib, build
    build.build()
    L = _lib.lib()
    err = lambda: L.cslgan_last_error()
    wsf = L.cslgan_ovr_logreg_u8_ws_floats
    for n, d in ((0, 784), (-1, 784), (2 ** 31, 784), (10, 0), (10, -1), (10, 65537)):
        assert wsf(n, d) == 0, (n, d)
    for n, d in ((1, 1), (10, 896), (20, 65536), (10000, 12288), (162770, 12288)):
        assert wsf(n, d) > 0, (n, d)
    assert wsf(162770, 12288) * 4 < 64 * 2 ** 20                          # the residuals and at most 64 row chunks of partials
    N, D = 100, 930
    need = wsf(N, D)
    ok = dict(X=16, lab=16, U=16, N=N, D=D, K=10, loss=16, grad=16, ws=16)

    def ev(**kw):
        a = dict(ok, **kw)
        return L.cslgan_ovr_logreg_eval_u8(a["X"], a["lab"], a["U"], a["N"], a["D"], a["K"], a["loss"], a["grad"], a["ws"], kw.get("wsn", need), None)

    for name in ("X", "lab", "U", "loss", "grad", "ws"):
        assert ev(**{name: None}) == -1 and b"null" in err(), name
    for k in (1, 17):
        assert ev(K=k) == -1 and b"K=" in err()
    for d in (0, -1, 65537):
        assert ev(D=d) == -1 and b"D=" in err()
    for n in (0, 2 ** 31):
        assert ev(N=n) == -1 and b"N=" in err()
    assert ev(wsn=need - 1) == -1 and b"workspace" in err()
    assert ev(ws=20) == -1 and b"misaligned" in err()
    assert ev(X=17) == -1 and b"X misaligned" in err()

    def pr(X=16, U=16, M=10, D=930, K=10, P=16):
        return L.cslgan_ovr_logreg_proba_u8(X, U, M, D, K, P, None)

    for name in ("X", "U", "P"):
        assert pr(**{name: None}) == -1 and b"null" in err(), name
    for k in (1, 17):
        assert pr(K=k) == -1 and b"K=" in err()
    for d in (0, -1, 65537):
        assert pr(D=d) == -1 and b"D=" in err()
    assert pr(M=0) == -1 and b"M=" in err()
    assert pr(X=17) == -1 and b"misaligned" in err()


def test_ops_have_no_cpu_path():
    from csl_gan_amd import ops
    X, U = torch.zeros((8, 20), dtype=torch.uint8), torch.zeros(21, 3)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.ovr_logreg_eval_u8(X, torch.zeros(8, dtype=torch.int32), U)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.ovr_logreg_proba_u8(X, U)
