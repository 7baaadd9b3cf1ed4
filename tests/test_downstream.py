"""csl_gan_amd.classify / csl_gan_amd.downstream on the CPU: the host estimator against vectors made by scikit-learn's own classes
(tests/golden/make_downstream_golden.py), the AUROC against roc_curve + auc on tied and untied scores, the refusals, repeatability,
the command line end to end on a tiny saved generator, and the host-side argument checks of the two C-ABI entries behind the device
path (no launch, no device needed)."""
import csv
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "downstream_lr.npz")))


@pytest.fixture(scope="module")
def host_fit(gold):
    from csl_gan_amd import classify
    clf = classify.OvrLogReg(10)
    report = clf.fit(gold["x_train"], gold["y_train"])
    return clf, report


def test_fixture_is_what_the_tests_lean_on(gold):
    x = gold["x_train"]
    assert x.dtype == np.float32 and x.shape == (600, 64) and x.min() >= 0 and x.max() <= 1
    assert len(gold["zero_cols"]) == 6 and not x[:, gold["zero_cols"]].any()
    assert gold["x_test"].dtype == np.uint8 and gold["x_test"].shape == (400, 64)
    assert set(gold["y_train"].tolist()) == set(range(10))
    assert 0.85 < float(gold["auroc_micro"]) < 0.995 and float(gold["auroc_slack"]) <= 0.01 and float(gold["c2_gap"]) <= 1e-4


def test_host_probabilities_equal_the_golden(gold, host_fit):
    """1e-4: scikit-learn's two formulations of the estimator agree to 8e-6 and a float64 prototype reached 2.3e-6."""
    clf, report = host_fit
    assert all(report["converged"]) and not any(report["stalled"])
    P = clf.predict_proba(gold["x_test"]).numpy()
    assert P.dtype == np.float64 and P.shape == (400, 10)
    err = float(np.abs(P - gold["P_gold"]).max())
    print("host max|P - P_gold| = %.3g, iterations %s, evaluations %s" % (err, report["iterations"], report["evaluations"]))
    assert err <= 1e-4
    assert np.abs(P.sum(1) - 1).max() < 1e-12
    # the same rows as floats: bytes / 255 is the scaling
    P2 = clf.predict_proba(gold["x_test"].astype(np.float64) / 255.0).numpy()
    assert np.abs(P2 - P).max() < 1e-12


def test_objective_host_is_the_written_objective(gold):
    """Loss by its formula in plain numpy, gradient by central differences of it."""
    from csl_gan_amd import classify
    rng = np.random.default_rng(3)
    X, y = gold["x_train"][:50].astype(np.float64), gold["y_train"][:50]
    U = rng.standard_normal((65, 10)) * 0.3

    def f(U):
        z = X @ U[:64] + U[64]
        s = 2.0 * (y[:, None] == np.arange(10)[None]) - 1
        return np.logaddexp(0, -s * z).sum(0) + (U[:64] ** 2).sum(0) / 4

    loss, grad = classify.objective_host(X, y, U)
    assert np.abs(loss.numpy() - f(U)).max() < 1e-10
    for d, k in ((0, 0), (17, 3), (63, 9), (64, 5)):
        E = np.zeros_like(U)
        E[d, k] = 1e-5
        assert abs((f(U + E)[k] - f(U - E)[k]) / 2e-5 - float(grad[d, k])) < 1e-5


def test_auroc_equals_roc_curve_auc(gold):
    from csl_gan_amd import classify
    a = classify.auroc(gold["P_gold"].astype(np.float32), gold["y_test"])
    assert abs(a["micro"] - float(gold["auroc_micro"])) <= 1e-9
    assert np.abs(np.array(a["per_class"]) - gold["auroc_per_class"]).max() <= 1e-9
    t = np.load(os.path.join(GOLDEN, "downstream_ties.npz"))
    assert len(np.unique(t["scores"])) < 20                          # ties decide
    a = classify.auroc(t["scores"], t["y"])
    assert abs(a["micro"] - float(t["auroc_micro"])) <= 1e-9
    assert np.abs(np.array(a["per_class"]) - t["auroc_per_class"]).max() <= 1e-9
    # tensors and arrays are the same thing
    b = classify.auroc(torch.from_numpy(t["scores"]), torch.from_numpy(t["y"]))
    assert a == b


def test_refusals(gold):
    from csl_gan_amd import classify
    for k in (1, 17, 0, -3):
        with pytest.raises(ValueError, match="n_classes"):
            classify.OvrLogReg(k)
    y = gold["y_train"].copy()
    y[y == 4] = 5
    with pytest.raises(ValueError, match="every class"):
        classify.OvrLogReg(10).fit(gold["x_train"], y)
    with pytest.raises(ValueError, match="every class"):
        classify.OvrLogReg(3).fit(gold["x_train"], gold["y_train"])          # labels beyond the classes
    with pytest.raises(RuntimeError, match="fit first"):
        classify.OvrLogReg(10).predict_proba(gold["x_test"])


def test_two_fits_give_identical_bits(gold, host_fit):
    from csl_gan_amd import classify
    clf, report = host_fit
    again = classify.OvrLogReg(10)
    rep2 = again.fit(gold["x_train"], gold["y_train"])
    assert np.array_equal(again.coef.numpy().view(np.uint64), clf.coef.numpy().view(np.uint64))
    assert rep2 == report


def test_frozen_columns_and_the_stall_report():
    """A quadratic per column, one of them already at its minimiser, one whose evaluation never decreases."""
    from csl_gan_amd import classify
    A = torch.tensor([1.0, 10.0, 3.0], dtype=torch.float64)
    target = torch.tensor([[1.0, -2.0, 0.0], [0.5, 4.0, 0.0]], dtype=torch.float64)

    def ev(U):
        d = U - target
        loss, grad = 0.5 * (A * d * d).sum(0), A * d
        loss[1] = 7.0 + (U[:, 1] - 0.0).abs().sum()                 # column 1: the loss grows along every direction its gradient offers
        return loss, grad

    U, rep = classify.lbfgs_columns(ev, torch.zeros((2, 3), dtype=torch.float64), 1, 1e-9, 50)
    assert rep["iterations"][2] == 0 and rep["evaluations"][2] == 1 and rep["converged"][2]
    assert rep["converged"][0] and not rep["stalled"][0] and torch.allclose(U[:, 0], target[:, 0], atol=1e-8)
    assert rep["stalled"][1] and not rep["converged"][1] and rep["iterations"][1] == 0 and torch.equal(U[:, 1], torch.zeros(2, dtype=torch.float64))


# ---- the command line on the CPU -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """An MNIST Vanilla conditional generator with non-default weights, saved twice as train.py saves it, next to its opt.txt, and a
    synthetic labelled test cache of blurred class blobs."""
    from csl_gan_amd import init_util, options, pipeline, util
    out = str(tmp_path_factory.mktemp("downstream_run")) + "/"
    opt = options.parse(["MNIST", "-cond", "-o", out, "--manual_seed", "77", "--synthetic"])
    with open(out + "opt.txt", "w") as f:
        json.dump(opt.__dict__, f)
    G, _ = init_util.init_models(opt, init_D=False)
    g = torch.Generator().manual_seed(5)
    for epoch in (2, 4):
        with torch.no_grad():
            for p in G.parameters():
                p.mul_(1.2).add_(torch.randn(p.shape, generator=g) * 0.05)
        util.save_model(epoch, G, torch.optim.Adam(G.parameters()), 0, out + "saves/G-%d" % epoch)
    rng = np.random.default_rng(8)
    y = np.arange(120) % 10
    x = np.zeros((120, 28, 28, 1), dtype=np.uint8)
    for i, k in enumerate(y):
        r, c = 4 + 2 * (k // 3), 4 + 6 * (k % 3)
        x[i, r:r + 8, c:c + 8, 0] = rng.integers(100, 256, (8, 8))
    x = np.clip(x.astype(np.int64) + rng.integers(0, 40, x.shape), 0, 255).astype(np.uint8)
    cache = out + "test_cache"
    u8p, labp, hdrp = pipeline.cache_paths(cache)
    np.save(open(u8p, "wb"), x)
    np.save(labp, y.astype(np.int64))
    with open(hdrp, "w") as f:
        json.dump({"version": pipeline.CACHE_VERSION, "n": 120, "H": 28, "W": 28, "C": 1, "signed": False, "dtype": "uint8", "layout": "NHWC"}, f)
    return out, cache


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_cli_on_the_cpu(run_dir, capsys):
    from csl_gan_amd import downstream
    out, cache = run_dir
    args = [out, "-d", "cpu", "-n", "200", "-bs", "64", "--test_cache", cache]
    res = downstream.main(args + ["-ei", "2"])
    assert sorted(res) == [2, 4]                                      # G-6 is missing: the loop ends there
    rows = _rows(out + "downstream_log.csv")
    assert rows[0] == ["Epoch", "lr AUROC"] and [r[0] for r in rows[1:]] == ["2", "4"]
    for r in rows[1:]:
        assert float(r[1]) == res[int(r[0])]["micro"] and 0.0 <= float(r[1]) <= 1.0
    for e in (2, 4):
        assert len(res[e]["per_class"]) == 10 and all(res[e]["solver"]["converged"])
    assert res[2]["micro"] != res[4]["micro"]                         # another checkpoint, another figure
    assert "lr AUROC (2):  %s" % res[2]["micro"] in capsys.readouterr().out
    # a second run appends; one epoch; another batch size and the same samples -> the same figure up to the generator's batch rounding
    res2 = downstream.main([out, "-d", "cpu", "-n", "200", "-bs", "50", "--test_cache", cache, "-e", "4"])
    rows = _rows(out + "downstream_log.csv")
    assert len(rows) == 5 and rows[3] == ["Epoch", "lr AUROC"] and rows[4][0] == "4"
    assert abs(res2[4]["micro"] - res[4]["micro"]) < 1e-3


def test_cli_refusals(run_dir, tmp_path):
    from csl_gan_amd import downstream, options
    out, cache = run_dir
    with pytest.raises(SystemExit, match="only the logistic regression is built"):
        downstream.main([out, "-d", "cpu", "-c", "svm"])
    with pytest.raises(SystemExit, match="only the logistic regression is built"):
        downstream.main([out, "-d", "cpu", "-c", "lr", "mlp"])
    with pytest.raises(SystemExit):
        downstream.main([out, "-d", "cpu", "-c", "xgboost"])             # no name of the reference's list
    for argv, msg in ((["CelebA", "-cond"], "only implemented for MNIST"), (["MNIST"], "conditional generator")):
        d = str(tmp_path / argv[0]) + ("c/" if len(argv) > 1 else "u/")
        os.makedirs(d)
        opt = options.parse(argv + ["-o", d, "--synthetic"])
        with open(d + "opt.txt", "w") as f:
            json.dump(opt.__dict__, f)
        with pytest.raises(SystemExit, match=msg):
            downstream.main([d, "-d", "cpu", "--test_cache", cache])


# ---- the C-ABI entries validate on the host -------------------------------------------------------------------------------------------

def test_abi_entries_reject_bad_arguments_without_a_device():
    from csl_gan_amd import _lib, build
    build.build()
    L = _lib.lib()
    err = lambda: L.cslgan_last_error()
    ok = dict(X=16, lab=16, U=16, N=100, D=784, K=10, loss=16, grad=16, ws=16)
    need = L.cslgan_ovr_logreg_ws_floats(100, 784)
    assert need == 7 * (800 * 16 + 32)                                # 7 row tiles, one partial each: [800, 16] floats + 16 doubles
    assert L.cslgan_ovr_logreg_ws_floats(10 ** 6, 784) == 256 * (800 * 16 + 32)
    assert L.cslgan_ovr_logreg_ws_floats(0, 784) == 0 and L.cslgan_ovr_logreg_ws_floats(10, 0) == 0 and L.cslgan_ovr_logreg_ws_floats(10, 896) == 0

    def ev(**kw):
        a = dict(ok, **kw)
        return L.cslgan_ovr_logreg_eval_f32(a["X"], a["lab"], a["U"], a["N"], a["D"], a["K"], a["loss"], a["grad"], a["ws"], kw.get("wsn", need), None)

    for name in ("X", "lab", "U", "loss", "grad", "ws"):
        assert ev(**{name: None}) == -1 and b"null" in err(), name
    for k in (1, 0, 17):
        assert ev(K=k) == -1 and b"K=" in err()
    for d in (0, -1, 896):
        assert ev(D=d) == -1 and b"D=" in err()
    for n in (0, -5, 2 ** 31):
        assert ev(N=n) == -1 and b"N=" in err()
    assert ev(wsn=need - 1) == -1 and b"workspace" in err()
    assert ev(ws=20) == -1 and b"misaligned" in err()

    def pr(X=16, u8=0, U=16, M=10, D=784, K=10, P=16):
        return L.cslgan_ovr_logreg_proba_f32(X, u8, U, M, D, K, P, None)

    for name in ("X", "U", "P"):
        assert pr(**{name: None}) == -1 and b"null" in err(), name
    assert pr(K=1) == -1 and b"K=" in err() and pr(K=17) == -1
    assert pr(D=0) == -1 and b"D=" in err()
    assert pr(M=0) == -1 and b"M=" in err()
    assert pr(u8=2) == -1 and b"is_u8" in err()
    assert pr(X=18, u8=0) == -1 and b"misaligned" in err()


def test_ops_have_no_cpu_path(gold):
    from csl_gan_amd import ops
    X, U = torch.from_numpy(gold["x_train"]), torch.zeros(65, 10)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.ovr_logreg_eval(X, torch.from_numpy(gold["y_train"]).int(), U)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.ovr_logreg_proba(torch.from_numpy(gold["x_test"]), U)
