"""The device path of csl_gan_amd.classify / csl_gan_amd.downstream (-m gpu): cslgan_ovr_logreg_eval_f32 and
cslgan_ovr_logreg_proba_f32 against float64 numpy evaluations of the written formulas, the device fit against the vectors of
scikit-learn's own classes (tests/golden/downstream_lr.npz), the device AUROC against the host's by equality, and the command line
on cuda:0 against the same command on the CPU."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# one row | a ragged row tile of 16, D no multiple of 4, K padded to 16 | the MNIST D = 784 | a ragged tile with all 16 columns
SHAPES = [(1, 4, 2), (257, 50, 10), (512, 784, 10), (1000, 784, 16)]
MANY_TILES = (4200, 12, 3)          # 263 row tiles on 256 workgroups: some walk two tiles, the prefetch path with a ragged end


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _problem(N, D, K, big):
    """X in [0, 1] with zero columns, labels, U; big: logits of about +-80 in the first rows."""
    rng = np.random.default_rng(1000 * N + 10 * D + K)
    X = rng.random((N, D)).astype(np.float32)
    X[:, ::7] = 0.0
    X[rng.random((N, D)) < 0.3] = 0.0
    y = rng.integers(0, K, N).astype(np.int32)
    U = (rng.standard_normal((D + 1, K)) * (0.5 / np.sqrt(D))).astype(np.float32)
    if big:
        X[0, :] = 1.0
        U[:D] += np.float32(80.0 / D) * np.where(np.arange(K) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return X, y, U


@functools.lru_cache(maxsize=None)
def _expected_eval(N, D, K, big):
    X, y, U = (a.astype(np.float64) if a.dtype == np.float32 else a for a in _problem(N, D, K, big))
    Z = X @ U[:D] + U[D]
    T = (y[:, None] == np.arange(K)[None]).astype(np.float64)
    loss = np.logaddexp(0.0, -(2 * T - 1) * Z).sum(0) + (U[:D] ** 2).sum(0) / 4
    R = 1.0 / (1.0 + np.exp(-Z)) - T
    grad = np.concatenate([X.T @ R + U[:D] / 2, R.sum(0, keepdims=True)], 0)
    return loss, grad, Z


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("N,D,K", SHAPES + [MANY_TILES])
def test_eval_equals_the_float64_objective(N, D, K, big):
    """1e-3 of the largest |loss| / |grad| entry, the project's standing tolerance against reference-class vectors; the second call
    returns the same bits."""
    from csl_gan_amd import ops
    X, y, U = _problem(N, D, K, big)
    loss, grad, Z = _expected_eval(N, D, K, big)
    if big:
        assert np.abs(Z).max() > 75
    dX, dy, dU = _dev(X), _dev(y), _dev(U)
    l1, g1 = ops.ovr_logreg_eval(dX, dy, dU)
    l2, g2 = ops.ovr_logreg_eval(dX, dy, dU, out_loss=torch.full_like(l1, -1.0), out_grad=torch.full_like(g1, -1.0))
    a, b = l1.cpu().numpy(), g1.cpu().numpy()
    assert a.shape == (K,) and b.shape == (D + 1, K) and np.isfinite(a).all() and np.isfinite(b).all()
    el, eg = np.abs(a - loss).max() / np.abs(loss).max(), np.abs(b - grad).max() / np.abs(grad).max()
    print("(%d, %d, %d) big=%s: loss err %.2e, grad err %.2e" % (N, D, K, big, el, eg))
    assert el <= 1e-3 and eg <= 1e-3
    assert np.array_equal(a.view(np.uint32), l2.cpu().numpy().view(np.uint32))
    assert np.array_equal(b.view(np.uint32), g2.cpu().numpy().view(np.uint32))


def test_eval_on_rows_that_are_not_16_byte_aligned():
    """D % 4 == 0 but X starts 4 bytes into an allocation: the element-by-element loads."""
    from csl_gan_amd import ops
    N, D, K = 257, 52, 10
    X, y, U = _problem(N, D, K, False)
    loss, grad, _ = _expected_eval(N, D, K, False)
    buf = torch.zeros(N * D + 1, device="cuda")
    dX = buf[1:].view(N, D)
    dX.copy_(_dev(X))
    assert dX.data_ptr() % 16 == 4
    l, g = ops.ovr_logreg_eval(dX, _dev(y), _dev(U))
    assert np.abs(l.cpu().numpy() - loss).max() <= 1e-3 * np.abs(loss).max()
    assert np.abs(g.cpu().numpy() - grad).max() <= 1e-3 * np.abs(grad).max()


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_proba_equals_the_float64_formula(N, D, K):
    from csl_gan_amd import ops
    X, _, U = _problem(N, D, K, False)
    U = (U * 8).astype(np.float32)                                       # logits of a few units: probabilities that differ
    Xb = np.rint(X * 255).astype(np.uint8)
    for Xin, Xf in ((Xb, Xb.astype(np.float64) / 255.0), (X, X.astype(np.float64))):
        S = 1.0 / (1.0 + np.exp(-(Xf @ U[:D].astype(np.float64) + U[D].astype(np.float64))))
        exp = S / S.sum(1, keepdims=True)
        got = ops.ovr_logreg_proba(_dev(Xin), _dev(U)).cpu().numpy()
        assert got.shape == (N, K) and got.dtype == np.float32
        err = float(np.abs(got - exp).max())
        print("(%d, %d, %d) %s: proba err %.2e" % (N, D, K, Xin.dtype, err))
        assert err <= 1e-3
        assert np.abs(got.sum(1) - 1).max() < 1e-5


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "downstream_lr.npz")))


@pytest.fixture(scope="module")
def device_fit(gold):
    from csl_gan_amd import classify
    clf = classify.OvrLogReg(10)
    report = clf.fit(_dev(gold["x_train"]), _dev(gold["y_train"]))
    P = clf.predict_proba(_dev(gold["x_test"]))
    torch.cuda.synchronize()
    return clf, report, P


def test_device_fit_equals_the_golden(gold, device_fit):
    """Every probability within 1e-3 of scikit-learn's converged fit at the default gtol_rel; no column stalled; the AUROCs within the
    share of pairs that a 1e-3 move can reorder.  (An fp32 emulation of the device evaluation on the host reaches 3.8e-5.)"""
    from csl_gan_amd import classify
    clf, report, P = device_fit
    err = float(np.abs(P.cpu().numpy().astype(np.float64) - gold["P_gold"]).max())
    print("device max|P - P_gold| = %.3g  iterations %s  evaluations %s  max|g| %s  gtol %.3g" % (
        err, report["iterations"], report["evaluations"], ["%.2g" % v for v in report["grad_norm"]], report["gtol"]))
    assert report["gtol_rel"] == classify.GTOL_REL_DEVICE
    assert err <= 1e-3
    assert not any(report["stalled"]) and all(report["converged"])
    a = classify.auroc(P, gold["y_test"])
    assert abs(a["micro"] - float(gold["auroc_micro"])) <= float(gold["auroc_slack"])
    for k in range(10):
        assert abs(a["per_class"][k] - float(gold["auroc_per_class"][k])) <= float(gold["auroc_slack_per_class"][k]), k


def test_device_auroc_equals_the_host_auroc_of_the_same_scores(gold, device_fit):
    from csl_gan_amd import classify
    _, _, P = device_fit
    assert P.is_cuda
    assert classify.auroc(P, gold["y_test"]) == classify.auroc(P.cpu().numpy(), gold["y_test"])
    t = np.load(os.path.join(GOLDEN, "downstream_ties.npz"))
    a = classify.auroc(_dev(t["scores"]), t["y"])
    assert a == classify.auroc(t["scores"], t["y"])
    assert abs(a["micro"] - float(t["auroc_micro"])) <= 1e-9


def test_device_fit_repeats_bit_for_bit(gold, device_fit):
    from csl_gan_amd import classify
    clf, report, _ = device_fit
    again = classify.OvrLogReg(10)
    rep2 = again.fit(_dev(gold["x_train"]), _dev(gold["y_train"]))
    assert torch.equal(again.coef, clf.coef) and rep2 == report


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def _close_pair_share(pos, neg, gap):
    sn = np.sort(neg)
    lo, hi = np.searchsorted(sn, pos - gap, side="right"), np.searchsorted(sn, pos + gap, side="left")
    return float((hi - lo).sum()) / (len(pos) * len(neg))


def test_cli_on_the_device_agrees_with_the_cpu(tmp_path, monkeypatch):
    """The slack is computed here from the CPU run's scores: the share of positive-negative pairs closer than 2e-3, the only pairs
    whose order can change when every probability moves by at most 1e-3."""
    from csl_gan_amd import classify, downstream, init_util, options, pipeline, util
    out = str(tmp_path) + "/"
    opt = options.parse(["MNIST", "-cond", "-o", out, "--manual_seed", "77", "--synthetic"])
    with open(out + "opt.txt", "w") as f:
        json.dump(opt.__dict__, f)
    G, _ = init_util.init_models(opt, init_D=False)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in G.parameters():
            p.mul_(1.5).add_(torch.randn(p.shape, generator=g) * 0.05)
    util.save_model(3, G, torch.optim.Adam(G.parameters()), 0, out + "saves/G-3")
    rng = np.random.default_rng(8)
    y = np.arange(300) % 10
    x = np.zeros((300, 28, 28, 1), dtype=np.uint8)
    for i, k in enumerate(y):                                            # a blob per class, then noise
        r, c = 4 + 2 * (k // 3), 4 + 6 * (k % 3)
        x[i, r:r + 8, c:c + 8, 0] = rng.integers(100, 256, (8, 8))
    x = np.clip(x.astype(np.int64) + rng.integers(0, 40, x.shape), 0, 255).astype(np.uint8)
    u8p, labp, hdrp = pipeline.cache_paths(out + "tc")
    np.save(open(u8p, "wb"), x)
    np.save(labp, y.astype(np.int64))
    with open(hdrp, "w") as f:
        json.dump({"version": pipeline.CACHE_VERSION, "n": 300, "H": 28, "W": 28, "C": 1, "signed": False, "dtype": "uint8", "layout": "NHWC"}, f)

    scores, real = {}, classify.auroc

    def keeping(P, yy):
        scores[str(P.device)] = P.cpu().numpy().astype(np.float64)
        return real(P, yy)

    monkeypatch.setattr(classify, "auroc", keeping)
    args = [out, "-e", "3", "-n", "512", "-bs", "128", "--hip_graph", "true", "--test_cache", out + "tc"]
    dev = downstream.main(args + ["-d", "cuda:0"])[3]
    cpu = downstream.main(args + ["-d", "cpu"])[3]
    assert not any(dev["solver"]["stalled"]) and all(dev["solver"]["converged"])
    Pc, Pd = scores["cpu"], scores["cuda:0"]
    dp = float(np.abs(Pc - Pd).max())
    hot = y[:, None] == np.arange(10)[None]
    slack = _close_pair_share(Pc[hot], Pc[~hot], 2e-3)
    print("max|P_cpu - P_dev| = %.3g  AUROC cpu %.6f dev %.6f  slack %.3g" % (dp, cpu["micro"], dev["micro"], slack))
    assert dp <= 1e-3
    assert abs(cpu["micro"] - dev["micro"]) <= slack
    lines = open(out + "downstream_log.csv").read().splitlines()
    assert lines[0] == "Epoch,lr AUROC" and len([r for r in lines if r.startswith("3,")]) == 2
