"""The device path of csl_gan_amd.tstr (-m gpu): cslgan_ovr_logreg_eval_u8 and cslgan_ovr_logreg_proba_u8 against float64 numpy
evaluations of the written formulas on bytes / 255, the new entries beside the old ones on the same problem, the device fit on
bytes against the host fit, and the command line on cuda:0 against the same command on the CPU."""
import functools
import os

import numpy as np
import pytest
import torch

from test_tstr import PROBLEMS, host_fit, make_caches

pytestmark = pytest.mark.gpu

# one row, one column | D below one 16-byte load, a ragged row tile | the first D the fp32 entries refuse, all 16 columns | rows not
# 16-byte aligned, D no multiple of 4 | a 256-column slab plus a 16-column remainder | CelebA's row | the largest D
SHAPES = [(1, 1, 2), (17, 5, 3), (64, 896, 16), (257, 930, 10), (300, 1040, 2), (100, 12288, 2), (20, 65536, 16)]
# The forward pass runs at most 1024 workgroups of 64 rows: 65536 + 64 + 37 rows are 1026 row blocks, so workgroups 0 and 1 walk
# two and the last block is ragged.  The gradient pass cuts them into 64 chunks of 1040 rows, the last one of 117 (no multiple of 4).
MANY_ROWS = (65637, 12, 3)
OUTSIDE = (257, 930, 10)            # the shape that also runs with labels outside 0 .. K-1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _problem(N, D, K, big, outside=False):
    """Bytes with zero columns and one row of 255s, labels, U; big: logits of about +-80 in that row."""
    rng = np.random.default_rng(1000 * N + 10 * D + K)
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    X[:, ::7] = 0
    X[rng.random((N, D)) < 0.3] = 0
    X[0, :] = 255
    y = (rng.integers(-2, K + 2, N) if outside else rng.integers(0, K, N)).astype(np.int32)
    U = (rng.standard_normal((D + 1, K)) * (0.5 / np.sqrt(D))).astype(np.float32)
    if big:
        U[:D] += np.float32(80.0 / D) * np.where(np.arange(K) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return X, y, U


@functools.lru_cache(maxsize=None)
def _expected(N, D, K, big, outside=False):
    X, y, U = _problem(N, D, K, big, outside)
    X, U = X.astype(np.float64) / 255.0, U.astype(np.float64)
    Z = X @ U[:D] + U[D]
    T = (y[:, None] == np.arange(K)[None]).astype(np.float64)
    loss = np.logaddexp(0.0, -(2 * T - 1) * Z).sum(0) + (U[:D] ** 2).sum(0) / 4
    S = 0.5 * (1.0 + np.tanh(0.5 * Z))                                   # the sigmoid without overflow
    R = S - T
    grad = np.concatenate([X.T @ R + U[:D] / 2, R.sum(0, keepdims=True)], 0)
    return loss, grad, Z, S / S.sum(1, keepdims=True)


def _check_eval(N, D, K, big, outside=False):
    from csl_gan_amd import ops
    X, y, U = _problem(N, D, K, big, outside)
    loss, grad, Z, _ = _expected(N, D, K, big, outside)
    if big:
        assert np.abs(Z).max() > 75
    dX, dy, dU = _dev(X), _dev(y), _dev(U)
    ws = torch.full((ops.ovr_logreg_u8_ws_floats(N, D) + 2,), float("nan"), device="cuda")      # nothing may be read before written
    l1, g1 = ops.ovr_logreg_eval_u8(dX, dy, dU, ws=ws)
    l2, g2 = ops.ovr_logreg_eval_u8(dX, dy, dU, out_loss=torch.full_like(l1, -1.0), out_grad=torch.full_like(g1, -1.0))
    a, b = l1.cpu().numpy(), g1.cpu().numpy()
    assert a.shape == (K,) and b.shape == (D + 1, K) and np.isfinite(a).all() and np.isfinite(b).all()
    el, eg = np.abs(a - loss).max() / np.abs(loss).max(), np.abs(b - grad).max() / np.abs(grad).max()
    print("(%d, %d, %d) big=%s outside=%s: loss err %.2e, grad err %.2e" % (N, D, K, big, outside, el, eg))
    assert el <= 1e-3 and eg <= 1e-3
    assert np.array_equal(a.view(np.uint32), l2.cpu().numpy().view(np.uint32))
    assert np.array_equal(b.view(np.uint32), g2.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("N,D,K", SHAPES + [MANY_ROWS])
def test_eval_u8_equals_the_float64_objective(N, D, K, big):
    """1e-3 of the largest |loss| / |grad| entry, the standing tolerance of these kernels, for small logits and logits of +-80; the
    workspace is handed over full of NaN; the second call returns the same bits.  Measured on an MI355X over all shapes: at most
    4.1e-7 in a loss and 1.5e-7 in a gradient."""
    _check_eval(N, D, K, big)


def test_eval_u8_with_labels_outside_the_classes():
    """Labels -2 .. K + 1: rows outside 0 .. K-1 are negatives of every class."""
    y = _problem(*OUTSIDE, False, True)[1]
    assert (y < 0).any() and (y >= OUTSIDE[2]).any()
    _check_eval(*OUTSIDE, False, True)


@pytest.mark.parametrize("N,D,K", SHAPES + [MANY_ROWS])
def test_proba_u8_equals_the_float64_formula(N, D, K):
    """1e-3 absolute in P, rows summing to 1 within 1e-5.  Measured on an MI355X: at most 8.7e-7."""
    from csl_gan_amd import ops
    X, _, U = _problem(N, D, K, False)
    U8 = (U * 8).astype(np.float32)                                      # logits of a few units: probabilities that differ
    Z = (X.astype(np.float64) / 255.0) @ U8[:D].astype(np.float64) + U8[D].astype(np.float64)
    S = 1.0 / (1.0 + np.exp(-Z))
    exp = S / S.sum(1, keepdims=True)
    got = ops.ovr_logreg_proba_u8(_dev(X), _dev(U8)).cpu().numpy()
    assert got.shape == (N, K) and got.dtype == np.float32
    err = float(np.abs(got - exp).max())
    print("(%d, %d, %d): proba err %.2e" % (N, D, K, err))
    assert err <= 1e-3
    assert np.abs(got.sum(1) - 1).max() < 1e-5


def test_new_entries_beside_the_old_ones():
    """(512, 784, 10): the new entries on bytes and the old ones on bytes / 255 as fp32, both within 1e-3 of the same float64 values."""
    from csl_gan_amd import ops
    N, D, K = 512, 784, 10
    X, y, U = _problem(N, D, K, False)
    loss, grad, _, P = _expected(N, D, K, False)
    dXb, dXf, dy, dU = _dev(X), _dev((X.astype(np.float64) / 255.0).astype(np.float32)), _dev(y), _dev(U)
    for name, (l, g), p in (("u8", ops.ovr_logreg_eval_u8(dXb, dy, dU), ops.ovr_logreg_proba_u8(dXb, dU)),
                            ("f32", ops.ovr_logreg_eval(dXf, dy, dU), ops.ovr_logreg_proba(dXf, dU))):
        el = np.abs(l.cpu().numpy() - loss).max() / np.abs(loss).max()
        eg = np.abs(g.cpu().numpy() - grad).max() / np.abs(grad).max()
        ep = np.abs(p.cpu().numpy() - P).max()
        print("%s: loss err %.2e, grad err %.2e, proba err %.2e" % (name, el, eg, ep))
        assert el <= 1e-3 and eg <= 1e-3 and ep <= 1e-3


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------

def _close_pair_share(pos, neg, gap):
    sn = np.sort(neg)
    lo, hi = np.searchsorted(sn, pos - gap, side="right"), np.searchsorted(sn, pos + gap, side="left")
    return float((hi - lo).sum()) / (len(pos) * len(neg))


def _agree(Ph, Pd, yt, K, auc_h, auc_d, hits_h, hits_d):
    """The slacks of DESIGN.md §6j, computed from the HOST's scores: probabilities within 1e-3; AUROC within the share of
    positive-negative pairs closer than 2e-3; hit counts within the number of rows whose two largest probabilities are closer than
    2e-3, and that number below 2 % of the rows."""
    dp = float(np.abs(Ph - Pd).max())
    hot = yt[:, None] == np.arange(K)[None]
    slack = _close_pair_share(Ph[hot], Ph[~hot], 2e-3)
    top = np.sort(Ph, 1)
    close = int((top[:, -1] - top[:, -2] < 2e-3).sum())
    print("max|P_host - P_dev| = %.3g  AUROC host %.6f dev %.6f (slack %.3g)  hits host %d dev %d (close rows %d of %d)" % (
        dp, auc_h, auc_d, slack, hits_h, hits_d, close, len(yt)))
    assert dp <= 1e-3
    assert abs(auc_h - auc_d) <= slack
    assert close < 0.02 * len(yt)
    assert abs(hits_h - hits_d) <= close


@pytest.mark.parametrize("i", range(len(PROBLEMS)))
def test_device_fit_on_bytes_equals_the_host_fit(i):
    """The three problems of DESIGN.md §6j (1200 x 1024, K = 3; 256 x 3072, K = 2; 96 x 12288, K = 2): no class stalls, every class
    converges at the default gtol_rel, probabilities on the held-out rows within 1e-3 of the float64 host fit (a float32 model of the
    evaluation under the same solver ends 2.9e-6 / 9.2e-7 / 9.1e-8 away), AUROC and hit count within the slacks; a second device
    fit returns the same bits and the same report.  Measured on an MI355X: max|P_dev - P_host| = 3.6e-6 / 8.9e-7 / 1.4e-7, equal hit
    counts (544 / 371 / 190), AUROCs within 6e-6, no row with its two largest probabilities closer than 2e-3."""
    from csl_gan_amd import classify
    K = PROBLEMS[i][4]
    _, rep_h, Ph, (x, y), (xt, yt) = host_fit(i)
    assert all(rep_h["converged"]) and not any(rep_h["stalled"])
    clf = classify.OvrLogReg(K)
    rep = clf.fit_bytes(_dev(x), _dev(y))
    P = clf.predict_proba_bytes(_dev(xt))
    assert P.is_cuda and P.dtype == torch.float32
    print("iterations %s  evaluations %s  max|g| %s  gtol %.3g" % (rep["iterations"], rep["evaluations"], ["%.2g" % v for v in rep["grad_norm"]],
                                                                    rep["gtol"]))
    assert rep["gtol_rel"] == classify.GTOL_REL_DEVICE
    assert not any(rep["stalled"]) and all(rep["converged"])
    Pd = P.cpu().numpy().astype(np.float64)
    _agree(Ph, Pd, yt, K, classify.auroc(Ph, yt)["micro"], classify.auroc(P, yt)["micro"], classify.accuracy(Ph, yt)["hits"],
           classify.accuracy(P, yt)["hits"])
    again = classify.OvrLogReg(K)
    rep2 = again.fit_bytes(_dev(x), _dev(y))
    assert torch.equal(again.coef, clf.coef) and rep2 == rep


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_cli_on_the_device_agrees_with_the_cpu(tmp_path):
    """P from --values_dir within 1e-3, AUROC and accuracy within the slacks of _agree, for the synthetic cache and the baseline.
    Measured on an MI355X: max|P_dev - P_host| = 1.4e-6 and 4.2e-7, equal hit counts and AUROCs."""
    from csl_gan_amd import tstr
    c = make_caches(tmp_path)
    yt = c["test"][2]
    args = ["--syn_cache", c["syn"][0], "--test_cache", c["test"][0], "--train_cache", c["train"][0], "--baseline"]
    dev = tstr.main(args + ["-d", "cuda:0", "--values_dir", str(tmp_path / "dev")])
    cpu = tstr.main(args + ["-d", "cpu", "--values_dir", str(tmp_path / "cpu")])
    assert list(dev) == list(cpu) == ["syn", "baseline_train"]
    for lab in dev:
        d, h = dev[lab], cpu[lab]
        assert not any(d["solver"]["stalled"]) and all(d["solver"]["converged"])
        assert (d["n_train"], d["n_test"], d["classes"]) == (h["n_train"], h["n_test"], h["classes"])
        Ph = np.load(os.path.join(str(tmp_path / "cpu"), lab + "_P.npy")).astype(np.float64)
        Pd = np.load(os.path.join(str(tmp_path / "dev"), lab + "_P.npy")).astype(np.float64)
        assert np.load(os.path.join(str(tmp_path / "dev"), lab + "_U.npy")).shape == (1025, 3)
        _agree(Ph, Pd, yt, 3, h["auroc_micro"], d["auroc_micro"], h["accuracy_hits"], d["accuracy_hits"])
