"""The device path of csl_gan_amd.classify.OvrMlp (-m gpu): cslgan_ovr_mlp_eval_u8 and cslgan_ovr_mlp_proba_u8 against
the float64 definition, their refusals through ops, the device fit against the host fit over a short horizon, a long device fit
judged on its own, and `tstr --classifier mlp` on cuda:0.

ReLU's derivative jumps at 0, so no assertion here depends on the sign of a pre-activation that float64 places within
1e-5 max|Z1| of zero.  Large shapes make the signs exact: W1 holds multiples of 1/64 in [-1/16, 1/16] (in [-1/64, 1/64] for
D = 65536) and b1 = 0, so every partial sum of bytes times weights is an integer multiple of 1/64 below 2^24 / 64 — exact in fp32 in
any order, an exact zero included.  Small shapes take general weights and a non-zero b1 from a fixed seed and ASSERT that margin on
the float64 pre-activations before the device is looked at."""
import functools
import os

import numpy as np
import pytest
import torch

from csl_gan_amd.classify import OvrMlp, accuracy, objective_mlp_host_bytes, proba_mlp_host_bytes

from test_mlp import XOR_BAR, xor_host_fit, xor_problem
from test_tstr import PROBLEMS, make, make_caches

pytestmark = pytest.mark.gpu

# (N, D, K, H): smallest | C = 21, everything ragged | C = 256, aligned rows
GENERAL = [(1, 1, 2, 1), (17, 5, 3, 7), (64, 896, 16, 16)]
# C = 1000: a ragged column tile, unaligned rows | CelebA's row | the widest row | 1026 row blocks on 1024 workgroups, a ragged last
# block and a ragged last chunk of the gradient pass | C = 2048, the widest
EXACT = [(257, 930, 10, 100), (100, 12288, 2, 100), (20, 65536, 2, 16), (65637, 12, 3, 5), (33, 48, 16, 128)]
SHAPES = GENERAL + EXACT
OUTSIDE = (64, 896, 16, 16)         # the shape that also runs with labels outside 0 .. K-1
MARGIN = 1e-5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _problem(N, D, K, H, outside=False):
    """Bytes with zero columns and one row of 255s, labels, U (float32).  The regime follows the shape (the module docstring)."""
    rng = np.random.default_rng(1000 * N + 10 * D + K + H)
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    X[:, ::7] = 0
    X[rng.random((N, D)) < 0.3] = 0
    X[0, :] = 255
    y = (rng.integers(-2, K + 2, N) if outside else rng.integers(0, K, N)).astype(np.int32)
    U = np.zeros(((D + 2) * H + 1, K), dtype=np.float32)
    if (N, D, K, H) in EXACT:
        top = 1 if D > 12288 else 4
        assert D * 255 * top < 2 ** 24
        U[:D * H] = rng.integers(-top, top + 1, (D * H, K)).astype(np.float32) / 64
    else:
        U[:D * H] = rng.standard_normal((D * H, K)) / np.sqrt(D)
        U[D * H:(D + 1) * H] = 0.3 * rng.standard_normal((H, K))
    U[(D + 1) * H:(D + 2) * H] = rng.standard_normal((H, K)) * (2 / np.sqrt(H))
    U[-1] = 0.5 * rng.standard_normal(K)
    return X, y, U


@functools.lru_cache(maxsize=None)
def _expected(N, D, K, H, alpha, outside=False):
    """(loss, grad) of the float64 definition as numpy; for the general regime the margin is asserted first."""
    X, y, U = _problem(N, D, K, H, outside)
    if (N, D, K, H) in GENERAL:
        Z1 = (X.astype(np.float64) @ U[:D * H].astype(np.float64).reshape(D, H * K)) / 255 + U[D * H:(D + 1) * H].astype(np.float64).reshape(-1)
        assert np.abs(Z1).min() >= MARGIN * np.abs(Z1).max(), (np.abs(Z1).min(), np.abs(Z1).max())
    loss, grad = objective_mlp_host_bytes(X, y, U, H, alpha)
    return loss.numpy(), grad.numpy()


def _check_eval(N, D, K, H, alpha, outside=False):
    from csl_gan_amd import ops
    X, y, U = _problem(N, D, K, H, outside)
    loss, grad = _expected(N, D, K, H, alpha, outside)
    dX, dy, dU = _dev(X), _dev(y), _dev(U)
    ws = torch.full((ops.ovr_mlp_u8_ws_floats(N, D, K, H),), float("nan"), device="cuda")      # nothing may be read before written
    l1, g1 = ops.ovr_mlp_eval_u8(dX, dy, dU, H, alpha, ws=ws)
    l2, g2 = ops.ovr_mlp_eval_u8(dX, dy, dU, H, alpha, out_loss=torch.full_like(l1, -1.0), out_grad=torch.full_like(g1, -1.0))
    a, b = l1.cpu().numpy(), g1.cpu().numpy()
    assert a.shape == (K,) and b.shape == U.shape and np.isfinite(a).all() and np.isfinite(b).all()
    el, eg = np.abs(a - loss).max() / np.abs(loss).max(), np.abs(b - grad).max() / np.abs(grad).max()
    print("(%d, %d, %d, %d) alpha=%g outside=%s: loss err %.2e, grad err %.2e" % (N, D, K, H, alpha, outside, el, eg))
    assert el <= 1e-3 and eg <= 1e-3
    assert np.array_equal(a.view(np.uint32), l2.cpu().numpy().view(np.uint32))
    assert np.array_equal(b.view(np.uint32), g2.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("alpha", [1.0, 0.0])
@pytest.mark.parametrize("N,D,K,H", SHAPES)
def test_eval_u8_equals_the_float64_definition(N, D, K, H, alpha):
    """1e-3 of the largest |loss| and of the largest |grad| entry, the standing tolerance of these kernels; the workspace is handed
    over full of NaN; the second call returns the same bits.  Measured on an MI355X over all shapes: at most 6.7e-8 in a loss and
    2.4e-7 in a gradient."""
    _check_eval(N, D, K, H, alpha)


def test_eval_u8_with_labels_outside_the_classes():
    """Labels -2 .. K + 1: rows outside 0 .. K-1 are negatives of every class."""
    y = _problem(*OUTSIDE, True)[1]
    assert (y < 0).any() and (y >= OUTSIDE[2]).any()
    _check_eval(*OUTSIDE, 1.0, True)


@pytest.mark.parametrize("N,D,K,H", SHAPES)
def test_proba_u8_equals_the_float64_definition(N, D, K, H):
    """1e-3 absolute in P, rows summing to 1 within 1e-5.  Measured on an MI355X: at most 1.4e-7."""
    from csl_gan_amd import ops
    X, _, U = _problem(N, D, K, H)
    _expected(N, D, K, H, 1.0)                                             # the margin of the general regime
    exp = proba_mlp_host_bytes(X, U, H).numpy()
    got = ops.ovr_mlp_proba_u8(_dev(X), _dev(U), H).cpu().numpy()
    assert got.shape == (N, K) and got.dtype == np.float32
    err = float(np.abs(got - exp).max())
    print("(%d, %d, %d, %d): proba err %.2e" % (N, D, K, H, err))
    assert err <= 1e-3
    assert np.abs(got.sum(1) - 1).max() < 1e-5


def test_bad_arguments_raise():
    """D = 0, H = 129, K = 17, a misaligned X and a workspace of the wrong size: an exception each, nothing launched."""
    from csl_gan_amd import ops
    N, D, K, H = 17, 5, 3, 7
    X, y, U = (_dev(a) for a in _problem(N, D, K, H))
    y1 = y[:1].contiguous()
    for x, lab, u, h, match in ((torch.zeros((1, 0), dtype=torch.uint8, device="cuda"), y1, torch.zeros((2 * H + 1, K), device="cuda"), H, "D = 0"),
                                (X, y, torch.zeros(((D + 2) * 129 + 1, K), device="cuda"), 129, "hidden = 129"),
                                (X, y, torch.zeros(((D + 2) * H + 1, 17), device="cuda"), H, "K = 17")):
        with pytest.raises(RuntimeError, match=match):
            ops.ovr_mlp_eval_u8(x, lab, u, h)
    # an empty tensor has no address, so D = 0 reaches the entry as a null pointer: refused all the same
    for x, u, h, match in ((torch.zeros((1, 0), dtype=torch.uint8, device="cuda"), torch.zeros((2 * H + 1, K), device="cuda"), H, "D=0|null"),
                           (X, torch.zeros(((D + 2) * 129 + 1, K), device="cuda"), 129, "H=129"),
                           (X, torch.zeros(((D + 2) * H + 1, 17), device="cuda"), H, "K=17")):
        with pytest.raises(RuntimeError, match=match):
            ops.ovr_mlp_proba_u8(x, u, h)
    shifted = torch.zeros(N * D + 16, dtype=torch.uint8, device="cuda")[1:1 + N * D].view(N, D)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 1
    with pytest.raises(RuntimeError, match="X misaligned"):
        ops.ovr_mlp_eval_u8(shifted, y, U, H)
    with pytest.raises(RuntimeError, match="misaligned"):
        ops.ovr_mlp_proba_u8(shifted, U, H)
    need = ops.ovr_mlp_u8_ws_floats(N, D, K, H)
    for n in (need - 1, need + 1):
        with pytest.raises(RuntimeError, match="workspace of %d floats, need %d" % (n, need)):
            ops.ovr_mlp_eval_u8(X, y, U, H, ws=torch.empty(n, device="cuda"))
    with pytest.raises(RuntimeError, match="need X"):
        ops.ovr_mlp_eval_u8(X, y, U[:-1].contiguous(), H)
    with pytest.raises(RuntimeError, match="alpha"):
        ops.ovr_mlp_eval_u8(X, y, U, H, alpha=-1.0)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _celeba_sized():
    """The (96 x 12288, K = 2) problem of tests/test_tstr.py with its 200 held-out rows."""
    N, H, W, C, K, M = PROBLEMS[2]
    return make(N, H, W, C, K, 1), make(M, H, W, C, K, 2)


@pytest.mark.parametrize("name", ["xor", "celeba_sized"])
def test_short_device_fit_equals_the_host_fit(name):
    """OvrMlp(2, hidden=16, max_iter=5) on the device and on the host: max|U_dev - U_host| <= 1e-3 max|U_host| and
    max|P_dev - P_host| <= 1e-3.  A float32 host model of the evaluation under the same solver ends 2e-7 .. 6e-7 from the float64 run
    in U and 1e-7 .. 2e-7 in P after 5 iterations, which leaves three orders of magnitude for another summation order.  Long fits
    are not compared entry by entry: the objective is not convex, and the same pair is 4 apart in U after 500 iterations.
    Measured on an MI355X: 2.2e-7 / 9.0e-8 (XOR) and 1.9e-6 / 6.4e-7 (96 x 12288)."""
    (x, y), (xt, _) = xor_problem() if name == "xor" else _celeba_sized()
    if name == "xor":
        host, _, Ph = xor_host_fit(5)
    else:
        host = OvrMlp(2, hidden=16, max_iter=5)
        host.fit_bytes(x, y)
        Ph = host.predict_proba_bytes(xt).numpy()
    dev = OvrMlp(2, hidden=16, max_iter=5)
    rep = dev.fit_bytes(_dev(x), _dev(y))
    Pd = dev.predict_proba_bytes(_dev(xt))
    assert dev.coef.is_cuda and dev.coef.dtype == torch.float32 and Pd.is_cuda and Pd.dtype == torch.float32
    Uh = host.coef.numpy()
    eu = float(np.abs(dev.coef.cpu().numpy().astype(np.float64) - Uh).max()) / float(np.abs(Uh).max())
    ep = float(np.abs(Pd.cpu().numpy().astype(np.float64) - Ph).max())
    print("%s: iterations %s (host %s)  max|U_dev - U_host| / max|U_host| = %.3g  max|P_dev - P_host| = %.3g" % (
        name, rep["iterations"], host.report["iterations"], eu, ep))
    assert eu <= 1e-3 and ep <= 1e-3


def test_long_device_fit_judged_on_its_own():
    """The XOR problem at max_iter = 200 on the device: the float64 host objective at the returned U equals the reported loss to
    1e-3 relative per class, that loss lies below the loss at the initial point, the hits on the 400 test rows reach H* (the CPU
    test's bar), and a second fit returns the same bits and the same report.  Measured on an MI355X: 200 iterations and 305
    evaluations per class, losses 292.504 / 338.989 (float64 at U within 9e-8; 573.4 / 755.5 at the initial point), 316 hits."""
    (x, y), (xt, yt) = xor_problem()
    dx, dy = _dev(x), _dev(y)
    clf = OvrMlp(2, hidden=16, max_iter=200)
    rep = clf.fit_bytes(dx, dy)
    loss, _ = objective_mlp_host_bytes(x, y, clf.coef.cpu().double(), 16, 1.0)
    loss0, _ = objective_mlp_host_bytes(x, y, clf.initial_point(64), 16, 1.0)
    hits = accuracy(clf.predict_proba_bytes(_dev(xt)), yt)["hits"]
    print("iterations %s  evaluations %s  loss %s (float64 at U: %s; initial %s)  hits %d / 400" % (
        rep["iterations"], rep["evaluations"], rep["loss"], loss.tolist(), loss0.tolist(), hits))
    for k in range(2):
        assert abs(rep["loss"][k] - float(loss[k])) <= 1e-3 * float(loss[k])
        assert rep["loss"][k] < float(loss0[k])
    assert hits >= XOR_BAR
    again = OvrMlp(2, hidden=16, max_iter=200)
    rep2 = again.fit_bytes(dx, dy)
    assert torch.equal(again.coef, clf.coef) and rep2 == rep


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_cli_with_the_mlp_on_the_device(tmp_path):
    """`tstr --classifier mlp -d cuda:0 --baseline` on the blob caches of tests/test_tstr.py (K = 3, 200 test rows).  Each line's
    bar is derived as H* is: the midpoint between what needs no learning (the count of the most frequent test label) and the hit
    count M of the same line of the `-d cpu` run.  The two runs' hit counts are not compared for equality.  Measured on an
    MI355X: 176 / 200 on both lines on both paths, bar 125."""
    from csl_gan_amd import tstr
    c = make_caches(tmp_path)
    yt = c["test"][2]
    floor = int(np.bincount(yt).max())
    args = ["--syn_cache", c["syn"][0], "--test_cache", c["test"][0], "--train_cache", c["train"][0], "--baseline", "--classifier", "mlp",
            "--hidden", "16", "--max_iter", "30"]
    dev = tstr.main(args + ["-d", "cuda:0", "--values_dir", str(tmp_path / "dev")])
    cpu = tstr.main(args + ["-d", "cpu"])
    assert list(dev) == list(cpu) == ["syn", "baseline_train"]
    for lab in dev:
        d, h = dev[lab], cpu[lab]
        assert (d["classifier"], d["hidden"], d["alpha"], d["seed"]) == ("mlp", 16, 1.0, 0)
        assert (d["n_train"], d["n_test"], d["classes"]) == (h["n_train"], h["n_test"], h["classes"])
        assert np.load(os.path.join(str(tmp_path / "dev"), lab + "_U.npy")).shape == ((1024 + 2) * 16 + 1, 3)
        bar = (floor + h["accuracy_hits"] + 1) // 2
        print("%s: hits device %d, host %d, most frequent label %d, bar %d" % (lab, d["accuracy_hits"], h["accuracy_hits"], floor, bar))
        assert h["accuracy_hits"] > floor
        assert d["accuracy_hits"] >= bar
