"""csl_gan_amd.classify.OvrMlp and `tstr --classifier mlp` on the CPU: the float64 definition against autograd, its
row blocks, labels outside the classes, the solver, the XOR-of-blobs problem that a linear model cannot do, the command line with its
refusals, and the three C-ABI entries behind the device path (declared, exported, validating on the host; no launch, no device)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from csl_gan_amd.classify import OvrLogReg, OvrMlp, accuracy, objective_mlp_host_bytes, proba_mlp_host_bytes

from test_tstr import make_caches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The XOR problem, measured on the CPU (float64, OvrMlp(2, hidden=16, max_iter=200), seed 0 of the initial point):
XOR_SEED = 7            # seed of the problem
XOR_LR_CAP = 240        # a linear model stays at or below this many of the 400 test rows (the host logistic regression gets 223)
XOR_M = 327             # hits of the host float64 MLP
XOR_BAR = 284           # H*: the midpoint 283.5 between 240 and M, as a hit count


def xor_problem(seed=XOR_SEED, n_train=800, n_test=400, D=64):
    """XOR of blobs on bytes: two orthonormal directions u, v; row = 128 + 7.5 sqrt(D) (su u + sv v) + 25 noise, rounded and clipped
    to a byte; label [su sv > 0] with 10 % of the labels flipped.  ((x, y), (xt, yt))."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, 2)))
    u, v = Q[:, 0], Q[:, 1]

    def rows(n):
        su, sv = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
        x = 128 + 7.5 * np.sqrt(D) * (su[:, None] * u[None] + sv[:, None] * v[None]) + 25 * rng.standard_normal((n, D))
        y = (su * sv > 0).astype(np.int64)
        flip = rng.random(n) < 0.10
        return np.clip(np.rint(x), 0, 255).astype(np.uint8), np.where(flip, 1 - y, y)

    return rows(n_train), rows(n_test)


@functools.lru_cache(maxsize=None)
def xor_host_fit(max_iter):
    """(classifier, report, P on the test rows as float64 numpy) of OvrMlp(2, hidden=16, max_iter) on the host; computed once."""
    (x, y), (xt, _) = xor_problem()
    clf = OvrMlp(2, hidden=16, max_iter=max_iter)
    rep = clf.fit_bytes(x, y)
    return clf, rep, clf.predict_proba_bytes(xt).numpy()


def _random_case(N, D, K, H, seed=3, outside=False):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    y = rng.integers(-2, K + 2, N) if outside else rng.integers(0, K, N)
    U = rng.standard_normal(((D + 2) * H + 1, K)) * 0.3
    return X, y, U


def _autograd(X, y, U, H, alpha):
    """The loss formula of the issue, written without any code of the package, and its gradient by torch.autograd."""
    N, D = X.shape
    K = U.shape[1]
    U = torch.from_numpy(U).clone().requires_grad_()
    W1, b1 = U[:D * H].reshape(D, H, K), U[D * H:(D + 1) * H]
    w2, b2 = U[(D + 1) * H:(D + 2) * H], U[-1]
    x = torch.from_numpy(X).double() / 255
    Z1 = torch.einsum("id,dhk->ihk", x, W1) + b1
    z = (torch.relu(Z1) * w2).sum(1) + b2
    s = 2.0 * (torch.from_numpy(np.asarray(y))[:, None] == torch.arange(K)[None]).double() - 1
    f = torch.nn.functional.softplus(-s * z).sum(0) + 0.5 * alpha * ((W1 ** 2).sum((0, 1)) + (w2 ** 2).sum(0))
    g, = torch.autograd.grad(f.sum(), U)
    return f.detach(), g


# ---- the definition -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [1.0, 0.0])
@pytest.mark.parametrize("N,D,K,H", [(1, 1, 2, 1), (17, 5, 3, 7), (40, 64, 4, 16)])
def test_objective_against_autograd(N, D, K, H, alpha):
    """1e-10 of the largest entry."""
    X, y, U = _random_case(N, D, K, H)
    f, g = _autograd(X, y, U, H, alpha)
    loss, grad = objective_mlp_host_bytes(X, y, U, H, alpha)
    assert loss.dtype == torch.float64 and grad.dtype == torch.float64 and loss.shape == (K,) and grad.shape == U.shape
    assert float((loss - f).abs().max()) <= 1e-10 * float(f.abs().max())
    assert float((grad - g).abs().max()) <= 1e-10 * float(g.abs().max())


def test_row_blocks_agree():
    """Row blocks of 1, 7 and >= N: 1e-12 of the largest entry, for the objective and for P."""
    X, y, U = _random_case(40, 64, 4, 16)
    l0, g0 = objective_mlp_host_bytes(X, y, U, 16, 1.0, block=40)
    P0 = proba_mlp_host_bytes(X, U, 16, block=4096)
    for block in (1, 7, 4096):
        l, g = objective_mlp_host_bytes(X, y, U, 16, 1.0, block=block)
        assert float((l - l0).abs().max()) <= 1e-12 * float(l0.abs().max()), block
        assert float((g - g0).abs().max()) <= 1e-12 * float(g0.abs().max()), block
        assert float((proba_mlp_host_bytes(X, U, 16, block=block) - P0).abs().max()) <= 1e-12, block
    with pytest.raises(ValueError, match="uint8"):
        objective_mlp_host_bytes(X.astype(np.float64), y, U, 16)
    with pytest.raises(ValueError, match="need U"):
        objective_mlp_host_bytes(X, y, U[:-1], 16)


def test_labels_outside_the_classes_belong_to_no_class():
    """Rows with labels -2, -1, K, K + 1 are negatives of every class: the autograd formula, whose target is a comparison, agrees;
    and moving such a row's label to another value outside changes nothing."""
    N, D, K, H = 17, 5, 3, 7
    X, y, U = _random_case(N, D, K, H, outside=True)
    assert (y < 0).any() and (y >= K).any()
    f, g = _autograd(X, y, U, H, 1.0)
    loss, grad = objective_mlp_host_bytes(X, y, U, H, 1.0)
    assert float((loss - f).abs().max()) <= 1e-10 * float(f.abs().max())
    assert float((grad - g).abs().max()) <= 1e-10 * float(g.abs().max())
    y2 = np.where((y < 0) | (y >= K), 99, y)
    loss2, grad2 = objective_mlp_host_bytes(X, y2, U, H, 1.0)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_probabilities_sum_to_one():
    X, _, U = _random_case(40, 64, 4, 16)
    P = proba_mlp_host_bytes(X, U, 16)
    assert P.shape == (40, 4) and P.dtype == torch.float64 and float(P.min()) > 0
    assert float((P.sum(1) - 1).abs().max()) <= 1e-12


# ---- the solver -------------------------------------------------------------------------------------------------------------------------

def test_fit_on_the_host_descends_and_depends_on_the_seed_alone():
    (x, y), _ = xor_problem()
    clf, rep, _ = xor_host_fit(20)
    U0 = clf.initial_point(64)
    assert U0.shape == (66 * 16 + 1, 2) and U0.dtype == torch.float64
    assert float(U0[:64 * 16].abs().max()) <= np.sqrt(6 / 80) and float(U0[65 * 16:66 * 16].abs().max()) <= np.sqrt(6 / 17)
    assert float(U0[64 * 16:65 * 16].abs().max()) == 0 and float(U0[-1].abs().max()) == 0          # the intercepts start at zero
    l0, _ = objective_mlp_host_bytes(x, y, U0, 16, 1.0)
    assert all(l < l0k for l, l0k in zip(rep["loss"], l0.tolist())), (rep["loss"], l0.tolist())
    assert max(rep["iterations"]) <= 20 and clf.coef.shape == U0.shape
    again = OvrMlp(2, hidden=16, max_iter=20)
    rep2 = again.fit_bytes(x, y)
    assert np.array_equal(again.coef.numpy().view(np.uint64), clf.coef.numpy().view(np.uint64)) and rep2 == rep
    other = OvrMlp(2, hidden=16, max_iter=20, seed=1)
    other.fit_bytes(x, y)
    assert not torch.equal(other.coef, clf.coef)


def test_fit_refusals():
    (x, y), _ = xor_problem()
    with pytest.raises(ValueError, match="every class"):
        OvrMlp(3, hidden=4).fit_bytes(x, y)
    with pytest.raises(ValueError, match="uint8"):
        OvrMlp(2, hidden=4).fit_bytes(x.astype(np.float32), y)
    with pytest.raises(RuntimeError, match="fit first"):
        OvrMlp(2, hidden=4).predict_proba_bytes(x)
    for hidden in (0, 129):
        with pytest.raises(ValueError, match="hidden"):
            OvrMlp(2, hidden=hidden)
    with pytest.raises(ValueError, match="alpha"):
        OvrMlp(2, alpha=-1.0)
    with pytest.raises(ValueError, match="n_classes"):
        OvrMlp(17)


def test_the_problem_a_linear_model_cannot_do():
    """XOR of blobs (seed 7): the host logistic regression stays at or below 240 / 400; the host MLP (16 units, 200 iterations)
    was measured at M = 327 and must reach H* = 284, the midpoint between 240 and M."""
    (x, y), (xt, yt) = xor_problem()
    lr = OvrLogReg(2)
    lr.fit_bytes(x, y)
    hits_lr = accuracy(lr.predict_proba_bytes(xt), yt)["hits"]
    _, rep, P = xor_host_fit(200)
    hits = accuracy(P, yt)["hits"]
    print("XOR: logistic regression %d / 400, MLP %d / 400 after %s iterations" % (hits_lr, hits, rep["iterations"]))
    assert hits_lr <= XOR_LR_CAP
    assert hits >= XOR_BAR


# ---- the command line -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    return make_caches(tmp_path_factory.mktemp("mlp_caches"))


def test_cli_with_the_mlp_on_the_cpu(caches, tmp_path):
    from csl_gan_amd import tstr
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    vals = str(tmp_path / "vals")
    args = ["--syn_cache", syn, "--test_cache", test, "--train_cache", caches["train"][0], "--baseline", "-d", "cpu"]
    res = tstr.main(args + ["--classifier", "mlp", "--hidden", "8", "--alpha", "0.5", "--seed", "3", "--max_iter", "15", "--values_dir", vals])
    assert list(res) == ["syn", "baseline_train"]
    for lab, n in (("syn", 300), ("baseline_train", 240)):
        m = res[lab]
        assert (m["classifier"], m["hidden"], m["alpha"], m["seed"]) == ("mlp", 8, 0.5, 3)
        assert m["n_train"] == n and m["n_test"] == 200 and m["classes"] == 3 and max(m["solver"]["iterations"]) <= 15
        assert np.load(os.path.join(vals, lab + "_U.npy")).shape == ((1024 + 2) * 8 + 1, 3)
        assert np.load(os.path.join(vals, lab + "_P.npy")).shape == (200, 3)
    clf = OvrMlp(3, hidden=8, alpha=0.5, seed=3, max_iter=15)
    rep = clf.fit_bytes(x, y)
    P = clf.predict_proba_bytes(xt)
    assert res["syn"]["solver"] == rep and res["syn"]["accuracy_hits"] == accuracy(P, yt)["hits"]
    assert np.array_equal(np.load(os.path.join(vals, "syn_U.npy")), clf.coef.numpy())
    assert res["syn"]["accuracy_hits"] > 100                             # three classes, 200 rows: well above chance after 15 iterations


def test_cli_without_the_flag_is_the_logistic_regression(caches):
    from csl_gan_amd import tstr
    args = ["--syn_cache", caches["syn"][0], "--test_cache", caches["test"][0], "-d", "cpu"]
    plain = tstr.main(args)
    lr = tstr.main(args + ["--classifier", "lr"])
    assert plain == lr and list(plain["syn"]) == list(lr["syn"])
    assert list(plain["syn"]) == ["n_train", "n_test", "classes", "auroc_micro", "auroc_per_class", "accuracy", "accuracy_hits", "solver"]
    assert plain["syn"]["solver"]["gtol_rel"] == 1e-8 and all(plain["syn"]["solver"]["converged"])
    assert tstr.main(args + ["--hidden", "7", "--alpha", "0", "--seed", "9"]) == plain      # the MLP's flags mean nothing to it


def test_cli_refusals(caches):
    from csl_gan_amd import tstr
    args = ["--syn_cache", caches["syn"][0], "--test_cache", caches["test"][0], "--classifier", "mlp"]
    for hidden in ("0", "129"):
        with pytest.raises(SystemExit, match="--hidden"):
            tstr.main(args + ["--hidden", hidden])
    with pytest.raises(SystemExit, match="--alpha"):
        tstr.main(args + ["--alpha", "-0.5"])
    with pytest.raises(SystemExit):
        tstr.main(args[:-1] + ["tree"])                                  # argparse: not one of lr, mlp


# ---- the C-ABI entries ----------------------------------------------------------------------------------------------------------------

def test_abi_entries_are_declared_exported_and_validate_on_the_host():
    from csl_gan_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "cslgan.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for proto in ("int64_t cslgan_ovr_mlp_u8_ws_floats(int64_t N, int D, int K, int H);",
                  "int cslgan_ovr_mlp_eval_u8(const void* X, const int32_t* labels, const float* U, int64_t N, int D, int K, int H, "
                  "float alpha, float* loss, float* grad, float* ws, void* stream);",
                  "int cslgan_ovr_mlp_proba_u8(const void* Xtest, const float* U, int64_t M, int D, int K, int H, float* P, void* stream);"):
        assert proto in flat, proto
    assert re.search(r"#define\s+CSLGAN_ABI_VERSION\s+7\b", hdr)
    L = ctypes.CDLL(build.build())
    for name in ("cslgan_ovr_mlp_u8_ws_floats", "cslgan_ovr_mlp_eval_u8", "cslgan_ovr_mlp_proba_u8"):
        assert hasattr(L, name), name
    L = _lib.lib()
    assert L.cslgan_version() == 7 == _lib.ABI_VERSION
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert L.cslgan_ovr_mlp_u8_ws_floats.argtypes == [i64, i32, i32, i32] and L.cslgan_ovr_mlp_u8_ws_floats.restype == i64
    assert L.cslgan_ovr_mlp_eval_u8.argtypes == [vp, vp, vp, i64, i32, i32, i32, f32, vp, vp, vp, vp]
    assert L.cslgan_ovr_mlp_proba_u8.argtypes == [vp, vp, i64, i32, i32, i32, vp, vp]

    err = lambda: L.cslgan_last_error()
    wsf = L.cslgan_ovr_mlp_u8_ws_floats
    for n, d, k, h in ((0, 784, 10, 100), (2 ** 31, 784, 10, 100), (10, 0, 10, 100), (10, 65537, 10, 100), (10, 784, 1, 100),
                       (10, 784, 17, 100), (10, 784, 10, 0), (10, 784, 10, 129)):
        assert wsf(n, d, k, h) == 0, (n, d, k, h)
    # one forward workgroup: 2 (48 + 2 C) floats of partials; dZ1 [N, C]; one chunk of partial gradients [D, C]
    assert wsf(1, 1, 2, 1) == 2 * (48 + 4) + 2 + 2
    assert wsf(100, 12288, 2, 100) == 2 * 2 * (48 + 400) + 100 * 200 + 12288 * 200
    assert 0 < wsf(60000, 784, 10, 100) * 4 < 2 ** 29 and wsf(20, 65536, 16, 128) > 0
    ok = dict(X=16, lab=16, U=16, N=100, D=930, K=10, H=100, alpha=1.0, loss=16, grad=16, ws=16)

    def ev(**kw):
        a = dict(ok, **kw)
        return L.cslgan_ovr_mlp_eval_u8(a["X"], a["lab"], a["U"], a["N"], a["D"], a["K"], a["H"], a["alpha"], a["loss"], a["grad"], a["ws"], None)

    for name in ("X", "lab", "U", "loss", "grad", "ws"):
        assert ev(**{name: None}) == -1 and b"null" in err(), name
    for bad, tag in ((dict(K=1), b"K="), (dict(K=17), b"K="), (dict(H=0), b"H="), (dict(H=129), b"H="), (dict(D=0), b"D="),
                     (dict(D=65537), b"D="), (dict(N=0), b"N="), (dict(N=2 ** 31), b"N="), (dict(alpha=-1.0), b"alpha="),
                     (dict(alpha=float("nan")), b"alpha="), (dict(ws=20), b"workspace misaligned"), (dict(X=17), b"X misaligned")):
        assert ev(**bad) == -1 and tag in err(), bad

    def pr(X=16, U=16, M=10, D=930, K=10, H=100, P=16):
        return L.cslgan_ovr_mlp_proba_u8(X, U, M, D, K, H, P, None)

    for name in ("X", "U", "P"):
        assert pr(**{name: None}) == -1 and b"null" in err(), name
    for bad, tag in ((dict(K=17), b"K="), (dict(H=129), b"H="), (dict(D=0), b"D="), (dict(M=0), b"N="), (dict(X=17), b"misaligned")):
        assert pr(**bad) == -1 and tag in err(), bad


def test_ops_have_no_cpu_path():
    from csl_gan_amd import ops
    X, U = torch.zeros((8, 20), dtype=torch.uint8), torch.zeros((22 * 4 + 1, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.ovr_mlp_eval_u8(X, torch.zeros(8, dtype=torch.int32), U, 4)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.ovr_mlp_proba_u8(X, U, 4)
