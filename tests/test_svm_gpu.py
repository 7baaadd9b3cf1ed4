"""The device path of csl_gan_amd.svm (-m gpu): cslgan_gram_d2_u8 against numpy's integer squared distances in every
entry, cslgan_svc_smo_f64 against smo_host bit for bit — alpha, the gradient, the iteration count, the done flag — for every problem of
the test problems and every chunk size, the device fit against the host fit, the probabilities, and the command line on cuda:0 against
-d cpu."""
import os

import numpy as np
import pytest
import torch

from test_svm import NAMES, host_fit, problem
from test_tstr import make_caches

pytestmark = pytest.mark.gpu


def _gram(X):
    """(d2 as a uint32 numpy view [n, pitch], the device tensor, s int64 on the device) of byte rows X."""
    from csl_gan_amd import _lib, ops, svm
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    xs, sq = ops.nn_prepare(Xd)
    out = torch.full((len(X), ops.gram_pitch(len(X))), -1, dtype=torch.int32, device="cuda")
    got = ops.gram_d2(xs, sq, out=out)
    assert got is out and _lib.lib().cslgan_last_kernel() == b"gram_d2_u8_kernel"
    return out.cpu().numpy().view(np.uint32), out, svm._byte_sqnorms_device(Xd)


def _asymmetric():
    """130 x 17: two row tiles, the second of 2 rows, one K stage of 17 bytes; every row and every column distinct, bytes 0 and 255 among them."""
    rng = np.random.default_rng(130)
    X = rng.integers(0, 256, (130, 17)).astype(np.uint8)
    X[0], X[129], X[64, :8] = 255, 0, 255
    return X


@pytest.mark.parametrize("which", ["ragged", "asymmetric"])
def test_gram_equals_numpy_in_every_entry(which):
    """Padding columns are not compared; the squared norms of the byte rows are exact too."""
    X = problem("ragged")[0] if which == "ragged" else _asymmetric()
    n = len(X)
    Xi = X.astype(np.int64)
    s = (Xi * Xi).sum(1)
    want = s[:, None] + s[None, :] - 2 * (Xi @ Xi.T)
    got, _, sd = _gram(X)
    assert got.shape == (n, (n + 31) // 32 * 32) and np.array_equal(sd.cpu().numpy(), s)
    bad = np.argwhere(got[:, :n].astype(np.int64) != want)
    assert len(bad) == 0, "%d entries differ, first at %s: device %d, numpy %d" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    if which == "asymmetric":
        assert want[0, 129] == 17 * 65025


def _assert_same_bits(name, dev, host):
    alpha, G, iters, done = dev
    for p, st in enumerate(host):
        assert iters[p] == st["iterations"] and bool(done[p]) == st["done"], "%s problem %d: device %d iterations done %s, host %d done %s" % (
            name, p, iters[p], done[p], st["iterations"], st["done"])
        for what, d, h in (("alpha", alpha[p], st["alpha"]), ("gradient", G[p], st["grad"])):
            bad = np.nonzero(d.view(np.uint64) != h.view(np.uint64))[0]
            assert len(bad) == 0, "%s problem %d: %d %s entries differ, first row %d: device %r, host %r" % (
                name, p, len(bad), what, bad[0], d[bad[0]], h[bad[0]])


@pytest.mark.parametrize("chunk", [1, 7, 4096])
@pytest.mark.parametrize("name", NAMES)
def test_smo_equals_the_host_model_bit_for_bit(name, chunk):
    """All K (1 + folds) problems of the fit in one launch sequence, against the host fit's solution (smo_host, uncut): alpha, the gradient,
    the iteration count and the done flag.  No tolerance: a difference is a wrong operation order or tie rule in the kernel."""
    from csl_gan_amd import svm
    clf = host_fit(name)
    sol = clf.solution
    _, d2, s = _gram(problem(name)[0])
    dev = svm.solve_device(d2, s, sol["Y"], sol["active"], clf.C, clf.tol, clf.max_iter, chunk=chunk)
    host = [{"alpha": sol["alpha"][p], "grad": sol["grad"][p], "iterations": int(sol["iterations"][p]), "done": bool(sol["done"][p])}
            for p in range(len(sol["Y"]))]
    assert min(st["iterations"] for st in host) > 50
    _assert_same_bits(name, dev, host)


def test_smo_with_its_state_in_global_memory():
    """n = 3200 is past the rows whose alpha and gradient a workgroup keeps in LDS: the other instance of the kernel.  Two problems, one with
    a fifth of the rows inactive, cut at 300 iterations in chunks of 64 (neither is done: both sides must say so), then both run on to
    max_iter = 340, past a launch that has only 40 iterations left."""
    from csl_gan_amd import svm
    rng = np.random.default_rng(3200)
    n, D = 3200, 17
    y = np.where(rng.random(n) < 0.5, 1, -1)
    X = np.clip(rng.normal(128 + 12 * y[:, None], 40, (n, D)), 0, 255).astype(np.uint8)
    X[1001] = X[17]
    y[17], y[1001] = 1, -1
    Y = np.stack([y, -y]).astype(np.int8)
    active = np.ones((2, n), dtype=bool)
    active[1, rng.random(n) < 0.2] = False
    got, d2, s = _gram(X)
    hd2, hs = svm.gram_d2_host(X)
    assert np.array_equal(got[:, :n], hd2)
    for max_iter in (300, 340):
        host = [svm.smo_host(hd2, hs, Y[p], active[p], 1.0, 1e-3, max_iter) for p in range(2)]
        assert all(st["iterations"] == max_iter and not st["done"] for st in host)
        _assert_same_bits("global", svm.solve_device(d2, s, Y, active, 1.0, 1e-3, max_iter, chunk=64), host)


@pytest.mark.parametrize("name", NAMES)
def test_device_fit_equals_the_host_fit(name):
    """coef in the same bits, the same report; the device probabilities of cslgan_ovr_logreg_proba_u8 within 1e-3 of proba_host_bytes with rows
    summing to 1 within 1e-5, the tolerance tests/test_tstr_gpu.py holds that kernel to."""
    from csl_gan_amd import classify, svm
    host = host_fit(name)
    X, y, K = problem(name)
    clf = svm.OvrSvc(K)
    rep = clf.fit_bytes(torch.from_numpy(X).cuda(), torch.from_numpy(y))
    assert rep == host.report
    assert clf.coef.device.type == "cpu" and np.array_equal(clf.coef.numpy().view(np.uint64), host.coef.numpy().view(np.uint64))
    rng = np.random.default_rng(12)
    Xt = np.clip(X[rng.integers(0, len(X), 77)].astype(np.int64) + rng.integers(-20, 21, (77, X.shape[1])), 0, 255).astype(np.uint8)
    P = clf.predict_proba_bytes(torch.from_numpy(Xt).cuda())
    assert P.is_cuda and P.dtype == torch.float32
    want = classify.proba_host_bytes(Xt, host.coef).numpy()
    err = float(np.abs(P.cpu().numpy() - want).max())
    print("%s: proba err %.2e" % (name, err))
    assert err <= 1e-3
    assert np.abs(P.cpu().numpy().sum(1) - 1).max() < 1e-5


def test_cli_on_the_device_agrees_with_the_cpu(tmp_path):
    """Identical fit reports; U from --values_dir in the same bits; P within 1e-3, and the scores within what rows that close can move."""
    from csl_gan_amd import tstr_svm
    from test_tstr_gpu import _agree
    c = make_caches(tmp_path)
    yt = c["test"][2]
    args = ["--syn_cache", c["syn"][0], "--test_cache", c["test"][0], "--train_cache", c["train"][0], "--baseline"]
    dev = tstr_svm.main(args + ["-d", "cuda:0", "--values_dir", str(tmp_path / "dev")])
    cpu = tstr_svm.main(args + ["-d", "cpu", "--values_dir", str(tmp_path / "cpu")])
    assert list(dev) == list(cpu) == ["syn", "baseline_train"]
    for lab in dev:
        d, h = dev[lab], cpu[lab]
        assert d["fit"] == h["fit"] and all(d["fit"]["converged"]) and d["classifier"] == "svm"
        assert {k: d[k] for k in ("n_train", "n_test", "classes", "C", "tol", "folds", "seed")} == {k: h[k] for k in ("n_train", "n_test", "classes", "C", "tol", "folds", "seed")}
        Uh, Ud = (np.load(os.path.join(str(tmp_path / w), lab + "_U.npy")) for w in ("cpu", "dev"))
        assert Uh.dtype == np.float64 and np.array_equal(Uh.view(np.uint64), Ud.view(np.uint64))
        Ph = np.load(os.path.join(str(tmp_path / "cpu"), lab + "_P.npy")).astype(np.float64)
        Pd = np.load(os.path.join(str(tmp_path / "dev"), lab + "_P.npy")).astype(np.float64)
        _agree(Ph, Pd, yt, 3, h["auroc_micro"], d["auroc_micro"], h["accuracy_hits"], d["accuracy_hits"])
