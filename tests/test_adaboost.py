"""csl_gan_amd.classify.AdaBoost and tstr --classifier ab on the CPU: the host fit against scikit-learn's
AdaBoostClassifier of depth-1 trees, the host model of the stump search against a one-candidate-at-a-time evaluation of its formula
and on hand-made cases, its tie to the tree split search, the stopping rules, the fits (weight range, determinism), the command line
with its refusals, and the host-side argument checks of the C-ABI entry (no launch, no device)."""
import math
import os

import numpy as np
import pytest
import torch

from test_trees import sklearn_problem
from test_tstr import make, make_caches

W1 = 1 << 28


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    return make_caches(tmp_path_factory.mktemp("ab_caches"))


def stump1(X, y, w=None, K=2, cls=1):
    """The stump of ONE class on the rows of X: (j, v, v_hi, nL, pL, n, p) as a tuple of ints, and the bits of the score."""
    from csl_gan_amd import classify
    X = np.ascontiguousarray(X, dtype=np.uint8)
    W = np.full((K, len(X)), W1, dtype=np.int64)
    if w is not None:
        W[cls] = w
    out, score = classify.boost_stump_host_bytes(X, y, W, K)
    assert out.dtype == torch.int64 and tuple(out.shape) == (K, 7) and score.dtype == torch.int64 and tuple(score.shape) == (K,)
    return tuple(int(a) for a in out[cls]), int(score[cls])


def bits(s):
    return int(np.float64(s).view(np.int64))


def brute_stump(X, t, w):
    """The definition, one candidate at a time in Python integers and single float64 operations: ((j, v, v_hi, nL, pL, n, p), score bits)."""
    w = np.asarray(w, dtype=np.int64)
    live = w > 0
    wt = w * t
    n, p = int(w.sum()), int(wt.sum())
    best = None
    for j in range(X.shape[1]):
        vals = np.unique(X[live, j])
        for i, v in enumerate(vals[:-1]):
            left = live & (X[:, j] <= v)
            nL, pL = int(w[left].sum()), int(wt[left].sum())
            a, c = np.float64(pL), np.float64(p - pL)
            s = (a * a) / np.float64(nL) + (c * c) / np.float64(n - nL)
            if best is None or s > best[0]:                          # j, then v ascending: the first of equal scores stays
                best = (s, (j, int(v), int(vals[i + 1]), nL, pL, n, p))
    return ((-1, -1, -1, 0, 0, n, p), 0) if best is None else (best[1], bits(best[0]))


# ---- against scikit-learn -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lr", [1.0, 0.5])
@pytest.mark.parametrize("seed", range(10))
def test_fit_equals_scikit_learn(seed, lr):
    """AdaBoostClassifier(DecisionTreeClassifier(max_depth=1), n_estimators=50, learning_rate=lr, random_state=0) on X / 255: the same
    number of rounds and P within 1e-6 on the training rows and on 200 fresh rows.  The 2^-28 weight grid gives about 2e-8; a stump
    that differed would show at about 1e-2.  Class 1 is the estimator scikit-learn fits on y, class 0 the one it fits on 1 - y."""
    ensemble, tree = pytest.importorskip("sklearn.ensemble"), pytest.importorskip("sklearn.tree")
    from csl_gan_amd import classify
    X, y = sklearn_problem(seed)
    Xt, _ = sklearn_problem(100 + seed)
    clf = classify.AdaBoost(2, n_rounds=50, learning_rate=lr)
    rep = clf.fit_bytes(X, y)
    P, Pt = clf.predict_proba_bytes(X).numpy(), clf.predict_proba_bytes(Xt).numpy()
    for cls, target in ((1, y), (0, 1 - y)):
        ref = ensemble.AdaBoostClassifier(tree.DecisionTreeClassifier(max_depth=1), n_estimators=50, learning_rate=lr, random_state=0).fit(X / 255., target)
        assert rep["rounds"][cls] == len(ref.estimators_) == 50
        d = max(np.abs(P[:, cls] - ref.predict_proba(X / 255.)[:, 1]).max(), np.abs(Pt[:, cls] - ref.predict_proba(Xt / 255.)[:, 1]).max())
        print("seed %d lr %g class %d: max |P - P_sklearn| = %.3g" % (seed, lr, cls, d))
        assert d <= 1e-6


# ---- the stump search ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,D", [(30, 9), (64, 5), (65, 5), (150, 12)])
def test_host_stump_equals_brute_force(N, D):
    """Random weights in 0 .. 2^28 with zeros among them, on both sides of the host model's switch from sorting to histograms: every
    integer and the bits of the score."""
    rng = np.random.default_rng(N)
    X = (rng.integers(0, 256, (N, D)) // 16 * 16).astype(np.uint8)
    X[:, 1] = X[:, 0]
    y = rng.integers(0, 3, N)
    from csl_gan_amd import classify
    for trial in range(3):
        W = rng.integers(0, W1 + 1, (3, N)) * (rng.random((3, N)) < 0.7)
        W[:, trial] = W1
        out, score = classify.boost_stump_host_bytes(X, y, W, 3)
        for k in range(3):
            want, sbits = brute_stump(X, y == k, W[k])
            assert tuple(int(a) for a in out[k]) == want and int(score[k]) == sbits, (trial, k)
            assert want[0] != 1                                      # the duplicate of column 0 never wins


@pytest.mark.parametrize("n_live", [64, 65])
def test_host_stump_at_the_switch_from_sorting_to_histograms(n_live):
    """Exactly 64 and 65 rows of weight > 0 (the switch counts those), 12 more of weight 0: the last size that is sorted and the first
    that goes into histograms, against the definition in every integer and the bits of the score."""
    from csl_gan_amd import classify
    rng = np.random.default_rng(n_live)
    N = n_live + 12
    X = (rng.integers(0, 256, (N, 6)) // 16 * 16).astype(np.uint8)
    y = rng.integers(0, 2, N)
    W = rng.integers(1, W1 + 1, (2, N))
    W[:, rng.choice(N, 12, replace=False)] = 0
    assert ((W > 0).sum(1) == n_live).all()
    out, score = classify.boost_stump_host_bytes(X, y, W, 2)
    for k in range(2):
        want, sbits = brute_stump(X, y == k, W[k])
        assert tuple(int(a) for a in out[k]) == want and int(score[k]) == sbits, k


def test_hand_made_cases():
    y = np.array([0, 0, 1, 1])
    col = lambda *b: np.array(b, dtype=np.uint8)[:, None]
    out, s = stump1(col(0, 0, 255, 255), y)
    assert out == (0, 0, 255, 2 * W1, 0, 4 * W1, 2 * W1) and (out[1] + out[2]) // 2 == 127 and s == bits(2.0 * W1)
    for v in (0, 100, 254):
        out, _ = stump1(col(v, v, v + 1, v + 1), y)
        assert out[:3] == (0, v, v + 1) and (out[1] + out[2]) // 2 == v             # adjacent bytes: the threshold is v itself
    X = np.array([[7, 1, 9], [7, 2, 9], [7, 3, 9], [7, 4, 9]], dtype=np.uint8)
    assert stump1(X, y)[0][:3] == (1, 2, 3)                                          # the constant columns are never chosen
    assert stump1(np.full((4, 3), 9), y) == ((-1, -1, -1, 0, 0, 4 * W1, 2 * W1), 0)  # all rows equal: no candidate
    X = np.array([[1, 5, 1, 5], [2, 6, 2, 6], [3, 7, 3, 7], [4, 8, 4, 8]], dtype=np.uint8)
    assert stump1(X, y)[0][:3] == (0, 2, 3)                                          # duplicate columns: the smaller j
    assert stump1(X[:, ::-1], np.array([0, 1, 1, 0]))[0][:3] == (0, 5, 6)            # equal scores at v = 5 and v = 7: the smaller v
    assert stump1(col(3), np.array([1])) == ((-1, -1, -1, 0, 0, W1, W1), 0)          # one row
    # weight 0 equals the row being absent: a byte that only such rows hold is neither a threshold nor a v_hi
    X, t = col(10, 20, 30, 40), np.array([0, 1, 1, 1])
    got = stump1(X, t, w=[W1, 0, 5, 7])
    assert got == stump1(X[[0, 2, 3]], t[[0, 2, 3]], w=[W1, 5, 7]) and got[0] == (0, 10, 30, W1, 0, W1 + 12, 12)
    # all weight on one target: p == n, the best candidate is still reported, by the formula
    got = stump1(X, t, w=[0, 3, 4, 5])
    assert got == brute_stump(X, t == 1, [0, 3, 4, 5]) and got[0][3:] == (3, 3, 12, 12) and got[0][:3] == (0, 20, 30)
    from csl_gan_amd import classify
    for bad in (-1, W1 + 1):
        with pytest.raises(ValueError, match="2\\^28"):
            classify.boost_stump_host_bytes(X, t, np.array([[1, 1, 1, 1], [1, 1, bad, 1]]), 2)
    with pytest.raises(ValueError, match="weights"):
        classify.boost_stump_host_bytes(X, t, np.ones((3, 4), dtype=np.int64), 2)


@pytest.mark.parametrize("seed", range(3))
def test_unit_weights_give_the_root_of_the_tree_search(seed):
    """(j, v, v_hi) of best_split_host_bytes at the root, its integers times 2^28, its score scaled by 2^28 bit for bit."""
    from csl_gan_amd import classify
    X, y = sklearn_problem(seed)
    N = len(y)
    to, ts = classify.best_split_host_bytes(X, y, np.tile(np.arange(N), 2), [0, N, 2 * N], [0, 1])
    bo, bs = classify.boost_stump_host_bytes(X, y, np.full((2, N), W1), 2)
    to, bo = to.numpy().astype(np.int64), bo.numpy()
    assert np.array_equal(bo[:, :3], to[:, :3]) and np.array_equal(bo[:, 3:], to[:, 3:] * W1)
    assert np.array_equal(bs.numpy(), np.ldexp(ts.numpy().view(np.float64), 28).view(np.int64))


# ---- stopping and fits --------------------------------------------------------------------------------------------------------------

def test_stopping_rules():
    from csl_gan_amd import classify
    X = np.array([[10], [20], [200], [220]], dtype=np.uint8)
    clf = classify.AdaBoost(2)
    rep = clf.fit_bytes(X, np.array([0, 0, 1, 1]))                                   # separable: e == 0 keeps one stump, alpha 1
    assert rep["rounds"] == [1, 1] and rep["alpha_sum"] == [1.0, 1.0] and rep["first_err"] == [0.0, 0.0]
    assert clf.coef.dtype == torch.float64 and clf.coef.tolist() == [[0, 0, 0, 110, 1, 0, 1], [1, 0, 0, 110, 0, 1, 1]]
    assert clf.decision_bytes(X).tolist() == [[1, -1], [1, -1], [-1, 1], [-1, 1]]
    lo, hi = 1.0 / (1.0 + np.exp(2.0)), 1.0 / (1.0 + np.exp(-2.0))
    assert clf.predict_proba_bytes(X).tolist() == [[hi, lo], [hi, lo], [lo, hi], [lo, hi]]
    clf = classify.AdaBoost(2)
    rep = clf.fit_bytes(np.array([[5], [5]], dtype=np.uint8), np.array([0, 1]))      # two equal rows: no split, 2 e == n, discarded
    assert rep["rounds"] == [0, 0] and rep["alpha_sum"] == [0.0, 0.0] and rep["first_err"] == [0.5, 0.5] and tuple(clf.coef.shape) == (0, 7)
    assert clf.decision_bytes(np.array([[5], [9]], dtype=np.uint8)).tolist() == [[0, 0], [0, 0]]
    assert clf.predict_proba_bytes(np.array([[5], [9]], dtype=np.uint8)).tolist() == [[0.5, 0.5], [0.5, 0.5]]
    clf = classify.AdaBoost(2)
    # three equal rows, one against two: a single leaf with e = n / 3 is kept; the missed row doubles, the next leaf ties and is discarded
    rep = clf.fit_bytes(np.array([[5], [5], [5]], dtype=np.uint8), np.array([0, 1, 1]))
    assert rep["rounds"] == [1, 1] and rep["alpha_sum"] == [math.log(2.0)] * 2 and rep["first_err"] == [1 / 3, 1 / 3]
    assert clf.coef.tolist() == [[0, 0, -1, 0, 0, 0, math.log(2.0)], [1, 0, -1, 0, 1, 1, math.log(2.0)]]
    assert clf.decision_bytes(np.array([[0]], dtype=np.uint8)).tolist() == [[-1, 1]]


def test_fits():
    from csl_gan_amd import classify
    x, y = make(150, 8, 8, 1, 3, 1)
    seen = []

    def on_round(rnd, w):
        assert w.dtype == torch.int32 and tuple(w.shape) == (3, 150)
        seen.append((rnd, int(w.min()), [int(m) for m in w.max(1)[0]]))

    clf = classify.AdaBoost(3, n_rounds=12)
    rep = clf.fit_bytes(x, y, on_round=on_round)
    assert [s[0] for s in seen] == list(range(12)) and all(s[1] >= 0 and s[2] == [W1] * 3 for s in seen)
    c = clf.coef.numpy()
    assert rep["kind"] == "ab" and rep["n_per_class"] == np.bincount(y, minlength=3).tolist() and rep["rounds"] == [12, 12, 12]
    assert c.shape == (36, 7) and np.array_equal(c[:, 0], np.repeat(np.arange(3), 12)) and np.array_equal(c[:, 1], np.tile(np.arange(12), 3))
    assert (c[:, 2] >= 0).all() and (c[:, 4] != c[:, 5]).any() and (c[:, 6] > 0).all()
    assert rep["alpha_sum"] == [sum(c[c[:, 0] == k, 6].tolist()) for k in range(3)]
    assert all(0 < e < 0.5 for e in rep["first_err"]) and [math.log((1 - e) / e) for e in rep["first_err"]] == pytest.approx(c[::12, 6].tolist(), rel=1e-12)
    F, P = clf.decision_bytes(x).numpy(), clf.predict_proba_bytes(x).numpy()
    assert (np.abs(F) <= 1).all() and np.array_equal(P, 1.0 / (1.0 + np.exp(-2.0 * F))) and classify.accuracy(P, y)["accuracy"] > 0.7
    again = classify.AdaBoost(3, n_rounds=12)                                        # a second fit: the same bits
    assert again.fit_bytes(x, y) == rep and np.array_equal(again.coef.numpy().view(np.uint64), c.view(np.uint64))
    one = classify.AdaBoost(3, n_rounds=1)
    assert one.fit_bytes(x, y)["rounds"] == [1, 1, 1] and np.array_equal(one.coef.numpy(), c[::12])
    half = classify.AdaBoost(3, n_rounds=12, learning_rate=0.5)
    half.fit_bytes(x, y)
    assert half.coef[0, 6] == 0.5 * c[0, 6] and np.array_equal(half.coef.numpy()[::12, :6], c[::12, :6])
    # a label outside the classes is negative for every class
    yo = y.copy()
    yo[::7] = np.where(np.arange(len(yo[::7])) % 2 == 0, -1, 5)
    out = classify.AdaBoost(3, n_rounds=4)
    rep_o = out.fit_bytes(x, yo)
    assert rep_o["n_per_class"] == [int((yo == k).sum()) for k in range(3)]
    for k in range(3):
        ref = classify.AdaBoost(3, n_rounds=4)
        ref.fit_bytes(x, np.where((yo < 0) | (yo > 2), (k + 1) % 3, yo))
        assert np.array_equal(out.coef.numpy()[out.coef.numpy()[:, 0] == k], ref.coef.numpy()[ref.coef.numpy()[:, 0] == k])
    with pytest.raises(RuntimeError, match="fit first"):
        classify.AdaBoost(3).predict_proba_bytes(x)
    with pytest.raises(ValueError, match="every class"):
        classify.AdaBoost(4).fit_bytes(x, y)
    for kw in ({"n_rounds": 0}, {"n_rounds": 4096}, {"learning_rate": 0.0}, {"learning_rate": float("inf")}, {"learning_rate": float("nan")}):
        with pytest.raises(ValueError):
            classify.AdaBoost(3, **kw)


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_cli_on_the_cpu(caches, tmp_path, capsys):
    from csl_gan_amd import classify, tstr
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    vals = str(tmp_path / "vals")
    args = ["--syn_cache", syn, "--test_cache", test, "-d", "cpu", "--classifier", "ab", "--n_rounds", "20", "--learning_rate", "0.5", "--values_dir", vals]
    res = tstr.main(args)
    m = res["syn"]
    clf = classify.AdaBoost(3, n_rounds=20, learning_rate=0.5)
    rep = clf.fit_bytes(x, y)
    P = clf.predict_proba_bytes(xt)
    a, acc = classify.auroc(P, yt), classify.accuracy(P, yt)
    assert m["classifier"] == "ab" and m["fit"] == rep and m["n_rounds"] == 20 and m["learning_rate"] == 0.5 and "solver" not in m
    assert m["auroc_micro"] == a["micro"] and m["auroc_per_class"] == a["per_class"] and m["accuracy_hits"] == acc["hits"]
    assert 0.5 < m["accuracy"] < 1.0
    first = (np.load(os.path.join(vals, "syn_P.npy")), np.load(os.path.join(vals, "syn_U.npy")))
    assert np.array_equal(first[0], P.numpy()) and np.array_equal(first[1], clf.coef.numpy()) and first[1].shape == (60, 7)
    assert "rounds per class [20, 20, 20]" in capsys.readouterr().out
    assert tstr.main(args) == res                                                    # a second run: the same output
    assert np.array_equal(np.load(os.path.join(vals, "syn_P.npy")), first[0]) and np.array_equal(np.load(os.path.join(vals, "syn_U.npy")), first[1])
    d = tstr.build_parser().parse_args(args[:6])
    assert (d.n_rounds, d.learning_rate) == (50, 1.0)


def test_cli_refusals(caches):
    from csl_gan_amd import tstr
    base = ["--syn_cache", caches["syn"][0], "--test_cache", caches["test"][0], "-d", "cpu", "--classifier", "ab"]
    for flags, msg in ((["--n_rounds", "0"], "--n_rounds 0"), (["--n_rounds", "4096"], "--n_rounds 4096"), (["--learning_rate", "0"], "--learning_rate 0")):
        with pytest.raises(SystemExit, match=msg):
            tstr.main(base + flags)


# ---- the C-ABI entry validates on the host ------------------------------------------------------------------------------------------

def test_abi_entry_rejects_bad_arguments_without_a_device():
    from csl_gan_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert {"cslgan_boost_stump_ws_bytes", "cslgan_boost_stump_u8"} <= set(_lib.EXPORTS) and L.cslgan_version() == 7
    err = lambda: L.cslgan_last_error()
    wsb = L.cslgan_boost_stump_ws_bytes
    for k, d in ((1, 784), (17, 784), (2, 0), (2, 65537)):
        assert wsb(k, d) == 0, (k, d)
    assert wsb(2, 1) == 128 and wsb(3, 17) == 384 and wsb(10, 784) == 10 * 49 * 64 and wsb(16, 65536) == 16 * 4096 * 64
    need = wsb(10, 930)
    ok = dict(X=16, lab=16, W=16, N=100, D=930, K=10, out=16, score=16, ws=16, wsn=need)

    def bs(**kw):
        a = dict(ok, **kw)
        return L.cslgan_boost_stump_u8(a["X"], a["lab"], a["W"], a["N"], a["D"], a["K"], a["out"], a["score"], a["ws"], a["wsn"], None)

    for name in ("X", "lab", "W", "out", "score", "ws"):
        assert bs(**{name: None}) == -1 and b"null" in err(), name
    for n in (0, -1, 2 ** 24):
        assert bs(N=n) == -1 and b"N=" in err()
    for d in (0, -1, 65537):
        assert bs(D=d) == -1 and b"D=" in err()
    for k in (1, 17):
        assert bs(K=k) == -1 and b"K=" in err()
    for x in (17, 24):
        assert bs(X=x) == -1 and b"X misaligned" in err()
    assert bs(wsn=need - 1) == -1 and b"workspace" in err()
    assert bs(wsn=0) == -1 and b"workspace" in err()
    for name in ("lab", "W"):
        assert bs(**{name: 18}) == -1 and b"int32 array misaligned" in err(), name
    for name in ("out", "score", "ws"):
        assert bs(**{name: 20}) == -1 and b"misaligned (8 bytes)" in err(), name


def test_ops_have_no_cpu_path():
    from csl_gan_amd import ops
    X = torch.zeros((8, 20), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.boost_stump_u8(X, torch.zeros(8, dtype=torch.int32), 2, torch.zeros((2, 8), dtype=torch.int32))
