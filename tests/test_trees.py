"""csl_gan_amd.classify.Trees and tstr --classifier dt / rf on the CPU: the host model of the split search against
scikit-learn's depth-1 tree and on hand-made nodes, the fits (purity, the growth bounds, determinism, rf tied to dt), the command
line with its refusals, and the host-side argument checks of the two C-ABI entries (no launch, no device).  Every comparison is
exact."""
import os

import numpy as np
import pytest
import torch

from test_tstr import make, make_caches


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    return make_caches(tmp_path_factory.mktemp("tree_caches"))


def split1(X, y, K=2, cls=1, w=None, **kw):
    """The best split of ONE node holding every row of X: (j, v, v_hi, nL, pL, n, p) as a tuple, and the float64 score."""
    from csl_gan_amd import classify
    X = np.ascontiguousarray(X, dtype=np.uint8)
    N = len(X)
    extra = {} if w is None else {"seg_wrow": [0], "weights": np.asarray(w).reshape(1, N)}
    out, score = classify.best_split_host_bytes(X, y, np.arange(N), [0, N], [cls], **extra, **kw)
    assert out.dtype == torch.int32 and tuple(out.shape) == (1, 7) and score.dtype == torch.int64 and tuple(score.shape) == (1,)
    return tuple(int(a) for a in out[0]), float(score.numpy().view(np.float64)[0])


def sklearn_problem(seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 2, 200)
    X = np.clip(rng.normal(120 + 25 * y[:, None] * (np.arange(30) % 3 == 0), 40, (200, 30)), 0, 255).astype(np.uint8) // 8 * 8
    return X, y


def brute_scores(X, y):
    """Every candidate's score by the definition, one (feature, byte) at a time: {(j, v): s}."""
    n, p = len(y), int(y.sum())
    out = {}
    for j in range(X.shape[1]):
        for v in np.unique(X[:, j])[:-1]:
            left = X[:, j] <= v
            nL, pL = int(left.sum()), int(y[left].sum())
            out[(j, int(v))] = float(np.float64(pL * pL) / np.float64(nL) + np.float64((p - pL) * (p - pL)) / np.float64(n - nL))
    return out


@pytest.mark.parametrize("seed", range(10))
def test_root_split_equals_scikit_learn(seed):
    """The root of best_split_host_bytes against DecisionTreeClassifier(max_depth=1, random_state=0) on X / 255: the same feature, the
    same left / right partition of the rows, the Gini decrease within 1e-12; the best score is unique (so scikit-learn's random feature
    order cannot matter), and it is the brute-force maximum of the definition, in the same bits."""
    tree = pytest.importorskip("sklearn.tree")
    X, y = sklearn_problem(seed)
    (j, v, vh, nL, pL, n, p), s = split1(X, y)
    sc = brute_scores(X, y)
    top = max(sc.values())
    assert sorted(sc.values())[-2] < top                                            # unique
    assert sc[(j, v)] == top == s
    ref = tree.DecisionTreeClassifier(max_depth=1, random_state=0).fit(X / 255., y).tree_
    assert ref.node_count == 3 and int(ref.feature[0]) == j
    left = X[:, j] <= (v + vh) // 2
    assert np.array_equal(left, X[:, j] / 255. <= ref.threshold[0])
    assert (n, p, nL, pL) == (200, int(y.sum()), int(left.sum()), int(y[left].sum()))
    gini = lambda a, b: 2.0 * (a / b) * (1.0 - a / b)
    ours = gini(p, n) - (nL / n) * gini(pL, nL) - ((n - nL) / n) * gini(p - pL, n - nL)
    theirs = ref.impurity[0] - (ref.n_node_samples[1] * ref.impurity[1] + ref.n_node_samples[2] * ref.impurity[2]) / 200
    assert abs(ours - theirs) <= 1e-12
    assert abs(ours - (2.0 / n) * (s - p * p / n)) <= 1e-12                        # maximising s minimises the weighted Gini


def test_hand_made_nodes():
    y = np.array([0, 0, 1, 1])
    col = lambda *b: np.array(b, dtype=np.uint8)[:, None]
    assert split1(col(0, 0, 255, 255), y) == ((0, 0, 255, 2, 0, 4, 2), 2.0)         # only 0 and 255: the threshold is (0 + 255) // 2 = 127
    for v in (0, 100, 254):
        out, _ = split1(col(v, v, v + 1, v + 1), y)
        assert out[:3] == (0, v, v + 1) and (out[1] + out[2]) // 2 == v             # adjacent bytes: the threshold is v itself
    X = np.array([[7, 1, 9], [7, 2, 9], [7, 3, 9], [7, 4, 9]], dtype=np.uint8)
    assert split1(X, y)[0][:3] == (1, 2, 3)                                          # the constant columns are never chosen
    assert split1(np.full((4, 3), 9), y) == ((-1, -1, -1, 0, 0, 4, 2), 0.0)          # all rows equal: no candidate
    X = np.array([[1, 5, 1, 5], [2, 6, 2, 6], [3, 7, 3, 7], [4, 8, 4, 8]], dtype=np.uint8)
    assert split1(X, y)[0][:3] == (0, 2, 3)                                          # duplicate columns: the smaller j
    assert split1(X[:, ::-1], np.array([0, 1, 1, 0]))[0][:3] == (0, 5, 6)            # equal scores at v = 5 and v = 7: the smaller v
    assert split1(col(3), np.array([1])) == ((-1, -1, -1, 0, 0, 1, 1), 0.0)          # a single row
    out, s = split1(col(1, 2, 3, 4), np.array([0, 0, 0, 0]))                         # a pure node still reports its best candidate
    assert out == (0, 1, 2, 1, 0, 4, 0) and s == 0.0


def test_weights_equal_repeated_rows_and_zero_weight_rows_are_absent():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 256, (40, 9)).astype(np.uint8) // 32 * 32
    y = rng.integers(0, 3, 40)
    w = rng.integers(0, 4, 40)
    w[5] = 65535
    rep = np.repeat(np.arange(40), w)
    for cls in range(3):
        assert split1(X, y, 3, cls, w=w) == split1(X[rep], y[rep], 3, cls)
    # a byte that only rows of weight 0 hold is not present: it is neither a threshold nor a v_hi
    X = np.array([[10], [20], [30], [40]], dtype=np.uint8)
    assert split1(X, np.array([0, 1, 1, 1]), w=[1, 0, 1, 1])[0] == (0, 10, 30, 1, 0, 3, 2)
    with pytest.raises(ValueError, match="2\\^31"):
        split1(X, np.array([0, 1, 1, 1]), w=[2 ** 30, 2 ** 30, 1, 1])


@pytest.mark.parametrize("n_live", [64, 65])
def test_host_search_agrees_on_both_sides_of_its_switch(n_live):
    """64 rows are the last that the host search sorts, 65 the first that go into 256-bin histograms.  On both sides, with unit weights
    and with weights 1 .. 4 on n_live rows among 10 rows of weight 0, best_split_host_bytes is the maximum of brute_scores (the
    definition on the repeated rows) with ties to the smallest (j, v): every integer and the bits of the score."""
    rng = np.random.default_rng(n_live)
    for weighted in (False, True):
        N = n_live + (10 if weighted else 0)
        X = (rng.integers(0, 256, (N, 7)) // 16 * 16).astype(np.uint8)
        X[:, 3] = X[:, 2]                                                            # a duplicate column: the smaller j
        y = rng.integers(0, 2, N)
        w = np.ones(N, dtype=np.int64)
        if weighted:
            w = rng.integers(1, 5, N)
            w[rng.choice(N, 10, replace=False)] = 0
        assert int((w > 0).sum()) == n_live
        rep = np.repeat(np.arange(N), w)
        Xr, yr = X[rep], y[rep]
        sc = brute_scores(Xr, yr)
        top = max(sc.values())
        j, v = min(k for k, s in sc.items() if s == top)
        left = Xr[:, j] <= v
        want = (j, v, int(Xr[~left, j].min()), int(left.sum()), int(yr[left].sum()), len(yr), int(yr.sum()))
        got, s = split1(X, y, w=w if weighted else None)
        assert got == want and j != 3, (weighted, got, want)
        assert np.float64(s).view(np.int64) == np.float64(top).view(np.int64), (weighted, s, top)


def test_labels_outside_the_classes_are_negative_for_every_class():
    rng = np.random.default_rng(4)
    X = rng.integers(0, 256, (60, 7)).astype(np.uint8)
    y = rng.integers(-2, 6, 60)
    for cls in range(3):
        assert split1(X, y, 3, cls) == split1(X, np.where(y == cls, cls, (cls + 1) % 3), 3, cls)
        assert split1(X, y, 3, cls)[0][6] == int((y == cls).sum())


def test_segments_masks_and_refusals():
    from csl_gan_amd import classify
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (50, 40)).astype(np.uint8)
    y = rng.integers(0, 2, 50)
    rows = rng.permutation(50)
    off = [0, 20, 20, 50]                                                            # the middle segment is empty
    tree, node = np.array([3, 0, 7]), np.array([0, 5, 11])
    thr = classify.tree_mask_threshold(6, 40)
    assert thr == (6 << 32) // 40 and classify.tree_mask_threshold(40, 40) == 0 and classify.tree_mask_threshold(99, 40) == 0
    out, score = classify.best_split_host_bytes(X, y, rows, off, [1, 0, 1], seg_key=(tree, node), mask_thr=thr, seed=9)
    assert tuple(out[1]) == (-1, -1, -1, 0, 0, 0, 0) and int(score[1]) == 0
    for s in (0, 2):
        m = classify.tree_feature_mask(9, tree[s], node[s], 40, thr)
        assert 0 < m.sum() < 40 and m[int(out[s, 0])]
        r = rows[off[s]:off[s + 1]]
        Xm = X[r] * m[None, :].astype(np.uint8)                                      # a masked feature as a constant column
        assert split1(Xm, y[r]) == (tuple(int(a) for a in out[s]), float(score.numpy().view(np.float64)[s]))
    masks = np.stack([classify.tree_feature_mask(9, 1, q, 4096, classify.tree_mask_threshold(64, 4096)) for q in range(8)])
    assert 40 < masks.sum(1).min() and masks.sum(1).max() < 90 and len({m.tobytes() for m in masks}) == 8      # binomial(4096, 1 / 64), keyed by node
    assert not np.array_equal(masks[0], classify.tree_feature_mask(10, 1, 0, 4096, classify.tree_mask_threshold(64, 4096)))
    with pytest.raises(ValueError, match="uint8"):
        classify.best_split_host_bytes(X.astype(np.float32), y, rows, off, [1, 0, 1])
    with pytest.raises(ValueError, match="go together"):
        classify.best_split_host_bytes(X, y, rows, off, [1, 0, 1], seg_wrow=[0, 0, 0])
    with pytest.raises(ValueError, match="seg_key"):
        classify.best_split_host_bytes(X, y, rows, off, [1, 0, 1], mask_thr=5)
    with pytest.raises(ValueError, match="max_features"):
        classify.tree_mask_threshold(0, 40)


def test_apply_host_model_and_malformed_tables():
    from csl_gan_amd import classify
    X = np.array([[0, 9], [5, 9], [6, 9], [255, 0]], dtype=np.uint8)
    # tree 0: root splits on feature 0 at 5, its right child on feature 1 at 4; tree 1: one node
    feature, threshold, child = [0, -1, 1, -1, -1, -1], [5, 0, 4, 0, 0, 0], [1, -1, 3, -1, -1, -1]
    leaf = classify.tree_apply_host_bytes(X, feature, threshold, child, [0, 5, 6])
    assert leaf.dtype == torch.int32 and leaf.tolist() == [[1, 1, 4, 3], [0, 0, 0, 0]]
    bad = classify.tree_apply_host_bytes(X, [0, -1, 2, -1, -1, -1], threshold, [1, -1, 1, -1, -1, -1], [0, 5, 6])     # feature 2, child before parent
    assert bad.tolist() == [[1, 1, -1, -1], [0, 0, 0, 0]]
    assert classify.tree_apply_host_bytes(X, feature, threshold, [1, -1, 4, -1, -1, -1], [0, 5, 6]).tolist()[0] == [1, 1, -1, -1]   # child + 1 beyond the tree


# ---- fits -------------------------------------------------------------------------------------------------------------------------------

def test_full_dt_is_pure_and_bounds_are_honoured():
    from csl_gan_amd import classify
    x, y = make(150, 8, 8, 1, 3, 1)
    x, idx = np.unique(x, axis=0, return_index=True)                                 # equal rows with unequal labels could not be told apart
    y = y[idx]
    clf = classify.Trees(3, "dt")
    rep = clf.fit_bytes(x, y)
    c = clf.coef.numpy()
    assert clf.coef.dtype == torch.int32 and c.shape == (sum(rep["nodes"]), 6) and rep["kind"] == "dt"
    assert rep["n_per_class"] == np.bincount(y, minlength=3).tolist() and len(rep["nodes"]) == 3
    leaves = c[:, 1] < 0
    assert rep["leaves"] == np.bincount(c[leaves, 0], minlength=3).tolist() and all(2 * l - 1 == q for l, q in zip(rep["leaves"], rep["nodes"]))
    assert ((c[leaves, 5] == 0) | (c[leaves, 5] == c[leaves, 4])).all()              # fully grown: every leaf is pure
    assert rep["levels"] == max(rep["depth"]) + 1
    P = clf.predict_proba_bytes(x)
    assert P.dtype == torch.float64 and set(np.unique(P.numpy())) <= {0.0, 1.0}
    assert classify.accuracy(P, y) == {"hits": len(y), "n": len(y), "accuracy": 1.0}
    # the tables are a tree: children behind their parents, numbered level by level; n and p add up
    for t in range(3):
        ct = c[c[:, 0] == t]
        inner = np.nonzero(ct[:, 1] >= 0)[0]
        assert np.array_equal(ct[inner, 3], 1 + 2 * np.arange(len(inner)))           # creation order: parents in order, left before right
        assert np.array_equal(ct[ct[inner, 3], 4] + ct[ct[inner, 3] + 1, 4], ct[inner, 4])
        assert np.array_equal(ct[ct[inner, 3], 5] + ct[ct[inner, 3] + 1, 5], ct[inner, 5])
        assert ct[0, 4] == len(y) and ct[0, 5] == (y == t).sum()
    leaf = clf.apply_bytes(x).numpy()
    off = classify.tree_tables(clf.coef)[3]
    for t in range(3):
        assert np.array_equal(np.bincount(leaf[t], minlength=rep["nodes"][t])[c[off[t]:off[t + 1], 1] < 0], c[off[t]:off[t + 1]][c[off[t]:off[t + 1], 1] < 0, 4])
    # a second fit: the same bits
    again = classify.Trees(3, "dt")
    assert again.fit_bytes(x, y) == rep and np.array_equal(again.coef.numpy(), c)
    # max_depth and min_samples_split
    for d in (1, 3):
        lim = classify.Trees(3, "dt", max_depth=d)
        r = lim.fit_bytes(x, y)
        assert max(r["depth"]) == d and max(r["nodes"]) <= 2 ** (d + 1) - 1
    stump = classify.Trees(3, "dt", max_depth=1)
    stump.fit_bytes(x, y)
    for t in range(3):                                                               # the root of the stump is the root of the full tree
        assert np.array_equal(stump.coef.numpy()[stump.coef.numpy()[:, 0] == t][0], c[c[:, 0] == t][0])
    mss = classify.Trees(3, "dt", min_samples_split=20)
    mss.fit_bytes(x, y)
    cm = mss.coef.numpy()
    assert (cm[cm[:, 1] >= 0, 4] >= 20).all() and ((cm[:, 1] < 0) & (cm[:, 4] < 20) & (cm[:, 5] > 0) & (cm[:, 5] < cm[:, 4])).any()
    with pytest.raises(RuntimeError, match="fit first"):
        classify.Trees(3).predict_proba_bytes(x)
    with pytest.raises(ValueError, match="every class"):
        classify.Trees(4).fit_bytes(x, y)
    for kw in ({"kind": "gbm"}, {"kind": "rf", "n_trees": 0}, {"max_depth": -1}, {"min_samples_split": 1}, {"max_features": 0}, {"seed": -1}):
        with pytest.raises(ValueError):
            classify.Trees(3, **kw)


def test_rf_ties_to_dt_and_is_a_function_of_the_seed():
    from csl_gan_amd import classify
    x, y = make(120, 8, 8, 1, 2, 1)
    N = len(y)
    dt = classify.Trees(2, "dt")
    dt.fit_bytes(x, y)
    one = classify.Trees(2, "rf", n_trees=1, max_features=64)                        # max_features = D: every feature
    assert one.mask_threshold(64) == 0
    one.fit_bytes(x, y, weights=np.ones((1, N), dtype=np.int64))
    assert np.array_equal(one.coef.numpy(), dt.coef.numpy())
    rf = classify.Trees(2, "rf", n_trees=3, seed=7)
    W = rf.bootstrap_weights(N)
    assert W.shape == (3, N) and (W.sum(1) == N).all() and len({w.tobytes() for w in W}) == 3
    assert np.array_equal(W[1], np.bincount(np.random.default_rng([7, 1]).integers(0, N, N), minlength=N))
    rf.fit_bytes(x, y, mask_thr=0)                                                   # a mask of 0: dt on the same weights
    c = rf.coef.numpy()
    for b in range(3):
        wdt = classify.Trees(2, "dt")
        wdt.fit_bytes(x, y, weights=W[b:b + 1])
        for k in range(2):
            assert np.array_equal(c[c[:, 0] == k * 3 + b][:, 1:], wdt.coef.numpy()[wdt.coef.numpy()[:, 0] == k][:, 1:])
    # the real thing: masked, bootstrapped; the same bits twice, other bits from another seed; P is a mean of leaf frequencies
    f1, f2, f3 = (classify.Trees(2, "rf", n_trees=5, seed=s) for s in (7, 7, 8))
    r1, r2, r3 = f1.fit_bytes(x, y), f2.fit_bytes(x, y), f3.fit_bytes(x, y)
    assert r1 == r2 and np.array_equal(f1.coef.numpy(), f2.coef.numpy()) and not np.array_equal(f1.coef.numpy(), f3.coef.numpy())
    assert len(r1["nodes"]) == 10 and f1.mask_threshold(64) == (8 << 32) // 64
    P = f1.predict_proba_bytes(x).numpy()
    assert P.shape == (N, 2) and (P >= 0).all() and (P <= 1).all() and len(np.unique(P)) > 2
    assert classify.accuracy(P, y)["accuracy"] > 0.8
    c1, leaf, off = f1.coef.numpy().astype(np.int64), f1.apply_bytes(x).numpy(), classify.tree_tables(f1.coef)[3]
    want = np.zeros(N)
    for b in range(5):
        want += c1[off[5 + b] + leaf[5 + b], 5] / c1[off[5 + b] + leaf[5 + b], 4]
    assert np.array_equal(P[:, 1], want / 5.0)


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_cli_on_the_cpu(caches, tmp_path, capsys):
    from csl_gan_amd import classify, tstr
    syn, x, y = caches["syn"]
    test, xt, yt = caches["test"]
    vals = str(tmp_path / "vals")
    res = tstr.main(["--syn_cache", syn, "--test_cache", test, "-d", "cpu", "--classifier", "dt", "--values_dir", vals])
    m = res["syn"]
    clf = classify.Trees(3, "dt")
    rep = clf.fit_bytes(x, y)
    P = clf.predict_proba_bytes(xt)
    a, acc = classify.auroc(P, yt), classify.accuracy(P, yt)
    assert m["classifier"] == "dt" and m["fit"] == rep and m["max_depth"] == 0 and m["min_samples_split"] == 2 and "solver" not in m
    assert m["auroc_micro"] == a["micro"] and m["auroc_per_class"] == a["per_class"] and m["accuracy_hits"] == acc["hits"]
    assert 0.5 < m["accuracy"] < 1.0
    assert np.array_equal(np.load(os.path.join(vals, "syn_P.npy")), P.numpy())
    assert np.array_equal(np.load(os.path.join(vals, "syn_U.npy")), clf.coef.numpy())
    assert "fit: rows per class" in capsys.readouterr().out
    res = tstr.main(["--syn_cache", syn, "--test_cache", test, "-d", "cpu", "--classifier", "rf", "--n_trees", "4", "--seed", "3", "--max_depth", "6",
                     "--values_dir", vals])
    m = res["syn"]
    clf = classify.Trees(3, "rf", n_trees=4, seed=3, max_depth=6)
    rep = clf.fit_bytes(x, y)
    P = clf.predict_proba_bytes(xt)
    assert m["classifier"] == "rf" and m["fit"] == rep and (m["n_trees"], m["max_features"], m["seed"], m["max_depth"]) == (4, 32, 3, 6)
    assert max(rep["depth"]) == 6 and len(rep["nodes"]) == 12
    assert m["auroc_micro"] == classify.auroc(P, yt)["micro"] and m["accuracy_hits"] == classify.accuracy(P, yt)["hits"]
    assert np.array_equal(np.load(os.path.join(vals, "syn_P.npy")), P.numpy())
    assert np.array_equal(np.load(os.path.join(vals, "syn_U.npy")), clf.coef.numpy())


def test_cli_refusals(caches):
    from csl_gan_amd import tstr
    base = ["--syn_cache", caches["syn"][0], "--test_cache", caches["test"][0], "-d", "cpu", "--classifier", "rf"]
    for flags, msg in ((["--n_trees", "0"], "--n_trees 0"), (["--n_trees", "4096"], "--n_trees 4096"), (["--max_features", "-1"], "--max_features -1"),
                       (["--max_depth", "-1"], "--max_depth -1"), (["--min_samples_split", "1"], "--min_samples_split 1"), (["--seed", "-1"], "--seed -1")):
        with pytest.raises(SystemExit, match=msg):
            tstr.main(base + flags)


# ---- the C-ABI entries validate on the host -----------------------------------------------------------------------------------------

def test_abi_entries_reject_bad_arguments_without_a_device():
    from csl_gan_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert {"cslgan_tree_best_split_ws_bytes", "cslgan_tree_best_split_u8", "cslgan_tree_apply_u8"} <= set(_lib.EXPORTS)
    err = lambda: L.cslgan_last_error()
    wsb = L.cslgan_tree_best_split_ws_bytes
    for s, d in ((0, 784), (-1, 784), (10, 0), (10, 65537), (2 ** 31 // 49 + 1, 784), (2 ** 19, 65536)):
        assert wsb(s, d) == 0, (s, d)
    assert wsb(1, 1) == 40 and wsb(3, 17) == 240 and wsb(300, 12288) == 300 * 768 * 40 and wsb(2 ** 19 - 1, 65536) > 0
    need = wsb(5, 930)
    ok = dict(X=16, lab=16, W=None, B=0, N=100, D=930, K=10, rows=16, R=100, off=16, cls=16, wrow=None, tree=None, node=None, S=5, thr=0, seed=0, out=16,
              score=16, ws=16, wsn=need)

    def bs(**kw):
        a = dict(ok, **kw)
        return L.cslgan_tree_best_split_u8(a["X"], a["lab"], a["W"], a["B"], a["N"], a["D"], a["K"], a["rows"], a["R"], a["off"], a["cls"], a["wrow"], a["tree"],
                                           a["node"], a["S"], a["thr"], a["seed"], a["out"], a["score"], a["ws"], a["wsn"], None)

    for name in ("X", "lab", "rows", "off", "cls", "out", "score", "ws"):
        assert bs(**{name: None}) == -1 and b"null" in err(), name
    for k in (1, 17):
        assert bs(K=k) == -1 and b"K=" in err()
    for d in (0, -1, 65537):
        assert bs(D=d) == -1 and b"D=" in err()
    for n in (0, 2 ** 24):
        assert bs(N=n) == -1 and b"N=" in err()
    for r in (-1, 2 ** 31):
        assert bs(R=r) == -1 and b"R=" in err()
    assert bs(S=0) == -1 and b"S=" in err()
    assert bs(S=2 ** 31 // 59 + 1, wsn=2 ** 62) == -1 and b"S=" in err()
    assert bs(wsn=need - 1) == -1 and b"workspace" in err()
    assert bs(W=16) == -1 and b"seg_wrow" in err()
    assert bs(W=16, wrow=16, B=0) == -1 and b"n_wrows" in err()
    assert bs(thr=5) == -1 and b"mask" in err()
    assert bs(thr=5, tree=16) == -1 and b"mask" in err()
    assert bs(X=17) == -1 and b"X misaligned" in err()
    for name in ("lab", "rows", "off", "cls", "out"):
        assert bs(**{name: 18}) == -1 and b"int32 array misaligned" in err(), name
    assert bs(score=20) == -1 and b"misaligned (8 bytes)" in err()
    assert bs(ws=20) == -1 and b"misaligned (8 bytes)" in err()

    def ap(X=16, M=10, D=930, f=16, t=16, c=16, off=16, T=2, Q=7, leaf=16):
        return L.cslgan_tree_apply_u8(X, M, D, f, t, c, off, T, Q, leaf, None)

    for name in ("X", "f", "t", "c", "off", "leaf"):
        assert ap(**{name: None}) == -1 and b"null" in err(), name
    for d in (0, 65537):
        assert ap(D=d) == -1 and b"D=" in err()
    for m in (0, 2 ** 31):
        assert ap(M=m) == -1 and b"M=" in err()
    for t in (0, 65536):
        assert ap(T=t, Q=70000) == -1 and b"T=" in err()
    assert ap(Q=1) == -1 and b"Q=" in err()
    assert ap(f=18) == -1 and b"misaligned" in err()


def test_ops_have_no_cpu_path():
    from csl_gan_amd import ops
    X = torch.zeros((8, 20), dtype=torch.uint8)
    i32 = lambda *a: torch.zeros(a, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.tree_best_split_u8(X, i32(8), 2, i32(8), i32(2), i32(1))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.tree_apply_u8(X, i32(1), i32(1), i32(1), i32(2))
