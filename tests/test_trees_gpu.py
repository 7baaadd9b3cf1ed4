"""The device path of csl_gan_amd.classify.Trees (-m gpu): cslgan_tree_best_split_u8 and cslgan_tree_apply_u8 against
their host models — every integer and the bits of every score — the device fit against the host fit on the three problems of
tests/test_tstr.py, and the command line on cuda:0 against -d cpu.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import torch

from test_tstr import PROBLEMS, make, make_caches

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 2), (2, 1, 2), (17, 5, 3), (257, 930, 10), (300, 1040, 2), (100, 12288, 2), (20, 65536, 16)]


def _dev(a, dtype=np.int32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _check_split(X, y, K, rows, off, cls, W=None, wrow=None, key=None, thr=0, seed=0):
    """One launch against the host model; the outputs are handed over filled with -1; a second call returns the same bits.  Returns
    the host's (out, score) as numpy."""
    from csl_gan_amd import _lib, classify, ops
    S = len(cls)
    ho, hs = classify.best_split_host_bytes(X, y, rows, off, cls, seg_wrow=wrow, weights=W, seg_key=key, mask_thr=thr, seed=seed)
    args = (_dev(X, np.uint8), _dev(y), K, _dev(rows), _dev(off), _dev(cls))
    kw = dict(seg_wrow=_dev(wrow), weights=_dev(W), seg_key=None if key is None else (_dev(key[0]), _dev(key[1])), mask_thr=thr, seed=seed)
    out = (torch.full((S, 7), -1, dtype=torch.int32, device="cuda"), torch.full((S,), -1, dtype=torch.int64, device="cuda"))
    got = ops.tree_best_split_u8(*args, out=out, **kw)
    assert got[0] is out[0] and got[1] is out[1] and _lib.lib().cslgan_last_kernel() == b"tree_split_tile_kernel"
    go, gs = out[0].cpu().numpy(), out[1].cpu().numpy()
    bad = np.nonzero((go != ho.numpy()).any(1) | (gs != hs.numpy()))[0]
    assert len(bad) == 0, "segments %s: device %s, host %s" % (bad[:5], go[bad[:5]].tolist(), ho.numpy()[bad[:5]].tolist())
    again = ops.tree_best_split_u8(*args, **kw)
    assert np.array_equal(again[0].cpu().numpy(), go) and np.array_equal(again[1].cpu().numpy(), gs)
    return go, gs


def _random_segments(rng, N, S):
    """A permutation of the rows cut into S segments (some may be empty)."""
    cuts = np.sort(rng.integers(0, N + 1, S - 1)) if S > 1 else np.zeros(0, dtype=np.int64)
    return rng.permutation(N), np.concatenate([[0], cuts, [N]])


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_best_split_equals_the_host_model(N, D, K):
    """Per shape: every class on all rows (unmasked, unit weights); then random segments with bootstrap-like weights, masked and
    unmasked.  Coarse bytes (multiples of 32) on half of the columns make equal scores in different features and tiles common."""
    from csl_gan_amd import classify
    rng = np.random.default_rng(N + D)
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    X[:, ::2] = X[:, ::2] // 32 * 32
    y = rng.integers(0, K, N)
    rows = np.tile(np.arange(N), K)                                                  # segment k: all rows, class k
    go, _ = _check_split(X, y, K, rows, np.arange(K + 1) * N, np.arange(K))
    assert (go[:, 5] == N).all() and np.array_equal(go[:, 6], np.bincount(y, minlength=K))
    S = min(7, N + 1)
    r, off = _random_segments(rng, N, S)
    cls = rng.integers(0, K, S)
    W = rng.integers(0, 4, (3, N))
    wrow = rng.integers(-1, 3, S)
    key = (rng.integers(0, 100, S), rng.integers(0, 5000, S))
    thr = classify.tree_mask_threshold(max(1, int(np.sqrt(D))), D)
    _check_split(X, y, K, r, off, cls, W, wrow)
    go, _ = _check_split(X, y, K, r, off, cls, W, wrow, key, thr, seed=11)
    if thr:
        for s in np.nonzero(go[:, 0] >= 0)[0]:
            assert classify.tree_feature_mask(11, key[0][s], key[1][s], D, thr)[go[s, 0]]


def test_best_split_of_many_small_segments_in_one_launch():
    rng = np.random.default_rng(1)
    sizes = rng.integers(1, 41, 300)
    N = int(sizes.sum())
    X = (rng.integers(0, 256, (N, 50)) // 16 * 16).astype(np.uint8)
    y = rng.integers(0, 4, N)
    go, _ = _check_split(X, y, 4, rng.permutation(N), np.concatenate([[0], np.cumsum(sizes)]), rng.integers(0, 4, 300))
    assert np.array_equal(go[:, 5], sizes) and (go[sizes == 1, 0] == -1).all() and (go[sizes >= 8, 0] >= 0).all()


def test_counters_do_not_wrap():
    """70 000 rows of 8 bytes in one segment, every byte of the positive class 255: one bin holds more than a 16-bit counter and pL pL
    more than 32 bits.  Then weights up to 65 535: sum w close to 2^31, the products close to 2^62."""
    rng = np.random.default_rng(2)
    N = 70000
    y = (rng.random(N) < 0.95).astype(np.int64)
    X = np.where(y[:, None] == 1, 255, rng.integers(0, 255, (N, 8))).astype(np.uint8)
    go, gs = _check_split(X, y, 2, np.arange(N), [0, N], [1])
    p = int(y.sum())
    assert p > 65535 and go[0].tolist()[3:] == [N - p, 0, N, p] and go[0, 2] == 255 and gs.view(np.float64)[0] == float(p)
    go, _ = _check_split(X, y, 2, np.arange(N), [0, N], [0])                         # the same node seen from the other class
    assert go[0].tolist()[3:] == [N - p, N - p, N, N - p]
    N = 32000
    W = rng.integers(0, 65536, (2, N))
    W[1, :7] = 65535
    y = rng.integers(0, 2, N)
    X = rng.integers(0, 256, (N, 20)).astype(np.uint8)
    X[:, 5] = np.where(y == 1, 200, 100)                                             # two bins hold everything
    go, _ = _check_split(X, y, 2, np.tile(np.arange(N), 2), [0, N, 2 * N], [1, 1], W, [0, 1])
    assert int(W.sum(1).max()) < 2 ** 31 and go[:, 5].tolist() == W.sum(1).tolist() and go[:, 0].tolist() == [5, 5]
    assert (go[:, 6].astype(np.int64) ** 2 > 2 ** 57).all()                          # pR pR: beyond what float64 holds exactly


def test_duplicate_columns_in_different_tiles_and_labels_outside_the_classes():
    rng = np.random.default_rng(3)
    N, D = 400, 100
    y = rng.integers(-3, 6, N)                                                       # K = 3: labels -3 .. -1 and 3 .. 5 belong to no class
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    X[:, 70] = np.where(y == 1, 180, 60) + rng.integers(0, 20, N)                    # the best feature of class 1 ...
    X[:, 35] = X[:, 70]                                                              # ... twice, in tiles 2 and 4: the smaller j wins
    X[:, 99] = X[:, 70]
    go, _ = _check_split(X, y, 3, np.tile(np.arange(N), 3), np.arange(4) * N, [0, 1, 2])
    assert go[1, 0] == 35 and go[:, 6].tolist() == [int((y == k).sum()) for k in range(3)]
    go, _ = _check_split(X[:, 36:], y, 3, np.arange(N), [0, N], [1])                 # rows of 64 bytes: the aligned loader
    assert go[0, 0] == 34


def _random_trees(rng, T, D, max_nodes):
    """Flat tables of T random trees in creation order (the first tree is a single node)."""
    feature, threshold, child, off = [], [], [], [0]
    for t in range(T):
        budget = 1 if t == 0 else int(rng.integers(3, max_nodes + 1)) | 1
        f, th, c, n = [], [], [], 1
        q = 0
        while q < n:
            if n + 2 <= budget and (q == 0 or rng.random() < 0.7):
                f.append(int(rng.integers(0, D))); th.append(int(rng.integers(0, 255))); c.append(n)
                n += 2
            else:
                f.append(-1); th.append(0); c.append(-1)
            q += 1
        feature += f; threshold += th; child += c
        off.append(off[-1] + n)
    return feature, threshold, child, off


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_apply_equals_the_host_model(N, D, K):
    from csl_gan_amd import _lib, classify, ops
    rng = np.random.default_rng(D)
    X = rng.integers(0, 256, (N, D)).astype(np.uint8)
    tabs = _random_trees(rng, 9, D, 61)
    want = classify.tree_apply_host_bytes(X, *tabs).numpy()
    out = torch.full((9, N), -7, dtype=torch.int32, device="cuda")
    got = ops.tree_apply_u8(_dev(X, np.uint8), *(_dev(t) for t in tabs), out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), want) and _lib.lib().cslgan_last_kernel() == b"tree_apply_kernel"
    assert (want[0] == 0).all() and (want >= 0).all()
    f = np.array(tabs[0])
    for t in range(9):
        assert (f[tabs[3][t] + want[t]] == -1).all()                                 # every row ends in a leaf


@functools.lru_cache(maxsize=None)
def _host_trees(i, kind):
    """(fitted host classifier, report, P on the held-out rows, train (x, y), held-out x) of PROBLEMS[i]; computed once, left unchanged."""
    from csl_gan_amd import classify
    N, H, W, C, K, M = PROBLEMS[i]
    x, y = make(N, H, W, C, K, 1)
    xt, _ = make(M, H, W, C, K, 2)
    clf = classify.Trees(K, kind, n_trees=4, seed=5)
    rep = clf.fit_bytes(x, y)
    return clf, rep, clf.predict_proba_bytes(xt).numpy(), (x, y), xt


@pytest.mark.parametrize("kind", ["dt", "rf"])
@pytest.mark.parametrize("i", range(len(PROBLEMS)))
def test_device_fit_equals_the_host_fit(i, kind):
    from csl_gan_amd import classify
    host, rep, P, (x, y), xt = _host_trees(i, kind)
    clf = classify.Trees(PROBLEMS[i][4], kind, n_trees=4, seed=5)
    rep_d = clf.fit_bytes(torch.from_numpy(x).cuda(), torch.from_numpy(y))
    assert rep_d == rep
    assert clf.coef.device.type == "cpu" and np.array_equal(clf.coef.numpy(), host.coef.numpy())
    xd = torch.from_numpy(xt).cuda()
    assert np.array_equal(clf.apply_bytes(xd).numpy(), host.apply_bytes(xt).numpy())
    Pd = clf.predict_proba_bytes(xd).numpy()
    assert np.array_equal(Pd.view(np.uint64), P.view(np.uint64))


@pytest.mark.parametrize("flags", [["--classifier", "dt"], ["--classifier", "rf", "--n_trees", "4"]])
def test_cli_on_the_device_agrees_with_the_cpu(tmp_path, flags):
    from csl_gan_amd import tstr
    c = make_caches(tmp_path)
    res = {}
    for dev in ("cpu", "cuda:0"):
        vals = str(tmp_path / ("vals_" + dev[:3]))
        res[dev] = (tstr.main(["--syn_cache", c["syn"][0], "--test_cache", c["test"][0], "-d", dev, "--values_dir", vals] + flags), vals)
    assert res["cpu"][0] == res["cuda:0"][0] and res["cpu"][0]["syn"]["classifier"] == flags[1]
    for name in ("syn_P.npy", "syn_U.npy"):
        a, b = (np.load(os.path.join(res[d][1], name)) for d in ("cpu", "cuda:0"))
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
