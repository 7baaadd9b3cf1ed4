"""Precision / recall / density / coverage on the CPU: the host models of csl_gan_amd.neighbours.kth_host and
csl_gan_amd.manifold against brute-force loops over Python integers, the metrics on configurations worked out by hand, and the
command on `-d cpu`.  Every comparison is integer equality."""
import json
import os

import numpy as np
import pytest
import torch

from csl_gan_amd import manifold as MF
from csl_gan_amd import neighbours as NB

NONE = int(NB.NONE_KEY)


def _loop_d2(Q, R):
    Q, R = Q.reshape(len(Q), -1).tolist(), R.reshape(len(R), -1).tolist()
    return [[sum((a - b) ** 2 for a, b in zip(q, r)) for r in R] for q in Q]


def _loop_kth(Q, R, k, index_base=0, self_base=-1, best=None):
    d2 = _loop_d2(Q, R)
    out = []
    for i, row in enumerate(d2):
        keys = [] if best is None else [int(v) for v in best[i] if int(v) != NONE]
        keys += [(d << 32) | (index_base + j) for j, d in enumerate(row) if not (self_base >= 0 and index_base + j == self_base + i)]
        keys = sorted(keys)[:k]
        out.append(keys + [NONE] * (k - len(keys)))
    return np.array(out, dtype=np.uint64)


def _loop_counts(Q, R, radii):
    return np.array([sum(1 for d, t in zip(row, radii) if d <= int(t)) for row in _loop_d2(Q, R)], dtype=np.int64)


def _rows(seed, nq=9, nr=23, D=7):
    rng = np.random.default_rng(seed)
    Q, R = rng.integers(0, 256, (nq, D), dtype=np.uint8), rng.integers(0, 256, (nr, D), dtype=np.uint8)
    R[20], R[11], R[3] = R[2], R[2], R[2]                 # four rows with the same bytes: ties that the index decides
    Q[4] = R[2]
    return Q, R


# ---- the host models against brute force ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 8])
def test_kth_host_equals_a_brute_force_loop(k):
    Q, R = _rows(1)
    got = NB.kth_host(Q, R, k, block=5)
    assert got.dtype == np.uint64 and np.array_equal(got, _loop_kth(Q, R, k))
    assert got[4].tolist()[:min(k, 4)] == [2, 3, 11, 20][:k]          # d2 = 0 four times: ascending indices
    assert np.array_equal(NB.kth_host(Q, R, k, index_base=77), _loop_kth(Q, R, k, index_base=77))


def test_a_row_is_excluded_by_its_index_and_a_twin_stays_at_distance_zero():
    _, X = _rows(2)
    got = NB.kth_host(X, X, 3, self_base=0, block=4)
    assert np.array_equal(got, _loop_kth(X, X, 3, self_base=0))
    d2, idx = NB.split_keys(got)
    assert not (idx == np.arange(len(X))[:, None]).any()
    assert d2[2].tolist() == [0, 0, 0] and idx[2].tolist() == [3, 11, 20] and idx[11].tolist() == [2, 3, 20]
    assert (d2[[0, 1, 5], 0] > 0).all()                                # rows without a twin: the own row was the only zero
    # shifted bases: a block of queries that starts at row 5 of the set
    assert np.array_equal(NB.kth_host(X[5:], X, 3, index_base=100, self_base=105), _loop_kth(X[5:], X, 3, 100, 105))
    assert np.array_equal(NB.kth_host(X, X, 3, self_base=-1)[:, 0] >> np.uint64(32), np.zeros(len(X), dtype=np.uint64))


def test_three_calls_over_thirds_equal_one_call_and_smaller_keys_in_best_survive():
    Q, R = _rows(3)
    want = NB.kth_host(Q, R, 5)
    best = None
    for r0, r1 in ((16, 23), (0, 8), (8, 16)):                         # disjoint index ranges, in any order
        best = NB.kth_host(Q, R[r0:r1], 5, index_base=r0, best=best)
    assert np.array_equal(best, want)
    pre = np.full((len(Q), 5), NB.NONE_KEY, dtype=np.uint64)
    pre[:, 0], pre[:, 1] = np.uint64(1000), np.uint64((1 << 32) | 1001)   # smaller than anything but a duplicate brings
    got = NB.kth_host(Q, R, 5, best=pre)
    assert np.array_equal(got, _loop_kth(Q, R, 5, best=pre))
    assert np.array_equal(got[0, :2], pre[0, :2]) and np.array_equal(got[0, 2:], want[0, :3])
    assert got[4].tolist() == [2, 3, 11, 20, 1000]
    assert (pre[:, 2:] == NB.NONE_KEY).all()                            # the argument is not written


def test_fewer_than_k_candidates_leave_all_ones_tails():
    Q, R = _rows(4)
    got = NB.kth_host(Q, R[:3], 8)
    assert np.array_equal(got, _loop_kth(Q, R[:3], 8)) and (got[:, 3:] == NB.NONE_KEY).all() and (got[:, :3] != NB.NONE_KEY).all()
    two = NB.kth_host(R[:3], R[:3], 3, self_base=0)
    assert (two[:, 2] == NB.NONE_KEY).all() and (two[:, :2] != NB.NONE_KEY).all()
    with pytest.raises(ValueError, match="not full"):
        MF.knn_radii(two)                                               # a set of k rows has no k-th OTHER row
    assert MF.knn_radii(two[:, :2]).tolist() == [int(v) >> 32 for v in two[:, 1]]


def test_kth_host_refuses():
    Q, R = _rows(5)
    for k in (0, 9):
        with pytest.raises(ValueError, match="k = "):
            NB.kth_host(Q, R, k)
    with pytest.raises(ValueError, match="index_base"):
        NB.kth_host(Q, R, 2, index_base=2 ** 32 - 1 - len(R) + 1)
    with pytest.raises(ValueError, match="self_base"):
        NB.kth_host(Q, R, 2, self_base=-2)
    with pytest.raises(ValueError, match="self_base"):
        NB.kth_host(Q, R, 2, self_base=2 ** 32 - len(Q))
    with pytest.raises(ValueError, match="best has shape"):
        NB.kth_host(Q, R, 2, best=np.zeros((len(Q), 3), dtype=np.uint64))
    with pytest.raises(ValueError, match="bytes"):
        NB.kth_host(Q, R[:, :5], 2)


def test_count_within_radii_host_equals_a_brute_force_loop():
    Q, R = _rows(6)
    d2 = np.array(_loop_d2(Q, R))
    radii = np.sort(d2, axis=0)[len(Q) // 2].copy()                     # per reference row the median over the queries: ties with <=
    radii[2], radii[3], radii[7] = 0, 0, 2 ** 32 - 1
    got = MF.count_within_radii_host(Q, R, radii, block=4)
    assert got.dtype == np.int64 and np.array_equal(got, _loop_counts(Q, R, radii))
    assert (d2 == radii[None, :]).any() and not np.array_equal(got, (d2 < radii[None, :]).sum(1))     # `<` is another function
    assert got[4] >= 3                                                  # d2 = 0 counts at radius 0: rows 2 and 3, and the all-ones row
    halves = MF.count_within_radii_host(Q, R[:10], radii[:10])
    assert np.array_equal(MF.count_within_radii_host(Q, R[10:], radii[10:], counts=halves), got)
    for bad in (radii[:5], radii.astype(np.float64), np.where(np.arange(len(R)) == 1, -1, radii), np.where(np.arange(len(R)) == 1, 2 ** 32, radii)):
        with pytest.raises(ValueError, match="radii"):
            MF.count_within_radii_host(Q, R, bad)


# ---- the metrics ---------------------------------------------------------------------------------------------------------------------------

def _cache(x):
    from csl_gan_amd.pipeline import CachedImages
    x = np.asarray(x, dtype=np.uint8)
    return CachedImages.from_arrays(x.reshape((len(x), 1, 1, -1)) if x.ndim < 4 else x, np.zeros(len(x)), True)


def _prdc(real, syn, k):
    v = MF.run_prdc(_cache(real), _cache(syn), k)
    return v, MF.prdc_metrics(v["counts_syn"], v["counts_real"], v["d2min_real"], v["rad_real"], k)


def test_metrics_on_a_line_worked_out_by_hand():
    """D = 1, k = 1.  X = 10 12 20 50, S = 11 13 21 100.
    rad_X = 4 4 64 900 (nearest other: 12, 10, 12, 20); rad_S = 4 4 64 6241 (13, 11, 13, 21).
    c[11] = {10, 12} = 2 (81 > 64 misses 20); c[13] = {12, 20} = 2 (9 > 4 misses 10, 49 <= 64); c[21] = {20, 50} = 2 (841 <= 900);
    c[100] = 0 (2500 > 900)                                       -> precision 3, density 6.
    x = 10, 12 lie inside 11's ball (1 <= 4), 20 inside 21's (1 <= 64), 50 inside 100's (2500 <= 6241)       -> recall 4.
    min_s d2 = 1 1 1 841 against rad_X 4 4 64 900                                                             -> coverage 4."""
    v, m = _prdc([10, 12, 20, 50], [11, 13, 21, 100], 1)
    assert v["rad_real"].tolist() == [4, 4, 64, 900] and v["rad_syn"].tolist() == [4, 4, 64, 6241]
    assert v["counts_syn"].tolist() == [2, 2, 2, 0] and v["d2min_real"].tolist() == [1, 1, 1, 841]
    assert m == {"n_real": 4, "n_syn": 4, "k": 1, "precision_hits": 3, "density_sum": 6, "recall_hits": 4, "coverage_hits": 4,
                 "precision": 0.75, "density": 1.5, "recall": 1.0, "coverage": 1.0}


def test_metrics_with_two_neighbours_worked_out_by_hand():
    """D = 1, k = 2.  X = 0 1 3 7, S = 2 8 30.
    rad_X (second nearest other) = 9 4 9 36; rad_S = 784 484 784 (of 2: 8 and 30; of 8: 2 and 30; of 30: 8 and 2).
    c[2] = {0: 4 <= 9, 1: 1 <= 4, 3: 1 <= 9, 7: 25 <= 36} = 4; c[8] = {7: 1 <= 36} = 1 (25 > 9 misses 3); c[30] = 0
                                                                   -> precision 2, density 5 / (2 * 3).
    every x lies inside 2's ball of 784                            -> recall 4.
    min_s d2 = 4 1 1 1 against 9 4 9 36                            -> coverage 4."""
    v, m = _prdc([0, 1, 3, 7], [2, 8, 30], 2)
    assert v["rad_real"].tolist() == [9, 4, 9, 36] and v["rad_syn"].tolist() == [784, 484, 784]
    assert v["counts_syn"].tolist() == [4, 1, 0]
    assert (m["precision_hits"], m["density_sum"], m["recall_hits"], m["coverage_hits"]) == (2, 5, 4, 4)
    assert m["density"] == 5 / 6 and m["precision"] == 2 / 3


def test_a_copy_scores_one_and_far_clusters_score_zero_and_half_inside_scores_a_half():
    rng = np.random.default_rng(8)
    X = rng.integers(0, 60, (40, 2, 2, 3), dtype=np.uint8)
    _, m = _prdc(X, X.copy(), 3)
    assert (m["precision"], m["recall"], m["coverage"]) == (1.0, 1.0, 1.0) and m["density_sum"] >= 40
    far = (X[:30] + 190).astype(np.uint8)                               # every byte > 130 away from every real byte: beyond any radius
    _, m = _prdc(X, far, 3)
    assert (m["precision_hits"], m["density_sum"], m["recall_hits"], m["coverage_hits"]) == (0, 0, 0, 0)
    assert (m["precision"], m["density"], m["recall"], m["coverage"]) == (0.0, 0.0, 0.0, 0.0)
    half = np.concatenate([X[:15], far[:15]])
    _, m = _prdc(X, half, 3)
    assert m["precision_hits"] == 15 and m["precision"] == 0.5 and m["n_syn"] == 30


def test_the_compare_is_less_or_equal():
    """X = 0 2, S = 4 100, k = 1: rad_X = 4 4 and d2(4, 2) = 4, an exact tie.  `<=` puts the sample inside 2's ball; `<` would not."""
    v, m = _prdc([0, 2], [4, 100], 1)
    assert v["rad_real"].tolist() == [4, 4] and v["counts_syn"].tolist() == [1, 0] and m["precision_hits"] == 1
    d2 = np.array(_loop_d2(np.array([[4], [100]]), np.array([[0], [2]])))
    assert ((d2 < v["rad_real"][None, :]).sum(1) > 0).sum() == 0


def test_metrics_and_sizes_refuse():
    with pytest.raises(ValueError, match="at least 3"):
        MF.run_prdc(_cache([1, 2]), _cache([1, 2, 3]), 2)
    with pytest.raises(ValueError, match="at least 3"):
        MF.run_prdc(_cache([1, 2, 3]), _cache([1, 2]), 2)
    for k in (0, 9):
        with pytest.raises(ValueError, match="k = "):
            MF.run_prdc(_cache(np.arange(20)), _cache(np.arange(20)), k)
        with pytest.raises(ValueError, match="k = "):
            MF.prdc_metrics([1], [1], [1], [1], k)
    with pytest.raises(ValueError):
        MF.prdc_metrics([1, 2], [1, 0], [3], [4, 4], 1)
    s = NB.NearestSearch("cpu").fit(_cache(np.arange(20)))
    with pytest.raises(ValueError, match="fitted reference"):
        s.kth(_cache(np.arange(20)), 2, exclude_self=True)
    with pytest.raises(ValueError, match="k = "):
        s.kth(s.ref, 9)
    with pytest.raises(ValueError, match="radii"):
        s.count_within_radii(s.ref, np.zeros(19, dtype=np.int64))
    with pytest.raises(RuntimeError, match="fit"):
        NB.NearestSearch("cpu").kth(_cache(np.arange(20)), 2)


def test_ops_refuse_cpu_tensors_and_wrong_types():
    from csl_gan_amd import ops
    z8, z32 = torch.zeros(4, 64, dtype=torch.int8), torch.zeros(4, dtype=torch.int32)
    best = torch.full((4, 3), -1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.nn_kth(z8, z32, z8, z32, 0, best)
    with pytest.raises(RuntimeError, match="best must be a contiguous int64"):
        ops.nn_kth(z8, z32, z8, z32, 0, best.to(torch.int32))
    with pytest.raises(RuntimeError, match="q must be a contiguous int8"):
        ops.nn_kth(z8.to(torch.uint8), z32, z8, z32, 0, best)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.nn_count_radius(z8, z32, z8, z32, z32, z32.clone())
    with pytest.raises(RuntimeError, match="radius must be a contiguous int32"):
        ops.nn_count_radius(z8, z32, z8, z32, z32.to(torch.int64), z32.clone())
    with pytest.raises(RuntimeError, match="counts must be a contiguous int32"):
        ops.nn_count_radius(z8, z32, z8, z32, z32, z32.to(torch.int64))


# ---- the command line on the CPU -------------------------------------------------------------------------------------------------------------

HWC = (4, 3, 2)


def _write(path, x):
    from csl_gan_amd.generate import CacheWriter
    n, H, W, C = x.shape
    w = CacheWriter(path, n, H, W, C, True, {"note": "test rows"})
    w(0, x, np.zeros(n, dtype=np.int64))
    w.close()


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("prdc")) + "/"
    rng = np.random.default_rng(7)
    x = {"train": rng.integers(0, 256, (40,) + HWC, dtype=np.uint8), "heldout": rng.integers(0, 256, (45,) + HWC, dtype=np.uint8),
         "syn": rng.integers(0, 256, (30,) + HWC, dtype=np.uint8), "syn2": rng.integers(0, 256, (12,) + HWC, dtype=np.uint8),
         "few": rng.integers(0, 256, (3,) + HWC, dtype=np.uint8)}
    x["syn"][:20] = x["train"][:20]                      # a generator that copied half of the training set, one bit off
    x["syn"][:20, 0, 0, 0] ^= 1
    for k, v in x.items():
        _write(d + k, v)
    _write(d + "odd", rng.integers(0, 256, (9, 3, 4, 2), dtype=np.uint8))
    os.makedirs(d + "other")
    _write(d + "other/syn", x["syn2"])
    return d, x


def test_cli_on_the_cpu(caches, tmp_path):
    from csl_gan_amd import prdc
    d, x = caches
    out, vals = str(tmp_path / "outputs"), str(tmp_path / "values")
    stats = prdc.main(["--syn_cache", d + "syn", d + "syn2", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "--baseline",
                       "-k", "3", "-d", "cpu", "--values_dir", vals, "--save", "--outputs_dir", out, "--name", "q"])
    assert list(stats) == ["syn", "syn2", "baseline_heldout"]
    keys = {"n_real", "n_syn", "k", "precision_hits", "density_sum", "recall_hits", "coverage_hits", "precision", "density", "recall", "coverage"}
    for lab, n in (("syn", 30), ("syn2", 12), ("baseline_heldout", 45)):
        m = stats[lab]
        assert set(m) == keys and (m["n_real"], m["n_syn"], m["k"]) == (40, n, 3)
        # against the definitions, pair by pair
        S = x["heldout" if lab.startswith("baseline") else lab]
        rad_x = MF.knn_radii(_loop_kth(x["train"], x["train"], 3, self_base=0))
        rad_s = MF.knn_radii(_loop_kth(S, S, 3, self_base=0))
        cs, cr = _loop_counts(S, x["train"], rad_x), _loop_counts(x["train"], S, rad_s)
        dm = np.array(_loop_d2(x["train"], S)).min(1)
        assert (m["precision_hits"], m["density_sum"], m["recall_hits"], m["coverage_hits"]) == \
            (int((cs > 0).sum()), int(cs.sum()), int((cr > 0).sum()), int((dm <= rad_x).sum()))
        assert (m["precision"], m["density"]) == (m["precision_hits"] / n, m["density_sum"] / (3 * n))
        assert (m["recall"], m["coverage"]) == (m["recall_hits"] / 40, m["coverage_hits"] / 40)
        load = lambda name: np.load(os.path.join(vals, "%s_%s.npy" % (lab, name)))
        assert load("counts_syn").dtype == np.int64 and np.array_equal(load("counts_syn"), cs) and np.array_equal(load("counts_real"), cr)
        assert np.array_equal(load("rad_syn"), rad_s) and np.array_equal(load("d2min_real"), dm)
    assert np.array_equal(np.load(os.path.join(vals, "rad_real.npy")), rad_x) and len(os.listdir(vals)) == 13
    assert stats["syn"]["precision_hits"] >= 20 and stats["syn"]["coverage_hits"] >= 20      # the copies lie inside, one bit away
    # the JSON on disk is what was returned, and a second run merges into it
    with open(os.path.join(out, "q.json")) as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    again = prdc.main(["--syn_cache", d + "heldout", "--train_cache", d + "train", "-d", "cpu", "--save", "--outputs_dir", out, "--name", "q"])
    assert list(again) == ["heldout"] and again["heldout"]["k"] == 5
    with open(os.path.join(out, "q.json")) as f:
        merged = json.load(f)
    assert set(merged) == {"syn", "syn2", "baseline_heldout", "heldout"} and merged["syn"] == json.loads(json.dumps(stats["syn"]))


def test_cli_refusals(caches):
    from csl_gan_amd import prdc
    d, _ = caches
    base = ["--train_cache", d + "train", "-d", "cpu"]
    with pytest.raises(SystemExit, match="one geometry"):
        prdc.main(["--syn_cache", d + "odd"] + base)
    with pytest.raises(SystemExit, match="one geometry"):
        prdc.main(["--syn_cache", d + "syn", "--nontrain_cache", d + "odd", "--baseline"] + base)
    for k in ("0", "9"):
        with pytest.raises(SystemExit, match="-k"):
            prdc.main(["--syn_cache", d + "syn", "-k", k] + base)
    with pytest.raises(SystemExit, match="few holds 3 images"):
        prdc.main(["--syn_cache", d + "few", "-k", "3"] + base)
    with pytest.raises(SystemExit, match="few holds 3 images"):
        prdc.main(["--syn_cache", d + "syn", "--train_cache", d + "few", "-d", "cpu", "-k", "3"])
    with pytest.raises(SystemExit, match="share the name"):
        prdc.main(["--syn_cache", d + "syn", d + "other/syn"] + base)
    with pytest.raises(SystemExit, match="--nontrain_cache"):
        prdc.main(["--syn_cache", d + "syn", "--baseline"] + base)
