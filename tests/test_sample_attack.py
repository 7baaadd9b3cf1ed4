"""csl_gan_amd.blackbox / csl_gan_amd.sample_attack without a GPU: the counting host model against a plain integer double loop, its
boundary, merging and range rules, the rank map, the eps^2 rule, the attack on a memorising and on an independent generator, the
driver and the command line on -d cpu, and the host-side argument checks of cslgan_nn_count_i8.  Counts are compared by equality."""
import json
import os

import numpy as np
import pytest
import torch

from csl_gan_amd import blackbox as BB
from csl_gan_amd import neighbours as NB

U32 = 2 ** 32 - 1


def _loop_d2(Q, R):
    Q, R = Q.reshape(len(Q), -1).astype(np.int64), R.reshape(len(R), -1).astype(np.int64)
    return [[int(((q - r) ** 2).sum()) for r in R] for q in Q]


def _loop_counts(Q, R, thr):
    """The definition, one pair at a time in Python integers."""
    return np.array([[sum(d <= t for d in row) for t in thr] for row in _loop_d2(Q, R)], dtype=np.int64).reshape(len(Q), len(thr))


@pytest.mark.parametrize("nq,nr,D", [(1, 1, 1), (5, 7, 3), (9, 4, 63), (6, 11, 130)])
def test_host_model_equals_a_double_loop(nq, nr, D):
    rng = np.random.default_rng(200 + D)
    Q, R = rng.integers(0, 256, (nq, D), dtype=np.uint8), rng.integers(0, 256, (nr, D), dtype=np.uint8)
    d = sorted(v for row in _loop_d2(Q, R) for v in row)
    for thr in ([d[len(d) // 2]], [d[-1], d[0], d[len(d) // 3]], [0, 1, U32, d[len(d) // 2] + 1]):        # unsorted on purpose
        got = BB.count_within_host(Q, R, thr)
        assert got.dtype == np.int64 and got.shape == (nq, len(thr)) and np.array_equal(got, _loop_counts(Q, R, thr))
        assert np.array_equal(BB.count_within_host(Q, R, thr, block=3), got)


def test_threshold_boundaries():
    rng = np.random.default_rng(1)
    R = rng.integers(0, 256, (20, 30), dtype=np.uint8)
    Q = R[[4, 9]].copy()
    Q[1, 3] ^= 2                                         # row 1: distance 4 to R[9], no duplicate
    R[15] = R[4]                                         # row 0: two exact duplicates
    d = np.array(_loop_d2(Q, R))
    t = int(d[1, 0])                                     # some pair's exact distance
    c = BB.count_within_host(Q, R, [t, t - 1, 0, U32])
    assert c[1, 0] == (d[1] <= t).sum() == c[1, 1] + (d[1] == t).sum() and (d[1] == t).sum() >= 1
    assert list(c[:, 2]) == [2, 0]                       # 0 counts exact duplicates only
    assert list(c[:, 3]) == [20, 20]                     # 2^32 - 1 counts every row
    assert BB.count_within_host(Q, R, [4])[1, 0] == 1 and BB.count_within_host(Q, R, [3])[1, 0] == 0


@pytest.mark.parametrize("block", [1, 2, 7, 64, 10 ** 6])
def test_merging_equals_one_call_and_block_does_not_matter(block):
    rng = np.random.default_rng(5)
    Q, R = rng.integers(0, 256, (13, 48), dtype=np.uint8), rng.integers(0, 256, (29, 48), dtype=np.uint8)
    thr = [450000, 600000, 0, 520000]
    one = _loop_counts(Q, R, thr)
    assert one.min() < one.max()
    assert np.array_equal(BB.count_within_host(Q, R, thr, block=block), one)
    first = BB.count_within_host(Q, R[:11], thr, block=block)
    keep = first.copy()
    two = BB.count_within_host(Q, R[11:], thr, counts=first, block=block)
    assert np.array_equal(two, one) and np.array_equal(first, keep)              # the argument is not written
    assert np.array_equal(BB.count_within_host(Q, R[:11], thr, counts=BB.count_within_host(Q, R[11:], thr)), one)


def test_distances_above_two_to_the_31_are_counted_exactly():
    D = 49152
    Q, R = np.zeros((2, D), dtype=np.uint8), np.full((3, D), 255, dtype=np.uint8)
    R[2, 0] = 254                                        # one row closer by 255^2 - 254^2 = 509
    d2 = 65025 * D
    assert d2 > 2 ** 31
    c = BB.count_within_host(Q, R, [d2, d2 - 1, d2 - 509, d2 - 510])
    assert c.tolist() == [[3, 1, 1, 0]] * 2


def test_the_host_model_refuses_what_it_cannot_hold():
    z = np.zeros((2, 4), dtype=np.uint8)
    for thr in ([], [1, 2, 3, 4, 5], [-1], [2 ** 32]):
        with pytest.raises(ValueError):
            BB.count_within_host(z, z, thr)
    with pytest.raises(ValueError):
        BB.count_within_host(z, np.zeros((2, 5), dtype=np.uint8), [1])
    with pytest.raises(ValueError):
        BB.count_within_host(z.astype(np.int8), z, [1])
    with pytest.raises(ValueError):
        BB.count_within_host(z, z, [1], counts=np.zeros((2, 2), dtype=np.int64))


# ---- the rank map and the eps^2 rule --------------------------------------------------------------------------------------------------

def test_dense_ranks_keep_order_and_ties_of_integers_that_float32_cannot_tell_apart():
    a, b = 2 ** 31, 2 ** 31 + 1
    assert np.float32(a) == np.float32(b)               # why the map is needed
    st, sn = np.array([b, -5, a, 7], dtype=np.int64), np.array([a, 7, 7, -(2 ** 32), b + 1], dtype=np.int64)
    rt, rn = BB.dense_ranks(st, sn)
    assert rt.dtype == np.float32 == rn.dtype
    # distinct pooled values: -2^32 < -5 < 7 < 2^31 < 2^31 + 1 < 2^31 + 2
    assert rt.tolist() == [4.0, 1.0, 3.0, 2.0] and rn.tolist() == [3.0, 2.0, 2.0, 0.0, 5.0]
    pooled, ranks = np.concatenate([st, sn]), np.concatenate([rt, rn])
    for i in range(len(pooled)):
        for j in range(len(pooled)):
            assert (pooled[i] < pooled[j]) == (ranks[i] < ranks[j]) and (pooled[i] == pooled[j]) == (ranks[i] == ranks[j])


def test_dense_ranks_refuse_more_distinct_values_than_float32_holds(monkeypatch):
    monkeypatch.setattr(BB, "MAX_DISTINCT", 5)
    BB.dense_ranks(np.arange(3), np.arange(2, 5))
    with pytest.raises(ValueError, match="distinct"):
        BB.dense_ranks(np.arange(3), np.arange(3, 6))


def test_eps2_is_element_floor_p_n_minus_1_of_the_sorted_array():
    d = np.array([40, 10, 30, 20, 70, 50, 60, 90, 80, 100, 110])                 # n = 11: sorted element k is 10 (k + 1)
    # p = 50 % -> floor(5.0) = 5 ; 10 % -> floor(1.0) = 1 ; 1 % -> floor(0.1) = 0 ; 99 % -> floor(9.9) = 9 ; 100 % -> 10
    assert BB.epsilon2(d, [50, 10, 1, 99]) == [60, 20, 10, 100]
    assert BB.epsilon2(d, [100, 0]) == [110, 10]
    assert BB.epsilon2(np.arange(1001)[::-1], [0.1, 29, 50]) == [1, 290, 500]    # 0.29 * 1000 is 289.99999999999994 in binary
    assert BB.epsilon2(np.arange(1000), BB.DEFAULT_PERCENTILES) == [499, 99, 9, 0]
    for bad in ([], [1, 2, 3, 4, 5], [-1], [101]):
        with pytest.raises(ValueError):
            BB.epsilon2(d, bad)


# ---- the attack ---------------------------------------------------------------------------------------------------------------------------

HWC = (4, 4, 3)                                          # D = 48


def _cache(x):
    from csl_gan_amd.pipeline import CachedImages
    return CachedImages.from_arrays(x, np.zeros(len(x)), True)


def _records(seed):
    rng = np.random.default_rng(seed)
    return rng, rng.integers(0, 256, (200,) + HWC, dtype=np.uint8), rng.integers(0, 256, (200,) + HWC, dtype=np.uint8)


def _metrics(S, train, heldout, percentiles=(50.0,), calib=None):
    v = BB.run_attack(_cache(S), _cache(train), _cache(heldout), percentiles)
    ref = BB.d2min_to(_cache(calib), (_cache(train), _cache(heldout))) if calib is not None else (None, None)
    return v, BB.sample_attack_metrics(v["d2_train"], v["d2_heldout"], v["counts_train"], v["counts_heldout"], percentiles, v["eps2"], len(S),
                                       ref[0], ref[1], pool=100, asr_iters=200)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_memorising_generator_is_caught_with_certainty(seed):
    rng, train, heldout = _records(seed)
    noise = rng.integers(-2, 3, train.shape)
    S = np.concatenate([np.clip(train.astype(np.int64) + noise, 0, 255).astype(np.uint8), rng.integers(0, 256, (100,) + HWC, dtype=np.uint8)])
    v, m = _metrics(S, train, heldout)
    assert v["d2_train"].max() <= 4 * 48 < v["d2_heldout"].min()
    assert v["eps2"] == [int(v["d2_train"].max())] and m["eps2"] == v["eps2"] and m["percentiles"] == [50.0]
    assert (m["n_train"], m["n_heldout"], m["n_syn"]) == (200, 200, 300)
    for name in ("fbb", "mc_p50"):
        s = m[name]
        assert s["auc"] == 1.0 and s["tpr_at_fpr_0.01"] == 1.0 and s["tpr_at_fpr_0.001"] == 1.0 and s["asr"] == 1.0, (name, s)
        assert (s["n"], s["m"], s["asr_iters"]) == (10, 90, 200)
    assert m["d2min_pooled"]["d2_min"] == int(v["d2_train"].min())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_an_independent_generator_is_not(seed):
    """Hanley-McNeil's sigma of an AUC of 0.5 at 200 + 200 is 0.029: the bound is five of them."""
    rng, train, heldout = _records(seed)
    S = rng.integers(0, 256, (300,) + HWC, dtype=np.uint8)
    _, m = _metrics(S, train, heldout)
    assert abs(m["fbb"]["auc"] - 0.5) < 0.15, m["fbb"]


def test_calibration_with_the_attacked_samples_themselves_knows_nothing():
    rng, train, heldout = _records(3)
    S = np.concatenate([train[:50], rng.integers(0, 256, (100,) + HWC, dtype=np.uint8)])
    v, m = _metrics(S, train, heldout, calib=S)
    ref = BB.d2min_to(_cache(S), (_cache(train), _cache(heldout)))               # the path the command line takes
    assert np.array_equal(ref[0], v["d2_train"]) and np.array_equal(ref[1], v["d2_heldout"]) and ref[0].dtype == np.int64
    scores = BB.attack_scores(v["d2_train"], v["d2_heldout"], d2ref_train=ref[0], d2ref_heldout=ref[1])
    assert not scores["cal"][0].any() and not scores["cal"][1].any() and scores["cal"][0].dtype == np.int64
    assert m["cal"]["auc"] == 0.5 and m["fbb"]["auc"] > 0.5
    # a calibration set that is farther from everything leaves the order of the plain attack
    far = BB.attack_scores([5, 9], [7], d2ref_train=[100, 100], d2ref_heldout=[100])
    assert far["cal"][0].tolist() == [95, 91] and far["cal"][1].tolist() == [93] and far["fbb"][0].tolist() == [-5, -9]


def test_count_within_on_the_cpu_is_the_host_model():
    rng = np.random.default_rng(6)
    ref, qry = _cache(rng.integers(0, 256, (37,) + HWC, dtype=np.uint8)), _cache(rng.integers(0, 256, (9,) + HWC, dtype=np.uint8))
    thr = [480000, 0, U32]
    s = NB.NearestSearch("cpu", block_rows=8).fit(ref)
    got = s.count_within(qry, thr)
    assert got.dtype == np.int64 and np.array_equal(got, _loop_counts(qry.x, ref.x, thr)) and 0 < got[:, 0].sum() < 9 * 37
    with pytest.raises(ValueError, match="one geometry"):
        s.count_within(_cache(np.zeros((2, 4, 3, 4), dtype=np.uint8)), thr)
    with pytest.raises(ValueError):
        s.count_within(qry, [1, 2, 3, 4, 5])
    with pytest.raises(RuntimeError, match="fit"):
        NB.NearestSearch("cpu").count_within(qry, thr)


# ---- the command line on the CPU ------------------------------------------------------------------------------------------------------

def _write(path, x):
    from csl_gan_amd.generate import CacheWriter
    n, H, W, C = x.shape
    w = CacheWriter(path, n, H, W, C, True, {"note": "test rows"})
    w(0, x, np.zeros(n, dtype=np.int64))
    w.close()


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sample_attack")) + "/"
    rng = np.random.default_rng(7)
    x = {"train": rng.integers(0, 256, (40,) + HWC, dtype=np.uint8), "heldout": rng.integers(0, 256, (45,) + HWC, dtype=np.uint8),
         "syn": rng.integers(0, 256, (30,) + HWC, dtype=np.uint8), "syn2": rng.integers(0, 256, (12,) + HWC, dtype=np.uint8),
         "ref": rng.integers(0, 256, (25,) + HWC, dtype=np.uint8), "few": rng.integers(0, 256, (10,) + HWC, dtype=np.uint8)}
    x["syn"][:20] = x["train"][:20]                      # a generator that memorised half of the training set
    x["syn"][:20, 0, 0, 0] ^= 1
    for k, v in x.items():
        _write(d + k, v)
    _write(d + "odd", rng.integers(0, 256, (4, 3, 4, 4), dtype=np.uint8))
    return d, x


POOL = ["--pool", "40", "--data_prop", "0.25", "--asr_iters", "50", "--seed", "3"]      # n = 10 of 40, m = 30 of 45


def test_cli_on_the_cpu(caches, tmp_path):
    from csl_gan_amd import sample_attack
    d, x = caches
    out, vals = str(tmp_path / "outputs"), str(tmp_path / "values")
    stats = sample_attack.main(["--syn_cache", d + "syn", d + "syn2", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "--calib_cache",
                                d + "ref", "--percentiles", "50", "10", "-d", "cpu", "--values_dir", vals, "--save", "--outputs_dir", out, "--name", "bb"]
                               + POOL)
    assert set(stats) == {"syn", "syn2"}
    m = stats["syn"]
    assert set(m) == {"n_train", "n_heldout", "n_syn", "percentiles", "eps2", "d2min_pooled", "fbb", "cal", "mc_p50", "mc_p10"}
    assert (m["n_train"], m["n_heldout"], m["n_syn"], m["percentiles"]) == (40, 45, 30, [50.0, 10.0])
    for name in ("fbb", "cal", "mc_p50", "mc_p10"):
        assert set(m[name]) == {"asr", "asr_stderr", "n", "m", "asr_iters", "auc", "tpr_at_fpr_0.01", "tpr_at_fpr_0.001"}
        assert (m[name]["n"], m[name]["m"], m[name]["asr_iters"]) == (10, 30, 50)
    # against the definitions, pair by pair
    dt, dh = np.array(_loop_d2(x["train"], x["syn"])).min(1), np.array(_loop_d2(x["heldout"], x["syn"])).min(1)
    pooled = np.sort(np.concatenate([dt, dh]))
    assert m["eps2"] == [int(pooled[42]), int(pooled[8])]                        # floor(.5 * 84), floor(.1 * 84)
    assert m["d2min_pooled"] == NB._order_stats(pooled) and m["d2min_pooled"]["d2_min"] == 1
    load = lambda name: np.load(os.path.join(vals, name + ".npy"))
    assert sorted(os.listdir(vals)) == sorted("%s_%s.npy" % (s, k) for s in ("syn", "syn2") for k in
                                              ("d2_train", "d2_heldout", "counts_train", "counts_heldout", "d2ref_train", "d2ref_heldout"))
    assert load("syn_d2_train").dtype == np.int64 and np.array_equal(load("syn_d2_train"), dt) and np.array_equal(load("syn_d2_heldout"), dh)
    assert np.array_equal(load("syn_counts_train"), _loop_counts(x["train"], x["syn"], m["eps2"]))
    assert np.array_equal(load("syn_counts_heldout"), _loop_counts(x["heldout"], x["syn"], m["eps2"]))
    assert np.array_equal(load("syn_d2ref_train"), np.array(_loop_d2(x["train"], x["ref"])).min(1))
    assert np.array_equal(load("syn2_d2ref_heldout"), load("syn_d2ref_heldout"))
    # half of the training set is memorised and nothing of the held-out set: every flagged record is a member
    assert m["fbb"]["auc"] > 0.6 and m["fbb"]["tpr_at_fpr_0.01"] >= 0.5 and m["mc_p10"]["tpr_at_fpr_0.001"] >= 8 / 40
    assert abs(stats["syn2"]["fbb"]["auc"] - 0.5) < 0.3
    # the JSON on disk is what was returned, and a second run merges into it
    with open(os.path.join(out, "bb.json")) as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    again = sample_attack.main(["--syn_cache", d + "ref", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "-d", "cpu", "--save",
                                "--outputs_dir", out, "--name", "bb"] + POOL)
    assert "cal" not in again["ref"] and again["ref"]["percentiles"] == [50.0, 10.0, 1.0, 0.1] and len(again["ref"]["eps2"]) == 4
    with open(os.path.join(out, "bb.json")) as f:
        merged = json.load(f)
    assert set(merged) == {"syn", "syn2", "ref"} and merged["syn"] == json.loads(json.dumps(m))


def test_cli_refusals(caches):
    from csl_gan_amd import sample_attack
    d, _ = caches
    base = ["--train_cache", d + "train", "--nontrain_cache", d + "heldout", "-d", "cpu"]
    with pytest.raises(SystemExit, match="one geometry"):
        sample_attack.main(["--syn_cache", d + "odd"] + base + POOL)
    with pytest.raises(SystemExit, match="one geometry"):
        sample_attack.main(["--syn_cache", d + "syn", "--calib_cache", d + "odd"] + base + POOL)
    with pytest.raises(SystemExit, match="percentiles"):
        sample_attack.main(["--syn_cache", d + "syn", "--percentiles", "50", "20", "10", "5", "1"] + base + POOL)
    with pytest.raises(SystemExit, match="pool"):
        sample_attack.main(["--syn_cache", d + "syn", "--train_cache", d + "train", "--nontrain_cache", d + "few", "-d", "cpu"] + POOL)
    with pytest.raises(SystemExit, match="pool"):
        sample_attack.main(["--syn_cache", d + "syn"] + base)                   # the default pool of 1000 against 40 + 45 records


# ---- host-side argument checks of the entry ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from csl_gan_amd import build, _lib
    build.build()
    return _lib.lib()


def test_nn_count_is_exported_and_refuses_bad_arguments_before_any_launch(L):
    import ctypes as C
    from csl_gan_amd import _lib
    assert "cslgan_nn_count_i8" in _lib.EXPORTS and _lib.ABI_VERSION == L.cslgan_version()
    err = lambda: L.cslgan_last_error()
    thr = (C.c_uint32 * 4)(1, 2, 3, 4)
    ok = dict(q=64, qn=64, nq=4, r=64, rn=64, nr=9, Dp=128, thr=thr, n_thr=2, counts=64)
    call = lambda **kw: L.cslgan_nn_count_i8(*[dict(ok, **kw)[k] for k in ("q", "qn", "nq", "r", "rn", "nr", "Dp", "thr", "n_thr", "counts")], None)
    for k in ("q", "qn", "r", "rn", "thr", "counts"):
        assert call(**{k: None}) == -1 and b"null" in err()
    assert call(n_thr=0) == -1 and b"n_thr=0" in err()
    assert call(n_thr=5) == -1 and b"n_thr=5" in err()
    assert call(Dp=0) == -1 and b"Dp=0" in err()
    assert call(Dp=96) == -1 and b"Dp=96" in err()
    assert call(Dp=65600) == -1 and b"Dp=65600" in err()
    assert call(nq=0) == -1 and b"nq=0" in err()
    assert call(nr=0) == -1 and b"nr=0" in err()
    assert call(nq=2 ** 31) == -1 and b"nq=2147483648" in err()
    assert call(nr=2 ** 31) == -1 and b"nr=2147483648" in err()
    assert call(q=72) == -1 and b"misaligned" in err()
    assert call(r=8) == -1 and b"misaligned" in err()
    assert call(qn=66) == -1 and b"misaligned" in err()
    assert call(rn=65) == -1 and b"misaligned" in err()
    assert call(counts=66) == -1 and b"misaligned" in err()
    assert call(nr=2 ** 31 - 1) == -1 and b"column ranges" in err()              # more tiles than 65535 ranges of 127 hold


def test_ops_nn_count_refuses_cpu_tensors_and_wrong_types():
    from csl_gan_amd import ops
    z8, z32 = torch.zeros(4, 64, dtype=torch.int8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.nn_count(z8, z32, z8, z32, [1], torch.zeros(4, 1, dtype=torch.int32))
    # a wrong type is refused before the device is looked at, so it shows here too
    c32 = torch.zeros(4, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="q must be a contiguous int8"):
        ops.nn_count(z8.to(torch.uint8), z32, z8, z32, [1], c32)
    with pytest.raises(RuntimeError, match="rn must be a contiguous int32"):
        ops.nn_count(z8, z32, z8, z32.to(torch.int64), [1], c32)
    with pytest.raises(RuntimeError, match="counts must be a contiguous int32"):
        ops.nn_count(z8, z32, z8, z32, [1], c32.to(torch.int64))
