"""csl_gan_amd.audit / csl_gan_amd.mem_inf_attack on the CPU: the package's Philox against the oracle's, the swap-or-not sampler
(distinct indices, uniform subsets), trial invariance of the host model, the host model against the reference estimator's recorded
runs (tests/golden/attack_*.npz, made by tests/golden/make_attack_golden.py), AUC / TPR against a double loop, the host-side
argument checks of the three C-ABI entries (no launch, no device) and the command line end to end with -d cpu."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from oracle import noise_streams as NS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_SEED = 20240611               # seed of the host model's trials on both fixtures (the subsets are then shared by the two)
TRIALS = 2000


def test_the_packages_philox_equals_the_oracles():
    from csl_gan_amd import audit
    rng = np.random.default_rng(5)
    c = [rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64) for _ in range(4)]
    c[0][:4] = [0, 0xFFFFFFFF, 1, 0xFFFFFFFF]
    c[3][:4] = [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    for k0, k1 in [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0xA4093822, 0x299F31D0), (123, 2 ** 31)]:
        ours, ref = audit.philox4x32_10(*c, k0, k1), NS.philox4x32_10(*c, k0, k1)
        for a, b in zip(ours, ref):
            assert np.array_equal(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
    assert audit.audit_key(0) == 0x6D656D696E666174 and audit.audit_key(2 ** 64 - 1) == 0x6D656D696E666174 ^ (2 ** 64 - 1)
    assert [audit.shuffle_rounds(N) for N in (1, 2, 3, 7, 1024, 1025, 2 ** 31 - 1)] == [8, 8, 16, 24, 80, 88, 248]


@pytest.mark.parametrize("N", [1, 2, 7, 1024, 1025])
def test_subset_indices_are_distinct_and_in_range(N):
    from csl_gan_amd import audit
    trials = [0, 1, 2 ** 32 - 1, 2 ** 40 + 7]
    for side in (0, 1):
        for k in (1, N):
            x = audit.subset_indices(9, trials, side, N, k)
            assert x.shape == (len(trials), k) and x.dtype == np.int64
            for row in x:
                assert len(set(row.tolist())) == k and row.min() >= 0 and row.max() < N
            assert np.array_equal(audit.subset_indices(9, trials[3], side, N, k), x[3])          # a scalar trial is the row
    if N >= 1024:                                                                                # sides, trials and seeds differ
        a = audit.subset_indices(9, [0, 1], 0, N, N)
        assert not np.array_equal(a[0], a[1])
        assert not np.array_equal(a[0], audit.subset_indices(9, 0, 1, N, N))
        assert not np.array_equal(a[0], audit.subset_indices(10, 0, 0, N, N))


def test_subsets_are_uniform_over_the_35_triples_of_7():
    from csl_gan_amd import audit
    T = 40000
    x = np.sort(audit.subset_indices(1, list(range(T)), 0, 7, 3), axis=1)
    index = {c: i for i, c in enumerate(itertools.combinations(range(7), 3))}
    cnt = np.bincount([index[tuple(r)] for r in x.tolist()], minlength=35)
    chi = float(((cnt - T / 35.0) ** 2 / (T / 35.0)).sum())
    df = 34
    print("\nchi-square over the 35 subsets: %.1f at %d degrees of freedom" % (chi, df))
    assert chi < df + 6 * np.sqrt(2 * df), chi
    first = np.bincount(audit.subset_indices(1, list(range(T)), 0, 7, 1)[:, 0], minlength=7)      # pi(0) alone is uniform too
    assert float(((first - T / 7.0) ** 2 / (T / 7.0)).sum()) < 6 + 6 * np.sqrt(12)


def test_trials_do_not_depend_on_how_they_are_cut():
    from csl_gan_amd import audit
    rng = np.random.default_rng(3)
    vt, vn = rng.standard_normal(50).astype(np.float32) + 0.5, rng.standard_normal(70).astype(np.float32)
    whole = audit.trial_hits(vt, vn, 10, 40, 7, 0, 64)
    assert np.array_equal(whole, np.concatenate([audit.trial_hits(vt, vn, 10, 40, 7, 0, 32), audit.trial_hits(vt, vn, 10, 40, 7, 32, 32)]))
    assert whole.min() >= 0 and whole.max() <= 10 and len(set(whole.tolist())) > 2
    big = 2 ** 32 + 2 ** 40 - 5                                  # the chunk carries across 2^32 in the low trial word's neighbour
    far = audit.trial_hits(vt, vn, 10, 40, 7, big, 16)
    assert np.array_equal(far[8:], audit.trial_hits(vt, vn, 10, 40, 7, big + 8, 8)) and not np.array_equal(far, whole[:16])
    wrap = audit.trial_hits(vt, vn, 10, 40, 7, 2 ** 64 - 4, 8)   # trial numbers wrap mod 2^64
    assert np.array_equal(wrap[4:], whole[:4])
    assert not np.array_equal(audit.trial_hits(vt, vn, 10, 40, 8, 0, 64), whole)
    assert np.array_equal(audit.trial_hits(np.ones(50, np.float32), np.ones(70, np.float32), 10, 40, 7, 0, 16), np.full(16, 10))
    assert np.array_equal(audit.trial_hits(vt, vn, 10, 0, 7, 0, 16), np.full(16, 10))
    assert np.array_equal(audit.trial_hits(vt, np.zeros(0, np.float32), 50, 0, 7, 0, 4), np.full(4, 50))
    for n, m in [(0, 40), (51, 40), (10, 71)]:
        with pytest.raises(ValueError):
            audit.trial_hits(vt, vn, n, m, 7, 0, 2)
    with pytest.raises(ValueError):
        audit.trial_hits(np.ones(5000, np.float32), np.ones(5000, np.float32), 4000, 97, 7, 0, 2)           # n + m = 4097


def test_the_rank_rule_on_a_pool_written_out():
    """hits_of_subsets against the definition, element by element, on a pool with ties across and inside the two sides."""
    from csl_gan_amd import audit
    vt, vn = np.array([1.0, 2.0, 2.0, -0.0, 3.0], np.float32), np.array([2.0, 0.0, 3.0, 1.0], np.float32)
    it, im = np.array([[3, 1, 0], [4, 2, 1]]), np.array([[0, 1, 2, 3], [2, 0, 3, 1]])
    for ties_to_train in (True, False):
        exp = []
        for rt, rn in zip(it, im):
            pool = [(float(vt[i]), 1) for i in rt] + [(float(vn[j]), 0) for j in rn]
            if not ties_to_train:
                pool = pool[len(rt):] + pool[:len(rt)]
            best = sorted(pool, key=lambda p: p[0], reverse=True)[:len(rt)]
            exp.append(sum(p[1] for p in best))
        assert audit.hits_of_subsets(vt, vn, it, im, _ties_to_train=ties_to_train).tolist() == exp
    assert audit.hits_of_subsets(vt, vn, it, im).tolist() == [1, 2] and audit.hits_of_subsets(vt, vn, it, im, _ties_to_train=False).tolist() == [1, 1]


# ---- against the reference estimator's recorded runs ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixtures():
    from csl_gan_amd import audit
    f = {name: dict(np.load(os.path.join(GOLDEN, name + ".npz"))) for name in ("attack_smooth", "attack_ties")}
    for d in f.values():
        assert d["vt"].shape == (600,) and d["vn"].shape == (1500,) and d["rates"].shape == (TRIALS,) and d["vt"].dtype == np.float32
    assert set(np.unique(f["attack_ties"]["vn"]).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    subsets = audit.trial_subsets(MODEL_SEED, 0, TRIALS, 600, 1500, 100, 900)          # shared: the subsets do not depend on the scores
    return f, subsets


def _agree(ref_rates, hits, n=100):
    """|mean_ref - mean_model| against 5 sqrt((s_ref^2 + s_model^2) / trials): the sampling error of two independent means."""
    model = hits / float(n)
    gap = abs(float(ref_rates.mean()) - float(model.mean()))
    bound = 5.0 * np.sqrt((ref_rates.std(ddof=1) ** 2 + model.std(ddof=1) ** 2) / len(model))
    return gap, bound, float(model.mean())


@pytest.mark.parametrize("name", ["attack_smooth", "attack_ties"])
def test_host_model_asr_agrees_with_the_reference_estimator(fixtures, name):
    from csl_gan_amd import audit
    f, (it, im) = fixtures
    d = f[name]
    hits = audit.hits_of_subsets(d["vt"], d["vn"], it, im)
    assert np.array_equal(hits[:64], audit.trial_hits(d["vt"], d["vn"], 100, 900, MODEL_SEED, 0, 64))      # the pieces are trial_hits
    gap, bound, mean = _agree(d["rates"], hits)
    print("\n%s: reference ASR %.5f, host model %.5f, gap %.5f, bound %.5f" % (name, d["rates"].mean(), mean, gap, bound))
    assert gap <= bound, (gap, bound)
    if name == "attack_ties":                                       # the other tie rule is told apart by this fixture
        flipped = audit.hits_of_subsets(d["vt"], d["vn"], it, im, _ties_to_train=False)
        fgap, fbound, fmean = _agree(d["rates"], flipped)
        print("ties to the non-train sample: %.5f, gap %.5f, bound %.5f" % (fmean, fgap, fbound))
        assert fgap > fbound, (fgap, fbound)


# ---- AUC / TPR ------------------------------------------------------------------------------------------------------------------------

def test_auc_and_tpr_equal_a_double_loop():
    from csl_gan_amd import audit
    rng = np.random.default_rng(8)
    a = np.round(rng.standard_normal(37) * 2 + 0.7).astype(np.float32)          # integers: many ties
    b = np.round(rng.standard_normal(53) * 2).astype(np.float32)
    a[0], b[0], b[1] = -0.0, 0.0, -0.0
    gt, eq = audit.rank_counts_host(a, b)
    g2 = [sum(1 for y in b if x > y) for x in a]
    e2 = [sum(1 for y in b if x == y) for x in a]
    assert gt.tolist() == g2 and eq.tolist() == e2 and eq[0] >= 2
    m = audit.rank_metrics(gt, eq, len(b))
    auc = sum((1.0 if x > y else 0.5 if x == y else 0.0) for x in a for y in b) / (37 * 53)
    assert abs(m["auc"] - auc) < 1e-12
    for name, num, den in audit.FPR_BUDGETS + (("tpr_probe", 1, 4),):
        budget = (53 * num) // den                                   # non-train scores that may sit at or above the threshold
        tpr = sum(1 for x in a if sum(1 for y in b if y >= x) <= budget) / 37.0
        got = audit.rank_metrics(gt, eq, len(b))[name] if name != "tpr_probe" else float(((53 - gt) <= budget).sum()) / 37.0
        assert abs(got - tpr) < 1e-12
    assert 0.0 < float(((53 - gt) <= 53 // 4).sum()) / 37.0 < 1.0        # the probe budget separates something
    full = audit.attack_metrics(a, b, data_prop=0.25, pool=40, asr_iters=50, seed=4)
    assert full["n"] == 10 and full["m"] == 30 and abs(full["auc"] - auc) < 1e-12
    hits = audit.trial_hits(a, b, 10, 30, 4, 0, 50)
    assert full["asr"] == float(hits.mean() / 10) and abs(full["asr_stderr"] - hits.std(ddof=1) / (10 * np.sqrt(50))) < 1e-15
    bad = a.copy()
    bad[3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        audit.attack_metrics(bad, b, data_prop=0.25, pool=40, asr_iters=5)
    with pytest.raises(ValueError):
        audit.attack_metrics(a, b, data_prop=0.1, pool=1000, asr_iters=5)            # n = 100 > N = 37


# ---- host-side argument checks of the three entries ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from csl_gan_amd import build, _lib
    build.build()
    return _lib.lib()


def test_the_three_entries_are_exported_and_the_abi_stays_7(L):
    from csl_gan_amd import _lib
    assert _lib.ABI_VERSION == 7 and L.cslgan_version() == 7
    assert {"cslgan_attack_trials", "cslgan_rank_counts", "cslgan_softmax_max_rows_f32"} <= set(_lib.EXPORTS)


def test_attack_trials_refuses_bad_arguments_before_any_launch(L):
    err = lambda: L.cslgan_last_error()
    ok = dict(vt=16, N=600, vn=16, M=1500, n=100, m=900, seed=1, first=0, trials=4, hits=16)
    call = lambda **kw: L.cslgan_attack_trials(*[dict(ok, **kw)[k] for k in ("vt", "N", "vn", "M", "n", "m", "seed", "first", "trials", "hits")], None)
    assert call(vt=None) == -1 and b"null" in err()
    assert call(hits=None) == -1 and b"null" in err()
    assert call(vn=None) == -1 and b"null" in err()
    assert call(n=601) == -1 and b"n=601" in err()
    assert call(n=0) == -1 and b"n=0" in err()
    assert call(m=1501) == -1 and b"m=1501" in err()
    assert call(m=-1) == -1 and b"m=-1" in err()
    assert call(N=5000, M=5000, n=500, m=3597) == -1 and b"n + m = 4097" in err()
    assert call(N=2 ** 31) == -1 and b"N=2147483648" in err()
    assert call(M=2 ** 31) == -1 and b"M=2147483648" in err()
    assert call(N=0, n=0) == -1
    assert call(trials=-1) == -1 and b"trials=-1" in err()
    assert call(trials=0) == 0                                       # nothing to do: no launch


def test_rank_counts_and_softmax_max_rows_refuse_bad_arguments_before_any_launch(L):
    err = lambda: L.cslgan_last_error()
    assert L.cslgan_rank_counts(None, 4, 16, 4, 16, 16, None) == -1 and b"null" in err()
    assert L.cslgan_rank_counts(16, 4, None, 4, 16, 16, None) == -1 and b"null" in err()
    assert L.cslgan_rank_counts(16, 4, 16, 4, None, 16, None) == -1 and b"null" in err()
    assert L.cslgan_rank_counts(16, 4, 16, 4, 16, None, None) == -1 and b"null" in err()
    assert L.cslgan_rank_counts(16, -1, 16, 4, 16, 16, None) == -1 and b"na=-1" in err()
    assert L.cslgan_rank_counts(16, 4, 16, 2 ** 31, 16, 16, None) == -1 and b"nb=2147483648" in err()
    assert L.cslgan_rank_counts(16, 0, 16, 4, 16, 16, None) == 0
    assert L.cslgan_softmax_max_rows_f32(None, 4, 10, 16, None) == -1 and b"null" in err()
    assert L.cslgan_softmax_max_rows_f32(16, 4, 10, None, None) == -1 and b"null" in err()
    assert L.cslgan_softmax_max_rows_f32(16, 4, 65, 16, None) == -1 and b"n_classes=65" in err()
    assert L.cslgan_softmax_max_rows_f32(16, 4, 0, 16, None) == -1 and b"n_classes=0" in err()
    assert L.cslgan_softmax_max_rows_f32(16, -2, 10, 16, None) == -1 and b"B=-2" in err()
    assert L.cslgan_softmax_max_rows_f32(16, 0, 10, 16, None) == 0


def test_the_ops_refuse_cpu_tensors():
    from csl_gan_amd import ops
    v = torch.zeros(8)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.attack_trials(v, v, 2, 2, 0, 0, 4)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.rank_counts(v, v)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.softmax_max_rows(torch.zeros(4, 10))


# ---- the command line on the CPU ----------------------------------------------------------------------------------------------------

N_TRAIN, N_NONTRAIN = 23, 31


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """An MNIST Vanilla conditional critic (ACGAN head) with non-default weights, saved as train.py saves it next to its opt.txt,
    and two caches written as pipeline.build_cache writes them."""
    from csl_gan_amd import init_util, options, util
    from csl_gan_amd.generate import CacheWriter
    out = str(tmp_path_factory.mktemp("audit")) + "/mnist_run/"
    os.makedirs(out + "saves")
    opt = options.parse(["MNIST", "-cond", "-o", out, "--manual_seed", "77", "--synthetic"])
    with open(out + "opt.txt", "w") as f:
        json.dump(opt.__dict__, f)
    _, D = init_util.init_models(opt, init_G=False)
    g = torch.Generator().manual_seed(5)
    for e in (3, 4):
        with torch.no_grad():
            for p in D.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
        util.save_model(e, D, torch.optim.Adam(D.parameters()), 0, out + "saves/D-%d" % e)
    rng = np.random.default_rng(12)
    for name, n in (("train", N_TRAIN), ("nontrain", N_NONTRAIN)):
        w = CacheWriter(out + name, n, 28, 28, 1, False, {"note": "test rows"})
        w(0, rng.integers(0, 256, size=(n, 28, 28, 1), dtype=np.uint8), np.arange(n) % 10)
        w.close()
    return out, opt, D


def _cli(run_dir, tmp, extra=()):
    from csl_gan_amd import mem_inf_attack
    out = run_dir[0]
    return mem_inf_attack.main([out, "--train_cache", out + "train", "--nontrain_cache", out + "nontrain", "-d", "cpu", "-bs", "10",
                                "--pool", "20", "--data_prop", "0.25", "--asr_iters", "40", "--values_dir", str(tmp / "values"),
                                "--outputs_dir", str(tmp / "outputs")] + list(extra))


def test_cli_on_the_cpu_writes_values_and_figures_and_reuses_them(run_dir, tmp_path, capsys):
    from csl_gan_amd import audit
    from csl_gan_amd.pipeline import CachedImages
    out, opt, D = run_dir
    stats = _cli(run_dir, tmp_path, ["--checkpoints", "3", "4", "--save"])
    assert sorted(stats) == ["3", "4"]
    for e in ("3", "4"):
        for k in ("asr", "asr_stderr", "auc", "tpr_at_fpr_0.01", "tpr_at_fpr_0.001"):
            assert k in stats[e] and np.isfinite(stats[e][k]), (e, k)
        assert stats[e]["n"] == 5 and stats[e]["m"] == 15 and 0.0 <= stats[e]["asr"] <= 1.0 and 0.0 <= stats[e]["auc"] <= 1.0
    assert "subset seed: 77" in capsys.readouterr().out
    saved = json.load(open(tmp_path / "outputs" / "mnist_run.json"))
    assert saved == stats
    # the values are the attack values of the saved critic: the aux head's largest softmax probability, tail of 3 / 1 included
    from csl_gan_amd import util
    vt = np.load(tmp_path / "values" / "mnist_run" / "checkpoint-3" / "attack_values_train.npy")
    vn = np.load(tmp_path / "values" / "mnist_run" / "checkpoint-3" / "attack_values_nontrain.npy")
    assert vt.shape == (N_TRAIN,) and vn.shape == (N_NONTRAIN,) and vt.dtype == np.float32
    util.load_model(out + "saves/D-3", D, device="cpu")
    D.eval()
    c = CachedImages(out + "train")
    with torch.no_grad():
        _, aux = D(c.to_float(c.x[:]), torch.from_numpy(c.labels))
    exp = torch.softmax(aux, 1).max(1)[0].numpy()
    assert float(np.abs(vt - exp).max()) <= 1e-6 and 0.1 <= vt.min() and vt.max() <= 1.0
    assert stats["3"] == audit.attack_metrics(vt, vn, 0.25, 20, 40, 77, "cpu")
    assert stats["3"] != stats["4"]
    assert torch.is_grad_enabled()
    # a second run is identical: without --save it recomputes the figures from the saved values ...
    mt = os.path.getmtime(tmp_path / "values" / "mnist_run" / "checkpoint-3" / "attack_values_train.npy")
    os.remove(tmp_path / "outputs" / "mnist_run.json")
    again = _cli(run_dir, tmp_path, ["--checkpoints", "3", "4"])
    assert again == stats and "attack values loaded" in capsys.readouterr().out
    assert os.path.getmtime(tmp_path / "values" / "mnist_run" / "checkpoint-3" / "attack_values_train.npy") == mt
    assert not os.path.exists(tmp_path / "outputs" / "mnist_run.json")
    # ... and with the JSON in place, checkpoints already there are skipped (mem_inf_attack.py:300-309)
    with open(tmp_path / "outputs" / "mnist_run.json", "w") as f:
        json.dump({"3": {"asr": -1.0}}, f)
    merged = _cli(run_dir, tmp_path, ["--checkpoint_min", "3", "--checkpoint_max", "4", "--checkpoint_step", "1", "--save"])
    assert merged["3"] == {"asr": -1.0} and merged["4"] == stats["4"]
    assert json.load(open(tmp_path / "outputs" / "mnist_run.json")) == merged
    # another seed is another estimate of the same thing
    other = _cli(run_dir, tmp_path / "other", ["--checkpoints", "3", "--seed", "78"])
    assert other["3"]["auc"] == stats["3"]["auc"] and other["3"]["asr"] != stats["3"]["asr"]


def test_cli_refuses_a_missing_checkpoint(run_dir, tmp_path):
    with pytest.raises(SystemExit, match="D-9"):
        _cli(run_dir, tmp_path, ["--checkpoints", "9"])


def test_the_package_does_not_import_the_oracle():
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csl_gan_amd")
    for name in ("audit.py", "mem_inf_attack.py"):
        src = open(os.path.join(root, name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), name
