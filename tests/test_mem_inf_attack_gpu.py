"""The device path of csl_gan_amd.audit (-m gpu): cslgan_attack_trials against the host model by integer equality,
cslgan_rank_counts against numpy, cslgan_softmax_max_rows_f32 against float64, CriticScorer (recorded graph + eager tail) against
eager batches and against the torch-CPU critic, attack_metrics on device tensors against the host model and the reference
estimator's recorded runs, and the command line on cuda:0."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRIALS = 64
SEED = 11


def _ops():
    from csl_gan_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the trial kernel -------------------------------------------------------------------------------------------------------------------

SHAPES = [(7, 5, 3, 4), (7, 5, 7, 0), (1024, 1025, 100, 900), (5000, 4100, 500, 3596)]        # the last one fills the pool of 4096


@functools.lru_cache(maxsize=None)
def _scores(N, M, kind):
    rng = np.random.default_rng(N + 3 * M)
    vt, vn = (rng.standard_normal(N) + 0.5).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    if kind == "levels":                                          # five levels: the tie rule decides many ranks
        vt, vn = np.clip(np.rint(vt), -2, 2).astype(np.float32), np.clip(np.rint(vn), -2, 2).astype(np.float32)
        if N > 7:
            vt[::5], vn[::7] = -0.0, 0.0                          # -0 ties with +0
    elif kind == "equal":
        vt, vn = np.full(N, 0.25, np.float32), np.full(M, 0.25, np.float32)
    return vt, vn


@functools.lru_cache(maxsize=None)
def _subsets(N, M, n, m, first):
    """The subsets of trials first .. first + 63: computed once per shape, shared by the three score sets."""
    from csl_gan_amd import audit
    return audit.trial_subsets(SEED, first, TRIALS, N, M, n, m)


@pytest.mark.parametrize("N,M,n,m", SHAPES)
def test_attack_trials_equal_the_host_model(N, M, n, m):
    from csl_gan_amd import audit
    ops = _ops()
    seen = set()
    for kind in ("smooth", "levels", "equal"):
        vt, vn = _scores(N, M, kind)
        exp = audit.hits_of_subsets(vt, vn, *_subsets(N, M, n, m, 0))
        got = ops.attack_trials(_dev(vt), _dev(vn), n, m, SEED, 0, TRIALS).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, exp), (kind, got[:8], exp[:8])
        if kind == "equal" or m == 0:
            assert np.array_equal(got, np.full(TRIALS, n))
        seen.update(got.tolist())
        # cut into launches, the same trials
        parts = [ops.attack_trials(_dev(vt), _dev(vn), n, m, SEED, lo, hi - lo) for lo, hi in ((0, 1), (1, 30), (30, 64))]
        assert np.array_equal(torch.cat(parts).cpu().numpy(), exp)
    if m and n < N:
        assert len(seen) > 2                                      # trials differ


def test_attack_trials_with_a_64_bit_first_trial_and_other_seeds():
    from csl_gan_amd import audit
    ops = _ops()
    N, M, n, m = 1024, 1025, 100, 900
    vt, vn = _scores(N, M, "smooth")
    base = audit.hits_of_subsets(vt, vn, *_subsets(N, M, n, m, 0))
    for first in (2 ** 32 - 30, 2 ** 40 + 7):                    # 2^32 - 30: the 64 trials carry into the high trial word
        exp = audit.hits_of_subsets(vt, vn, *_subsets(N, M, n, m, first))
        got = ops.attack_trials(_dev(vt), _dev(vn), n, m, SEED, first, TRIALS).cpu().numpy()
        assert np.array_equal(got, exp) and not np.array_equal(got, base)
    wrap = ops.attack_trials(_dev(vt), _dev(vn), n, m, SEED, 2 ** 64 - 4, 8).cpu().numpy()          # trial numbers wrap mod 2^64
    assert np.array_equal(wrap[4:], base[:4])
    other = ops.attack_trials(_dev(vt), _dev(vn), n, m, SEED + 1, 0, TRIALS).cpu().numpy()
    assert not np.array_equal(other, base)
    assert np.array_equal(other[:16], audit.trial_hits(vt, vn, n, m, SEED + 1, 0, 16))
    with pytest.raises(RuntimeError, match="n \\+ m"):
        ops.attack_trials(_dev(np.zeros(5000, np.float32)), _dev(np.zeros(5000, np.float32)), 500, 3597, SEED, 0, 4)
    with pytest.raises(RuntimeError, match="n=1025"):
        ops.attack_trials(_dev(vt), _dev(vn), 1025, 0, SEED, 0, 4)


# ---- rank counts ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("na,nb", [(1, 1), (257, 2049), (300, 7)])
def test_rank_counts_equal_numpy(na, nb):
    from csl_gan_amd import audit
    ops = _ops()
    rng = np.random.default_rng(na + nb)
    a, b = np.rint(rng.standard_normal(na) * 3).astype(np.float32), np.rint(rng.standard_normal(nb) * 3).astype(np.float32)
    a[::3] += np.float32(0.5) * (rng.random(len(a[::3])) < 0.5)
    a[0], b[0] = -0.0, 0.0
    if nb > 1:
        b[1] = -0.0
    gt, eq = ops.rank_counts(_dev(a), _dev(b))
    g2, e2 = (a[:, None] > b[None, :]).sum(1), (a[:, None] == b[None, :]).sum(1)
    assert np.array_equal(gt.cpu().numpy(), g2) and np.array_equal(eq.cpu().numpy(), e2)
    assert e2[0] >= 1 and g2[0] == (b < 0).sum()
    h1, h2 = audit.rank_counts_host(a, b)
    assert np.array_equal(h1, g2) and np.array_equal(h2, e2)


# ---- softmax max ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [2, 10, 64])
def test_softmax_max_rows_against_float64(C):
    """2e-6: at most 8 fp32 ulps of a value in [1/C, 1] — a sum of at most 64 exponentials and one reciprocal, with margin."""
    ops = _ops()
    rng = np.random.default_rng(C)
    for B in (1, 3, 257):
        l = (rng.standard_normal((B, C)) * rng.choice([0.1, 3.0, 40.0], size=(B, 1))).astype(np.float32)
        l = np.clip(l, -80, 80)
        l[0, 0], l[0, -1] = 80.0, -80.0
        if B > 2:
            l[1, :] = 80.0                                        # all equal: 1 / C
            l[2, :] = -80.0
            l[2, C // 2] = 80.0                                   # one class takes it all: 1
        exp = 1.0 / np.exp(l.astype(np.float64) - l.astype(np.float64).max(1, keepdims=True)).sum(1)
        got = ops.softmax_max_rows(_dev(l)).cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - exp).max())
        ref = torch.softmax(torch.from_numpy(l).double(), 1).max(1)[0].numpy()
        assert float(np.abs(ref - exp).max()) < 1e-12
        print("\nsoftmax_max_rows B=%d C=%d: max error %.3e" % (B, C, err))
        assert got.dtype == np.float32 and err <= 2e-6, err
        assert got.min() >= 1.0 / C - 2e-6 and got.max() <= 1.0 + 2e-6


# ---- the scorer -------------------------------------------------------------------------------------------------------------------------

CONFIGS = {
    "celeba_gn": ["CelebA", "-dpm", "gc", "-gcm", "adaptive-pl", "-nms", "4"],
    "mnist_vanilla_cond": ["MNIST", "-cond"],
}
N_IMG, BS = 19, 8


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(opt, D on the device, D on the CPU with the same weights, a cache of 19 images)."""
    import tempfile
    from csl_gan_amd import init_util, options
    from csl_gan_amd.pipeline import CachedImages
    out = tempfile.mkdtemp(prefix="audit_%s_" % name) + "/"
    opt = options.parse(CONFIGS[name] + ["-o", out, "--manual_seed", "9", "--synthetic", "-gd", "cpu", "-dd", "cpu"])
    _, Dc = init_util.init_models(opt, init_G=False)
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for p in Dc.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.02)
    Dc.eval()
    opt.d_device = "cuda:0"
    _, Dd = init_util.init_models(opt, init_G=False)
    Dd.load_state_dict(Dc.state_dict())
    opt.d_device = "cpu"
    rng = np.random.default_rng(4)
    shape = (N_IMG, 64, 64, 3) if opt.dataset == "CelebA" else (N_IMG, 28, 28, 1)
    # smooth images with structure (blurred noise): a critic's input, not white noise at full contrast
    base = rng.random(shape[:1] + (shape[1] // 4, shape[2] // 4) + shape[3:])
    x = (np.kron(base, np.ones((1, 4, 4, 1))) * 200 + rng.random(shape) * 55).astype(np.uint8)
    cache = CachedImages.from_arrays(x, np.arange(N_IMG) % 10, signed=opt.dataset == "CelebA")
    return opt, Dd, Dc, cache


def _score(D, opt, device, cache, graph, bs=BS, compute_dtype=None):
    from csl_gan_amd import audit
    sc = audit.CriticScorer(D, opt, device, bs, hip_graph=graph, compute_dtype=compute_dtype)
    try:
        v = sc.score(cache)
        graphed = sc.graph is not None
    finally:
        sc.release()
    assert graphed == (bool(graph) and device != "cpu" and len(cache) >= bs)
    assert sc.graph is None
    return v


def test_critic_scorer_on_the_celeba_critic():
    opt, Dd, Dc, cache = _setup("celeba_gn")
    ops = _ops()
    before = ops.get_compute_dtype()
    v_graph = _score(Dd, opt, "cuda:0", cache, True)              # two replays + a ragged 3
    v_eager = _score(Dd, opt, "cuda:0", cache, False)             # the same batches through eager D
    v_cpu = _score(Dc, opt, "cpu", cache, False)
    scale = float(np.abs(v_cpu).max())
    assert v_graph.shape == (N_IMG,) and v_graph.dtype == np.float32 and np.isfinite(v_graph).all()
    e_graph, e_cpu = float(np.abs(v_graph - v_eager).max()) / scale, float(np.abs(v_graph - v_cpu).max()) / scale
    print("\nCriticScorer celeba: graph vs eager %.3e, device vs torch-CPU %.3e of max |score| %.4f" % (e_graph, e_cpu, scale))
    assert e_graph <= 1e-5 and e_cpu <= 1e-3
    assert float(v_cpu.max() - v_cpu.min()) > 1e-3 * scale       # a critic that tells the images apart
    assert float(np.abs(v_graph[:8] - v_graph[8:16]).max()) > 0  # a replay scores new rows
    # the scores are the critic's first output of the rows, in index order
    with torch.no_grad():
        direct = Dc(cache.to_float(cache.x[8:19]))[0].reshape(-1).numpy()
    assert float(np.abs(direct - v_cpu[8:19]).max()) <= 1e-5 * scale
    assert ops.get_compute_dtype() == before
    # release() restores the process compute dtype whatever the scorer ran in
    v_auto = _score(Dd, opt, "cuda:0", cache, True, compute_dtype="fp32_auto")
    assert ops.get_compute_dtype() == before and float(np.abs(v_auto - v_cpu).max()) / scale <= 1e-3


def test_critic_scorer_takes_the_aux_head_on_mnist():
    opt, Dd, Dc, cache = _setup("mnist_vanilla_cond")
    v_graph, v_eager, v_cpu = _score(Dd, opt, "cuda:0", cache, True), _score(Dd, opt, "cuda:0", cache, False), _score(Dc, opt, "cpu", cache, False)
    with torch.no_grad():
        _, aux = Dc(cache.to_float(cache.x[:]), torch.from_numpy(cache.labels))
    exp = torch.softmax(aux, 1).max(1)[0].numpy()
    assert float(np.abs(v_cpu - exp).max()) <= 1e-6 and 0.1 <= v_cpu.min() and v_cpu.max() <= 1.0
    print("\nCriticScorer mnist aux: graph vs eager %.3e, device vs torch-CPU %.3e" % (np.abs(v_graph - v_eager).max(), np.abs(v_graph - v_cpu).max()))
    assert float(np.abs(v_graph - v_eager).max()) <= 1e-5 and float(np.abs(v_graph - v_cpu).max()) <= 1e-3


# ---- the figures ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["attack_smooth", "attack_ties"])
def test_attack_metrics_on_the_device_equal_the_host_model_and_agree_with_the_reference(name):
    from csl_gan_amd import audit
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    vt, vn, rates = d["vt"], d["vn"], d["rates"]
    dev = audit.attack_metrics(_dev(vt), _dev(vn), 0.1, 1000, 96, 20240611, "cuda:0")
    host = audit.attack_metrics(vt, vn, 0.1, 1000, 96, 20240611, "cpu")
    assert dev == host, (dev, host)
    assert dev == audit.attack_metrics(vt, vn, 0.1, 1000, 96, 20240611, "cuda:0")                  # host arrays, device work
    # 2000 trials on the device against the reference estimator's 2000: two independent Monte-Carlo means
    hits = _ops().attack_trials(_dev(vt), _dev(vn), 100, 900, 20240611, 0, len(rates)).cpu().numpy()
    assert np.array_equal(hits[:96], audit.trial_hits(vt, vn, 100, 900, 20240611, 0, 96))
    model = hits / 100.0
    gap = abs(float(rates.mean()) - float(model.mean()))
    bound = 5.0 * np.sqrt((rates.std(ddof=1) ** 2 + model.std(ddof=1) ** 2) / len(model))
    print("\n%s: reference ASR %.5f, device %.5f, gap %.5f, bound %.5f" % (name, rates.mean(), model.mean(), gap, bound))
    assert gap <= bound
    full = audit.attack_metrics(_dev(vt), _dev(vn), 0.1, 1000, len(rates), 20240611, "cuda:0")
    assert full["asr"] == float(hits.mean() / 100) and abs(full["asr_stderr"] - model.std(ddof=1) / np.sqrt(len(rates))) < 1e-12
    with pytest.raises(ValueError, match="non-finite"):
        audit.attack_metrics(_dev(np.where(np.arange(600) == 5, np.nan, vt).astype(np.float32)), _dev(vn), 0.1, 1000, 8, 1, "cuda:0")


# ---- the command line -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mnist_vanilla_cond", "celeba_gn"])
def test_cli_on_the_device(name, tmp_path):
    from csl_gan_amd import mem_inf_attack, util
    from csl_gan_amd.generate import CacheWriter
    opt, Dd, Dc, cache = _setup(name)
    out = str(tmp_path) + "/run_%s/" % name
    os.makedirs(out + "saves")
    with open(out + "opt.txt", "w") as f:
        json.dump(dict(opt.__dict__, output_dir=out), f)
    state = {k: v.clone() for k, v in Dc.state_dict().items()}
    try:
        util.save_model(2, Dc, torch.optim.Adam(Dc.parameters()), 0, out + "saves/D-2")
        with torch.no_grad():
            g = torch.Generator().manual_seed(2)
            for p in Dc.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.02)
        util.save_model(3, Dc, torch.optim.Adam(Dc.parameters()), 0, out + "saves/D-3")
    finally:
        Dc.load_state_dict(state)
    for which, rows in (("train", slice(0, 11)), ("nontrain", slice(6, 19))):
        w = CacheWriter(out + which, len(cache.x[rows]), cache.H, cache.W, cache.C, cache.signed, {"note": "test rows"})
        w(0, cache.x[rows], cache.labels[rows])
        w.close()
    args = [out, "--train_cache", out + "train", "--nontrain_cache", out + "nontrain", "-d", "cuda:0", "-bs", str(BS), "--pool", "12",
            "--data_prop", "0.25", "--asr_iters", "64", "--checkpoints", "2", "3", "--values_dir", str(tmp_path / "values"),
            "--outputs_dir", str(tmp_path / "outputs")]
    stats = mem_inf_attack.main(args + ["--save"])
    assert sorted(stats) == ["2", "3"] and json.load(open(tmp_path / "outputs" / ("run_%s.json" % name))) == stats
    for e in ("2", "3"):
        for k in ("asr", "asr_stderr", "auc", "tpr_at_fpr_0.01", "tpr_at_fpr_0.001"):
            assert np.isfinite(stats[e][k]), (e, k)
        assert stats[e]["n"] == 3 and stats[e]["m"] == 9
    assert _ops().get_compute_dtype() == "fp32" and torch.is_grad_enabled()
    # the saved values are the device scores of the rows (recorded graph for the full batch, eager for the tail)
    v2 = np.load(tmp_path / "values" / ("run_%s" % name) / "checkpoint-2" / "attack_values_train.npy")
    exp = _score(Dc, opt, "cpu", cache, False)[:11]
    assert v2.shape == (11,) and float(np.abs(v2 - exp).max()) <= 1e-3 * float(np.abs(exp).max())
    v3 = np.load(tmp_path / "values" / ("run_%s" % name) / "checkpoint-3" / "attack_values_train.npy")
    assert float(np.abs(v3 - v2).max()) > 1e-3 * float(np.abs(exp).max())          # the second checkpoint was scored with its own weights
    # a rerun is identical: from the saved values (no --save: the figures are recomputed on the device) ...
    os.remove(tmp_path / "outputs" / ("run_%s.json" % name))
    assert mem_inf_attack.main(args) == stats
    # ... and from scratch the scores come back within the graph-vs-eager bound, the figures complete
    fresh = mem_inf_attack.main(args[:-4] + ["--values_dir", str(tmp_path / "values2"), "--outputs_dir", str(tmp_path / "outputs2")])
    w2 = np.load(tmp_path / "values2" / ("run_%s" % name) / "checkpoint-2" / "attack_values_train.npy")
    assert float(np.abs(w2 - v2).max()) <= 1e-5 * float(np.abs(v2).max()) and sorted(fresh) == ["2", "3"]
