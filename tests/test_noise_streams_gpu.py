"""The device's random draws against the host Philox model (-m gpu): every normal the gradient-noise kernel adds and every
permutation index, label, jitter and pixel normal the mean sampler draws is compared, element by element over the whole output,
with oracle/noise_streams.py — for one launch, for chunked and mixed-type calls, with the call counter in HBM, through the whole
clip / sum / scale formula, through both privacy engines (steps, ranks, resume) and through MeanSampler.

Tolerance of a unit normal: the device evaluates Box-Muller in fp32 with fast log / sincos, the model in float64.  D is the distance
between the SAME formula in numpy float32 and in float64 over the draws of the bare-stream cases, computed on the host; the gate is
|z_dev - z_model| <= 4 D (a factor 4 for the fast intrinsics).  On these draws D = 3.0e-5 (gate 1.2e-4): fp32 rounds u1 to the
nearest 2^-24 above 1/2, which moves r = sqrt(-2 ln u1) by up to sqrt(2^-25 / 2k) at u1 = 1 - k 2^-25; the largest k = 1 event
(u1 -> 1.0, r = 0 instead of 2.44e-4) is not among them.  An unrelated N(0,1) value falls inside the gate with probability 1e-4.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import noise_streams as NS

pytestmark = pytest.mark.gpu

FULL_LENS = [4800, 64, 7, 1031, 3, 1, 1024, 1025, 4101, 3276800]      # tails of 1..3 columns, block multiples, block + 1, 3200 blocks
SHORT_LENS = FULL_LENS[:-1]
SEEDS = [0, 123, 2 ** 32 + 5, 2 ** 64 - 1]
OFFSETS = [0, 1, 2 ** 18 - 1, 2 ** 18, 2 ** 26 + 3]                   # 64 * 2^18 = 2^24 carries into c3; 2^26: c2 has wrapped
BARE_CASES = [(FULL_LENS, s, 0) for s in SEEDS] + [(SHORT_LENS, 123, o) for o in OFFSETS]


def _ops():
    from csl_gan_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _model(lens, seed, offset):
    return NS.clip_call_normals(list(lens), seed, offset)


@functools.lru_cache(maxsize=None)
def _D():
    """max |z_fp32 - z_fp64| of the Box-Muller formula over every draw of the bare-stream cases: host arithmetic only."""
    d = 0.0
    for lens, seed, offset in BARE_CASES:
        z32 = NS.clip_call_normals(lens, seed, offset, dtype=np.float32)
        d = max(d, max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(z32, _model(tuple(lens), seed, offset))))
    assert 1e-5 < d < 2.5e-4, d          # no larger than the k = 1 rounding event of the docstring
    return d


def _gate():
    return 4.0 * _D()


def _np(t):
    return t.detach().double().cpu().numpy().reshape(-1)


def _device_stream(lens, seed, offset, call_counter=None, dtypes=None):
    """Zero inputs, noise_std 1, scale 1, beta 0: the outputs ARE the unit normals of the call."""
    ops = _ops()
    dts = [torch.float32] * len(lens) if dtypes is None else dtypes
    mats = [torch.zeros(1, L, device="cuda", dtype=dt) for L, dt in zip(lens, dts)]
    outs = [torch.full((L,), float("nan"), device="cuda") for L in lens]
    ops.clip_accum_noise(mats, outs, noise_std=torch.ones(len(lens), device="cuda"), seed=seed, offset=offset, call_counter=call_counter)
    torch.cuda.synchronize()
    return outs


def _assert_stream(got, exp, what, tol=None):
    tol = _gate() if tol is None else tol
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    err = np.abs(got - exp)
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, "%s: %d of %d elements off by more than %.3e (first at %d: got %.7f, model %.7f; max %.3e)" % (
        what, bad.size, got.size, tol, bad[0], got[bad[0]], exp[bad[0]], np.nanmax(err))
    return err


# ---- (a) the bare stream -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(BARE_CASES)), ids=["seed%d" % s for s in SEEDS] + ["offset%d" % o for o in OFFSETS])
def test_bare_stream_equals_model(case):
    lens, seed, offset = BARE_CASES[case]
    outs = _device_stream(lens, seed, offset)
    exp = _model(tuple(lens), seed, offset)
    errs = np.concatenate([np.abs(_np(o) - e) for o, e in zip(outs, exp)])
    # the record of profiles/noise_stream_report.txt (run with -s), printed before anything is asserted
    print("\nnoise-stream deviation: seed=%d offset=%d draws=%d  max=%.3e  p99.9=%.3e  D=%.3e  gate=%.3e"
          % (seed, offset, errs.size, np.nanmax(errs), np.nanpercentile(errs, 99.9), _D(), _gate()))
    for s, (o, e) in enumerate(zip(outs, exp)):
        _assert_stream(o, e, "segment %d (len %d) seed %d offset %d" % (s, lens[s], seed, offset))
    assert float(np.abs(np.concatenate(exp)).max()) <= np.sqrt(-2.0 * np.log(2.0 ** -25))


# ---- (b) chunked calls and element types ---------------------------------------------------------------------------------------

def _many_lens(n):
    return [1024 + 37 * i + (i % 4) for i in range(n)]


@pytest.mark.parametrize("n,mixed", [(17, False), (40, False), (20, True), (64, True)])
def test_chunks_and_element_types_get_their_own_streams(n, mixed):
    lens = _many_lens(n)
    dts = [torch.bfloat16 if (mixed and i % 2) else torch.float32 for i in range(n)]
    outs = _device_stream(lens, 99, 3, dtypes=dts)
    exp = NS.clip_call_normals(lens, 99, 3, dtypes=[str(d) for d in dts])
    got = [_np(o) for o in outs]
    for i in range(n):
        _assert_stream(got[i], exp[i], "tensor %d of %d" % (i, n))
    for i in range(n):
        for j in range(i + 1, n):
            m = min(lens[i], lens[j])
            assert float(np.mean(got[i][:m] == got[j][:m])) < 1e-3, "tensors %d and %d share a stream" % (i, j)


# ---- (c) the call counter in HBM -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 5, 2 ** 18])
def test_call_counter_in_hbm_is_the_offset(k):
    a = (k + 1) // 2
    ctr = lambda v: torch.full((1,), v, device="cuda", dtype=torch.int64)
    by_value = _device_stream(SHORT_LENS, 7, k)
    by_counter = _device_stream(SHORT_LENS, 7, 0, call_counter=ctr(k))
    split = _device_stream(SHORT_LENS, 7, a, call_counter=ctr(k - a))
    exp = NS.clip_call_normals(SHORT_LENS, 7, 0, call_counter=k)
    for s in range(len(SHORT_LENS)):
        assert torch.equal(by_value[s], by_counter[s]) and torch.equal(by_value[s], split[s]), "segment %d" % s
        _assert_stream(by_value[s], exp[s], "segment %d at call %d" % (s, k))
    other = _device_stream(SHORT_LENS, 7, 0, call_counter=ctr(k + 1))
    assert float(np.mean(_np(other[0]) == _np(by_value[0]))) < 1e-3


# ---- (d) the whole formula with device noise -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_clip_sum_scale_with_device_noise(dtype, shift):
    """out = 0.5 old + 0.125 (sum_r f_r m_r + sigma_s z_model); shift: the inputs start 1 or 3 elements into their storage, which
    takes the kernel's element-wise path."""
    ops = _ops()
    rows, lens = 8, [4800, 64, 1031, 3, 2050]
    g = torch.Generator().manual_seed(40 + shift)
    store = [(torch.randn(rows * L + shift, generator=g) * (1.0 + s)).to(dtype).cuda() for s, L in enumerate(lens)]
    mats = [st[shift:].view(rows, L) for st, L in zip(store, lens)]
    assert all(m.data_ptr() % 16 == (shift * m.element_size()) % 16 for m in mats)
    f = (torch.rand(len(lens), rows, generator=g) * 0.9 + 0.1).cuda()
    std = torch.tensor([0.5, 1.0, 2.0, 0.25, 4.0])
    old = [torch.randn(L, generator=g) for L in lens]
    outs = [o.clone().cuda() for o in old]
    ops.clip_accum_noise(mats, outs, factors=f, noise_std=std.cuda(), seed=2 ** 33 + 17, offset=6, scale=0.125, beta=0.5)
    torch.cuda.synchronize()
    z = NS.clip_call_normals(lens, 2 ** 33 + 17, 6)
    for s, L in enumerate(lens):
        m64, f64 = mats[s].double().cpu().numpy(), f[s].double().cpu().numpy()          # bf16 reference: the rounded inputs in float64
        ref = 0.5 * old[s].double().numpy() + 0.125 * ((f64[:, None] * m64).sum(0) + float(std[s]) * z[s])
        tol = float(std[s]) * 0.125 * _gate() + 1e-4 * float(np.abs(ref).max())
        _assert_stream(outs[s], ref, "segment %d (%s, shift %d)" % (s, dtype, shift), tol=tol)


def test_more_than_64_tensors_are_refused_on_the_device_too():
    ops = _ops()
    mats = [torch.zeros(1, 8, device="cuda") for _ in range(65)]
    outs = [torch.full((8,), 7.0, device="cuda") for _ in range(65)]
    with pytest.raises(RuntimeError, match="at most 64 tensors"):
        ops.clip_accum_noise(mats, outs, noise_std=torch.ones(65, device="cuda"), seed=1)
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)                 # nothing was launched
    ops.clip_accum_noise(mats, outs, noise_std=torch.ones(65, device="cuda"), noises=[torch.ones(8, device="cuda")] * 65)
    assert all(bool((o == 1.0).all()) for o in outs)                 # pre-drawn noise and plain sums keep taking any number
    ops.clip_accum_noise(mats, outs)
    assert all(bool((o == 0.0).all()) for o in outs)


# ---- (e) the engines -----------------------------------------------------------------------------------------------------------

B_ENGINE, SIGMA = 8, 0.5


def _engine(tmp_path, name, mode, rank=0):
    from csl_gan_amd import init_util, options
    from csl_gan_amd.trainer import Trainer
    extra = ["-gcm", "adaptive-pl", "--materialize", "all"] if mode == "gc" else ["-ispp", "True"]
    out = str(tmp_path / name)
    os.makedirs(out, exist_ok=True)
    opt = options.parse(["MNIST", "--model", "DeepConvResNet", "-dpm", mode, "-nms", "4", "-bs", str(B_ENGINE), "-gd", "cuda:0", "-dd", "cuda:0",
                         "-o", out, "--manual_seed", "1", "--g_latent_dim", "16", "--sigma", "0.8", "--penalty", "WGAN-GP"] + extra)
    G, D = init_util.init_models(opt)
    tr = Trainer(opt, G, D, log_to=os.path.join(out, "log.csv"), rank=rank)
    pe = tr.setup_privacy_engine()
    assert pe.seed == NS.engine_seed(1, rank) and pe.grad_reducer is None
    return tr, pe, list(D.parameters())


def _wrapped_step(tr, pe, ps, mode, R, scales):
    """One wrapped optimizer step on a zero gradient -> the unit normals it drew, one array per parameter in its memory order."""
    pe.world_size, pe.noise_multiplier = R, SIGMA
    if mode == "gc":
        pe.set_max_grad_norm(scales)
        for p in ps:
            p.summed_grad = torch.zeros_like(p, memory_format=torch.preserve_format)
        std = [SIGMA * c / R ** 0.5 for c in scales]                            # of the sum, which is then divided by B * R
        unit = [B_ENGINE * R / s for s in std]
    else:
        for p in ps:
            p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
        pe._sens_dev = torch.tensor(scales, device="cuda", dtype=torch.float32)
        std = [c * SIGMA / (B_ENGINE * R ** 0.5) for c in scales]               # of the mean gradient, which is then divided by R
        unit = [R / s for s in std]
    tr.d_optimizer.step()
    torch.cuda.synchronize()
    out = []
    for p, u in zip(ps, unit):
        g = p.grad
        out.append(_np(g.as_strided((g.numel(),), (1,), g.storage_offset())) * u)
    return out


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("mode", ["gc", "is"])
def test_engine_steps_draw_the_model_stream_once(tmp_path, mode, R):
    tr, pe, ps = _engine(tmp_path, "a", mode)
    lens = [p.numel() for p in ps]
    scales = [0.5 + 0.25 * i for i in range(len(ps))]             # clip norms (gc) / sensitivities (is): one per tensor, all different
    seen = []
    for k in range(3):
        z = _wrapped_step(tr, pe, ps, mode, R, scales)
        exp = NS.clip_call_normals(lens, NS.engine_seed(1, 0), 0, call_counter=k)
        for i in range(len(ps)):
            _assert_stream(z[i], exp[i], "%s R=%d step %d tensor %d" % (mode, R, k, i))
        seen.append(np.concatenate(z))
    assert pe.steps == 3 and pe.state_dict()["noise_calls"] == 3
    # a resume continues the stream: call 3, not call 0
    tr2, pe2, ps2 = _engine(tmp_path, "b", mode)
    pe2.load_state_dict(pe.state_dict())
    z = _wrapped_step(tr2, pe2, ps2, mode, R, scales)
    exp3 = NS.clip_call_normals(lens, NS.engine_seed(1, 0), 0, call_counter=3)
    for i in range(len(ps)):
        _assert_stream(z[i], exp3[i], "%s R=%d resumed step tensor %d" % (mode, R, i))
    resumed = np.concatenate(z)
    assert all(float(np.mean(resumed == s)) < 1e-3 for s in seen), "the resumed step replayed an earlier step's noise"
    assert pe2.state_dict()["noise_calls"] == 4
    # ... also when the engine's device counter already exists: restoring the saved state again gives call 3 again, bit for bit
    pe2.load_state_dict(pe.state_dict())
    again = np.concatenate(_wrapped_step(tr2, pe2, ps2, mode, R, scales))
    assert np.array_equal(again, resumed)
    # another rank: its own seed, nothing shared with rank 0
    tr1, pe1, ps1 = _engine(tmp_path, "c", mode, rank=1)
    z1 = _wrapped_step(tr1, pe1, ps1, mode, R, scales)
    exp1 = NS.clip_call_normals(lens, NS.engine_seed(1, 1), 0, call_counter=0)
    for i in range(len(ps)):
        _assert_stream(z1[i], exp1[i], "%s R=%d rank 1 tensor %d" % (mode, R, i))
    r1 = np.concatenate(z1)
    assert all(float(np.mean(r1 == s)) < 1e-3 for s in seen + [resumed]), "rank 1 shares noise with rank 0"


# ---- (f) the mean sampler ------------------------------------------------------------------------------------------------------

S1, S2 = 0.05, 0.02


def _ms_tol(table_vals):
    return (S1 + S2) * _gate() + 2.0 ** -23 * np.abs(table_vals)


@pytest.mark.parametrize("n", [128, 70])
@pytest.mark.parametrize("length", [768, 50])
def test_mean_sample_noise_equals_model(length, n):
    ops = _ops()
    g = torch.Generator().manual_seed(length + n)
    table = torch.randn(3, 32, length, generator=g)
    labels, perms = torch.randint(0, 3, (n,), generator=g), torch.randint(0, 32, (n,), generator=g)
    for seed, offset in ((11, 1), (2 ** 40 + 7, 2 ** 32 + 1)):
        out = ops.mean_sample(table.cuda(), labels.cuda(), perms.cuda(), S1, S2, seed=seed, offset=offset)
        torch.cuda.synchronize()
        m = NS.mean_sample_draws(n, 32, 3, length, seed, offset)
        base = table[labels, perms].double().numpy()
        res = out.double().cpu().numpy().reshape(n, length) - base
        err = np.abs(res - (S1 * m["jitter"][:, None] + S2 * m["pixel"]))
        bad = np.argwhere(~(err <= _ms_tol(base)))
        assert bad.size == 0, "seed %d offset %d: %d elements off, first %s, max %.3e" % (seed, offset, len(bad), bad[0], np.nanmax(err))
        # the two parts one at a time: the jitter is one value per image, the pixel noise has none of it
        jit = ops.mean_sample(table.cuda(), labels.cuda(), perms.cuda(), S1, 0.0, seed=seed, offset=offset).double().cpu().numpy().reshape(n, length)
        assert bool((np.abs(jit - base - S1 * m["jitter"][:, None]) <= _ms_tol(base)).all())
        pix = ops.mean_sample(table.cuda(), labels.cuda(), perms.cuda(), 0.0, S2, seed=seed, offset=offset).double().cpu().numpy().reshape(n, length)
        assert bool((np.abs(pix - base - S2 * m["pixel"]) <= _ms_tol(base)).all())


@pytest.mark.parametrize("offset", [1, 2, 2 ** 32 + 1])
@pytest.mark.parametrize("n", [128, 70])
def test_mean_sample_draws_its_permutations_and_labels_as_the_model(n, offset):
    """perms = labels = None: the in-LDS ranking and the label draw, also for a batch that is not a multiple of num_samples."""
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    table = torch.randn(3, 32, 768, generator=g)
    m = NS.mean_sample_draws(n, 32, 3, 768, 2 ** 40 + 7, offset)
    for rep in range((n + 31) // 32):
        blk = m["perms"][32 * rep:32 * rep + 32]
        assert len(set(blk.tolist())) == len(blk) and (len(blk) < 32 or sorted(blk.tolist()) == list(range(32)))
    assert set(m["labels"].tolist()) == {0, 1, 2}
    rows = table[torch.from_numpy(m["labels"]), torch.from_numpy(m["perms"])]
    out, lab = ops.mean_sample(table.cuda(), None, None, 0.0, 0.0, seed=2 ** 40 + 7, offset=offset, n=n, want_labels=True)
    torch.cuda.synchronize()
    assert np.array_equal(lab.cpu().numpy(), m["labels"])
    assert torch.equal(out.cpu(), rows), "rows differ from table[label_model, perm_model]"
    out, lab = ops.mean_sample(table.cuda(), None, None, S1, S2, seed=2 ** 40 + 7, offset=offset, n=n, want_labels=True)
    assert np.array_equal(lab.cpu().numpy(), m["labels"])
    base = rows.double().numpy()
    err = np.abs(out.double().cpu().numpy() - base - (S1 * m["jitter"][:, None] + S2 * m["pixel"]))
    assert bool((err <= _ms_tol(base)).all()), np.nanmax(err)


def test_mean_sampler_advances_and_resumes_its_stream():
    from csl_gan_amd.mean_sampler import MeanSampler
    torch.manual_seed(77)
    g = torch.Generator().manual_seed(5)

    def sampler():
        ms = MeanSampler(noise_std=0.12, num_samples=32, mean_size=1000, dataset_size=180000, n_classes=2, smallest_class_size=70000, device="cuda")
        ms.mean_samples = table.cuda()
        return ms

    table = torch.randn(2, 32, 3, 16, 16, generator=g)
    nhwc = table.permute(0, 1, 3, 4, 2).reshape(2, 32, 768)
    seed = NS.mean_sampler_seed(77)

    def check(ms, offset, n):
        r, y = ms.sample(n, noise_std=S2, noise_mean_std=S1)
        torch.cuda.synchronize()
        assert ms._seed == seed and ms.state_dict() == {"seed": seed, "draws": offset}
        m = NS.mean_sample_draws(n, 32, 2, 768, seed, offset)
        assert np.array_equal(y.cpu().numpy(), m["labels"])
        base = nhwc[torch.from_numpy(m["labels"]), torch.from_numpy(m["perms"])].double().numpy()
        got = r.permute(0, 2, 3, 1).double().cpu().numpy().reshape(n, 768)          # the batch is channels-last in memory
        err = np.abs(got - base - (S1 * m["jitter"][:, None] + S2 * m["pixel"]))
        assert bool((err <= _ms_tol(base)).all()), (offset, np.nanmax(err))

    ms = sampler()
    check(ms, 1, 128)
    check(ms, 2, 70)
    ms2 = sampler()
    ms2.load_state_dict(ms.state_dict())
    check(ms2, 3, 128)
