"""The device path of csl_gan_amd.generate (-m gpu): cslgan_latent_normal_f32 against a host model built from the oracle's Philox
primitives, cslgan_f32_to_u8 bit for bit against the host expression, and the generation loop end to end (recorded graph + eager
tail) for three generator families against the package's CPU path.

Tolerance of a unit normal: the project's gate of tests/test_noise_streams_gpu.py.  D is the largest distance between the Box-Muller
formula in numpy float32 and in float64 over exactly the draws of the case grid below, computed on the host; the gate is 4 D (the
factor 4 is the project's margin for the device's fast log / sincos).  On this grid D = 1.31e-5, the gate 5.2e-5.
"""
import functools
import json

import numpy as np
import pytest
import torch

from oracle import noise_streams as NS

pytestmark = pytest.mark.gpu

SEEDS = [0, 123, 2 ** 32 + 5, 2 ** 64 - 1]
FIRSTS = [0, 1, 2 ** 32 - 3, 2 ** 40 + 7]          # 2^32 - 3: the rows carry into the counter's high index word
DIMS = [1, 3, 100, 128, 130]
N_ROWS = 257
SEED_TAG, COUNTER_TAG = 0x6C6174656E747A73, 0x7A6C6174
GRID = [(s, f, d) for s in SEEDS for f in FIRSTS for d in DIMS]


def _ops():
    from csl_gan_amd import ops
    return ops


def _words(seed, first, n, dim):
    k0, k1 = NS.seed_words((int(seed) ^ SEED_TAG) & (2 ** 64 - 1))
    g = np.array([(int(first) + i) & (2 ** 64 - 1) for i in range(n)], dtype=np.uint64)[:, None]
    q = np.arange((dim + 3) // 4, dtype=np.uint64)[None, :]
    return NS.philox4x32_10(q, g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), COUNTER_TAG, k0, k1)


@functools.lru_cache(maxsize=None)
def _model(seed, first, n, dim):
    return NS.normals_of_words(_words(seed, first, n, dim), dim)


@functools.lru_cache(maxsize=None)
def _D():
    """max |z_fp32 - z_fp64| of the formula over every draw of the grid: host arithmetic only."""
    d = 0.0
    for s, f, dim in GRID:
        z32 = NS.normals_of_words(_words(s, f, N_ROWS, dim), dim, np.float32)
        d = max(d, float(np.abs(z32.astype(np.float64) - _model(s, f, N_ROWS, dim)).max()))
    assert 5e-6 < d < 2.5e-4, d
    return d


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- the latent kernel ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_latent_normal_equals_the_model(seed):
    ops, gate = _ops(), 4.0 * _D()
    worst = 0.0
    for first in FIRSTS:
        for dim in DIMS:
            z = ops.latent_normal(seed, first, N_ROWS, dim)
            torch.cuda.synchronize()
            assert tuple(z.shape) == (N_ROWS, dim) and z.dtype == torch.float32
            err = np.abs(z.double().cpu().numpy() - _model(seed, first, N_ROWS, dim))
            worst = max(worst, float(np.nanmax(err)))
            bad = np.argwhere(~(err <= gate))
            assert bad.size == 0, "seed %d first %d dim %d: %d elements off by more than %.3e (first at %s, max %.3e)" % (
                seed, first, dim, len(bad), gate, bad[0], np.nanmax(err))
    print("\nlatent stream deviation: seed=%d  max=%.3e  D=%.3e  gate=%.3e" % (seed, worst, _D(), gate))


@pytest.mark.parametrize("dim", [3, 100, 128])
def test_latent_index_by_value_in_hbm_and_in_chunks_is_the_same_row_bitwise(dim):
    ops = _ops()
    dev = lambda v: torch.full((1,), v, device="cuda", dtype=torch.int64)
    for first in (5, 2 ** 32 - 9, 2 ** 40 + 7):                  # 2^32 - 9 .. 2^32 + 23: the chunk boundaries straddle the carry
        n = 32
        whole = ops.latent_normal(77, first, n, dim)
        in_hbm = ops.latent_normal(77, 0, n, dim, first_index_dev=dev(first))
        a = first // 2
        split = ops.latent_normal(77, a, n, dim, first_index_dev=dev(first - a))
        assert torch.equal(_bits(whole), _bits(in_hbm)) and torch.equal(_bits(whole), _bits(split))
        parts = [ops.latent_normal(77, first + lo, hi - lo, dim) for lo, hi in ((0, 4), (4, 9), (9, 10), (10, 32))]
        assert torch.equal(_bits(whole), _bits(torch.cat(parts)))
        # a chunk that starts one float into its allocation takes the element-wise stores: the same bits
        store = torch.empty(1 + 7 * dim, device="cuda")
        off = ops.latent_normal(77, first + 4, 7, dim, out=store[1:].view(7, dim))
        assert torch.equal(_bits(off), _bits(whole[4:11]))
        other = ops.latent_normal(78, first, n, dim)
        assert float((other == whole).float().mean()) < 0.05


def test_latent_labels_are_the_index_mod_classes():
    ops = _ops()
    for first in (0, 2 ** 32 - 3, 2 ** 40 + 7):
        for nc in (1, 2, 10):
            z, y = ops.latent_normal(3, first, 40, 16, n_classes=nc, want_labels=True)
            assert np.array_equal(y.cpu().numpy(), np.array([(first + i) % nc for i in range(40)]))
            _, y2 = ops.latent_normal(3, 1, 40, 16, first_index_dev=torch.full((1,), first - 1, device="cuda", dtype=torch.int64), n_classes=nc,
                                      want_labels=True)
            assert torch.equal(y, y2)
    _, y = ops.latent_normal(3, 2 ** 32 - 3, 40, 16, n_classes=10, fixed_label=7, want_labels=True)
    assert bool((y == 7).all())
    with pytest.raises(RuntimeError, match="fixed_label"):
        ops.latent_normal(3, 0, 4, 16, n_classes=10, fixed_label=10, want_labels=True)


# ---- the quantisation kernel ----------------------------------------------------------------------------------------------------------

LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 3 * 28 * 28, 64 * 64 * 3 + 1]
PAIRS = [(0.5, 0.5), (1.0, 0.0)]


def _host_u8(x, scale, bias):
    t = x * scale + bias
    return t.clamp(0, 1).mul(255).add(0.5).clamp(0, 255).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _probe_values(scale, bias):
    """fp32 inputs around every rounding boundary (k + 0.5) / 255 of the host expression (+- 4 ulp), the endpoints, values outside
    [-1.2, 1.2] and +- inf."""
    k = np.arange(255, dtype=np.float64)
    centre = (((k + 0.5) / 255.0 - bias) / scale).astype(np.float32)
    vals = [centre]
    up, dn = centre.copy(), centre.copy()
    for _ in range(4):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        vals += [up.copy(), dn.copy()]
    ends = np.array([-1.0, 0.0, 1.0, -bias / scale, (1.0 - bias) / scale, -0.0, 1e-45, -1e-45, 0.999999, -0.999999], dtype=np.float32)
    ends = np.concatenate([ends] + [np.nextafter(ends, np.float32(s)) for s in (np.inf, -np.inf)])
    out = np.array([-1.2, 1.2, -1.2000001, 1.2000001, -1.5, 1.5, 2.0, -2.0, 100.0, -100.0, 3e38, -3e38, np.inf, -np.inf], dtype=np.float32)
    return torch.from_numpy(np.concatenate(vals + [ends, out]))


@pytest.mark.parametrize("scale,bias", PAIRS)
def test_f32_to_u8_is_bit_identical_to_the_host_expression(scale, bias):
    ops = _ops()
    vals = _probe_values(scale, bias)
    assert vals.numel() > 2295 and len(set(_host_u8(vals, scale, bias).tolist())) == 256          # every level is reached
    g = torch.Generator().manual_seed(11)
    for L in LENGTHS + [vals.numel(), vals.numel() + 2]:
        reps = -(-L // vals.numel())
        shift = int(torch.randint(0, vals.numel(), (1,), generator=g))
        x = torch.roll(vals, shift).repeat(reps)[:L].contiguous()
        exp = _host_u8(x, scale, bias)
        for so in (0, 1):
            for do in (0, 1):
                src = torch.empty(L + 1, device="cuda")
                src[so:so + L].copy_(x)
                dst = torch.full((L + 2,), 77, device="cuda", dtype=torch.uint8)
                ops.f32_to_u8(src[so:so + L], scale, bias, out=dst[do:do + L])
                torch.cuda.synchronize()
                got = dst.cpu()
                bad = torch.nonzero(got[do:do + L] != exp).flatten()
                assert bad.numel() == 0, "len %d src+%d dst+%d: %d bytes differ, first at %d: x=%r got %d host %d" % (
                    L, so, do, bad.numel(), int(bad[0]), float(x[bad[0]]), int(got[do + bad[0]]), int(exp[bad[0]]))
                assert bool((got[:do] == 77).all()) and bool((got[do + L:] == 77).all()), "wrote outside its %d bytes" % L


def test_f32_to_u8_maps_nan_to_zero():
    ops = _ops()
    x = torch.tensor([float("nan"), 0.3, float("nan"), -float("nan"), 1.0, float("nan"), float("nan")], device="cuda")
    for scale, bias in PAIRS:
        for t in (x, x[1:]):                                         # aligned and element-wise paths
            got = ops.f32_to_u8(t, scale, bias).cpu()
            nan = torch.isnan(t.cpu())
            assert bool((got[nan] == 0).all())
            assert torch.equal(got[~nan], _host_u8(t.cpu()[~nan], scale, bias))


@pytest.mark.parametrize("signed", [True, False])
def test_all_256_levels_survive_the_round_trip(signed):
    from csl_gan_amd import _lib
    ops = _ops()
    levels = torch.arange(256, dtype=torch.uint8, device="cuda")
    f = torch.empty(256, device="cuda")
    scale, bias = (1.0 / 127.5, -1.0) if signed else (1.0 / 255.0, 0.0)         # CachedImages.scale / .bias
    ops.check(_lib.lib().cslgan_u8_to_f32_nhwc(ops._p(levels), None, 1, 1, 256, 1, scale, bias, ops._p(f), torch.cuda.current_stream().cuda_stream),
              "u8_to_f32_nhwc")
    back = ops.f32_to_u8(f, *((0.5, 0.5) if signed else (1.0, 0.0)))
    assert torch.equal(back, levels)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

CONFIGS = {
    "celeba_gn": ["CelebA", "-dpm", "gc", "-gcm", "adaptive-pl", "-nms", "4"],
    "mnist_dcrn_bn": ["MNIST", "--model", "DeepConvResNet"],
    "mnist_vanilla_cond": ["MNIST", "-cond"],
}
N, BS, SEED = 10, 4, 4242


class _Collect:
    def __init__(self, n, shape, dtype):
        self.a = np.zeros((n,) + tuple(shape), dtype=dtype)

    def __call__(self, start, rows, labels=None):
        self.a[start:start + len(rows)] = rows


def _run(G, opt, device, bs, graph, first=0, n=N, compute_dtype=None):
    from csl_gan_amd import generate
    gen = generate.SampleGenerator(G, opt, device, SEED, bs, hip_graph=graph, compute_dtype=compute_dtype, keep_float=True)
    u8, f32 = _Collect(n, (gen.H, gen.W, gen.C), np.uint8), _Collect(n, (gen.H, gen.W, gen.C), np.float32)
    labels = np.zeros(n, dtype=np.int64)

    def sink(start, rows, lab):
        u8(start, rows)
        labels[start:start + len(rows)] = lab
    try:
        gen.generate(first, n, sink, float_sink=f32)
        graphed = gen.graph is not None
    finally:
        gen.release()
    assert graphed == (bool(graph) and device != "cpu" and n >= bs)
    return u8.a, f32.a, labels


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(opt, G on the device, G on the CPU with the same weights, the CPU path's bytes / floats / labels of rows 0..9)."""
    import tempfile
    from csl_gan_amd import init_util, options
    out = tempfile.mkdtemp(prefix="gensamples_%s_" % name) + "/"
    opt = options.parse(CONFIGS[name] + ["-o", out, "--manual_seed", "9", "--synthetic", "-gd", "cpu", "-dd", "cpu"])
    Gc, _ = init_util.init_models(opt, init_D=False)
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for p in Gc.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.02)
        if name == "mnist_dcrn_bn":                          # move the running statistics so that the eval path matters
            Gc.train()
            for _ in range(2):
                Gc(torch.randn(16, opt.g_latent_dim, generator=g) * 1.5)
            assert any(float(m.running_mean.abs().max()) > 1e-3 for m in Gc.modules() if isinstance(m, torch.nn.BatchNorm2d))
    Gc.eval()
    opt.g_device = "cuda:0"
    Gd, _ = init_util.init_models(opt, init_D=False)
    Gd.load_state_dict(Gc.state_dict())
    opt.g_device = "cpu"
    return opt, Gd, Gc, _run(Gc, opt, "cpu", N, False)


def _apart(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_generation_end_to_end(name):
    opt, Gd, Gc, (u8_cpu, f_cpu, lab_cpu) = _setup(name)
    ops = _ops()
    u8_g, f_g, lab_g = _run(Gd, opt, "cuda:0", BS, True)                   # two graph replays + an eager tail of 2
    # float bound against the CPU path (tests/test_models_golden.py's tolerance for the same forward), hence one level on the bytes
    err = float(np.abs(f_g - f_cpu).max())
    print("\n%s: graphed vs CPU path: float max %.3e, bytes apart %d, float range [%.3f, %.3f]" % (name, err, _apart(u8_g, u8_cpu), f_cpu.min(), f_cpu.max()))
    assert np.isfinite(f_g).all() and err <= 1e-3, err
    assert _apart(u8_g, u8_cpu) <= 1
    assert np.array_equal(lab_g, lab_cpu) and np.array_equal(lab_g, (np.arange(N) % 10) if opt.conditional else np.zeros(N))
    assert float(f_cpu.max() - f_cpu.min()) > 0.05                         # a generator that paints something
    # batch-size and graph invariance
    z_whole = ops.latent_normal(SEED, 0, N, opt.g_latent_dim)
    z_parts = torch.cat([ops.latent_normal(SEED, s, min(BS, N - s), opt.g_latent_dim) for s in range(0, N, BS)])
    assert torch.equal(_bits(z_whole), _bits(z_parts))
    u8_a, f_a, _ = _run(Gd, opt, "cuda:0", N, False)
    u8_b, f_b, _ = _run(Gd, opt, "cuda:0", BS, False)
    print("%s: -bs %d eager vs -bs %d eager: float max %.3e; graphed vs eager -bs %d: %.3e" % (
        name, N, BS, float(np.abs(f_a - f_b).max()), BS, float(np.abs(f_g - f_b).max())))
    assert float(np.abs(f_a - f_b).max()) <= 1e-5 and _apart(u8_a, u8_b) <= 1
    assert float(np.abs(f_g - f_b).max()) <= 1e-5 and _apart(u8_g, u8_b) <= 1
    # a replay draws new rows
    assert float(np.abs(f_g[0:4] - f_g[4:8]).max()) > 1e-3 and not np.array_equal(u8_g[0:4], u8_g[4:8])
    # the bytes are the quantisation of the floats that were handed over
    q = _host_u8(torch.from_numpy(f_g), *((0.5, 0.5) if name == "celeba_gn" else (1.0, 0.0))).numpy()
    assert np.array_equal(q, u8_g)


def test_a_shard_equals_the_rows_of_the_whole_range():
    opt, Gd, Gc, _ = _setup("mnist_vanilla_cond")
    u8_g, f_g, lab_g = _run(Gd, opt, "cuda:0", BS, True)
    u8_s, f_s, lab_s = _run(Gd, opt, "cuda:0", 3, True, first=4, n=5)       # one replay of 3 + an eager tail of 2
    assert np.array_equal(lab_s, lab_g[4:9])
    assert float(np.abs(f_s - f_g[4:9]).max()) <= 1e-5 and _apart(u8_s, u8_g[4:9]) <= 1


def test_celeba_cache_from_the_command_line_restores_the_generators_range(tmp_path):
    from csl_gan_amd import gensamples, util
    from csl_gan_amd.pipeline import CachedImages
    opt, Gd, Gc, (u8_cpu, f_cpu, _) = _setup("celeba_gn")
    out = str(tmp_path) + "/"
    import os
    os.makedirs(out + "saves")
    d = dict(opt.__dict__, output_dir=out)
    with open(out + "opt.txt", "w") as f:
        json.dump(d, f)
    util.save_model(2, Gc, torch.optim.Adam(Gc.parameters()), 0, out + "saves/G-2")
    gen = gensamples.main([out, "-e", "2", "-n", str(N), "-bs", str(BS), "-d", "cuda:0", "--seed", str(SEED), "--cache", out + "syn"])
    assert gen.compute_dtype == "fp32" and gen.graph is None                 # released
    c = CachedImages(out + "syn")
    assert c.signed is True and (c.n, c.H, c.W, c.C) == (N, 64, 64, 3) and not c.labels.any()
    assert c.hdr["generator"]["compute_dtype"] == "fp32" and c.hdr["generator"]["seed"] == SEED
    assert _apart(np.asarray(c.x), u8_cpu) <= 1
    back = c.to_float(c.x[:]).permute(0, 2, 3, 1).numpy()
    assert float(np.abs(back - f_cpu).max()) <= 1.0 / 255.0 + 1e-3


def test_fp32_auto_route_on_the_celeba_generator():
    opt, Gd, Gc, (u8_cpu, f_cpu, _) = _setup("celeba_gn")
    u8, f, _ = _run(Gd, opt, "cuda:0", BS, True, compute_dtype="fp32_auto")
    err = float(np.abs(f - f_cpu).max())
    print("\nfp32_auto vs CPU path: float max %.3e" % err)
    assert err <= 1e-3 and _apart(u8, u8_cpu) <= 1
    assert _ops().get_compute_dtype() == "fp32"                              # release() put the switch back
