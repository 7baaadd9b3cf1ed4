"""csl_gan_amd.generate / csl_gan_amd.gensamples on the CPU: the host restatement of the indexed latent stream against a model
built here from the oracle's Philox primitives, chunk invariance, seed separation from the other device streams, the command line
end to end (cache format, PNGs, tail, batch-size / shard invariance, labels) and the host-side argument checks of the two C-ABI
entries behind the device path (no launch, no device needed)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import noise_streams as NS

SEEDS = [0, 123, 2 ** 32 + 5, 2 ** 64 - 1]
FIRSTS = [0, 1, 2 ** 32 - 3, 2 ** 40 + 7]          # 2^32 - 3: the rows carry into the counter's high index word
DIMS = [1, 3, 100, 128, 130]
N_ROWS = 257
SEED_TAG, COUNTER_TAG = 0x6C6174656E747A73, 0x7A6C6174


def model_normals(seed, first, n, dim, dtype=np.float64):
    """The stream as include/cslgan.h states it, from the oracle's primitives: key = seed_words(seed ^ tag), counter
    (q, g lo, g hi, tag) -> columns 4q .. 4q+3 of row g - first."""
    k0, k1 = NS.seed_words((int(seed) ^ SEED_TAG) & (2 ** 64 - 1))
    g = np.array([(int(first) + i) & (2 ** 64 - 1) for i in range(n)], dtype=np.uint64)[:, None]
    q = np.arange((dim + 3) // 4, dtype=np.uint64)[None, :]
    words = NS.philox4x32_10(q, g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), COUNTER_TAG, k0, k1)
    return NS.normals_of_words(words, dim, dtype)


@pytest.mark.parametrize("seed", SEEDS)
def test_host_latent_stream_equals_the_oracle_model(seed):
    from csl_gan_amd import generate
    assert generate.latent_seed(seed) == (seed ^ SEED_TAG) & (2 ** 64 - 1)
    for first in FIRSTS:
        for dim in DIMS:
            z = generate.latent_normals_host(seed, first, N_ROWS, dim)
            assert z.dtype == np.float32 and z.shape == (N_ROWS, dim)
            exp = model_normals(seed, first, N_ROWS, dim)
            err = float(np.abs(z.astype(np.float64) - exp).max())
            assert err <= 1e-6, (seed, first, dim, err)            # the fp32 cast of values up to 5.9
            assert float(np.abs(exp).max()) <= np.sqrt(-2.0 * np.log(2.0 ** -25))
    # rows are distinct streams, and so are seeds
    a, b = generate.latent_normals_host(seed, 0, 4, 128), generate.latent_normals_host(seed ^ 1, 0, 4, 128)
    assert float(np.mean(a[0] == a[1])) < 0.05 and float(np.mean(a == b)) < 0.05


@pytest.mark.parametrize("first,n,a,b", [(0, 64, 5, 23), (2 ** 32 - 9, 20, 3, 17), (2 ** 40 + 7, 33, 0, 33), (7, 10, 9, 10)])
def test_a_chunk_equals_the_slice_of_a_larger_draw_bitwise(first, n, a, b):
    from csl_gan_amd import generate
    for dim in (3, 100, 128):
        whole = generate.latent_normals_host(99, first, n, dim)
        part = generate.latent_normals_host(99, first + a, b - a, dim)
        assert np.array_equal(whole[a:b].view(np.uint32), part.view(np.uint32))
    assert np.array_equal(generate.labels_host(first, n, 10)[a:b], generate.labels_host(first + a, b - a, 10))
    assert np.array_equal(generate.labels_host(first, n, 10), np.array([(first + i) % 10 for i in range(n)]))


def test_latent_seed_is_no_seed_of_the_other_streams():
    from csl_gan_amd import generate
    for s in (0, 1, 42, 2 ** 32 + 5):
        ours = generate.latent_seed(s)
        for r in range(8):
            assert ours != NS.engine_seed(s, r) & (2 ** 64 - 1)
            for dist in (False, True):
                assert ours != NS.mean_sampler_seed(NS.process_seed(s, r, dist))


# ---- the command line on the CPU ----------------------------------------------------------------------------------------------------

ARGS = ["-e", "3", "-d", "cpu"]


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """An MNIST Vanilla conditional generator with non-default weights, saved as train.py saves it, next to its opt.txt."""
    from csl_gan_amd import init_util, options, util
    out = str(tmp_path_factory.mktemp("gensamples_run")) + "/"
    opt = options.parse(["MNIST", "-cond", "-o", out, "--manual_seed", "77", "--synthetic"])
    with open(out + "opt.txt", "w") as f:
        json.dump(opt.__dict__, f)
    G, _ = init_util.init_models(opt, init_D=False)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in G.parameters():
            p.mul_(1.5).add_(torch.randn(p.shape, generator=g) * 0.05)
    util.save_model(3, G, torch.optim.Adam(G.parameters()), 0, out + "saves/G-3")
    return out, opt, G


@pytest.fixture(scope="module")
def base_run(run_dir):
    from csl_gan_amd import gensamples
    from csl_gan_amd.pipeline import CachedImages
    out = run_dir[0]
    gensamples.main([out] + ARGS + ["-n", "25", "-bs", "10", "--cache", out + "syn", "--png", "4"])
    return CachedImages(out + "syn")


def _expected(run_dir, first, n, label=-1, bs=10):
    """The bytes the test computes itself: the host expression on G(latent_normals_host, labels), in the run's batches (a CPU GEMM
    may round differently per batch shape)."""
    from csl_gan_amd import generate
    _, opt, G = run_dir
    z = torch.from_numpy(generate.latent_normals_host(opt.manual_seed, first, n, opt.g_latent_dim))
    y = torch.full((n,), label, dtype=torch.int64) if label >= 0 else (torch.arange(first, first + n) % 10)
    G.eval()
    with torch.no_grad():
        x = torch.cat([G(z[i:i + bs], y[i:i + bs]) for i in range(0, n, bs)]).permute(0, 2, 3, 1)
    t = x * 1.0 + 0.0
    return t.clamp(0, 1).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).numpy(), y.numpy()


def test_cli_writes_a_cache_that_cached_images_opens(run_dir, base_run):
    c = base_run
    assert c.n == 25 and len(c) == 25 and (c.H, c.W, c.C) == (28, 28, 1) and c.signed is False       # the tail of 5 is there
    assert c.x.shape == (25, 28, 28, 1) and c.x.dtype == np.uint8
    assert np.array_equal(c.labels, np.arange(25) % 10)
    for k in ("version", "n", "H", "W", "C", "signed", "dtype", "layout", "generator"):
        assert k in c.hdr
    gen = c.hdr["generator"]
    assert gen["seed"] == 77 and gen["first_index"] == 0 and gen["epochs"] == 3 and gen["checkpoint"].endswith("saves/G-3")
    exp, lab = _expected(run_dir, 0, 25)
    assert np.array_equal(np.asarray(c.x), exp), "bytes differ from the host expression on G(latent_normals_host(...), labels)"
    assert int(exp.max()) - int(exp.min()) > 64                     # a generator that paints something
    assert torch.is_grad_enabled()                                   # main() leaves the process as it found it


def test_cli_pngs_are_the_cache_rows_as_rgb(run_dir, base_run):
    from PIL import Image
    d = run_dir[0] + "G-3-samples/"
    assert sorted(os.listdir(d)) == ["1.png", "2.png", "3.png", "4.png"]
    for k in range(4):
        im = Image.open(d + "%d.png" % (k + 1))
        assert im.mode == "RGB" and im.size == (28, 28)
        assert np.array_equal(np.asarray(im), np.repeat(np.asarray(base_run.x[k]), 3, axis=2))


def test_cli_without_cache_writes_one_png_per_sample(run_dir, tmp_path):
    import shutil
    from csl_gan_amd import gensamples
    from PIL import Image
    out = str(tmp_path / "run") + "/"
    os.makedirs(out + "saves")
    shutil.copy(run_dir[0] + "opt.txt", out + "opt.txt")
    shutil.copy(run_dir[0] + "saves/G-3", out + "saves/G-3")
    gensamples.main([out] + ARGS + ["-n", "25", "-bs", "10"])
    assert sorted(os.listdir(out + "G-3-samples/"), key=lambda s: int(s[:-4])) == ["%d.png" % k for k in range(1, 26)]
    assert not [f for f in os.listdir(out) if f.endswith((".u8", ".json", ".npy"))]
    exp, _ = _expected(run_dir, 0, 25)
    for k in (0, 9, 10, 24):
        assert np.array_equal(np.asarray(Image.open(out + "G-3-samples/%d.png" % (k + 1)))[:, :, :1], exp[k])


def _levels_apart(a, b):
    return int(np.abs(np.asarray(a).astype(np.int16) - np.asarray(b).astype(np.int16)).max())


def test_cli_output_does_not_depend_on_batch_size_or_sharding(run_dir, base_run, tmp_path):
    """A CPU GEMM may round differently per batch shape, so the bytes are held to one level; labels and z are exact."""
    from csl_gan_amd import gensamples
    from csl_gan_amd.pipeline import CachedImages
    out = run_dir[0]
    gensamples.main([out] + ARGS + ["-n", "25", "-bs", "7", "--cache", str(tmp_path / "bs7")])
    c7 = CachedImages(str(tmp_path / "bs7"))
    assert np.array_equal(c7.labels, base_run.labels)
    assert _levels_apart(c7.x, base_run.x) <= 1
    gensamples.main([out] + ARGS + ["-n", "5", "-bs", "10", "--first_index", "10", "--cache", str(tmp_path / "shard")])
    sh = CachedImages(str(tmp_path / "shard"))
    assert sh.n == 5 and np.array_equal(sh.labels, base_run.labels[10:15]) and sh.hdr["generator"]["first_index"] == 10
    assert _levels_apart(sh.x, base_run.x[10:15]) <= 1
    assert not os.path.exists(str(tmp_path / "G-3-samples"))


def test_cli_fixed_label_and_seed(run_dir, base_run, tmp_path):
    from csl_gan_amd import gensamples
    from csl_gan_amd.pipeline import CachedImages
    out = run_dir[0]
    gensamples.main([out] + ARGS + ["-n", "12", "-bs", "5", "--label", "3", "--cache", str(tmp_path / "l3")])
    c = CachedImages(str(tmp_path / "l3"))
    assert np.array_equal(c.labels, np.full(12, 3)) and c.hdr["generator"]["label_mode"] == "fixed:3"
    exp, _ = _expected(run_dir, 0, 12, label=3, bs=5)
    assert _levels_apart(c.x, exp) <= 1
    gensamples.main([out] + ARGS + ["-n", "12", "-bs", "12", "--seed", "78", "--cache", str(tmp_path / "s78")])
    other = CachedImages(str(tmp_path / "s78"))
    assert other.hdr["generator"]["seed"] == 78 and _levels_apart(other.x, base_run.x[:12]) > 1


def test_cached_rows_feed_the_prefetcher(base_run):
    """The synthetic cache goes through the trainer's own reader: EpochSampler + DevicePrefetcher (host form)."""
    from csl_gan_amd.pipeline import DevicePrefetcher, EpochSampler
    pf = DevicePrefetcher(base_run, EpochSampler(base_run.n, 5, shuffle=False), device="cpu", flip=False)
    batches = list(pf)
    assert len(batches) == 5
    x, y = batches[0]
    assert tuple(x.shape) == (5, 1, 28, 28) and np.array_equal(y.numpy(), np.arange(5))
    assert torch.equal(x, base_run.to_float(base_run.x[:5]))


def test_trainer_data_path_reads_the_synthetic_cache(run_dir, base_run, tmp_path):
    """`train --data_cache OUT` on the cache `gensamples --cache OUT` wrote: no --data_path, no rebuild."""
    from csl_gan_amd import data, options
    opt = options.parse(["MNIST", "-cond", "-bs", "5", "-tss", "25", "--data_cache", run_dir[0] + "syn", "-d", str(tmp_path / "no_such_dir"),
                         "-o", str(tmp_path / "o")])
    assert data.is_image_cache(opt.data_cache) and not data.is_image_cache(run_dir[0] + "nothing")
    ds, dl, pub, pdl = data.init_data(opt)
    assert pub is None and pdl is None and len(ds) == 25 and len(dl) == 5
    seen = sorted(int(v) for _, y in dl for v in y)
    assert seen == sorted((np.arange(25) % 10).tolist())
    x, y = ds.get_item_with_label(3, number=13)
    assert y == 3 and torch.equal(x, base_run.to_float(base_run.x[13:14])[0])
    opt.dataset, opt.im_size = "CelebA", 64
    with pytest.raises(RuntimeError, match="holds 28x28x1"):
        data.init_data(opt)


# ---- host-side argument checks of the two entries -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from csl_gan_amd import build, _lib
    build.build()
    return _lib.lib()


def test_abi_is_version_7_with_the_two_entries(L):
    from csl_gan_amd import _lib
    assert _lib.ABI_VERSION == 7 and L.cslgan_version() == 7
    assert {"cslgan_latent_normal_f32", "cslgan_f32_to_u8"} <= set(_lib.EXPORTS)


def test_latent_normal_refuses_bad_arguments_before_any_launch(L):
    err = lambda: L.cslgan_last_error()
    ok = dict(seed=1, first=0, dev=None, n=4, dim=8, z=16, n_classes=10, fixed=-1, labels=16)
    call = lambda **kw: L.cslgan_latent_normal_f32(*[dict(ok, **kw)[k] for k in ("seed", "first", "dev", "n", "dim", "z", "n_classes", "fixed", "labels")], None)
    assert call(z=None) == -1 and b"null" in err()
    assert call(n=0) == -1 and b"n=0" in err()
    assert call(n=-3) == -1 and b"n=-3" in err()
    assert call(dim=0) == -1 and b"dim=0" in err()
    assert call(dim=-1) == -1 and b"dim=-1" in err()
    assert call(fixed=10) == -1 and b"fixed_label=10" in err()
    assert call(fixed=11, n_classes=1) == -1 and b"fixed_label=11" in err()
    assert call(n_classes=0) == -1 and b"n_classes=0" in err()


def test_f32_to_u8_refuses_bad_arguments_before_any_launch(L):
    err = lambda: L.cslgan_last_error()
    assert L.cslgan_f32_to_u8(None, 8, 0.5, 0.5, 16, None) == -1 and b"null" in err()
    assert L.cslgan_f32_to_u8(16, 8, 0.5, 0.5, None, None) == -1 and b"null" in err()
    assert L.cslgan_f32_to_u8(16, 0, 0.5, 0.5, 16, None) == -1 and b"n=0" in err()
    assert L.cslgan_f32_to_u8(16, -5, 0.5, 0.5, 16, None) == -1 and b"n=-5" in err()


def test_the_package_does_not_import_the_oracle():
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csl_gan_amd")
    for name in ("generate.py", "gensamples.py"):
        src = open(os.path.join(root, name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), name
