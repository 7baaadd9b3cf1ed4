"""cslgan_mom_transpose_u8, cslgan_mom_colsum_i64, cslgan_mom_gram_i64, cslgan_mom_mirror_i64 and their driver on the device against the
host model of csl_gan_amd.moments.  Random bytes from fixed seeds; every comparison of moments is integer equality."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csl_gan_amd import moments as MO

DEV = "cuda:0"
CANARY8 = 77
CANARY64 = -123456789012345
SHAPES = [(1, 1), (63, 50), (64, 64), (65, 129), (300, 784)]


@functools.lru_cache(maxsize=None)
def _case(n, D, seed=0):
    """(x uint8 [n, D], its host moments): rows of all 0 and all 255 among random ones.  Read-only."""
    x = np.random.default_rng(1000 * n + D + seed).integers(0, 256, (n, D), dtype=np.uint8)
    x[0] = 0
    x[n - 1] = 255
    m = MO.byte_moments_host(x)
    for a in (x, m["s1"], m["s2"]):
        a.setflags(write=False)
    return x, m


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared cases are read-only


def _tight(x):
    """x on the device at an odd byte address, its last row ending with the last byte of its allocation."""
    buf = torch.empty(x.size + 1, device=DEV, dtype=torch.uint8)
    t = buf[1:].view(x.shape)
    t.copy_(torch.from_numpy(np.array(x)))
    return t


def _tile_mask(D):
    """True where mom_gram writes: the 128 x 128 tiles on and below the diagonal."""
    t = np.arange(D) // 128
    return t[:, None] >= t[None, :]


# ---- transpose ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,D", SHAPES)
def test_transpose_values_padding_and_margins(n, D):
    from csl_gan_amd import ops
    x, _ = _case(n, D)
    np_ = ops.mom_padded_rows(n)
    assert np_ % 64 == 0 and 0 <= np_ - n < 64
    front, back = 256, 4096
    buf = torch.full((front + D * np_ + back,), CANARY8, device=DEV, dtype=torch.int8)
    out = buf[front:front + D * np_].view(D, np_)
    got = ops.mom_transpose(_tight(x), out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    xt = host[front:front + D * np_].reshape(D, np_)
    assert np.array_equal(xt[:, :n].astype(np.int64), x.T.astype(np.int64) - 128)
    assert not xt[:, n:].any()
    assert (host[:front] == CANARY8).all() and (host[front + D * np_:] == CANARY8).all()
    fresh = ops.mom_transpose(_dev(x))                     # allocated by the wrapper, an aligned input
    assert fresh.shape == (D, np_) and fresh.dtype == torch.int8 and np.array_equal(fresh.cpu().numpy(), xt)


# ---- column sums -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,D", SHAPES)
def test_column_sums_add_over_two_calls(n, D):
    from csl_gan_amd import ops
    (x, m), (x2, m2) = _case(n, D), _case(n // 2 + 1, D, seed=5)
    buf = torch.full((D + 8,), CANARY64, device=DEV, dtype=torch.int64)
    s1 = buf[4:4 + D]
    s1.zero_()
    ops.mom_colsum(ops.mom_transpose(_dev(x)), s1)
    assert np.array_equal(s1.cpu().numpy(), m["s1"])
    ops.mom_colsum(ops.mom_transpose(_dev(x2)), s1)
    got = buf.cpu().numpy()
    assert np.array_equal(got[4:4 + D], m["s1"] + m2["s1"])
    assert (got[:4] == CANARY64).all() and (got[4 + D:] == CANARY64).all()


# ---- Gram -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,D", SHAPES + [(200, 257)])
def test_gram_triangle_of_tiles_two_calls_slack_and_mirror(n, D):
    """mom_gram writes the tiles on and below the diagonal and nothing else: a canary in the tiles above and in the slack of ld > D stays.
    mom_mirror then fills the tiles above; the slack still stays."""
    from csl_gan_amd import ops
    (x, m), (x2, m2) = _case(n, D), _case(n // 2 + 1, D, seed=5)
    ld = D + 5
    mask = _tile_mask(D)
    start = np.full((D, ld), CANARY64, dtype=np.int64)
    start[:, :D][mask] = 0
    S2 = _dev(start)
    ops.mom_gram(ops.mom_transpose(_dev(x)), S2)
    got = S2.cpu().numpy()
    assert np.array_equal(got[:, :D][mask], m["s2"][mask])
    assert (got[:, :D][~mask] == CANARY64).all() and (got[:, D:] == CANARY64).all()
    ops.mom_gram(ops.mom_transpose(_dev(x2)), S2)          # another chunk, another n
    got = S2.cpu().numpy()
    want = m["s2"] + m2["s2"]
    assert np.array_equal(got[:, :D][mask], want[mask])
    assert (got[:, :D][~mask] == CANARY64).all() and (got[:, D:] == CANARY64).all()
    ops.mom_mirror(S2)
    got = S2.cpu().numpy()
    assert np.array_equal(got[:, :D], want) and (got[:, D:] == CANARY64).all()


@pytest.mark.parametrize("pattern", ["all 0", "all 255", "rows alternate", "columns alternate"])
def test_accumulator_at_its_bound(pattern):
    """65536 rows, the longest chunk: every sum is +-2^30 or nearly, in the int32 accumulator of one launch."""
    from csl_gan_amd import ops
    n, D = 65536, 16
    x = np.zeros((n, D), dtype=np.uint8)
    if pattern == "all 255":
        x[:] = 255
    elif pattern == "rows alternate":
        x[1::2] = 255
    elif pattern == "columns alternate":
        x[:, 1::2] = 255
    want = MO.byte_moments_host(x)
    if pattern == "all 0":
        assert (want["s2"] == 2 ** 30).all() and (want["s1"] == -(2 ** 23)).all()
    if pattern == "columns alternate":
        assert want["s2"][0, 1] == -128 * 127 * 65536 and want["s2"][1, 1] == 127 * 127 * 65536
    xt = ops.mom_transpose(_dev(x))
    s1 = torch.zeros(D, device=DEV, dtype=torch.int64)
    S2 = torch.zeros((D, D), device=DEV, dtype=torch.int64)
    ops.mom_colsum(xt, s1)
    ops.mom_gram(xt, S2)
    assert np.array_equal(s1.cpu().numpy(), want["s1"]) and np.array_equal(S2.cpu().numpy(), want["s2"])
    ops.mom_gram(xt, S2)                                   # past int32 in the int64 matrix
    assert np.array_equal(S2.cpu().numpy(), 2 * want["s2"])


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block_rows", [100, 300])
def test_byte_moments_on_the_device_equal_the_host_model(block_rows):
    from csl_gan_amd.pipeline import CachedImages
    x, m = _case(300, 784)
    cache = CachedImages.from_arrays(np.array(x).reshape(300, 28, 28, 1), np.zeros(300), True)
    got = MO.byte_moments(cache, DEV, block_rows=block_rows, chunk_rows=128)
    assert got["n"] == 300 and got["s1"].dtype == np.int64 and got["s2"].dtype == np.int64
    assert np.array_equal(got["s1"], m["s1"]) and np.array_equal(got["s2"], m["s2"])


HWC = (8, 8, 3)


def _run(tmp_path, name, extra):
    from csl_gan_amd import frechet
    vals = str(tmp_path / name)
    stats = frechet.main(["--syn_cache", str(tmp_path / "syn"), "--train_cache", str(tmp_path / "train"), "--nontrain_cache",
                          str(tmp_path / "heldout"), "--baseline", "--values_dir", vals] + extra)
    return stats, {f: np.load(os.path.join(vals, f)) for f in sorted(os.listdir(vals))}


def test_cli_on_the_device_equals_the_cpu_whatever_the_blocking(tmp_path):
    from csl_gan_amd.generate import CacheWriter
    rng = np.random.default_rng(31)
    for name, n, hi in (("train", 300, 256), ("heldout", 257, 256), ("syn", 130, 200)):
        w = CacheWriter(str(tmp_path / name), n, *HWC, True, {"note": "test rows"})
        w(0, rng.integers(0, hi, (n,) + HWC, dtype=np.uint8), np.zeros(n, dtype=np.int64))
        w.close()
    cpu, cpu_vals = _run(tmp_path, "cpu", ["-d", "cpu"])
    cpu2, _ = _run(tmp_path, "cpu2", ["-d", "cpu"])
    dev, dev_vals = _run(tmp_path, "dev", ["-d", DEV])
    blk, blk_vals = _run(tmp_path, "blk", ["-d", DEV, "--block_rows", "128"])
    assert set(cpu) == {"syn", "baseline_heldout"}
    assert list(cpu_vals) == ["baseline_heldout_s1.npy", "baseline_heldout_s2.npy", "syn_s1.npy", "syn_s2.npy"]
    for vals in (dev_vals, blk_vals):
        assert list(vals) == list(cpu_vals)
        for f, v in vals.items():
            assert v.dtype == np.int64 and np.array_equal(v, cpu_vals[f]), f
    # the float step is one host function of equal integers: two runs on the CPU gave identical floats, so the device's are held to equality
    assert json.dumps(cpu2) == json.dumps(cpu)
    assert json.dumps(dev) == json.dumps(cpu) and json.dumps(blk) == json.dumps(cpu)
    assert cpu["syn"]["fd"] > cpu["baseline_heldout"]["fd"] > 0.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python_with_the_message_of_the_library():
    from csl_gan_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros((65, 10), device=DEV, dtype=torch.uint8)
    buf = torch.zeros(10 * 128 + 64, device=DEV, dtype=torch.int8)
    xt = buf[:10 * 128].view(10, 128)
    S2 = torch.zeros((10, 10), device=DEV, dtype=torch.int64)
    p = lambda t: t.data_ptr()
    with pytest.raises(RuntimeError, match="mom_gram_i64: null argument"):
        _lib.check(L.cslgan_mom_gram_i64(None, 10, 128, p(S2), 10, None), "mom_gram")
    with pytest.raises(RuntimeError, match="mom_transpose_u8: np=64 is not the padded width 128 of n=65"):
        _lib.check(L.cslgan_mom_transpose_u8(p(x), 65, 10, 64, p(xt), None), "mom_transpose")
    with pytest.raises(RuntimeError, match="mom_colsum_i64: np=100 must be a multiple of 64"):
        ops.mom_colsum(buf[:1000].view(10, 100), S2[0])
    with pytest.raises(RuntimeError, match="mom_transpose_u8: n=65537 must lie in 1 .. 65536"):
        _lib.check(L.cslgan_mom_transpose_u8(p(x), 65537, 10, 65600, p(xt), None), "mom_transpose")
    with pytest.raises(RuntimeError, match="need 1 .. 65536 rows"):
        ops.mom_transpose(torch.zeros((65537, 1), device=DEV, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="mom_transpose_u8: misaligned pointer"):
        ops.mom_transpose(x, out=buf[8:8 + 10 * 128].view(10, 128))
    with pytest.raises(RuntimeError, match="mom_gram_i64: misaligned pointer"):
        ops.mom_gram(buf[8:8 + 10 * 128].view(10, 128), S2)
    with pytest.raises(RuntimeError, match="out has the shape"):
        ops.mom_transpose(x, out=buf[:10 * 64].view(10, 64))
    with pytest.raises(RuntimeError, match=r"S2 \[D, ld >= D\]"):
        ops.mom_gram(xt, S2[:, :9].contiguous())
    assert not S2.any().item() and not buf.any().item()    # nothing was launched
