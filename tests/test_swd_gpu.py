"""cslgan_swd_directions_i8, cslgan_swd_project_i8, cslgan_sort_rows_i32, cslgan_swd_w1_i64 and their driver on the device against the host
models of csl_gan_amd.sliced and np.sort.  Every comparison is integer equality."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csl_gan_amd import sliced as SL

DEV = "cuda:0"
SENTINEL = -123456789
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared cases are read-only


# ---- directions ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,D", [(3, 200), (130, 784), (2, 65536)])
def test_directions_equal_the_host_stream_and_the_padding_is_zero(P, D):
    from csl_gan_amd import ops
    Dp = ops.nn_padded_dim(D)
    out = torch.full((P, Dp), 77, device=DEV, dtype=torch.int8)
    got = ops.swd_directions(P, D, 12345, DEV, out=out).cpu().numpy()
    assert got.shape == (P, Dp) and np.array_equal(got[:, :D], SL.directions_host(P, D, 12345))
    assert not got[:, D:].any()
    assert not np.array_equal(ops.swd_directions(P, D, 12346, DEV).cpu().numpy(), got)


# ---- projection -----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _proj_case(P, n, D):
    """Asymmetric data: every row and every column differs; rows of all 0 and all 255 among them, and two rows that follow the signs of
    direction 0 and their opposites, whose projections on it are the extremes.  (x, dirs [P, D], want [P, n])."""
    rng = np.random.default_rng(3 * P + 5 * n + 7 * D)
    x = rng.integers(0, 256, (n, D), dtype=np.uint8)
    s = SL.directions_host(P, D, 9)
    x[0] = 0
    x[n - 1] = 255
    if n > 4:
        x[n // 2, : D // 2] = 255                          # half a row high: the two K halves are not alike
        x[1], x[2] = np.where(s[0] > 0, 255, 0), np.where(s[0] > 0, 0, 255)
    want = SL.project_host(s, x)
    for a in (x, s, want):
        a.setflags(write=False)
    return x, s, want


def _project(x, P, D, Y, col0=0, seed=9):
    from csl_gan_amd import ops
    xs, _ = ops.nn_prepare(_dev(x))
    return ops.swd_project(ops.swd_directions(P, D, seed, DEV), xs, Y, col0)


@pytest.mark.parametrize("P,n,D", [(1, 1, 1), (130, 257, 100), (256, 1000, 12288), (130, 257, 65536)])
def test_projection_equals_the_host_model(P, n, D):
    x, s, want = _proj_case(P, n, D)
    Y = torch.full((P, n), SENTINEL, device=DEV, dtype=torch.int32)
    got = _project(x, P, D, Y).cpu().numpy()
    assert np.array_equal(got, want)
    if D == 65536:                                         # a row of zeros gives -128 sum_j s[j]; the rows along direction 0 give +-2^23 nearly
        assert np.array_equal(got[:, 0], -128 * s.astype(np.int64).sum(1))
        assert got[0, 1] >= 127 * D and got[0, 2] <= -127 * D and got[0, 1] - got[0, 2] == 255 * D


def test_projection_writes_its_columns_only_and_two_calls_equal_one():
    P, n, D = 130, 257, 100
    x, s, want = _proj_case(P, n, D)
    Y = torch.full((P + 6, 1024), SENTINEL, device=DEV, dtype=torch.int32)
    _project(x, P, D, Y[:P], col0=300)
    got = Y.cpu().numpy()
    assert np.array_equal(got[:P, 300:300 + n], want)
    assert (got[:P, :300] == SENTINEL).all() and (got[:P, 300 + n:] == SENTINEL).all() and (got[P:] == SENTINEL).all()
    Z = torch.full((P, n), SENTINEL, device=DEV, dtype=torch.int32)
    _project(x[:129], P, D, Z, col0=0)
    _project(x[129:], P, D, Z, col0=129)
    assert np.array_equal(Z.cpu().numpy(), want)


# ---- the sort ---------------------------------------------------------------------------------------------------------------------------------------

def _variants(P, n, rng):
    full = rng.integers(I32_MIN, I32_MAX, (P, n), endpoint=True, dtype=np.int64)
    full[:, 0], full[:, -1] = I32_MIN, I32_MAX
    inc = np.sort(full, axis=1)
    yield "full range", full, 32
    yield "all equal", np.full((P, n), -7, dtype=np.int64), 32
    yield "sorted", inc, 32
    yield "reversed", inc[:, ::-1], 32
    yield "two values", np.where(rng.integers(0, 2, (P, n)) == 1, 5, -3), 32
    small = rng.integers(-2 ** 23, 2 ** 23, (P, n), endpoint=True, dtype=np.int64)
    small[:, 0], small[:, -1] = -2 ** 23, 2 ** 23
    yield "25 bits", small, 25
    yield "8 bits", rng.integers(-128, 128, (P, n), dtype=np.int64), 8                  # one pass: the result comes back from the workspace


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097, 70001])
def test_sort_equals_numpy_and_leaves_what_lies_behind_n(n):
    from csl_gan_amd import ops
    P, ld = 3, n + 5
    rng = np.random.default_rng(n)
    for name, data, bits in _variants(P, n, rng):
        x = np.full((P, ld), SENTINEL, dtype=np.int32)
        x[:, :n] = data
        t = _dev(x)
        ops.sort_rows(t, n, key_bits=bits)
        got = t.cpu().numpy()
        assert np.array_equal(got[:, :n], np.sort(x[:, :n], axis=1)), name
        assert (got[:, n:] == SENTINEL).all(), name


def test_sort_of_many_rows_at_once():
    from csl_gan_amd import ops
    rng = np.random.default_rng(1)
    x = rng.integers(I32_MIN, I32_MAX, (1024, 1000), endpoint=True, dtype=np.int64).astype(np.int32)
    x[5] = x[5, 0]
    ws = torch.empty(ops.sort_rows_ws_bytes(1024, 1000) + 64, device=DEV, dtype=torch.uint8)
    assert np.array_equal(ops.sort_rows(_dev(x), ws=ws).cpu().numpy(), np.sort(x, axis=1))
    with pytest.raises(RuntimeError, match="ws has"):
        ops.sort_rows(_dev(x), ws=ws[:1000])


def test_sort_of_one_row_past_two_to_the_24():
    """4097 tiles of one row: the scan's walk along the tiles and destination indices above 2^24."""
    from csl_gan_amd import ops
    n = 2 ** 24 + 3
    x = np.random.default_rng(2).integers(-2 ** 23, 2 ** 23, (1, n), endpoint=True, dtype=np.int64).astype(np.int32)
    assert np.array_equal(ops.sort_rows(_dev(x), key_bits=25).cpu().numpy(), np.sort(x, axis=1))


# ---- the numerators -----------------------------------------------------------------------------------------------------------------------------------

def _w1_case(na, nb, P, scale):
    rng = np.random.default_rng(na + 3 * nb + P)
    a = np.sort(rng.integers(-9, 10, (P, na)) * scale, axis=1).astype(np.int32)         # few values: ties inside and between the sets
    b = np.sort(rng.integers(-7, 12, (P, nb)) * scale, axis=1).astype(np.int32)
    return a, b


@pytest.mark.parametrize("na,nb", [(1, 1), (5, 3), (3, 5), (1, 257), (1000, 1000), (4097, 1000)])
def test_numerators_equal_the_host_model(na, nb):
    from csl_gan_amd import ops
    a, b = _w1_case(na, nb, 130, 1)
    want = SL.w1_numerators_host(a, b)
    pa, pb = np.full((130, na + 3), SENTINEL, dtype=np.int32), np.full((130, nb + 1), SENTINEL, dtype=np.int32)
    pa[:, :na], pb[:, :nb] = a, b
    got = ops.swd_w1(_dev(pa), na, _dev(pb), nb)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.swd_w1(_dev(pb), nb, _dev(pa), na).cpu().numpy(), want)    # symmetric


def test_numerators_at_the_extremes_need_their_int64_products():
    from csl_gan_amd import ops
    n = 4097
    a, b = np.full((4, n), -2 ** 23, dtype=np.int32), np.full((4, n), 2 ** 23, dtype=np.int32)
    a[1], b[1] = _w1_case(n, n, 1, 2 ** 23 // 11)
    a[2, n // 2:] = 2 ** 23
    want = SL.w1_numerators_host(a, b)
    assert want[0] == 2 ** 24 * n * n and want[0] > 2 ** 47
    assert np.array_equal(ops.swd_w1(_dev(a), n, _dev(b), n).cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="overflows"):
        ops.swd_w1(torch.empty((1, 2 ** 19), device=DEV, dtype=torch.int32), 2 ** 19, torch.empty((1, 2 ** 19), device=DEV, dtype=torch.int32),
                   2 ** 19)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------

HWC = (8, 8, 3)


def _run(tmp_path, name, extra):
    from csl_gan_amd import swd
    vals = str(tmp_path / name)
    stats = swd.main(["--syn_cache", str(tmp_path / "syn"), "--train_cache", str(tmp_path / "train"), "--nontrain_cache", str(tmp_path / "heldout"),
                      "--baseline", "--per_class", "--n_dirs", "96", "--seed", "5", "--values_dir", vals] + extra)
    return stats, {f: np.load(os.path.join(vals, f)) for f in sorted(os.listdir(vals))}


def test_cli_on_the_device_equals_the_cpu_whatever_the_blocking(tmp_path):
    from csl_gan_amd.generate import CacheWriter
    rng = np.random.default_rng(31)
    for name, n, hi, classes in (("train", 300, 256, 3), ("heldout", 257, 256, 3), ("syn", 130, 200, 4)):
        w = CacheWriter(str(tmp_path / name), n, *HWC, True, {"note": "test rows"})
        w(0, rng.integers(0, hi, (n,) + HWC, dtype=np.uint8), np.arange(n, dtype=np.int64) % classes)
        w.close()
    cpu, cpu_vals = _run(tmp_path, "cpu", ["-d", "cpu"])
    dev, dev_vals = _run(tmp_path, "dev", ["-d", DEV])
    blk, blk_vals = _run(tmp_path, "blk", ["-d", DEV, "--block_rows", "128", "--resident_gb", "0.0001"])     # 12 directions per block
    assert SL._dir_block(96, 130, 300, 0.0001) < 96 // 4
    assert set(cpu) == {"syn", "baseline_heldout"} and list(cpu["syn"]["per_class"]) == ["0", "1", "2"]
    assert "syn_num.npy" in cpu_vals and "baseline_heldout_num_class2.npy" in cpu_vals and len(cpu_vals) == 8
    for vals in (dev_vals, blk_vals):
        assert list(vals) == list(cpu_vals)
        for f, v in vals.items():
            assert v.dtype == np.int64 and v.shape == (96,) and np.array_equal(v, cpu_vals[f]), f
    assert json.dumps(dev) == json.dumps(cpu) and json.dumps(blk) == json.dumps(cpu)
    assert cpu["syn"]["swd"] > cpu["baseline_heldout"]["swd"] > 0.0
