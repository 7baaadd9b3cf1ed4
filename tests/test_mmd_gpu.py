"""cslgan_tri_hist_u32, cslgan_mmd_kernel_u32, cslgan_mmd_partition_sums_i64 and their driver on the device against the host model of
csl_gan_amd.kernel_test.  Every comparison is integer or bit equality; every case names the kernel that ran."""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csl_gan_amd import kernel_test as KT
from csl_gan_amd import svm

DEV = "cuda:0"
N = 130                                                        # three 64-row tiles, the last of 2 rows; three K stages, the last of 2 columns
LIMB_EDGES = [0, 0x7F, 0x80, 0xFF, 0x100, 0xFFFF, 0x10000, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF]


def _last_kernel():
    from csl_gan_amd import _lib
    return _lib.lib().cslgan_last_kernel().decode()


def _dev_matrix(a, pad):
    """uint32 [n, n] on the device in the layout of ops.gram_d2: int32 [n, gram_pitch(n)], the padding columns holding `pad`."""
    from csl_gan_amd import ops
    n = len(a)
    full = np.full((n, ops.gram_pitch(n)), pad, dtype=np.uint32)
    full[:, :n] = a
    return torch.from_numpy(full.view(np.int32)).to(DEV)


def _host_u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:, :n]


def _asymmetric():
    """130 x 17 bytes, every row and every column distinct, bytes 0 and 255 among them (the rows of tests/test_svm_gpu.py)."""
    rng = np.random.default_rng(130)
    X = rng.integers(0, 256, (130, 17)).astype(np.uint8)
    X[0], X[129], X[64, :8] = 255, 0, 255
    return X


@functools.lru_cache(maxsize=None)
def _asymmetric_d2():
    d2, _ = svm.gram_d2_host(_asymmetric())
    d2.setflags(write=False)
    return d2


def _gram_on_device(X):
    from csl_gan_amd import ops
    xs, sq = ops.nn_prepare(torch.from_numpy(np.array(X)).to(DEV))
    return ops.gram_d2(xs, sq)


# ---- the histogram --------------------------------------------------------------------------------------------------------------------------

def _bytes(b0, b1, b2, b3):
    return (b0 << 24) | (b1 << 16) | (b2 << 8) | b3


def test_tri_hist_counts_the_upper_triangle_only():
    """Entries above the diagonal: bytes (1|2, 3|4, 5|6, 7|8).  The diagonal, the lower triangle and the padding columns hold values that
    share every prefix with them and end in bins of their own, 9, 10 and 11: reading any of them shows, and the last call says which."""
    from csl_gan_amd import ops
    rng = np.random.default_rng(81)
    pick = lambda a, b: rng.integers(0, 2, (N, N)) * (b - a) + a
    a = (pick(1, 2) << 24 | pick(3, 4) << 16 | pick(5, 6) << 8 | pick(7, 8)).astype(np.uint32)
    a[0, 1] = a[0, N - 1] = a[N - 2, N - 1] = _bytes(1, 3, 5, 7)                        # the corners of the triangle are in the prefix's bin
    low = np.tril_indices(N, -1)
    a[low] = _bytes(1, 3, 5, 10)
    a[np.arange(N), np.arange(N)] = _bytes(1, 3, 5, 9)
    d2 = _dev_matrix(a, _bytes(1, 3, 5, 11))
    prefix = _bytes(1, 3, 5, 0)
    for pb in (0, 8, 16, 24):
        want = KT.tri_hist_host(a, N, prefix, pb)
        got = ops.tri_hist(d2, prefix, pb)
        assert _last_kernel() == "tri_hist_u32_kernel"
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), pb
        assert want.sum() > 0 and (pb or want.sum() == N * (N - 1) // 2)
    assert got.cpu().numpy()[9:12].tolist() == [0, 0, 0] and got.cpu().numpy()[7] > 0
    again = ops.tri_hist(d2, prefix, 24, hist=got)                                      # adds to what the caller passes
    assert again.data_ptr() == got.data_ptr() and np.array_equal(again.cpu().numpy(), 2 * want)


def test_tri_hist_of_a_single_pair_and_the_select():
    from csl_gan_amd import ops
    a = np.array([[5, 0xC0FFEE42], [7, 9]], dtype=np.uint32)
    d2 = _dev_matrix(a, 0xC0FFEE42)
    for pb, prefix, v in ((0, 0, 0xC0), (8, 0xC0000000, 0xFF), (16, 0xC0FF0000, 0xEE), (24, 0xC0FFEE00, 0x42)):
        want = np.zeros(256, dtype=np.int64)
        want[v] = 1
        assert np.array_equal(ops.tri_hist(d2, prefix, pb).cpu().numpy(), want)
        assert not ops.tri_hist(d2, prefix ^ 0x80000000, pb).any().item() or pb == 0
    assert KT.median_d2(d2, 2, DEV) == 0xC0FFEE42
    # the four-call select on the distances of real bytes
    dev = _gram_on_device(_asymmetric())
    want = KT.median_d2(_asymmetric_d2(), N)
    assert KT.median_d2(dev, N, DEV) == want == int(np.sort(_asymmetric_d2()[np.triu_indices(N, 1)])[KT.median_rank(N)])
    assert _last_kernel() == "tri_hist_u32_kernel"


# ---- the kernel matrix ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 7])
def test_kernel_matrix_is_the_host_model_bit_for_bit(B):
    """d2 over the whole uint32 range with 0 off the diagonal, both sides of the table split (65535, 65536) and 2^32 - 1; two entries of
    lo are replaced by (k + 1/2) / 2^28 under hi[0] = 1, so that 2^28 hi lo is 2.5 and 3.5 exactly: half-even gives 2 and 4."""
    from csl_gan_amd import ops
    rng = np.random.default_rng(90 + B)
    a = rng.integers(0, 2 ** 32, (N, N), dtype=np.int64).astype(np.uint32)
    a[:, ::3] = rng.integers(0, 200000, (N, (N + 2) // 3))                              # a third in the range where the kernels are not zero
    a[0, 1], a[1, 0], a[2, 129], a[129, 3], a[64, 63], a[5, 5] = 0, 0, 65535, 65536, 0xFFFFFFFF, 12345
    a[7, 8], a[8, 7], a[128, 64] = 777, 778, 777
    scales = [0.25, 1.0, 4.0, 0.5, 2.0, 8.0, 16.0][:B]
    hi, lo = KT.kernel_tables(40000, scales)
    assert (hi[:, 0] == 1.0).all()
    lo[:, 777], lo[:, 778] = 2.5 / 2 ** 28, 3.5 / 2 ** 28
    want = KT.kernel_matrix_host(a, N, hi, lo)
    assert want[7, 8] == 2 * B and want[8, 7] == 4 * B and want[0, 1] == B * 2 ** 28 and want[5, 5] == 0 and want.max() < 2 ** 31
    d2 = _dev_matrix(a, 0xFFFFFFFF)
    got = ops.mmd_kernel(d2, torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV))
    assert _last_kernel() == "mmd_kernel_u32_kernel" and got.data_ptr() == d2.data_ptr()
    assert np.array_equal(_host_u32(got, N), want)


def test_kernel_matrix_of_real_distances():
    from csl_gan_amd import ops
    d2 = _asymmetric_d2()
    hi, lo = KT.kernel_tables(KT.median_d2(d2, N), KT.DEFAULT_SCALES)
    want = KT.kernel_matrix_host(d2, N, hi, lo)
    dev = _gram_on_device(_asymmetric())
    assert _last_kernel() == "gram_d2_u8_kernel" and np.array_equal(_host_u32(dev, N), d2)
    got = _host_u32(ops.mmd_kernel(dev, torch.from_numpy(hi).to(DEV), torch.from_numpy(lo).to(DEV)), N)
    assert _last_kernel() == "mmd_kernel_u32_kernel"
    assert np.array_equal(got, want) and not np.diag(got).any() and np.array_equal(got, got.T) and got.max() > 2 ** 28


# ---- the partition sums -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _limb_matrix():
    """An asymmetric uint32 matrix below 2^31 with an entry on every limb boundary, each in a row and a column of its own, in all three
    row tiles and all three K stages, the diagonal not zero.  Read-only."""
    rng = np.random.default_rng(17)
    a = rng.integers(0, 2 ** 31, (N, N), dtype=np.int64).astype(np.uint32)
    rows = [1, 63, 64, 127, 128, 129, 30, 70, 100, 5]
    cols = [129, 128, 127, 64, 63, 0, 65, 31, 2, 5]
    for v, i, j in zip(LIMB_EDGES, rows, cols):
        a[i, j] = v
    assert len(set(rows)) == len(set(cols)) == len(LIMB_EDGES) and not np.array_equal(a, a.T)
    a.setflags(write=False)
    return a


def _members(P, n, seed):
    ld = KT.padded_cols(n)
    m = np.zeros((P, ld), dtype=np.int8)
    m[:, :n] = np.random.default_rng(seed).integers(0, 2, (P, n))
    m[0, :n] = 1                                                                          # all ones: sxx2 is the total, sxy nothing
    if P > 2:
        m[1] = 0                                                                          # nobody: both sums are zero
        m[2] = 0
        m[2, n - 1] = 1                                                                   # one member, in the last K stage and row tile
    return m


@pytest.mark.parametrize("P", [1, 33, 130])
def test_partition_sums_on_every_limb_boundary(P):
    from csl_gan_amd import ops
    a = _limb_matrix()
    member = _members(P, N, P)
    xx, xy = KT.partition_sums_host(a, member)
    assert int(xx[0]) == int(a.astype(np.int64).sum()) and xy[0] == 0
    wrong = KT.partition_sums_host(np.ascontiguousarray(a.T), member)                    # what a transposed operand would give
    if P > 2:
        assert (xx[1], xy[1]) == (0, 0) and int(xx[2]) == int(a[N - 1, N - 1]) and int(xy[2]) == int(a[:N - 1, N - 1].astype(np.int64).sum())
        assert not np.array_equal(wrong[1], xy)
    kq = _dev_matrix(a, 0xFFFFFFFF)                                                       # the padding columns must not be read as entries
    front = 3                                                                             # canaries around both outputs
    buf = torch.full((2, P + 2 * front), -77, device=DEV, dtype=torch.int64)
    sxx2, sxy = buf[0, front:front + P], buf[1, front:front + P]
    sxx2.zero_()
    sxy.zero_()
    got = ops.mmd_partition_sums(kq, torch.from_numpy(member).to(DEV), sxx2, sxy)
    assert _last_kernel() == "mmd_partition_sums_i64_kernel" and got[0].data_ptr() == sxx2.data_ptr()
    assert np.array_equal(sxx2.cpu().numpy(), xx) and np.array_equal(sxy.cpu().numpy(), xy)
    ops.mmd_partition_sums(kq, torch.from_numpy(member).to(DEV), sxx2, sxy)               # a second call adds
    host = buf.cpu().numpy()
    assert np.array_equal(host[0, front:front + P], 2 * xx) and np.array_equal(host[1, front:front + P], 2 * xy)
    assert (host[:, :front] == -77).all() and (host[:, front + P:] == -77).all()
    fresh = ops.mmd_partition_sums(kq, torch.from_numpy(member).to(DEV))                  # allocated by the wrapper
    assert np.array_equal(fresh[0].cpu().numpy(), xx) and np.array_equal(fresh[1].cpu().numpy(), xy)


def test_partition_sums_past_32_bits():
    """Every entry 2^31 - 1, 520 rows: r = 520 (2^31 - 1) > 2^40 per row, the total 520^2 (2^31 - 1) > 2^49."""
    from csl_gan_amd import ops
    n = 520
    a = np.full((n, n), 0x7FFFFFFF, dtype=np.uint32)
    member = _members(4, n, 3)
    xx, xy = KT.partition_sums_host(a, member)
    cnt = member[:, :n].astype(np.int64).sum(1)
    assert xx.tolist() == [int(c) * int(c) * 0x7FFFFFFF for c in cnt] and xy.tolist() == [int(c) * (n - int(c)) * 0x7FFFFFFF for c in cnt]
    assert xx[0] == n * n * 0x7FFFFFFF > 2 ** 49
    got = ops.mmd_partition_sums(_dev_matrix(a, 0), torch.from_numpy(member).to(DEV))
    assert _last_kernel() == "mmd_partition_sums_i64_kernel"
    assert np.array_equal(got[0].cpu().numpy(), xx) and np.array_equal(got[1].cpu().numpy(), xy)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------

def test_run_on_the_device_equals_the_cpu():
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (130, 17)).astype(np.uint8)
    Y = rng.integers(64, 192, (70, 17)).astype(np.uint8)
    cpu, cv = KT.mmd_rows(X, Y, n_perms=199, seed=0)
    dev, dv = KT.mmd_rows(X, Y, n_perms=199, seed=0, device=DEV, chunk=64)
    assert dev == cpu and dv["T"] == cv["T"] and dv["tot2"] == cv["tot2"] and dv["median_d2"] == cv["median_d2"]
    assert np.array_equal(dv["sxx2"], cv["sxx2"]) and np.array_equal(dv["sxy"], cv["sxy"])
    assert cpu["n_ge"] == 0 and cpu["p_value"] == 1 / 200
    A, B = rng.integers(0, 256, (64, 48)).astype(np.uint8), rng.integers(0, 256, (64, 48)).astype(np.uint8)     # balanced, one K stage
    cpu, cv = KT.mmd_rows(A, B, n_perms=99, seed=2)
    dev, dv = KT.mmd_rows(A, B, n_perms=99, seed=2, device=DEV)
    assert dev == cpu and dv["T"] == cv["T"]


HWC = (4, 4, 3)


def test_cli_on_the_device_writes_the_json_of_the_cpu(tmp_path):
    from csl_gan_amd import mmd
    from csl_gan_amd.generate import CacheWriter
    rng = np.random.default_rng(31)
    for name, n, lo, hi in (("train", 150, 0, 256), ("heldout", 90, 0, 256), ("syn", 70, 64, 192)):
        w = CacheWriter(str(tmp_path / name), n, *HWC, True, {"note": "test rows"})
        w(0, rng.integers(lo, hi, (n,) + HWC, dtype=np.uint8), np.zeros(n, dtype=np.int64))
        w.close()
    out = {}
    for name, dev in (("cpu", "cpu"), ("dev", DEV)):
        mmd.main(["--syn_cache", str(tmp_path / "syn"), "--train_cache", str(tmp_path / "train"), "--nontrain_cache", str(tmp_path / "heldout"),
                  "--baseline", "--n_perms", "99", "-d", dev, "--save", "--outputs_dir", str(tmp_path / name), "--values_dir", str(tmp_path / name)])
        with open(str(tmp_path / name / "mmd.json")) as f:
            out[name] = f.read()
        out[name + "_T"] = np.load(str(tmp_path / name / "syn_T.npy")).tolist()
    assert out["dev"] == out["cpu"] and out["dev_T"] == out["cpu_T"]
    stats = json.loads(out["cpu"])
    assert set(stats) == {"syn", "baseline_heldout"} and stats["syn"]["p_value"] == 1 / 100 and stats["syn"]["n_real"] == 70


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python_with_the_message_of_the_library():
    from csl_gan_amd import ops
    d2 = torch.zeros((130, 160), device=DEV, dtype=torch.int32)
    tab = torch.ones((8, 65536), device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="tri_hist_u32: prefix_bits=4 must be 0, 8, 16 or 24"):
        ops.tri_hist(d2, 0, 4)
    with pytest.raises(RuntimeError, match="mmd_kernel_u32: B=8 bandwidths"):
        ops.mmd_kernel(d2, tab, tab)
    with pytest.raises(RuntimeError, match="mmd_partition_sums_i64: ldm=160 must be a multiple of 64"):
        ops.mmd_partition_sums(d2, torch.ones((3, 160), device=DEV, dtype=torch.int8))
    with pytest.raises(RuntimeError, match=r"need member \[P, ldm >= n = 130\]"):
        ops.mmd_partition_sums(d2, torch.ones((3, 128), device=DEV, dtype=torch.int8))
    with pytest.raises(RuntimeError, match="need the matrix of gram_d2"):
        ops.tri_hist(torch.zeros((130, 192), device=DEV, dtype=torch.int32))
    assert not d2.any().item()                                                            # nothing was launched
