"""The kernel two-sample test on the CPU: the host model of csl_gan_amd.kernel_test against a brute force in fractions, numpy's sort and
the partitions themselves, the command on `-d cpu`, its refusals and the argument checks of the new entries.  Every comparison is integer
or bit equality."""
import functools
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from csl_gan_amd import audit
from csl_gan_amd import kernel_test as KT
from csl_gan_amd import svm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["cslgan_tri_hist_u32", "cslgan_mmd_kernel_u32", "cslgan_mmd_partition_sums_i64"]


def _rows(n, D, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (n, D)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _clear_case():
    """The pool of a clear difference: 130 rows over the whole byte range against 70 rows of its middle half, 199 relabellings."""
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (130, 17)).astype(np.uint8)
    Y = rng.integers(64, 192, (70, 17)).astype(np.uint8)
    fig, vals = KT.mmd_rows(X, Y, n_perms=199, seed=0)
    for a in (X, Y, vals["sxx2"], vals["sxy"]):
        a.setflags(write=False)
    return X, Y, fig, vals


# ---- the statistic ----------------------------------------------------------------------------------------------------------------------------

def test_statistic_equals_a_brute_force_in_fractions():
    n, m = 9, 7
    X, Y = _rows(n, 5, 1), _rows(m, 5, 2, hi=200)
    scales = (0.5, 2.0)
    fig, vals = KT.mmd_rows(X, Y, n_perms=3, scales=scales, seed=11)
    Z = np.concatenate([X, Y])
    d2, _ = svm.gram_d2_host(Z)
    med = KT.median_d2(d2, n + m)
    assert vals["median_d2"] == med == sorted(int(d2[i, j]) for i in range(n + m) for j in range(i + 1, n + m))[KT.median_rank(n + m)]
    hi, lo = KT.kernel_tables(med, scales)
    kq = KT.kernel_matrix_host(d2, n + m, hi, lo)
    assert kq.dtype == np.uint32 and not np.diag(kq).any() and np.array_equal(kq, kq.T)
    for i, j in ((0, 1), (3, 12), (15, 8)):                    # the definition, entry by entry
        v = int(d2[i, j])
        assert int(kq[i, j]) == sum(int(np.rint(2.0 ** 28 * (hi[b][v >> 16] * lo[b][v & 65535]))) for b in range(2))
        assert hi[0][1] == np.exp(-65536.0 / (2.0 * med * 0.5)) and lo[1][v & 65535] == np.exp(-float(v & 65535) / (2.0 * med * 2.0))
    k = [[Fraction(int(kq[i, j]), 2 ** 28 * len(scales)) for j in range(n + m)] for i in range(n + m)]

    def brute(first):
        """The unbiased MMD^2 with the rows `first` as one sample and the rest as the other."""
        rest = [i for i in range(n + m) if i not in first]
        xx = sum(k[i][j] for i in first for j in first if i != j) / (len(first) * (len(first) - 1))
        yy = sum(k[i][j] for i in rest for j in rest if i != j) / (len(rest) * (len(rest) - 1))
        xy = sum(k[i][j] for i in first for j in rest) / (len(first) * len(rest))
        return xx + yy - 2 * xy

    den = 2 ** 28 * len(scales) * n * (n - 1) * m * (m - 1)
    assert all(isinstance(t, int) for t in vals["T"]) and len(vals["T"]) == 4
    assert Fraction(vals["T"][0], den) == brute(list(range(n)))
    for p in (1, 2, 3):
        assert Fraction(vals["T"][p], den) == brute(sorted(audit.subset_indices(11, p, 0, n + m, n).tolist()))
    assert fig["mmd2"] == vals["T"][0] / den and fig["n_perms"] == 3 and (fig["n_syn"], fig["n_real"]) == (n, m)
    assert vals["tot2"] == int(kq.astype(np.int64).sum())
    assert fig["p_value"] == (1 + fig["n_ge"]) / 4 and fig["n_ge"] == sum(t >= vals["T"][0] for t in vals["T"][1:])


@pytest.mark.parametrize("N", [2, 3, 130])
def test_median_equals_the_sorted_triangle_at_the_stated_rank(N):
    Z = _rows(N, 17, 40 + N)
    d2, _ = svm.gram_d2_host(Z)
    tri = np.sort(d2[np.triu_indices(N, 1)])
    rank = (N * (N - 1) // 2 - 1) // 2
    assert KT.median_rank(N) == rank
    got = KT.median_d2(d2, N)
    assert isinstance(got, int) and got == int(tri[rank])
    pad = np.full((N + 3, N + 5), 0xFFFFFFFF, dtype=np.uint32)                         # rows and columns behind n are not counted
    pad[:N, :N] = d2
    assert KT.median_d2(pad, N) == got
    hist = KT.tri_hist_host(d2, N)
    assert hist.dtype == np.int64 and int(hist.sum()) == N * (N - 1) // 2
    with pytest.raises(ValueError, match="prefix_bits = 4"):
        KT.tri_hist_host(d2, N, 0, 4)


def test_a_clear_difference_gives_the_smallest_p_value_and_none_a_large_one():
    X, Y, fig, vals = _clear_case()
    assert fig["n_ge"] == 0 and fig["n_eq"] == 0 and fig["p_value"] == 1 / 200
    assert fig["mmd2"] > 0 and fig["z_score"] > 3.0 and (fig["n_syn"], fig["n_real"], fig["n_perms"]) == (130, 70, 199)
    same, _ = KT.mmd_rows(X, _rows(70, 17, 6), n_perms=199, seed=0)
    print("same range: n_ge %d, p %.4f" % (same["n_ge"], same["p_value"]))
    assert same["p_value"] > 0.05


def test_exact_ties_of_a_tiny_balanced_pool_are_counted():
    """n = m = 4: a relabelling that is the identity or its complement has T[p] = T[0] exactly, and no other has."""
    X, Y = _rows(4, 6, 21), _rows(4, 6, 22, hi=128)
    P, seed = 199, 3
    fig, vals = KT.mmd_rows(X, Y, n_perms=P, seed=seed)
    member = KT.partitions(seed, 0, P + 1, 8, 4)[:, :8]
    assert member.sum(1).tolist() == [4] * (P + 1) and member[0].tolist() == [1] * 4 + [0] * 4
    same = [bool((member[p] == member[0]).all() or (member[p] == 1 - member[0]).all()) for p in range(1, P + 1)]
    assert 0 < sum(same) < P
    assert fig["n_eq"] == sum(same)
    assert [t == vals["T"][0] for t in vals["T"][1:]] == same
    assert fig["n_ge"] >= fig["n_eq"] and fig["p_value"] == (1 + fig["n_ge"]) / (P + 1)


def test_the_result_does_not_depend_on_the_chunk():
    X, Y, fig, vals = _clear_case()
    for chunk in (7, 200):
        f, v = KT.mmd_rows(X, Y, n_perms=199, seed=0, chunk=chunk)
        assert f == fig and v["T"] == vals["T"] and np.array_equal(v["sxx2"], vals["sxx2"]) and np.array_equal(v["sxy"], vals["sxy"])
    f1, v1 = KT.mmd_rows(X, Y, n_perms=12, seed=0, chunk=1)                              # a prefix of the same stream
    assert v1["T"] == vals["T"][:13] and f1["mmd2"] == fig["mmd2"]
    m = KT.partitions(0, 0, 200, 200, 130)
    assert m.shape == (200, 256) and m.dtype == np.int8 and not m[:, 200:].any()
    assert np.array_equal(m[5:12], KT.partitions(0, 5, 7, 200, 130))
    assert np.array_equal(np.nonzero(m[9, :200])[0], np.sort(audit.subset_indices(0, 9, 0, 200, 130)))


def test_partition_sums_host_on_an_asymmetric_matrix():
    rng = np.random.default_rng(8)
    kq = rng.integers(0, 2 ** 31, (11, 11), dtype=np.int64).astype(np.uint32)
    member = (rng.random((5, 64)) < 0.5).astype(np.int8)
    member[:, 11:] = 0
    xx, xy = KT.partition_sums_host(kq, member)
    K = [[int(v) for v in row] for row in kq]
    for p in range(5):
        r = [sum(K[i][j] for j in range(11) if member[p, j]) for i in range(11)]
        assert int(xx[p]) == sum(r[i] for i in range(11) if member[p, i]) and int(xy[p]) == sum(r[i] for i in range(11) if not member[p, i])


def test_sizes_and_bandwidths_are_refused():
    with pytest.raises(ValueError, match=r"a pool of 65530 \+ 7 = 65537 rows: the stored matrix takes at most 65536"):
        KT.check_sizes(65530, 7)
    with pytest.raises(ValueError, match="at least 2 of each"):
        KT.check_sizes(1, 5)
    with pytest.raises(ValueError, match="median squared distance is 0"):
        KT.kernel_tables(0)
    with pytest.raises(ValueError, match="1 .. 7 finite scales"):
        KT.kernel_tables(5, [1.0] * 8)
    with pytest.raises(ValueError, match="median squared distance is 0"):
        KT.mmd_rows(np.zeros((5, 3), dtype=np.uint8), np.zeros((4, 3), dtype=np.uint8), n_perms=3)


# ---- the command line on the CPU --------------------------------------------------------------------------------------------------------------

HWC = (3, 2, 2)


def _write(path, x):
    from csl_gan_amd.generate import CacheWriter
    n, H, W, C = x.shape
    w = CacheWriter(path, n, H, W, C, True, {"note": "test rows"})
    w(0, x, np.zeros(n, dtype=np.int64))
    w.close()


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mmd")) + "/"
    rng = np.random.default_rng(7)
    x = {"train": rng.integers(0, 256, (60,) + HWC, dtype=np.uint8), "heldout": rng.integers(0, 256, (25,) + HWC, dtype=np.uint8),
         "syn": rng.integers(64, 192, (30,) + HWC, dtype=np.uint8), "syn2": rng.integers(0, 256, (70,) + HWC, dtype=np.uint8)}
    for k, v in x.items():
        _write(d + k, v)
    _write(d + "odd", rng.integers(0, 256, (9, 2, 3, 2), dtype=np.uint8))
    _write(d + "flat", np.zeros((9,) + HWC, dtype=np.uint8))
    return d, x


def test_cli_on_the_cpu(caches, tmp_path, capsys):
    from csl_gan_amd import mmd
    d, x = caches
    out, vals = str(tmp_path / "outputs"), str(tmp_path / "values")
    stats = mmd.main(["--syn_cache", d + "syn", d + "syn2", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "--baseline",
                      "-d", "cpu", "--n_perms", "49", "--seed", "4", "--values_dir", vals, "--save", "--outputs_dir", out, "--name", "q"])
    assert list(stats) == ["syn", "syn2", "baseline_heldout"]
    printed = capsys.readouterr().out
    for lab, n, m in (("syn", 30, 30), ("syn2", 70, 60), ("baseline_heldout", 25, 25)):
        f = stats[lab]
        rows = x["heldout" if lab.startswith("baseline") else lab].reshape(n, -1)
        real = x["train"].reshape(60, -1)
        real = real if m == 60 else real[audit.subset_indices(4, 0, 1, 60, m)]
        want, wv = KT.mmd_rows(rows, real, n_perms=49, seed=4)
        assert f == want and (f["n_syn"], f["n_real"], f["n_perms"], f["seed"]) == (n, m, 49, 4)
        T = np.load(os.path.join(vals, lab + "_T.npy"))
        assert [int(t) for t in T] == wv["T"]
        for key in ("sxx2", "sxy"):
            got = np.load(os.path.join(vals, "%s_%s.npy" % (lab, key)))
            assert got.dtype == np.int64 and np.array_equal(got, wv[key])
        assert np.load(os.path.join(vals, lab + "_tot2.npy")).tolist() == [wv["tot2"]]
        assert ("%s: %d samples against %d images: mmd2 " % (lab, n, m)) in printed
    assert stats["syn"]["p_value"] == 1 / 50 and stats["baseline_heldout"]["p_value"] > 1 / 50
    with open(os.path.join(out, "q.json")) as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    fewer = mmd.main(["--syn_cache", d + "syn", "--train_cache", d + "train", "-d", "cpu", "--n_perms", "5", "--n_real", "12", "--scales", "1"])
    assert (fewer["syn"]["n_real"], fewer["syn"]["n_scales"], fewer["syn"]["n_perms"]) == (12, 1, 5)


def test_cli_refusals(caches, tmp_path):
    from csl_gan_amd import mmd
    d, _ = caches
    base = ["--train_cache", d + "train", "-d", "cpu", "--n_perms", "3"]
    with pytest.raises(SystemExit, match="--nontrain_cache"):
        mmd.main(["--syn_cache", d + "syn", "--baseline"] + base)
    with pytest.raises(SystemExit, match="one geometry"):
        mmd.main(["--syn_cache", d + "odd"] + base)
    with pytest.raises(SystemExit, match="median squared distance is 0"):
        mmd.main(["--syn_cache", d + "flat", "--train_cache", d + "flat", "-d", "cpu"])
    with pytest.raises(SystemExit, match="1 .. 7 finite scales"):
        mmd.main(["--syn_cache", d + "syn", "--scales"] + ["1"] * 8 + base)
    big = str(tmp_path / "big")
    _write(big, np.zeros((65535,) + HWC, dtype=np.uint8))
    with pytest.raises(SystemExit, match=r"a pool of 65535 \+ 2 = 65537 rows: the stored matrix takes at most 65536"):
        mmd.main(["--syn_cache", big, "--n_real", "2"] + base)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from csl_gan_amd import _lib, build
    build.build()
    return _lib.lib()


def test_the_entries_are_declared_and_exported_and_the_abi_version_stays(L):
    from csl_gan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cslgan.h")).read()
    assert "Kernel two-sample test" in hdr
    declared = set(re.findall(r"\b(cslgan_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name)
    assert L.cslgan_version() == 7 and _lib.ABI_VERSION == 7
    assert "mmd_kernels.hip" in __import__("csl_gan_amd.build", fromlist=["SOURCES"]).SOURCES


def test_the_entries_refuse_bad_arguments_before_any_launch(L):
    """Validation runs on the host before any launch: no device is needed.  128 stands for an aligned non-null pointer."""
    err = lambda: L.cslgan_last_error()
    ok = 128
    # the histogram
    assert L.cslgan_tri_hist_u32(None, 160, 130, 0, 0, ok, None) == -1 and b"tri_hist_u32: null" in err()
    assert L.cslgan_tri_hist_u32(ok, 160, 130, 0, 0, None, None) == -1 and b"tri_hist_u32: null" in err()
    assert L.cslgan_tri_hist_u32(ok, 160, 130, 0, 4, ok, None) == -1 and b"tri_hist_u32: prefix_bits=4 must be 0, 8, 16 or 24" in err()
    assert L.cslgan_tri_hist_u32(ok, 160, 130, 0, 32, ok, None) == -1 and b"tri_hist_u32: prefix_bits=32" in err()
    assert L.cslgan_tri_hist_u32(ok, 65568, 65537, 0, 0, ok, None) == -1 and b"tri_hist_u32: n=65537 rows; the stored matrix takes 1 .. 65536" in err()
    assert L.cslgan_tri_hist_u32(ok, 160, 0, 0, 0, ok, None) == -1 and b"tri_hist_u32: n=0" in err()
    assert L.cslgan_tri_hist_u32(ok, 150, 130, 0, 0, ok, None) == -1 and b"tri_hist_u32: pitch=150 must be a multiple of 32" in err()
    assert L.cslgan_tri_hist_u32(ok, 128, 130, 0, 0, ok, None) == -1 and b"tri_hist_u32: pitch=128" in err()
    assert L.cslgan_tri_hist_u32(64, 160, 130, 0, 0, ok, None) == -1 and b"tri_hist_u32: misaligned" in err()
    assert L.cslgan_tri_hist_u32(ok, 160, 130, 0, 0, 20, None) == -1 and b"tri_hist_u32: misaligned" in err()
    # the kernel matrix
    assert L.cslgan_mmd_kernel_u32(None, 160, 130, ok, ok, 3, None) == -1 and b"mmd_kernel_u32: null" in err()
    assert L.cslgan_mmd_kernel_u32(ok, 160, 130, None, ok, 3, None) == -1 and b"mmd_kernel_u32: null" in err()
    assert L.cslgan_mmd_kernel_u32(ok, 160, 130, ok, None, 3, None) == -1 and b"mmd_kernel_u32: null" in err()
    assert L.cslgan_mmd_kernel_u32(ok, 160, 130, ok, ok, 8, None) == -1 and b"mmd_kernel_u32: B=8 bandwidths; 1 .. 7" in err()
    assert L.cslgan_mmd_kernel_u32(ok, 160, 130, ok, ok, 0, None) == -1 and b"mmd_kernel_u32: B=0" in err()
    assert L.cslgan_mmd_kernel_u32(ok, 65568, 65537, ok, ok, 3, None) == -1 and b"mmd_kernel_u32: n=65537" in err()
    assert L.cslgan_mmd_kernel_u32(ok, 150, 130, ok, ok, 3, None) == -1 and b"mmd_kernel_u32: pitch=150 must be a multiple of 32" in err()
    assert L.cslgan_mmd_kernel_u32(64, 160, 130, ok, ok, 3, None) == -1 and b"mmd_kernel_u32: misaligned" in err()
    assert L.cslgan_mmd_kernel_u32(ok, 160, 130, 20, ok, 3, None) == -1 and b"mmd_kernel_u32: misaligned" in err()
    # the partition sums
    for args in ((None, 160, 130, ok, 192, 5, ok, ok), (ok, 160, 130, None, 192, 5, ok, ok), (ok, 160, 130, ok, 192, 5, None, ok),
                 (ok, 160, 130, ok, 192, 5, ok, None)):
        assert L.cslgan_mmd_partition_sums_i64(*args, None) == -1 and b"mmd_partition_sums_i64: null" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 65568, 65537, ok, 65600, 5, ok, ok, None) == -1 and b"mmd_partition_sums_i64: n=65537" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 150, 130, ok, 192, 5, ok, ok, None) == -1 and b"mmd_partition_sums_i64: pitch=150" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 160, 130, ok, 128, 5, ok, ok, None) == -1 and b"mmd_partition_sums_i64: ldm=128 must be a multiple of 64 in n" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 160, 130, ok, 160, 5, ok, ok, None) == -1 and b"mmd_partition_sums_i64: ldm=160 must be a multiple of 64" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 160, 130, ok, 192, 0, ok, ok, None) == -1 and b"mmd_partition_sums_i64: P=0" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 160, 130, ok, 192, 2 ** 20 + 1, ok, ok, None) == -1 and b"mmd_partition_sums_i64: P=1048577" in err()
    assert L.cslgan_mmd_partition_sums_i64(64, 160, 130, ok, 192, 5, ok, ok, None) == -1 and b"mmd_partition_sums_i64: misaligned" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 160, 130, 8, 192, 5, ok, ok, None) == -1 and b"mmd_partition_sums_i64: misaligned" in err()
    assert L.cslgan_mmd_partition_sums_i64(ok, 160, 130, ok, 192, 5, 20, ok, None) == -1 and b"mmd_partition_sums_i64: misaligned" in err()


def test_ops_refuse_cpu_tensors_and_wrong_types(L):
    import torch
    from csl_gan_amd import ops
    d2 = torch.zeros(130, 160, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.tri_hist(d2)
    with pytest.raises(RuntimeError, match="d2 must be a contiguous int32"):
        ops.tri_hist(d2.to(torch.int64))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mmd_kernel(d2, torch.zeros(3, 65536, dtype=torch.float64), torch.zeros(3, 65536, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="hi must be a contiguous float64"):
        ops.mmd_kernel(d2, torch.zeros(3, 65536), torch.zeros(3, 65536, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mmd_partition_sums(d2, torch.zeros(5, 192, dtype=torch.int8))
    with pytest.raises(RuntimeError, match="member must be a contiguous int8"):
        ops.mmd_partition_sums(d2, torch.zeros(5, 192, dtype=torch.uint8))
    assert ops.mmd_padded_cols(1) == 64 and ops.mmd_padded_cols(64) == 64 and ops.mmd_padded_cols(130) == 192
