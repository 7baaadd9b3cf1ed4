"""The Fréchet distance of cache bytes on the CPU: the integer moments of csl_gan_amd.moments against direct int64 and Python-int sums,
the float step against mpmath at 60 digits, pytorch_fid's sqrtm form and closed forms, the command on `-d cpu`, its refusals and the
argument checks of the new entries.  Every comparison of moments is integer equality; every float bound is relative to trace_term,
10x the error measured for that case (written beside it) and never above CAP."""
import json
import os
import re

import numpy as np
import pytest

from csl_gan_amd import moments as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["cslgan_mom_transpose_u8", "cslgan_mom_colsum_i64", "cslgan_mom_gram_i64", "cslgan_mom_mirror_i64"]
CAP = 1e-6          # derived, not measured: clipping near-zero eigenvalues costs up to about sqrt(D 2^-52) of the trace, 5e-8 at D = 12


def _cache(x):
    from csl_gan_amd.pipeline import CachedImages
    x = np.asarray(x, dtype=np.uint8)
    return CachedImages.from_arrays(x, np.zeros(len(x)), True)


def _rows(n, D, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (n, D), dtype=np.uint8)


# ---- the integers ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,D", [(1, 1), (2, 1), (63, 50), (65, 129), (300, 784)])
def test_host_moments_equal_the_direct_int64_product(n, D):
    x = _rows(n, D, 100 * n + D)
    x[0], x[-1] = 0, 255
    y = x.astype(np.int64) - 128
    want2 = y.T @ y
    want1 = [sum(int(v) - 128 for v in x[:, j]) for j in range(D)]
    for block in (7, 4096):
        m = MO.byte_moments_host(x, block=block)
        assert m["n"] == n and m["s1"].dtype == np.int64 and m["s2"].dtype == np.int64
        assert m["s1"].tolist() == want1 and np.array_equal(m["s2"], want2)
    c = MO.byte_moments(_cache(x.reshape(n, D, 1, 1)), "cpu", block_rows=64)
    assert c["n"] == n and np.array_equal(c["s1"], m["s1"]) and np.array_equal(c["s2"], want2)


def test_host_moments_of_constant_rows():
    for byte, sq in ((0, 16384), (255, 16129)):
        m = MO.byte_moments_host(np.full((300, 5), byte, dtype=np.uint8), block=128)
        assert (m["s2"] == 300 * sq).all() and (m["s1"] == 300 * (byte - 128)).all()
    with pytest.raises(ValueError, match="exact float64 product"):
        MO.byte_moments_host(np.zeros((3, 2), dtype=np.uint8), block=2 ** 38)


def test_centred_moments_equal_the_python_int_expression():
    x = _rows(37, 9, 4)
    x[:, 0], x[:, 1] = 0, 255
    m = MO.byte_moments_host(x)
    M = MO.centred(m["s1"], m["s2"], 37)
    assert M.dtype == np.int64
    assert M.tolist() == [[37 * int(m["s2"][i, j]) - int(m["s1"][i]) * int(m["s1"][j]) for j in range(9)] for i in range(9)]
    assert M[0, 0] == 0 and M[1, 1] == 0 and not M[0].any()                            # a constant column has no variance at all
    big = 2 ** 24 - 1                                                                  # the largest N: both terms reach N^2 2^14 < 2^62
    M = MO.centred(np.array([-128 * big]), np.array([[16384 * big]]), big)
    assert int(M[0, 0]) == big * 16384 * big - (128 * big) ** 2 == 0
    assert np.array_equal(MO.covariance(m["s1"], m["s2"], 37), MO.centred(m["s1"], m["s2"], 37) / (37.0 * 36.0))
    assert np.allclose(MO.covariance(m["s1"], m["s2"], 37), np.cov(x.astype(np.float64), rowvar=False), rtol=1e-12, atol=1e-9)


# ---- the float step -------------------------------------------------------------------------------------------------------------------------

def _fd(A, B):
    return MO.frechet_from_moments(MO.byte_moments_host(A), MO.byte_moments_host(B))


def _mp_reference(A, B):
    """FD at 60 digits from the exact integers: eigsy for both roots, eigenvalues clipped at 0 (they are then below 1e-55)."""
    import mpmath as mp
    with mp.workdps(60):
        def cov(x):
            m = MO.byte_moments_host(x)
            n, D = m["n"], len(m["s1"])
            M = mp.matrix(D, D)
            for i in range(D):
                for j in range(D):
                    M[i, j] = mp.mpf(n * int(m["s2"][i, j]) - int(m["s1"][i]) * int(m["s1"][j])) / (n * (n - 1))
            return M, [mp.mpf(int(v)) / n for v in m["s1"]]

        def root(C):
            w, V = mp.eigsy(C)
            S = mp.diag([mp.sqrt(max(v, mp.mpf(0))) for v in w])
            return V * S * V.T

        ca, mua = cov(A)
        cb, mub = cov(B)
        D = len(mua)
        ra = root(ca)
        inner = ra * cb * ra
        w = mp.eigsy((inner + inner.T) / 2, eigvals_only=True)
        root_term = sum(mp.sqrt(max(v, mp.mpf(0))) for v in w)
        mean = sum((a - b) ** 2 for a, b in zip(mua, mub))
        tr = sum(ca[i, i] + cb[i, i] for i in range(D))
        return float(mean + tr - 2 * root_term), float(tr)


# (name, rows of A, rows of B, D): measured error relative to trace_term -> bound = 10x, capped
MP_CASES = [
    ("full rank D=6", 50, 40, 6, 4.3e-16),
    ("full rank D=12", 100, 80, 12, 5.8e-16),
    ("rank deficient D=6", 4, 5, 6, 4.6e-9),
    ("rank deficient D=12", 8, 12, 12, 3.7e-9),
    ("A full, B deficient D=12", 100, 7, 12, 3.7e-9),
]


@pytest.mark.parametrize("name,na,nb,D,measured", MP_CASES, ids=[c[0] for c in MP_CASES])
def test_float_step_against_mpmath_at_60_digits(name, na, nb, D, measured):
    A, B = _rows(na, D, 11 * D + na), _rows(nb, D, 13 * D + nb, hi=200)
    got = _fd(A, B)
    want, tr = _mp_reference(A, B)
    err = abs(got["fd"] - want) / tr
    print("%s: fd %.6f, mpmath %.6f, error / trace_term = %.3e" % (name, got["fd"], want, err))
    assert got["trace_term"] == pytest.approx(tr, rel=1e-14)
    bound = min(10.0 * measured, CAP)
    assert bound <= CAP and err <= bound


def test_float_step_against_the_sqrtm_form_of_pytorch_fid():
    """tr sqrtm(CA CB) at D = 32, full rank (300 / 200 rows): the route pytorch_fid takes, without its eps offset."""
    from scipy import linalg
    A, B = _rows(300, 32, 1), _rows(200, 32, 2, hi=180)
    got = _fd(A, B)
    ca, cb = np.cov(A.astype(np.float64), rowvar=False), np.cov(B.astype(np.float64), rowvar=False)
    d = A.mean(0) - B.mean(0)
    covmean = linalg.sqrtm(ca.dot(cb))
    want = d.dot(d) + np.trace(ca) + np.trace(cb) - 2.0 * np.trace(covmean.real)
    err = abs(got["fd"] - want) / got["trace_term"]
    print("sqrtm form: fd %.6f, pytorch_fid's %.6f, error / trace_term = %.3e" % (got["fd"], want, err))
    measured = 4.5e-16
    assert err <= min(10.0 * measured, CAP)


def test_closed_forms():
    # D = 1: (dmu)^2 + (sigma_a - sigma_b)^2
    a, b = _rows(40, 1, 3), _rows(25, 1, 4, hi=100)
    m = _fd(a, b)
    fa, fb = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    want = (fa.mean() - fb.mean()) ** 2 + (fa.std(ddof=1) - fb.std(ddof=1)) ** 2
    assert abs(m["fd"] - want) <= 1e-12 * m["trace_term"]                              # scalars only: a few roundings of 2^-53 each
    assert set(m) == {"fd", "fd_unit", "fd_per_dim", "mean_term", "trace_term", "sqrt_term", "n_a", "n_b", "dim"}
    assert (m["n_a"], m["n_b"], m["dim"]) == (40, 25, 1) and m["fd_unit"] == m["fd"] / 255.0 ** 2 and m["fd_per_dim"] == m["fd"]
    assert m["fd"] == m["mean_term"] + m["trace_term"] - 2.0 * m["sqrt_term"]
    for n, D in ((60, 24), (10, 24)):                                                  # full rank and N <= D
        A = _rows(n, D, n + D, hi=253)
        # A against A: no mean term at all, and fd is a rounding error of either sign, reported as computed
        same = _fd(A, A)
        print("A against A, %d x %d: fd %.3e, trace_term %.3e" % (n, D, same["fd"], same["trace_term"]))
        assert same["mean_term"] == 0.0 and abs(same["fd"]) <= CAP * same["trace_term"]
        # every byte 3 higher: the same covariance, dmu = 3 exactly in every column
        up = _fd(A, A + 3)
        assert up["mean_term"] == 9.0 * D and abs(up["fd"] - 9.0 * D) <= CAP * up["trace_term"]
        assert up["trace_term"] == same["trace_term"]
        # the arguments swapped
        B = _rows(n + 5, D, n, hi=200)
        ab, ba = _fd(A, B), _fd(B, A)
        assert ab["mean_term"] == ba["mean_term"] and ab["trace_term"] == pytest.approx(ba["trace_term"], rel=1e-15)
        assert abs(ab["fd"] - ba["fd"]) <= CAP * ab["trace_term"] and (ab["n_a"], ab["n_b"]) == (ba["n_b"], ba["n_a"])
        assert ab["fd"] > 100.0 * CAP * ab["trace_term"]                               # a distance that the cap does not swallow


def test_real_side_is_computed_once_and_agrees():
    A, B = _rows(50, 12, 8).reshape(50, 2, 3, 2), _rows(30, 12, 9, hi=99).reshape(30, 2, 3, 2)
    real = MO.real_side(_cache(A), block_rows=16)
    m, mom = MO.run_frechet(real, _cache(B), block_rows=7)
    assert m == _fd(A, B) and np.array_equal(mom["s2"], MO.byte_moments_host(B)["s2"])
    with pytest.raises(ValueError, match="one geometry"):
        MO.run_frechet(real, _cache(B.reshape(30, 3, 2, 2)))


def test_sizes_are_refused_with_the_figures():
    MO.check_sizes(162770, 12288)                                                      # CelebA: 1.2 GB of second moments
    MO.check_sizes(2 ** 24 - 1, 784)
    for n in (0, 1):
        with pytest.raises(ValueError, match="needs at least 2"):
            MO.check_sizes(n, 784)
    with pytest.raises(ValueError, match=r"N < 2\^24 = 16777216"):
        MO.check_sizes(2 ** 24, 784)
    with pytest.raises(ValueError, match="1 <= D <= 65536"):
        MO.check_sizes(10, 65537)
    with pytest.raises(ValueError, match=r"D \* D \* 8 = 1207959552 bytes .* above --resident_gb 1"):
        MO.check_sizes(162770, 12288, resident_gb=1.0)
    for n in (1, 2 ** 24):
        with pytest.raises(ValueError, match="need 2 <= N < 2.24"):
            MO.centred(np.zeros(2, dtype=np.int64), np.zeros((2, 2), dtype=np.int64), n)


# ---- the command line on the CPU ----------------------------------------------------------------------------------------------------------------

HWC = (4, 3, 2)
KEYS = {"fd", "fd_unit", "fd_per_dim", "mean_term", "trace_term", "sqrt_term", "n_a", "n_b", "dim"}


def _write(path, x):
    from csl_gan_amd.generate import CacheWriter
    n, H, W, C = x.shape
    w = CacheWriter(path, n, H, W, C, True, {"note": "test rows"})
    w(0, x, np.zeros(n, dtype=np.int64))
    w.close()


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("frechet")) + "/"
    rng = np.random.default_rng(7)
    x = {"train": rng.integers(0, 256, (60,) + HWC, dtype=np.uint8), "heldout": rng.integers(0, 256, (45,) + HWC, dtype=np.uint8),
         "syn": rng.integers(0, 200, (30,) + HWC, dtype=np.uint8), "syn2": rng.integers(0, 256, (12,) + HWC, dtype=np.uint8)}
    for k, v in x.items():
        _write(d + k, v)
    _write(d + "odd", rng.integers(0, 256, (9, 3, 4, 2), dtype=np.uint8))
    _write(d + "one", x["syn"][:1])
    return d, x


def test_cli_on_the_cpu(caches, tmp_path, capsys):
    from csl_gan_amd import frechet
    d, x = caches
    out, vals = str(tmp_path / "outputs"), str(tmp_path / "values")
    stats = frechet.main(["--syn_cache", d + "syn", d + "syn2", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "--baseline",
                          "-d", "cpu", "--block_rows", "16", "--values_dir", vals, "--save", "--outputs_dir", out, "--name", "q"])
    assert list(stats) == ["syn", "syn2", "baseline_heldout"]
    printed = capsys.readouterr().out
    for lab, n in (("syn", 30), ("syn2", 12), ("baseline_heldout", 45)):
        m = stats[lab]
        rows = x["heldout" if lab.startswith("baseline") else lab]
        assert set(m) == KEYS and (m["n_a"], m["n_b"], m["dim"]) == (60, n, 24)
        want = MO.byte_moments_host(rows)
        s1, s2 = np.load(os.path.join(vals, lab + "_s1.npy")), np.load(os.path.join(vals, lab + "_s2.npy"))
        assert s1.dtype == np.int64 and s2.dtype == np.int64 and np.array_equal(s1, want["s1"]) and np.array_equal(s2, want["s2"])
        assert m == _fd(x["train"], rows)
        assert ("%s: %d samples against 60 images of 24 bytes: fd " % (lab, n)) in printed
    assert len(os.listdir(vals)) == 6
    assert stats["syn"]["fd"] > stats["baseline_heldout"]["fd"] > 0.0                  # darker samples lie further off than real ones
    with open(os.path.join(out, "q.json")) as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    assert "s2 is 8 * D * D bytes" in frechet.build_parser().format_help()


def test_cli_refusals(caches):
    from csl_gan_amd import frechet
    d, _ = caches
    base = ["--train_cache", d + "train", "-d", "cpu"]
    with pytest.raises(SystemExit, match="--nontrain_cache"):
        frechet.main(["--syn_cache", d + "syn", "--baseline"] + base)
    with pytest.raises(SystemExit, match="one geometry"):
        frechet.main(["--syn_cache", d + "odd"] + base)
    with pytest.raises(SystemExit, match="one geometry"):
        frechet.main(["--syn_cache", d + "syn", "--nontrain_cache", d + "odd", "--baseline"] + base)
    with pytest.raises(SystemExit, match="a set of 1 rows: the unbiased covariance needs at least 2"):
        frechet.main(["--syn_cache", d + "one"] + base)
    with pytest.raises(SystemExit, match=r"D \* D \* 8 = 4608 bytes .* above --resident_gb 1e-06"):
        frechet.main(["--syn_cache", d + "syn", "--resident_gb", "0.000001"] + base)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from csl_gan_amd import _lib, build
    build.build()
    return _lib.lib()


def test_the_entries_are_declared_and_exported_and_the_abi_version_stays(L):
    from csl_gan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cslgan.h")).read()
    assert "Byte moments" in hdr
    declared = set(re.findall(r"\b(cslgan_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name)
    assert L.cslgan_version() == 7 and _lib.ABI_VERSION == 7
    assert "moment_kernels.hip" in __import__("csl_gan_amd.build", fromlist=["SOURCES"]).SOURCES


def test_the_entries_refuse_bad_arguments_before_any_launch(L):
    """Validation runs on the host before any launch: no device is needed.  16 stands for an aligned non-null pointer."""
    err = lambda: L.cslgan_last_error()
    ok = 16
    # transpose
    assert L.cslgan_mom_transpose_u8(None, 4, 10, 64, ok, None) == -1 and b"mom_transpose_u8: null" in err()
    assert L.cslgan_mom_transpose_u8(ok, 4, 10, 64, None, None) == -1 and b"mom_transpose_u8: null" in err()
    assert L.cslgan_mom_transpose_u8(ok, 0, 10, 64, ok, None) == -1 and b"mom_transpose_u8: n=0 must lie in 1 .. 65536" in err()
    assert L.cslgan_mom_transpose_u8(ok, 65537, 10, 65600, ok, None) == -1 and b"mom_transpose_u8: n=65537 must lie in 1 .. 65536" in err()
    assert L.cslgan_mom_transpose_u8(ok, 4, 0, 64, ok, None) == -1 and b"mom_transpose_u8: D=0" in err()
    assert L.cslgan_mom_transpose_u8(ok, 4, 65537, 64, ok, None) == -1 and b"mom_transpose_u8: D=65537" in err()
    assert L.cslgan_mom_transpose_u8(ok, 65, 10, 64, ok, None) == -1 and b"mom_transpose_u8: np=64 is not the padded width 128 of n=65" in err()
    assert L.cslgan_mom_transpose_u8(ok, 4, 10, 64, 8, None) == -1 and b"mom_transpose_u8: misaligned" in err()
    # column sums
    assert L.cslgan_mom_colsum_i64(None, 10, 64, ok, None) == -1 and b"mom_colsum_i64: null" in err()
    assert L.cslgan_mom_colsum_i64(ok, 10, 64, None, None) == -1 and b"mom_colsum_i64: null" in err()
    assert L.cslgan_mom_colsum_i64(ok, 0, 64, ok, None) == -1 and b"mom_colsum_i64: D=0" in err()
    assert L.cslgan_mom_colsum_i64(ok, 10, 100, ok, None) == -1 and b"mom_colsum_i64: np=100 must be a multiple of 64" in err()
    assert L.cslgan_mom_colsum_i64(ok, 10, 65600, ok, None) == -1 and b"mom_colsum_i64: np=65600" in err()
    assert L.cslgan_mom_colsum_i64(8, 10, 64, ok, None) == -1 and b"mom_colsum_i64: misaligned" in err()
    assert L.cslgan_mom_colsum_i64(ok, 10, 64, 20, None) == -1 and b"mom_colsum_i64: misaligned" in err()
    # Gram
    assert L.cslgan_mom_gram_i64(None, 10, 64, ok, 10, None) == -1 and b"mom_gram_i64: null" in err()
    assert L.cslgan_mom_gram_i64(ok, 10, 64, None, 10, None) == -1 and b"mom_gram_i64: null" in err()
    assert L.cslgan_mom_gram_i64(ok, 65537, 64, ok, 65537, None) == -1 and b"mom_gram_i64: D=65537" in err()
    assert L.cslgan_mom_gram_i64(ok, 10, 0, ok, 10, None) == -1 and b"mom_gram_i64: np=0" in err()
    assert L.cslgan_mom_gram_i64(ok, 10, 65600, ok, 10, None) == -1 and b"mom_gram_i64: np=65600 must be a multiple of 64 in 64 .. 65536" in err()
    assert L.cslgan_mom_gram_i64(ok, 10, 64, ok, 9, None) == -1 and b"mom_gram_i64: ld=9 is smaller than D=10" in err()
    assert L.cslgan_mom_gram_i64(8, 10, 64, ok, 10, None) == -1 and b"mom_gram_i64: misaligned" in err()
    assert L.cslgan_mom_gram_i64(ok, 10, 64, 20, 10, None) == -1 and b"mom_gram_i64: misaligned" in err()
    # mirror
    assert L.cslgan_mom_mirror_i64(None, 10, 10, None) == -1 and b"mom_mirror_i64: null" in err()
    assert L.cslgan_mom_mirror_i64(ok, 0, 10, None) == -1 and b"mom_mirror_i64: D=0" in err()
    assert L.cslgan_mom_mirror_i64(ok, 10, 9, None) == -1 and b"mom_mirror_i64: ld=9" in err()
    assert L.cslgan_mom_mirror_i64(20, 10, 10, None) == -1 and b"mom_mirror_i64: misaligned" in err()


def test_ops_refuse_cpu_tensors_and_wrong_types(L):
    import torch
    from csl_gan_amd import ops
    u8, x8, s64 = torch.zeros(4, 10, dtype=torch.uint8), torch.zeros(10, 64, dtype=torch.int8), torch.zeros(10, 10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mom_transpose(u8)
    with pytest.raises(RuntimeError, match="u8 must be a contiguous uint8"):
        ops.mom_transpose(u8.to(torch.int8))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mom_colsum(x8, s64[0])
    with pytest.raises(RuntimeError, match="s1 must be a contiguous int64"):
        ops.mom_colsum(x8, s64[0].to(torch.int32))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mom_gram(x8, s64)
    with pytest.raises(RuntimeError, match="S2 must be a contiguous int64"):
        ops.mom_gram(x8, s64.to(torch.float64))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mom_mirror(s64)
    assert ops.mom_padded_rows(1) == 64 and ops.mom_padded_rows(64) == 64 and ops.mom_padded_rows(65) == 128
