"""The sliced Wasserstein distance on the CPU: the direction stream, the host models of csl_gan_amd.sliced against three independent
statements of the one-dimensional W1 numerator, the overflow bound, the command on `-d cpu`, and the argument checks of the new
entries.  Every comparison of numerators is integer equality."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from csl_gan_amd import sliced as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["cslgan_swd_directions_i8", "cslgan_swd_project_i8", "cslgan_sort_rows_ws_bytes", "cslgan_sort_rows_i32", "cslgan_swd_w1_i64"]


# ---- directions -------------------------------------------------------------------------------------------------------------------------------

def test_directions_are_signs_that_depend_on_seed_direction_and_column_only():
    d8 = SL.directions_host(8, 300, 4)
    assert d8.dtype == np.int8 and d8.shape == (8, 300) and set(np.unique(d8).tolist()) == {-1, 1}
    d3000 = SL.directions_host(3000, 300, 4)
    assert np.array_equal(d3000[5], d8[5]) and np.array_equal(d3000[:8], d8)
    assert np.array_equal(SL.directions_host(8, 200, 4), d8[:, :200])                  # a shorter row is a prefix
    assert np.array_equal(SL.directions_host(3, 300, 4, first=5), d3000[5:8])
    assert not np.array_equal(SL.directions_host(8, 300, 5), d8)
    assert len({d3000[p].tobytes() for p in range(3000)}) == 3000                      # no two directions alike


def test_directions_follow_the_rule_of_the_header_word_by_word():
    """Column 128 b + t of direction p is bit t & 31 of word t >> 5 of Philox(counter (b, p, 0, tag), key seed ^ tag)."""
    from csl_gan_amd.generate import _philox4x32_10
    seed, D = 77, 700
    key = (seed ^ SL.SWD_SEED_TAG) & (2 ** 64 - 1)
    got = SL.directions_host(4, D, seed)
    for p, j in ((0, 0), (1, 31), (2, 32), (3, 127), (1, 128), (2, 300), (3, 699)):
        w = _philox4x32_10(j // 128, p, 0, SL.SWD_COUNTER_TAG, key & 0xFFFFFFFF, key >> 32)
        t = j % 128
        assert got[p, j] == (1 if (int(w[t >> 5]) >> (t & 31)) & 1 else -1)
    hdr = open(os.path.join(ROOT, "include", "cslgan.h")).read()
    assert "0x%08X" % SL.SWD_COUNTER_TAG in hdr and "0x%016X" % SL.SWD_SEED_TAG in hdr


def test_the_signs_are_balanced_to_five_sigma():
    s = SL.directions_host(64, 4096, 0).astype(np.float64)
    assert abs(s.mean()) <= 5.0 / math.sqrt(64 * 4096)


def test_the_tags_collide_with_no_other_stream():
    from csl_gan_amd import audit, classify, generate
    keys = {generate.LATENT_SEED_TAG, audit.AUDIT_SEED_TAG, classify.TREE_SEED_TAG, 0x6D65616E73616D70}
    counters = {generate.LATENT_COUNTER_TAG, classify.TREE_COUNTER_TAG, audit.ROUND_KEY_TAG} | set(audit.SIDE_TAG)
    assert SL.SWD_SEED_TAG not in keys and SL.SWD_COUNTER_TAG not in counters
    for name in ("device_prims.h", "clip_kernels.hip", "attack_kernels.hip", "tree_kernels.hip"):
        src = open(os.path.join(ROOT, "csl_gan_amd", "csrc", name)).read().lower()
        assert "%x" % SL.SWD_COUNTER_TAG not in src and "%x" % SL.SWD_SEED_TAG not in src


# ---- the numerators against three independent statements -------------------------------------------------------------------------------------------

SIZES = [(1, 1), (5, 3), (3, 5), (1, 257), (64, 64), (100, 37)]


def _sorted_sets(na, nb, P=7, seed=0):
    rng = np.random.default_rng(100 * na + nb + seed)
    a, b = rng.integers(-6, 7, (P, na)), rng.integers(-4, 9, (P, nb))               # few values: many ties
    a[0], b[0] = a[0] * (2 ** 23 // 6), b[0] * (2 ** 23 // 8)                        # one direction at the scale of the extremes
    return np.sort(a, axis=1).astype(np.int32), np.sort(b, axis=1).astype(np.int32)


def _brute(a, b):
    """Repeat every a Nb times and every b Na times, sort both, and sum |difference|: Python integers."""
    out = []
    for ra, rb in zip(a.tolist(), b.tolist()):
        ea, eb = sorted(v for v in ra for _ in rb), sorted(v for v in rb for _ in ra)
        out.append(sum(abs(x - y) for x, y in zip(ea, eb)))
    return out


@pytest.mark.parametrize("na,nb", SIZES)
def test_numerators_equal_the_brute_force_expansion(na, nb):
    a, b = _sorted_sets(na, nb)
    got = SL.w1_numerators_host(a, b, block=3)
    assert got.dtype == np.int64 and got.tolist() == _brute(a, b)
    if na == nb:
        assert got.tolist() == (na * np.abs(a.astype(np.int64) - b).sum(1)).tolist()


@pytest.mark.parametrize("na,nb", SIZES)
def test_numerators_equal_scipy(na, nb):
    stats = pytest.importorskip("scipy.stats")
    a, b = _sorted_sets(na, nb, seed=1)
    got = SL.w1_numerators_host(a, b)
    for p in range(len(a)):
        want = stats.wasserstein_distance(a[p].astype(np.float64), b[p].astype(np.float64)) * na * nb
        assert abs(int(got[p]) - want) <= 1e-12 * abs(want)


def _cache(x, labels=None):
    from csl_gan_amd.pipeline import CachedImages
    x = np.asarray(x, dtype=np.uint8)
    return CachedImages.from_arrays(x, np.zeros(len(x)) if labels is None else labels, True)


def _num(A, B, P=16, seed=3, **kw):
    real = SL.real_side(_cache(A), P, seed, **kw)
    return SL.run_swd(real, _cache(B), **kw)["num"]


def test_closed_forms():
    rng = np.random.default_rng(5)
    A = rng.integers(0, 253, (21, 3, 4, 2), dtype=np.uint8)
    B = rng.integers(0, 256, (13, 3, 4, 2), dtype=np.uint8)
    assert _num(A, A).tolist() == [0] * 16
    assert _num(A, np.repeat(A, 2, axis=0)).tolist() == [0] * 16                     # the same distribution at another size
    ab = _num(A, B)
    assert (ab > 0).all() and np.array_equal(_num(B, A), ab)
    # every byte c higher: every projection moves by c sum_j s_p[j], so num_p = c |sum_j s_p[j]| Na Nb
    c = 3
    s = SL.directions_host(16, 24, 3).astype(np.int64).sum(1)
    assert np.array_equal(_num(A, A + c), c * np.abs(s) * 21 * 21)
    assert np.array_equal(_num(A, np.repeat(A + c, 2, axis=0)), c * np.abs(s) * 21 * 42)
    # the blocking of the directions does not show
    assert np.array_equal(_num(A, B, resident_gb=1e-6, block_rows=4), ab)


def test_projection_is_the_definition():
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (9, 2, 5, 3), dtype=np.uint8)
    x[0], x[1] = 0, 255
    s = SL.directions_host(5, 30, 1)
    got = SL.project_host(s, x, block=4)
    want = [[sum(int(sj) * (int(v) - 128) for sj, v in zip(sp, row)) for row in x.reshape(9, -1)] for sp in s]
    assert got.dtype == np.int32 and got.tolist() == want


def test_metrics_from_numerators():
    m = SL.swd_metrics([40, 80, 120], 4, 5, 16, seed=9)
    assert set(m) == {"swd", "swd_unit", "max_sliced", "stderr", "n_a", "n_b", "n_dirs", "seed"}
    assert (m["n_a"], m["n_b"], m["n_dirs"], m["seed"]) == (4, 5, 3, 9)
    assert m["swd"] == pytest.approx(1.0) and m["max_sliced"] == pytest.approx(1.5) and m["swd_unit"] == m["swd"] / 255.0
    assert m["stderr"] == pytest.approx(0.5 / math.sqrt(3))
    assert SL.swd_metrics([7], 1, 1, 1)["stderr"] == 0.0


def test_sizes_past_the_overflow_bound_are_refused():
    SL.check_sizes(162770, 162770)                                                   # CelebA against itself: far inside
    SL.check_sizes(2 ** 19, 2 ** 19 - 1)
    for na, nb in ((2 ** 19, 2 ** 19), (2 ** 38, 1), (1, 2 ** 38)):
        with pytest.raises(ValueError, match=r"2\^25 >= 2\^63 overflows"):
            SL.check_sizes(na, nb)
    with pytest.raises(ValueError, match="at least one"):
        SL.check_sizes(0, 5)


# ---- the command line on the CPU ----------------------------------------------------------------------------------------------------------------

HWC = (4, 3, 2)


def _write(path, x, labels):
    from csl_gan_amd.generate import CacheWriter
    n, H, W, C = x.shape
    w = CacheWriter(path, n, H, W, C, True, {"note": "test rows"})
    w(0, x, np.asarray(labels, dtype=np.int64))
    w.close()


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("swd")) + "/"
    rng = np.random.default_rng(7)
    x = {"train": rng.integers(0, 256, (40,) + HWC, dtype=np.uint8), "heldout": rng.integers(0, 256, (45,) + HWC, dtype=np.uint8),
         "syn": rng.integers(0, 200, (30,) + HWC, dtype=np.uint8), "syn2": rng.integers(0, 256, (12,) + HWC, dtype=np.uint8)}
    y = {"train": np.arange(40) % 3, "heldout": np.arange(45) % 3, "syn": np.arange(30) % 2, "syn2": np.where(np.arange(12) % 2, 5, 1)}
    for k, v in x.items():
        _write(d + k, v, y[k])
    _write(d + "odd", rng.integers(0, 256, (9, 3, 4, 2), dtype=np.uint8), np.zeros(9))
    os.makedirs(d + "other")
    _write(d + "other/syn", x["syn2"], y["syn2"])
    return d, x, y


KEYS = {"swd", "swd_unit", "max_sliced", "stderr", "n_a", "n_b", "n_dirs", "seed"}


def test_cli_on_the_cpu(caches, tmp_path):
    from csl_gan_amd import swd
    d, x, y = caches
    out, vals = str(tmp_path / "outputs"), str(tmp_path / "values")
    stats = swd.main(["--syn_cache", d + "syn", d + "syn2", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "--baseline",
                      "--n_dirs", "20", "--seed", "11", "-d", "cpu", "--values_dir", vals, "--save", "--outputs_dir", out, "--name", "q"])
    assert list(stats) == ["syn", "syn2", "baseline_heldout"]
    s = SL.directions_host(20, 24, 11)
    a = np.sort(SL.project_host(s, x["train"]), axis=1)
    for lab, n in (("syn", 30), ("syn2", 12), ("baseline_heldout", 45)):
        m = stats[lab]
        assert set(m) == KEYS and (m["n_a"], m["n_b"], m["n_dirs"], m["seed"]) == (40, n, 20, 11)
        b = np.sort(SL.project_host(s, x["heldout" if lab.startswith("baseline") else lab]), axis=1)
        num = np.load(os.path.join(vals, lab + "_num.npy"))
        assert num.dtype == np.int64 and num.tolist() == _brute(a, b)
        w1 = num / (40.0 * n) / math.sqrt(24.0)
        assert m["swd"] == w1.mean() and m["max_sliced"] == w1.max() and m["swd_unit"] == m["swd"] / 255.0
        assert m["stderr"] == w1.std(ddof=1) / math.sqrt(20)
    assert len(os.listdir(vals)) == 3
    assert stats["syn"]["swd"] > stats["baseline_heldout"]["swd"]                    # darker samples lie further off than real ones
    with open(os.path.join(out, "q.json")) as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    again = swd.main(["--syn_cache", d + "heldout", "--train_cache", d + "train", "-d", "cpu", "--n_dirs", "4", "--save", "--outputs_dir", out,
                      "--name", "q"])
    assert list(again) == ["heldout"] and again["heldout"]["n_dirs"] == 4 and again["heldout"]["seed"] == 0
    with open(os.path.join(out, "q.json")) as f:
        merged = json.load(f)
    assert set(merged) == {"syn", "syn2", "baseline_heldout", "heldout"} and merged["syn"] == json.loads(json.dumps(stats["syn"]))


def test_cli_per_class(caches, tmp_path):
    from csl_gan_amd import swd
    d, x, y = caches
    vals = str(tmp_path / "values")
    stats = swd.main(["--syn_cache", d + "syn", d + "syn2", "--train_cache", d + "train", "--n_dirs", "6", "--per_class", "-d", "cpu",
                      "--values_dir", vals])
    # train holds 0 1 2; syn holds 0 1; syn2 holds 1 and 5: a label on one side only is skipped
    assert set(stats["syn"]) == KEYS | {"per_class"}
    assert list(stats["syn"]["per_class"]) == ["0", "1"] and list(stats["syn2"]["per_class"]) == ["1"]
    s = SL.directions_host(6, 24, 0)
    for lab, l in (("syn", 0), ("syn", 1), ("syn2", 1)):
        A, B = x["train"][y["train"] == l], x[lab][y[lab] == l]
        m = stats[lab]["per_class"][str(l)]
        assert set(m) == KEYS and (m["n_a"], m["n_b"]) == (len(A), len(B))
        num = np.load(os.path.join(vals, "%s_num_class%d.npy" % (lab, l)))
        assert num.dtype == np.int64 and num.tolist() == _brute(np.sort(SL.project_host(s, A), axis=1), np.sort(SL.project_host(s, B), axis=1))
    assert sorted(os.listdir(vals)) == ["syn2_num.npy", "syn2_num_class1.npy", "syn_num.npy", "syn_num_class0.npy", "syn_num_class1.npy"]


def test_cli_refusals(caches):
    from csl_gan_amd import swd
    d, _, _ = caches
    base = ["--train_cache", d + "train", "-d", "cpu"]
    with pytest.raises(SystemExit, match="--nontrain_cache"):
        swd.main(["--syn_cache", d + "syn", "--baseline"] + base)
    with pytest.raises(SystemExit, match="one geometry"):
        swd.main(["--syn_cache", d + "odd"] + base)
    with pytest.raises(SystemExit, match="one geometry"):
        swd.main(["--syn_cache", d + "syn", "--nontrain_cache", d + "odd", "--baseline"] + base)
    with pytest.raises(SystemExit, match="share the name"):
        swd.main(["--syn_cache", d + "syn", d + "other/syn"] + base)
    for n in ("0", "-3"):
        with pytest.raises(SystemExit, match="--n_dirs"):
            swd.main(["--syn_cache", d + "syn", "--n_dirs", n] + base)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from csl_gan_amd import _lib, build
    build.build()
    return _lib.lib()


def test_the_entries_are_declared_and_exported_and_the_abi_version_stays(L):
    from csl_gan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cslgan.h")).read()
    assert "Sliced Wasserstein audit" in hdr
    declared = set(re.findall(r"\b(cslgan_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name)
    assert L.cslgan_version() == 7 and _lib.ABI_VERSION == 7
    assert "swd_kernels.hip" in __import__("csl_gan_amd.build", fromlist=["SOURCES"]).SOURCES


def test_the_entries_refuse_bad_arguments_before_any_launch(L):
    """Validation runs on the host before any launch: no device is needed.  16 stands for an aligned non-null pointer."""
    err = lambda: L.cslgan_last_error()
    ok = 16
    # directions
    assert L.cslgan_swd_directions_i8(1, 4, 100, 128, None, None) == -1 and b"swd_directions_i8: null" in err()
    assert L.cslgan_swd_directions_i8(1, 0, 100, 128, ok, None) == -1 and b"swd_directions_i8: P=0" in err()
    assert L.cslgan_swd_directions_i8(1, 2 ** 31, 100, 128, ok, None) == -1 and b"swd_directions_i8: P=" in err()
    assert L.cslgan_swd_directions_i8(1, 4, 100, 100, ok, None) == -1 and b"swd_directions_i8: Dp=100 is not the padded width 128" in err()
    assert L.cslgan_swd_directions_i8(1, 4, 65537, 65600, ok, None) == -1 and b"swd_directions_i8: D=65537" in err()
    assert L.cslgan_swd_directions_i8(1, 4, 100, 128, 8, None) == -1 and b"swd_directions_i8: misaligned" in err()
    # projection
    assert L.cslgan_swd_project_i8(None, 4, ok, 4, 128, ok, 4, 0, None) == -1 and b"swd_project_i8: null" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 4, 128, None, 4, 0, None) == -1 and b"swd_project_i8: null" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 2 ** 31, 128, ok, 2 ** 32, 0, None) == -1 and b"swd_project_i8: n=2147483648 out of range" in err()
    assert L.cslgan_swd_project_i8(ok, 2 ** 31, ok, 4, 128, ok, 4, 0, None) == -1 and b"swd_project_i8: P=2147483648 out of range" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 0, 128, ok, 4, 0, None) == -1 and b"swd_project_i8: n=0" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 4, 128, ok, 303, 300, None) == -1 and b"swd_project_i8: ldy=303 is smaller than col0 + n = 300 + 4" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 4, 128, ok, 8, -1, None) == -1 and b"swd_project_i8: ldy" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 4, 100, ok, 4, 0, None) == -1 and b"swd_project_i8: Dp=100 must be a multiple of 64" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 4, 65600, ok, 4, 0, None) == -1 and b"swd_project_i8: Dp=65600" in err()
    assert L.cslgan_swd_project_i8(8, 4, ok, 4, 128, ok, 4, 0, None) == -1 and b"swd_project_i8: misaligned" in err()
    assert L.cslgan_swd_project_i8(ok, 4, ok, 4, 128, 18, 4, 0, None) == -1 and b"swd_project_i8: misaligned" in err()
    # sort
    assert L.cslgan_sort_rows_ws_bytes(0, 5) == 0 and L.cslgan_sort_rows_ws_bytes(5, 0) == 0 and L.cslgan_sort_rows_ws_bytes(5, 2 ** 31) == 0
    assert L.cslgan_sort_rows_ws_bytes(3, 5) >= 3 * 5 * 4 + 3 * 256 * 4
    assert L.cslgan_sort_rows_ws_bytes(2, 2 ** 24) >= 2 * 2 ** 24 * 4
    big = 1 << 20
    assert L.cslgan_sort_rows_i32(None, 3, 5, 5, 32, ok, big, None) == -1 and b"sort_rows_i32: null" in err()
    assert L.cslgan_sort_rows_i32(ok, 3, 5, 5, 32, None, big, None) == -1 and b"sort_rows_i32: null" in err()
    assert L.cslgan_sort_rows_i32(ok, 3, 0, 5, 32, ok, big, None) == -1 and b"sort_rows_i32: n=0 out of range" in err()
    assert L.cslgan_sort_rows_i32(ok, 3, 2 ** 31, 2 ** 31, 32, ok, big, None) == -1 and b"sort_rows_i32: n=2147483648 out of range" in err()
    assert L.cslgan_sort_rows_i32(ok, 0, 5, 5, 32, ok, big, None) == -1 and b"sort_rows_i32: P=0" in err()
    assert L.cslgan_sort_rows_i32(ok, 3, 5, 4, 32, ok, big, None) == -1 and b"sort_rows_i32: ld=4 is smaller than n=5" in err()
    for bits in (0, 33):
        assert L.cslgan_sort_rows_i32(ok, 3, 5, 5, bits, ok, big, None) == -1 and b"sort_rows_i32: key_bits" in err()
    assert L.cslgan_sort_rows_i32(ok, 3, 5, 5, 32, ok, 100, None) == -1 and b"sort_rows_i32: workspace of 100 bytes" in err()
    assert L.cslgan_sort_rows_i32(ok, 2 ** 20, 2 ** 24, 2 ** 24, 32, ok, big, None) == -1 and b"sort_rows_i32: P=1048576 rows" in err()
    assert L.cslgan_sort_rows_i32(18, 3, 5, 5, 32, ok, big, None) == -1 and b"sort_rows_i32: misaligned" in err()
    assert L.cslgan_sort_rows_i32(ok, 3, 5, 5, 32, 8, big, None) == -1 and b"sort_rows_i32: misaligned" in err()
    # numerators
    assert L.cslgan_swd_w1_i64(None, 5, 5, ok, 3, 3, 2, ok, None) == -1 and b"swd_w1_i64: null" in err()
    assert L.cslgan_swd_w1_i64(ok, 5, 5, ok, 3, 3, 2, None, None) == -1 and b"swd_w1_i64: null" in err()
    assert L.cslgan_swd_w1_i64(ok, 5, 0, ok, 3, 3, 2, ok, None) == -1 and b"swd_w1_i64: Na=0" in err()
    assert L.cslgan_swd_w1_i64(ok, 2 ** 31, 2 ** 31, ok, 3, 3, 2, ok, None) == -1 and b"swd_w1_i64: Na=2147483648" in err()
    assert L.cslgan_swd_w1_i64(ok, 5, 5, ok, 3, 3, 0, ok, None) == -1 and b"swd_w1_i64: P=0" in err()
    assert L.cslgan_swd_w1_i64(ok, 4, 5, ok, 3, 3, 2, ok, None) == -1 and b"swd_w1_i64: lda=4" in err()
    assert L.cslgan_swd_w1_i64(ok, 5, 5, ok, 2, 3, 2, ok, None) == -1 and b"swd_w1_i64: lda=5 / ldb=2" in err()
    assert L.cslgan_swd_w1_i64(ok, 2 ** 19, 2 ** 19, ok, 2 ** 19, 2 ** 19, 2, ok, None) == -1 and b"swd_w1_i64: Na * Nb * 2^25" in err() \
        and b">= 2^63 overflows" in err()
    assert L.cslgan_swd_w1_i64(ok, 5, 5, ok, 3, 3, 2, 20, None) == -1 and b"swd_w1_i64: misaligned" in err()


def test_ops_refuse_cpu_tensors_and_wrong_types(L):
    import torch
    from csl_gan_amd import ops
    d8, y32 = torch.zeros(4, 64, dtype=torch.int8), torch.zeros(4, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.swd_project(d8, d8, y32)
    with pytest.raises(RuntimeError, match="Y must be a contiguous int32"):
        ops.swd_project(d8, d8, y32.to(torch.int64))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.sort_rows(y32)
    with pytest.raises(RuntimeError, match="x must be a contiguous int32"):
        ops.sort_rows(y32.to(torch.int64))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.swd_w1(y32, 8, y32, 8)
    with pytest.raises(RuntimeError, match="b must be a contiguous int32"):
        ops.swd_w1(y32, 8, y32.to(torch.int64), 8)
