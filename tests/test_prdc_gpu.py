"""cslgan_nn_kth_i8, cslgan_nn_count_radius_i8 and their drivers on the device against the host models
(csl_gan_amd.neighbours.kth_host, csl_gan_amd.manifold.count_within_radii_host).  Every comparison is integer equality."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csl_gan_amd import manifold as MF
from csl_gan_amd import neighbours as NB

DEV = "cuda:0"
U32 = 2 ** 32 - 1
NONE = NB.NONE_KEY


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)         # a copy: the shared cases are read-only


def _prepared(x):
    from csl_gan_amd import ops
    return ops.nn_prepare(_dev(x))


def _device_kth(Q, R, k, index_base=0, self_base=-1, best=None):
    from csl_gan_amd import ops
    q, qn = _prepared(Q)
    r, rn = _prepared(R)
    b = torch.full((len(Q), k), -1, device=DEV, dtype=torch.int64) if best is None else best
    ops.nn_kth(q, qn, r, rn, index_base, b, self_base)
    return b.cpu().numpy().view(np.uint64)


def _device_counts(Q, R, radii, counts=None):
    from csl_gan_amd import ops
    q, qn = _prepared(Q)
    r, rn = _prepared(R)
    c = torch.zeros(len(Q), device=DEV, dtype=torch.int32) if counts is None else counts
    ops.nn_count_radius(q, qn, r, rn, _dev(np.asarray(radii, dtype=np.int64).astype(np.uint32).view(np.int32)), c)
    return c.cpu().numpy().astype(np.int64)


# ---- the k smallest keys against the host model ------------------------------------------------------------------------------------------
# The launch rule is nn_min's (column ranges for about 1024 workgroups): at 300 x 5000 every one of the 40 column tiles is its own
# workgroup — the merge of 40 partial lists; at 8192 x 5120 a workgroup walks three column tiles — the running bound across tiles.
SHAPES = [(1, 2, 1, 1), (17, 33, 63, 3), (130, 257, 784, 5), (300, 5000, 192, 8), (256, 1000, 12288, 5), (8192, 5120, 64, 5)]


@functools.lru_cache(maxsize=None)
def _case(nq, nr, D, k):
    """Random bytes; min(k + 1, nr) reference rows scattered over R hold the SAME bytes and one query equals them, so that query's
    k-th and (k + 1)-th d2 are both 0 and every other query meets k + 1 equal distances: the index decides.  (Q, R, radii)."""
    rng = np.random.default_rng(11 + nq + 3 * nr + 5 * D + 7 * k)
    Q, R = rng.integers(0, 256, (nq, D), dtype=np.uint8), rng.integers(0, 256, (nr, D), dtype=np.uint8)
    copies = np.linspace(0, nr - 1, min(k + 1, nr)).astype(np.int64)
    R[copies] = R[copies[0]]
    Q[nq // 2] = R[copies[0]]
    # radii around the typical d2 of random bytes (D (256^2 - 1) / 6), with zeros and all-ones among them
    radii = rng.integers(9000 * D, 13000 * D, nr, dtype=np.int64)
    radii[rng.integers(0, nr, max(1, nr // 8))] = 0
    radii[rng.integers(0, nr, max(1, nr // 8))] = U32
    radii[copies] = 0
    for x in (Q, R, radii, copies):
        x.setflags(write=False)
    return Q, R, radii, copies


@functools.lru_cache(maxsize=None)
def _want_kth(nq, nr, D, k):
    Q, R, _, _ = _case(nq, nr, D, k)
    w = NB.kth_host(Q, R, k)
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("nq,nr,D,k", SHAPES)
def test_kth_equals_the_host_model(nq, nr, D, k):
    Q, R, _, copies = _case(nq, nr, D, k)
    want = _want_kth(nq, nr, D, k)
    got = _device_kth(Q, R, k)
    assert got.shape == (nq, k) and np.array_equal(got, want)
    # the query that equals the tied rows: the k smallest INDICES of them, all at d2 = 0
    assert got[nq // 2].tolist() == [int(c) for c in copies[:k]]
    assert (np.diff(got.astype(object), axis=1) > 0).all()          # ascending and distinct


@pytest.mark.parametrize("nq,nr,D,k", SHAPES)
def test_counts_inside_radii_equal_the_host_model(nq, nr, D, k):
    Q, R, radii, copies = _case(nq, nr, D, k)
    got = _device_counts(Q, R, radii)
    assert np.array_equal(got, MF.count_within_radii_host(Q, R, radii))
    assert got[nq // 2] >= len(copies)                               # radius 0 and d2 = 0: the duplicates count (<=, not <)
    if nq * nr > 100:
        assert 0 < got.sum() < nq * nr


def _descending(nr, D=64):
    """R[j] whose d2 to EVERY row with bytes <= 3 strictly decreases with j: row j + 1 is row j with one byte lowered by 1, and all
    bytes stay >= 4."""
    T = 4 * D + (nr - 1 - np.arange(nr))
    return (T[:, None] // D + (np.arange(D)[None, :] < (T % D)[:, None])).astype(np.uint8)


def test_every_column_inserts_and_only_the_first_k_insert():
    nq, nr, D, k = 130, 600, 64, 5
    Q = np.random.default_rng(3).integers(0, 4, (nq, D), dtype=np.uint8)
    R = _descending(nr, D)
    a, b = Q.astype(np.int64), R.astype(np.int64)
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)
    assert (np.diff(d2, axis=1) < 0).all()                           # every column beats every earlier one
    got = _device_kth(Q, R, k)
    assert np.array_equal(got, NB.kth_host(Q, R, k))
    assert np.array_equal(NB.split_keys(got)[1], np.tile(np.arange(nr - 1, nr - 1 - k, -1), (nq, 1)))
    rev = np.ascontiguousarray(R[::-1])                              # now only the first k columns insert
    got = _device_kth(Q, rev, k)
    assert np.array_equal(got, NB.kth_host(Q, rev, k))
    assert np.array_equal(NB.split_keys(got)[1], np.tile(np.arange(k), (nq, 1)))


# ---- the self search -------------------------------------------------------------------------------------------------------------------------

def test_self_search_leaves_out_the_own_index_only_and_does_not_depend_on_the_calls():
    from csl_gan_amd import ops
    n, D, k = 700, 100, 5
    X = np.random.default_rng(5).integers(0, 256, (n, D), dtype=np.uint8)
    X[600], X[130], X[699] = X[5], X[129], X[0]                      # twins: same bytes, another index
    want = NB.kth_host(X, X, k, self_base=0)
    got = _device_kth(X, X, k, self_base=0)
    assert np.array_equal(got, want)
    d2, idx = NB.split_keys(got)
    assert not (idx == np.arange(n)[:, None]).any()                  # no list holds its own index
    for a, b in ((5, 600), (129, 130), (0, 699)):
        assert (d2[a, 0], idx[a, 0], d2[b, 0], idx[b, 0]) == (0, b, 0, a)
    assert (d2[1:5, 0] > 0).all()
    assert np.array_equal(_device_kth(X, X, k, self_base=0), got)    # a rerun repeats the bits
    # the same search in 2 x 3 calls: query rows 0 .. 299 and 300 .. 699 against thirds of the reference, indices shifted by 1000
    off = 1000
    parts = []
    for s, e in ((0, 300), (300, n)):
        q, qn = _prepared(X[s:e])
        best = torch.full((e - s, k), -1, device=DEV, dtype=torch.int64)
        for r0, r1 in ((0, 233), (233, 466), (466, n)):
            r, rn = _prepared(X[r0:r1])
            ops.nn_kth(q, qn, r, rn, off + r0, best, off + s)
        parts.append(best.cpu().numpy().view(np.uint64))
    assert np.array_equal(np.concatenate(parts), got + np.uint64(off))
    assert np.array_equal(NB.kth_host(X, X, k, index_base=off, self_base=off), got + np.uint64(off))


# ---- ranges ----------------------------------------------------------------------------------------------------------------------------------

def _far_rows():
    nq, nr, D = 4, 70, 49152
    alt = np.tile(np.array([0, 255], dtype=np.uint8), D // 2)
    Q = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8), alt, 255 - alt])
    R = np.stack([(np.full(D, 255, np.uint8), np.zeros(D, np.uint8), 255 - alt, alt, np.full(D, 255, np.uint8))[j % 5] for j in range(nr)])
    return Q, R, 65025 * D


def test_distances_above_two_to_the_31_come_back_exact_and_in_order():
    """Rows near 0 and 255: R[j] is all 255 with its first j bytes at 254, so the all-zero query is 65025 D - 509 j away from it."""
    Q, _, far = _far_rows()
    nr, D = 70, Q.shape[1]
    R = np.full((nr, D), 255, dtype=np.uint8)
    for j in range(nr):
        R[j, :j] = 254
    base = U32 - nr                                                  # the last index is 2^32 - 2
    got = _device_kth(Q, R, 3, index_base=base)
    assert np.array_equal(got, NB.kth_host(Q, R, 3, index_base=base))
    d2, idx = NB.split_keys(got)
    assert d2[0].tolist() == [far - 509 * j for j in (69, 68, 67)] and d2[0].min() > 2 ** 31
    assert (idx[0] - base).tolist() == [69, 68, 67] and idx[0, 0] == U32 - 1
    assert d2[1].tolist() == [0, 1, 2] and (idx[1] - base).tolist() == [0, 1, 2]


def test_fewer_than_k_candidates_leave_all_ones_tails_and_smaller_keys_in_best_survive():
    rng = np.random.default_rng(9)
    Q, R = rng.integers(0, 256, (9, 50), dtype=np.uint8), rng.integers(0, 256, (3, 50), dtype=np.uint8)
    got = _device_kth(Q, R, 8)
    assert np.array_equal(got, NB.kth_host(Q, R, 8))
    assert (got[:, :3] != NONE).all() and (got[:, 3:] == NONE).all()
    # best already holds two keys per row that are smaller than anything R brings (d2 = 0 and 1 at indices past R's) and one larger
    pre = np.full((9, 8), NONE, dtype=np.uint64)
    pre[:, 0], pre[:, 1], pre[:, 2] = np.uint64(100), np.uint64((1 << 32) | 101), np.uint64((U32 - 1) << 32 | 102)
    best = _dev(pre.view(np.int64))
    got = _device_kth(Q, R, 8, best=best)
    assert np.array_equal(got, NB.kth_host(Q, R, 8, best=pre))
    assert np.array_equal(got[:, :2], pre[:, :2]) and np.array_equal(got[:, 5], pre[:, 2]) and (got[:, 6:] == NONE).all()


def test_every_existing_column_is_counted_once_and_no_other_and_guard_rows_keep_their_fill():
    """At radius 2^32 - 1 every d2 passes, the zero padding's too: a count other than nr is a column past nr or one counted twice."""
    nq, nr, D, k = 130, 257, 784, 5
    Q, R, _, _ = _case(nq, nr, D, k)
    buf = torch.full((nq + 140,), 77, device=DEV, dtype=torch.int32)
    got = _device_counts(Q, R, np.full(nr, U32), counts=buf[:nq])
    assert (got == 77 + nr).all()
    assert (buf[nq:].cpu().numpy() == 77).all()


def test_radii_above_two_to_the_31_compare_as_unsigned_and_two_calls_over_halves_add_up():
    from csl_gan_amd import ops
    Q, R, far = _far_rows()
    nr, half = len(R), far // 2
    radii = np.array([(far, far - 1, half, half - 1, 0)[(j // 5) % 5] for j in range(nr)], dtype=np.int64)
    want = MF.count_within_radii_host(Q, R, radii)
    assert np.array_equal(_device_counts(Q, R, radii), want)
    assert 0 < want.min() and want.max() < nr
    q, qn = _prepared(Q)
    c = torch.zeros(len(Q), device=DEV, dtype=torch.int32)
    for r0, r1 in ((0, 33), (33, nr)):
        r, rn = _prepared(R[r0:r1])
        ops.nn_count_radius(q, qn, r, rn, _dev(radii[r0:r1].astype(np.uint32).view(np.int32)), c)
    assert np.array_equal(c.cpu().numpy().astype(np.int64), want)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_the_entries_refuse_bad_arguments_before_any_launch():
    from csl_gan_amd import _lib
    L = _lib.lib()
    assert {"cslgan_nn_kth_workspace_bytes", "cslgan_nn_kth_i8", "cslgan_nn_count_radius_i8"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == L.cslgan_version() == 7
    err = lambda: L.cslgan_last_error()
    need = L.cslgan_nn_kth_workspace_bytes(4, 9, 3)
    assert need == 4 * 3 * 8                                         # one column range
    assert L.cslgan_nn_kth_workspace_bytes(300, 5000, 8) == 40 * 300 * 8 * 8
    for bad in ((0, 9, 3), (4, 0, 3), (4, 9, 0), (4, 9, 9), (2 ** 31, 9, 3), (4, 2 ** 31, 3)):
        assert L.cslgan_nn_kth_workspace_bytes(*bad) == 0
    names = ("q", "qn", "nq", "r", "rn", "nr", "Dp", "index_base", "self_base", "k", "best", "ws", "ws_bytes")
    ok = dict(q=64, qn=64, nq=4, r=64, rn=64, nr=9, Dp=128, index_base=0, self_base=-1, k=3, best=64, ws=64, ws_bytes=need)
    call = lambda **kw: L.cslgan_nn_kth_i8(*[dict(ok, **kw)[n] for n in names], None)
    for n in ("q", "qn", "r", "rn", "best", "ws"):
        assert call(**{n: None}) == -1 and b"null" in err()
    assert call(k=0) == -1 and b"k=0" in err()
    assert call(k=9) == -1 and b"k=9" in err()
    for dp in (0, 96, 65600):
        assert call(Dp=dp) == -1 and b"Dp=%d" % dp in err()
    assert call(nq=0) == -1 and b"nq=0" in err()
    assert call(nr=0) == -1 and b"nr=0" in err()
    assert call(nq=2 ** 31) == -1 and b"nq=2147483648" in err()
    assert call(nr=2 ** 31) == -1 and b"nr=2147483648" in err()
    assert call(index_base=-1) == -1 and b"index_base" in err()
    assert call(index_base=U32 - 8) == -1 and b"index_base" in err()
    assert call(self_base=-2) == -1 and b"self_base=-2" in err()
    assert call(self_base=U32 - 3) == -1 and b"self_base" in err()
    assert call(ws_bytes=need - 1) == -1 and b"workspace" in err()
    for n, p in (("q", 72), ("r", 8), ("qn", 66), ("rn", 65), ("best", 68), ("ws", 68)):
        assert call(**{n: p}) == -1 and b"misaligned" in err()
    names = ("q", "qn", "nq", "r", "rn", "nr", "Dp", "radius", "counts")
    ok = dict(q=64, qn=64, nq=4, r=64, rn=64, nr=9, Dp=128, radius=64, counts=64)
    call = lambda **kw: L.cslgan_nn_count_radius_i8(*[dict(ok, **kw)[n] for n in names], None)
    for n in ("q", "qn", "r", "rn", "radius", "counts"):
        assert call(**{n: None}) == -1 and b"null" in err()
    for dp in (0, 96, 65600):
        assert call(Dp=dp) == -1 and b"Dp=%d" % dp in err()
    for kw, msg in ((dict(nq=0), b"nq=0"), (dict(nr=0), b"nr=0"), (dict(nq=2 ** 31), b"nq=2147483648"), (dict(nr=2 ** 31), b"nr=2147483648")):
        assert call(**kw) == -1 and msg in err()
    for n, p in (("q", 72), ("r", 8), ("qn", 66), ("rn", 65), ("radius", 66), ("counts", 66)):
        assert call(**{n: p}) == -1 and b"misaligned" in err()


# ---- NearestSearch -------------------------------------------------------------------------------------------------------------------------------

HWC = (8, 8, 3)


def _cache(x):
    from csl_gan_amd.pipeline import CachedImages
    return CachedImages.from_arrays(x, np.zeros(len(x)), True)


@functools.lru_cache(maxsize=None)
def _sets():
    rng = np.random.default_rng(21)
    ref, qry = rng.integers(0, 256, (2600,) + HWC, dtype=np.uint8), rng.integers(0, 256, (300,) + HWC, dtype=np.uint8)
    ref[2599], ref[70], qry[3] = ref[0], ref[1500], ref[64]
    cpu = NB.NearestSearch("cpu").fit(_cache(ref))
    self_keys = cpu.kth(cpu.ref, 5, exclude_self=True)
    radii = MF.knn_radii(self_keys)
    return ref, qry, self_keys, cpu.kth(_cache(qry), 3), radii, cpu.count_within_radii(_cache(qry), radii)


@pytest.mark.parametrize("block_rows,query_rows", [(64, 16384), (1000, 700), (2500, 128)])
def test_the_search_does_not_depend_on_blocks_chunks_or_the_device(block_rows, query_rows):
    ref, qry, self_keys, qry_keys, radii, counts = _sets()
    s = NB.NearestSearch(DEV, block_rows=block_rows, query_rows=query_rows, resident_gb=0.0004).fit(_cache(ref))
    assert np.array_equal(s.kth(s.ref, 5, exclude_self=True), self_keys)
    assert np.array_equal(s.kth(_cache(qry), 3), qry_keys)
    got = s.count_within_radii(_cache(qry), radii)
    assert got.dtype == np.int64 and np.array_equal(got, counts)
    with pytest.raises(ValueError, match="fitted reference"):
        s.kth(_cache(ref), 5, exclude_self=True)


# ---- the command ---------------------------------------------------------------------------------------------------------------------------------

def test_cli_on_the_device_equals_the_cpu(tmp_path):
    from csl_gan_amd import prdc
    from csl_gan_amd.generate import CacheWriter
    rng = np.random.default_rng(31)
    x = {"train": rng.integers(0, 256, (300,) + HWC, dtype=np.uint8), "heldout": rng.integers(0, 256, (260,) + HWC, dtype=np.uint8),
         "syn": rng.integers(0, 256, (200,) + HWC, dtype=np.uint8), "syn2": rng.integers(0, 256, (150,) + HWC, dtype=np.uint8)}
    x["syn"][:100] = x["train"][:100]
    x["syn"][:100, 0, 0, 0] ^= 1
    for name, v in x.items():
        w = CacheWriter(str(tmp_path / name), len(v), *HWC, True, {"note": "test rows"})
        w(0, v, np.zeros(len(v), dtype=np.int64))
        w.close()
    args = ["--syn_cache", str(tmp_path / "syn"), str(tmp_path / "syn2"), "--train_cache", str(tmp_path / "train"), "--nontrain_cache",
            str(tmp_path / "heldout"), "--baseline", "-k", "4", "--block_rows", "128"]
    cpu = prdc.main(args + ["-d", "cpu"])
    dev = prdc.main(args + ["-d", DEV])
    assert set(dev) == {"syn", "syn2", "baseline_heldout"} and dev == cpu
    assert dev["syn"]["precision_hits"] >= 100 and dev["syn"]["n_syn"] == 200 and dev["syn"]["k"] == 4
