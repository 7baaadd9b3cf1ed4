"""The nearest-neighbour kernels and their driver on the device against the host model (csl_gan_amd.neighbours.nearest_host).
Every comparison is integer equality: the keys as uint64, the prepared bytes and norms as they are."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csl_gan_amd import neighbours as NB

DEV = "cuda:0"
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)         # a copy: the shared cases are read-only


def _prepared(x):
    from csl_gan_amd import ops
    return ops.nn_prepare(_dev(x))


def _device_keys(Q, R, index_base=0, best=None):
    from csl_gan_amd import ops
    q, qn = _prepared(Q)
    r, rn = _prepared(R)
    b = torch.full((len(Q),), -1, device=DEV, dtype=torch.int64) if best is None else _dev(np.asarray(best, dtype=np.uint64).view(np.int64))
    ops.nn_min(q, qn, r, rn, index_base, b)
    return b.cpu().numpy().view(np.uint64)


# ---- nn_prepare -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [1, 16, 63, 64, 65, 784, 12288])
@pytest.mark.parametrize("rows", [1, 17, 300])
def test_prepare_shifts_pads_with_zero_and_sums_squares(rows, D):
    from csl_gan_amd import ops
    rng = np.random.default_rng(1000 * rows + D)
    x = rng.integers(0, 256, (rows, D), dtype=np.uint8)
    x[0, 0], x[-1, -1] = 0, 255                         # both ends of the byte range, the last byte of the tensor included
    Dp = ops.nn_padded_dim(D)
    assert Dp % 64 == 0 and D <= Dp < D + 64
    out = torch.full((rows, Dp), 0x5A, device=DEV, dtype=torch.int8)             # garbage: unwritten padding would show
    sq = torch.full((rows,), -12345, device=DEV, dtype=torch.int32)
    xs, n = ops.nn_prepare(_dev(x), out=out, out_sqnorm=sq)
    assert xs.data_ptr() == out.data_ptr() and n.data_ptr() == sq.data_ptr()
    xs, n = xs.cpu().numpy(), n.cpu().numpy()
    want = x.astype(np.int16) - 128
    assert xs.dtype == np.int8 and np.array_equal(xs[:, :D], want)
    assert not xs[:, D:].any()
    assert np.array_equal(n.astype(np.int64), (want.astype(np.int64) ** 2).sum(1))


def test_prepare_takes_an_image_shaped_tensor():
    from csl_gan_amd import ops
    x = np.random.default_rng(3).integers(0, 256, (5, 7, 3, 3), dtype=np.uint8)
    xs, n = ops.nn_prepare(_dev(x))
    assert tuple(xs.shape) == (5, 64) and np.array_equal(xs.cpu().numpy()[:, :63], x.reshape(5, 63).astype(np.int16) - 128)


# ---- nn_min against the host model ----------------------------------------------------------------------------------------------------

SHAPES = [(1, 1, 1), (17, 33, 63), (130, 257, 784), (256, 1000, 12288), (300, 5000, 192)]


@functools.lru_cache(maxsize=None)
def _case(nq, nr, D):
    """Random bytes with planted duplicates and tied reference rows; Q is unrelated to R otherwise.  (Q, R, host keys), read-only."""
    rng = np.random.default_rng(7 + nq + 3 * nr + 5 * D)
    Q, R = rng.integers(0, 256, (nq, D), dtype=np.uint8), rng.integers(0, 256, (nr, D), dtype=np.uint8)
    if nr > 1:
        lo, hi = nr // 3, nr - 1
        R[hi] = R[lo]                                   # a tied pair of reference rows: the smaller index must win ...
        Q[nq // 2] = R[lo]                              # ... for an exact duplicate of them,
        if nq > 2:
            Q[nq - 1] = R[lo]
            Q[nq - 1, D - 1] ^= 1                       # ... and at distance 1
        if nq > 3:
            Q[1] = R[nr // 2 + 1 if nr // 2 + 1 < hi else 0]      # a plain duplicate
    keys = NB.nearest_host(Q, R)
    for a in (Q, R, keys):
        a.setflags(write=False)
    return Q, R, keys


@pytest.mark.parametrize("nq,nr,D", SHAPES)
def test_keys_equal_the_host_model(nq, nr, D):
    Q, R, want = _case(nq, nr, D)
    got = _device_keys(Q, R)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    if nr > 1:
        d2, idx = NB.split_keys(got)
        assert (d2[nq // 2], idx[nq // 2]) == (0, nr // 3)
        if nq > 2:
            assert (d2[nq - 1], idx[nq - 1]) == (1, nr // 3)


def test_a_permuted_neighbour_is_found_not_the_own_row():
    """Q's row i lies next to R's row pi(i) for a fixed non-identity permutation: a kernel that answers with its own row index, or
    that swaps rows and columns, fails."""
    n, D = 200, 100
    rng = np.random.default_rng(11)
    R = rng.integers(0, 256, (n, D), dtype=np.uint8)
    pi = (np.arange(n) * 37 + 11) % n                   # 37 is coprime to 200: a permutation, and without a fixed point
    assert len(set(pi)) == n and not (pi == np.arange(n)).any()
    Q = R[pi].copy()
    Q[:, 5] ^= 3
    got = _device_keys(Q, R)
    d2, idx = NB.split_keys(got)
    assert np.array_equal(idx, pi) and (d2 > 0).all() and (d2 <= 9).all()
    assert np.array_equal(got, NB.nearest_host(Q, R))


# ---- range ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,nr,D", [(4, 70, 49152), (2, 5, 65536)])
def test_distances_above_two_to_the_31_come_back_exact(nq, nr, D):
    alt = np.tile(np.array([0, 255], dtype=np.uint8), D // 2)
    Q = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8), alt, 255 - alt][:nq])
    R = np.stack([(np.full(D, 255, np.uint8), np.zeros(D, np.uint8), 255 - alt, alt, np.full(D, 255, np.uint8))[j % 5] for j in range(nr)])
    # one query at a time against the rows that are far from it, so that every minimum itself is above 2^31
    for i in range(nq):
        far = np.array([j for j in range(nr) if ((Q[i].astype(np.int64) - R[j].astype(np.int64)) ** 2).sum() > 2 ** 31])
        assert len(far) >= 1
        want = NB.nearest_host(Q[i:i + 1], R[far])
        got = _device_keys(Q[i:i + 1], R[far])
        assert np.array_equal(got, want) and NB.split_keys(got)[0][0] > 2 ** 31
    assert np.array_equal(_device_keys(Q, R), NB.nearest_host(Q, R))
    d2, idx = NB.split_keys(_device_keys(Q[:1], R[:1]))
    assert d2[0] == 65025 * D and idx[0] == 0


# ---- index width ----------------------------------------------------------------------------------------------------------------------

def test_indices_above_two_to_the_31():
    Q, R, _ = _case(17, 33, 63)
    base = 2 ** 32 - 1 - 33
    got = _device_keys(Q, R, index_base=base)
    assert np.array_equal(got, NB.nearest_host(Q, R, index_base=base))
    d2, idx = NB.split_keys(got)
    assert (idx > 2 ** 31).all() and idx.max() <= 2 ** 32 - 2 and (got != NONE).all()


# ---- merging --------------------------------------------------------------------------------------------------------------------------

def test_smaller_keys_in_best_survive_and_the_others_are_replaced():
    Q, R, plain = _case(130, 257, 784)
    best = np.full(130, NONE, dtype=np.uint64)
    best[::3] = plain[::3] - np.uint64(1)               # smaller: must survive
    best[1::3] = plain[1::3] + np.uint64(1)             # larger: replaced
    got = _device_keys(Q, R, best=best)
    assert np.array_equal(got, NB.nearest_host(Q, R, best=best))
    assert np.array_equal(got[::3], best[::3]) and np.array_equal(got[1::3], plain[1::3]) and np.array_equal(got[2::3], plain[2::3])


def test_three_calls_over_thirds_equal_one_call_and_a_rerun_repeats_the_bits():
    from csl_gan_amd import ops
    Q, R, want = _case(300, 5000, 192)
    q, qn = _prepared(Q)
    best = torch.full((300,), -1, device=DEV, dtype=torch.int64)
    for s, e in ((3334, 5000), (0, 1667), (1667, 3334)):
        r, rn = _prepared(R[s:e])
        ops.nn_min(q, qn, r, rn, s, best)
    assert np.array_equal(best.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(_device_keys(Q, R), want) and np.array_equal(_device_keys(Q, R), want)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def _cache(x):
    from csl_gan_amd.pipeline import CachedImages
    return CachedImages.from_arrays(x, np.zeros(len(x)), True)


def test_nearest_search_does_not_depend_on_block_rows_or_the_device():
    rng = np.random.default_rng(21)
    R, Q = rng.integers(0, 256, (2500, 7, 5, 3), dtype=np.uint8), rng.integers(0, 256, (150, 7, 5, 3), dtype=np.uint8)
    R[2400], Q[9] = R[70], R[70]
    ref, qry = _cache(R), _cache(Q)
    want = NB.NearestSearch("cpu").fit(ref).query(qry)
    assert NB.split_keys(want)[1][9] == 70
    for block_rows in (64, 1000, 2500):
        s = NB.NearestSearch(DEV, block_rows=block_rows, query_rows=64 if block_rows == 1000 else 16384).fit(ref)
        first = s.query(qry)
        assert np.array_equal(first, want), block_rows
        assert s.resident_rows() == 2500
        assert np.array_equal(s.query(qry), first)      # against the resident reference
    s = NB.NearestSearch(DEV, block_rows=1000, resident_gb=1200 * 128 / 2 ** 30).fit(ref)      # room for one block: the rest streams again
    assert np.array_equal(s.query(qry), want) and s.resident_rows() == 1000
    assert np.array_equal(s.query(qry), want)
    with pytest.raises(ValueError, match="one geometry"):
        s.query(_cache(np.zeros((3, 5, 7, 3), dtype=np.uint8)))


def test_cli_on_the_device_agrees_with_the_cpu(tmp_path):
    from csl_gan_amd import nearest
    from csl_gan_amd.generate import CacheWriter
    rng = np.random.default_rng(22)
    d = str(tmp_path) + "/"
    x = {"train": rng.integers(0, 256, (700, 8, 8, 3), dtype=np.uint8), "heldout": rng.integers(0, 256, (300, 8, 8, 3), dtype=np.uint8),
         "syn": rng.integers(0, 256, (90, 8, 8, 3), dtype=np.uint8)}
    x["syn"][4] = x["train"][650]
    for k, v in x.items():
        w = CacheWriter(d + k, len(v), 8, 8, 3, True, {"note": "test rows"})
        w(0, v, np.zeros(len(v), dtype=np.int64))
        w.close()
    runs = {}
    for dev in ("cpu", DEV):
        tag = dev.replace(":", "")
        runs[dev] = nearest.main(["--syn_cache", d + "syn", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "-d", dev, "--baseline",
                                  "--block_rows", "256", "--values_dir", d + "values_" + tag, "--grid", "3", "--outputs_dir", d + "out_" + tag])
    assert json.dumps(runs["cpu"], sort_keys=True) == json.dumps(runs[DEV], sort_keys=True)
    assert runs["cpu"]["syn"]["duplicates"] == 1
    names = sorted(os.listdir(d + "values_cpu"))
    assert names == ["baseline_keys_train.npy", "syn_keys_heldout.npy", "syn_keys_train.npy"] == sorted(os.listdir(d + "values_cuda0"))
    for f in names:
        a, b = np.load(d + "values_cpu/" + f), np.load(d + "values_cuda0/" + f)
        assert a.dtype == np.uint64 == b.dtype and np.array_equal(a, b)
    with open(d + "out_cpu/nearest_syn_nearest.png", "rb") as f, open(d + "out_cuda0/nearest_syn_nearest.png", "rb") as g:
        assert f.read() == g.read()
