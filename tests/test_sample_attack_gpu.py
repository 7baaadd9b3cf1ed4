"""cslgan_nn_count_i8 and its driver on the device against the host model (csl_gan_amd.blackbox.count_within_host).  Every comparison
is integer equality."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csl_gan_amd import blackbox as BB
from csl_gan_amd import neighbours as NB

DEV = "cuda:0"
U32 = 2 ** 32 - 1


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)         # a copy: the shared cases are read-only


def _prepared(x):
    from csl_gan_amd import ops
    return ops.nn_prepare(_dev(x))


def _device_counts(Q, R, thr, counts=None):
    from csl_gan_amd import ops
    q, qn = _prepared(Q)
    r, rn = _prepared(R)
    c = torch.zeros((len(Q), len(thr)), device=DEV, dtype=torch.int32) if counts is None else counts
    ops.nn_count(q, qn, r, rn, thr, c)
    return c.cpu().numpy().astype(np.int64)


# ---- against the host model -----------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1, 1), (17, 33, 63), (130, 257, 784), (300, 5000, 192), (256, 1000, 12288)]


@functools.lru_cache(maxsize=None)
def _case(nq, nr, D):
    """Random bytes with planted duplicates, a tied pair of reference rows and a row at distance 1, as tests/test_nearest_gpu.py
    plants them.  (Q, R, the threshold sets), read-only.  The thresholds come from the exact d2 matrix (float64 holds it)."""
    rng = np.random.default_rng(7 + nq + 3 * nr + 5 * D)
    Q, R = rng.integers(0, 256, (nq, D), dtype=np.uint8), rng.integers(0, 256, (nr, D), dtype=np.uint8)
    if nr > 1:
        lo, hi = nr // 3, nr - 1
        R[hi] = R[lo]
        Q[nq // 2] = R[lo]
        if nq > 2:
            Q[nq - 1] = R[lo]
            Q[nq - 1, D - 1] ^= 1
        if nq > 3:
            Q[1] = R[nr // 2 + 1 if nr // 2 + 1 < hi else 0]
    a, b = Q.astype(np.float64), R.astype(np.float64)
    d2 = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int64)
    lowest = int(d2[d2 > 0].min()) if (d2 > 0).any() else 1
    sets = ((0, 1, U32), (int(np.sort(d2.reshape(-1))[d2.size // 2]),), (lowest + 1, lowest, lowest - 1, 2 * lowest))
    for x in (Q, R):
        x.setflags(write=False)
    return Q, R, sets


@functools.lru_cache(maxsize=None)
def _want(nq, nr, D, k):
    Q, R, sets = _case(nq, nr, D)
    w = BB.count_within_host(Q, R, sets[k])
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("nq,nr,D", SHAPES)
def test_counts_equal_the_host_model(nq, nr, D, k):
    Q, R, sets = _case(nq, nr, D)
    want = _want(nq, nr, D, k)
    got = _device_counts(Q, R, sets[k])
    assert got.shape == (nq, len(sets[k])) and np.array_equal(got, want)
    if nr > 1 and k == 0:
        assert got[nq // 2].tolist() == [2, 2, nr]       # the duplicate of the tied pair
        if nq > 2:
            assert got[nq - 1].tolist() == [0, 2, nr]    # at distance 1 of both
    if k == 1 and nq * nr > 1:
        assert 0 < got.sum() < nq * nr                   # the median splits the matrix


@pytest.mark.parametrize("nq,nr,D", [(17, 33, 63), (130, 257, 784), (300, 5000, 192)])
def test_every_existing_column_is_counted_once_and_no_other_and_guard_rows_keep_their_fill(nq, nr, D):
    """At 2^32 - 1 every d2 passes, the zero padding's too: a count other than nr is a column past nr or a column counted twice."""
    Q, R, _ = _case(nq, nr, D)
    buf = torch.full((nq + 140, 2), 77, device=DEV, dtype=torch.int32)
    got = _device_counts(Q, R, (U32, 0), counts=buf[:nq])
    assert (got[:, 0] == 77 + nr).all()
    assert np.array_equal(got[:, 1] - 77, _want(nq, nr, D, 0)[:, 0])
    assert (buf[nq:].cpu().numpy() == 77).all()


def test_distances_above_two_to_the_31_compare_as_unsigned():
    nq, nr, D = 4, 70, 49152
    alt = np.tile(np.array([0, 255], dtype=np.uint8), D // 2)
    Q = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8), alt, 255 - alt])
    R = np.stack([(np.full(D, 255, np.uint8), np.zeros(D, np.uint8), 255 - alt, alt, np.full(D, 255, np.uint8))[j % 5] for j in range(nr)])
    far = 65025 * D                                      # all 0 against all 255
    half = far // 2                                      # against an alternating row
    assert far > 2 ** 31 > half
    thr = (far, far - 1, half, half - 1)
    got = _device_counts(Q, R, thr)
    assert np.array_equal(got, BB.count_within_host(Q, R, thr))
    # the all-zero query: 28 rows of 255 at `far`, 28 alternating rows at `half`, 14 duplicates
    assert got[0].tolist() == [70, 42, 42, 14] and got[1].tolist() == [70, 56, 56, 28]
    # a signed compare sees far as negative: far <= half - 1 would hold and far <= far - 1 as well


# ---- IN/OUT ---------------------------------------------------------------------------------------------------------------------------

def test_three_calls_over_thirds_equal_one_call_a_prefilled_buffer_is_added_to_and_a_rerun_repeats_the_bits():
    from csl_gan_amd import ops
    nq, nr, D = 300, 5000, 192
    Q, R, sets = _case(nq, nr, D)
    thr, want = sets[1] + sets[0], BB.count_within_host(Q, R, sets[1] + sets[0])
    q, qn = _prepared(Q)
    counts = torch.zeros((nq, 4), device=DEV, dtype=torch.int32)
    for s, e in ((3334, 5000), (0, 1667), (1667, 3334)):
        r, rn = _prepared(R[s:e])
        ops.nn_count(q, qn, r, rn, thr, counts)
    assert np.array_equal(counts.cpu().numpy(), want)
    pre = np.arange(nq * 4, dtype=np.int32).reshape(nq, 4)
    assert np.array_equal(_device_counts(Q, R, thr, counts=_dev(pre)), want + pre)
    assert np.array_equal(_device_counts(Q, R, thr), want) and np.array_equal(_device_counts(Q, R, thr), want)


def test_a_workgroup_that_counts_every_column_of_its_127_tiles():
    """The four counters of a row are the bytes of one register and grow by up to 2 per tile: 127 tiles are what a byte holds, and
    the entry caps a workgroup there.  One row tile and 127 * 1024 column tiles make every workgroup walk exactly 127 tiles, and
    identical rows make every lane count both of its columns in every one of them."""
    from csl_gan_amd import ops
    nr = 127 * 1024 * 128
    r, rn = ops.nn_prepare(torch.full((nr, 1), 7, device=DEV, dtype=torch.uint8))       # 1.06 GB at Dp = 64
    q, qn = _prepared(np.array([[7], [9], [200]], dtype=np.uint8))
    counts = torch.zeros((3, 4), device=DEV, dtype=torch.int32)
    ops.nn_count(q, qn, r, rn, (0, 4, 3, U32), counts)
    assert counts.cpu().numpy().tolist() == [[nr, nr, nr, nr], [0, nr, 0, nr], [0, 0, 0, nr]]
    # a ragged reference: the last range is short and its last tile has 5 columns
    counts.zero_()
    ops.nn_count(q, qn, r[:nr - 127 * 128 + 5], rn[:nr - 127 * 128 + 5], (0, 4, 3, U32), counts)
    assert counts[:, 3].cpu().numpy().tolist() == [nr - 127 * 128 + 5] * 3


def test_ops_nn_count_refuses_wrong_types_and_shapes_on_the_device():
    from csl_gan_amd import ops
    q, qn = _prepared(np.zeros((4, 8), dtype=np.uint8))
    ok = torch.zeros((4, 2), device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="int32"):
        ops.nn_count(q, qn, q, qn, (1, 2), ok.to(torch.int64))
    with pytest.raises(RuntimeError, match="shape"):
        ops.nn_count(q, qn, q, qn, (1, 2, 3), ok)
    for thr in ((), (1, 2, 3, 4, 5), (-1,), (2 ** 32,)):
        with pytest.raises(RuntimeError, match="thresholds"):
            ops.nn_count(q, qn, q, qn, thr, ok)
    assert not ok.any()


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def _cache(x):
    from csl_gan_amd.pipeline import CachedImages
    return CachedImages.from_arrays(x, np.zeros(len(x)), True)


def test_count_within_does_not_depend_on_block_rows_query_rows_or_the_device():
    rng = np.random.default_rng(21)
    R, Q = rng.integers(0, 256, (2500, 7, 5, 3), dtype=np.uint8), rng.integers(0, 256, (150, 7, 5, 3), dtype=np.uint8)
    R[2400], Q[9] = R[70], R[70]
    ref, qry = _cache(R), _cache(Q)
    thr = (1140000, 0, U32, 1000000)                     # d2 of random rows of 105 bytes: 1.15e6 +- 1e5
    want = NB.NearestSearch("cpu").fit(ref).count_within(qry, thr)
    assert want[9, 1] == 2 and (want[:, 2] == 2500).all() and 0 < want[:, 0].sum() < 150 * 2500
    for block_rows in (64, 1000, 2500):
        s = NB.NearestSearch(DEV, block_rows=block_rows, query_rows=64 if block_rows == 1000 else 16384).fit(ref)
        first = s.count_within(qry, thr)
        assert first.dtype == np.int64 and np.array_equal(first, want), block_rows
        assert np.array_equal(s.count_within(qry, thr), first)                   # against the resident reference
        assert np.array_equal(s.query(qry), NB.nearest_host(Q, R))               # which the search shares
    with pytest.raises(ValueError, match="one geometry"):
        s.count_within(_cache(np.zeros((3, 5, 7, 3), dtype=np.uint8)), thr)


def test_cli_on_the_device_agrees_with_the_cpu(tmp_path):
    from csl_gan_amd import sample_attack
    from csl_gan_amd.generate import CacheWriter
    rng = np.random.default_rng(22)
    d = str(tmp_path) + "/"
    x = {"train": rng.integers(0, 256, (700, 8, 8, 3), dtype=np.uint8), "heldout": rng.integers(0, 256, (300, 8, 8, 3), dtype=np.uint8),
         "syn": rng.integers(0, 256, (900, 8, 8, 3), dtype=np.uint8), "ref": rng.integers(0, 256, (90, 8, 8, 3), dtype=np.uint8)}
    x["syn"][:100] = x["train"][600:]
    x["syn"][:100, 0, 0, :] ^= 5
    for k, v in x.items():
        w = CacheWriter(d + k, len(v), 8, 8, 3, True, {"note": "test rows"})
        w(0, v, np.zeros(len(v), dtype=np.int64))
        w.close()
    runs = {}
    for dev in ("cpu", DEV):
        tag = dev.replace(":", "")
        runs[dev] = sample_attack.main(["--syn_cache", d + "syn", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "--calib_cache", d + "ref",
                                        "-d", dev, "--block_rows", "256", "--pool", "200", "--asr_iters", "300", "--values_dir", d + "values_" + tag])
    assert json.dumps(runs["cpu"], sort_keys=True) == json.dumps(runs[DEV], sort_keys=True)
    assert runs["cpu"]["syn"]["fbb"]["tpr_at_fpr_0.001"] >= 100 / 700 and runs["cpu"]["syn"]["d2min_pooled"]["d2_min"] <= 75
    names = sorted(os.listdir(d + "values_cpu"))
    assert len(names) == 6 and names == sorted(os.listdir(d + "values_cuda0"))
    for f in names:
        a, b = np.load(d + "values_cpu/" + f), np.load(d + "values_cuda0/" + f)
        assert a.dtype == np.int64 == b.dtype and np.array_equal(a, b)
