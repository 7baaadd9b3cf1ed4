"""csl_gan_amd.neighbours / csl_gan_amd.nearest without a GPU: the host model against a plain integer double loop, the tie and range
rules, merging, the metrics on inputs worked out by hand, the command line on -d cpu, and the host-side argument checks of the two
C-ABI entries.  Every comparison of keys is integer equality."""
import json
import os

import numpy as np
import pytest
import torch

from csl_gan_amd import neighbours as NB

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _loop_keys(Q, R, base=0):
    """The definition, one pair at a time in Python integers."""
    out = []
    for q in Q.reshape(len(Q), -1).astype(np.int64):
        best = 2 ** 64 - 1
        for j, r in enumerate(R.reshape(len(R), -1).astype(np.int64)):
            d2 = int(((q - r) ** 2).sum())
            best = min(best, (d2 << 32) | (base + j))
        out.append(best)
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("nq,nr,D", [(1, 1, 1), (5, 7, 3), (9, 4, 63), (6, 11, 130)])
def test_host_model_equals_a_double_loop(nq, nr, D):
    rng = np.random.default_rng(100 + D)
    Q, R = rng.integers(0, 256, (nq, D), dtype=np.uint8), rng.integers(0, 256, (nr, D), dtype=np.uint8)
    assert np.array_equal(NB.nearest_host(Q, R), _loop_keys(Q, R))
    assert np.array_equal(NB.nearest_host(Q, R, index_base=1000, block=3), _loop_keys(Q, R, 1000))


def test_planted_duplicates_have_distance_zero_and_the_right_index():
    rng = np.random.default_rng(1)
    R = rng.integers(0, 256, (40, 4, 4, 3), dtype=np.uint8)
    Q = rng.integers(0, 256, (6, 4, 4, 3), dtype=np.uint8)
    Q[1], Q[4] = R[33], R[0]
    d2, idx = NB.split_keys(NB.nearest_host(Q, R))
    assert (d2[1], idx[1]) == (0, 33) and (d2[4], idx[4]) == (0, 0)
    assert (d2[[0, 2, 3, 5]] > 0).all()


def test_ties_go_to_the_smallest_index():
    rng = np.random.default_rng(2)
    R = rng.integers(0, 256, (30, 50), dtype=np.uint8)
    R[21] = R[8]
    Q = R[[8]].copy()
    Q[0, 0] ^= 1                                       # distance 1 to rows 8 and 21 alike
    d2, idx = NB.split_keys(NB.nearest_host(Q, R))
    assert (d2[0], idx[0]) == (1, 8)
    d2, idx = NB.split_keys(NB.nearest_host(Q, R, block=4))          # rows 8 and 21 in different blocks
    assert (d2[0], idx[0]) == (1, 8)


def test_distances_above_two_to_the_31_are_exact():
    Q = np.zeros((1, 65536), dtype=np.uint8)
    R = np.full((3, 65536), 255, dtype=np.uint8)
    d2, idx = NB.split_keys(NB.nearest_host(Q, R))
    assert d2[0] == 4261478400 == 255 * 255 * 65536 and d2[0] > 2 ** 31 and idx[0] == 0


def test_merging_keeps_the_smaller_keys():
    rng = np.random.default_rng(3)
    Q, R = rng.integers(0, 256, (8, 20), dtype=np.uint8), rng.integers(0, 256, (12, 20), dtype=np.uint8)
    plain = NB.nearest_host(Q, R)
    best = np.full(8, NONE, dtype=np.uint64)
    best[2], best[5] = np.uint64(7), plain[5] + np.uint64(1)
    merged = NB.nearest_host(Q, R, best=best)
    assert merged[2] == 7 and merged[5] == plain[5]
    assert np.array_equal(np.delete(merged, 2), np.delete(plain, 2))
    assert best[2] == 7 and best[0] == NONE            # the argument is not written


def test_two_calls_with_index_base_equal_one_call():
    rng = np.random.default_rng(4)
    Q, R = rng.integers(0, 256, (10, 33), dtype=np.uint8), rng.integers(0, 256, (25, 33), dtype=np.uint8)
    R[20] = R[3]
    Q[0] = R[3]
    one = NB.nearest_host(Q, R)
    two = NB.nearest_host(Q, R[11:], index_base=11, best=NB.nearest_host(Q, R[:11]))
    rev = NB.nearest_host(Q, R[:11], best=NB.nearest_host(Q, R[11:], index_base=11))
    assert np.array_equal(one, two) and np.array_equal(one, rev)
    assert NB.split_keys(one)[1][0] == 3


@pytest.mark.parametrize("block", [1, 2, 7, 64, 10 ** 6])
def test_block_size_does_not_matter(block):
    rng = np.random.default_rng(5)
    Q, R = rng.integers(0, 256, (13, 48), dtype=np.uint8), rng.integers(0, 256, (29, 48), dtype=np.uint8)
    assert np.array_equal(NB.nearest_host(Q, R, block=block), _loop_keys(Q, R))


def test_host_model_refuses_what_the_keys_cannot_hold():
    z = np.zeros((2, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match="2\\^32"):
        NB.nearest_host(z, z, index_base=2 ** 32 - 2)
    with pytest.raises(ValueError):
        NB.nearest_host(z, np.zeros((2, 5), dtype=np.uint8))
    with pytest.raises(ValueError):
        NB.nearest_host(z.astype(np.int8), z)
    assert NB.nearest_host(z, z, index_base=2 ** 32 - 3)[0] == np.uint64(2 ** 32 - 3)


def _key(d2, idx):
    return (np.uint64(d2) << np.uint64(32)) | np.uint64(idx)


def test_metrics_on_hand_computed_inputs():
    # train distances 0 9 4 0 25 16 100 1 ; held-out distances 1 9 5 3 16 16 400 0
    dt = [0, 9, 4, 0, 25, 16, 100, 1]
    dh = [1, 9, 5, 3, 16, 16, 400, 0]
    kt = np.array([_key(d, 10 + i) for i, d in enumerate(dt)], dtype=np.uint64)
    kh = np.array([_key(d, 90 - i) for i, d in enumerate(dh)], dtype=np.uint64)
    m = NB.dcr_metrics(kt)
    # sorted: 0 0 1 4 9 16 25 100 ; element floor(p * 7): p = 0, .01, .05 -> 0 ; p = .5 -> element 3 = 4
    assert m == {"n": 8, "duplicates": 2, "d2_min": 0, "dcr_min": 0.0, "d2_p01": 0, "dcr_p01": 0.0, "d2_p05": 0, "dcr_p05": 0.0, "d2_p50": 4,
                 "dcr_p50": 2.0 / 255.0}
    m = NB.dcr_metrics(kt, kh)
    # strictly closer to train: rows 0, 2, 3, 6 -> 4 ; ties: rows 1, 5 -> 2 halves ; share (4 + 1) / 8
    assert m["closer_to_train"] == 4 and m["ties"] == 2 and m["closer_to_train_share"] == 0.625
    assert m["closer_to_train_stderr"] == pytest.approx((0.625 * 0.375 / 8) ** 0.5, rel=1e-15)
    # held-out sorted: 0 1 3 5 9 16 16 400
    assert m["heldout_duplicates"] == 1 and m["heldout_d2_min"] == 0 and m["heldout_d2_p50"] == 5 and m["heldout_dcr_p50"] == 5 ** 0.5 / 255.0
    assert m["d2_p50"] == 4 and m["duplicates"] == 2
    big = NB.dcr_metrics(np.array([_key(4261478400, 2 ** 32 - 2)], dtype=np.uint64))
    assert big["d2_min"] == 4261478400 and big["dcr_p50"] == 4261478400 ** 0.5 / 255.0
    with pytest.raises(ValueError):
        NB.dcr_metrics(kt, kh[:3])


def test_order_statistics_follow_the_stated_rule():
    d = np.arange(1000, 0, -1)                          # 1 .. 1000 shuffled by order: sorted element k is k + 1
    m = NB.dcr_metrics(np.array([_key(v, 0) for v in d], dtype=np.uint64))
    assert (m["d2_min"], m["d2_p01"], m["d2_p05"], m["d2_p50"]) == (1, 10, 50, 500)     # floor(.01 * 999) = 9, 49, 499


def test_nearest_search_on_the_cpu_is_the_host_model():
    from csl_gan_amd.pipeline import CachedImages
    rng = np.random.default_rng(6)
    ref = CachedImages.from_arrays(rng.integers(0, 256, (37, 5, 4, 3), dtype=np.uint8), np.zeros(37), False)
    qry = CachedImages.from_arrays(rng.integers(0, 256, (9, 5, 4, 3), dtype=np.uint8), np.zeros(9), False)
    s = NB.NearestSearch("cpu", block_rows=8).fit(ref)
    assert np.array_equal(s.query(qry), _loop_keys(qry.x, ref.x))
    other = CachedImages.from_arrays(np.zeros((2, 4, 5, 3), dtype=np.uint8), np.zeros(2), False)
    with pytest.raises(ValueError, match="one geometry"):
        s.query(other)
    with pytest.raises(RuntimeError, match="fit"):
        NB.NearestSearch("cpu").query(qry)


# ---- the command line on the CPU ------------------------------------------------------------------------------------------------------

N_SYN, N_TRAIN, N_HELD, HWC = 12, 29, 17, (6, 5, 3)


def _write(path, x):
    from csl_gan_amd.generate import CacheWriter
    n, H, W, C = x.shape
    w = CacheWriter(path, n, H, W, C, True, {"note": "test rows"})
    w(0, x, np.zeros(n, dtype=np.int64))
    w.close()


@pytest.fixture(scope="module")
def caches(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("nearest")) + "/"
    rng = np.random.default_rng(7)
    x = {"train": rng.integers(0, 256, (N_TRAIN,) + HWC, dtype=np.uint8), "heldout": rng.integers(0, 256, (N_HELD,) + HWC, dtype=np.uint8),
         "syn": rng.integers(0, 256, (N_SYN,) + HWC, dtype=np.uint8), "syn2": rng.integers(0, 256, (5,) + HWC, dtype=np.uint8)}
    x["syn"][3] = x["train"][20]                        # a memorised sample
    x["syn"][7] = x["heldout"][2]
    for k, v in x.items():
        _write(d + k, v)
    _write(d + "odd", rng.integers(0, 256, (4, 5, 6, 3), dtype=np.uint8))
    return d, x


def test_cli_on_the_cpu(caches, tmp_path, capsys):
    from csl_gan_amd import nearest
    d, x = caches
    out, vals = str(tmp_path / "outputs"), str(tmp_path / "values")
    stats = nearest.main(["--syn_cache", d + "syn", d + "syn2", "--train_cache", d + "train", "--nontrain_cache", d + "heldout", "-d", "cpu",
                          "--baseline", "--grid", "4", "--values_dir", vals, "--save", "--outputs_dir", out, "--name", "audit"])
    assert set(stats) == {"syn", "syn2", "baseline_heldout_to_train"}
    kt, kh = _loop_keys(x["syn"], x["train"]), _loop_keys(x["syn"], x["heldout"])
    assert stats["syn"] == NB.dcr_metrics(kt, kh)
    assert stats["syn"]["n"] == N_SYN and stats["syn"]["duplicates"] == 1 and stats["syn"]["heldout_duplicates"] == 1 and stats["syn"]["d2_min"] == 0
    for f in ("closer_to_train_share", "closer_to_train_stderr", "d2_p01", "d2_p05", "d2_p50", "dcr_p50", "heldout_d2_p50", "ties", "closer_to_train"):
        assert f in stats["syn"]
    assert stats["syn2"] == NB.dcr_metrics(_loop_keys(x["syn2"], x["train"]), _loop_keys(x["syn2"], x["heldout"]))
    assert stats["baseline_heldout_to_train"] == NB.dcr_metrics(_loop_keys(x["heldout"], x["train"]))
    # the saved keys
    assert np.array_equal(np.load(os.path.join(vals, "syn_keys_train.npy")), kt) and np.load(os.path.join(vals, "syn_keys_train.npy")).dtype == np.uint64
    assert np.array_equal(np.load(os.path.join(vals, "syn_keys_heldout.npy")), kh)
    assert np.array_equal(np.load(os.path.join(vals, "baseline_keys_train.npy")), _loop_keys(x["heldout"], x["train"]))
    assert NB.split_keys(kt)[1][3] == 20 and NB.split_keys(kh)[1][7] == 2
    # the JSON on disk is what was returned, and a second run merges into it
    with open(os.path.join(out, "audit.json")) as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    nearest.main(["--syn_cache", d + "heldout", "--train_cache", d + "train", "-d", "cpu", "--save", "--outputs_dir", out, "--name", "audit"])
    with open(os.path.join(out, "audit.json")) as f:
        merged = json.load(f)
    assert set(merged) == {"syn", "syn2", "baseline_heldout_to_train", "heldout"} and "closer_to_train_share" not in merged["heldout"]
    assert merged["heldout"]["d2_p50"] == stats["baseline_heldout_to_train"]["d2_p50"]
    # the picture: 4 rows of synthetic | train | held-out, util.make_grid's 2-pixel padding
    from PIL import Image
    img = Image.open(os.path.join(out, "audit_syn_nearest.png"))
    H, W, _ = HWC
    assert img.size == (3 * (W + 2) + 2, 4 * (H + 2) + 2) and img.mode == "RGB"
    a = np.asarray(img)
    # first row: the memorised sample (key 0 sorts first) beside the training image it copies
    assert np.array_equal(a[2:2 + H, 2:2 + W], x["syn"][3]) and np.array_equal(a[2:2 + H, 4 + W:4 + 2 * W], x["train"][20])
    assert os.path.exists(os.path.join(out, "audit_syn2_nearest.png"))


def test_cli_refuses_mismatched_geometry_and_a_baseline_without_a_held_out_set(caches, tmp_path):
    from csl_gan_amd import nearest
    d, _ = caches
    with pytest.raises(SystemExit, match="one geometry"):
        nearest.main(["--syn_cache", d + "odd", "--train_cache", d + "train", "-d", "cpu"])
    with pytest.raises(SystemExit, match="one geometry"):
        nearest.main(["--syn_cache", d + "syn", "--train_cache", d + "train", "--nontrain_cache", d + "odd", "-d", "cpu"])
    with pytest.raises(SystemExit, match="nontrain_cache"):
        nearest.main(["--syn_cache", d + "syn", "--train_cache", d + "train", "--baseline", "-d", "cpu"])


# ---- host-side argument checks of the entries -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from csl_gan_amd import build, _lib
    build.build()
    return _lib.lib()


def test_the_entries_are_exported(L):
    from csl_gan_amd import _lib
    assert {"cslgan_nn_padded_dim", "cslgan_nn_prepare_u8", "cslgan_nn_min_i8"} <= set(_lib.EXPORTS)
    for D, Dp in ((1, 64), (63, 64), (64, 64), (65, 128), (784, 832), (12288, 12288), (65536, 65536), (0, 0), (65537, 0), (-3, 0)):
        assert L.cslgan_nn_padded_dim(D) == Dp
    from csl_gan_amd import ops
    assert ops.nn_padded_dim(784) == 832


def test_nn_prepare_refuses_bad_arguments_before_any_launch(L):
    err = lambda: L.cslgan_last_error()
    ok = dict(x=64, rows=4, D=63, Dp=64, xs=64, sq=64)
    call = lambda **kw: L.cslgan_nn_prepare_u8(*[dict(ok, **kw)[k] for k in ("x", "rows", "D", "Dp", "xs", "sq")], None)
    for k in ("x", "xs", "sq"):
        assert call(**{k: None}) == -1 and b"null" in err()
    assert call(D=0) == -1 and b"D=0" in err()
    assert call(D=65537, Dp=65600) == -1 and b"D=65537" in err()
    assert call(Dp=128) == -1 and b"Dp=128" in err()
    assert call(Dp=63) == -1 and b"Dp=63" in err()
    assert call(rows=0) == -1 and b"rows=0" in err()
    assert call(rows=2 ** 31) == -1 and b"rows=2147483648" in err()
    assert call(x=72) == -1 and b"misaligned" in err()
    assert call(xs=68) == -1 and b"misaligned" in err()
    assert call(sq=66) == -1 and b"misaligned" in err()


def test_nn_min_refuses_bad_arguments_before_any_launch(L):
    err = lambda: L.cslgan_last_error()
    ok = dict(q=64, qn=64, nq=4, r=64, rn=64, nr=9, Dp=128, base=0, best=64)
    call = lambda **kw: L.cslgan_nn_min_i8(*[dict(ok, **kw)[k] for k in ("q", "qn", "nq", "r", "rn", "nr", "Dp", "base", "best")], None)
    for k in ("q", "qn", "r", "rn", "best"):
        assert call(**{k: None}) == -1 and b"null" in err()
    assert call(Dp=0) == -1 and b"Dp=0" in err()
    assert call(Dp=96) == -1 and b"Dp=96" in err()
    assert call(Dp=65600) == -1 and b"Dp=65600" in err()
    assert call(nq=0) == -1 and b"nq=0" in err()
    assert call(nr=0) == -1 and b"nr=0" in err()
    assert call(nq=2 ** 31) == -1 and b"nq=2147483648" in err()
    assert call(base=-1) == -1 and b"index_base" in err()
    assert call(base=2 ** 32 - 9) == -1 and b"4294967296" in err()          # index_base + nr = 2^32: one too many
    assert call(q=72) == -1 and b"misaligned" in err()
    assert call(r=8) == -1 and b"misaligned" in err()
    assert call(qn=66) == -1 and b"misaligned" in err()
    assert call(rn=65) == -1 and b"misaligned" in err()
    assert call(best=68) == -1 and b"misaligned" in err()


def test_the_ops_refuse_cpu_tensors_and_wrong_types():
    from csl_gan_amd import ops
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.nn_prepare(torch.zeros(4, 8, dtype=torch.uint8))
    z8, z32, z64 = torch.zeros(4, 64, dtype=torch.int8), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.nn_min(z8, z32, z8, z32, 0, z64)
    with pytest.raises(RuntimeError, match="nn_min: best must be a contiguous int64 tensor"):
        ops.nn_min(z8, z32, z8, z32, 0, z32)
