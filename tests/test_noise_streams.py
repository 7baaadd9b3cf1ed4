"""The host model of the device noise streams (oracle/noise_streams.py) and the keying it restates (include/cslgan.h "Device random
streams"): Philox known answers, no Philox input used twice inside a run, distinct seeds for every rank and for the two kernels
that draw, and the refusal of a call that would leave the domain the keying is unique on.  The device side of the same model is
tests/test_noise_streams_gpu.py."""

import numpy as np
import pytest
import torch

from oracle import noise_streams as NS

# Random123 known-answer vectors for philox4x32 with 10 rounds (kat_vectors: counter, key -> output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

TENSOR_COUNTS = [1, 9, 16, 17, 33, 64]
CALLS = [0, 1, 2, 63, 64, 2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1, 2 ** 26]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    got = NS.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == out


def test_philox_is_vectorised_over_counters():
    """Arrays of counters give what the scalar calls give (the model is used on whole tensors)."""
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint64)
    for key in ((0, 0), (0xa4093822, 0x299f31d0)):
        got = NS.philox4x32_10(ctrs[:, 0], ctrs[:, 1], ctrs[:, 2], ctrs[:, 3], *key)
        for r in range(len(KAT)):
            assert tuple(int(w[r]) for w in got) == tuple(int(w) for w in NS.philox4x32_10(*KAT[r][0], *key))
    assert tuple(int(w[0]) for w in got) != KAT[0][2]          # the key matters
    q = np.arange(5, dtype=np.uint64)
    a = NS.philox4x32_10(q, 0, 7, 0, 1, 2)                       # scalars broadcast against the counter array
    assert all(a[w].shape == (5,) for w in range(4)) and len({int(x) for x in a[0]}) == 5


def test_box_muller_grid_and_bound():
    """u1 lies on a 2^-24 grid offset by 2^-25, so |z| <= sqrt(-2 ln 2^-25) = 5.887; word pairs map to columns 4q .. 4q+3."""
    z0, z1 = NS.box_muller(np.array([0, 0xFFFFFFFF, 0x80000000]), np.array([0, 0, 0x40000000]))
    bound = np.sqrt(-2.0 * np.log(2.0 ** -25))
    assert z0[0] == pytest.approx(bound, rel=1e-12) and z1[0] == 0.0 and 5.88 < bound < 5.89
    assert z0[1] == pytest.approx(np.sqrt(-2.0 * np.log(1.0 - 2.0 ** -25)), rel=1e-9)            # the smallest radius: 2.44e-4
    assert abs(z0[2]) < 1e-12 and z1[2] == pytest.approx(np.sqrt(-2.0 * np.log(0.5 + 2.0 ** -25)), rel=1e-12)    # u2 = 1/4
    words = NS.philox4x32_10(np.arange(3, dtype=np.uint64), 0, 5, 0, 123, 0)
    z = NS.normals_of_words(words, 10)
    a, b = NS.box_muller(words[0], words[1])
    c, d = NS.box_muller(words[2], words[3])
    assert z.shape == (10,) and np.array_equal(z[0:4], [a[0], b[0], c[0], d[0]]) and np.array_equal(z[8:10], [a[2], b[2]])
    assert abs(a[0] - c[0]) > 1e-6                                # the second pair is a draw of its own


def test_model_moments():
    """The model's own stream is N(0, 1) (a restatement that mis-scaled u1 or u2 would show here, before any device run)."""
    z = NS.clip_noise_normals([1 << 20], seed=123, offset=0)[0]
    assert abs(z.mean()) < 4e-3 and abs(z.std() - 1.0) < 3e-3 and abs((z ** 4).mean() - 3.0) < 0.05
    assert abs((z[:-1] * z[1:]).mean()) < 4e-3 and abs((z[0::4] * z[2::4]).mean()) < 8e-3


def test_raw_abi_and_python_entry_offsets_agree():
    """ops.clip_accum_noise(offset=o) launches with 64 * o + first_index; the counter in HBM adds 64 per call either way."""
    assert NS.clip_off64(3, call_counter=2, first_index=16) == 64 * 5 + 16 == NS.clip_off64(64 * 3 + 16, call_counter=2, raw=True)
    assert NS.clip_counter_words(5, 2 ** 24) == (5, 1)                  # the offset carries into the fourth counter word
    assert NS.clip_counter_words(5, 2 ** 24 - 1) == (5 + 0xFFFFFF00, 0)
    a = NS.clip_noise_normals([8], 9, offset=1, first_index=3)[0]
    b = NS.clip_noise_normals([8], 9, offset=67, raw=True)[0]
    assert np.array_equal(a, b)
    assert NS.clip_launches(["f32"] * 17) == [(0, list(range(16))), (16, [16])]
    assert NS.clip_launches(["f32", "bf16"] * 2) == [(0, [0, 2]), (1, [1, 3])]


def _all_distinct(keys):
    return len(set(keys)) == len(keys)


@pytest.mark.parametrize("n_tensors", TENSOR_COUNTS)
def test_no_gradient_noise_key_is_used_twice(n_tensors):
    """One rank, offset 0 and the call counter in HBM as the engines launch it: every (call, tensor) has its own (c2, c3).  2^18
    calls is where the stream offset reaches 2^24 and carries into c3; at 2^26 its low part has long wrapped in c2."""
    keys = NS.clip_keys(seed=1, calls=CALLS, n_tensors=n_tensors)
    assert len(keys) == n_tensors * len(CALLS) and _all_distinct(keys)
    # the keying is injective on its whole domain (s < 16, first_index < 64, off64 < 2^56), not only on the calls listed: (c2, c3)
    # gives back (s, off64)
    rng = np.random.default_rng(n_tensors)
    off64 = rng.integers(0, 2 ** 56, size=4096, dtype=np.uint64)
    s = rng.integers(0, 16, size=4096, dtype=np.uint64)
    c2, c3 = NS.clip_counter_words(s, off64)
    assert np.array_equal(c2 & np.uint64(0xFF), s) and np.array_equal((c3 << np.uint64(24)) | (c2 >> np.uint64(8)), off64)


def test_no_key_is_used_twice_in_a_mixed_fp32_bf16_list():
    """Two launches (one per element type), first_index = the position of each launch's first tensor in the caller's list."""
    for dtypes in (["f32", "bf16"] * 9, ["bf16"] + ["f32"] * 20 + ["bf16"] * 20, ["f32", "bf16"] * 32):
        keys = NS.clip_keys(seed=1, calls=CALLS, dtypes=dtypes)
        assert len(keys) == len(dtypes) * len(CALLS) and _all_distinct(keys)


def test_position_64_would_repeat_the_next_call():
    """The hole the 64-tensor limit closes: tensor 64 of call k has the stream of tensor 0 of call k + 1."""
    a = NS.clip_counter_words(0, NS.clip_off64(0, call_counter=0, first_index=64))
    b = NS.clip_counter_words(0, NS.clip_off64(0, call_counter=1, first_index=0))
    assert a == b == (16384, 0)
    with pytest.raises(ValueError):
        NS.clip_keys(seed=1, calls=[0], n_tensors=65)


@pytest.mark.parametrize("n_tensors", [9, 64])
def test_gradient_noise_and_mean_sampler_share_no_key(n_tensors):
    """A rank's gradient-noise streams and its mean sampler's (draws 1 .. 2 * calls: two per D-step, in the layout of the flagship
    run: 128 images from 32 mean samples) as the trainer seeds them: all distinct inside each, disjoint between them."""
    ck, mk = NS.keys_of_run(manual_seed=1, rank=0, calls=range(64), n_tensors=n_tensors)
    assert _all_distinct(ck) and _all_distinct(mk) and not set(ck) & set(mk)
    far = [2 * c + d for c in CALLS for d in (1, 2)] + [2 ** 32 + 1, 2 ** 32 + 2]
    ck, mk = NS.keys_of_run(manual_seed=1, rank=0, calls=CALLS, n_tensors=n_tensors, n_classes=3, ms_batch=70, ms_offsets=far)
    assert _all_distinct(ck) and _all_distinct(mk) and not set(ck) & set(mk)
    # what keeps them apart is the seed alone: under ONE seed the sampler's pixel stream of image 0, draw 1 is (c1, c2, c3) =
    # (0, 1, 0), which is tensor 1 of the engine's call 0 — the header says so, and test_seeds_* hold the seeds apart
    same = NS.mean_sample_keys(NS.engine_seed(1), [1], 128, 32)
    assert set(NS.clip_keys(NS.engine_seed(1), [0], n_tensors=9)) & set(same) == {(1, 0, 1, 0)}


@pytest.mark.parametrize("manual_seed", [0, 1, 1000000])
def test_seeds_of_ranks_and_kernels_are_distinct(manual_seed):
    """--manual_seed s (the default draws one from 1 .. 10^6): rank r's engine seed is s + 7919 r (Trainer.setup_privacy_engine); the
    mean sampler's is its process seed (s, or s + 7919 r once a --dist run re-seeded the rank) xor a 64-bit tag."""
    eng = [NS.engine_seed(manual_seed, r) for r in range(8)]
    assert len(set(eng)) == 8
    ms = {NS.mean_sampler_seed(NS.process_seed(manual_seed, r, dist)) for r in range(8) for dist in (False, True)}
    assert len(ms) == 8 and not ms & set(eng)
    # ... and no engine seed of ANY seed the option can take meets a sampler seed: the tag sets bits far above 10^6 + 7919 * 7
    assert all(0 <= e < 2 ** 32 for e in eng) and min(ms) > 2 ** 62


def test_model_seeds_are_the_trainers():
    """The seed formulas above are restated from the product; hold the restatement to the product's own text."""
    import inspect
    from csl_gan_amd import mean_sampler, trainer
    assert "pe._set_seed(o.manual_seed + %d * self.rank)" % NS.RANK_SEED_STRIDE in inspect.getsource(trainer.Trainer.setup_privacy_engine)
    assert "^ 0x%X" % NS.MEAN_SAMPLER_SEED_TAG in inspect.getsource(mean_sampler.MeanSampler.sample)


@pytest.mark.parametrize("n,dtypes", [(65, None), (80, None), (66, "mixed")])
def test_more_than_64_tensors_with_philox_noise_are_refused(n, dtypes):
    """ops.clip_accum_noise refuses the call before anything is launched (no device is needed to see it)."""
    from csl_gan_amd import ops
    mats = [torch.zeros(1, 4, dtype=(torch.bfloat16 if (dtypes and i % 2) else torch.float32)) for i in range(n)]
    outs = [torch.zeros(4) for _ in range(n)]
    with pytest.raises(RuntimeError, match="at most 64 tensors"):
        ops.clip_accum_noise(mats, outs, noise_std=torch.ones(n), seed=1, offset=0)
    assert all(float(o.abs().sum()) == 0.0 for o in outs)
