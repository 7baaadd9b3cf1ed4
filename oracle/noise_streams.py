"""Host model of the device noise streams (numpy only).  TEST INFRASTRUCTURE: nothing under csl_gan_amd/ imports it.

A plain restatement, from the layout documented in include/cslgan.h ("Device random streams"), of what the two kernels that
draw on the device produce: the Gaussian gradient noise of cslgan_clip_accum_noise_* and the permutations, labels, per-image
jitter and per-pixel noise of cslgan_mean_sample_f32.  Integers are uint64 numpy holding 32-bit words, the normals float64.
philox4x32_10 is held to the Random123 known-answer vectors by tests/test_noise_streams.py, so it does not depend on the kernel
it is compared with.

    gradient noise, tensor s of a launch, column j (q = j >> 2, word pair (j & 3) >> 1, Box-Muller output j & 1):
        counter (q lo, q hi, s + (off64 << 8 mod 2^32), off64 >> 24)      key (seed lo, seed hi)
        off64 = offset + 64 * call_counter                         (C ABI: `offset` as passed)
              = 64 * offset + first_index + 64 * call_counter      (csl_gan_amd.ops.clip_accum_noise: first_index is the position,
                                                                    in the caller's list, of the first tensor of the launch)
    mean sampler, draw `offset`, image i (off lo / off hi = the 32-bit halves of offset):
        permutation keys  (j, i / num_samples, off lo, 0x7065726D ^ off hi)  word 0, ranked (stable) over j < num_samples
        label             (i, 0x6C61626C, off lo, off hi)                     mulhi(word 0, n_classes)
        jitter            (i, 0xFFFFFFFF, off lo, off hi)                     first Box-Muller output of words 0, 1
        pixels 4q..4q+3   (q, i, off lo, off hi)                              as the gradient noise
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
MAX_SEGS = 16                    # tensors per launch (CSLGAN_MAX_SEGS)
MAX_TENSORS = 64                 # tensors per ops.clip_accum_noise call with Philox noise: first_index < 64
PERM_TAG, LABEL_TAG, JITTER_TAG = 0x7065726D, 0x6C61626C, 0xFFFFFFFF
MEAN_SAMPLER_SEED_TAG = 0x6D65616E73616D70
RANK_SEED_STRIDE = 7919


def _u64(x):
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF)
    return np.asarray(x).astype(np.uint64)


def _w32(x):
    return _u64(x) & _M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11; Random123 philox4x32_R(10, ...)).  Counters broadcast against each other;
    returns the four output words as uint64 arrays of 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(_w32(c0), _w32(c1), _w32(c2), _w32(c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                       # 32 x 32 -> 64 bit products: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def box_muller(a, b, dtype=np.float64):
    """Two unit normals from two 32-bit words: u1 = (a >> 8) 2^-24 + 2^-25 in (0, 1), u2 = (b >> 8) 2^-24 in [0, 1).
    dtype=np.float32 restates the same formula in single precision (the tests measure its distance to float64 with it)."""
    dt = np.dtype(dtype).type
    u1 = (_u64(a) >> np.uint64(8)).astype(dtype) * dt(1.0 / 16777216.0) + dt(0.5 / 16777216.0)
    u2 = (_u64(b) >> np.uint64(8)).astype(dtype) * dt(1.0 / 16777216.0)
    r = np.sqrt(dt(-2.0) * np.log(u1))
    t = dt(6.283185307179586) * u2
    return r * np.cos(t), r * np.sin(t)


def normals_of_words(words, length, dtype=np.float64):
    """Counter q -> columns 4q (words 0, 1: cos), 4q+1 (sin), 4q+2 (words 2, 3: cos), 4q+3 (sin); the first `length` columns."""
    z0, z1 = box_muller(words[0], words[1], dtype)
    z2, z3 = box_muller(words[2], words[3], dtype)
    return np.stack([z0, z1, z2, z3], axis=-1).reshape(z0.shape[:-1] + (-1,))[..., :length]


def seed_words(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


# ---- gradient noise (cslgan_clip_accum_noise_f32 / _bf16) ------------------------------------------------------------------

def clip_off64(offset, call_counter=0, first_index=0, raw=False):
    """The 64-bit stream offset of one launch.  raw: `offset` is the C ABI's argument; else it is ops.clip_accum_noise's."""
    base = int(offset) if raw else 64 * int(offset) + int(first_index)
    return (base + 64 * int(call_counter)) & 0xFFFFFFFFFFFFFFFF


def clip_counter_words(s, off64):
    """(c2, c3) of segment s of a launch at stream offset off64 (arrays allowed)."""
    off64 = _u64(off64)
    return (_u64(s) + ((off64 << np.uint64(8)) & _M32)) & _M32, (off64 >> np.uint64(24)) & _M32


def clip_noise_normals(lens, seed, offset, call_counter=0, first_index=0, raw=False, dtype=np.float64):
    """The unit normals one launch of cslgan_clip_accum_noise_* draws: a list with one [len] array per segment."""
    if len(lens) > MAX_SEGS:
        raise ValueError("a launch has at most %d segments" % MAX_SEGS)
    k0, k1 = seed_words(seed)
    off64 = clip_off64(offset, call_counter, first_index, raw)
    out = []
    for s, n in enumerate(lens):
        q = np.arange((int(n) + 3) // 4, dtype=np.uint64)
        c2, c3 = clip_counter_words(s, off64)
        out.append(normals_of_words(philox4x32_10(q, q >> np.uint64(32), c2, c3, k0, k1), int(n), dtype))
    return out


def clip_launches(dtypes):
    """How ops.clip_accum_noise splits a caller's tensor list: one group per element type, launches of at most MAX_SEGS tensors;
    -> [(first_index, [positions in the caller's list])], first_index = the position of the launch's first tensor."""
    groups = {}
    for i, dt in enumerate(dtypes):
        groups.setdefault(dt, []).append(i)
    out = []
    for idx in groups.values():
        for i in range(0, len(idx), MAX_SEGS):
            out.append((idx[i], idx[i:i + MAX_SEGS]))
    return out


def clip_call_normals(lens, seed, offset, call_counter=0, dtypes=None, dtype=np.float64):
    """The unit normals of one ops.clip_accum_noise call, in the order of the caller's list."""
    dtypes = ["f32"] * len(lens) if dtypes is None else list(dtypes)
    out = [None] * len(lens)
    for first, idx in clip_launches(dtypes):
        for j, z in zip(idx, clip_noise_normals([lens[j] for j in idx], seed, offset, call_counter, first, dtype=dtype)):
            out[j] = z
    return out


# ---- mean sampler (cslgan_mean_sample_f32) ----------------------------------------------------------------------------------

def mean_sample_draws(n, num_samples, n_classes, length, seed, offset, dtype=np.float64):
    """-> dict(perms [n] int64, labels [n] int64, jitter [n], pixel [n, length]) for draw `offset`."""
    k0, k1 = seed_words(seed)
    off = int(offset) & 0xFFFFFFFFFFFFFFFF
    lo, hi = off & 0xFFFFFFFF, off >> 32
    i = np.arange(n, dtype=np.uint64)
    reps = (n + num_samples - 1) // num_samples
    j = np.arange(num_samples, dtype=np.uint64)
    perms = np.empty(reps * num_samples, dtype=np.int64)
    for rep in range(reps):
        key = philox4x32_10(j, rep, lo, PERM_TAG ^ hi, k0, k1)[0]
        # position p of the permutation holds the sample whose key has rank p; equal keys rank by index (stable)
        perms[rep * num_samples:(rep + 1) * num_samples] = np.argsort(key, kind="stable")
    labels = (philox4x32_10(i, LABEL_TAG, lo, hi, k0, k1)[0] * np.uint64(n_classes)) >> np.uint64(32)
    jw = philox4x32_10(i, JITTER_TAG, lo, hi, k0, k1)
    jitter = box_muller(jw[0], jw[1], dtype)[0]
    q = np.arange((length + 3) // 4, dtype=np.uint64)
    pixel = normals_of_words(philox4x32_10(q[None, :], i[:, None], lo, hi, k0, k1), length, dtype)
    return dict(perms=perms[:n], labels=labels.astype(np.int64), jitter=jitter, pixel=pixel)


# ---- seeds -----------------------------------------------------------------------------------------------------------------

def engine_seed(manual_seed, rank=0):
    """Trainer.setup_privacy_engine: the gradient-noise seed of a rank."""
    return int(manual_seed) + RANK_SEED_STRIDE * int(rank)


def process_seed(manual_seed, rank=0, distributed=False):
    """torch's default-generator seed of a rank: options.parse seeds with --manual_seed; a --dist run re-seeds every rank."""
    return int(manual_seed) + (RANK_SEED_STRIDE * int(rank) if distributed else 0)


def mean_sampler_seed(torch_seed):
    """MeanSampler.sample: fixed at the first device draw from the seed of the generator in use."""
    return (int(torch_seed) ^ MEAN_SAMPLER_SEED_TAG) & 0xFFFFFFFFFFFFFFFF


# ---- which Philox inputs a run touches --------------------------------------------------------------------------------------

def clip_keys(seed, calls, n_tensors=None, dtypes=None, offset=0, c1_max=0):
    """(seed, c1, c2, c3) of every gradient-noise stream of the given engine steps (`calls`: the call-counter values; the engines
    pass offset 0).  A stream is all c0 under one such prefix; c1 = q >> 32 is 0 below 2^34 columns (c1_max: larger tensors)."""
    dtypes = ["f32"] * n_tensors if dtypes is None else list(dtypes)
    if len(dtypes) > MAX_TENSORS:
        raise ValueError("more than %d tensors" % MAX_TENSORS)
    keys = []
    for call in calls:
        for first, idx in clip_launches(dtypes):
            off64 = clip_off64(offset, call, first)
            for s in range(len(idx)):
                c2, c3 = clip_counter_words(s, off64)
                keys += [(int(seed), c1, int(c2), int(c3)) for c1 in range(c1_max + 1)]
    return keys


def mean_sample_keys(seed, offsets, n, num_samples, n_classes=1):
    """(seed, c1, c2, c3) of every stream the mean sampler touches in the given draws."""
    keys = []
    for off in offsets:
        off = int(off) & 0xFFFFFFFFFFFFFFFF
        lo, hi = off & 0xFFFFFFFF, off >> 32
        keys += [(int(seed), rep, lo, PERM_TAG ^ hi) for rep in range((n + num_samples - 1) // num_samples)]
        if n_classes > 1:
            keys.append((int(seed), LABEL_TAG, lo, hi))
        keys.append((int(seed), JITTER_TAG, lo, hi))
        keys += [(int(seed), i, lo, hi) for i in range(n)]
    return keys


def keys_of_run(manual_seed, rank, calls, n_tensors=9, dtypes=None, ms_batch=128, num_samples=32, n_classes=1, distributed=False,
                ms_offsets=None):
    """One rank's run: the gradient-noise streams of `calls` and the mean sampler's of draws 1..2*len(calls) (two per D-step)
    unless ms_offsets names them, each under the seed the trainer derives.  -> (clip keys, mean-sampler keys)."""
    calls = list(calls)
    if ms_offsets is None:
        ms_offsets = range(1, 2 * len(calls) + 1)
    ck = clip_keys(engine_seed(manual_seed, rank), calls, n_tensors, dtypes)
    mk = mean_sample_keys(mean_sampler_seed(process_seed(manual_seed, rank, distributed)), ms_offsets, ms_batch, num_samples, n_classes)
    return ck, mk
