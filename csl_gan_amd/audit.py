"""Membership-inference audit of a saved critic (reference mem_inf_attack.py:29-101; Hayes et al., "LOGAN", PoPETs 2019).

Three pieces, each with a device path on the kernels of csrc/attack_kernels.hip and a host path in numpy / torch:

  * the sampler and the trial.  `subset_indices` and `trial_hits` are THE definition of the estimate (include/cslgan.h "Audit
    sampler"): trial T draws n of the N train scores and m of the M non-train scores without replacement through a keyed
    permutation (swap-or-not shuffle on Philox4x32-10), ranks the pool with ties going to the train sample, and counts the train
    samples among the n best.  A trial is a function of (score arrays, seed, T) alone, so an estimate does not depend on how its
    trials are cut into launches, and cslgan_attack_trials is held to this model by integer equality;
  * `CriticScorer`: the attack value of every image of a uint8 cache, in index order, ragged tail included — pinned uint8 gather,
    H2D, cslgan_u8_to_f32_nhwc, the frozen critic, the value; full batches are one recorded HIP graph (generate.SampleGenerator's
    mould);
  * `attack_metrics`: ASR with its standard error, and from exact rank counts the AUC and the TPR at 1 % and 0.1 % FPR.
"""
from __future__ import annotations

import numpy as np
import torch

from .generate import _philox4x32_10 as philox4x32_10

AUDIT_SEED_TAG = 0x6D656D696E666174            # include/cslgan.h: xor-ed into the seed (apart from the noise, sampler and latent streams)
SIDE_TAG = (0x7472616E, 0x6E6F6E74)            # train, non-train: xor-ed into the high trial word of every counter
ROUND_KEY_TAG = 0xFFFFFFFF                     # counter word 0 of K_r
MAX_POOL = 4096                                # n + m of the device kernel (the pool lives in LDS)
FPR_BUDGETS = (("tpr_at_fpr_0.01", 1, 100), ("tpr_at_fpr_0.001", 1, 1000))
_M64 = 0xFFFFFFFFFFFFFFFF


def audit_key(seed):
    """The 64-bit Philox key of the audit sampler of `seed`."""
    return (int(seed) ^ AUDIT_SEED_TAG) & _M64


def shuffle_rounds(N):
    """R = 8 max(1, ceil(log2 N))."""
    return 8 * max(1, (int(N) - 1).bit_length())


def subset_indices(seed, trial, side, N, k):
    """pi(0) .. pi(k-1) of the side's permutation of [0, N) in trial `trial`: k distinct indices, int64.  `trial` may be an array
    of trial numbers (any Python ints / uint64): the result is then [len(trial), k]."""
    N, k = int(N), int(k)
    if not 0 <= k <= N or N >= 2 ** 31:
        raise ValueError("need 0 <= k <= N < 2^31, got k=%d N=%d" % (k, N))
    scalar = np.ndim(trial) == 0
    t = np.array([int(v) & _M64 for v in np.atleast_1d(np.asarray(trial, dtype=object))], dtype=np.uint64)[:, None]
    key = audit_key(seed)
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    t_lo, t_hi = t & np.uint64(0xFFFFFFFF), (t >> np.uint64(32)) ^ np.uint64(SIDE_TAG[int(side)])
    x = np.broadcast_to(np.arange(k, dtype=np.uint64)[None, :], (t.shape[0], k)).copy()
    if N == 0 or k == 0:
        return x.astype(np.int64)[0] if scalar else x.astype(np.int64)
    n64 = np.uint64(N)
    for r in range(shuffle_rounds(N)):
        kr = (philox4x32_10(ROUND_KEY_TAG, r, t_lo, t_hi, k0, k1)[0] * n64) >> np.uint64(32)          # mulhi32(word, N), [T, 1]
        xp = (kr + n64 - x) % n64
        bit = philox4x32_10(np.maximum(x, xp), r, t_lo, t_hi, k0, k1)[0] & np.uint64(1)
        x = np.where(bit == 1, xp, x)
    x = x.astype(np.int64)
    return x[0] if scalar else x


def _as_scores(v, name):
    a = np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32).reshape(-1)
    if not np.isfinite(a).all():
        raise ValueError("%s holds non-finite scores" % name)
    return a


def check_sizes(N, M, n, m):
    if not (1 <= n <= N and 0 <= m <= M and n + m <= MAX_POOL):
        raise ValueError("need 1 <= n <= N, 0 <= m <= M and n + m <= %d, got n=%d N=%d m=%d M=%d" % (MAX_POOL, n, N, m, M))


def trial_subsets(seed, first_trial, trials, N, M, n, m, chunk=None):
    """(train indices [trials, n], non-train indices [trials, m]) of trials first_trial .. first_trial + trials - 1 (mod 2^64): what
    the trials read, whatever the scores are."""
    chunk = int(chunk) if chunk else max(1, (1 << 15) // max(n + m, 1))      # numpy temporaries that stay in the cache
    it, im = np.zeros((trials, n), dtype=np.int64), np.zeros((trials, m), dtype=np.int64)
    for s in range(0, trials, chunk):
        T = [(int(first_trial) + s + i) & _M64 for i in range(min(chunk, trials - s))]
        it[s:s + len(T)] = subset_indices(seed, T, 0, N, n)
        if m:
            im[s:s + len(T)] = subset_indices(seed, T, 1, M, m)
    return it, im


def hits_of_subsets(vt, vn, it, im, _ties_to_train=True):
    """hits per trial (int64) for the subsets (it, im) of trial_subsets.  The pool is the n train values followed by the m
    non-train values, rank(i) = #{j : v[j] > v[i]} + #{j < i : v[j] == v[i]} — a stable descending sort, so ties go to the train
    sample, as Python's sorted(pairs, reverse=True) leaves them (mem_inf_attack.py:52-56) — and hits = #{i < n : rank(i) < n}.
    _ties_to_train=False is the other tie rule (tests show that the fixtures tell the two apart)."""
    vt, vn = np.asarray(vt, dtype=np.float32).reshape(-1), np.asarray(vn, dtype=np.float32).reshape(-1)
    n, m = it.shape[1], im.shape[1]
    a = vt[it]
    b = vn[im] if m else np.zeros((len(it), 0), dtype=np.float32)
    pool = np.concatenate([a, b] if _ties_to_train else [b, a], axis=1)
    order = np.argsort(-pool, axis=1, kind="stable")[:, :n]                      # -(+-0) compare equal; the callers refuse NaN
    return ((order < n) if _ties_to_train else (order >= m)).sum(axis=1).astype(np.int64)


def trial_hits(vt, vn, n, m, seed, first_trial, trials, _ties_to_train=True):
    """hits[t], t < trials (int64): the train samples among the n best of trial first_trial + t — the host model that
    cslgan_attack_trials is held to."""
    vt, vn = np.asarray(vt, dtype=np.float32).reshape(-1), np.asarray(vn, dtype=np.float32).reshape(-1)
    n, m, trials = int(n), int(m), int(trials)
    check_sizes(len(vt), len(vn), n, m)
    step = max(1, (1 << 22) // (n + m))                                          # bounds the index arrays of a long estimate
    parts = [hits_of_subsets(vt, vn, *trial_subsets(seed, int(first_trial) + s, min(step, trials - s), len(vt), len(vn), n, m), _ties_to_train)
             for s in range(0, trials, step)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


# ---- rank counts, AUC, TPR at an FPR budget ------------------------------------------------------------------------------------------

def rank_counts_host(a, b):
    """(gt, eq) int64: gt[i] = #{j : a[i] > b[j]}, eq[i] = #{j : a[i] == b[j]} (what cslgan_rank_counts computes)."""
    a, sb = np.asarray(a, dtype=np.float32).reshape(-1), np.sort(np.asarray(b, dtype=np.float32).reshape(-1))
    lo, hi = np.searchsorted(sb, a, side="left"), np.searchsorted(sb, a, side="right")
    return lo.astype(np.int64), (hi - lo).astype(np.int64)


def rank_metrics(gt, eq, nb):
    """AUC = sum(gt + eq / 2) / (na nb) — P(train > non-train) + P(tie) / 2 — and, per FPR budget num / den, the share of train
    samples flagged when train sample i is flagged iff at most floor(nb num / den) non-train scores are >= its own:
    nb - gt[i] <= (nb * num) // den.  Exact integer arithmetic up to the final divisions."""
    gt, eq = np.asarray(gt, dtype=np.int64), np.asarray(eq, dtype=np.int64)
    na, nb = len(gt), int(nb)
    out = {"auc": float((2 * int(gt.sum()) + int(eq.sum())) / (2.0 * na * nb)) if na and nb else float("nan")}
    for name, num, den in FPR_BUDGETS:
        out[name] = float(int((nb - gt <= (nb * num) // den).sum()) / na) if na else float("nan")
    return out


def attack_metrics(vt, vn, data_prop=0.1, pool=1000, asr_iters=10000, seed=0, device="cpu", first_trial=0):
    """The audit's figures as exact functions of (score arrays, seed, pool, data_prop, asr_iters):
        asr          mean(hits) / n over trials first_trial .. first_trial + asr_iters - 1, n = int(pool * data_prop),
                     m = int(pool * (1 - data_prop)) as mem_inf_attack.py:48-49 writes them (pool = its literal 1000)
        asr_stderr   the standard error of that mean, std(hits, ddof=1) / (n sqrt(asr_iters))
        auc, tpr_at_fpr_0.01, tpr_at_fpr_0.001   rank_metrics of the train scores against the non-train scores
    vt / vn: numpy arrays or tensors on any device.  On a HIP device the trials and the rank counts run in cslgan_attack_trials /
    cslgan_rank_counts; on the CPU in the host model: the integers, hence the figures, are the same."""
    a, b = _as_scores(vt, "vt"), _as_scores(vn, "vn")
    n, m = int(pool * data_prop), int(pool * (1 - data_prop))
    check_sizes(len(a), len(b), n, m)
    asr_iters = int(asr_iters)
    if asr_iters < 1:
        raise ValueError("asr_iters must be positive")
    dev = torch.device(device)
    if dev.type == "cuda":
        from . import ops
        with torch.cuda.device(dev):
            da = vt.to(dev, torch.float32).reshape(-1).contiguous() if torch.is_tensor(vt) else torch.from_numpy(a).to(dev)
            db = vn.to(dev, torch.float32).reshape(-1).contiguous() if torch.is_tensor(vn) else torch.from_numpy(b).to(dev)
            hits = ops.attack_trials(da, db, n, m, seed, first_trial, asr_iters).cpu().numpy().astype(np.int64)
            if len(b):
                gt, eq = (t.cpu().numpy().astype(np.int64) for t in ops.rank_counts(da, db))
            else:
                gt = eq = np.zeros(len(a), dtype=np.int64)
    else:
        hits = trial_hits(a, b, n, m, seed, first_trial, asr_iters)
        gt, eq = rank_counts_host(a, b)
    out = {"asr": float(hits.mean() / n),
           "asr_stderr": float(hits.std(ddof=1) / (n * np.sqrt(asr_iters))) if asr_iters > 1 else float("nan"),
           "n": n, "m": m, "asr_iters": asr_iters}
    out.update(rank_metrics(gt, eq, len(b)))
    return out


# ---- scoring a cache with the critic ---------------------------------------------------------------------------------------------------

def softmax_max_rows_host(logits):
    """softmax(logits, 1).max(1)[0] (mem_inf_attack.py:80)."""
    return torch.nn.functional.softmax(logits.float(), 1).max(1)[0]


class CriticScorer:
    """Attack values of the images of a pipeline.CachedImages: `score(cache) -> float32[len(cache)]`, index order, no flip, no
    shuffle, the ragged tail included.  The value is the critic's first output, flattened (mem_inf_attack.py:97) — for an MNIST
    critic with an auxiliary class head the largest softmax probability of the head's logits (:79-80).  D is frozen (eval, no
    grad).  On a HIP device full batches replay one recorded graph over static buffers; the ragged batch runs eagerly."""

    def __init__(self, D, train_opt, device, batch_size, hip_graph=True, compute_dtype=None):
        self.D, self.opt, self.device, self.B = D, train_opt, torch.device(device), int(batch_size)
        if self.B < 1:
            raise ValueError("batch_size must be positive")
        self.conditional = bool(train_opt.conditional)
        self.aux_value = train_opt.dataset == "MNIST"
        self.on_gpu = self.device.type == "cuda"
        self.compute_dtype = compute_dtype or getattr(train_opt, "compute_dtype", None) or "fp32"
        D.eval()
        for p in D.parameters():
            p.requires_grad_(False)
        self.use_graph = bool(hip_graph) and self.on_gpu
        self.graph, self._pinned_ws, self._static, self._shape = None, [], None, None
        self._prev_compute = None
        if self.on_gpu:
            from . import ops
            self._prev_compute = ops.get_compute_dtype()      # process-wide switch: release() puts it back
            ops.set_compute_dtype(self.compute_dtype)

    # ---- one batch ---------------------------------------------------------------------------------------------------------------
    def _value(self, out, aux):
        if self.aux_value and aux is not None:
            if self.on_gpu:
                from . import ops
                return ops.softmax_max_rows(aux.float().contiguous())
            return softmax_max_rows_host(aux)
        return out.reshape(-1).float()

    def _buffers(self, n, cache):
        dev, shape = self.device, (n, cache.H, cache.W, cache.C)
        return dict(u8=torch.empty(shape, device=dev, dtype=torch.uint8), x=torch.empty(shape, device=dev, dtype=torch.float32),
                    y=torch.zeros(n, device=dev, dtype=torch.int64), v=torch.empty(n, device=dev, dtype=torch.float32))

    def _steps(self, b, scale, bias):
        """bytes -> normalised fp32 NHWC batch -> D(x, y) -> attack value, on the current stream."""
        from . import _lib, ops
        n, H, W, C = b["u8"].shape
        ops.check(_lib.lib().cslgan_u8_to_f32_nhwc(ops._p(b["u8"]), None, n, H, W, C, float(scale), float(bias), ops._p(b["x"]),
                                                   torch.cuda.current_stream().cuda_stream), "u8_to_f32_nhwc")
        with torch.no_grad():
            out, aux = self.D(b["x"].permute(0, 3, 1, 2), b["y"] if self.conditional else None)
            v = self._value(out, aux)
        if v.numel() != n:
            raise RuntimeError("critic returned %d values for %d images" % (v.numel(), n))
        b["v"].copy_(v)

    def _record(self, cache):
        """Full batches as ONE recorded graph (generate.SampleGenerator._record's steps: two eager batches, the critic's filter
        workspaces pinned, no cyclic collection under capture, the repack cache cleared of what the capture created)."""
        from . import ops
        import gc
        b = self._static
        for _ in range(2):
            self._steps(b, cache.scale, cache.bias)
        torch.cuda.synchronize(self.device)
        self._pinned_ws = ops.repack_cache.pin({m._wtoken for m in self.D.modules() if hasattr(m, "_wtoken")})
        ops.repack_cache.clear()
        graph = torch.cuda.CUDAGraph()
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                self._steps(b, cache.scale, cache.bias)
        finally:
            if gc_was_on:
                gc.enable()
        ops.repack_cache.clear()
        self.graph = graph

    def release(self):
        """Drop the recorded graph, its pool and the pins it held; the compute-dtype switch goes back to what it was."""
        self._drop_graph()
        self._shape = None
        if self._prev_compute is not None:
            from . import ops
            ops.set_compute_dtype(self._prev_compute)
            self._prev_compute = None

    # ---- the loop ----------------------------------------------------------------------------------------------------------------
    def score(self, cache):
        n = len(cache)
        blocks = [(s, min(self.B, n - s)) for s in range(0, n, self.B)]
        if not self.on_gpu:
            out = np.zeros(n, dtype=np.float32)
            for s, k in blocks:
                x = cache.to_float(cache.x[s:s + k]).to(self.device)
                y = torch.from_numpy(np.asarray(cache.labels[s:s + k], dtype=np.int64)).to(self.device) if self.conditional else None
                with torch.no_grad():
                    o, aux = self.D(x, y)
                    out[s:s + k] = self._value(o, aux).cpu().numpy()
            return out
        with torch.cuda.device(self.device):
            return self._score_gpu(cache, n, blocks)

    def _score_gpu(self, cache, n, blocks):
        shape = (self.B, cache.H, cache.W, cache.C)
        if self._shape not in (None, shape + (cache.scale, cache.bias)):
            self._drop_graph()
        self._shape = shape + (cache.scale, cache.bias)
        stream = torch.cuda.current_stream(self.device)
        host = [dict(u8=torch.empty(shape, dtype=torch.uint8, pin_memory=True), y=torch.zeros(self.B, dtype=torch.int64, pin_memory=True),
                     sent=None) for _ in range(2)]
        scores = torch.empty(n, device=self.device, dtype=torch.float32)
        for k, (s, cnt) in enumerate(blocks):
            h = host[k % 2]
            if h["sent"] is not None:
                h["sent"].synchronize()                     # the upload of batch k - 2 has left this pinned buffer
            cache.gather(np.arange(s, s + cnt), h["u8"][:cnt])
            h["y"][:cnt].copy_(torch.from_numpy(np.asarray(cache.labels[s:s + cnt], dtype=np.int64)))
            full = cnt == self.B
            if full and self._static is None:
                self._static = self._buffers(self.B, cache)
            b = self._static if full else self._buffers(cnt, cache)
            b["u8"].copy_(h["u8"][:cnt], non_blocking=True)
            b["y"].copy_(h["y"][:cnt], non_blocking=True)
            h["sent"] = torch.cuda.Event()
            h["sent"].record(stream)
            if full and self.use_graph and self.graph is None:
                self._record(cache)                         # leaves the static buffers holding this batch's bytes
            if full and self.graph is not None:
                self.graph.replay()
            else:
                self._steps(b, cache.scale, cache.bias)
            scores[s:s + cnt].copy_(b["v"])
        out = scores.cpu().numpy()
        torch.cuda.synchronize(self.device)
        return out

    def weights_changed(self):
        """Call after loading another checkpoint into D: the recorded graph reads the repacked filters of the weights it was
        recorded with, so it is dropped and the next full batch records a new one."""
        self._drop_graph()

    def _drop_graph(self):
        """The recorded graph, its static buffers and its pins go; the compute dtype stays (also: a cache of another geometry)."""
        self.graph, self._static = None, None
        if self._pinned_ws:
            from . import ops
            ops.repack_cache.unpin(self._pinned_ws)
            self._pinned_ws = []
