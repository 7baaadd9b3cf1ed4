"""Tensor-level wrappers over the C-ABI (include/cslgan.h).  torch is plumbing here: it owns the
device memory and the stream; every kernel launched is hand-written HIP from csl_gan_amd/csrc.

Layout convention: activations are NHWC-contiguous fp32 tensors of shape [N,H,W,C]; conv filters
are [K,R,S,C].  Device tensors only — there is no CPU path in this module.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import ConvT, SegsT, check

# the header's constants, as _lib read them
ACT_NONE, ACT_LRELU02, ACT_RELU, ACT_TANH = _lib.ACT_NONE, _lib.ACT_LRELU02, _lib.ACT_RELU, _lib.ACT_TANH
COMPUTE_F32, COMPUTE_BF16, COMPUTE_BF16X3 = _lib.COMPUTE_F32, _lib.COMPUTE_BF16, _lib.COMPUTE_BF16X3          # cslgan_conv_t.compute

_compute = COMPUTE_F32
_auto = False


def set_compute_dtype(name):
    """Arithmetic of every MFMA conv / linear / weight-gradient launch of this process (tensors are fp32 in HBM either way):
      "fp32"    exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the default;
      "bf16"    operands rounded to bfloat16 in the kernels, fp32 accumulate (BASELINE configs[4]);
      "bf16x3"  fp32 emulated from three bfloat16 pieces per operand on the bf16 matrix cores (fp32-accurate, see
                csrc/igemm_bf16.hip) for every launch;
      "fp32_auto"  fp32 accuracy on whichever of the two fp32-accurate paths is faster for the launch: bf16x3 for forward /
                data-gradient launches that fill the chip (the generator's 5x5 convs, the critic's fused 384-row passes),
                exact fp32 MFMA for weight gradients and small launches.
    One process drives one GPU and one training run, so this is process-wide state set once from --compute_dtype."""
    global _compute, _auto
    if name not in ("fp32", "bf16", "bf16x3", "fp32_auto"):
        raise ValueError("compute dtype must be 'fp32', 'bf16', 'bf16x3' or 'fp32_auto', got %r" % (name,))
    _auto = name == "fp32_auto"
    _compute = {"fp32": COMPUTE_F32, "bf16": COMPUTE_BF16, "bf16x3": COMPUTE_BF16X3, "fp32_auto": COMPUTE_F32}[name]


def get_compute_dtype():
    return "fp32_auto" if _auto else {COMPUTE_F32: "fp32", COMPUTE_BF16: "bf16", COMPUTE_BF16X3: "bf16x3"}[_compute]


def _kc_compute(rows, n_out, kdim):
    """compute field for a forward / data-gradient launch of `rows` output rows x n_out output channels with reduction
    length kdim.  fp32_auto: measured same-box (scripts/compute_modes.py) the three-piece path wins once the launch has
    >= 128 tiles of 128x128 and a long reduction (150-185 vs 110-135 TF on the generator's convs, 100-155 vs 81-112 TF on
    the critic's 384-row passes) and loses on the 128-row launches of the small layers."""
    if _auto and n_out >= 64 and kdim >= _AUTO_MIN_K and ((rows + 127) // 128) * ((n_out + 127) // 128) >= _AUTO_MIN_TILES:
        return COMPUTE_BF16X3
    return _compute


_F32_HALO = True        # exact-fp32 launches the round-4 LDS-halo kernel takes run on it (igemm_x3h<., 0, .>); set_f32_halo switches it


# Largest channel split of a low-fill halo launch (<= 1: never split).  OFF by default: measured alone the critic's last convs gain
# (conv4 forward, 384 rows: 167 -> 200 TF; 128 rows: 86 -> 140 TF), but inside the two-stream recorded step the other branch
# already fills the idle CUs and the step does not move (6.797 ms split, 6.731 ms unsplit, 6.723 ms split + 128-wide tiles: noise)
# while every split launch adds a reduce launch.  8 switches it on (single-stream / eager runs; the kernel side caps the split at 8).
_X3_SPLIT = 0


def _split_scratch(d, rows, cols, red_channels, out):
    """Scratch for the channel split of the LDS-halo kernel (cslgan_conv_t.split_ws): a launch of fewer than 512 128x128 tiles may
    divide its reduction channels over up to _X3_SPLIT workgroups per tile, at least two 16-channel chunks each.  The tensor comes
    from the caching allocator like the output (stream-ordered, graph-pool safe); the C side decides the actual split."""
    s = min(_X3_SPLIT, (red_channels // 16) // 2)
    if s < 2 or -(-rows // 128) * -(-cols // 128) >= 512:
        return None
    ws = torch.empty(s * out.numel(), device=out.device, dtype=torch.float32)
    d.split_ws, d.split_ws_floats = ws.data_ptr(), ws.numel()
    return ws


_GN_FUSE = True            # GroupNorm statistics from the producing conv's epilogue (tests switch it off to compare)


class gn_partials:
    """Ask the NEXT conv2d_fwd on this thread to leave GroupNorm(groups) partial statistics of its output behind
    (cslgan_conv_t.gn_part): `with ops.gn_partials(32) as cell: y = conv(...)`, then `groupnorm_act(y, ..., part=cell.part)`.
    cell.part stays None when the conv's shape or route cannot produce them — the normalisation then runs its own statistics pass."""
    _req = None

    def __init__(self, groups):
        self.groups, self.part = int(groups), None

    def __enter__(self):
        self._prev, gn_partials._req = gn_partials._req, (self if _GN_FUSE else None)
        return self

    def __exit__(self, *a):
        gn_partials._req = self._prev


_ones_cache = {}


def ones_like_const(t):
    """A persistent tensor of ones with t's shape / dtype / device: the constant cotangent of a backward() or autograd.grad call
    (torch.ones_like there is one fill launch per call, re-run by every replay of a recorded step).  Never written to."""
    key = (tuple(t.shape), t.dtype, str(t.device))
    c = _ones_cache.get(key)
    if c is None:
        c = _ones_cache[key] = torch.ones(t.shape, dtype=t.dtype, device=t.device)
    return c


def set_f32_halo(on):
    """Switch the exact-fp32 form of the round-4 halo kernel on or off at run time (returns the previous setting): the same products
    summed in a different order, so the golden tests use it to prove which activation units sit within rounding of zero."""
    global _F32_HALO
    prev, _F32_HALO = _F32_HALO, bool(on)
    return prev


# fp32_auto thresholds (scripts/compute_modes.py): 128x128 tiles of a forward / data-gradient launch, its reduction length, and the
# FLOP from which an eligible weight gradient goes to the three-piece kernel
_AUTO_MIN_TILES = 32
_AUTO_MIN_K = 512
_AUTO_WG_MIN_FLOP = 0.5e9


class compute_dtype:
    """Context manager form of set_compute_dtype (tests)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = get_compute_dtype()
        set_compute_dtype(self.name)

    def __exit__(self, *a):
        set_compute_dtype(self.prev)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_storage_bf16 = False


def set_storage_dtype(name):
    """Element type of the ACTIVATIONS and ACTIVATION GRADIENTS between the critic's conv layers in HBM (BASELINE configs[4],
    csrc/igemm_bf16s.hip, csrc/igemm_mcs.hip):
      "fp32"  the default: every tensor is fp32;
      "bf16"  the critic's conv layers write bfloat16 outputs; every conv / data-gradient / weight-gradient call whose activation
              operands are bfloat16 runs on the bf16-stored kernels (bf16 filter copies cached per parameter version, fp32
              accumulation, fp32 weight gradients).  Parameters, weight gradients, per-sample gradients, norms, clip, noise and
              Adam stay fp32.  The dtype then FOLLOWS the tensors: an op handed bf16 activations answers in kind.
    Process-wide like set_compute_dtype, set once from --storage_dtype."""
    global _storage_bf16
    if name not in ("fp32", "bf16"):
        raise ValueError("storage dtype must be 'fp32' or 'bf16', got %r" % (name,))
    _storage_bf16 = name == "bf16"


def get_storage_dtype():
    return "bf16" if _storage_bf16 else "fp32"


def storage_bf16():
    return _storage_bf16


class storage_dtype:
    """Context manager form of set_storage_dtype (tests)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = get_storage_dtype()
        set_storage_dtype(self.name)

    def __exit__(self, *a):
        set_storage_dtype(self.prev)


def cast_bf16(t):
    """fp32 -> bfloat16 (round to nearest even), same shape and strides; one pass of cslgan_cast_f32_bf16."""
    if t.dtype == torch.bfloat16:
        return t
    _chk(t, "t", any_order=True)
    out = torch.empty_like(t, dtype=torch.bfloat16)
    check(_lib.lib().cslgan_cast_f32_bf16(_p(t), _p(out), t.numel(), _stream()), "cast_f32_bf16")
    return out


def cast_f32(t):
    """bfloat16 -> fp32 (exact), same shape and strides."""
    if t is None or t.dtype == torch.float32:
        return t
    _chk(t, "t", allow_bf16=True, any_order=True)
    out = torch.empty_like(t, dtype=torch.float32)
    check(_lib.lib().cslgan_cast_bf16_f32(_p(t), _p(out), t.numel(), _stream()), "cast_bf16_f32")
    return out


def _dense_block(t):
    """True when t's elements fill one block of memory exactly once (any dimension order: e.g. channels-last views)."""
    dims = sorted(((st, sz) for sz, st in zip(t.shape, t.stride()) if sz > 1))
    run = 1
    for st, sz in dims:
        if st != run:
            return False
        run *= sz
    return True


def _is_bf16(t):
    return t is not None and t.dtype == torch.bfloat16


class _RepackCache:
    """Repacked filter matrices (data-gradient classes, stride-2 parity classes, the channel-folded filters of the
    generator's UpsampleConv layers) keyed by the filter tensor's storage and autograd version counter: any in-place
    torch op bumps the counter, and HipAdam — which writes the weights through raw pointers — bumps it explicitly
    (torch.autograd.graph.increment_version).  A D-step reuses each critic layer's repack four times and the
    generator's folded filters until the next generator step.

    Pinned entries (round 4): a recorded HIP graph bakes the ADDRESS of every workspace it reads.  The generator is frozen during
    D-steps, so its folded / pre-split filters need not be re-made by every replay: GraphedDStep pins the generator's entries (made
    by the eager warm-up steps), records the step with cache hits on them, and calls refresh_pinned() before each replay — an entry
    whose source parameter has a new version (a train_G step ran) is rebuilt IN PLACE by the closure it was made with.  A pinned
    entry is never evicted or replaced; a version mismatch seen by get() reuses its buffer (repack = 1)."""

    def __init__(self, max_entries=256):
        self.d, self.max = {}, max_entries      # callers pass wkey (a never-reused per-module token, csl_gan_amd.nn) only for module-owned filters
        self.pinned = {}                         # key -> number of recorded graphs that read the entry's buffer

    def get(self, kind, w, numel, wkey=None, version=None):
        """version: the autograd version to key on when `w` is itself derived from a parameter (its own counter is always 0): an int,
        or an object with a `.version` property (csl_gan_amd.nn.VersionRef) that refresh_pinned() can read again later.
        A hit from another stream than the one that packed the buffer waits for that pack (the D-step runs its gradient-penalty
        branch on a second stream, and both branches read the critic's re-packed filters)."""
        if wkey is None:          # not known to be a live parameter (a temporary may reuse an address): never cache
            return torch.empty(numel, device=w.device, dtype=torch.float32), 1
        key = (kind, wkey, w.data_ptr(), tuple(w.shape))
        src = version if hasattr(version, "version") else (w if version is None else None)
        ver = w._version if version is None else (version.version if hasattr(version, "version") else version)
        hit = self.d.get(key)
        cur = torch.cuda.current_stream()
        if hit is not None and hit[1].numel() == numel and hit[1].device == w.device:
            if hit[0] == ver:
                if hit[2] != cur.cuda_stream and hit[3] is not None:
                    cur.wait_event(hit[3])
                self._fresh = None
                return hit[1], 0
            if key in self.pinned:        # a recorded graph reads this buffer: rebuild it where it is
                hit[0], hit[2], hit[3] = ver, cur.cuda_stream, None
                self._fresh = key
                return hit[1], 1
        if len(self.d) >= self.max:
            self.clear()
        ws = torch.empty(numel, device=w.device, dtype=torch.float32)
        self.d[key] = [ver, ws, cur.cuda_stream, None, None, src]
        self._fresh = key
        return ws, 1

    def set_rebuild(self, fn):
        """Attach to the entry get() has just made (a miss) the closure that re-makes its contents in place: fn() launches the
        packing kernels on the current stream.  Only entries with a rebuild closure and a version source can be pinned."""
        key = getattr(self, "_fresh", None)
        if key is not None and key in self.d:
            self.d[key][4] = fn

    def packed(self):
        """Called right after the launch that filled the most recent fresh buffer: marks the point other streams must wait for."""
        key = getattr(self, "_fresh", None)
        if key is not None and key in self.d and self.multi_stream:
            ev = torch.cuda.Event()
            ev.record()
            self.d[key][3] = ev
        self._fresh = None

    multi_stream = False        # set while a second stream is in use (Trainer): events are only recorded then

    def pin(self, tokens):
        """Pin every entry that belongs to a module token in `tokens` (key[1] is the token or a tuple starting with it) and can be
        rebuilt in place.  Returns the pinned keys (hand them back to unpin())."""
        keys = []
        for key, e in self.d.items():
            tok = key[1][0] if isinstance(key[1], tuple) else key[1]
            if tok in tokens and e[4] is not None and e[5] is not None:
                self.pinned[key] = self.pinned.get(key, 0) + 1
                e[3] = None           # (the caller has synchronised the device: no cross-stream wait is owed any more)
                keys.append(key)
        return keys

    def unpin(self, keys):
        for key in keys:
            n = self.pinned.get(key, 0) - 1
            if n > 0:
                self.pinned[key] = n
            else:
                self.pinned.pop(key, None)

    def refresh_pinned(self):
        """Rebuild (in place, in insertion order: a folded filter before its pieces) every pinned entry whose source has a new
        version.  Returns how many were rebuilt."""
        n = 0
        for key in self.d:
            if key not in self.pinned:
                continue
            e = self.d[key]
            ver = e[5].version if hasattr(e[5], "version") else e[5]._version
            if ver != e[0]:
                e[4]()
                e[0], e[2], e[3] = ver, torch.cuda.current_stream().cuda_stream, None
                n += 1
        return n

    def clear(self):
        """Drop every entry that is not pinned."""
        self.d = {k: v for k, v in self.d.items() if k in self.pinned}


repack_cache = _RepackCache()


class LaunchTimer:
    """HIP-event timing of individual C-ABI launches on the stream they are enqueued on (torch's
    current stream), for bench.py's live roofline figures.  Events are resolved once, after the
    caller has synchronised.  Each record carries the name of the device kernel the entry dispatched to
    (cslgan_last_kernel), so figures can be grouped per KERNEL as rocprofv3 lists them."""

    def __init__(self, only=None):
        """only: optional set of (entry name, shape tag) pairs — launches outside it are not instrumented (two event records
        per launch cost the host ~5 us; bench.py watches just the dominant kernel's launches inside its timed region)."""
        self.records = []
        self.only = only

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name, flop, nbytes, start, exec_flop=None, tag=None, kernel=None):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.records.append((name, flop, nbytes, start, e, flop if exec_flop is None else exec_flop, tag, kernel or name))

    def keys_of_kernel(self, kernel_name):
        """(entry name, shape tag) pairs whose launches dispatched to `kernel_name`."""
        return {(name, tag) for name, _, _, _, _, _, tag, kernel in self.records if kernel == kernel_name}

    def summary(self, by_shape=False, by_kernel=False):
        out = {}
        for name, flop, nbytes, s, e, xf, tag, kernel in self.records:
            if by_kernel:
                name = kernel
            if by_shape and tag:
                name = "%s %s" % (name, tag)
            d = out.setdefault(name, {"name": name, "ms": 0.0, "flop": 0.0, "exec_flop": 0.0, "bytes": 0.0, "n": 0})
            d["ms"] += s.elapsed_time(e)
            d["flop"] += flop
            d["exec_flop"] += xf
            d["bytes"] += nbytes
            d["n"] += 1
        return out


_timer = None


def set_launch_timer(t):
    global _timer
    _timer = t


def _timed(name, flop, nbytes, fn, exec_flop=None, tag=None):
    """flop = algorithmic FLOP of the op as the reference executes it; exec_flop = FLOP the kernel really issues
    (differs for the UpsampleConv layers, which run on C/4 folded channels, and for the zero-padded RGB input)."""
    if _timer is None:
        return fn()
    tg = tag() if callable(tag) else tag
    if _timer.only is not None and (name, tg) not in _timer.only:
        return fn()
    s = _timer.begin()
    r = fn()
    _timer.end(name, flop, nbytes, s, exec_flop, tg, _lib.lib().cslgan_last_kernel().decode(errors="replace"))
    return r


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t: torch.Tensor, name: str, allow_bf16=False, any_order=False):
    """A device tensor of fp32 (or bf16) elements, contiguous — any_order (the casts are layout-agnostic): one dense block of memory
    in some dimension order."""
    if not t.is_cuda:
        raise RuntimeError("%s must be a device tensor (csl_gan_amd.ops has no CPU path)" % name)
    if t.dtype != torch.float32 and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise RuntimeError("%s must be float32%s, got %s" % (name, " or bfloat16" if allow_bf16 else "", t.dtype))
    if not t.is_contiguous() and not (any_order and _dense_block(t)):
        raise RuntimeError("%s must be %s" % (name, "dense" if any_order else "contiguous"))
    return t


def conv_out_size(H, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1


# ---- conv dispatch: one geometry per call, each shape rule once, one launch helper ----------------------------------------------------

class _Geom(NamedTuple("_Geom", [(f, int) for f in "N H W C K R S stride pad P Q".split()])):
    """The shape of one conv call, built and checked once per public op: x[N,H,W,C], w[K,R,S,C], y / gy[N,P,Q,K]."""
    __slots__ = ()

    def __new__(cls, N, H, W, Cc, K, R, S, stride, pad):
        return tuple.__new__(cls, (N, H, W, Cc, K, R, S, stride, pad, conv_out_size(H, R, stride, pad), conv_out_size(W, S, stride, pad)))

    flop = property(lambda g: 2.0 * g.N * g.P * g.Q * g.K * g.R * g.S * g.C)
    wsize = property(lambda g: g.K * g.R * g.S * g.C)         # elements of the filter / of one weight gradient

    def desc(self, comp):
        return ConvT(*self[:9], comp, self.P, self.Q)

    def tag(self, sfx="", vals=(), stride=True):
        """Shape tag of a launch-timer record, the one place its format is written: the shape, then the route's words (sfx % vals)."""
        return ("N%d %dx%d C%d K%d R%d" % (self.N, self.H, self.W, self.C, self.K, self.R) + (" s%d" % self.stride if stride else "")
                + (" " + sfx % vals if sfx else ""))


def _fwd_geom(x, w, stride, pad):
    _chk(x, "x", allow_bf16=True); _chk(w, "w")
    N, H, W, Cc = x.shape
    K, R, S, C2 = w.shape
    if C2 != Cc:
        raise RuntimeError("conv2d_fwd: channel mismatch x C=%d, w C=%d" % (Cc, C2))
    return _Geom(N, H, W, Cc, K, R, S, stride, pad)


def _dgrad_geom(gy, w, in_hw, stride, pad):
    _chk(gy, "gy", allow_bf16=True); _chk(w, "w")
    N, P, Q, K = gy.shape
    K2, R, S, Cc = w.shape
    H, W = in_hw
    g = _Geom(N, H, W, Cc, K, R, S, stride, pad)
    if K2 != K or (g.P, g.Q) != (P, Q):
        raise RuntimeError("conv2d_dgrad: gy shape %s inconsistent with input %dx%d" % (tuple(gy.shape), H, W))
    return g


def _wgrad_geom(op, gy, x, R, S, stride, pad):
    """Geometry of a weight gradient / Gram call from its operands' shapes (element types are the route's business)."""
    N, H, W, Cc = x.shape
    N2, P, Q, K = gy.shape
    g = _Geom(N, H, W, Cc, K, R, S, stride, pad)
    if N2 != N or (g.P, g.Q) != (P, Q):
        raise RuntimeError("%s: gy %s inconsistent with x %s" % (op, tuple(gy.shape), tuple(x.shape)))
    return g


def _auto_desc(g, kind, group=None):
    """Descriptor in the process's compute mode.  kind: "fwd" / "dgrad" may take the bf16x3 path under fp32_auto; weight gradients
    only on the LDS-resident three-piece kernel's shapes."""
    N, H, W, Cc, K, R, S, stride, pad, P, Q = g
    comp = _compute
    if kind == "fwd":
        comp = _kc_compute(N * P * Q, K, R * S * Cc)
    elif kind == "dgrad":
        comp = _kc_compute(N * H * W, Cc, (R * S * K) // (stride * stride))
    elif (kind == "wgrad" and _auto and S == 5 and stride in (1, 2) and K % 64 == 0 and Cc % 64 == 0 and g.flop >= _AUTO_WG_MIN_FLOP
          and ((P % 8 == 0 and Q % 8 == 0) or
               ((P, Q, H, W, stride, pad) == (4, 4, 8, 8, 2, 2) and group is not None and group % 2 == 0))):
        comp = COMPUTE_BF16X3          # weight gradient on the LDS-resident three-piece kernel (csrc/igemm_wgh.hip: igemm_x3w_kernel)
    if comp == COMPUTE_BF16 and H == 1 and W == 1 and R == 1 and S == 1 and 2.0 * N * K * Cc < 1e9:
        # small linear layers (the critic's head, the generator's first layer): a few hundred MFLOP on skinny GEMMs where the bf16
        # gather kernels ran at < 1 TF (0.35 ms for 268 MFLOP); the fp32 kernels take 15-30 us and are exact
        comp = COMPUTE_F32
    return ConvT(N, H, W, Cc, K, R, S, stride, pad, comp, P, Q)


def _conv_desc(N, H, W, Cc, K, R, S, stride, pad, kind="wgrad", group=None):
    """(descriptor, P, Q) from plain sizes: _auto_desc for callers that hold no geometry (the tests)."""
    g = _Geom(N, H, W, Cc, K, R, S, stride, pad)
    return _auto_desc(g, kind, group), g.P, g.Q


def _launch(name, entry, args, g, nbytes, sfx="", vals=(), exec_flop=None, flop=None, tag_stride=True):
    """One C-ABI launch, cslgan_<entry>(*args, stream), timed as `name`.  The timer's figures are callables (or plain numbers), so
    that like the tag they cost nothing when no timer is installed: nbytes; flop (default g.flop), the op as the reference executes
    it; exec_flop, what the kernel really issues; sfx % vals, the route's words in the shape tag."""
    fn = getattr(_lib.lib(), "cslgan_" + entry)
    if _timer is None:
        return check(fn(*args, _stream()), entry)
    flop, nbytes, exec_flop = (v() if callable(v) else v for v in (g.flop if flop is None else flop, nbytes, exec_flop))
    return _timed(name, flop, nbytes, lambda: check(fn(*args, _stream()), entry), exec_flop=exec_flop, tag=lambda: g.tag(sfx, vals, tag_stride))


# -- shape rules: each kernel's "takes this launch", written once (the C side re-checks what it needs)

# Per compute mode of an LDS-halo launch (csrc/igemm_x3.hip): suffix of the stride-2 / data-gradient repack-cache keys and timer tags,
# cache key of the stride-1 forward filter copy, bfloat16 pieces of that copy (0: a step-major fp32 copy).
_HALO_KIND = {COMPUTE_BF16X3: ("x3", "x3w", 3), COMPUTE_BF16: ("b16", "bf16w", 1), COMPUTE_F32: ("f32h", "f32w", 0)}


def _halo_arith(comp):
    """Arithmetic the LDS-halo kernel of csrc/igemm_x3.hip runs in: both bf16 forms, and exact fp32 unless set_f32_halo(False)."""
    return comp in (COMPUTE_BF16X3, COMPUTE_BF16) or (comp == COMPUTE_F32 and _F32_HALO)


def _fwd_halo_s1(comp, g):
    """This fp32-tensor forward call takes the stride-1 LDS-halo kernel (cslgan_conv2d_fwd_x3_f32): the one rule for conv2d_fwd's
    route and for in_affine_ok's promise about it."""
    return (_halo_arith(comp) and g.stride == 1 and g.R * g.S > 1 and g.C % 16 == 0 and g.K >= 64 and g.K % 4 == 0
            and g.P % 8 == 0 and g.Q % 8 == 0)


def _fwd_parity_s2(g, c_mult, residual):
    """A stride-2 forward conv as parity sub-images: odd square filter, channels a multiple of c_mult, no residual."""
    return g.stride == 2 and g.R == g.S and g.R % 2 == 1 and g.R > 1 and g.C % c_mult == 0 and g.K >= 64 and residual is None


def _skinny(g):
    """The 1..4-output-channel vector-ALU kernels (csrc/igemm_skinny.hip): 64 input channels, stride 1, up to 3x3, 8x8-patchable output."""
    return g.K <= 4 and g.C == 64 and g.stride == 1 and g.R * g.S <= 9 and g.P % 8 == 0 and g.Q % 8 == 0


def _c3_layer(g, grid_ok):
    """The critic's first conv as csrc/conv_c3.hip takes it (c3_shape there): 3 -> 64 channels, 5x5, stride 2, pad 2, even image."""
    return g.K == 64 and g.R == 5 and g.S == 5 and g.stride == 2 and g.pad == 2 and g.H % 2 == 0 and g.W % 2 == 0 and grid_ok


def _c3_fwd(g):
    return g.C == 3 and _c3_layer(g, g.H % 16 == 0 and g.W % 32 == 0)


def _c3_wgrad(g):
    """The first-layer kernel's weight gradient: RGB input, an output grid of 16 / 32 / 64 columns in whole 128-pixel row groups."""
    return g.C == 3 and _c3_layer(g, g.Q in (16, 32, 64) and g.P % (128 // g.Q) == 0)


def _head_bf16(g):
    """The critic's head on bf16 features (csrc/linear_k1.hip): one output, 1x1 input, feature rows of whole 16-byte vectors."""
    return g.K == 1 and g.R == 1 and g.S == 1 and g.H == 1 and g.W == 1 and g.C % 8 == 0


def _f32_or_none(t):
    return t is None or t.dtype == torch.float32


def _wgrad_bf16s_ok(g, gy, x, want_gw, sq, out, row_scale):
    """The bf16-stored weight-gradient kernels take this call (cslgan_conv2d_wgrad_grouped_bf16s; with row_scale
    cslgan_conv2d_wgrad_scaled_bf16s: a K tile of 64 pixels must lie inside one sample, fp32 gradient out, no norms)."""
    return (gy.dtype == x.dtype == torch.bfloat16 and g.K % 8 == 0 and g.C % 8 == 0 and (want_gw or sq is not None)
            and (row_scale is None or ((g.P * g.Q) % 64 == 0 and sq is None and want_gw and _f32_or_none(out))))


def _wgh_shape(S, stride, K, Cc, P, Q):
    """Launches the LDS-resident weight-gradient kernels take (mirrors wgh_eligible in csrc/igemm_wgh.hip): they exist in exact fp32
    (2..5 filter columns) and in the three-piece form (5 columns)."""
    return ((_compute == COMPUTE_F32 or (_compute == COMPUTE_BF16X3 and S == 5)) and stride in (1, 2) and 2 <= S <= 5
            and K % 64 == 0 and Cc % 64 == 0 and P % 8 == 0 and Q % 8 == 0)


_GRAM_MAX_PIX = 64     # (16 was the round-1 rule: ghost clipping for conv4 + linear only)


def _chk_bias_residual(bias, residual, y_shape, allow_bf16=False):
    if bias is not None:
        _chk(bias, "bias")
    if residual is not None:
        _chk(residual, "residual", allow_bf16=allow_bf16)
        if tuple(residual.shape) != tuple(y_shape):
            raise RuntimeError("conv2d_fwd: residual shape %s, expected %s" % (tuple(residual.shape), tuple(y_shape)))


def _conv2d_fwd_stored(g, x, w, bias, residual, act, out, wkey, alg_scale, wversion, out_dtype):
    """conv2d_fwd with bf16-stored activations (x and / or y bfloat16): the bf16-stored kernel when x is bf16 with C % 8 == 0,
    otherwise the fp32 kernels between casts."""
    N, P, Q, K = g.N, g.P, g.Q, g.K
    x_bf16 = x.dtype == torch.bfloat16
    if out_dtype is None:           # follow the input: conv layers answer bf16 activations in kind; heads and 1..4-channel images stay fp32
        out_dtype = torch.bfloat16 if (x_bf16 and P * Q > 1 and K > 4) else torch.float32
    y_bf16 = out_dtype == torch.bfloat16
    if x_bf16 and g.C % 8 == 0 and (K > 4 or P * Q == 1):      # 1..4 output channels of an image: the fp32 vector-ALU kernel below
        y = out if out is not None else torch.empty((N, P, Q, K), device=x.device, dtype=out_dtype)
        if y.dtype != out_dtype:
            raise RuntimeError("conv2d_fwd: out has dtype %s, expected %s" % (y.dtype, out_dtype))
        _chk_bias_residual(bias, residual, (N, P, Q, K), allow_bf16=True)
        ws, repack = repack_cache.get("bf16s_fwd", w, (w.numel() + 1) // 2, wkey, version=wversion)
        _launch("conv2d_fwd", "conv2d_fwd_bf16s", (C.byref(g.desc(COMPUTE_BF16)), _p(x), _p(w), _p(ws), repack, _p(bias), _p(residual),
                                                   1 if _is_bf16(residual) else 0, act, _p(y), 1 if y_bf16 else 0),
                g, lambda: 2.0 * (x.numel() + w.numel()) + y.element_size() * float(N * P * Q * K), "bf16s", flop=lambda: g.flop * alg_scale, exec_flop=lambda: g.flop)
        repack_cache.packed()
        return y
    if x_bf16 and not y_bf16 and _skinny(g) and residual is None and out is None:
        # the generator's output conv (64 -> 3 channels): the vector-ALU kernel reads the bf16-stored input as it is
        y = torch.empty((N, P, Q, K), device=x.device, dtype=torch.float32)
        _chk_bias_residual(bias, None, y.shape)
        _launch("conv2d_fwd", "conv2d_fwd_skinny_bf16in", (C.byref(g.desc(COMPUTE_F32)), _p(x), _p(w), _p(bias), act, _p(y)),
                g, lambda: 2.0 * x.numel() + 4.0 * N * P * Q * K, "bf16in")
        return y
    if x.dtype == torch.float32 and y_bf16 and residual is None and out is None and _c3_fwd(g):
        # the RGB first layer: fp32 image in, bf16-stored activations out of the same kernel (no cast pass)
        y = torch.empty((N, P, Q, K), device=x.device, dtype=torch.bfloat16)
        _chk_bias_residual(bias, None, y.shape)
        _launch("conv2d_fwd", "conv2d_c3_fwd_bf16out", (C.byref(g.desc(COMPUTE_F32)), _p(x), _p(w), _p(bias), act, _p(y)),
                g, lambda: 4.0 * x.numel() + 2.0 * N * P * Q * K, "bf16out")
        return y
    yf = conv2d_fwd(cast_f32(x), w, bias, stride=g.stride, pad=g.pad, residual=cast_f32(residual), act=act, wkey=wkey, alg_scale=alg_scale,
                    wversion=wversion)
    y = cast_bf16(yf) if y_bf16 else yf
    if out is not None:
        out.copy_(y)
        return out
    return y


def in_affine_ok(x, w, stride, pad):
    """Can conv2d_fwd(x, w, in_affine=...) fold a per-(image, channel) affine map into its staging?  The stride-1 launches of the
    LDS-halo kernel (fp32 / three-piece arithmetic) and the 1..4-output-channel kernel (64 input channels)."""
    if not (_GN_FUSE and x.is_cuda and x.dtype == torch.float32 and stride == 1 and x.dim() == 4):
        return False
    N, H, W, Cc = x.shape
    K, R, S, _ = w.shape
    g = _Geom(N, H, W, Cc, K, R, S, stride, pad)
    if K <= 4:
        return _skinny(g) and 1 < R * S
    comp = _kc_compute(N * g.P * g.Q, K, R * S * Cc)
    return comp != COMPUTE_BF16 and _fwd_halo_s1(comp, g)


def groupnorm_affine(part, gamma, beta, groups, eps, N, HW, Cc):
    """(scale, shift)[N, C] of GroupNorm(groups) from a conv epilogue's partial statistics (gn_partials): the normalisation as the
    affine map conv2d_fwd(in_affine=...) applies while it stages its input."""
    pt, n_part = part
    sc = torch.empty((N, Cc), device=pt.device, dtype=torch.float32)
    sh = torch.empty((N, Cc), device=pt.device, dtype=torch.float32)
    check(_lib.lib().cslgan_groupnorm_affine_parts_f32(_p(pt), n_part, _p(gamma), _p(beta), N, HW, Cc, groups, float(eps), _p(sc), _p(sh),
                                                       _stream()), "groupnorm_affine_parts")
    return sc, sh


def conv2d_fwd(x, w, bias=None, stride=1, pad=0, residual=None, act=ACT_NONE, out=None, wkey=None, alg_scale=1.0, wversion=None,
               out_dtype=None, in_affine=None):
    """y[N,P,Q,K] = act(conv(x[N,H,W,C], w[K,R,S,C]) + bias [+ residual[N,P,Q,K]]).

    in_affine = (scale[N,C], shift[N,C], relu): x is replaced by max(scale * x + shift, 0 if relu else -inf) while it is staged
    (cslgan_conv_t.in_scale; only where in_affine_ok says so — an error otherwise).

    alg_scale: FLOP the reference spends on this layer / FLOP of this call (4 for an UpsampleConv's conv, which the
    reference runs over four identical channel groups) — bench accounting only.
    out_dtype: torch.bfloat16 stores the output as bfloat16 (set_storage_dtype); None follows the input's element type."""
    g = _fwd_geom(x, w, stride, pad)
    if x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16 or _is_bf16(residual):
        return _conv2d_fwd_stored(g, x, w, bias, residual, act, out, wkey, alg_scale, wversion, out_dtype)
    alg = g                       # the conv the reference executes (FLOP and byte accounting)
    if g.C == 3 and g.R * g.S > 1 and not (residual is None and _c3_fwd(g)):
        # RGB input on a shape the first-layer kernel (csrc/conv_c3.hip) does not take: a zero 4th channel makes every tap one
        # aligned 16-byte load (scalar gathers ran at 22-32 TF); the zero channel adds nothing to the sums
        x, w, g, wkey = _pad_c4(x), _pad_c4(w), g._replace(C=4), None
    N, P, Q, K = g.N, g.P, g.Q, g.K
    d = _auto_desc(g, "fwd")
    y = out if out is not None else torch.empty((N, P, Q, K), device=x.device, dtype=torch.float32)
    _chk_bias_residual(bias, residual, (N, P, Q, K))
    if in_affine is not None:
        a_sc, a_sh, a_relu = in_affine
        _chk(a_sc, "in_affine scale"); _chk(a_sh, "in_affine shift")
        if tuple(a_sc.shape) != (N, g.C) or tuple(a_sh.shape) != (N, g.C):
            raise RuntimeError("conv2d_fwd: in_affine tables must be [N, C] = [%d, %d]" % (N, g.C))
        d.in_scale, d.in_shift, d.in_relu = a_sc.data_ptr(), a_sh.data_ptr(), 1 if a_relu else 0
    flop, xflop = (lambda: alg.flop * alg_scale), (lambda: g.flop)   # the dense conv the reference executes / this launch
    nbytes = lambda: 4.0 * (alg.N * alg.H * alg.W * alg.C + alg.wsize + N * P * Q * K)
    kind_sfx, s1_key, s1_pieces = _HALO_KIND[d.compute]
    if _halo_arith(d.compute) and _fwd_parity_s2(g, 16, residual) and w.numel() % 8 == 0:
        # parity sub-images through the LDS-halo kernel of the bf16 matrix cores (csrc/igemm_x3.hip): one workspace holds the fp32
        # class matrices and, behind them, their bfloat16 pieces in step-major order
        nw = w.numel()
        ws, repack = repack_cache.get("s2_fwd_" + kind_sfx, w, nw + (3 * nw + 1) // 2, wkey)
        part = _split_scratch(d, N * P * Q, K, g.C, y)
        _launch("conv2d_fwd", "conv2d_s2_fwd_x3_f32", (C.byref(d), _p(x), _p(w), _p(ws), C.c_void_p(ws.data_ptr() + 4 * nw), repack, _p(bias),
                                                       act, _p(y)), g, nbytes, kind_sfx, flop=flop, exec_flop=xflop)
        del part
        repack_cache.packed()
        return y
    if _fwd_parity_s2(g, 32, residual):
        # parity sub-images through the LDS-halo kernel (the C entry falls back to the generic kernel for other grids)
        ws, repack = repack_cache.get("s2_fwd", w, w.numel(), wkey)
        _launch("conv2d_fwd", "conv2d_s2_fwd_f32", (C.byref(d), _p(x), _p(w), _p(ws), repack, _p(bias), act, _p(y)), g, nbytes, "halo",
                flop=flop, exec_flop=xflop)
        repack_cache.packed()
        return y
    if _fwd_halo_s1(d.compute, g):
        # the round-4 LDS-halo kernel reads the filter in step-major order: pre-split into bfloat16 pieces / pre-rounded / as an fp32 copy
        # (cached per parameter version)
        ws, repack = repack_cache.get(s1_key, w, (3 * w.numel() + 1) // 2, wkey, version=wversion)
        req, gpart = gn_partials._req, None
        if req is not None:
            gn_partials._req = None         # one conv per request
            cpg = K // req.groups if K % req.groups == 0 else 0
            if act == ACT_NONE and cpg in (1, 2, 4, 8, 16, 32) and P * Q // 64 <= 64 and K % 64 == 0:
                gpart = torch.empty(N * (P * Q // 64) * req.groups * 2, device=x.device, dtype=torch.float32)
                d.gn_part, d.gn_groups = gpart.data_ptr(), req.groups
                req.part = (gpart, P * Q // 64)
        _launch("conv2d_fwd", "conv2d_fwd_x3_f32", (C.byref(d), _p(x), _p(w), _p(ws), repack, _p(bias), _p(residual), act, _p(y)), g, nbytes,
                flop=flop, exec_flop=xflop)
        if repack:
            repack_cache.set_rebuild(lambda: check(_lib.lib().cslgan_split_filter_x3_f32(_p(w), K, g.R * g.S, g.C, _p(ws), s1_pieces, _stream()), "split_filter_x3"))
        repack_cache.packed()
        return y
    _launch("conv2d_fwd", "conv2d_fwd_f32", (C.byref(d), _p(x), _p(w), _p(bias), _p(residual), act, _p(y)), g, nbytes, flop=flop, exec_flop=xflop)
    return y


def depth_to_space(x, inverse=False):
    """UpsampleConv's data movement (DCResNet_models.py:13-15) on NHWC data: [N,H,W,C] -> [N,2H,2W,C/4] with
    out[n,2h+i,2w+j,c'] = x[n,h,w,4c'+2i+j]; inverse=True maps [N,2H,2W,C/4] back to [N,H,W,C] (its gradient)."""
    if x.dtype == torch.bfloat16:          # parity-test route only (the product path shuffles inside the normalisation kernel)
        return cast_bf16(depth_to_space(cast_f32(x), inverse=inverse))
    _chk(x, "x")
    if inverse:
        N, H2, W2, Cq = x.shape
        if H2 % 2 or W2 % 2:
            raise RuntimeError("depth_to_space(inverse): spatial dims must be even, got %dx%d" % (H2, W2))
        H, W, Cc = H2 // 2, W2 // 2, Cq * 4
        out = torch.empty((N, H, W, Cc), device=x.device, dtype=torch.float32)
    else:
        N, H, W, Cc = x.shape
        if Cc % 4:
            raise RuntimeError("depth_to_space: C=%d is not a multiple of 4 (the HIP UpsampleConv path needs C %% 4 == 0)" % Cc)
        out = torch.empty((N, 2 * H, 2 * W, Cc // 4), device=x.device, dtype=torch.float32)
    check(_lib.lib().cslgan_depth_to_space_f32(_p(x), N, H, W, Cc, 1 if inverse else 0, _p(out), _stream()), "depth_to_space")
    return out


def fold_channels4(w, wkey=None):
    """[K,R,S,C] -> [K,R,S,C/4]: wf[...,c'] = sum_q w[...,c'+q*C/4] — the filter UpsampleConv's conv applies to the
    depth-to-space tensor (whose four channel groups are identical).  Cached per parameter version when wkey is given."""
    _chk(w, "w")
    K, R, S, Cc = w.shape
    if Cc % 4:
        raise RuntimeError("fold_channels4: C=%d is not a multiple of 4" % Cc)
    wf, fresh = repack_cache.get("fold4", w, w.numel() // 4, wkey)
    if fresh:
        fold = lambda: check(_lib.lib().cslgan_fold_channels4_f32(_p(w), K * R * S, Cc, 0, _p(wf), _stream()), "fold_channels4")
        fold()
        repack_cache.set_rebuild(fold)
        repack_cache.packed()
    return wf.view(K, R, S, Cc // 4)


def unfold_channels4(gwf):
    """Gradient of fold_channels4: [K,R,S,C/4] -> [K,R,S,C] with gw[...,c'+q*C/4] = gwf[...,c']."""
    _chk(gwf, "gwf")
    K, R, S, Cq = gwf.shape
    gw = torch.empty((K, R, S, 4 * Cq), device=gwf.device, dtype=torch.float32)
    check(_lib.lib().cslgan_fold_channels4_f32(_p(gwf), K * R * S, 4 * Cq, 1, _p(gw), _stream()), "unfold_channels4")
    return gw


def _pad_c4(t):
    """[..., 3] -> [..., 4] with a zero last channel (one small elementwise pass)."""
    out = torch.zeros(t.shape[:-1] + (4,), device=t.device, dtype=t.dtype)
    out[..., :3] = t
    return out


def _chk_mask(mask, gx, allow_bf16=False):
    if mask is not None:
        _chk(mask, "mask", allow_bf16=allow_bf16)
        if tuple(mask.shape) != tuple(gx.shape):
            raise RuntimeError("conv2d_dgrad: mask shape mismatch")


def _conv2d_dgrad_stored(g, gy, w, in_hw, mask, wkey, out_dtype):
    """conv2d_dgrad with bf16-stored activation gradients: the bf16-stored kernel when gy is bf16 with K % 8 == 0, otherwise the
    fp32 kernels between casts."""
    N, H, W, Cc, K, stride = g.N, g.H, g.W, g.C, g.K, g.stride
    gy_bf16 = gy.dtype == torch.bfloat16
    if out_dtype is None:
        out_dtype = torch.bfloat16 if (gy_bf16 and Cc > 4) else torch.float32
    if mask is not None and mask.dtype != out_dtype:
        mask = cast_bf16(mask) if out_dtype == torch.bfloat16 else cast_f32(mask)
    if (gy.dtype == torch.float32 and out_dtype == torch.bfloat16 and _head_bf16(g) and g.P == 1 and g.Q == 1 and N <= 65535
            and stride == 1 and g.pad == 0):
        # the critic's head: fp32 loss cotangent, bf16 features
        gx = torch.empty((N, 1, 1, Cc), device=gy.device, dtype=torch.bfloat16)
        _chk_mask(mask, gx, allow_bf16=True)
        _launch("conv2d_dgrad", "linear_k1_dgrad_bf16s", (_p(gy), _p(w), _p(mask), N, Cc, _p(gx)), g,
                lambda: 2.0 * N * Cc * (2 if mask is not None else 1) + 4.0 * Cc, "bf16s")
        return gx
    if gy_bf16 and K % 8 == 0 and stride in (1, 2) and Cc > 4:
        gx = torch.empty((N, H, W, Cc), device=gy.device, dtype=out_dtype)
        _chk_mask(mask, gx, allow_bf16=True)
        ws, repack = repack_cache.get("bf16s_dgrad%d" % stride, w, (w.numel() + 1) // 2, wkey)
        _launch("conv2d_dgrad", "conv2d_dgrad_bf16s", (C.byref(g.desc(COMPUTE_BF16)), _p(gy), _p(w), _p(ws), repack, _p(mask), _p(gx),
                                                       1 if out_dtype == torch.bfloat16 else 0),
                g, lambda: 2.0 * (w.numel() + gy.numel()) + gx.element_size() * float(N * H * W * Cc), "bf16s")
        repack_cache.packed()
        return gx
    if (gy_bf16 and out_dtype == torch.float32 and mask is None and Cc <= 4 and K == 64 and stride in (1, 2) and g.R * g.S <= 25
            and H % stride == 0 and W % stride == 0 and (H // stride) % 8 == 0 and (W // stride) % 8 == 0 and (g.R <= 3 or stride == 2)):
        # the critic's first layer: the image gradient from a bf16-stored output gradient on the vector-ALU kernel
        gx = torch.empty((N, H, W, Cc), device=gy.device, dtype=torch.float32)
        ws, repack = repack_cache.get("dgrad%d" % stride, w, w.numel(), wkey)
        _launch("conv2d_dgrad", "conv2d_dgrad_skinny_bf16in", (C.byref(g.desc(COMPUTE_F32)), _p(gy), _p(w), _p(ws), repack, _p(gx)),
                g, lambda: 2.0 * gy.numel() + 4.0 * N * H * W * Cc, "bf16in")
        repack_cache.packed()
        return gx
    gx = conv2d_dgrad(cast_f32(gy), w, in_hw, stride=stride, pad=g.pad, mask=cast_f32(mask), wkey=wkey)
    return cast_bf16(gx) if out_dtype == torch.bfloat16 else gx


def conv2d_dgrad(gy, w, in_hw, stride=1, pad=0, mask=None, wkey=None, out_dtype=None):
    """gx[N,H,W,C] = conv_transpose(gy[N,P,Q,K], w[K,R,S,C]) (* lrelu'(mask)).  out_dtype as for conv2d_fwd."""
    g = _dgrad_geom(gy, w, in_hw, stride, pad)
    if gy.dtype == torch.bfloat16 or out_dtype == torch.bfloat16 or _is_bf16(mask):
        return _conv2d_dgrad_stored(g, gy, w, in_hw, mask, wkey, out_dtype)
    N, H, W, Cc, K = g.N, g.H, g.W, g.C, g.K
    d = _auto_desc(g, "dgrad")
    gx = torch.empty((N, H, W, Cc), device=gy.device, dtype=torch.float32)
    _chk_mask(mask, gx)
    nbytes = lambda: 4.0 * (gx.numel() + w.numel() + gy.numel())
    if (_halo_arith(d.compute) and K % 16 == 0 and Cc >= 64 and Cc % 4 == 0 and g.R * g.S > 1 and w.numel() % 8 == 0
            and (H // stride) % 4 == 0 and (W // stride) % 4 == 0 and H % stride == 0 and W % stride == 0):
        # LDS-halo kernel of the bf16 matrix cores (csrc/igemm_x3.hip): the repacked class matrices and, behind them, their bfloat16
        # pieces in step-major order share one cached workspace
        nw = w.numel()
        sfx = _HALO_KIND[d.compute][0]
        ws, repack = repack_cache.get("dgrad%d_%s" % (stride, sfx), w, nw + (3 * nw + 1) // 2, wkey)
        part = _split_scratch(d, N * H * W, Cc, K, gx)
        _launch("conv2d_dgrad", "conv2d_dgrad_x3_f32", (C.byref(d), _p(gy), _p(w), _p(ws), C.c_void_p(ws.data_ptr() + 4 * nw), repack, _p(mask),
                                                        _p(gx)), g, nbytes, sfx)
        del part
        repack_cache.packed()
        return gx
    ws, repack = repack_cache.get("dgrad%d" % stride, w, w.numel(), wkey)
    _launch("conv2d_dgrad", "conv2d_dgrad_f32", (C.byref(d), _p(gy), _p(w), _p(ws), repack, _p(mask), _p(gx)), g, nbytes)
    repack_cache.packed()
    return gx


def dense_wgrad_group(N, K, Cc, R, S, PQ, stride=1, out_hw=None):
    """Samples per slab for a dense (summed) weight gradient.  The slab count sets the workgroup count, and the launch
    time follows how well that count fills 256 CUs x 3 resident workgroups (800 workgroups take two rounds, 3200 take
    4.2: measured 1.45 vs 1.16 ms on the same 55 GFLOP); more slabs cost their write + re-read by the column sum.
    Model: t(g) = FLOP / (100 TF x fill(g)) + 2 x slab bytes / 4 TB/s, minimised over g | N."""
    if out_hw is not None and _wgh_shape(S, stride, K, Cc, out_hw[0], out_hw[1]):
        # igemm_wgh (LDS-resident operands): (K/128)(C/64)R tiles per slab.  Big launches (the generator's convs, >= 40 GFLOP):
        # ONE slab — the kernel splits the patch loop over workgroups itself (atomic adds), no slab traffic.  Small ones:
        # the largest group that keeps >= 1024 workgroups (scripts/wgrad_group_sweep.py).
        if 2.0 * N * PQ * K * R * S * Cc >= 40e9:
            return N
        tiles = (K // 128 if K % 128 == 0 else K // 64) * (Cc // 64) * R
        best = 1
        g = 1
        while g <= N:
            if N % g == 0 and (N // g) * tiles >= 1024:
                best = g
            g *= 2
        return best
    ndim = R * S * Cc
    bn = 256 if (32 < K <= 64 and ndim >= 1024) else 128
    tiles = ((K + 127) // 128 if K > 64 else 1) * ((ndim + bn - 1) // bn)
    flop = 2.0 * N * PQ * K * ndim
    out_bytes = 4.0 * K * ndim
    best, best_t = 1, None
    g = 1
    while g <= N:
        if N % g == 0:
            blocks = (N // g) * tiles
            if blocks >= 1024 or g == 1:
                rounds = -(-blocks // 768)
                t = flop / (100e12 * blocks / (rounds * 768.0)) + (2.0 * (N // g) * out_bytes / 4e12 if N // g > 1 else 0.0)
                if best_t is None or t < best_t:
                    best, best_t = g, t
        g *= 2
    return best


def gram_norms_eligible(gy_shape, x_shape):
    """Shapes cslgan_conv2d_wgrad_sqnorm_gram_f32 accepts (and where the Gram form is cheaper than the product)."""
    _, P, Q, K = gy_shape
    return P * Q <= 64 and K % 32 == 0 and x_shape[-1] % 32 == 0


def gram_norms_preferred(gy_shape, x_shape, stride):
    """Shapes where the Gram form runs on the pixel-pair kernels (output pixels and input pixels per stride-parity class both
    <= 16: gram_sqnorm_small_kernel; both <= 64: gram_sqnorm_cls64_kernel): there it is far cheaper than the product (the critic's
    conv3: 6.3 vs 105 MFLOP per sample, and no 419 MB of per-sample gradients), so the engine uses it for norms and ghost clipping."""
    _, P, Q, K = gy_shape
    _, H, W, Cc = x_shape
    if P * Q == 1 and H * W == 1:
        return True              # a linear layer: ||gy_b x_b^T||^2 = ||gy_b||^2 ||x_b||^2
    if stride not in (1, 2) or P * Q > _GRAM_MAX_PIX or K % 64 or Cc % 32:
        return False
    return ((H + stride - 1) // stride) * ((W + stride - 1) // stride) <= _GRAM_MAX_PIX


def conv2d_wgrad_sqnorm_gram(gy, x, R, S, stride=1, pad=0, alpha=1.0, sq=None):
    """sq[N] += ||alpha * per-sample weight gradient||^2 from the two PQ x PQ Gram matrices (no gradient formed)."""
    gy, x = cast_f32(gy), cast_f32(x)       # fp32 kernels only (ghost clipping is not combined with bf16 storage)
    _chk(gy, "gy"); _chk(x, "x")
    g = _wgrad_geom("conv2d_wgrad_sqnorm_gram", gy, x, R, S, stride, pad)
    N, PQ = g.N, g.P * g.Q
    if sq is None:
        sq = torch.zeros(N, device=x.device, dtype=torch.float32)
    _chk(sq, "sq")
    if sq.numel() != N:
        raise RuntimeError("conv2d_wgrad_sqnorm_gram: sq needs %d entries" % N)
    if PQ == 1 and g.H * g.W == 1 and R == 1 and S == 1:
        # linear layer: the 1x1 Gram matrices are the two row norms (one pass of the contract norm kernel over gy and x)
        both = sample_sqnorm([gy.reshape(N, g.K), x.reshape(N, g.C)])
        sq.view(-1).addcmul_(both[0], both[1], value=float(alpha) ** 2)
        return sq
    flop = lambda: 2.0 * N * PQ ** 2 * (g.K + R * S * g.C)          # the tap-by-tap Gram form

    def xflop():            # pixel-pair kernels: s^2 class Gram matrices (+ GY GY^T once / per class)
        cls_pix = ((g.H + stride - 1) // stride) * ((g.W + stride - 1) // stride)
        if stride in (1, 2) and PQ <= 16 and cls_pix <= 16:
            return 2.0 * N * (PQ ** 2 * g.K + stride * stride * cls_pix ** 2 * g.C)
        if stride in (1, 2) and PQ <= 64 and cls_pix <= 64:
            return 2.0 * N * stride * stride * 64 * 64 * (g.K + g.C)
        return flop()

    _launch("conv2d_wgrad_gram_norms", "conv2d_wgrad_sqnorm_gram_f32", (C.byref(_auto_desc(g, "gram")), _p(gy), _p(x), float(alpha), _p(sq)),
            g, lambda: 4.0 * (gy.numel() + x.numel()), flop=flop, exec_flop=xflop)
    return sq


def _wgrad_outputs(g, group, x, want_gw, sq, out, row_scale=None, bf16_gw=False):
    """The checked outputs of a weight-gradient route: gw = `out` or a fresh fp32 [N/group,K,R,S,C] (None unless want_gw; a bf16
    `out` only where the route's kernel writes one), sq and row_scale as the kernels read them."""
    gw = None
    if want_gw:
        gw = out if out is not None else torch.empty((g.N // group, g.K, g.R, g.S, g.C), device=x.device, dtype=torch.float32)
        _chk(gw, "gw", allow_bf16=bf16_gw)
    if sq is not None:
        _chk(sq, "sq")
    if row_scale is not None:
        _chk(row_scale, "row_scale")
        if row_scale.numel() != g.N:
            raise RuntimeError("conv2d_wgrad: row_scale needs [N] factors")
    return gw


_WGRAD_NAME = {True: "conv2d_wgrad_grouped", False: "conv2d_wgrad_grouped_normonly"}       # launch-timer name by "a gradient is stored"


def _wgrad_head(g, gy, x, group, alpha, want_gw, sq, out, row_scale):
    """The critic's head: fp32 loss cotangent times bf16 feature rows."""
    N, Cc = g.N, g.C
    _chk(gy, "gy"); _chk(x, "x", allow_bf16=True)
    gw = _wgrad_outputs(g, group, x, want_gw, sq, out, row_scale)
    _launch(_WGRAD_NAME[want_gw], "linear_k1_wgrad_bf16s", (_p(gy), _p(x), _p(row_scale), N, Cc, group, float(alpha), _p(gw), _p(sq)), g,
            lambda: 2.0 * N * Cc + (4.0 * (N // group) * Cc if want_gw else 0.0), "g%d bf16s scaled" if row_scale is not None else "g%d bf16s", (group,))
    return gw


def _wgrad_c3_bf16gy(g, gy, x, alpha, want_gw, sq, out):
    """The RGB first layer: bf16-stored output gradient, fp32 image, the first-layer kernel reads gy as stored."""
    _chk(gy, "gy", allow_bf16=True); _chk(x, "x")
    gw = _wgrad_outputs(g, 1, x, want_gw, sq, out)
    _launch(_WGRAD_NAME[want_gw], "conv2d_c3_wgrad_bf16gy", (C.byref(g.desc(COMPUTE_F32)), _p(gy), _p(x), float(alpha), _p(gw), _p(sq)), g,
            lambda: 4.0 * x.numel() + 2.0 * gy.numel(), "g1 bf16gy")
    return gw


def _wgrad_bf16s(g, gy, x, group, alpha, want_gw, sq, out, row_scale):
    """bf16 gy and bf16 x (cslgan_conv2d_wgrad_grouped_bf16s): fp32 (or bf16) gw and / or sq.  row_scale [N] (clip-weighted sums):
    cslgan_conv2d_wgrad_scaled_bf16s — the fp32 weight meets each sample's accumulated product."""
    _chk(gy, "gy", allow_bf16=True); _chk(x, "x", allow_bf16=True)
    if g.N % group:
        raise RuntimeError("conv2d_wgrad: N=%d not divisible by group=%d" % (g.N, group))
    d = g.desc(COMPUTE_BF16)
    gw = _wgrad_outputs(g, group, x, want_gw, sq, out, row_scale, bf16_gw=True)
    nbytes = lambda: 2.0 * (x.numel() + gy.numel()) + (float(gw.element_size()) * ((g.N // group) * g.wsize) if want_gw else 0.0)
    if row_scale is not None:
        _launch("conv2d_wgrad_grouped", "conv2d_wgrad_scaled_bf16s", (C.byref(d), _p(gy), _p(x), _p(row_scale), group, float(alpha), _p(gw)),
                g, nbytes, "g%d bf16s scaled", (group,))
        return gw
    _launch(_WGRAD_NAME[want_gw], "conv2d_wgrad_grouped_bf16s", (C.byref(d), _p(gy), _p(x), group, float(alpha), _p(gw), 1 if _is_bf16(gw) else 0,
                                                                 _p(sq)), g, nbytes, "g%d bf16s", (group,))
    return gw


def _wgrad_rgb_padded(gy, x, R, S, stride, pad, group, alpha, want_gw, sq, out):
    """RGB input on a shape the first-layer kernel does not take: run on a zero-padded 4th channel (aligned 16-byte gathers), then
    drop that channel's (zero) gradients."""
    g4 = conv2d_wgrad_grouped(gy, _pad_c4(x), R, S, stride=stride, pad=pad, group=group, alpha=alpha, want_gw=want_gw, sq=sq)
    if g4 is None:
        return None
    if out is not None:
        out.view(g4.shape[:-1] + (3,)).copy_(g4[..., :3])
        return out
    return g4[..., :3].contiguous()


def conv2d_wgrad_grouped(gy, x, R, S, stride=1, pad=0, group=1, alpha=1.0, want_gw=True, sq=None, out=None, row_scale=None):
    """gw[N/group,K,R,S,C] (per-group weight gradients) and/or sq[N/group] += ||alpha*gw_g||^2.
    row_scale [N]: gy of sample n is weighted by row_scale[n] (clip-weighted sums; fp32 output, no sq)."""
    g = _wgrad_geom("conv2d_wgrad", gy, x, R, S, stride, pad)
    N, K, Cc, P, Q = g.N, g.K, g.C, g.P, g.Q
    if gy.dtype == torch.bfloat16 or x.dtype == torch.bfloat16:
        if _wgrad_bf16s_ok(g, gy, x, want_gw, sq, out, row_scale):
            return _wgrad_bf16s(g, gy, x, group, alpha, want_gw, sq, out, row_scale)
        if (gy.dtype == torch.float32 and x.dtype == torch.bfloat16 and _head_bf16(g) and _f32_or_none(out)
                and N % group == 0 and N // group <= 65535 and (row_scale is None or (sq is None and want_gw))):
            return _wgrad_head(g, gy, x, group, alpha, want_gw, sq, out, row_scale)
        if (gy.dtype == torch.bfloat16 and x.dtype == torch.float32 and _c3_wgrad(g) and group == 1 and row_scale is None
                and _f32_or_none(out) and (want_gw or sq is not None)):
            return _wgrad_c3_bf16gy(g, gy, x, alpha, want_gw, sq, out)
        gy, x = cast_f32(gy), cast_f32(x)       # mixed element types / shapes the bf16-stored kernel does not take
    _chk(gy, "gy"); _chk(x, "x")
    c3 = _c3_wgrad(g) and group == 1 and row_scale is None and _f32_or_none(out)
    if Cc == 3 and R * S > 1 and row_scale is None and _f32_or_none(out) and not c3:
        return _wgrad_rgb_padded(gy, x, R, S, stride, pad, group, alpha, want_gw, sq, out)
    if N % group:
        raise RuntimeError("conv2d_wgrad: N=%d not divisible by group=%d" % (N, group))
    G = N // group
    d = _auto_desc(g, "wgrad", group)
    if row_scale is not None:
        if sq is not None or not want_gw:
            raise RuntimeError("conv2d_wgrad: row_scale needs [N] factors, a gradient output and no sq")
        gw = _wgrad_outputs(g, group, x, True, None, out, row_scale)
        _launch("conv2d_wgrad_grouped", "conv2d_wgrad_scaled_f32", (C.byref(d), _p(gy), _p(x), _p(row_scale), group, float(alpha), _p(gw)),
                g, lambda: 4.0 * (x.numel() + gy.numel() + G * g.wsize), "g%d scaled", (group,))
        return gw
    scratch = False
    if not want_gw and sq is not None:
        # norms only, but a layer with a handful of tiles and a long pixel loop (the 3-channel first conv) runs several
        # times faster when its pixels are split over workgroups, which needs a (small) output to accumulate into
        tiles = ((K + 63) // 64) * ((R * S * Cc + 127) // 128) * G
        if not c3 and tiles < 192 and group * P * Q >= 512 and G * K * R * S * Cc <= (1 << 22):
            want_gw, scratch = True, True
    gw = _wgrad_outputs(g, group, x, want_gw, sq, out, bf16_gw=True)
    nbytes = lambda: 4.0 * (x.numel() + gy.numel()) + (float(gw.element_size()) * (G * g.wsize) if want_gw else 0.0)
    _launch(_WGRAD_NAME[want_gw and not scratch], "conv2d_wgrad_grouped_bf16out_f32" if _is_bf16(gw) else "conv2d_wgrad_grouped_f32",
            (C.byref(d), _p(gy), _p(x), group, float(alpha), _p(gw), _p(sq)), g, nbytes, "g%d", (group,))
    return None if scratch else gw


def wgrad_blocks_eligible(gy_shape, x_shape, R, S, stride):
    """Shapes cslgan_conv2d_wgrad_blocks_f32 takes (the LDS-resident fp32 kernel)."""
    _, P, Q, K = gy_shape
    return _wgh_shape(S, stride, K, x_shape[-1], P, Q)


def conv2d_wgrad_blocks(gy, x, R, S, stride, pad, alpha, blocks):
    """Per-sample weight gradients of consecutive row blocks in ONE launch.  blocks: [(n_rows, gw_out or None, sq or None)] —
    gw_out [n_rows, K*R*S*C] fp32 (None: nothing stored), sq [n_rows] accumulated (None: no norms)."""
    _chk(gy, "gy"); _chk(x, "x")
    g = _wgrad_geom("conv2d_wgrad_blocks", gy, x, R, S, stride, pad)
    if sum(b[0] for b in blocks) != g.N:
        raise RuntimeError("conv2d_wgrad_blocks: blocks inconsistent with x %s" % (tuple(x.shape),))
    per_row = g.wsize
    nb = len(blocks)
    first = (C.c_int32 * nb)()
    gws, sqs = (C.c_void_p * nb)(), (C.c_void_p * nb)()
    r0 = 0
    for i, (n, gw, sq) in enumerate(blocks):
        first[i] = r0
        r0 += n
        if gw is not None:
            _chk(gw, "gw")
            if gw.numel() != n * per_row:
                raise RuntimeError("conv2d_wgrad_blocks: gw of block %d has %d elements, expected %d" % (i, gw.numel(), n * per_row))
        if sq is not None:
            _chk(sq, "sq")
            if sq.numel() != n:
                raise RuntimeError("conv2d_wgrad_blocks: sq of block %d needs %d entries" % (i, n))
        gws[i] = None if gw is None else gw.data_ptr()
        sqs[i] = None if sq is None else sq.data_ptr()
    nbytes = lambda: 4.0 * (x.numel() + gy.numel() + sum(b[1].numel() for b in blocks if b[1] is not None))
    _launch("conv2d_wgrad_grouped", "conv2d_wgrad_blocks_f32", (C.byref(_auto_desc(g, "wgrad")), _p(gy), _p(x), float(alpha), nb, first, gws, sqs),
            g, nbytes, "g1 blocks%d", (nb,))


def conv2d_wgrad_dense(gy, x, R, S, stride=1, pad=0, alpha=1.0, row_scale=None, out=None, want_rows=False):
    """The summed weight gradient [K,R,S,C] of a batch: slabs of the grouped MFMA kernel + a column sum, or the
    vector-ALU kernel for 1..4 output channels.  out (optional, flat fp32 [K*R*S*C]): destination of the sum.
    want_rows: return the UN-SUMMED slabs [n_slabs, K*R*S*C] instead (the caller column-sums them together with other
    contributions in one launch: PrivacyEngine._add_dense_rows)."""
    g = _wgrad_geom("conv2d_wgrad_dense", gy, x, R, S, stride, pad)
    N, K, Cc, P, Q = g.N, g.K, g.C, g.P, g.Q
    if gy.dtype == torch.float32 and x.dtype == torch.bfloat16 and _head_bf16(g):
        # the critic's head on bf16 features: weighted sums of feature rows in slabs of 8 samples + a column sum
        slabs = conv2d_wgrad_grouped(gy, x, 1, 1, group=8 if N % 8 == 0 else 1, alpha=alpha, row_scale=row_scale)
        res = torch.empty(Cc, device=x.device, dtype=torch.float32) if out is None else out
        sum_rows(slabs.reshape(slabs.shape[0], -1), res.view(-1))
        return res.view(1, 1, 1, -1)
    c3 = row_scale is None and _c3_wgrad(g)         # the grouped call below runs the first-layer kernel (group 1, fp32 slabs)
    if ((gy.dtype == torch.bfloat16 or x.dtype == torch.bfloat16) and not (c3 and gy.dtype == torch.bfloat16 and x.dtype == torch.float32)
            and not _wgrad_bf16s_ok(g, gy, x, True, None, None, row_scale)):
        gy, x = cast_f32(gy), cast_f32(x)
    if _skinny(g) and row_scale is None:
        _chk(gy, "gy"); _chk(x, "x")
        nb = min(512, N * (P // 8) * (Q // 8))
        partial = torch.empty((nb, g.wsize), device=x.device, dtype=torch.float32)
        _launch("conv2d_wgrad_grouped", "conv2d_wgrad_skinny_f32", (C.byref(_auto_desc(g, "wgrad")), _p(gy), _p(x), float(alpha), _p(partial), nb),
                g, lambda: 4.0 * (x.numel() + gy.numel()), "skinny", tag_stride=False)
        out = torch.empty(g.wsize, device=x.device, dtype=torch.float32) if out is None else out
        sum_rows(partial, out)
        return out.view(K, R, S, Cc)
    # first-layer kernel: per-image gradients (19 KB each), summed below
    group = 1 if c3 else dense_wgrad_group(N, K, Cc, R, S, P * Q, stride=stride, out_hw=(P, Q))
    slabs = conv2d_wgrad_grouped(gy, x, R, S, stride=stride, pad=pad, group=group, alpha=alpha, row_scale=row_scale)
    if want_rows and out is None:
        return slabs.reshape(slabs.shape[0], -1)
    if slabs.shape[0] == 1:
        if out is not None:
            out.copy_(slabs[0].reshape(-1))
            return out.view(slabs.shape[1:])
        return slabs[0]
    out = torch.empty(slabs[0].numel(), device=x.device, dtype=torch.float32) if out is None else out
    sum_rows(slabs.reshape(slabs.shape[0], -1), out.view(-1))
    return out.view(slabs.shape[1:])


def norm_act_bwd(x, dy, y, gamma, stats, rows_per_stat, groups, eps, relu):
    """Backward of groupnorm_act / batchnorm_act: returns (dx, dgamma, dbeta)."""
    for t, n in ((x, "x"), (dy, "dy"), (gamma, "gamma"), (stats, "stats")):
        _chk(t, n)
    if relu and y is not None:      # (a missing y is the library's error)
        _chk(y, "y")
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    L = _lib.lib()
    ws = torch.empty(L.cslgan_norm_bwd_ws_floats(rows, rows_per_stat, Cc, groups), device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, device=x.device, dtype=torch.float32)
    dbeta = torch.empty(Cc, device=x.device, dtype=torch.float32)
    check(L.cslgan_norm_act_bwd_f32(_p(x), _p(dy), _p(y), _p(gamma), _p(stats), rows, rows_per_stat, Cc, groups, float(eps),
                                    1 if relu else 0, _p(ws), _p(dx), _p(dgamma), _p(dbeta), _stream()), "norm_act_bwd")
    return dx, dgamma, dbeta


def bias_grad_grouped(gy, group=1, alpha=1.0, want_gb=True, sq=None, out=None):
    N, K = gy.shape[0], gy.shape[-1]
    PQ = gy.numel() // (N * K)
    gb = None
    if want_gb:
        gb = out if out is not None else torch.empty((N // group, K), device=gy.device, dtype=torch.float32)
    if gy.dtype == torch.bfloat16:
        if K % 8 == 0 and K <= 2048 and 256 % (K // 8) == 0:
            _chk(gy, "gy", allow_bf16=True)
            check(_lib.lib().cslgan_bias_grad_grouped_bf16(_p(gy), N, PQ, K, group, float(alpha), _p(gb), _p(sq), _stream()), "bias_grad_bf16")
            return gb
        gy = cast_f32(gy)
    _chk(gy, "gy")
    check(_lib.lib().cslgan_bias_grad_grouped_f32(_p(gy), N, PQ, K, group, float(alpha), _p(gb), _p(sq), _stream()), "bias_grad")
    return gb


def _segs(ins: Sequence[torch.Tensor], outs=None, noises=None, ragged=False):
    """ragged: the segments may have different row counts (column sums only: cslgan_segs_t.rows)."""
    s = SegsT()
    if len(ins) > _lib.MAX_SEGS:
        raise RuntimeError("at most %d segments per launch" % _lib.MAX_SEGS)
    s.n_seg = len(ins)
    n_rows = ins[0].shape[0] if len(ins) else 0
    if ragged:
        n_rows = max(t.shape[0] for t in ins)
    for i, t in enumerate(ins):
        _chk(t, "segment %d" % i, allow_bf16=True)
        if t.dtype != ins[0].dtype:
            raise RuntimeError("segments of one launch must share a dtype")
        if t.dim() != 2 or (t.shape[0] != n_rows and not ragged):
            raise RuntimeError("segments must be 2-D [n_rows, len] with equal n_rows")
        if ragged:
            s.rows[i] = t.shape[0]
        s.inp[i] = t.data_ptr()
        s.len[i] = t.shape[1]
        s.row_stride[i] = t.shape[1]
        if outs is not None:
            _chk(outs[i], "out %d" % i)
            if outs[i].numel() != t.shape[1]:
                raise RuntimeError("out %d has %d elements, expected %d" % (i, outs[i].numel(), t.shape[1]))
            s.out[i] = outs[i].data_ptr()
        if noises is not None and noises[i] is not None:
            _chk(noises[i], "noise %d" % i)
            if noises[i].numel() != t.shape[1]:
                raise RuntimeError("noise %d size mismatch" % i)
            s.noise[i] = noises[i].data_ptr()
    return s, n_rows


def _take_rows(t, idx):
    """t[idx] for a list of row indices WITHOUT building an index tensor on the host (that is a host-to-device copy, which a HIP-graph
    capture refuses): a slice when the indices are consecutive, a stack of row views otherwise."""
    if all(b - a == 1 for a, b in zip(idx, idx[1:])):
        return t[idx[0]:idx[-1] + 1].contiguous()
    return torch.stack([t[j] for j in idx])


def _by_dtype(mats):
    """Index lists of the fp32 and the bf16 segments (a launch handles one element type)."""
    parts = {}
    for i, m in enumerate(mats):
        parts.setdefault(m.dtype, []).append(i)
    return parts


def sample_sqnorm(mats: Sequence[torch.Tensor]) -> torch.Tensor:
    """mats: list of [n_rows, len_i] (fp32 or bf16) -> [n_seg, n_rows] squared row norms."""
    n_rows = mats[0].shape[0]
    out = torch.empty((len(mats), n_rows), device=mats[0].device, dtype=torch.float32)
    L = _lib.lib()
    for dt, idx in _by_dtype(mats).items():
        fn = L.cslgan_sample_sqnorm_bf16 if dt == torch.bfloat16 else L.cslgan_sample_sqnorm_f32
        for i in range(0, len(idx), _lib.MAX_SEGS):
            sub = idx[i:i + _lib.MAX_SEGS]
            chunk = [mats[j] for j in sub]
            s, _ = _segs(chunk)
            o = torch.empty((len(chunk), n_rows), device=chunk[0].device, dtype=torch.float32)
            nbytes = float(sum(n_rows * m.shape[1] * m.element_size() for m in chunk))
            _timed("sample_sqnorm", 0.0, nbytes, lambda: check(fn(C.byref(s), n_rows, _p(o), _stream()), "sample_sqnorm"))
            if len(sub) == len(mats):
                return o
            for k, j in enumerate(sub):
                out[j].copy_(o[k])
    return out


def clip_factors(sq, max_norm, flat, eps=1e-6, first_private_row=0, want_norms=False):
    """sq [n_seg,n_rows], max_norm device tensor [1] (flat) or [n_seg] -> factors ([n_rows] | [n_seg,n_rows])."""
    _chk(sq, "sq"); _chk(max_norm, "max_norm")
    n_seg, n_rows = sq.shape
    if max_norm.numel() != (1 if flat else n_seg):
        raise RuntimeError("clip_factors: max_norm has %d entries" % max_norm.numel())
    shape = (n_rows,) if flat else (n_seg, n_rows)
    f = torch.empty(shape, device=sq.device, dtype=torch.float32)
    nrm = torch.empty(shape, device=sq.device, dtype=torch.float32) if want_norms else None
    check(_lib.lib().cslgan_clip_factors_f32(_p(sq), n_seg, n_rows, _p(max_norm), 1 if flat else 0, float(eps),
                                             int(first_private_row), _p(f), _p(nrm), _stream()), "clip_factors")
    return (f, nrm) if want_norms else f


def adaptive_clip(sq_adapt, sq_rows, stat_max, scalar, per_layer, eps, first_private_row, mat_layers=(), jobs=()):
    """cslgan_adaptive_clip_f32: sq_adapt / sq_rows are lists (one entry per layer) of 1-D fp32 device tensors of equal length each;
    jobs = [(dst tensor [count], layer, first row, scale)].  Returns (r [L], C [L] | [1], sq [L, n_rows], f, f_mat | None)."""
    L = len(sq_rows)
    if L > _lib.MAX_CLIP_LAYERS or len(jobs) > _lib.MAX_CLIP_JOBS or len(mat_layers) > _lib.MAX_CLIP_LAYERS:
        raise RuntimeError("adaptive_clip: too many layers / jobs for one launch")
    n_adapt, n_rows = sq_adapt[0].numel(), sq_rows[0].numel()
    a = _lib.AdaptiveClipT()
    a.n_layers, a.n_mat, a.n_jobs = L, len(mat_layers), len(jobs)
    for l in range(L):
        _chk(sq_adapt[l], "sq_adapt"); _chk(sq_rows[l], "sq_rows")
        if sq_adapt[l].numel() != n_adapt or sq_rows[l].numel() != n_rows:
            raise RuntimeError("adaptive_clip: ragged norm vectors")
        a.sq_adapt[l], a.sq_rows[l] = sq_adapt[l].data_ptr(), sq_rows[l].data_ptr()
    for m, l in enumerate(mat_layers):
        a.mat_layer[m] = int(l)
    for j, (dst, layer, first, scale) in enumerate(jobs):
        _chk(dst, "job dst")
        a.job_dst[j], a.job_layer[j], a.job_first[j], a.job_count[j], a.job_scale[j] = dst.data_ptr(), int(layer), int(first), dst.numel(), float(scale)
    dev = sq_rows[0].device
    r = torch.empty(L, device=dev, dtype=torch.float32)
    c = torch.empty(L if per_layer else 1, device=dev, dtype=torch.float32)
    sq = torch.empty((L, n_rows), device=dev, dtype=torch.float32)
    f = torch.empty((L, n_rows) if per_layer else (n_rows,), device=dev, dtype=torch.float32)
    f_mat = torch.empty((len(mat_layers), n_rows), device=dev, dtype=torch.float32) if (mat_layers and per_layer) else None
    check(_lib.lib().cslgan_adaptive_clip_f32(C.byref(a), n_adapt, n_rows, 1 if stat_max else 0, float(scalar), 1 if per_layer else 0, float(eps),
                                              int(first_private_row), _p(r), _p(c), _p(sq), _p(f), _p(f_mat), _stream()), "adaptive_clip")
    return r, c, sq, f, f_mat


class deferred_sums:
    """Inside this context the column sums requested through sum_rows() are only queued; they run as ONE multi-segment launch
    (segments of different heights: cslgan_segs_t.rows) at exit.  For callers that take several dense weight gradients and read
    none of them before the block ends — the parameter gradients of the gradient penalty (train.py:427), which were nine
    latency-sized launches per step.  A queued destination holds garbage until the flush: never use this around code that consumes
    a sum inside the block (autograd accumulating two contributions into one parameter, a double backward)."""

    def __enter__(self):
        global _pending_sums
        self._prev, _pending_sums = _pending_sums, []
        return self

    def __exit__(self, *exc):
        global _pending_sums
        pend, _pending_sums = _pending_sums, self._prev
        if exc[0] is None:
            flush_sums(pend)


_pending_sums = None


def flush_sums(pend):
    for i in range(0, len(pend), _lib.MAX_SEGS):
        chunk = pend[i:i + _lib.MAX_SEGS]
        clip_accum_noise([m for m, _ in chunk], [o for _, o in chunk], ragged=True)


def sum_rows(slabs, out):
    """out[len] = sum over the rows of slabs [n, len] (fp32) — queued when a deferred_sums block is open."""
    if _pending_sums is not None and slabs.dtype == torch.float32:
        _pending_sums.append((slabs, out))
        return out
    clip_accum_noise([slabs], [out])
    return out


PHILOX_MAX_TENSORS = 64            # include/cslgan.h "Device random streams": first_index < 64


def clip_accum_noise(mats, outs, factors=None, noise_std=None, noises=None, seed=0, offset=0, scale=1.0, beta=0.0, call_counter=None,
                     ragged=False):
    """outs[i] = beta*outs[i] + scale*(sum_r f_r * mats[i][r] + noise_std[i]*z_i).  mats may mix fp32 and bf16
    segments (one launch per element type, fp32 accumulation either way).  call_counter: device int64 [1] whose value is
    added to `offset` inside the kernel (graph-captured steps: the counter lives in HBM, not in the launch arguments).
    ragged: the segments may have different row counts (plain column sums: no factors).
    Philox noise (noise_std without noises): tensor i draws the stream of (seed, offset + *call_counter, i) — include/cslgan.h
    "Device random streams"; at most 64 tensors per call, and the caller never repeats (seed, offset + *call_counter)."""
    if ragged and factors is not None:
        raise RuntimeError("clip_accum_noise: ragged segments take no clip factors")
    if noise_std is not None and noises is None and len(mats) > PHILOX_MAX_TENSORS:
        # a launch's stream offset is 64 * (offset + call counter) + the position of its first tensor: position 64 of this call
        # would draw exactly the normals of position 0 of the next one
        raise RuntimeError("clip_accum_noise: Philox noise for at most %d tensors per call, got %d (a tensor's position takes the low "
                           "6 bits of the stream offset; beyond that it repeats the next call's noise)" % (PHILOX_MAX_TENSORS, len(mats)))
    L = _lib.lib()
    if factors is not None:
        _chk(factors, "factors")
    if noise_std is not None:
        _chk(noise_std, "noise_std")
    for dt, idx in _by_dtype(mats).items():
        fn = L.cslgan_clip_accum_noise_bf16 if dt == torch.bfloat16 else L.cslgan_clip_accum_noise_f32
        for i in range(0, len(idx), _lib.MAX_SEGS):
            sub = idx[i:i + _lib.MAX_SEGS]
            whole = len(sub) == len(mats)
            s, n_rows = _segs([mats[j] for j in sub], [outs[j] for j in sub], None if noises is None else [noises[j] for j in sub], ragged=ragged)
            if call_counter is not None:
                if call_counter.dtype != torch.int64 or not call_counter.is_cuda:
                    raise RuntimeError("call_counter must be a device int64 tensor")
                s.call_counter = call_counter.data_ptr()
            per_seg, f = 0, None
            if factors is not None:
                if factors.dim() == 2:
                    per_seg = 1
                    f = factors if whole else _take_rows(factors, sub)
                else:
                    f = factors
            ns = None
            if noise_std is not None:
                ns = noise_std if whole else _take_rows(noise_std, sub)
            nbytes = float(sum(mats[j].shape[0] * mats[j].shape[1] * mats[j].element_size() + 4 * mats[j].shape[1] for j in sub))
            # the Philox stream is keyed by (offset, segment index within the launch): make it unique per launch
            _timed("clip_accum_noise", 0.0, nbytes, lambda: check(
                fn(C.byref(s), n_rows, _p(f), per_seg, _p(ns), int(seed), int(offset) * 64 + sub[0], float(scale), float(beta),
                   _stream()), "clip_accum_noise"))


def l2_clip_rows(t, Cval):
    _chk(t, "t")
    n = t.shape[0]
    flat = t.reshape(n, -1)
    out = torch.empty_like(flat)
    ws = torch.empty(n, device=t.device, dtype=torch.float32)
    check(_lib.lib().cslgan_l2_clip_rows_f32(_p(flat), _p(out), n, flat.shape[1], float(Cval), _p(ws), _stream()), "l2_clip_rows")
    return out.reshape(t.shape)


def mean_sample(mean_samples, labels, perms, noise_mean_std, noise_std, seed, offset, n=None, want_labels=False, out=None):
    """MeanSampler.sample's gather + per-image jitter + per-pixel noise (mean_sampler.py:75-84) in one pass.
    mean_samples [n_classes, num_samples, ...] fp32, labels / perms [n] int64 or None: missing permutations (and, with several
    classes, missing labels) are drawn inside the kernel; n is then required.  want_labels: also return the labels used."""
    _chk(mean_samples, "mean_samples")
    n_cls, num = mean_samples.shape[0], mean_samples.shape[1]
    if perms is not None:
        n = perms.numel()
    elif n is None:
        raise RuntimeError("mean_sample: n is required when the kernel draws the permutations")
    elif num > 1024:
        raise RuntimeError("mean_sample: in-kernel permutations need num_samples <= 1024")
    ln = mean_samples[0, 0].numel()
    for t, nm in ((labels, "labels"), (perms, "perms")):
        if t is not None and (t.dtype != torch.int64 or not t.is_cuda or t.numel() != n):
            raise RuntimeError("mean_sample: %s must be an int64 device tensor of %d entries" % (nm, n))
    if out is None:
        out = torch.empty((n,) + tuple(mean_samples.shape[2:]), device=mean_samples.device, dtype=torch.float32)
    else:           # caller-owned destination (a slice of the trainer's fused critic batch): n dense rows of ln floats
        _chk(out, "out")
        if out.numel() != n * ln:
            raise RuntimeError("mean_sample: out has %d elements, expected %d" % (out.numel(), n * ln))
    lab_out = torch.empty(n, device=mean_samples.device, dtype=torch.int64) if (want_labels and labels is None and n_cls > 1) else None
    check(_lib.lib().cslgan_mean_sample_f32(_p(mean_samples), n_cls, num, ln, None if labels is None else _p(labels.contiguous()),
                                            None if perms is None else _p(perms.contiguous()), n,
                                            float(noise_mean_std or 0.0), float(noise_std or 0.0), int(seed) & (2 ** 64 - 1),
                                            int(offset) & (2 ** 64 - 1), _p(out), _p(lab_out), _stream()), "mean_sample")
    if want_labels:
        return out, (labels if labels is not None else lab_out)
    return out


def latent_normal(seed, first_index, n, dim, first_index_dev=None, n_classes=1, fixed_label=-1, want_labels=False, out=None, labels_out=None,
                  device=None):
    """The generator's latent rows of samples first_index + *first_index_dev + (0 .. n-1): [n, dim] unit normals of the indexed
    stream of include/cslgan.h "Device random streams" (sample g is a function of (seed, g) alone).  first_index_dev: device int64
    [1] added inside the kernel (a recorded graph draws new rows on every replay).  want_labels / labels_out: also the labels,
    fixed_label when >= 0 else g mod n_classes.  out / labels_out: caller-owned destinations (static buffers of a recorded graph)."""
    if out is None:
        out = torch.empty((n, dim), device=device if device is not None else "cuda", dtype=torch.float32)
    else:
        _chk(out, "out")
        if tuple(out.shape) != (n, dim):
            raise RuntimeError("latent_normal: out is %s, expected %s" % (tuple(out.shape), (n, dim)))
    if labels_out is None and want_labels:
        labels_out = torch.empty(n, device=out.device, dtype=torch.int64)
    if labels_out is not None and (labels_out.dtype != torch.int64 or not labels_out.is_cuda or labels_out.numel() != n or not labels_out.is_contiguous()):
        raise RuntimeError("latent_normal: labels_out must be a contiguous int64 device tensor of %d entries" % n)
    if first_index_dev is not None and (first_index_dev.dtype != torch.int64 or not first_index_dev.is_cuda or first_index_dev.numel() != 1):
        raise RuntimeError("latent_normal: first_index_dev must be a device int64 tensor of one entry")
    check(_lib.lib().cslgan_latent_normal_f32(int(seed) & (2 ** 64 - 1), int(first_index) & (2 ** 64 - 1), _p(first_index_dev), n, dim, _p(out),
                                              int(n_classes), int(fixed_label), _p(labels_out), _stream()), "latent_normal")
    return (out, labels_out) if (want_labels or labels_out is not None) else out


def f32_to_u8(src, scale, bias, out=None):
    """uint8 bytes of a dense fp32 device tensor in its memory order: clamp(src * scale + bias, 0, 1) * 255 + 0.5, truncated —
    bit-identical to util.denorm_celeba + util.save_image's quantisation on the host ((0.5, 0.5); (1, 0) for [0, 1] images)."""
    _chk(src, "src", any_order=True)
    if out is None:
        out = torch.empty(src.numel(), device=src.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_cuda or out.numel() != src.numel() or not out.is_contiguous():
        raise RuntimeError("f32_to_u8: out must be a contiguous uint8 device tensor of %d entries" % src.numel())
    check(_lib.lib().cslgan_f32_to_u8(_p(src), src.numel(), float(scale), float(bias), _p(out), _stream()), "f32_to_u8")
    return out


def attack_trials(vt, vn, n, m, seed, first_trial, trials, out=None):
    """hits[t], t < trials: train samples among the n best of trial first_trial + t of the membership-inference estimate
    (mem_inf_attack.py:29-66; sampler and tie rule under include/cslgan.h "Audit sampler") — uint32 stored as an int32 device tensor.
    vt [N] / vn [M]: the train / non-train scores; n + m <= 4096.  csl_gan_amd.audit.trial_hits is the host model."""
    _chk(vt, "vt")
    if vn is not None and vn.numel():
        _chk(vn, "vn")
    else:
        vn = None
    M = 0 if vn is None else vn.numel()
    if out is None:
        out = torch.empty(int(trials), device=vt.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or not out.is_cuda or out.numel() != int(trials) or not out.is_contiguous():
        raise RuntimeError("attack_trials: out must be a contiguous int32 device tensor of %d entries" % int(trials))
    check(_lib.lib().cslgan_attack_trials(_p(vt), vt.numel(), _p(vn), M, int(n), int(m), int(seed) & (2 ** 64 - 1),
                                          int(first_trial) & (2 ** 64 - 1), int(trials), _p(out), _stream()), "attack_trials")
    return out


def rank_counts(a, b):
    """(gt, eq), int32 device tensors of a.numel() entries: gt[i] = #{j : a[i] > b[j]}, eq[i] = #{j : a[i] == b[j]} (IEEE compares)."""
    _chk(a, "a")
    if b.numel():
        _chk(b, "b")
    elif not b.is_cuda:
        raise RuntimeError("b must be a device tensor (csl_gan_amd.ops has no CPU path)")
    gt = torch.empty(a.numel(), device=a.device, dtype=torch.int32)
    eq = torch.empty(a.numel(), device=a.device, dtype=torch.int32)
    check(_lib.lib().cslgan_rank_counts(_p(a), a.numel(), _p(b) if b.numel() else None, b.numel(), _p(gt), _p(eq), _stream()), "rank_counts")
    return gt, eq


def softmax_max_rows(logits, out=None):
    """softmax(logits, 1).max(1)[0] of [B, n_classes <= 64] fp32 logits (mem_inf_attack.py:80) in one launch."""
    _chk(logits, "logits")
    if logits.dim() != 2:
        raise RuntimeError("softmax_max_rows: logits must be [B, n_classes], got %s" % (tuple(logits.shape),))
    B, Cn = logits.shape
    if out is None:
        out = torch.empty(B, device=logits.device, dtype=torch.float32)
    else:
        _chk(out, "out")
        if out.numel() != B:
            raise RuntimeError("softmax_max_rows: out has %d entries, expected %d" % (out.numel(), B))
    check(_lib.lib().cslgan_softmax_max_rows_f32(_p(logits), B, Cn, _p(out), _stream()), "softmax_max_rows")
    return out


def _logreg_shapes(X, U, what):
    if X.dim() != 2 or U.dim() != 2 or U.shape[0] != X.shape[1] + 1:
        raise RuntimeError("%s: need X [N, D] and U [D + 1, K], got %s and %s" % (what, tuple(X.shape), tuple(U.shape)))
    return X.shape[0], X.shape[1], U.shape[1]


def _ovr_eval_outputs(what, X, labels, U, out_loss, out_grad):
    """What the three ovr_*_eval wrappers share once X [N, D] and U [P, K] have their shapes: labels must be N int32 entries on the
    device, and (out_loss [K], out_grad like U) are checked, or allocated when absent."""
    N, K = X.shape[0], U.shape[1]
    _chk_i32(labels, "labels", what, N)
    if out_loss is None:
        out_loss = torch.empty(K, device=X.device, dtype=torch.float32)
    elif _chk(out_loss, "out_loss").numel() != K:
        raise RuntimeError("%s: out_loss has %d entries, expected %d" % (what, out_loss.numel(), K))
    if out_grad is None:
        out_grad = torch.empty(tuple(U.shape), device=X.device, dtype=torch.float32)
    elif _chk(out_grad, "out_grad").numel() != U.numel():
        raise RuntimeError("%s: out_grad has %d entries, expected %d" % (what, out_grad.numel(), U.numel()))
    return out_loss, out_grad


def _ovr_proba_out(what, M, U, out):
    """The [M, K] float32 output of the three ovr_*_proba wrappers on U's device: checked, or allocated when absent."""
    K = U.shape[1]
    if out is None:
        out = torch.empty((M, K), device=U.device, dtype=torch.float32)
    elif _chk(out, "out").numel() != M * K:
        raise RuntimeError("%s: out has %d entries, expected %d" % (what, out.numel(), M * K))
    return out


def ovr_logreg_eval(X, labels, U, out_loss=None, out_grad=None, ws=None):
    """(loss [K], grad [D + 1, K]) of the K one-vs-rest logistic-regression objectives of include/cslgan.h "downstream classifier" at
    U [D + 1, K] (last row: the intercepts) on X [N, D] fp32 with int32 labels [N] — one evaluation of downstream.py:87's fit, all
    classes in one pass over X.  ws: a float32 device tensor of at least ovr_logreg_ws_floats(N, D) entries (an optimiser keeps one
    across its evaluations); allocated when absent.  csl_gan_amd.classify.objective_host is the host model."""
    _chk(X, "X"); _chk(U, "U")
    N, D, K = _logreg_shapes(X, U, "ovr_logreg_eval")
    out_loss, out_grad = _ovr_eval_outputs("ovr_logreg_eval", X, labels, U, out_loss, out_grad)
    if ws is None:
        ws = torch.empty(max(ovr_logreg_ws_floats(N, D), 2), device=X.device, dtype=torch.float32)
    else:
        _chk(ws, "ws")
    check(_lib.lib().cslgan_ovr_logreg_eval_f32(_p(X), _p(labels), _p(U), N, D, K, _p(out_loss), _p(out_grad), _p(ws), ws.numel(), _stream()),
          "ovr_logreg_eval")
    return out_loss, out_grad


def ovr_logreg_ws_floats(N, D):
    """Workspace of ovr_logreg_eval in floats (0: a shape the kernel does not take)."""
    return int(_lib.lib().cslgan_ovr_logreg_ws_floats(int(N), int(D)))


def ovr_logreg_proba(Xtest, U, out=None):
    """P [M, K] = sigmoid(z) / sum_k sigmoid(z), z = Xtest U[:D] + U[D] (downstream.py:87 predict_proba).  Xtest [M, D]: float32, or
    uint8 bytes that are scaled by 1 / 255 in the load (downstream.py:106)."""
    _chk(U, "U")
    if Xtest.dtype == torch.uint8:
        if not Xtest.is_cuda:
            raise RuntimeError("Xtest must be a device tensor (csl_gan_amd.ops has no CPU path)")
        if not Xtest.is_contiguous():
            raise RuntimeError("Xtest must be contiguous")
    else:
        _chk(Xtest, "Xtest")
    M, D, K = _logreg_shapes(Xtest, U, "ovr_logreg_proba")
    out = _ovr_proba_out("ovr_logreg_proba", M, U, out)
    check(_lib.lib().cslgan_ovr_logreg_proba_f32(_p(Xtest), 1 if Xtest.dtype == torch.uint8 else 0, _p(U), M, D, K, _p(out), _stream()),
          "ovr_logreg_proba")
    return out


def _chk_bytes(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must be a device tensor (csl_gan_amd.ops has no CPU path)" % name)
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous uint8 tensor" % name)
    return t


def ovr_logreg_eval_u8(X, labels, U, out_loss=None, out_grad=None, ws=None):
    """(loss [K], grad [D + 1, K]) of the objectives of ovr_logreg_eval on cache bytes: X [N, D] uint8 with x = byte / 255, any
    1 <= D <= 65536 (include/cslgan.h "The same estimator on cache BYTES"): two passes over X.  ws: a float32 device tensor of at least
    ovr_logreg_u8_ws_floats(N, D) entries; allocated when absent.  csl_gan_amd.classify.objective_host_bytes is the host model."""
    _chk_bytes(X, "X"); _chk(U, "U")
    N, D, K = _logreg_shapes(X, U, "ovr_logreg_eval_u8")
    out_loss, out_grad = _ovr_eval_outputs("ovr_logreg_eval_u8", X, labels, U, out_loss, out_grad)
    if ws is None:
        ws = torch.empty(max(ovr_logreg_u8_ws_floats(N, D), 2), device=X.device, dtype=torch.float32)
    else:
        _chk(ws, "ws")
    check(_lib.lib().cslgan_ovr_logreg_eval_u8(_p(X), _p(labels), _p(U), N, D, K, _p(out_loss), _p(out_grad), _p(ws), ws.numel(), _stream()),
          "ovr_logreg_eval_u8")
    return out_loss, out_grad


def ovr_logreg_u8_ws_floats(N, D):
    """Workspace of ovr_logreg_eval_u8 in floats (0: a shape the kernels do not take)."""
    return int(_lib.lib().cslgan_ovr_logreg_u8_ws_floats(int(N), int(D)))


def ovr_logreg_proba_u8(Xtest, U, out=None):
    """P [M, K] = sigmoid(z) / sum_k sigmoid(z), z = (Xtest / 255) U[:D] + U[D], for uint8 Xtest [M, D] with any 1 <= D <= 65536."""
    _chk(U, "U"); _chk_bytes(Xtest, "Xtest")
    M, D, K = _logreg_shapes(Xtest, U, "ovr_logreg_proba_u8")
    out = _ovr_proba_out("ovr_logreg_proba_u8", M, U, out)
    check(_lib.lib().cslgan_ovr_logreg_proba_u8(_p(Xtest), _p(U), M, D, K, _p(out), _stream()), "ovr_logreg_proba_u8")
    return out


def _mlp_shapes(X, U, hidden, what):
    H = int(hidden)
    if X.dim() != 2 or U.dim() != 2 or H < 1 or U.shape[0] != (X.shape[1] + 2) * H + 1:
        raise RuntimeError("%s: need X [N, D] and U [(D + 2) hidden + 1, K] with hidden >= 1, got %s, %s and hidden = %d" % (
            what, tuple(X.shape), tuple(U.shape), H))
    return X.shape[0], X.shape[1], U.shape[1], H


def ovr_mlp_u8_ws_floats(N, D, K, hidden):
    """Workspace of ovr_mlp_eval_u8 in floats (0: a shape the kernels do not take)."""
    return int(_lib.lib().cslgan_ovr_mlp_u8_ws_floats(int(N), int(D), int(K), int(hidden)))


def ovr_mlp_eval_u8(X, labels, U, hidden, alpha=1.0, out_loss=None, out_grad=None, ws=None):
    """(loss [K], grad like U) of the K one-vs-rest MLP objectives of include/cslgan.h "One-vs-rest MLP on cache bytes" at
    U [(D + 2) hidden + 1, K] on X [N, D] uint8 with x = byte / 255 and int32 labels [N].  ws: a float32 device tensor of exactly
    ovr_mlp_u8_ws_floats(N, D, K, hidden) entries (an optimiser keeps one across its evaluations); allocated when absent.
    csl_gan_amd.classify.objective_mlp_host_bytes is the host model."""
    _chk_bytes(X, "X"); _chk(U, "U")
    N, D, K, H = _mlp_shapes(X, U, hidden, "ovr_mlp_eval_u8")
    out_loss, out_grad = _ovr_eval_outputs("ovr_mlp_eval_u8", X, labels, U, out_loss, out_grad)
    need = ovr_mlp_u8_ws_floats(N, D, K, H)
    if need == 0:
        raise RuntimeError("ovr_mlp_eval_u8: N = %d, D = %d, K = %d, hidden = %d is outside 1 <= N < 2^31, 1 <= D <= 65536, 2 <= K <= 16, "
                           "1 <= hidden <= 128" % (N, D, K, H))
    if ws is None:
        ws = torch.empty(need, device=X.device, dtype=torch.float32)
    elif _chk(ws, "ws").numel() != need:                # the entry takes no size: the wrapper is where a wrong one can be told
        raise RuntimeError("ovr_mlp_eval_u8: workspace of %d floats, need %d" % (ws.numel(), need))
    check(_lib.lib().cslgan_ovr_mlp_eval_u8(_p(X), _p(labels), _p(U), N, D, K, H, float(alpha), _p(out_loss), _p(out_grad), _p(ws), _stream()),
          "ovr_mlp_eval_u8")
    return out_loss, out_grad


def ovr_mlp_proba_u8(Xtest, U, hidden, out=None):
    """P [M, K] = sigmoid(z) / sum_k sigmoid(z) of the K networks of ovr_mlp_eval_u8 on uint8 Xtest [M, D]."""
    _chk(U, "U"); _chk_bytes(Xtest, "Xtest")
    M, D, K, H = _mlp_shapes(Xtest, U, hidden, "ovr_mlp_proba_u8")
    out = _ovr_proba_out("ovr_mlp_proba_u8", M, U, out)
    check(_lib.lib().cslgan_ovr_mlp_proba_u8(_p(Xtest), _p(U), M, D, K, H, _p(out), _stream()), "ovr_mlp_proba_u8")
    return out


def class_moments_u8(X, labels, n_classes, binarize=0, out=None):
    """{"n": [K], "s1": [K, D], "s2": [K, D], "cnt": [K, D]}, int64 device tensors: per class the row count, sum b, sum b^2 and the
    number of rows with b > binarize of X [N, D] uint8 with int32 labels [N] (include/cslgan.h "naive Bayes"): one pass over X, exact,
    the same integers in every schedule.  out: such a dict to write into (whatever it holds is overwritten); allocated when absent.
    csl_gan_amd.classify.class_moments_host_bytes is the host model."""
    N, D = _byte_rows(X, "class_moments_u8")
    K = int(n_classes)
    _chk_i32(labels, "labels", "class_moments_u8", N)
    shapes = {"n": (K,), "s1": (K, D), "s2": (K, D), "cnt": (K, D)}
    if out is None:
        out = {k: torch.empty(s, device=X.device, dtype=torch.int64) for k, s in shapes.items()}
    for k, s in shapes.items():
        t = out[k]
        if not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or tuple(t.shape) != s:
            raise RuntimeError("class_moments_u8: out[%r] must be a contiguous int64 device tensor of shape %s" % (k, s))
    check(_lib.lib().cslgan_class_moments_u8(_p(X), _p(labels), N, D, K, int(binarize), _p(out["n"]), _p(out["s1"]), _p(out["s2"]), _p(out["cnt"]),
                                             None, _stream()), "class_moments_u8")
    return out


def _nb_tables(what, Xtest, tables):
    _chk_bytes(Xtest, "Xtest")
    for t in tables:
        _chk(t, "table")
    if Xtest.dim() != 2 or any(t.dim() != 2 or t.shape[1] != Xtest.shape[1] or t.shape != tables[0].shape for t in tables):
        raise RuntimeError("%s: need Xtest [M, D] and tables [K, D], got %s and %s" % (what, tuple(Xtest.shape), [tuple(t.shape) for t in tables]))
    return Xtest.shape[0], Xtest.shape[1], tables[0].shape[0]


def _nb_out(what, M, K, device, out):
    if out is None:
        out = torch.empty((M, K), device=device, dtype=torch.float32)
    elif _chk(out, "out").numel() != M * K:
        raise RuntimeError("%s: out has %d entries, expected %d" % (what, out.numel(), M * K))
    return out


def nb_score_gauss_u8(Xtest, m, w, out=None):
    """S [M, K] fp32, S[i][k] = sum_j w[k][j] (byte_ij - m[k][j])^2 for uint8 Xtest [M, D] and fp32 tables m, w [K, D]: the sum of a
    Gaussian naive-Bayes log-likelihood in byte units (include/cslgan.h "naive Bayes"); fixed order, the same bits on every call."""
    M, D, K = _nb_tables("nb_score_gauss_u8", Xtest, (m, w))
    out = _nb_out("nb_score_gauss_u8", M, K, Xtest.device, out)
    check(_lib.lib().cslgan_nb_score_gauss_u8(_p(Xtest), _p(m), _p(w), M, D, K, _p(out), _stream()), "nb_score_gauss_u8")
    return out


def nb_score_bern_u8(Xtest, delta, binarize=0, out=None):
    """S [M, K] fp32, S[i][k] = sum_j [byte_ij > binarize] delta[k][j] for uint8 Xtest [M, D] and the fp32 table delta [K, D]."""
    M, D, K = _nb_tables("nb_score_bern_u8", Xtest, (delta,))
    out = _nb_out("nb_score_bern_u8", M, K, Xtest.device, out)
    check(_lib.lib().cslgan_nb_score_bern_u8(_p(Xtest), _p(delta), M, D, K, int(binarize), _p(out), _stream()), "nb_score_bern_u8")
    return out


def _chk_i32(t, name, what, numel=None):
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise RuntimeError("%s: %s must be a contiguous int32 device tensor%s" % (what, name, "" if numel is None else " of %d entries" % numel))
    return t


def _byte_rows(X, what, name="X", rows="N"):
    """(rows, D) of X [rows, D], contiguous device bytes."""
    _chk_bytes(X, name)
    if X.dim() != 2:
        raise RuntimeError("%s: need %s [%s, D], got %s" % (what, name, rows, tuple(X.shape)))
    return X.shape


def _split_outputs(what, X, S, dtype, out, need, refusal, ws):
    """What the two split searches share once X [N, D] is checked: the pair (out [S, 7] of dtype, score int64 [S]) and the byte
    workspace of at least `need` (0: a shape the entry does not take, refused with `refusal`), each checked, or allocated when absent."""
    if need == 0:
        raise RuntimeError("%s: %s" % (what, refusal))
    if out is None:
        out = (torch.empty((S, 7), device=X.device, dtype=dtype), torch.empty(S, device=X.device, dtype=torch.int64))
    for t, name, dt, numel in ((out[0], "out[0]", dtype, 7 * S), (out[1], "out[1]", torch.int64, S)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.numel() != numel:
            raise RuntimeError("%s: %s must be a contiguous %s device tensor of %d entries" % (what, name, str(dt).replace("torch.", ""), numel))
    if ws is None:
        ws = torch.empty(need, device=X.device, dtype=torch.uint8)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise RuntimeError("%s: ws must be a contiguous uint8 device tensor of at least %d bytes" % (what, need))
    return out, ws


def tree_best_split_ws_bytes(S, D):
    """Workspace of tree_best_split_u8 in bytes (0: a shape one launch does not take; split the segments over several calls)."""
    return int(_lib.lib().cslgan_tree_best_split_ws_bytes(int(S), int(D)))


def tree_best_split_u8(X, labels, n_classes, rows, seg_off, seg_class, seg_wrow=None, weights=None, seg_key=None, mask_thr=0, seed=0, out=None, ws=None):
    """(out int32 [S, 7] = (j, v, v_hi, nL, pL, n, p), score int64 [S]: the bits of the float64 score) of the best split of S segments of
    rows of X [N, D] uint8 (include/cslgan.h "decision trees"): rows int32 [R] row indices, seg_off int32 [S + 1], seg_class int32 [S];
    weights int32 [B, N] with seg_wrow int32 [S] (-1: weight 1) or neither; seg_key = (seg_tree, seg_node), int32 [S] each, with
    mask_thr in 1 .. 2^32 - 1 for the keyed feature mask (0: every feature).  out: such a pair to write into; ws: a uint8 device tensor
    of at least tree_best_split_ws_bytes(S, D) bytes; both allocated when absent.  Exact: csl_gan_amd.classify.best_split_host_bytes
    is the host model, equalled in every integer and in the score's bits."""
    what = "tree_best_split_u8"
    N, D = _byte_rows(X, what)
    K = int(n_classes)
    _chk_i32(labels, "labels", what, N)
    _chk_i32(rows, "rows", what)
    S = _chk_i32(seg_class, "seg_class", what).numel()
    _chk_i32(seg_off, "seg_off", what, S + 1)
    if (weights is None) != (seg_wrow is None):
        raise RuntimeError("%s: weights and seg_wrow go together" % what)
    B = 0
    if weights is not None:
        if weights.dim() != 2 or weights.shape[1] != N:
            raise RuntimeError("%s: need weights [B, %d], got %s" % (what, N, tuple(weights.shape)))
        B = _chk_i32(weights, "weights", what).shape[0]
        _chk_i32(seg_wrow, "seg_wrow", what, S)
    mask_thr, seed = int(mask_thr), int(seed)
    if not 0 <= mask_thr < 2 ** 32 or not 0 <= seed < 2 ** 64:
        raise RuntimeError("%s: need 0 <= mask_thr < 2^32 and 0 <= seed < 2^64, got %d and %d" % (what, mask_thr, seed))
    if mask_thr and seg_key is None:
        raise RuntimeError("%s: a feature mask needs seg_key = (seg_tree, seg_node)" % what)
    tree, node = (None, None) if seg_key is None else (_chk_i32(seg_key[0], "seg_tree", what, S), _chk_i32(seg_key[1], "seg_node", what, S))
    out, ws = _split_outputs(what, X, S, torch.int32, out, tree_best_split_ws_bytes(S, D),
                             "S = %d segments of D = %d features is outside 1 <= S, 1 <= D <= 65536, S ceil(D / 16) < 2^31" % (S, D), ws)
    check(_lib.lib().cslgan_tree_best_split_u8(_p(X), _p(labels), _p(weights), B, N, D, K, _p(rows), rows.numel(), _p(seg_off), _p(seg_class), _p(seg_wrow),
                                               _p(tree), _p(node), S, mask_thr, seed, _p(out[0]), _p(out[1]), _p(ws), ws.numel(), _stream()), what)
    return out


def tree_apply_u8(Xtest, feature, threshold, child, tree_off, out=None):
    """leaf int32 [T, M]: the tree-local leaf number of every row of uint8 Xtest [M, D] under T trees given as flat int32 node tables
    feature, threshold, child [Q] and tree_off [T + 1] (include/cslgan.h "decision trees"); -1 where a table is malformed.
    csl_gan_amd.classify.tree_apply_host_bytes is the host model."""
    what = "tree_apply_u8"
    M, D = _byte_rows(Xtest, what, "Xtest", "M")
    Q = _chk_i32(feature, "feature", what).numel()
    _chk_i32(threshold, "threshold", what, Q)
    _chk_i32(child, "child", what, Q)
    T = _chk_i32(tree_off, "tree_off", what).numel() - 1
    if out is None:
        out = torch.empty((max(T, 0), M), device=Xtest.device, dtype=torch.int32)
    _chk_i32(out, "out", what, max(T, 0) * M)
    check(_lib.lib().cslgan_tree_apply_u8(_p(Xtest), M, D, _p(feature), _p(threshold), _p(child), _p(tree_off), T, Q, _p(out), _stream()), what)
    return out


def boost_stump_ws_bytes(n_classes, D):
    """Workspace of boost_stump_u8 in bytes (0: n_classes outside 2 .. 16 or D outside 1 .. 65536)."""
    return int(_lib.lib().cslgan_boost_stump_ws_bytes(int(n_classes), int(D)))


def boost_stump_u8(X, labels, n_classes, weights, out=None, ws=None):
    """(out int64 [K, 7] = (j, v, v_hi, nL, pL, n, p), score int64 [K]: the bits of the float64 score) of the best stump of each of the K
    one-vs-rest classes on all rows of X [N, D] uint8 under the fixed-point weights int32 [K, N], 0 .. 2^28 (include/cslgan.h "boosted
    stumps"; a weight outside the range is clamped).  out: such a pair to write into; ws: a uint8 device tensor of at least
    boost_stump_ws_bytes(K, D) bytes; both allocated when absent.  Exact: csl_gan_amd.classify.boost_stump_host_bytes is the host
    model, equalled in every integer and in the score's bits."""
    what = "boost_stump_u8"
    N, D = _byte_rows(X, what)
    K = int(n_classes)
    _chk_i32(labels, "labels", what, N)
    if weights.dim() != 2 or tuple(weights.shape) != (K, N):
        raise RuntimeError("%s: need weights [%d, %d], got %s" % (what, K, N, tuple(weights.shape)))
    _chk_i32(weights, "weights", what)
    out, ws = _split_outputs(what, X, K, torch.int64, out, boost_stump_ws_bytes(K, D),
                             "K = %d classes of D = %d features is outside 2 <= K <= 16, 1 <= D <= 65536" % (K, D), ws)
    check(_lib.lib().cslgan_boost_stump_u8(_p(X), _p(labels), _p(weights), N, D, K, _p(out[0]), _p(out[1]), _p(ws), ws.numel(), _stream()), what)
    return out


def nn_padded_dim(D):
    """Row pitch of the prepared operands of nn_min: D rounded up to the kernel's K tile (0: a D outside 1 .. 65536)."""
    return int(_lib.lib().cslgan_nn_padded_dim(int(D)))


def _chk_dev(t, name, dtype, what):
    if not t.is_cuda:
        raise RuntimeError("%s must be a device tensor (csl_gan_amd.ops has no CPU path)" % name)
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError("%s: %s must be a contiguous %s tensor" % (what, name, str(dtype).replace("torch.", "")))
    return t


def nn_prepare(u8, out=None, out_sqnorm=None):
    """(int8 [rows, Dp], int32 [rows]) of a uint8 device tensor [rows, ...]: the bytes minus 128 with zero padding up to
    Dp = nn_padded_dim(D), and the squared norm of every shifted row (include/cslgan.h "Nearest-neighbour audit")."""
    _chk_dev(u8, "u8", torch.uint8, "nn_prepare")
    rows = u8.shape[0]
    D = u8.numel() // max(rows, 1)
    Dp = nn_padded_dim(D)
    if rows < 1 or Dp == 0:
        raise RuntimeError("nn_prepare: need at least one row of 1 .. 65536 bytes, got %s" % (tuple(u8.shape),))
    if out is None:
        out = torch.empty((rows, Dp), device=u8.device, dtype=torch.int8)
    elif _chk_dev(out, "out", torch.int8, "nn_prepare").numel() != rows * Dp:
        raise RuntimeError("nn_prepare: out has %d entries, expected %d" % (out.numel(), rows * Dp))
    if out_sqnorm is None:
        out_sqnorm = torch.empty(rows, device=u8.device, dtype=torch.int32)
    elif _chk_dev(out_sqnorm, "out_sqnorm", torch.int32, "nn_prepare").numel() != rows:
        raise RuntimeError("nn_prepare: out_sqnorm has %d entries, expected %d" % (out_sqnorm.numel(), rows))
    check(_lib.lib().cslgan_nn_prepare_u8(_p(u8), rows, D, Dp, _p(out), _p(out_sqnorm), _stream()), "nn_prepare")
    return out, out_sqnorm


def _nn_operands(what, q, qn, r, rn, extra):
    """(nq, nr, Dp) of the prepared operands q [nq, Dp] / r [nr, Dp] (int8) with their norms qn / rn (int32), the check that the
    four nn_* wrappers share; `extra`: the entry's further tensors as (tensor, name, dtype).  The types first — a wrong one is
    refused wherever the tensor lives — then device and contiguity, then the shapes of the operands; the shapes of `extra` are the
    caller's."""
    args = ((q, "q", torch.int8), (r, "r", torch.int8), (qn, "qn", torch.int32), (rn, "rn", torch.int32)) + tuple(extra)
    for t, name, dt in args:
        if t.dtype != dt:
            raise RuntimeError("%s: %s must be a contiguous %s tensor" % (what, name, str(dt).replace("torch.", "")))
    for t, name, dt in args:
        _chk_dev(t, name, dt, what)
    if q.dim() != 2 or r.dim() != 2 or q.shape[1] != r.shape[1]:
        raise RuntimeError("%s: need q [nq, Dp] and r [nr, Dp], got %s and %s" % (what, tuple(q.shape), tuple(r.shape)))
    return q.shape[0], r.shape[0], q.shape[1]


def nn_min(q, qn, r, rn, index_base, best):
    """best[i] = min(best[i], min_j (d2(q_i, r_j) << 32 | index_base + j)) as uint64, in place.  q [nq, Dp] / r [nr, Dp]: prepared
    int8 operands of nn_prepare with their int32 squared norms qn / rn; best: int64 device tensor [nq] that the caller filled with
    -1 (all ones) once.  Ties go to the smallest index.  csl_gan_amd.neighbours.nearest_host is the host model."""
    nq, nr, Dp = _nn_operands("nn_min", q, qn, r, rn, [(best, "best", torch.int64)])
    if qn.numel() != nq or rn.numel() != nr or best.numel() != nq:
        raise RuntimeError("nn_min: qn / rn / best have %d / %d / %d entries, expected %d / %d / %d" % (qn.numel(), rn.numel(), best.numel(), nq, nr, nq))
    check(_lib.lib().cslgan_nn_min_i8(_p(q), _p(qn), nq, _p(r), _p(rn), nr, Dp, int(index_base), _p(best), _stream()), "nn_min")
    return best


def nn_count(q, qn, r, rn, thresholds, counts):
    """counts[i, j] += #{k : d2(q_i, r_k) <= thresholds[j]}, in place.  q / qn / r / rn as for nn_min; thresholds: 1 .. 4 Python
    integers in [0, 2^32 - 1], any order; counts: int32 device tensor [nq, J] that the caller zeroed once.  The device adds as
    uint32 and torch reads int32: the TOTAL count of an entry over all calls must stay below 2^31 on this path.
    csl_gan_amd.neighbours.count_within_host is the host model."""
    nq, nr, Dp = _nn_operands("nn_count", q, qn, r, rn, [(counts, "counts", torch.int32)])
    thr = [int(t) for t in thresholds]
    if not 1 <= len(thr) <= 4 or any(t < 0 or t > 0xFFFFFFFF for t in thr):
        raise RuntimeError("nn_count: need 1 .. 4 thresholds in [0, 2^32 - 1], got %s" % (thr,))
    J = len(thr)
    if qn.numel() != nq or rn.numel() != nr or tuple(counts.shape) != (nq, J):
        raise RuntimeError("nn_count: qn / rn have %d / %d entries and counts the shape %s, expected %d / %d and (%d, %d)"
                           % (qn.numel(), rn.numel(), tuple(counts.shape), nq, nr, nq, J))
    check(_lib.lib().cslgan_nn_count_i8(_p(q), _p(qn), nq, _p(r), _p(rn), nr, Dp, (C.c_uint32 * J)(*thr), J, _p(counts), _stream()), "nn_count")
    return counts


_NN_KTH_WS = {}                                         # device -> the cached workspace of nn_kth (int64, grown on demand)


def nn_kth_workspace_bytes(nq, nr, k):
    """Workspace of nn_kth in bytes (0: sizes or a k that the search refuses)."""
    return int(_lib.lib().cslgan_nn_kth_workspace_bytes(int(nq), int(nr), int(k)))


def nn_kth(q, qn, r, rn, index_base, best, self_base=-1):
    """best[i, :] = the k smallest of best[i, :] and the keys d2(q_i, r_j) << 32 | index_base + j, ascending as uint64, in place; k is
    best.shape[1], 1 .. 8.  With self_base >= 0 row i skips the one column whose index index_base + j equals self_base + i.  q / qn /
    r / rn as for nn_min; best: int64 device tensor [nq, k] that the caller filled with -1 (all ones) once; successive calls must
    bring disjoint index ranges.  The workspace is ONE device tensor cached per device, whatever the stream: calls on different streams
    of one device would race on it, so keep nn_kth on one stream per device (NearestSearch does).  csl_gan_amd.neighbours.kth_host is the host
    model."""
    nq, nr, Dp = _nn_operands("nn_kth", q, qn, r, rn, [(best, "best", torch.int64)])
    if best.dim() != 2 or best.shape[0] != nq or not 1 <= best.shape[1] <= 8:
        raise RuntimeError("nn_kth: best has the shape %s, expected (%d, k) with k in 1 .. 8" % (tuple(best.shape), nq))
    k = best.shape[1]
    if qn.numel() != nq or rn.numel() != nr:
        raise RuntimeError("nn_kth: qn / rn have %d / %d entries, expected %d / %d" % (qn.numel(), rn.numel(), nq, nr))
    need = nn_kth_workspace_bytes(nq, nr, k)
    if need <= 0:
        raise RuntimeError("nn_kth: %d x %d rows with k = %d are out of range" % (nq, nr, k))
    ws = _NN_KTH_WS.get(q.device)
    if ws is None or ws.numel() * 8 < need:
        ws = _NN_KTH_WS[q.device] = torch.empty((need + 7) // 8, device=q.device, dtype=torch.int64)
    check(_lib.lib().cslgan_nn_kth_i8(_p(q), _p(qn), nq, _p(r), _p(rn), nr, Dp, int(index_base), int(self_base), k, _p(best), _p(ws),
                                      ws.numel() * 8, _stream()), "nn_kth")
    return best


def nn_count_radius(q, qn, r, rn, radius, counts):
    """counts[i] += #{j : d2(q_i, r_j) <= radius[j]}, in place, compared as unsigned values.  q / qn / r / rn as for nn_min; radius:
    int32 device tensor [nr] holding the uint32 bits; counts: int32 device tensor [nq] that the caller zeroed once (the device adds
    uint32: the total of an entry must stay below 2^31 on this path).  csl_gan_amd.neighbours.count_within_radii_host is the host
    model."""
    nq, nr, Dp = _nn_operands("nn_count_radius", q, qn, r, rn, [(radius, "radius", torch.int32), (counts, "counts", torch.int32)])
    if qn.numel() != nq or rn.numel() != nr or tuple(radius.shape) != (nr,) or tuple(counts.shape) != (nq,):
        raise RuntimeError("nn_count_radius: qn / rn have %d / %d entries, radius and counts the shapes %s and %s; expected %d / %d, (%d,) and (%d,)"
                           % (qn.numel(), rn.numel(), tuple(radius.shape), tuple(counts.shape), nq, nr, nr, nq))
    check(_lib.lib().cslgan_nn_count_radius_i8(_p(q), _p(qn), nq, _p(r), _p(rn), nr, Dp, _p(radius), _p(counts), _stream()), "nn_count_radius")
    return counts


SVM_MAX_ROWS = 65536            # include/cslgan.h "linear SVC": the stored matrix of more rows is refused


def gram_pitch(n):
    """Row pitch of the matrix of gram_d2 in entries: n rounded up to 32, so that every row is whole 128-byte lines."""
    return (int(n) + 31) // 32 * 32


def gram_d2(xs, sq, out=None):
    """d2 [n, gram_pitch(n)] as int32 holding the uint32 bits: the exact squared distance of every pair of the rows that nn_prepare turned
    into xs [n, Dp] / sq [n] (include/cslgan.h "linear SVC").  The columns n .. pitch - 1 mean nothing.  n <= 65536.
    csl_gan_amd.svm.gram_d2_host is the host model."""
    n, _, Dp = _nn_operands("gram_d2", xs, sq, xs, sq, [])
    if n > SVM_MAX_ROWS:
        raise RuntimeError("gram_d2: %d rows; the stored matrix takes at most %d (16 GiB)" % (n, SVM_MAX_ROWS))
    pitch = gram_pitch(n)
    if out is None:
        out = torch.empty((n, pitch), device=xs.device, dtype=torch.int32)
    elif _chk_dev(out, "out", torch.int32, "gram_d2").shape != (n, pitch):
        raise RuntimeError("gram_d2: out has the shape %s, expected %s" % (tuple(out.shape), (n, pitch)))
    check(_lib.lib().cslgan_gram_d2_u8(_p(xs), _p(sq), n, Dp, _p(out), pitch, _stream()), "gram_d2")
    return out


def svc_smo(d2, s, y, active, C, tol, chunk, max_iter, alpha, grad, iters, done):
    """At most `chunk` more SMO iterations on each of the P dual problems over the rows of d2 (gram_d2's matrix; s: int64 [n], the byte
    rows' squared norms), in place on the state alpha / grad (float64 [P, n], started at 0 / -1), iters (int64 [P]) and done (int32 [P]),
    both started at 0; y: int8 [P, n] of +1 / -1, active: uint8 [P, n].  The caller repeats the call until every problem is done or has
    run max_iter iterations.  Equal to csl_gan_amd.svm.smo_host bit for bit."""
    what = "svc_smo"
    for t, name, dt in ((d2, "d2", torch.int32), (s, "s", torch.int64), (y, "y", torch.int8), (active, "active", torch.uint8),
                        (alpha, "alpha", torch.float64), (grad, "grad", torch.float64), (iters, "iters", torch.int64), (done, "done", torch.int32)):
        _chk_dev(t, name, dt, what)
    if d2.dim() != 2 or y.dim() != 2:
        raise RuntimeError("%s: need d2 [n, pitch] and y [P, n], got %s and %s" % (what, tuple(d2.shape), tuple(y.shape)))
    n, pitch = d2.shape
    P = y.shape[0]
    shapes = [tuple(t.shape) for t in (s, y, active, alpha, grad, iters, done)]
    if shapes != [(n,), (P, n), (P, n), (P, n), (P, n), (P,), (P,)] or pitch != gram_pitch(n):
        raise RuntimeError("%s: d2 %s with s, y, active, alpha, grad, iters, done of the shapes %s" % (what, tuple(d2.shape), shapes))
    check(_lib.lib().cslgan_svc_smo_f64(_p(d2), pitch, _p(s), n, _p(y), _p(active), P, float(C), float(tol), int(chunk), int(max_iter),
                                         _p(alpha), _p(grad), _p(iters), _p(done), _stream()), what)


def swd_directions(P, D, seed, device, out=None):
    """int8 [P, nn_padded_dim(D)] on `device`: the P Rademacher directions of the stream of `seed` (include/cslgan.h "Sliced Wasserstein
    audit"), +1 / -1 in the columns < D and zero behind them — the shape of nn_prepare's operands.  csl_gan_amd.sliced.directions_host is
    the host model."""
    P, D, Dp = int(P), int(D), nn_padded_dim(D)
    if P < 1 or Dp == 0:
        raise RuntimeError("swd_directions: need at least one direction of 1 .. 65536 columns, got P = %d, D = %d" % (P, D))
    if out is None:
        out = torch.empty((P, Dp), device=device, dtype=torch.int8)
    elif tuple(_chk_dev(out, "out", torch.int8, "swd_directions").shape) != (P, Dp):
        raise RuntimeError("swd_directions: out has the shape %s, expected %s" % (tuple(out.shape), (P, Dp)))
    with torch.cuda.device(out.device):
        check(_lib.lib().cslgan_swd_directions_i8(int(seed) & 0xFFFFFFFFFFFFFFFF, P, D, Dp, _p(out), _stream()), "swd_directions")
    return out


def swd_project(dirs, xs, Y, col0=0):
    """Y[p, col0 + i] = dirs[p] . xs[i], in place: dirs int8 [P, Dp] of swd_directions, xs int8 [n, Dp] of nn_prepare, Y int32
    [P, ld] with ld >= col0 + n.  Nothing else of Y is written.  csl_gan_amd.sliced.project_host is the host model."""
    what = "swd_project"
    args = ((dirs, "dirs", torch.int8), (xs, "xs", torch.int8), (Y, "Y", torch.int32))
    for t, name, dt in args:                            # the types first, wherever the tensor lives (as _nn_operands)
        if t.dtype != dt:
            raise RuntimeError("%s: %s must be a contiguous %s tensor" % (what, name, str(dt).replace("torch.", "")))
    for t, name, dt in args:
        _chk_dev(t, name, dt, what)
    if dirs.dim() != 2 or xs.dim() != 2 or Y.dim() != 2 or dirs.shape[1] != xs.shape[1] or Y.shape[0] != dirs.shape[0]:
        raise RuntimeError("%s: need dirs [P, Dp], xs [n, Dp] and Y [P, ld], got %s, %s and %s" % (what, tuple(dirs.shape), tuple(xs.shape), tuple(Y.shape)))
    P, Dp = dirs.shape
    n, ld, col0 = xs.shape[0], Y.shape[1], int(col0)
    if col0 < 0 or ld < col0 + n:
        raise RuntimeError("%s: Y has %d columns, col0 + n = %d + %d" % (what, ld, col0, n))
    check(_lib.lib().cslgan_swd_project_i8(_p(dirs), P, _p(xs), n, Dp, _p(Y), ld, col0, _stream()), what)
    return Y


def sort_rows_ws_bytes(P, n):
    """Workspace of sort_rows in bytes (0: sizes that the sort refuses)."""
    return int(_lib.lib().cslgan_sort_rows_ws_bytes(int(P), int(n)))


def sort_rows(x, n=None, key_bits=32, ws=None):
    """The first n (default: all) entries of every row of x, int32 [P, ld] on the device, sorted ascending as signed values, in place;
    the entries behind n stay.  key_bits < 32 promises values in [-2^(key_bits - 1), 2^(key_bits - 1)) and saves passes.  ws: a uint8
    device tensor of at least sort_rows_ws_bytes(P, n) bytes, allocated when absent.  Equal to np.sort(axis=1)."""
    what = "sort_rows"
    if x.dtype != torch.int32:
        raise RuntimeError("%s: x must be a contiguous int32 tensor" % what)
    _chk_dev(x, "x", torch.int32, what)
    if x.dim() != 2:
        raise RuntimeError("%s: need x [P, ld], got %s" % (what, tuple(x.shape)))
    P, ld = x.shape
    n, key_bits = ld if n is None else int(n), int(key_bits)
    if not 1 <= n <= ld or not 1 <= key_bits <= 32:
        raise RuntimeError("%s: n = %d of %d columns, key_bits = %d; need 1 <= n <= ld and 1 <= key_bits <= 32" % (what, n, ld, key_bits))
    need = sort_rows_ws_bytes(P, n)
    if need <= 0:
        raise RuntimeError("%s: %d rows of %d entries are out of range" % (what, P, n))
    if ws is None:
        ws = torch.empty(need, device=x.device, dtype=torch.uint8)
    elif _chk_dev(ws, "ws", torch.uint8, what).numel() < need:
        raise RuntimeError("%s: ws has %d bytes, need %d" % (what, ws.numel(), need))
    check(_lib.lib().cslgan_sort_rows_i32(_p(x), P, n, ld, key_bits, _p(ws), ws.numel(), _stream()), what)
    return x


SWD_MAX_CELLS = 2 ** 38         # include/cslgan.h "Sliced Wasserstein audit": Na Nb 2^25 must stay below 2^63


def swd_w1(a, na, b, nb, out=None):
    """int64 [P]: the W1 numerators of the sorted rows a [P, lda] (their first na entries) and b [P, ldb] (first nb), int32 device tensors
    (include/cslgan.h "Sliced Wasserstein audit").  csl_gan_amd.sliced.w1_numerators_host is the host model."""
    what = "swd_w1"
    for t, name in ((a, "a"), (b, "b")):
        if t.dtype != torch.int32:
            raise RuntimeError("%s: %s must be a contiguous int32 tensor" % (what, name))
    for t, name in ((a, "a"), (b, "b")):
        _chk_dev(t, name, torch.int32, what)
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise RuntimeError("%s: need a [P, lda] and b [P, ldb], got %s and %s" % (what, tuple(a.shape), tuple(b.shape)))
    P, na, nb = a.shape[0], int(na), int(nb)
    if not 1 <= na <= a.shape[1] or not 1 <= nb <= b.shape[1]:
        raise RuntimeError("%s: na = %d of %d columns, nb = %d of %d" % (what, na, a.shape[1], nb, b.shape[1]))
    if na * nb >= SWD_MAX_CELLS:
        raise RuntimeError("%s: Na * Nb * 2^25 = %d * %d * 2^25 >= 2^63 overflows the int64 numerator" % (what, na, nb))
    if out is None:
        out = torch.empty(P, device=a.device, dtype=torch.int64)
    elif tuple(_chk_dev(out, "out", torch.int64, what).shape) != (P,):
        raise RuntimeError("%s: out has the shape %s, expected (%d,)" % (what, tuple(out.shape), P))
    check(_lib.lib().cslgan_swd_w1_i64(_p(a), a.shape[1], na, _p(b), b.shape[1], nb, P, _p(out), _stream()), what)
    return out


MOM_MAX_ROWS = 65536            # include/cslgan.h "Byte moments": rows of one chunk, the reduction length of the Gram product


def mom_padded_rows(n):
    """Row pitch of the transposed image of mom_transpose: n rounded up to the K tile of the Gram product."""
    return (int(n) + 63) // 64 * 64


def _mom_operands(what, args):
    """The check that the mom_* wrappers share, as swd_project: the types first, wherever a tensor lives, then device and contiguity."""
    for t, name, dt in args:
        if t.dtype != dt:
            raise RuntimeError("%s: %s must be a contiguous %s tensor" % (what, name, str(dt).replace("torch.", "")))
    for t, name, dt in args:
        _chk_dev(t, name, dt, what)


def mom_transpose(u8, out=None):
    """int8 [D, mom_padded_rows(n)]: the transposed image of a uint8 device tensor [n, ...] of D bytes per row, out[j, i] = u8[i, j] - 128
    and zero in the columns n .. (include/cslgan.h "Byte moments").  n <= 65536."""
    what = "mom_transpose"
    _mom_operands(what, [(u8, "u8", torch.uint8)])
    n = u8.shape[0] if u8.dim() else 0
    D = u8.numel() // max(n, 1)
    if not 1 <= n <= MOM_MAX_ROWS or not 1 <= D <= 65536:
        raise RuntimeError("%s: need 1 .. %d rows of 1 .. 65536 bytes, got %s" % (what, MOM_MAX_ROWS, tuple(u8.shape)))
    np_ = mom_padded_rows(n)
    if out is None:
        out = torch.empty((D, np_), device=u8.device, dtype=torch.int8)
    else:
        _mom_operands(what, [(out, "out", torch.int8)])
        if tuple(out.shape) != (D, np_):
            raise RuntimeError("%s: out has the shape %s, expected %s" % (what, tuple(out.shape), (D, np_)))
    check(_lib.lib().cslgan_mom_transpose_u8(_p(u8), n, D, np_, _p(out), _stream()), what)
    return out


def mom_colsum(xt, s1):
    """s1[j] += sum_i xt[j, i], in place: xt int8 [D, np] of mom_transpose, s1 int64 [D] that the caller zeroed once."""
    what = "mom_colsum"
    _mom_operands(what, [(xt, "xt", torch.int8), (s1, "s1", torch.int64)])
    if xt.dim() != 2 or tuple(s1.shape) != (xt.shape[0],):
        raise RuntimeError("%s: need xt [D, np] and s1 [D], got %s and %s" % (what, tuple(xt.shape), tuple(s1.shape)))
    check(_lib.lib().cslgan_mom_colsum_i64(_p(xt), xt.shape[0], xt.shape[1], _p(s1), _stream()), what)
    return s1


def mom_gram(xt, S2):
    """S2[i, j] += xt[i] . xt[j] on the 128 x 128 tiles on and below the diagonal, in place: xt int8 [D, np] of mom_transpose, S2 int64
    [D, ld] with ld >= D that the caller zeroed once.  The tiles strictly above the diagonal and the columns D .. are not touched:
    mom_mirror fills the tiles once, after the last chunk.  csl_gan_amd.moments.byte_moments_host is the host model."""
    what = "mom_gram"
    _mom_operands(what, [(xt, "xt", torch.int8), (S2, "S2", torch.int64)])
    if xt.dim() != 2 or S2.dim() != 2 or S2.shape[0] != xt.shape[0] or S2.shape[1] < xt.shape[0]:
        raise RuntimeError("%s: need xt [D, np] and S2 [D, ld >= D], got %s and %s" % (what, tuple(xt.shape), tuple(S2.shape)))
    check(_lib.lib().cslgan_mom_gram_i64(_p(xt), xt.shape[0], xt.shape[1], _p(S2), S2.shape[1], _stream()), what)
    return S2


def mom_mirror(S2):
    """S2[i, j] = S2[j, i] on the 128 x 128 tiles strictly above the diagonal, in place: S2 int64 [D, ld >= D] of mom_gram."""
    what = "mom_mirror"
    _mom_operands(what, [(S2, "S2", torch.int64)])
    if S2.dim() != 2 or S2.shape[1] < S2.shape[0]:
        raise RuntimeError("%s: need S2 [D, ld >= D], got %s" % (what, tuple(S2.shape)))
    check(_lib.lib().cslgan_mom_mirror_i64(_p(S2), S2.shape[0], S2.shape[1], _stream()), what)
    return S2


MMD_MAX_B = 7                   # include/cslgan.h "Kernel two-sample test": 7 * 2^28 < 2^31
MMD_TABLE = 65536               # entries of one exp table


def mmd_padded_cols(n):
    """Row pitch of the partition matrix of mmd_partition_sums: n rounded up to the K stage of 64 columns."""
    return (int(n) + 63) // 64 * 64


def _mmd_matrix(what, d2, extra=()):
    """The rows n of the stored matrix d2 int32 [n, gram_pitch(n)] of gram_d2, checked together with the entry's further tensors `extra`
    as (tensor, name, dtype): types first, as _mom_operands."""
    _mom_operands(what, [(d2, "d2", torch.int32)] + list(extra))
    if d2.dim() != 2 or d2.shape[1] != gram_pitch(d2.shape[0]):
        raise RuntimeError("%s: need the matrix of gram_d2, [n, gram_pitch(n)], got %s" % (what, tuple(d2.shape)))
    return d2.shape[0]


def tri_hist(d2, prefix=0, prefix_bits=0, hist=None):
    """hist[v] += #{i < j < n : the top prefix_bits (0, 8, 16, 24) bits of d2[i, j] equal those of `prefix` and the next 8 bits are v},
    in place: d2 the matrix of gram_d2 (int32 holding the uint32 bits), hist int64 [256] on the device, zeros when absent
    (include/cslgan.h "Kernel two-sample test").  csl_gan_amd.kernel_test.tri_hist_host is the host model."""
    what = "tri_hist"
    n = _mmd_matrix(what, d2)
    if hist is None:
        hist = torch.zeros(256, device=d2.device, dtype=torch.int64)
    else:
        _mom_operands(what, [(hist, "hist", torch.int64)])
        if tuple(hist.shape) != (256,):
            raise RuntimeError("%s: hist has the shape %s, expected (256,)" % (what, tuple(hist.shape)))
    check(_lib.lib().cslgan_tri_hist_u32(_p(d2), d2.shape[1], n, int(prefix) & 0xFFFFFFFF, int(prefix_bits), _p(hist), _stream()), what)
    return hist


def mmd_kernel(d2, hi, lo):
    """d2 rewritten in place as Kq = sum_b rint(2^28 hi[b, d2 >> 16] lo[b, d2 & 65535]), zero on the diagonal: d2 the matrix of gram_d2,
    hi / lo float64 [B, 65536] on the device, B <= 7.  csl_gan_amd.kernel_test.kernel_matrix_host is the host model, equalled bit for bit."""
    what = "mmd_kernel"
    n = _mmd_matrix(what, d2, [(hi, "hi", torch.float64), (lo, "lo", torch.float64)])
    if hi.dim() != 2 or hi.shape[1] != MMD_TABLE or tuple(lo.shape) != tuple(hi.shape):
        raise RuntimeError("%s: need hi and lo [B, %d], got %s and %s" % (what, MMD_TABLE, tuple(hi.shape), tuple(lo.shape)))
    check(_lib.lib().cslgan_mmd_kernel_u32(_p(d2), d2.shape[1], n, _p(hi), _p(lo), hi.shape[0], _stream()), what)
    return d2


def mmd_partition_sums(kq, member, sxx2=None, sxy=None):
    """(sxx2, sxy) int64 [P], added to in place (zeros when absent): with r[i, p] = sum_j kq[i, j] member[p, j], sxx2[p] += the sum of
    r[i, p] over the rows i that member[p, i] marks and sxy[p] += the sum over the others.  kq: int32 [n, gram_pitch(n)] holding uint32
    entries below 2^31; member: int8 [P, mmd_padded_cols(n)].  csl_gan_amd.kernel_test.partition_sums_host is the host model."""
    what = "mmd_partition_sums"
    n = _mmd_matrix(what, kq, [(member, "member", torch.int8)])
    if member.dim() != 2 or member.shape[0] < 1 or member.shape[1] < n:
        raise RuntimeError("%s: need member [P, ldm >= n = %d], got %s" % (what, n, tuple(member.shape)))
    P = member.shape[0]
    outs = []
    for t, name in ((sxx2, "sxx2"), (sxy, "sxy")):
        if t is None:
            t = torch.zeros(P, device=kq.device, dtype=torch.int64)
        else:
            _mom_operands(what, [(t, name, torch.int64)])
            if tuple(t.shape) != (P,):
                raise RuntimeError("%s: %s has the shape %s, expected (%d,)" % (what, name, tuple(t.shape), P))
        outs.append(t)
    check(_lib.lib().cslgan_mmd_partition_sums_i64(_p(kq), kq.shape[1], n, _p(member), member.shape[1], P, _p(outs[0]), _p(outs[1]), _stream()), what)
    return outs[0], outs[1]


def row_l2norm(t2d):
    _chk(t2d, "t")
    n, L = t2d.shape
    out = torch.empty(n, device=t2d.device, dtype=torch.float32)
    check(_lib.lib().cslgan_row_l2norm_f32(_p(t2d), n, L, _p(out), _stream()), "row_l2norm")
    return out


def row_l2norm_bwd(t2d, norm, gnorm):
    _chk(t2d, "t"); _chk(norm, "norm"); _chk(gnorm, "gnorm")
    n, L = t2d.shape
    out = torch.empty_like(t2d)
    check(_lib.lib().cslgan_row_l2norm_bwd_f32(_p(t2d), _p(norm), _p(gnorm), n, L, _p(out), _stream()), "row_l2norm_bwd")
    return out


def act_bwd(g, y, slope):
    if g.dtype == torch.bfloat16 or y.dtype == torch.bfloat16:
        if g.dtype == y.dtype and g.numel() % 8 == 0:
            _chk(g, "g", allow_bf16=True); _chk(y, "y", allow_bf16=True)
            out = torch.empty_like(g)
            check(_lib.lib().cslgan_act_bwd_bf16(_p(g), _p(y), g.numel(), float(slope), _p(out), _stream()), "act_bwd_bf16")
            return out
        out = act_bwd(cast_f32(g), cast_f32(y), slope)
        return cast_bf16(out) if g.dtype == torch.bfloat16 else out
    _chk(g, "g"); _chk(y, "y")
    out = torch.empty_like(g)
    check(_lib.lib().cslgan_act_bwd_f32(_p(g), _p(y), g.numel(), float(slope), _p(out), _stream()), "act_bwd")
    return out


def _d2s_out(x, d2s, want_raw, dtype=torch.float32):
    """(y, xs, dW, rpi) of a normalisation: the output, x's own shuffled copy (want_raw) or None, and what tells the kernels to write
    depth-to-space shuffled — the row width and the rows per image of x (0, 0: plain)."""
    if not d2s:
        if want_raw:
            raise RuntimeError("want_raw needs d2s=True")
        return torch.empty_like(x, dtype=dtype), None, 0, 0
    N, H, W, Cc = x.shape
    if Cc % 4:
        raise RuntimeError("depth-to-space output needs C %% 4 == 0 (C=%d)" % Cc)
    shp = (N, 2 * H, 2 * W, Cc // 4)
    y = torch.empty(shp, device=x.device, dtype=dtype)
    return y, (torch.empty(shp, device=x.device, dtype=dtype) if want_raw else None), W, H * W


_norm_scratch = {}


NORM_PARTIAL_BLOCKS = _lib.NORM_PARTIAL_BLOCKS


def _scratch(dev, n_stats_floats):
    """Workspace for the per-workgroup partial statistics of the two-launch normalisation (cslgan_groupnorm_act_f32's `scratch`):
    n_stats_floats (= 2 * statistics) x NORM_PARTIAL_BLOCKS floats, persistent per (device, stream) — launches on one stream are
    ordered, and nothing in it outlives the apply launch that follows."""
    need = int(n_stats_floats) * NORM_PARTIAL_BLOCKS
    key = (dev, torch.cuda.current_stream().cuda_stream)
    t = _norm_scratch.get(key)
    if t is None or t.numel() < need:
        t = _norm_scratch[key] = torch.empty(max(need, 1 << 16), device=dev, dtype=torch.float32)
    return t


def groupnorm_act(x, gamma, beta, groups, eps=1e-5, relu=True, return_stats=False, d2s=False, want_raw=False, out_dtype=None, part=None):
    """GroupNorm(+ReLU).  d2s=True: the output is written depth-to-space shuffled ([N,2H,2W,C/4], see depth_to_space);
    want_raw=True additionally returns the raw x in that layout (one read of x feeds ResBlockUp's convUp and shortcut).
    out_dtype torch.bfloat16 (or a bfloat16 x): bf16-stored outputs (set_storage_dtype), fp32 statistics and arithmetic."""
    stored = x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16
    _chk(x, "x", allow_bf16=stored); _chk(gamma, "gamma"); _chk(beta, "beta")
    N, H, W, Cc = x.shape
    y, xs, dW, _ = _d2s_out(x, d2s, want_raw, torch.bfloat16 if stored else torch.float32)
    ws = torch.empty(2 * N * groups, device=x.device, dtype=torch.float32)
    lib = _lib.lib()
    if stored:
        check(lib.cslgan_groupnorm_act_bf16s(_p(x), 1 if x.dtype == torch.bfloat16 else 0, _p(gamma), _p(beta), N, H * W, Cc, groups,
                                             float(eps), 1 if relu else 0, _p(ws), _p(y), dW, _p(xs), _stream()), "groupnorm_act_bf16s")
    elif part is not None:      # statistics left by the producing conv's epilogue (gn_partials): the apply launch alone
        pt, n_part = part
        check(lib.cslgan_groupnorm_apply_parts_f32(_p(x), _p(gamma), _p(beta), N, H * W, Cc, groups, float(eps), 1 if relu else 0,
                                                   _p(pt), n_part, _p(ws), _p(y), dW, _p(xs), _stream()), "groupnorm_apply_parts")
    else:
        sc = _scratch(x.device, 2 * N * groups)
        check(lib.cslgan_groupnorm_act_f32(_p(x), _p(gamma), _p(beta), N, H * W, Cc, groups, float(eps), 1 if relu else 0,
                                           _p(ws), _p(y), dW, _p(xs), _p(sc), _stream()), "groupnorm_act")
    out = (y, xs) if want_raw else y
    return (out, ws) if return_stats else out


_GN_SHORTCUT_FUSE = True   # ResBlockUp's bn1 apply, shuffle and 1x1 shortcut conv in one launch (tests switch it off to compare)


def gn_shortcut_ok(x, K, part):
    """Does groupnorm_apply_shortcut take this block?  (csrc/gn_shortcut.hip: C/4 in {32, 64, 128}, K a multiple of 64, the
    statistics of a conv epilogue.)"""
    if not (_GN_SHORTCUT_FUSE and part is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    N, H, W, Cc = x.shape
    return Cc in (128, 256, 512) and K >= 64 and K % 64 == 0 and N <= 65535 and H * W == 64 * part[1] and 4 * H * W * K < 2 ** 31


def groupnorm_apply_shortcut(x, gamma, beta, groups, part, wf, bias=None, eps=1e-5, relu=True, return_stats=False):
    """(a_ps, s) of ResBlockUp from one read of x[N,H,W,C]: a_ps[N,2H,2W,C/4] = depth_to_space(act(groupnorm(x))) exactly as
    groupnorm_act(d2s=True, part=part) writes it, and s[N,2H,2W,K] = conv1x1(depth_to_space(x), wf[K,1,1,C/4]) + bias — the raw
    shuffled x never reaches HBM.  part: the conv-epilogue statistics of x (gn_partials); wf: the folded shortcut filter."""
    _chk(x, "x"); _chk(gamma, "gamma"); _chk(beta, "beta"); _chk(wf, "wf")
    N, H, W, Cc = x.shape
    K = wf.shape[0]
    if wf.numel() != K * (Cc // 4):
        raise RuntimeError("groupnorm_apply_shortcut: wf must be [K, 1, 1, C/4] = [%d, 1, 1, %d]" % (K, Cc // 4))
    if bias is not None:
        _chk(bias, "bias")
        if bias.numel() != K:
            raise RuntimeError("groupnorm_apply_shortcut: bias must have K = %d elements" % K)
    pt, n_part = part
    a_ps = torch.empty((N, 2 * H, 2 * W, Cc // 4), device=x.device, dtype=torch.float32)
    s = torch.empty((N, 2 * H, 2 * W, K), device=x.device, dtype=torch.float32)
    ws = torch.empty(2 * N * groups, device=x.device, dtype=torch.float32)
    rows = 4 * N * H * W
    # timed as the shortcut conv it replaces: the reference runs it over four identical channel groups
    _timed("groupnorm_apply_shortcut", 2.0 * rows * K * Cc, 4.0 * (2 * N * H * W * Cc + wf.numel() + rows * K),
           lambda: check(_lib.lib().cslgan_groupnorm_apply_parts_shortcut_f32(
               _p(x), _p(gamma), _p(beta), N, H * W, Cc, groups, float(eps), 1 if relu else 0, _p(pt), n_part, _p(ws), _p(a_ps), W,
               _p(wf), _p(bias), K, _p(s), _stream()), "groupnorm_apply_parts_shortcut"),
           exec_flop=2.0 * rows * K * (Cc // 4), tag=lambda: "N%d %dx%d C%d K%d" % (N, H, W, Cc, K))
    return (a_ps, s, ws) if return_stats else (a_ps, s)


def batchnorm_act(x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True, return_stats=False,
                  d2s=False, want_raw=False):
    """Training-mode BatchNorm (+ReLU) over all leading dims of NHWC x; updates the running stats in place.
    d2s / want_raw as for groupnorm_act (x must then be 4-D)."""
    _chk(x, "x"); _chk(gamma, "gamma"); _chk(beta, "beta")
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y, xs, dW, rpi = _d2s_out(x, d2s, d2s and want_raw)
    ws = torch.empty(2 * Cc, device=x.device, dtype=torch.float32)
    check(_lib.lib().cslgan_batchnorm_act_f32(_p(x), _p(gamma), _p(beta), rows, Cc, float(eps), 1 if relu else 0, float(momentum),
                                              _p(running_mean), _p(running_var), _p(ws), _p(y), rpi, dW, _p(xs),
                                              _p(_scratch(x.device, 2 * Cc)), _stream()), "batchnorm_act")
    out = (y, xs) if want_raw else y
    return (out, ws) if return_stats else out


def batchnorm_eval_act(x, gamma, beta, running_mean, running_var, eps=1e-5, relu=True, d2s=False, want_raw=False):
    """Eval-mode BatchNorm (+ReLU) from the running statistics (the generator in eval(), train.py:298-308)."""
    for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _chk(t, n)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y, xs, dW, rpi = _d2s_out(x, d2s, d2s and want_raw)
    ws = torch.empty(2 * Cc, device=x.device, dtype=torch.float32)
    check(_lib.lib().cslgan_batchnorm_eval_act_f32(_p(x), _p(gamma), _p(beta), _p(running_mean), _p(running_var), rows, Cc, float(eps),
                                                   1 if relu else 0, _p(ws), _p(y), rpi, dW, _p(xs), _stream()), "batchnorm_eval_act")
    return (y, xs) if want_raw else y


def adam_step(p, g, m, v, lr, b1, b2, eps, weight_decay, step):
    """step: int (1-based, passed by value) or a device int32 tensor [1] read by the kernel (graph-captured steps)."""
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, n)
    if isinstance(step, torch.Tensor):
        if step.dtype != torch.int32 or not step.is_cuda:
            raise RuntimeError("adam_step: a tensor step must be a device int32 tensor")
        check(_lib.lib().cslgan_adam_step_dev_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(b1), float(b2), float(eps),
                                                  float(weight_decay), _p(step), _stream()), "adam_step_dev")
        return
    check(_lib.lib().cslgan_adam_step_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(b1), float(b2), float(eps),
                                          float(weight_decay), int(step), _stream()), "adam_step")


def adam_multi(ps, gs, ms, vs, lr, b1, b2, eps, weight_decay, step):
    """Adam over lists of flat fp32 tensors in ONE launch per <= 16 tensors.  step: int (1-based) or a device int32 [1] tensor."""
    dev_step = isinstance(step, torch.Tensor)
    if dev_step and (step.dtype != torch.int32 or not step.is_cuda):
        raise RuntimeError("adam_multi: a tensor step must be a device int32 tensor")
    for lst, nm in ((ps, "p"), (gs, "g"), (ms, "m"), (vs, "v")):
        for t in lst:
            _chk(t, nm)
    L = _lib.lib()
    VP = C.c_void_p
    for i in range(0, len(ps), _lib.MAX_SEGS):
        sub = range(i, min(i + _lib.MAX_SEGS, len(ps)))
        n = len(sub)
        arr = lambda lst: (VP * n)(*[lst[j].data_ptr() for j in sub])
        check(L.cslgan_adam_multi_f32(n, arr(ps), arr(gs), arr(ms), arr(vs), (C.c_int64 * n)(*[ps[j].numel() for j in sub]), float(lr),
                                      float(b1), float(b2), float(eps), float(weight_decay), 0 if dev_step else int(step),
                                      _p(step) if dev_step else None, _stream()), "adam_multi")


def _roles(sizes, scale):
    n = len(sizes)
    if not 1 <= n <= 8 or len(scale) != n:
        raise RuntimeError("segment means: 1..8 row blocks with one scale each, got %d / %d" % (n, len(scale)))
    return n, (C.c_int32 * n)(*[int(s) for s in sizes]), (C.c_float * n)(*[float(s) for s in scale])


def segment_means(x, sizes, scale):
    """vec[s] = scale[s] * sum(x[block s]), total = sum(vec): the critic's +-mean losses over the row blocks of one pass."""
    _chk(x, "x")
    if x.numel() != sum(sizes):
        raise RuntimeError("segment_means: %d values for blocks %s" % (x.numel(), list(sizes)))
    n, cs, sc = _roles(sizes, scale)
    out = torch.empty(n + 1, device=x.device, dtype=torch.float32)
    check(_lib.lib().cslgan_segment_means_f32(_p(x), n, cs, sc, _p(out), C.c_void_p(out.data_ptr() + 4 * n), _stream()), "segment_means")
    return out[:n], out[n]


def segment_means_bwd(g_total, g_vec, sizes, scale, shape, device):
    n, cs, sc = _roles(sizes, scale)
    gx = torch.empty(shape, device=device, dtype=torch.float32)
    check(_lib.lib().cslgan_segment_means_bwd_f32(_p(g_total), _p(g_vec), n, cs, sc, _p(gx), _stream()), "segment_means_bwd")
    return gx


def dstep_stats(d_real, d_fake, real_loss, fake_loss, penalty, acc7):
    """train.py:488-496 in one launch; acc7 (persistent, device) += the seven statistics (see include/cslgan.h)."""
    for t, nm in ((d_real, "d_real"), (d_fake, "d_fake"), (real_loss, "real_loss"), (fake_loss, "fake_loss"), (acc7, "acc7")):
        _chk(t, nm)
    if acc7.numel() != 7:
        raise RuntimeError("dstep_stats: acc7 must hold 7 floats")
    if penalty is not None:
        _chk(penalty, "penalty")
    check(_lib.lib().cslgan_dstep_stats_f32(_p(d_real), d_real.numel(), _p(d_fake), d_fake.numel(), _p(real_loss), _p(fake_loss),
                                            _p(penalty), _p(acc7), _stream()), "dstep_stats")


def grad_log_stats(sq, col0, B, max_norm, per_layer, eps, acc):
    """update_grad_logging (train.py:310-329) from the clip's squared norms sq [L, ld]; acc: [5, L or 1] persistent sums
    (means, stds, maxes, clip norms, clipped fraction)."""
    _chk(sq, "sq"); _chk(max_norm, "max_norm"); _chk(acc, "acc")
    Lr, ld = sq.shape
    rows = Lr if per_layer else 1
    if tuple(acc.shape) != (5, rows) or max_norm.numel() < (rows if per_layer else 1):
        raise RuntimeError("grad_log_stats: acc must be [5, %d] and max_norm hold %d value(s)" % (rows, rows))
    a = [C.c_void_p(acc.data_ptr() + 4 * rows * i) for i in range(5)]
    check(_lib.lib().cslgan_grad_log_stats_f32(_p(sq), Lr, ld, int(col0), int(B), _p(max_norm), 1 if per_layer else 0, float(eps),
                                               a[0], a[1], a[2], a[3], a[4], _stream()), "grad_log_stats")


def _mem_order(t):
    return tuple(st for sz, st in zip(t.shape, t.stride()) if sz > 1)


def lerp_rows(real, fake, alpha):
    """alpha[b] * real[b] + (1 - alpha[b]) * fake[b] (gradient_penalty.py:36).  real / fake: same shape, same dense memory order
    (contiguous or channels-last), batch outermost; the result has real's strides."""
    _chk(alpha, "alpha")
    for t, nm in ((real, "real"), (fake, "fake")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError("lerp_rows: %s must be a float32 device tensor" % nm)
        if not (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
            raise RuntimeError("lerp_rows: %s is not dense" % nm)
    if real.shape != fake.shape or _mem_order(real) != _mem_order(fake):
        raise RuntimeError("lerp_rows: real and fake must share shape and memory order")
    B = real.shape[0]
    if alpha.numel() != B or (B > 1 and real.stride(0) * B != real.numel()):
        raise RuntimeError("lerp_rows: alpha must hold one weight per row of a batch-outermost tensor")
    out = torch.empty_strided(real.shape, real.stride(), device=real.device, dtype=torch.float32)
    check(_lib.lib().cslgan_lerp_rows_f32(_p(real), _p(fake), _p(alpha), B, real.numel() // B, _p(out), _stream()), "lerp_rows")
    return out


_tickets = {}


def _ticket(dev):
    t = _tickets.get(dev)
    if t is None:
        t = _tickets[dev] = torch.zeros(1, device=dev, dtype=torch.int32)
    return t


def lipschitz_term(t2d, one_sided, coef):
    """(norm [B], per [B], total []) with per = coef * (||t_b|| - 1)^2 (clamped at 0 from below when one_sided)."""
    _chk(t2d, "t")
    n, Ln = t2d.shape
    buf = torch.empty(2 * n + 1, device=t2d.device, dtype=torch.float32)
    check(_lib.lib().cslgan_lipschitz_term_f32(_p(t2d), n, Ln, 1 if one_sided else 0, float(coef), _p(buf),
                                               C.c_void_p(buf.data_ptr() + 4 * n), C.c_void_p(buf.data_ptr() + 8 * n),
                                               _p(_ticket(t2d.device)), _stream()), "lipschitz_term")
    return buf[:n], buf[n:2 * n], buf[2 * n]


def lipschitz_term_bwd(t2d, norm, g_total, g_per, one_sided, coef):
    _chk(t2d, "t"); _chk(norm, "norm")
    n, Ln = t2d.shape
    out = torch.empty_like(t2d)
    check(_lib.lib().cslgan_lipschitz_term_bwd_f32(_p(t2d), _p(norm), _p(g_total), _p(g_per), n, Ln, 1 if one_sided else 0, float(coef),
                                                   _p(out), _stream()), "lipschitz_term_bwd")
    return out
