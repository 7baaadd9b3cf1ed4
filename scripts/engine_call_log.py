"""What does csl_gan_amd.engine.PrivacyEngine launch for a D-step, and what does it leave on the parameters?  A log taken without a GPU.

The engine is host logic: per layer and row block it decides between norms only, a dense sum, materialised per-sample gradients and
ghost clipping, and clip() turns what was collected into the clipped sum.  Here it runs on a small critic

    HipConv2d(3, 64, 5, stride 2) on 32x32      the first-layer (c3) route
    HipConv2d(64, 64, 5, stride 2)  -> 8x8      Gram-preferred (a ghost layer); materialised: the blocks route
    HipConv2d(64, 128, 5, stride 2) -> 4x4      Gram-preferred
    HipLinear(2048, 1)                          the head

with B = 4, against the recording stand-in of scripts/conv_dispatch_log.py (imported, not copied) and with torch.cuda.current_stream /
Stream / stream replaced by no-ops.  No forward or backward runs: the collectors are driven by hand with zero-filled (gz, x) in
backward order, then the engine's public surface is called as Trainer.train_D does.

A case logs, in order, every library call (entry, scalars, struct fields; for each pointer where it points AT CALL TIME: the gz / x of
a layer, a live p.grad_sample._cslgan_rows, p.summed_grad, the squared-norm arena, an _idx_cache tensor, else "new") interleaved with
every ATen operator that is not a view or an allocation, and the state left on the parameters after each stage.

    python scripts/engine_call_log.py                          # entry names per case
    python scripts/engine_call_log.py --case fused_ghost_fp32_flat_mean
    python scripts/engine_call_log.py --time                   # host time of the whole list
    python scripts/engine_call_log.py --root ../parent --record tests/engine_calls.json

tests/engine_calls.json holds, per case, the ordered entry names and a SHA-1 of the canonical JSON of the full log, recorded with
--root pointing at a checkout of the commit BEFORE the engine was rewritten around one row-block handler;
tests/test_engine_calls.py asserts them.  Only the engine's public surface (and _before_step) is driven, so the script runs unchanged
on that commit.
"""
import argparse
import contextlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_dispatch_log import ROOT, Harness, Patches, digest      # noqa: E402

B = 4
# (cin, cout, input side, output side); every conv is 5x5, stride 2, pad 2; then HipLinear(128 * 4 * 4, 1)
CONVS = ((3, 64, 32, 16), (64, 64, 16, 8), (64, 128, 8, 4))
HEAD_IN = 128 * 4 * 4

# entries the case list must reach (tests/test_engine_calls.py); the second group only through the bf16-storage case
ENTRIES = sorted("cslgan_" + n for n in (
    "conv2d_wgrad_grouped_f32", "conv2d_wgrad_grouped_bf16out_f32", "conv2d_wgrad_blocks_f32", "conv2d_wgrad_scaled_f32",
    "conv2d_wgrad_sqnorm_gram_f32", "bias_grad_grouped_f32", "sample_sqnorm_f32", "clip_factors_f32", "adaptive_clip_f32",
    "clip_accum_noise_f32", "sample_sqnorm_bf16", "clip_accum_noise_bf16"))
ENTRIES_BF16S = sorted("cslgan_" + n for n in ("conv2d_c3_wgrad_bf16gy", "conv2d_wgrad_scaled_bf16s", "linear_k1_wgrad_bf16s",
                                                "bias_grad_grouped_bf16"))

# ATen operators that launch nothing: allocations and aliases (views are recognised by their schema)
_NO_LAUNCH = {"aten.empty.memory_format", "aten.empty_like.default", "aten.empty_strided.default", "aten.detach.default",
              "aten.alias.default", "aten.lift_fresh.default", "aten.new_empty.default"}


class _Stream:
    """torch.cuda.Stream / current_stream / stream without a device: nothing to order."""

    def __init__(self, *a, **k):
        pass

    def wait_stream(self, other):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class EngineHarness(Harness):
    def __init__(self, setattr_fn, root=ROOT, aten=True):
        super().__init__(setattr_fn, root=root, timer=False)
        torch = self.torch
        setattr_fn(torch.cuda, "current_stream", lambda *a, **k: _Stream())
        setattr_fn(torch.cuda, "Stream", _Stream)
        setattr_fn(torch.cuda, "stream", lambda s: _Stream())
        from csl_gan_amd import engine, nn as hnn
        self.engine, self.hnn, self.aten = engine, hnn, aten
        self.pe = None
        # aten=False is the --time mode: the clock should see the engine, so the stand-in library only counts calls and the critic and
        # the zero tensors are made once and reused
        self._pool = None if aten else {}
        from torch.utils._python_dispatch import TorchDispatchMode
        h = self

        class AtenLog(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                name = str(func)
                if not getattr(func, "is_view", False) and name not in _NO_LAUNCH:
                    h.calls.append({"aten": name, "shapes": [list(a.shape) for a in args if isinstance(a, torch.Tensor)],
                                    "out": list(out.shape) if isinstance(out, torch.Tensor) else None})
                return out

        self._aten_mode = AtenLog

    def __getattr__(self, name):
        if self.__dict__.get("_pool") is None or name == "cslgan_last_kernel":
            return super().__getattr__(name)
        if not name.startswith("cslgan_"):
            raise AttributeError(name)
        return self._count

    def _count(self, *args):
        self.n_untraced += 1
        return 0

    n_untraced = 0

    def _zeros(self, shape, dtype):
        if self._pool is None:
            return self.torch.zeros(shape, dtype=dtype)
        t = self._pool.get((shape, dtype))
        if t is None:
            t = self._pool[(shape, dtype)] = self.torch.zeros(shape, dtype=dtype)
        return t

    # -- where a pointer points, resolved when the call is made
    def _where(self, addr):
        if not addr:
            return "null"
        for lo, hi, name in self._live():
            if lo <= addr < hi:
                return name if addr == lo else "%s+%d" % (name, addr - lo)
        return "new"

    def _live(self):
        yield from self.spans
        pe = self.pe
        if pe is None:
            return
        known = []
        for name, p in pe.module.named_parameters():
            gs = getattr(p, "grad_sample", None)
            if gs is not None and getattr(gs, "_cslgan_rows", None) is not None:
                known.append(("rows[%s]" % name, gs._cslgan_rows))
            if getattr(p, "summed_grad", None) is not None:
                known.append(("summed[%s]" % name, p.summed_grad))
        if pe._sq_arena is not None:
            known.append(("arena", pe._sq_arena))
        known += [("cache%d" % i, t) for i, t in enumerate(pe._idx_cache.values())]
        for name, t in known:
            yield t.data_ptr(), t.data_ptr() + max(1, t.numel()) * t.element_size(), name

    # -- the critic and its engine
    def make_engine(self, materialize="all", accum=True, gs="fp32", per_layer=False):
        torch, hnn = self.torch, self.hnn
        layers = None if self._pool is None else self._pool.get("layers")
        if layers is None:
            layers = [hnn.HipConv2d(cin, cout, 5, stride=2, padding=2) for cin, cout, _, _ in CONVS] + [hnn.HipLinear(HEAD_IN, 1)]
            for l in layers[:-1]:
                l.weight.data = l.weight.data.contiguous(memory_format=torch.channels_last)     # as the models keep their filters
            if self._pool is not None:
                self._pool["layers"] = layers
        self.layers = layers
        module = torch.nn.Sequential(*layers)
        n_params = 2 * len(layers)
        self.pe = self.engine.PrivacyEngine(module, batch_size=B, sample_size=1000, alphas=[2.0, 4.0], noise_multiplier=1.1,
                                            max_grad_norm=[1.0 + 0.5 * i for i in range(n_params)] if per_layer else 1.0,
                                            accum_passes=accum, num_private_passes=None if accum else 1,
                                            auto_clip_and_accum_on_step=False, materialize=materialize, grad_sample_dtype=gs)
        self.pe._set_seed(5)
        return self.pe

    def backward(self, n_passes, rows, stored_bf16=False):
        """n_passes forwards (next_pass per layer, in forward order), then one backward: passes and layers in reverse order, each
        layer handing zero-filled (gz, x) of `rows` rows to its collector."""
        torch, pe = self.torch, self.pe
        idx = [[pe.next_pass(l) for l in self.layers] for _ in range(n_passes)]
        act = torch.bfloat16 if stored_bf16 else torch.float32
        for k in reversed(range(n_passes)):
            for li in reversed(range(len(self.layers))):
                layer = self.layers[li]
                if li == len(CONVS):           # the head: fp32 loss cotangent, features as stored
                    gz, x, geo = self._zeros((rows, 1, 1, 1), torch.float32), self._zeros((rows, 1, 1, HEAD_IN), act), (1, 1, 1, 0)
                else:
                    cin, cout, hin, hout = CONVS[li]
                    gz = self._zeros((rows, hout, hout, cout), act)
                    x = self._zeros((rows, hin, hin, cin), torch.float32 if li == 0 else act)     # the image stays fp32
                    geo = (5, 5, 2, 2)
                for t, nm in ((gz, "gz"), (x, "x")):
                    self.spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), "%s%dp%d" % (nm, li, idx[k][li])))
                    self.keep.append(t)
                pe.collector(layer).collect(idx[k][li], gz, x, *geo, True)

    # -- what is left behind
    def snap(self, label):
        pe, params = self.pe, {}
        for name, p in pe.module.named_parameters():
            st = {"grad_sample": hasattr(p, "grad_sample")}
            if st["grad_sample"]:
                gs = p.grad_sample
                rows = getattr(gs, "_cslgan_rows", None)
                st.update(shape=list(gs.shape), stride=list(gs.stride()), dtype=str(gs.dtype), rows=None if rows is None else list(rows.shape),
                          rows_share_storage=rows is not None and rows.untyped_storage().data_ptr() == gs.untyped_storage().data_ptr()
                          and rows.storage_offset() == gs.storage_offset())
            if getattr(p, "summed_grad", None) is not None:
                st["summed_grad_stride"] = list(p.summed_grad.stride())
            if p.grad is not None:
                st["grad"] = [p.grad.storage_offset(), list(p.grad.stride())]
            params[name] = st
        shape = lambda t: None if t is None else list(t.shape)
        self.state.append({"at": label, "params": params, "per_layer": pe._per_layer, "n_calls": len(self.calls),
                           "last_sq": shape(getattr(pe, "last_sq", None)), "last_factors": shape(getattr(pe, "last_factors", None))})

    def note(self, key, value):
        self.state.append({key: value, "n_calls": len(self.calls)})

    # -- cases
    def run(self, name):
        fn, kw = CASES[name]
        self.spans, self.keep, self.state, self.pe = [], [], [], None
        with contextlib.ExitStack() as stack:
            if kw.get("stored_bf16"):
                stack.enter_context(self.ops.storage_dtype("bf16"))
            if self.aten:
                stack.enter_context(self._aten_mode())
            fn(self, **kw)

    def log(self, name):
        self.calls, self.repack = [], []
        self.run(name)
        log = {"calls": self.calls, "repack": self.repack, "state": self.state}
        self.pe = None
        return log


def _finish(h):
    """clip() -> accumulate_batch() -> the noised gradient, as train_D ends a gc step."""
    pe = h.pe
    pe.clip()
    h.snap("clip")
    pe.accumulate_batch()
    pe._before_step()
    h.snap("step")


def _adaptive_norm(h, r, per_layer):
    h.pe.set_max_grad_norm_device(r * 1.5 if per_layer else (r.norm(2) * 1.5).reshape(1))


def separate(h, materialize, accum, gs, per_layer, steps=1, penalty=False):
    """update_adaptive_clipping_params (a norms_only = lean pass), then the generated and the real pass, clip and step."""
    torch = h.torch
    pe = h.make_engine(materialize, accum, gs, per_layer)
    for _ in range(steps):
        with torch.no_grad():
            pe.norms_only = pe.lean
            h.backward(2 if accum else 1, B)          # accumulated clipping differentiates the generated pass here too
            pe.norms_only = False
            h.snap("adaptive pass")
            sq = pe.sample_sqnorms()
            h.note("sample_sqnorms", list(sq.shape))
            _adaptive_norm(h, sq[:, :B].sqrt().mean(dim=1), per_layer)
            pe.zero_grad()
            h.backward(2, B)
            h.snap("passes")
            if penalty:
                pe.clip()
                h.snap("first clip")
                for p in pe.params:
                    pe.add_to_grad_sample(p, h._zeros((B, p.numel()), torch.float32), 0)
                pe.clip(recompute_norms=True)
                h.snap("clip")
                pe.accumulate_batch()
                pe._before_step()
                h.snap("step")
            else:
                _finish(h)


def plain(h, materialize, accum, gs, per_layer):
    """Collect two passes and clip(): no adaptive pass."""
    h.make_engine(materialize, accum, gs, per_layer)
    with h.torch.no_grad():
        h.backward(2, B)
        h.snap("passes")
        _finish(h)


def fused(h, materialize, gs, per_layer, roles, adapt=None, steps=1, stored_bf16=False, relist=False):
    """Trainer._fused_passes: one backward over the row blocks.  adapt: "mean" / "max" -> adaptive_clip_fused; "separate" -> the
    statistic from norms_rows_sqnorms() and set_max_grad_norm_device (world_size > 1); None -> the clip norm stays."""
    torch = h.torch
    pe = h.make_engine(materialize, False, gs, per_layer)
    for _ in range(steps):
        with torch.no_grad():
            pe.zero_grad()
            pe.row_roles = list(roles)
            h.backward(1, sum(n for _, n in roles), stored_bf16)
            h.snap("passes")
            r = None
            if adapt in ("mean", "max"):
                r = pe.adaptive_clip_fused(adapt, 1.5, per_layer)
                h.note("adaptive_clip_fused", None if r is None else list(r.shape))
            if adapt is not None and r is None:
                norms = pe.norms_rows_sqnorms().sqrt()
                _adaptive_norm(h, norms.mean(dim=1) if adapt != "max" else norms.max(dim=1).values, per_layer)
            if relist:                                 # a per-layer list set by hand after the fused launch: its results must be dropped
                pe.set_max_grad_norm([2.0] * len(pe.params))
            pe.row_roles = None
            _finish(h)


CASES = {}
_FL = ((False, "flat"), (True, "pl"))
_GS = ("fp32", "bf16")
for mat in ("all", "private", "ghost"):
    for accum in (True, False):
        if mat == "ghost" and accum:
            continue
        for gs in _GS:
            for pl, pln in _FL:
                CASES["sep_%s_%s_%s_%s" % (mat, "accum" if accum else "split", gs, pln)] = (separate, dict(
                    materialize=mat, accum=accum, gs=gs, per_layer=pl))
for accum in (True, False):
    for gs in _GS:
        for pl, pln in _FL:
            CASES["penalty_all_%s_%s_%s" % ("accum" if accum else "split", gs, pln)] = (separate, dict(
                materialize="all", accum=accum, gs=gs, per_layer=pl, penalty=True))
CASES["plain_all_accum"] = (plain, dict(materialize="all", accum=True, gs="fp32", per_layer=False))
CASES["plain_all_split_pl"] = (plain, dict(materialize="all", accum=False, gs="fp32", per_layer=True))
_NDP = (("norms", B), ("dense", B), ("private", B))
for mat in ("private", "ghost"):
    for gs in _GS:
        for pl, pln in _FL:
            for adapt in ("mean", "max", "separate"):
                CASES["fused_%s_%s_%s_%s" % (mat, gs, pln, adapt)] = (fused, dict(materialize=mat, gs=gs, per_layer=pl, roles=_NDP, adapt=adapt))
    for pl, pln in _FL:
        CASES["fused_%s_%s_fixed" % (mat, pln)] = (fused, dict(materialize=mat, gs="fp32", per_layer=pl, roles=(("dense", B), ("private", B))))
        CASES["fused_%s_%s_unequal" % (mat, pln)] = (fused, dict(materialize=mat, gs="fp32", per_layer=pl, adapt="mean",
                                                                 roles=(("norms", 2), ("dense", B), ("private", B))))
        CASES["fused_%s_%s_relist" % (mat, pln)] = (fused, dict(materialize=mat, gs="fp32", per_layer=pl, roles=_NDP, adapt="mean", relist=True))
    CASES["fused_%s_bf16_fixed" % mat] = (fused, dict(materialize=mat, gs="bf16", per_layer=False, roles=(("dense", B), ("private", B))))
    CASES["fused_%s_private_dense" % mat] = (fused, dict(materialize=mat, gs="fp32", per_layer=False, roles=(("private", B), ("dense", B))))
    CASES["fused_%s_dense_dense_private" % mat] = (fused, dict(materialize=mat, gs="fp32", per_layer=True,
                                                               roles=(("dense", B), ("dense", B), ("private", B))))
    CASES["fused_%s_two_steps" % mat] = (fused, dict(materialize=mat, gs="fp32", per_layer=True, roles=_NDP, adapt="mean", steps=2))
for pl, pln in _FL:
    CASES["fused_ghost_%s_stored_bf16" % pln] = (fused, dict(materialize="ghost", gs="fp32", per_layer=pl, roles=_NDP, adapt="mean", stored_bf16=True))
CASES["fused_ghost_stored_bf16_fixed"] = (fused, dict(materialize="ghost", gs="fp32", per_layer=False, roles=(("dense", B), ("private", B)),
                                                      stored_bf16=True))
CASES["sep_ghost_two_steps"] = (separate, dict(materialize="ghost", accum=False, gs="fp32", per_layer=False, steps=2))
CASES["sep_all_two_steps"] = (separate, dict(materialize="all", accum=True, gs="bf16", per_layer=True, steps=2))


def lib_entries(log):
    return [c["entry"] for c in log["calls"] if "entry" in c]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=ROOT, help="checkout whose csl_gan_amd is driven (default: this one)")
    ap.add_argument("--case", help="print the full log of this case")
    ap.add_argument("--record", metavar="JSON", help="write {case: {entries, sha1}} to this file")
    ap.add_argument("--time", action="store_true", help="host seconds for the whole case list, nothing but the library stand-in installed")
    ap.add_argument("--passes", type=int, default=10, help="--time: passes over the list (per case the fastest counts)")
    a = ap.parse_args()
    p = Patches()
    h = EngineHarness(p.setattr, root=os.path.abspath(a.root), aten=not a.time)
    try:
        if a.time:
            h.torch.set_num_threads(1)
            h.log(next(iter(CASES)))              # imports and first-call costs stay off the clock
            best = dict.fromkeys(CASES, float("inf"))     # per case the fastest of the passes: scheduling noise only ever adds time
            for _ in range(a.passes):
                for name in CASES:
                    h.calls, h.repack = [], []
                    t0 = time.perf_counter()
                    h.run(name)
                    best[name] = min(best[name], time.perf_counter() - t0)
            print("%.2f ms for %d cases, each the fastest of %d passes (%s)" % (1e3 * sum(best.values()), len(CASES), a.passes,
                                                                               h.engine.__file__))
            return
        if a.case:
            print(json.dumps(h.log(a.case), indent=1, sort_keys=True))
            return
        fixture, reached = {}, set()
        for name in CASES:
            log = h.log(name)
            fixture[name] = {"entries": lib_entries(log), "sha1": digest(log)}
            reached.update(lib_entries(log))
            print("%-40s %3d library calls, %3d ATen" % (name, len(lib_entries(log)), len(log["calls"]) - len(lib_entries(log))))
        missing = sorted(set(ENTRIES + ENTRIES_BF16S) - reached)
        print("%d cases; entries reached: %s%s" % (len(CASES), " ".join(sorted(e[len("cslgan_"):] for e in reached)),
                                                   "" if not missing else " — MISSING: %s" % missing))
        if a.record:
            with open(a.record, "w") as f:
                json.dump(fixture, f, indent=0, sort_keys=True)
                f.write("\n")
    finally:
        p.undo()


if __name__ == "__main__":
    main()
