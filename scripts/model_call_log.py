"""What does the model layer launch — csl_gan_amd.nn, DCResNet_models, the conv Functions of functional and the normalisation wrappers
of ops — and how does data flow between the launches?  A log taken without a GPU.

The layer is host logic: per normalisation and conv it decides between autograd, the recorder's two-launch form, statistics from a
conv epilogue, the norm as an affine map in the next conv's staging, the fused bn1 / shuffle / shortcut kernel, the per-sample sink
and the fused activation masks.  Here whole models run (generators at B = 8, critics at B = 4) on zero-filled CPU tensors against the
recording stand-in of scripts/conv_dispatch_log.py (imported, not copied) with torch.cuda.current_stream / Stream / stream replaced by
no-ops.  Only public surfaces are driven: the model classes, ops.set_compute_dtype / set_storage_dtype / _GN_FUSE / _GN_SHORTCUT_FUSE,
nn.set_mask_recorder, nn.to_device_layout and the _sink / _bpc attributes the engine and the clipper set.

A case logs, in order,
  * every library call: entry, every scalar, every struct field, and for each pointer where it points: "<module path of a parameter or
    buffer>", "<input name>", else "#n" — the ordinal of the allocation's first appearance in the case's calls.  Every tensor an
    operator returns during a case is kept alive, so no address recurs and the ordinals describe data flow, not allocator luck;
  * every ATen operator in between that is not a view or an allocation, with its shapes; what a per-sample sink was handed;
  * what the call returned (shape, dtype, strides, ordinal) or the type of the exception it raised, and after a backward the shape and
    dtype of every .grad.

    python scripts/model_call_log.py                          # entry counts per case
    python scripts/model_call_log.py --case g64_frozen_fp32
    python scripts/model_call_log.py --time                   # host time of the whole list
    python scripts/model_call_log.py --root ../parent --record tests/model_calls.json

tests/model_calls.json holds, per case, the ordered entry names and a SHA-1 of the canonical JSON of the full log, recorded with --root
pointing at a checkout of the commit BEFORE the layer was rewritten around one route per norm / conv stage; tests/test_model_calls.py
asserts them.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_dispatch_log import ROOT, Harness, Patches, digest      # noqa: E402
from engine_call_log import _NO_LAUNCH, _Stream                   # noqa: E402

BG, BD = 8, 4       # batch of the generator and of the critic cases

# entries the case list must reach (tests/test_model_calls.py): what the frozen fp32 generator runs, then the other routes
ENTRIES = sorted("cslgan_" + n for n in (
    "groupnorm_apply_parts_shortcut_f32", "groupnorm_affine_parts_f32", "groupnorm_act_f32", "conv2d_fwd_x3_f32", "conv2d_fwd_f32",
    "fold_channels4_f32", "groupnorm_act_bf16s", "conv2d_fwd_bf16s", "batchnorm_act_f32", "batchnorm_eval_act_f32", "norm_act_bwd_f32",
    "depth_to_space_f32", "groupnorm_apply_parts_f32", "cast_f32_bf16"))


class _NoStream(_Stream):
    cuda_stream = 0


class _Sink:
    """A recording csl_gan_amd.nn.PerSampleSink: logs what each layer's backward hands to collect()."""
    enabled = True

    def __init__(self, h, names):
        self.h, self.names, self.n = h, names, {}

    def next_pass(self, layer):
        self.n[layer] = self.n.get(layer, 0) + 1
        return self.n[layer] - 1

    def collector(self, layer):
        return _Collector(self, layer)


class _Collector:
    def __init__(self, sink, layer):
        self.sink, self.layer = sink, layer

    def collect(self, pass_idx, gz, x, *geo):
        h = self.sink.h
        if not h.timing:
            h.calls.append({"collect": self.sink.names[self.layer], "pass": pass_idx, "gz": [list(gz.shape), str(gz.dtype), h._where(gz.data_ptr())],
                            "x": [list(x.shape), str(x.dtype), h._where(x.data_ptr())], "geo": list(geo)})


class ModelHarness(Harness):
    def __init__(self, setattr_fn, root=ROOT, timing=False):
        super().__init__(setattr_fn, root=root, timer=False)
        torch = self.torch
        setattr_fn(torch.cuda, "current_stream", lambda *a, **k: _NoStream())
        setattr_fn(torch.cuda, "Stream", _NoStream)
        setattr_fn(torch.cuda, "stream", lambda s: _NoStream())
        from csl_gan_amd import CelebA_models, DCResNet_models, backprop_clip, nn as hnn
        self.hnn, self.zoo, self.dcrn, self.bpc = hnn, CelebA_models, DCResNet_models, backprop_clip
        self.timing = timing      # --time: the clock should see the model layer, so the stand-in library only counts its calls
        self.models, self.inputs, self.n_untraced = {}, {}, 0
        self.held, self.alloc, self.ordinal, self.quiet = [], {}, {}, False
        from torch.utils._python_dispatch import TorchDispatchMode
        h = self

        class AtenLog(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                for t in out if isinstance(out, (tuple, list)) else (out,):
                    if isinstance(t, torch.Tensor):
                        h._hold(t)
                name = str(func)
                if not (h.quiet or getattr(func, "is_view", False) or name in _NO_LAUNCH):
                    h.calls.append({"aten": name, "shapes": [list(a.shape) for a in args if isinstance(a, torch.Tensor)],
                                    "out": list(out.shape) if isinstance(out, torch.Tensor) else None})
                return out

        self._aten_mode = AtenLog

    def __getattr__(self, name):
        if not self.__dict__.get("timing") or name == "cslgan_last_kernel":
            return super().__getattr__(name)
        if not name.startswith("cslgan_"):
            raise AttributeError(name)
        return self._count

    def _count(self, *args):
        self.n_untraced += 1
        return 0

    # -- where a pointer points
    def _hold(self, t):
        st = t.untyped_storage()
        if st.nbytes():
            self.held.append(t)
            self.alloc.setdefault(st.data_ptr(), st.nbytes())

    def _where(self, addr):
        if not addr:
            return "null"
        for lo, hi, name in self.spans:
            if lo <= addr < hi and name != "ws":        # a repack workspace is data like any other: it gets an ordinal
                return name if addr == lo else "%s+%d" % (name, addr - lo)
        base = addr
        if addr not in self.alloc:
            base = next((lo for lo, n in self.alloc.items() if lo <= addr < lo + n), addr)
        n = self.ordinal.setdefault(base, len(self.ordinal))
        return "#%d" % n if addr == base else "#%d+%d" % (n, addr - base)

    def _arg(self, a):
        out = super()._arg(a)
        if isinstance(out, dict):                       # byref(struct): its pointer fields by where they point as well
            for field, v in out.items():
                if v == "set":
                    out[field] = self._where(getattr(a._obj, field))
        return out

    def _span(self, t, name):
        self.spans.append((t.data_ptr(), t.data_ptr() + max(1, t.numel()) * t.element_size(), name))

    # -- models and inputs, made once per harness (only what a case does with them is logged)
    def model(self, key, make):
        m = self.models.get(key)
        if m is None:
            self.quiet = True                 # construction and initialisation are not the layer's work
            m = self.models[key] = self.hnn.to_device_layout(make())
            self.quiet = False
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            t.grad = None
            self._span(t, name)
        return m

    def input(self, name, shape, dtype=None, grad=False):
        torch = self.torch
        t = self.inputs.get((name, shape, dtype, grad))
        if t is None:
            self.quiet = True
            t = self.inputs[(name, shape, dtype, grad)] = torch.zeros(shape, dtype=dtype or torch.float32, requires_grad=grad)
            self.quiet = False
        t.grad = None
        self._span(t, name)
        return t

    def describe(self, r, out=None):
        if isinstance(r, (tuple, list)):
            return [self.describe(e) for e in r]
        if isinstance(r, self.torch.Tensor):
            return {"shape": list(r.shape), "dtype": str(r.dtype), "stride": list(r.stride()), "at": self._where(r.data_ptr())}
        return r

    def grads(self, model, *inputs):
        named = list(model.named_parameters()) + [("input%d" % i, t) for i, t in enumerate(inputs)]
        return {n: None if t.grad is None else [list(t.grad.shape), str(t.grad.dtype)] for n, t in named}

    # -- cases
    def run(self, name):
        """Run one case: ((result, grads) or None, exception or None)."""
        fn, kw = CASES[name]
        ops = self.ops
        self.spans, self.keep, self.held, self.alloc, self.ordinal = [], [], [], {}, {}
        saved = ops._GN_FUSE, ops._GN_SHORTCUT_FUSE
        ops._GN_FUSE, ops._GN_SHORTCUT_FUSE = kw.get("gn_fuse", True), kw.get("sc_fuse", True)
        ops.set_compute_dtype(kw.get("mode", "fp32"))
        ops.set_storage_dtype(kw.get("storage", "fp32"))
        try:
            with contextlib.ExitStack() as stack:
                if not self.timing:
                    stack.enter_context(self._aten_mode())
                try:
                    return fn(self, **{k: v for k, v in kw.items() if k not in ("gn_fuse", "sc_fuse", "mode", "storage")}), None
                except Exception as e:           # noqa: BLE001 — a case may be about the exception
                    return None, e
        finally:
            ops._GN_FUSE, ops._GN_SHORTCUT_FUSE = saved
            ops.set_compute_dtype("fp32")
            ops.set_storage_dtype("fp32")
            self.hnn.set_mask_recorder(None)

    def log(self, name):
        self.calls, self.repack = [], []
        r, err = self.run(name)
        log = {"calls": self.calls, "repack": self.repack, "error": None if err is None else type(err).__name__,
               "result": None if r is None else self.describe(r[0]), "grads": None if r is None else r[1]}
        self.held, self.keep = [], []
        return log


def generator(h, cls="CelebA_DCRN_G64", bn=False, grad=False, eval_mode=False, recorder=False, out=False, n_classes=0):
    torch = h.torch
    G = h.model((cls, bn, n_classes), lambda: getattr(h.zoo, cls)(bn=bn, n_classes=n_classes, emb_mode="concat"))
    G.train(not eval_mode)
    z = h.input("z", (BG, G.z_dim))
    y = h.input("y", (BG,), torch.long) if n_classes > 1 else None
    if recorder:
        h.hnn.set_mask_recorder(h.hnn.ActivationMaskRecorder(G=G))
    if grad:
        img = G(z, y)
        img.sum().backward()
        return img, h.grads(G)
    with torch.no_grad():
        if out:
            side = G.first_filter_size * 2 ** len(G.blocks)
            return G(z, y, out=h.input("out", (BG, side, side, G.out_ch))), None
        return G(z, y), None


def critic(h, sink=False, clipper=False, penalty=False, **kw):
    torch = h.torch
    D = h.model(("CelebA_DCRN_D64", sink, clipper) + tuple(sorted(kw.items())), lambda: h.zoo.CelebA_DCRN_D64(**kw))
    layers = {m: n for n, m in D.named_modules() if isinstance(m, (h.hnn.HipConv2d, h.hnn.HipLinear))}
    if sink:
        s = _Sink(h, layers)
        for m in layers:
            m._sink = s
    if clipper:
        # the real clipper: its probe forward (a zero image, here at the critic's own size) and the per-layer clip it hangs on _bpc
        for m in layers:
            m._bpc = None
        with contextlib.redirect_stdout(io.StringIO()):
            h.bpc.BackpropClipper(D, input_size=(1, 3, 64, 64))
    x = h.input("x", (BD, 3, 64, 64), grad=True)
    y = h.input("y", (BD,), torch.long) if kw.get("n_classes", 0) > 1 else None
    o, aux = D(x, y)
    if penalty:             # the gradient penalty's double backward: Dgrad's and, behind it, Conv's and Wgrad's nodes
        gx, = torch.autograd.grad(o.sum(), x, create_graph=True)
        gx.pow(2).sum().backward()
        return (o, gx), h.grads(D, x)
    (o.sum() if aux is None else o.sum() + aux.sum()).backward()
    return (o, aux), h.grads(D, x)


def nchw(h, what, grad=False):
    """One layer's NCHW entry point alone on a small tensor."""
    torch, hnn = h.torch, h.hnn
    make, shape = {
        "conv2d": (lambda: hnn.HipConv2d(16, 64, 3, padding="same", act=h.ops.ACT_LRELU02), (2, 16, 8, 8)),
        "linear": (lambda: hnn.HipLinear(32, 8), (2, 32)),
        "groupnorm": (lambda: hnn.HipGroupNormAct(32, 64), (2, 64, 8, 8)),
        "upsampleconv": (lambda: h.dcrn.UpsampleConv(64, 64, 3), (2, 64, 8, 8)),
        "resblockup": (lambda: h.dcrn.ResBlockUp(128, 64, 5, bn=False), (2, 128, 8, 8)),
    }[what]
    m = h.model(("nchw", what), make)
    x = h.input("x", shape, grad=grad)
    if grad:
        r = m(x)
        r.sum().backward()
        return r, h.grads(m, x)
    with torch.no_grad():
        return m(x), None


CASES = {}
_G = "CelebA_DCRN_G64"
CASES["g64_frozen_fp32"] = (generator, dict())
CASES["g64_frozen_fp32_auto"] = (generator, dict(mode="fp32_auto"))
CASES["g64_frozen_no_shortcut_fuse"] = (generator, dict(sc_fuse=False))
CASES["g64_frozen_no_gn_fuse"] = (generator, dict(gn_fuse=False))
CASES["g64_frozen_bf16s"] = (generator, dict(storage="bf16"))
CASES["g64_frozen_recorder_fp32"] = (generator, dict(recorder=True))
CASES["g64_frozen_recorder_bf16s"] = (generator, dict(recorder=True, storage="bf16"))
CASES["g64_frozen_out"] = (generator, dict(out=True))
CASES["g64_grad"] = (generator, dict(grad=True))
CASES["g48_frozen_fp32"] = (generator, dict(cls="CelebA_DCRN_G48"))
CASES["g128_frozen_fp32"] = (generator, dict(cls="CelebA_DCRN_G128"))
CASES["g64bn_train_frozen"] = (generator, dict(bn=True))
CASES["g64bn_train_grad"] = (generator, dict(bn=True, grad=True))
CASES["g64bn_eval_frozen"] = (generator, dict(bn=True, eval_mode=True))
CASES["g64bn_eval_grad_error"] = (generator, dict(bn=True, eval_mode=True, grad=True))
CASES["g64bn_recorder"] = (generator, dict(bn=True, recorder=True))
CASES["g64_cond_frozen"] = (generator, dict(n_classes=10))
CASES["d64_grad"] = (critic, dict())
CASES["d64_grad_bf16s"] = (critic, dict(storage="bf16"))
CASES["d64_acgan_grad"] = (critic, dict(n_classes=10, conditional_arch="ACGAN"))
CASES["d64_penalty"] = (critic, dict(penalty=True))
CASES["d64_penalty_bf16s"] = (critic, dict(penalty=True, storage="bf16"))
CASES["d64_sink"] = (critic, dict(sink=True))
CASES["d64_bpc"] = (critic, dict(clipper=True))
for _w in ("conv2d", "linear", "groupnorm", "upsampleconv", "resblockup"):
    CASES["nchw_%s" % _w] = (nchw, dict(what=_w))
    CASES["nchw_%s_grad" % _w] = (nchw, dict(what=_w, grad=True))


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
    h = ModelHarness(p.setattr, root=os.path.abspath(a.root), timing=a.time)
    try:
        if a.time:
            h.torch.set_num_threads(1)
            for name in CASES:                    # imports, model construction and first-call costs stay off the clock
                h.run(name)
            best = dict.fromkeys(CASES, float("inf"))     # per case the fastest of the passes: scheduling noise only ever adds time
            for _ in range(a.passes):
                for name in CASES:
                    t0 = time.perf_counter()
                    h.run(name)
                    best[name] = min(best[name], time.perf_counter() - t0)
            print("%.2f ms for %d cases, each the fastest of %d passes (%s)" % (1e3 * sum(best.values()), len(CASES), a.passes,
                                                                               h.hnn.__file__))
            return
        if a.case:
            print(json.dumps(h.log(a.case), indent=1, sort_keys=True))
            return
        fixture, reached = {}, set()
        for name in CASES:
            log = h.log(name)
            fixture[name] = {"entries": lib_entries(log), "sha1": digest(log)}
            reached.update(lib_entries(log))
            print("%-30s %-20s %3d library calls, %3d other records" % (name, log["error"] or "", len(lib_entries(log)),
                                                                      len(log["calls"]) - len(lib_entries(log))))
        missing = sorted(set(ENTRIES) - reached)
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
