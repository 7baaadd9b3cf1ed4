"""Layer modules that keep torch.nn's parameter names / shapes / default initialisation (so
state_dict keys and weights_seed-initialised values match the reference's nn.Conv2d / nn.Linear /
nn.GroupNorm layers) but run their device math on the HIP kernels.

Device dispatch is explicit, never a fallback: a module whose parameters live on a HIP device always
calls the C-ABI library (and raises if it is missing); a module on the CPU runs the stock torch op —
that mode exists only for BASELINE.json configs[0] ("-gd cpu -dd cpu", plumbing without a GPU).
"""
from __future__ import annotations

import itertools

import torch
import torch.nn.functional as F
from torch import nn

from . import functional as HF
from . import ops


# Cache keys for repacked filters (ops.repack_cache).  id(parameter) is NOT safe: CPython reuses ids and the caching
# allocator reuses addresses, so a model built later in the same process (a test suite, a resumed run) could collide with
# a dead one's entry — same id, same data_ptr, same shape, same version counter, different weights.  A token is never reused.
_tokens = itertools.count(1)


class ActivationMaskRecorder:
    """Parity-test hook: records the sign mask (output > 0) of every fused ReLU / LeakyReLU this package applies, per module
    and in call order, as logical-NCHW bool tensors on the host.  The CPU oracle replays them (oracle.nets.MaskPlayer) so
    gradient tensors can be compared entry by entry without the discontinuity of a unit that sits at zero.  Off (None) in
    every product run; while installed, the fused depth-to-space normalisation takes its two-launch form."""

    def __init__(self, **nets):
        self.names = {id(m): "%s.%s" % (tag, n) for tag, net in nets.items() for n, m in net.named_modules()}
        self.masks = {}

    def record(self, module, y, nhwc=True):
        m = y.detach() > 0
        if nhwc and m.dim() == 4:
            m = m.permute(0, 3, 1, 2)
        self.masks.setdefault(self.names[id(module)], []).append(m.contiguous().cpu())


_mask_recorder = None


def set_mask_recorder(r):
    global _mask_recorder
    _mask_recorder = r


def _record_mask(module, y, act=None, nhwc=True):
    if _mask_recorder is not None and (act is None or act in (ops.ACT_LRELU02, ops.ACT_RELU)):
        _mask_recorder.record(module, y, nhwc)
    return y


class VersionRef:
    """The version counter of a parameter, readable again later: the cache key of a workspace DERIVED from a parameter (the pieces of a
    folded filter) — ops.repack_cache.refresh_pinned() re-reads it to decide whether a pinned workspace must be rebuilt."""

    def __init__(self, p):
        self.p = p

    version = property(lambda self: self.p._version)


class PerSampleSink:
    """Interface the DP engine implements to receive per-sample gradients from a layer's backward."""

    enabled = False

    def next_pass(self, layer) -> int:
        raise NotImplementedError

    def collector(self, layer):
        raise NotImplementedError


class _PerSampleMixin:
    _sink = None  # set by the engine (csl_gan_amd.engine.PrivacyEngine)
    _bpc = None   # set by csl_gan_amd.backprop_clip.BackpropClipper: per-sample input / output-gradient clip of this layer

    def _wkey(self, w):
        # only a zero-copy view of the parameter shares its version counter; a re-laid-out copy must not be cached
        return self._wtoken if w.data_ptr() == self.weight.data_ptr() else None

    def _conv(self, x, w, residual, o):
        """The layer's conv node: ConvPerSample while the engine's sink collects (its backward hands this layer's per-sample
        gradients to the sink; there is no such node with a residual), else Conv."""
        sink = self._sink
        if sink is not None and sink.enabled and torch.is_grad_enabled() and residual is None:
            return HF.ConvPerSample.apply(x, w, self.bias, o._replace(sink=sink.collector(self), pass_idx=sink.next_pass(self)))
        return HF.Conv.apply(x, w, self.bias, residual, o)


def _differentiated(x, *params):
    """Will autograd ask for a backward through an op on x with these parameters?"""
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))


class HipConv2d(nn.Conv2d, _PerSampleMixin):
    """nn.Conv2d (DCResNet_models.py:118, :11, :26, :85) with a fused activation epilogue.

    act: ops.ACT_* applied in the conv kernel's epilogue (D: LeakyReLU 0.2, DCResNet_models.py:132).
    """

    def __init__(self, cin, cout, k, stride=1, padding=0, bias=True, act=ops.ACT_NONE):
        if padding == "same":
            padding = k // 2
        super().__init__(cin, cout, k, stride=stride, padding=padding, bias=bias)
        self.act = act
        self._wtoken = next(_tokens)

    def forward_nhwc(self, x, residual=None, in_mask=False, out_masked=False, out_dtype=None, in_affine=None, out=None):
        """x: NHWC-contiguous device tensor -> NHWC output (+ residual before the activation).
        out_dtype: torch.bfloat16 stores the output as bfloat16 (ops.set_storage_dtype; the model that owns the chain decides);
        None follows x's element type.

        Activation-backward fusion, decided by the MODEL that owns the chain (DCResNetDiscriminator.forward):
          in_mask     x is the LeakyReLU(0.2) output of a layer that was called with out_masked: this layer multiplies the data
                      gradient it sends to x by that slope pattern (recovered from the sign of x) in its kernel's epilogue;
          out_masked  every consumer of this layer's output does so, hence this layer skips its own activation-backward pass."""
        w = self.weight.permute(0, 2, 3, 1).contiguous()
        if in_affine is not None:
            # frozen forward only (ops.in_affine_ok): the producing layer's GroupNorm + ReLU rides in this conv's staging as a
            # per-(image, channel) affine map — x is the RAW conv output and the normalised activation never reaches HBM
            if torch.is_grad_enabled() or self._bpc is not None:
                raise RuntimeError("in_affine is an inference-only fusion")
            return ops.conv2d_fwd(x, w.detach(), None if self.bias is None else self.bias.detach(), stride=self.stride[0], pad=self.padding[0],
                                  residual=residual, act=self.act, wkey=self._wkey(w), in_affine=in_affine, out=out)
        bpc = self._bpc
        if bpc is not None:
            x = bpc.clip_input(x)              # backprop_clip.py:103 (PGCWrapper.forward)
        im, om = bool(in_mask), bool(out_masked) and self.act == ops.ACT_LRELU02
        if (im or om) and bpc is not None:
            raise RuntimeError("activation-backward fusion and backprop clipping cannot be combined on one layer")
        y = self._conv(x, w, residual, HF.ConvOpts(self.stride[0], self.padding[0], self.act, self._wkey(w), bpc=bpc, in_mask=im,
                                                   out_masked=om, out_dtype=out_dtype))
        if _shape_log is not None:
            _shape_log[self] = ((x.shape[3], x.shape[1], x.shape[2]), (y.shape[3], y.shape[1], y.shape[2]))
        return _record_mask(self, y, self.act)

    def forward_shuffled(self, x_ps):
        """UpsampleConv's conv (DCResNet_models.py:16) on the depth-to-space tensor x_ps[N,2H,2W,C/4]: the reference convolves
        four identical channel groups, i.e. x_ps with the filter summed over the groups (a quarter of the MACs)."""
        w = self.weight.permute(0, 2, 3, 1).contiguous()
        if torch.is_grad_enabled() and w.requires_grad:     # not _differentiated: a backward to x alone still reads the cached fold
            wf = HF.FoldChannels4.apply(w)
            return HF.Conv.apply(x_ps, wf, self.bias, None, HF.ConvOpts(1, self.padding[0], self.act, alg_scale=4.0))
        wk = self._wkey(w)
        wf = ops.fold_channels4(w.detach(), wkey=wk)
        # wf is derived from the parameter (its own version counter is always 0, and a later fold may reuse its address): caches
        # downstream of it are keyed on the PARAMETER's version under a token of their own
        return HF.Conv.apply(x_ps, wf, self.bias, None, HF.ConvOpts(1, self.padding[0], self.act, None if wk is None else (wk, "fold4"), 4.0,
                                                                    VersionRef(self.weight)))

    def forward(self, x):
        if not x.is_cuda:
            return _forward_cpu(self, super().forward, x)
        return HF.nchw_view(self.forward_nhwc(HF.nhwc(x)))


_shape_log = None      # {layer: (in_shape, out_shape)} while BackpropClipper probes the model (the NHWC fast path skips module hooks)


def set_shape_log(d):
    global _shape_log
    _shape_log = d


def _forward_cpu(layer, plain_forward, x):
    """CPU plumbing path of a layer: optional backprop-clip of the input and of the pre-activation gradient around the stock op."""
    bpc = layer._bpc
    if bpc is None:
        return _act_cpu(plain_forward(x), layer.act)
    from .backprop_clip import ClipGrad
    return _act_cpu(ClipGrad.apply(plain_forward(bpc.clip_input(x)), bpc), layer.act)


class HipLinear(nn.Linear, _PerSampleMixin):
    """nn.Linear (DCResNet_models.py:77,124,126; MNIST_models.py:14-15,36-39) as a 1x1 conv on the
    MFMA kernel: x[B,in] is the NHWC tensor [B,1,1,in]."""

    def __init__(self, fin, fout, bias=True, act=ops.ACT_NONE):
        super().__init__(fin, fout, bias=bias)
        self.act = act
        self._wtoken = next(_tokens)

    def forward(self, x, in_mask=False):
        """in_mask: see HipConv2d.forward_nhwc."""
        if not x.is_cuda:
            return _forward_cpu(self, super().forward, x)
        B = x.shape[0]
        bpc = self._bpc
        if bpc is not None:
            x = bpc.clip_input(x)
        x4 = x.contiguous().reshape(B, 1, 1, self.in_features)
        w4 = self.weight.reshape(self.out_features, 1, 1, self.in_features)
        y = self._conv(x4, w4, None, HF.ConvOpts(1, 0, self.act, self._wkey(w4), bpc=bpc, in_mask=bool(in_mask) and bpc is None))
        return _record_mask(self, y.reshape(B, self.out_features), self.act)


class HipGroupNormAct(nn.GroupNorm):
    """nn.GroupNorm(32, C) followed by ReLU (DCResNet_models.py:55-57, 63-67, 84, 101-102) as one HIP op on
    NHWC data, forward and backward (cslgan_groupnorm_act_f32 / cslgan_norm_act_bwd_f32)."""

    def __init__(self, groups, channels, relu=True):
        super().__init__(groups, channels)
        self.relu = relu

    def _forward(self, x, d2s, part):
        stored = ops.storage_bf16()     # --storage_dtype bf16: a frozen generator keeps its activations bfloat16 in HBM from here on
        if _differentiated(x, self.weight):
            route = "autograd"          # train_G: stays fp32
        elif d2s and _mask_recorder is not None:
            route = "recorder"          # two launches: the recorder wants the activation before the shuffle
        elif part is not None and not stored and x.dtype == torch.float32:
            route = "parts"             # the statistics the producing conv's epilogue left: the apply launch alone
        else:
            route = "own"               # its own statistics pass
        fused = d2s and route in ("parts", "own")      # the kernel writes the shuffled activation and the shuffled x itself
        raw = x
        if route == "autograd":
            y = HF.NormAct.apply(x, self.weight, self.bias, self.num_groups, self.eps, self.relu, None, None, 0.0)
        else:
            if route == "recorder" and stored and x.dtype == torch.float32:
                raw = ops.cast_bf16(x)  # what the fused kernel writes for the shortcut in the bf16 storage mode
            y = ops.groupnorm_act(x, self.weight.detach(), self.bias.detach(), self.num_groups, eps=self.eps, relu=self.relu, d2s=fused,
                                  want_raw=fused, out_dtype=torch.bfloat16 if stored else None, part=part if route == "parts" else None)
        if fused:
            return y
        if self.relu:
            y = _record_mask(self, y)
        return (HF.DepthToSpace.apply(y), HF.DepthToSpace.apply(raw)) if d2s else y

    def forward_nhwc(self, x, part=None):
        """part: (partials, slots per image) left by the conv that produced x (ops.gn_partials) — inference only."""
        return self._forward(x, False, part)

    def forward_shuffled(self, x, part=None):
        """(depth_to_space(act(norm(x))), depth_to_space(x)) — the inputs of ResBlockUp's convUp and shortcut."""
        return self._forward(x, True, part)

    def forward(self, x):
        if not x.is_cuda:
            y = super().forward(x)
            return F.relu(y) if self.relu else y
        return HF.nchw_view(self.forward_nhwc(HF.nhwc(x)))


class _BatchNormAct(nn.BatchNorm2d):
    """BatchNorm2d + ReLU for the bn=True generator of the non-per-sample modes (init_util.py:46): batch statistics and the
    running-stat update run on cslgan_batchnorm_act_f32, the backward on cslgan_norm_act_bwd_f32; eval mode (running
    statistics: the sampling path train.py:298-308, gensamples.py:26-41) on cslgan_batchnorm_eval_act_f32.
    Same two device methods as HipGroupNormAct; `part` is accepted and ignored (batch statistics span the images)."""

    def _forward(self, x, d2s):
        g, b, diff = self.weight, self.bias, _differentiated(x, self.weight)
        train = self.training or self.running_mean is None
        fused = d2s and not diff and _mask_recorder is None       # else (autograd, parity-test recorder) the shuffles are launches of their own
        if not train:
            if diff:
                raise NotImplementedError("eval-mode BatchNorm on HIP is inference-only (no backward)")
            y = ops.batchnorm_eval_act(x, g.detach(), b.detach(), self.running_mean, self.running_var, eps=self.eps, relu=True,
                                       d2s=fused, want_raw=fused)
        else:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked += 1
            if diff:
                y = HF.NormAct.apply(x, g, b, 0, self.eps, True, self.running_mean, self.running_var, self.momentum)
            else:
                y = ops.batchnorm_act(x, g.detach(), b.detach(), self.running_mean, self.running_var, momentum=self.momentum,
                                      eps=self.eps, relu=True, d2s=fused, want_raw=fused)
        if fused:
            return y
        y = _record_mask(self, y)
        return (HF.DepthToSpace.apply(y), HF.DepthToSpace.apply(x)) if d2s else y

    def forward_nhwc(self, x, part=None):
        return self._forward(x, False)

    def forward_shuffled(self, x, part=None):
        return self._forward(x, True)

    def forward(self, x):
        if x.is_cuda:
            return HF.nchw_view(self.forward_nhwc(HF.nhwc(x)))
        return F.relu(super().forward(x))


def _act_cpu(y, act):
    if act == ops.ACT_LRELU02:
        return F.leaky_relu(y, 0.2)
    if act == ops.ACT_RELU:
        return F.relu(y)
    if act == ops.ACT_TANH:
        return torch.tanh(y)
    return y


def to_device_layout(module: nn.Module) -> nn.Module:
    """After .to(device): keep 4-D conv filters channels-last in HBM (KRSC), so the kernels read them
    in place and per-sample gradients / Adam state share that layout."""
    for m in module.modules():
        if isinstance(m, nn.Conv2d) and m.weight.is_cuda:
            m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    return module
