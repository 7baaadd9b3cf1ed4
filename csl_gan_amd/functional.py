"""Autograd glue over the HIP kernels.  All tensors here are NHWC-contiguous device tensors.

The three conv Functions form a closed set under differentiation, so the WGAN-GP double backward
(gradient_penalty.py:48-54 then train.py:427) runs entirely on the hand-written kernels:

    Conv   (x, w, b) -> y          d/dx = Dgrad(gz, w)       d/dw = Wgrad(gz, x)      d/db = sum(gz)
    Dgrad  (gy, w)   -> gx         d/dgy = Conv(ggx, w)      d/dw = Wgrad(gy, ggx)
    Wgrad  (gy, x)   -> gw         d/dgy = Conv(x, ggw)      d/dx = Dgrad(gy, ggw)

LeakyReLU / ReLU are fused into the forward kernel's epilogue; their backward multiplies by a mask
recovered from the OUTPUT (slope > 0 keeps the sign), so no pre-activation tensor is stored.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch.autograd import Function

from . import ops

_SLOPE = {ops.ACT_LRELU02: 0.2, ops.ACT_RELU: 0.0}

_INPUT_GRADS_ONLY = False


class input_grads_only:
    """Context for forwards whose FIRST-order backward is only ever asked for input gradients — the
    gradient-penalty forward (gradient_penalty.py:46-50): parameters enter the penalty solely through the
    second-order Dgrad nodes, so the first-order weight / bias gradient kernels would be wasted work
    (autograd cannot tell a custom Function which of its outputs the caller requested)."""

    def __enter__(self):
        global _INPUT_GRADS_ONLY
        self._prev, _INPUT_GRADS_ONLY = _INPUT_GRADS_ONLY, True

    def __exit__(self, *a):
        global _INPUT_GRADS_ONLY
        _INPUT_GRADS_ONLY = self._prev


_PS_SINK = None


class per_sample_param_grads:
    """Context for the SECOND-order sweep of a per-sample gradient penalty (train.py:433-450, penalties computed on private
    data): the reference differentiates penalties[i] for every sample i separately (B autograd calls over the whole batch
    graph).  penalties[i] depends on row i alone, so the per-sample parameter gradients are the per-sample (group = 1) weight
    gradients of ONE sweep of sum_i penalties[i]: inside this context every second-order weight-gradient node hands its
    per-sample rows [B, numel(param)] (parameter memory order) to sink(param, rows) and returns no dense gradient."""

    def __init__(self, sink, params):
        self.sink, self.by_ptr = sink, {p.data_ptr(): p for p in params}

    def __enter__(self):
        global _PS_SINK
        self._prev, _PS_SINK = _PS_SINK, self

    def __exit__(self, *a):
        global _PS_SINK
        _PS_SINK = self._prev


def nhwc(x: torch.Tensor) -> torch.Tensor:
    """logical NCHW -> NHWC-contiguous view (copy only if x is not already channels-last)."""
    return x.permute(0, 2, 3, 1).contiguous()


def nchw_view(y: torch.Tensor) -> torch.Tensor:
    """NHWC-contiguous -> logical NCHW view (channels-last strides, no copy)."""
    return y.permute(0, 3, 1, 2)


class ActBwd(Function):
    """out = g * (y > 0 ? 1 : slope).  Linear in g; the mask has zero derivative."""

    @staticmethod
    def forward(ctx, g, y, slope):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y)
        ctx.slope = slope
        return ops.act_bwd(g.contiguous(), y, slope)

    @staticmethod
    def backward(ctx, gg):
        if gg is None:
            return None, None, None
        (y,) = ctx.saved_tensors
        return ActBwd.apply(gg, y, ctx.slope), None, None


class SegmentMeans(Function):
    """vec[s] = scale[s] * sum(x[row block s]), total = sum(vec): the critic's real_loss / fake_loss (DCResNet_models.py:149-153,
    -mean / +mean) over the row blocks of ONE fused pass and their sum, in one launch; the backward writes the (piecewise constant)
    cotangent in one launch (torch: three means, negations, adds, and their mirror image in the backward — ~17 launches)."""

    @staticmethod
    def forward(ctx, x, sizes, scale):
        ctx.set_materialize_grads(False)
        ctx.meta = (tuple(int(n) for n in sizes), tuple(float(c) for c in scale), x.shape)
        return ops.segment_means(x.contiguous().reshape(-1), ctx.meta[0], ctx.meta[1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_vec, g_total):
        if g_vec is None and g_total is None:
            return None, None, None
        sizes, scale, shape = ctx.meta
        dev = (g_vec if g_vec is not None else g_total).device
        g_vec = None if g_vec is None else g_vec.contiguous()
        return ops.segment_means_bwd(g_total, g_vec, sizes, scale, shape, dev), None, None


class LipschitzTerm(Function):
    """coef * phi(||t_b||), phi(n) = (n-1)^2 or max(n-1,0)^2 (gradient_penalty.py:52-54), summed over the batch unless per_sample —
    one launch forward, one backward (torch: norm, sub, clamp, pow, mean, mul, mul and their backward)."""

    @staticmethod
    def forward(ctx, t, one_sided, coef, per_sample):
        t = t.contiguous()
        norm, per, total = ops.lipschitz_term(t, one_sided, coef)
        ctx.cfg = (bool(one_sided), float(coef), bool(per_sample))
        ctx.save_for_backward(t, norm)
        return per if per_sample else total

    @staticmethod
    def backward(ctx, g):
        t, norm = ctx.saved_tensors
        one_sided, coef, per_sample = ctx.cfg
        if torch.is_grad_enabled() and (g.requires_grad or t.requires_grad):
            # differentiable form (immediate sensitivity differentiates the parameter gradients once more): plain torch ops
            n = t.norm(2, dim=1)
            d = (n - 1).clamp(min=0) if one_sided else n - 1
            gb = g if per_sample else g.expand(t.shape[0])
            # a zero row has factor 0, as torch's norm backward gives it (the kernel does the same), not 0 * inf
            f = torch.where(n > 0, gb * coef * 2 * d / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))
            return f.unsqueeze(1) * t, None, None, None
        g = g.contiguous()
        return ops.lipschitz_term_bwd(t, norm, None if per_sample else g, g if per_sample else None, one_sided, coef), None, None, None


class BiasGrad(Function):
    """gb[k] = sum over all pixels/samples of gy[...,k]."""

    @staticmethod
    def forward(ctx, gy):
        ctx.shape, ctx.dtype = gy.shape, gy.dtype
        N = gy.shape[0]
        group = _dense_group(N)
        part = ops.bias_grad_grouped(gy.contiguous(), group=group)
        if part.shape[0] == 1:
            return part[0]
        out = torch.empty(part.shape[1], device=gy.device, dtype=torch.float32)
        ops.sum_rows(part, out)
        return out

    @staticmethod
    def backward(ctx, ggb):
        return ggb.reshape((1,) * (len(ctx.shape) - 1) + (-1,)).expand(ctx.shape).to(ctx.dtype)


def _dense_group(N: int, tiles: int = 1) -> int:
    """Samples per slab for dense (summed) gradients: the largest group that still leaves >= 512
    workgroups (256 CUs x 2), so small layers keep per-sample slabs and big layers write few."""
    for g in (16, 8, 4, 2):
        if N % g == 0 and (N // g) * tiles >= 512:
            return g
    return 1


class ConvOpts(NamedTuple):
    """What Conv, ConvPerSample, Dgrad and Wgrad take besides tensors: one argument, so a new option lengthens no call and no backward."""
    stride: int = 1; pad: int = 0; act: int = ops.ACT_NONE
    wkey: object = None               # the owning layer's cache token (ops.repack_cache)
    alg_scale: float = 1.0; wversion: object = None       # Conv: see ops.conv2d_fwd
    bpc: object = None                # backprop clipping (csl_gan_amd.backprop_clip): per-sample clip of the pre-activation gradient
    in_mask: bool = False; out_masked: bool = False       # fused activation masks (HipConv2d.forward_nhwc)
    out_dtype: Optional[torch.dtype] = None               # of the result; None follows the input (torch.bfloat16: ops.set_storage_dtype)
    sink: object = None; pass_idx: int = 0                # ConvPerSample: the engine's collector of this layer, and which pass this is
    hw: tuple = None; rs: tuple = None                    # Dgrad: (H, W) of the conv's input; Wgrad: (R, S) of its filter


def _preact_grad(gy, y, o, differentiable):
    """gy, the gradient of a conv's activated output y, taken back through the activation and the backprop clip (contiguous).
    differentiable: as autograd nodes (Conv: the double backward runs through them), else on the kernels directly."""
    gz = gy if differentiable else gy.contiguous()
    if o.out_masked:
        pass                # the consumer's data-gradient epilogue already applied this layer's LeakyReLU slope pattern
    elif o.act in _SLOPE:
        # y.detach(): the slope pattern has zero derivative, so the double backward must not see an edge from this node back
        # into the forward graph.  With the edge, autograd.grad(penalty, params) (train.py:427) walked the whole first-order
        # forward again with zero-filled gradients — a wasted data-gradient chain per step (0.53 ms of 13.6 at bs=128).
        gz = ActBwd.apply(gz, y.detach(), _SLOPE[o.act]) if differentiable else ops.act_bwd(gz, y, _SLOPE[o.act])
    elif o.act == ops.ACT_TANH:
        gz = gz * (1 - y * y)
    gz = gz.contiguous()
    return gz if o.bpc is None else o.bpc.clip_grad(gz)


class Conv(Function):
    @staticmethod
    def forward(ctx, x, w, b, residual, o=ConvOpts()):
        y = ops.conv2d_fwd(x, w, b, stride=o.stride, pad=o.pad, residual=residual, act=o.act, wkey=o.wkey, alg_scale=o.alg_scale,
                           wversion=o.wversion, out_dtype=o.out_dtype)
        ctx.set_materialize_grads(False)      # an output nobody differentiates reaches backward as None, not as a zero tensor
        # the owning layer's cache token lets ops reuse repacked filters while the parameter is unchanged; a derived filter
        # (wversion given) must not be cached by the backward, whose caches key on w's own version counter
        ctx.o = o if o.wversion is None else o._replace(wkey=None)
        ctx.input_only = _INPUT_GRADS_ONLY
        ctx.save_for_backward(x, w, y if o.act != ops.ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return None, None, None, None, None
        x, w, y = ctx.saved_tensors
        o = ctx.o
        gz = _preact_grad(gy, y, o, True)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = Dgrad.apply(gz, w, x.detach() if o.in_mask else None, ConvOpts(o.stride, o.pad, wkey=o.wkey, out_dtype=x.dtype, hw=x.shape[1:3]))
        if ctx.needs_input_grad[1] and not ctx.input_only:
            gw = Wgrad.apply(gz, x, ConvOpts(o.stride, o.pad, in_mask=o.in_mask, rs=w.shape[1:3]))
        if ctx.needs_input_grad[2] and not ctx.input_only:
            gb = BiasGrad.apply(gz)
        # the residual is added before the activation (ResBlockUp's "o + s", DCResNet_models.py:38): its gradient is gz
        return gx, gw, gb, (gz if ctx.needs_input_grad[3] else None), None


class DepthToSpace(Function):
    """UpsampleConv's cat([x]*4, 1) + pixel_shuffle(2) (DCResNet_models.py:13-15) reduced to its C/4 distinct channels:
    [N,H,W,C] -> [N,2H,2W,C/4] (ops.depth_to_space).  A permutation: the backward is the inverse map."""

    @staticmethod
    def forward(ctx, x):
        return ops.depth_to_space(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return SpaceToDepth.apply(g)


class SpaceToDepth(Function):
    @staticmethod
    def forward(ctx, g):
        return ops.depth_to_space(g.contiguous(), inverse=True)

    @staticmethod
    def backward(ctx, gg):
        return DepthToSpace.apply(gg)


class FoldChannels4(Function):
    """wf[k,r,s,c'] = sum_q w[k,r,s,c'+q*C/4]: the filter of UpsampleConv's conv as seen by the depth-to-space tensor,
    whose four channel groups are identical.  Linear; the backward copies the folded gradient to the four groups."""

    @staticmethod
    def forward(ctx, w):
        return ops.fold_channels4(w.contiguous())      # never the cached tensor: autograd owns this output

    @staticmethod
    def backward(ctx, gwf):
        return UnfoldChannels4.apply(gwf)


class UnfoldChannels4(Function):
    @staticmethod
    def forward(ctx, gwf):
        return ops.unfold_channels4(gwf.contiguous())

    @staticmethod
    def backward(ctx, ggw):
        return FoldChannels4.apply(ggw)


class NormAct(Function):
    """GroupNorm / BatchNorm (+ReLU) on NHWC data with the HIP forward and backward kernels.
    groups == 0 selects BatchNorm (batch statistics per channel, running stats updated in place)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu, running_mean, running_var, momentum):
        if groups > 0:
            y, stats = ops.groupnorm_act(x, gamma, beta, groups, eps=eps, relu=relu, return_stats=True)
            ctx.rows_per_stat, ctx.groups = x.shape[1] * x.shape[2], groups
        else:
            y, stats = ops.batchnorm_act(x, gamma, beta, running_mean, running_var, momentum=momentum, eps=eps, relu=relu,
                                         return_stats=True)
            ctx.rows_per_stat, ctx.groups = x.numel() // x.shape[-1], x.shape[-1]
        ctx.eps, ctx.relu = eps, relu
        ctx.save_for_backward(x, y, gamma, stats)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, y, gamma, stats = ctx.saved_tensors
        dx, dgamma, dbeta = ops.norm_act_bwd(x, gy.contiguous(), y, gamma, stats, ctx.rows_per_stat, ctx.groups, ctx.eps, ctx.relu)
        return dx, dgamma, dbeta, None, None, None, None, None, None


class Dgrad(Function):
    @staticmethod
    def forward(ctx, gy, w, mask, o):
        """mask (optional, the conv's own input when that is a LeakyReLU(0.2) output): gx *= lrelu'(mask) in the kernel's epilogue."""
        ctx.set_materialize_grads(False)
        ctx.o = o
        ctx.save_for_backward(gy, w, mask)
        return ops.conv2d_dgrad(gy, w, o.hw, stride=o.stride, pad=o.pad, wkey=o.wkey, mask=mask, out_dtype=o.out_dtype)

    @staticmethod
    def backward(ctx, ggx):
        if ggx is None:
            return None, None, None, None
        gy, w, mask = ctx.saved_tensors
        o = ctx.o
        ggx = ggx.contiguous()
        if mask is not None:        # the epilogue's pointwise factor, applied to the incoming cotangent first (it is linear)
            ggx = ActBwd.apply(ggx, mask, 0.2)
        g_gy = g_w = None
        if ctx.needs_input_grad[0]:
            g_gy = Conv.apply(ggx, w, None, None, ConvOpts(o.stride, o.pad, wkey=o.wkey, out_dtype=gy.dtype))
        if ctx.needs_input_grad[1]:
            ps = _PS_SINK
            param = None if ps is None else ps.by_ptr.get(w.data_ptr())
            if param is not None:
                with torch.no_grad():
                    K, R, S, Cc = w.shape
                    rows = ops.conv2d_wgrad_grouped(gy.contiguous(), ggx, R, S, stride=o.stride, pad=o.pad, group=1, alpha=1.0)
                    ps.sink(param, rows.reshape(rows.shape[0], -1))
            else:
                g_w = Wgrad.apply(gy, ggx, ConvOpts(o.stride, o.pad, rs=w.shape[1:3]))
        return g_gy, g_w, None, None


class Wgrad(Function):
    """Dense weight gradient: grouped slabs on the MFMA kernel, then a column sum."""

    @staticmethod
    def forward(ctx, gy, x, o):
        """o.in_mask: x is a LeakyReLU(0.2) output whose producer relies on its consumers to apply the slope pattern
        (fused_act_masks): the gradient this node sends to x (immediate sensitivity differentiates weight gradients with respect
        to the inputs) must carry it too."""
        ctx.set_materialize_grads(False)
        ctx.o = o
        ctx.save_for_backward(gy, x)
        return ops.conv2d_wgrad_dense(gy, x, *o.rs, stride=o.stride, pad=o.pad)

    @staticmethod
    def backward(ctx, ggw):
        if ggw is None:
            return None, None, None
        gy, x = ctx.saved_tensors
        o = ctx.o
        ggw = ggw.contiguous()
        g_gy = g_x = None
        if ctx.needs_input_grad[0]:
            g_gy = Conv.apply(x, ggw, None, None, ConvOpts(o.stride, o.pad, out_dtype=gy.dtype))
        if ctx.needs_input_grad[1]:
            g_x = Dgrad.apply(gy, ggw, x.detach() if o.in_mask else None, ConvOpts(o.stride, o.pad, out_dtype=x.dtype, hw=x.shape[1:3]))
        return g_gy, g_x, None


class ConvPerSample(Function):
    """Forward identical to Conv; backward writes per-sample weight/bias gradients into the engine's
    store (the Opacus-hook replacement, train.py:373,387) and returns only the data gradient."""

    @staticmethod
    def forward(ctx, x, w, b, o):
        stored = x.dtype == torch.bfloat16 or o.out_dtype == torch.bfloat16       # the bf16 filter copy is cached per parameter version
        y = ops.conv2d_fwd(x, w, b, stride=o.stride, pad=o.pad, act=o.act, wkey=o.wkey if stored else None, out_dtype=o.out_dtype)
        ctx.o = o
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w, y if o.act != ops.ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        o = ctx.o
        with torch.no_grad():
            gz = _preact_grad(gy, y, o, False)
            o.sink.collect(o.pass_idx, gz, x, w.shape[1], w.shape[2], o.stride, o.pad, ctx.has_bias)
            gx = None
            if ctx.needs_input_grad[0]:
                gx = ops.conv2d_dgrad(gz, w, (x.shape[1], x.shape[2]), stride=o.stride, pad=o.pad, wkey=o.wkey,
                                      mask=x if o.in_mask else None, out_dtype=x.dtype)
        return gx, None, None, None


class RowL2Norm(Function):
    """norms[b] = ||t[b,:]||_2 (gradient_penalty.py:52-53) with a differentiable backward."""

    @staticmethod
    def forward(ctx, t):
        t = t.contiguous()
        n = ops.row_l2norm(t)
        ctx.save_for_backward(t, n)
        return n

    @staticmethod
    def backward(ctx, gn):
        t, n = ctx.saved_tensors
        if torch.is_grad_enabled() and (gn.requires_grad or t.requires_grad):
            # differentiable form for higher-order use (never hit by the D-step: the norm's backward is
            # the last first-order node before the parameter gradients)
            # a zero row divides by 1 and stays 0, as torch's norm backward leaves it (the kernel does the same), not 0 / 0
            return gn.unsqueeze(1) * t / torch.where(n > 0, n, torch.ones_like(n)).unsqueeze(1)
        return ops.row_l2norm_bwd(t, n, gn.contiguous())
