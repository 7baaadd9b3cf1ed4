"""Deep-conv ResNet GAN stacks (reference DCResNet_models.py) on the HIP kernels.

Same class names, constructor arguments, sub-module names (state_dict keys) and construction
order (weights_seed parity) as the reference; device tensors run NHWC through
csl_gan_amd.nn.HipConv2d / HipLinear / HipGroupNormAct.

MI355X-first differences, all exact re-associations of the reference arithmetic:
  * UpsampleConv (DCResNet_models.py:8-17) is cat([x]*4, 1) + pixel_shuffle(2) + conv.  pixel_shuffle is channel-major, so the
    shuffled tensor is up[c,2h+i,2w+j] = x[(4c+2i+j) mod C,h,w]: its C channels are the C/4 channels of the plain depth-to-space
    tensor ps[c',2h+i,2w+j] = x[4c'+2i+j,h,w] repeated four times.  The device path therefore never builds `up`: the
    normalisation kernel writes ps directly and the conv runs on ps with its filter summed over the four channel groups
    (ops.fold_channels4) — a quarter of the reference's multiply-adds for these layers;
  * the 1x1 shortcut's result is added in the epilogue of the block's last conv; in a frozen forward the shortcut itself is
    computed by the kernel that applies bn1 and shuffles (ops.groupnorm_apply_shortcut);
  * bias, LeakyReLU(0.2) / tanh are conv-kernel epilogues; GroupNorm/BatchNorm+ReLU is one op.
"""
import contextlib

import torch
import torch.nn.functional as F
from torch import nn

from . import functional as HF
from . import ops
from . import nn as hnn
from .models import Discriminator, Generator
from .nn import HipConv2d, HipGroupNormAct, HipLinear, _BatchNormAct


class UpsampleConv(nn.Module):
    """cat([x]*4, dim=1) -> pixel_shuffle(2) -> 'same' conv (DCResNet_models.py:8-17)."""

    def __init__(self, in_ch, out_ch, filter_size, bias=True):
        super().__init__()
        self.conv = HipConv2d(in_ch, out_ch, filter_size, padding="same", bias=bias)

    def forward_shuffled(self, x_ps):
        """x_ps: the depth-to-space tensor [N,2H,2W,C/4] (NHWC) of this layer's input."""
        return self.conv.forward_shuffled(x_ps)

    def forward(self, x):
        if x.is_cuda:
            if x.shape[1] % 4:
                raise NotImplementedError("UpsampleConv on HIP needs in_ch %% 4 == 0 (got %d)" % x.shape[1])
            return HF.nchw_view(self.forward_shuffled(HF.DepthToSpace.apply(HF.nhwc(x))))
        return self.conv(F.pixel_shuffle(torch.cat([x, x, x, x], 1), 2))


def _gn_fusable(x):
    """GroupNorm statistics may come from the producing conv's epilogue: a frozen fp32 device forward with no recorder attached."""
    return (not torch.is_grad_enabled()) and x.is_cuda and x.dtype == torch.float32 and not ops.storage_bf16() and hnn._mask_recorder is None


class _NoParts:
    part = None


def _parts_for(fuse, norm):
    """`with _parts_for(fuse, norm) as cell:` around the conv that feeds `norm`: in a frozen forward that conv leaves GroupNorm's
    partial statistics of its output in cell.part (ops.gn_partials); otherwise, and when its route cannot, cell.part is None."""
    return ops.gn_partials(norm.num_groups) if fuse and isinstance(norm, HipGroupNormAct) else contextlib.nullcontext(_NoParts)


def _norm_then_conv(norm, x, part, conv, **conv_kw):
    """conv(act(norm(x))), `conv` being the only consumer.  With statistics of x at hand (part) and a conv route that takes them
    (ops.in_affine_ok), GroupNorm(+ReLU) rides in the conv's staging as per-(image, channel) (scale, shift) tables
    (ops.groupnorm_affine) and conv reads the raw x; else the norm is a launch of its own (on `part`, if there is one)."""
    if part is not None and ops.in_affine_ok(x, conv.weight.permute(0, 2, 3, 1), conv.stride[0], conv.padding[0]):
        N, H, W, C = x.shape
        sc, sh = ops.groupnorm_affine(part, norm.weight.detach(), norm.bias.detach(), norm.num_groups, norm.eps, N, H * W, C)
        return conv.forward_nhwc(x, in_affine=(sc, sh, bool(norm.relu)), **conv_kw)
    return conv.forward_nhwc(norm.forward_nhwc(x, part=part), **conv_kw)


def _norm_act(bn, ch):
    return _BatchNormAct(ch) if bn else HipGroupNormAct(32, ch, relu=True)


class ResBlockUp(nn.Module):
    """DCResNet_models.py:19-38.  Sub-module creation order is part of the weights_seed contract."""

    def __init__(self, in_ch, out_ch, filter_size, bn=True):
        super().__init__()
        self.shortcut = UpsampleConv(in_ch, out_ch, 1)
        self.bn1 = _norm_act(bn, in_ch)
        self.convUp = UpsampleConv(in_ch, out_ch, filter_size, bias=False)
        self.bn2 = _norm_act(bn, out_ch)
        self.conv = HipConv2d(out_ch, out_ch, filter_size, padding="same")

    def forward_nhwc(self, x):
        return self.forward_nhwc_parts(x)[0]

    def forward_nhwc_parts(self, x, x_part=None, next_norm=None):
        """(block output, GroupNorm partial statistics of it for `next_norm` or None).  In a frozen forward (the generator inside a
        D-step) every GroupNorm of the stack reads its statistics from the epilogue of the conv that produced its input
        (ops.gn_partials, cslgan_conv_t.gn_part): x_part are the ones the previous block left for this block's bn1."""
        if x.shape[-1] % 4:
            raise NotImplementedError("ResBlockUp on HIP needs in_ch %% 4 == 0 (got %d)" % x.shape[-1])
        fuse = _gn_fusable(x)
        # 1. bn1 + shortcut.  A frozen forward on the previous block's statistics applies, shuffles and runs the 1x1 shortcut in one
        # launch: the raw shuffled x, which only the shortcut would read, is never written (csrc/gn_shortcut.hip).  Else bn1 writes
        # both shuffled tensors and the shortcut is a 1x1 conv over the C/4 shuffled channels at full resolution
        sc = self.shortcut.conv
        one_launch = (fuse and isinstance(self.bn1, HipGroupNormAct) and sc.kernel_size == (1, 1) and sc.act == ops.ACT_NONE
                      and sc._bpc is None and ops.gn_shortcut_ok(x, sc.out_channels, x_part))
        if one_launch:
            w = sc.weight.permute(0, 2, 3, 1).contiguous()
            a_ps, s = ops.groupnorm_apply_shortcut(x, self.bn1.weight.detach(), self.bn1.bias.detach(), self.bn1.num_groups, x_part,
                                                   ops.fold_channels4(w.detach(), wkey=sc._wkey(w)),
                                                   None if sc.bias is None else sc.bias.detach(), eps=self.bn1.eps, relu=self.bn1.relu)
        else:
            a_ps, x_ps = self.bn1.forward_shuffled(x, part=x_part)
            s = self.shortcut.forward_shuffled(x_ps)
        # 2. convUp, which leaves bn2's statistics
        with _parts_for(fuse, self.bn2) as cell:
            o = self.convUp.forward_shuffled(a_ps)
        # 3. bn2 and the last conv (the shortcut added in its epilogue), which leaves the statistics for the next norm
        with _parts_for(fuse, next_norm) as nxt:
            out = _norm_then_conv(self.bn2, o, cell.part, self.conv, residual=s)
        return out, nxt.part

    def forward(self, x):
        if x.is_cuda:
            return HF.nchw_view(self.forward_nhwc(HF.nhwc(x)))
        return self.conv(self.bn2(self.convUp(self.bn1(x)))) + self.shortcut(x)


class DCResNetGenerator(Generator):
    def __init__(self, channels, first_filter_size, **kwargs):
        super().__init__(**kwargs)
        self.first_filter_size = first_filter_size
        extra = self.n_classes if self.emb_mode == "concat" else 0
        self.linIn = HipLinear(self.z_dim + extra, first_filter_size ** 2 * channels[0])
        self.blocks = nn.ModuleList([ResBlockUp(a, b, 5, bn=self.bn) for a, b in zip(channels[:-1], channels[1:])])
        self.bn = _norm_act(self.bn, channels[-1])
        self.convOut = HipConv2d(channels[-1], self.out_ch, 3, padding="same", act=ops.ACT_TANH)

    def forward(self, z, y=None, out=None):
        """out (frozen device forward only): an NHWC-contiguous [B, H, W, out_ch] fp32 tensor the output conv writes the images
        into — the trainer hands in the generated rows' slice of the fused critic batch, so no copy follows."""
        f = self.first_filter_size
        x = self.linIn(self._condition(z, y)).reshape(z.size(0), -1, f, f)
        if not x.is_cuda:
            for blk in self.blocks:
                x = blk(x)
            return self.convOut(self.bn(x))
        x = HF.nhwc(x)
        part = None
        for i, blk in enumerate(self.blocks):           # each block leaves the statistics the NEXT normalisation needs (frozen forward)
            nxt = self.blocks[i + 1].bn1 if i + 1 < len(self.blocks) else self.bn
            x, part = blk.forward_nhwc_parts(x, part, nxt)
        return HF.nchw_view(_norm_then_conv(self.bn, x, part, self.convOut, out=out))

    def loss(self, d_output, device):
        return -torch.mean(d_output)


class DCResNetDiscriminator(Discriminator):
    linear_critic_losses = True     # real_loss = -mean(out), fake_loss = +mean(out): the trainer may evaluate them with one fused launch

    def __init__(self, channels, last_filter_size, **kwargs):
        super().__init__(**kwargs)
        channels = list(channels)       # the reference mutates its default list (DCResNet_models.py:115); we copy
        if self.emb_mode == "concat" and self.n_classes > 1:
            channels[0] += self.n_classes
        self.blocks = nn.ModuleList([HipConv2d(a, b, 5, stride=2, padding=2, act=ops.ACT_LRELU02)
                                     for a, b in zip(channels[:-1], channels[1:])])
        size = channels[-1] * last_filter_size ** 2
        if self.n_classes < 2 or self.conditional_arch != "WCGAN":
            self.linOut = HipLinear(size, 1, bias=False)
        if self.n_classes > 1 and self.conditional_arch in ("ACGAN", "WCGAN"):
            self.linOutAux = HipLinear(size, self.n_classes, bias=True)

    def forward(self, x, y=None, aux=True):
        B = x.size(0)
        o = x
        if self.emb_mode == "concat" and self.n_classes > 1:
            planes = F.one_hot(y, self.n_classes).to(x.dtype).view(B, -1, 1, 1).expand(-1, -1, x.size(2), x.size(3))
            o = torch.cat((x, planes), dim=1)
        fuse = False
        if o.is_cuda:
            # Activation-backward fusion: every LeakyReLU output of this stack is consumed ONLY by the next conv or by the linear
            # heads, so each consumer applies the producer's slope pattern in the epilogue of its data-gradient kernel and the
            # producer skips its own activation-backward pass (a read + a write of every activation gradient less).  Never with
            # backprop clipping: its input clip sits between the activation and the next conv.
            fuse = all(getattr(m, "_bpc", None) is None for m in self.modules())
            o = HF.nhwc(o)
            prev_lrelu = False
            # --storage_dtype bf16: the conv layers' outputs (and with them their gradients) live in HBM as bfloat16; the heads
            # answer in fp32 (csl_gan_amd.ops.set_storage_dtype)
            od = torch.bfloat16 if ops.storage_bf16() else None
            for blk in self.blocks:
                o = blk.forward_nhwc(o, in_mask=fuse and prev_lrelu, out_masked=fuse, out_dtype=od)   # conv + bias + LeakyReLU(0.2) in one kernel
                prev_lrelu = blk.act == ops.ACT_LRELU02
            fuse = fuse and prev_lrelu
            o = HF.nchw_view(o)
        else:
            for blk in self.blocks:
                o = blk(o)
        o = o.reshape(B, -1)                        # (c,h,w) feature order, as the reference's linOut expects
        head = (lambda lin: lin(o, in_mask=True)) if fuse else (lambda lin: lin(o))
        out_aux = head(self.linOutAux) if aux and hasattr(self, "linOutAux") else None
        if out_aux is not None and self.conditional_arch == "WCGAN":
            out = (out_aux * F.one_hot(y, self.n_classes)).sum(dim=1)
        else:
            out = head(self.linOut)
        return out, out_aux

    def real_loss(self, output, device):
        return -torch.mean(output)

    def fake_loss(self, output, device):
        return torch.mean(output)
