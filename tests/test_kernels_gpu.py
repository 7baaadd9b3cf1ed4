"""Kernel-level parity (-m gpu): every C-ABI entry point against a plain PyTorch fp32 CPU reference
of the same op.  Tolerance: 1e-4 relative to the output scale (fp32 MFMA is an exact fmaf chain; only
summation order differs), well inside the 1e-3 the north star asks for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

def _case_seed(case):
    """Deterministic per-case seed (crc32 of the case's repr): a red case can be replayed — hash() of a tuple holding None is
    address-based on Python 3.10 and differs between processes."""
    import zlib
    return zlib.crc32(repr(case).encode()) % 100000


pytestmark = pytest.mark.gpu


def _ops():
    from csl_gan_amd import ops
    return ops


def _dev(t):
    return t.cuda().contiguous()


def _nhwc(t):  # NCHW cpu -> NHWC device
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _krsc(w):  # [K,C,R,S] cpu -> [K,R,S,C] device
    return w.permute(0, 2, 3, 1).contiguous().cuda()


def _close(got, exp, rtol=1e-4, what=""):
    got = got.detach().cpu().double()
    exp = exp.detach().cpu().double()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    scale = exp.abs().max().item() + 1e-12
    err = (got - exp).abs().max().item()
    assert err <= rtol * scale, "%s: max abs err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale)


FWD_CASES = [
    # N, H, W, C, K, R, stride, pad, bias, act, UpsampleConv form (depth-to-space + folded filter), residual (0/1 = yes, None = no)
    (2, 8, 8, 8, 16, 5, 2, 2, True, 1, False, None),
    (3, 16, 16, 3, 64, 5, 2, 2, True, 1, False, None),
    (2, 8, 8, 64, 128, 5, 2, 2, True, 0, False, None),
    (4, 64, 64, 8, 160, 5, 1, 2, False, 2, False, None),
    (2, 4, 4, 32, 32, 5, 1, 2, False, 0, True, None),
    (3, 8, 8, 16, 24, 5, 1, 2, True, 2, True, 1),
    (2, 5, 7, 12, 20, 3, 1, 1, True, 0, True, None),
    (2, 4, 4, 512, 512, 5, 1, 2, False, 0, True, None),
    (16, 8, 8, 256, 512, 5, 2, 2, True, 1, False, None),
    (128, 1, 1, 8192, 1, 1, 1, 0, False, 0, False, None),
    (128, 1, 1, 8192, 1, 1, 1, 0, True, 0, False, None),
    (130, 1, 1, 8192, 1, 1, 1, 0, True, 1, False, 0),          # linear_k1 stream kernel with residual + LeakyReLU
    (7, 1, 1, 512, 1, 1, 1, 0, False, 3, False, None),
    (3, 1, 1, 1000, 10, 1, 1, 0, True, 0, False, None),
    (2, 8, 8, 32, 48, 5, 1, 2, True, 0, False, 1),
    # shapes that take the LDS-halo kernel (stride 1, C % 32 == 0, 8x8-patchable grid, K >= 64)
    (2, 16, 16, 64, 128, 5, 1, 2, True, 1, False, None),
    (3, 8, 8, 32, 64, 3, 1, 1, True, 0, False, None),
    (2, 8, 8, 64, 128, 5, 1, 2, False, 0, True, None),
    (2, 8, 8, 64, 192, 5, 1, 2, True, 2, True, 1),
    (3, 16, 24, 96, 80, 5, 1, 2, True, 0, False, 0),
    (2, 32, 32, 128, 128, 5, 1, 2, True, 0, False, None),
    (2, 8, 8, 32, 48, 1, 1, 0, True, 0, False, 0),
    # 1x1 stream kernel (csrc/conv1x1.hip): 32 / 64 / 128 input channels, a ragged last row tile, residual + activation
    (70, 32, 32, 32, 64, 1, 1, 0, True, 0, False, None),
    (47, 40, 36, 64, 128, 1, 1, 0, True, 1, False, None),         # 67680 rows: a ragged last row tile
    (3, 40, 36, 64, 128, 1, 1, 0, True, 1, False, 0),              # with a residual: the generic kernel
    (7, 1, 1, 794, 128, 1, 1, 0, True, 2, False, None),
    (5, 1, 1, 128, 1, 1, 1, 0, True, 0, False, None),
    (2, 16, 16, 64, 3, 3, 1, 1, True, 3, False, None),
    (2, 7, 7, 12, 20, 5, 2, 2, True, 1, False, None),
    (1, 6, 6, 5, 7, 3, 1, 1, False, 0, False, None),
    # stride 2 through the halo kernel (>= 512 tiles): four parity sub-images accumulated in one workgroup
    (64, 32, 32, 32, 64, 5, 2, 2, True, 0, False, None),
    (72, 32, 32, 64, 128, 5, 2, 2, True, 1, False, None),
    (16, 32, 64, 96, 288, 5, 2, 2, True, 3, False, None),
    (2048, 8, 8, 32, 128, 5, 2, 2, False, 1, False, None),    # 4x4 outputs: four-image patches
    # stride 2, too few tiles for it: generic kernel through the same entry
    (2, 16, 16, 64, 128, 5, 2, 2, True, 1, False, None),
    # 4x4 grids with N % 4 == 0: halo kernel, four images per 64-row patch
    (4, 4, 4, 64, 128, 5, 1, 2, True, 2, True, 1),
    (8, 4, 4, 96, 64, 3, 1, 1, True, 0, False, None),
    # 1..4 output channels from 64 input channels: the vector-ALU kernel (igemm_skinny)
    (2, 8, 8, 64, 1, 3, 1, 1, False, 0, False, None),
    (3, 16, 8, 64, 2, 3, 1, 1, True, 1, False, 0),
    (2, 8, 16, 64, 4, 3, 1, 1, True, 2, False, None),
    (5, 64, 64, 64, 3, 3, 1, 1, True, 3, False, None),
    # the critic's RGB first layer on unpadded 12-byte pixels (csrc/conv_c3.hip): 8x16-pixel tiles
    (5, 64, 64, 3, 64, 5, 2, 2, True, 1, False, None),
    (3, 32, 32, 3, 64, 5, 2, 2, False, 0, False, None),
    (2, 128, 128, 3, 64, 5, 2, 2, True, 1, False, None),
    (2, 16, 96, 3, 64, 5, 2, 2, True, 2, False, None),
    (260, 32, 32, 3, 64, 5, 2, 2, True, 1, False, None),      # more tiles than the persistent grid
]


@pytest.mark.parametrize("case", FWD_CASES)
def test_conv2d_fwd(case):
    ops = _ops()
    N, H, W, C, K, R, s, p, has_b, act, ups, res = case
    g = torch.Generator().manual_seed(_case_seed(case))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g) if has_b else None
    # the reference's UpsampleConv (DCResNet_models.py:13-16), literally
    xin = F.pixel_shuffle(torch.cat([x, x, x, x], 1), 2) if ups else x
    ref = F.conv2d(xin, w, b, stride=s, padding=p)
    resid = None
    if res is not None:
        rs = torch.randn(ref.shape, generator=g)
        ref = ref + rs
        resid = _nhwc(rs)
    if act == 1:
        ref = F.leaky_relu(ref, 0.2)
    elif act == 2:
        ref = F.relu(ref)
    elif act == 3:
        ref = torch.tanh(ref)
    xd, wd = _nhwc(x), _krsc(w)
    if ups:
        xd, wd = ops.depth_to_space(xd), ops.fold_channels4(wd)
        assert xd.shape == (N, 2 * H, 2 * W, C // 4) and wd.shape == (K, R, R, C // 4)
    y = ops.conv2d_fwd(xd, wd, None if b is None else b.cuda(), stride=s, pad=p, residual=resid, act=act)
    _close(y.permute(0, 3, 1, 2), ref, what="fwd %s" % (case,))


@pytest.mark.parametrize("N,H,W,C", [(2, 3, 5, 8), (3, 4, 4, 512), (1, 7, 7, 128), (2, 1, 1, 4), (5, 8, 8, 64)])
def test_depth_to_space_and_channel_fold(N, H, W, C):
    """cslgan_depth_to_space_f32 / cslgan_fold_channels4_f32 against the reference's own ops: the C channels of
    pixel_shuffle(cat([x]*4, 1), 2) (DCResNet_models.py:14-15) are the C/4 channels of depth_to_space(x), four times."""
    ops = _ops()
    g = torch.Generator().manual_seed(N * 1000 + C)
    x = torch.randn(N, C, H, W, generator=g)
    up = F.pixel_shuffle(torch.cat([x, x, x, x], 1), 2)                    # [N, C, 2H, 2W]
    ps = ops.depth_to_space(_nhwc(x))
    for q in range(4):
        assert torch.equal(ps.permute(0, 3, 1, 2).cpu(), up[:, q * (C // 4):(q + 1) * (C // 4)])
    assert torch.equal(ops.depth_to_space(ps, inverse=True).cpu(), x.permute(0, 2, 3, 1))
    w = torch.randn(6, C, 3, 3, generator=g)
    wf = ops.fold_channels4(_krsc(w))
    _close(wf.permute(0, 3, 1, 2), w.view(6, 4, C // 4, 3, 3).sum(1), rtol=1e-6, what="fold4")
    gw = ops.unfold_channels4(wf)
    assert torch.equal(gw.cpu(), wf.cpu().repeat(1, 1, 1, 4))
    with pytest.raises(RuntimeError):
        ops.depth_to_space(torch.zeros(1, 2, 2, 6, device="cuda"))


DGRAD_CASES = [
    # N, H, W, C, K, R, stride, pad, mask
    (2, 8, 8, 8, 16, 5, 2, 2, False),
    (3, 16, 16, 3, 64, 5, 2, 2, True),
    (2, 8, 8, 64, 128, 5, 2, 2, True),
    (2, 7, 9, 12, 20, 5, 2, 2, False),
    (2, 8, 8, 16, 24, 3, 1, 1, False),
    (6, 1, 1, 794, 128, 1, 1, 0, False),
    (2, 32, 32, 64, 128, 5, 2, 2, True),
    (3, 16, 16, 128, 64, 5, 2, 2, False),
    (2, 16, 16, 64, 96, 3, 1, 1, True),
    (2, 32, 32, 64, 256, 5, 2, 2, True),
    # 4x4 parity-class grids (halo kernel, four images per patch; classes paired 9+4 / 6+6 taps)
    (4, 8, 8, 64, 128, 5, 2, 2, True),
    (8, 8, 8, 256, 512, 5, 2, 2, False),
    (12, 8, 8, 128, 96, 5, 2, 2, True),
    # data gradients with 1..4 input channels and 64 output channels (igemm_skinny)
    (2, 32, 32, 4, 64, 5, 2, 2, False),
    (2, 16, 16, 1, 64, 5, 2, 2, True),
    (2, 8, 8, 2, 64, 3, 1, 1, False),
    (4, 64, 64, 3, 64, 5, 2, 2, False),
    (6, 1, 1, 8192, 1, 1, 1, 0, True),        # the critic's head: gx[n,:] = gy[n] * w (linear_k1 stream kernel), with a mask
    (130, 1, 1, 512, 1, 1, 1, 0, False),
]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_conv2d_dgrad(case):
    ops = _ops()
    N, H, W, C, K, R, s, p, use_mask = case
    g = torch.Generator().manual_seed(_case_seed(case))
    x = torch.randn(N, C, H, W, generator=g, requires_grad=True)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    y = F.conv2d(x, w, None, stride=s, padding=p)
    gy = torch.randn(y.shape, generator=g)
    ref, = torch.autograd.grad(y, x, gy)
    mask = None
    if use_mask:
        m = torch.randn(N, C, H, W, generator=g)
        ref = ref * torch.where(m > 0, 1.0, 0.2)
        mask = _nhwc(m)
    gx = ops.conv2d_dgrad(_nhwc(gy), _krsc(w), (H, W), stride=s, pad=p, mask=mask)
    _close(gx.permute(0, 3, 1, 2), ref, what="dgrad %s" % (case,))


WGRAD_CASES = [
    # N, H, W, C, K, R, stride, pad
    (4, 8, 8, 8, 16, 5, 2, 2),
    (4, 16, 16, 3, 64, 5, 2, 2),
    (4, 8, 8, 64, 128, 5, 2, 2),
    (2, 7, 9, 12, 20, 5, 2, 2),
    (6, 1, 1, 794, 128, 1, 1, 0),
    (6, 1, 1, 128, 1, 1, 1, 0),
    (6, 1, 1, 128, 10, 1, 1, 0),
    (2, 64, 64, 3, 64, 5, 2, 2),
    (2, 8, 8, 256, 512, 5, 2, 2),
    # 8x8-patchable outputs, K % 128 == 0, C % 64 == 0: LDS-resident weight-gradient kernel (igemm_wgh)
    (4, 16, 16, 64, 128, 5, 2, 2),
    (2, 32, 32, 64, 128, 5, 2, 2),
    (4, 8, 8, 128, 256, 5, 1, 2),
    (2, 16, 24, 64, 128, 3, 1, 1),
    (6, 16, 16, 128, 128, 5, 2, 2),
    (4, 16, 16, 64, 64, 5, 1, 2),       # 64-channel m tiles
    (2, 16, 16, 128, 192, 3, 2, 1),
    # the critic's RGB first layer (csrc/conv_c3.hip): strips of 8 / 4 / 2 output rows
    (6, 32, 32, 3, 64, 5, 2, 2),
    (4, 64, 64, 3, 64, 5, 2, 2),
    (2, 128, 128, 3, 64, 5, 2, 2),
    (2, 48, 64, 3, 64, 5, 2, 2),
]


@pytest.mark.parametrize("case", WGRAD_CASES)
@pytest.mark.parametrize("group", [1, 2, 0])
def test_conv2d_wgrad_grouped(case, group):
    ops = _ops()
    N, H, W, C, K, R, s, p = case
    group = N if group == 0 else group
    g = torch.Generator().manual_seed(_case_seed(case))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.zeros(K, C, R, R, requires_grad=True)
    alpha = 1.7
    gy_shape = F.conv2d(x, w, None, stride=s, padding=p).shape
    gy = torch.randn(gy_shape, generator=g)
    refs = []
    for gi in range(N // group):
        sl = slice(gi * group, (gi + 1) * group)
        y = F.conv2d(x[sl], w, None, stride=s, padding=p)
        gw, = torch.autograd.grad(y, w, gy[sl])
        refs.append(alpha * gw)
    ref = torch.stack(refs)                       # [G,K,C,R,S]
    sq = torch.zeros(N // group, device="cuda")
    gw = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=group, alpha=alpha, sq=sq)
    _close(gw.permute(0, 1, 4, 2, 3), ref, what="wgrad %s g=%d" % (case, group))
    _close(sq, ref.reshape(ref.shape[0], -1).pow(2).sum(1), rtol=2e-4, what="wgrad sq")
    # norms-only ("ghost") mode
    sq2 = torch.zeros(N // group, device="cuda")
    assert ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=group, alpha=alpha, want_gw=False, sq=sq2) is None
    _close(sq2, sq, rtol=1e-5, what="ghost sq")
    # bias gradient
    sqb = torch.zeros(N // group, device="cuda")
    gb = ops.bias_grad_grouped(_nhwc(gy), group=group, alpha=alpha, sq=sqb)
    refb = alpha * gy.reshape(N // group, group, K, -1).sum((1, 3))
    _close(gb, refb, what="bias grad")
    _close(sqb, refb.pow(2).sum(1), rtol=2e-4, what="bias sq")


def _rand_mats(rows, lens, g):
    return [torch.randn(rows, L, generator=g) * (1 + i) for i, L in enumerate(lens)]


@pytest.mark.parametrize("rows,lens", [(6, [4800, 64, 7, 204800, 1, 33]), (3, [8192 * 2 + 5]), (1, [16]),
                                       (5, [10] * 18)])
def test_sample_sqnorm(rows, lens):
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    mats = _rand_mats(rows, lens, g)
    sq = ops.sample_sqnorm([_dev(m) for m in mats])
    ref = torch.stack([m.double().pow(2).sum(1) for m in mats]).float()
    _close(sq, ref, rtol=2e-5, what="sqnorm")


@pytest.mark.parametrize("flat", [True, False])
def test_clip_factors_and_accum(flat):
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    rows, lens = 8, [4800, 64, 1031, 3]
    mats = _rand_mats(rows, lens, g)
    dm = [_dev(m) for m in mats]
    sq = ops.sample_sqnorm(dm)
    first_private = 4
    if flat:
        Cn = torch.tensor([30.0])
        norms = torch.sqrt(sum(m.pow(2).sum(1) for m in mats))
        f_ref = (Cn / (norms + 1e-6)).clamp(max=1.0)
        f_ref[:first_private] = 1.0
    else:
        Cn = torch.tensor([20.0, 5.0, 50.0, 1.0])
        norms = torch.stack([m.norm(dim=1) for m in mats])
        f_ref = (Cn[:, None] / (norms + 1e-6)).clamp(max=1.0)
        f_ref[:, :first_private] = 1.0
    f, nrm = ops.clip_factors(sq, Cn.cuda(), flat, first_private_row=first_private, want_norms=True)
    _close(f, f_ref, what="factors")
    _close(nrm, norms, what="norms")
    noises = [torch.randn(L, generator=g) for L in lens]
    std = torch.tensor([0.5, 1.0, 2.0, 0.25])
    outs = [torch.full((L,), 3.0, device="cuda") for L in lens]
    ops.clip_accum_noise(dm, outs, factors=f, noise_std=std.cuda(), noises=[_dev(z) for z in noises], scale=0.125, beta=0.5)
    for i, m in enumerate(mats):
        fr = f_ref if flat else f_ref[i]
        ref = 0.5 * 3.0 + 0.125 * ((m * fr[:, None]).sum(0) + std[i] * noises[i])
        _close(outs[i], ref, what="clip_accum seg %d" % i)
    # no factors, no noise, beta 0: plain column sum
    outs2 = [torch.empty(L, device="cuda") for L in lens]
    ops.clip_accum_noise(dm, outs2)
    for i, m in enumerate(mats):
        _close(outs2[i], m.sum(0), what="colsum %d" % i)


def test_philox_noise_statistics():
    ops = _ops()
    L = 1 << 20
    z = [torch.zeros(1, L, device="cuda")]
    std = torch.tensor([2.0], device="cuda")
    o1 = [torch.empty(L, device="cuda")]
    o2 = [torch.empty(L, device="cuda")]
    o3 = [torch.empty(L, device="cuda")]
    ops.clip_accum_noise(z, o1, noise_std=std, seed=123, offset=0)
    ops.clip_accum_noise(z, o2, noise_std=std, seed=123, offset=0)
    ops.clip_accum_noise(z, o3, noise_std=std, seed=123, offset=1)
    a, b, c = o1[0].cpu(), o2[0].cpu(), o3[0].cpu()
    assert torch.equal(a, b)                      # counter-based: reproducible
    assert (a != c).float().mean() > 0.99         # new offset -> new stream
    assert abs(a.mean().item()) < 0.01 and abs(a.std().item() - 2.0) < 0.01
    assert abs((a[:-1] * a[1:]).mean().item()) < 0.02
    k = ((a / 2.0) ** 4).mean().item()
    assert abs(k - 3.0) < 0.05                    # gaussian kurtosis


def test_l2_clip_rows_and_row_norm():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    t = torch.randn(9, 3, 10, 10, generator=g) * torch.linspace(0.1, 3, 9).view(-1, 1, 1, 1)
    Cn = 12.0
    n = t.reshape(9, -1).norm(dim=1)
    ref = torch.where((n > Cn).view(-1, 1, 1, 1), Cn * t / n.view(-1, 1, 1, 1), t)
    _close(ops.l2_clip_rows(_dev(t), Cn), ref, what="l2_clip")
    flat = t.reshape(9, -1)
    _close(ops.row_l2norm(_dev(flat)), n, what="row norm")
    gn = torch.randn(9, generator=g)
    _close(ops.row_l2norm_bwd(_dev(flat), _dev(n), _dev(gn)), gn[:, None] * flat / n[:, None], what="row norm bwd")


def test_act_bwd_groupnorm_adam():
    ops = _ops()
    g = torch.Generator().manual_seed(4)
    gg, y = torch.randn(1000003, generator=g), torch.randn(1000003, generator=g)
    _close(ops.act_bwd(_dev(gg), _dev(y), 0.2), torch.where(y > 0, gg, 0.2 * gg), what="act_bwd")
    for (N, H, C) in ((3, 8, 64), (2, 4, 512), (2, 16, 128), (2, 3, 96)):
        x = torch.randn(N, C, H, H, generator=g) * 2 + 0.5
        gn = torch.nn.GroupNorm(32, C)
        with torch.no_grad():
            gn.weight.copy_(torch.randn(C, generator=g)); gn.bias.copy_(torch.randn(C, generator=g))
            ref = F.relu(gn(x))
        out = ops.groupnorm_act(_nhwc(x), _dev(gn.weight.detach()), _dev(gn.bias.detach()), 32, eps=gn.eps, relu=True)
        _close(out.permute(0, 3, 1, 2), ref, what="groupnorm %s" % ((N, H, C),))
    for (N, H, C) in ((4, 8, 64), (3, 5, 12), (2, 16, 512)):
        x = torch.randn(N, C, H, H, generator=g) * 1.5 - 0.3
        bn = torch.nn.BatchNorm2d(C)
        with torch.no_grad():
            bn.weight.copy_(torch.randn(C, generator=g)); bn.bias.copy_(torch.randn(C, generator=g))
            bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        rm, rv = bn.running_mean.clone().cuda(), bn.running_var.clone().cuda()
        bn.train()
        with torch.no_grad():
            ref = F.relu(bn(x))
        out = ops.batchnorm_act(_nhwc(x), _dev(bn.weight.detach()), _dev(bn.bias.detach()), rm, rv, momentum=bn.momentum, eps=bn.eps)
        _close(out.permute(0, 3, 1, 2), ref, what="batchnorm %s" % ((N, H, C),))
        _close(rm, bn.running_mean, what="bn running mean")
        _close(rv, bn.running_var, what="bn running var")
    p = torch.randn(5000, generator=g)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3, betas=(0.0, 0.9), weight_decay=0.01)
    dp, m, v = _dev(p), torch.zeros(5000, device="cuda"), torch.zeros(5000, device="cuda")
    for step in range(1, 4):
        gr = torch.randn(5000, generator=g)
        pr.grad = gr.clone()
        opt.step()
        ops.adam_step(dp, _dev(gr), m, v, 1e-3, 0.0, 0.9, 1e-8, 0.01, step)
    _close(dp, pr, rtol=1e-5, what="adam")


@pytest.mark.parametrize("case", [(2, 4, 4, 32, 48, 5, True), (3, 5, 7, 12, 20, 3, False), (2, 8, 8, 64, 64, 5, False), (1, 3, 3, 8, 8, 1, True),
                                  (2, 4, 4, 128, 64, 5, False), (3, 8, 8, 256, 160, 5, False), (2, 5, 3, 256, 36, 5, False)])
def test_upsample_conv_module_forward_backward(case):
    """csl_gan_amd.DCResNet_models.UpsampleConv on the device (depth-to-space + channel-folded filter, autograd through
    DepthToSpace / FoldChannels4 / Conv) against the reference's op written out literally (DCResNet_models.py:8-17):
    output, data gradient, weight gradient (all four channel groups) and bias gradient."""
    from csl_gan_amd import nn as hnn
    from csl_gan_amd.DCResNet_models import UpsampleConv
    N, H, W, C, K, R, has_b = case
    torch.manual_seed(sum(case[:6]))
    m = hnn.to_device_layout(UpsampleConv(C, K, R, bias=has_b).cuda())
    g = torch.Generator().manual_seed(sum(case[:6]))
    x = torch.randn(N, C, H, W, generator=g, requires_grad=True)
    w = m.conv.weight.detach().cpu().contiguous().requires_grad_(True)
    b = m.conv.bias.detach().cpu().requires_grad_(True) if has_b else None
    y = F.conv2d(F.pixel_shuffle(torch.cat([x, x, x, x], 1), 2), w, b, padding=R // 2)
    gy = torch.randn(y.shape, generator=g)
    refs = torch.autograd.grad(y, (x, w) + ((b,) if has_b else ()), gy)
    xd = x.detach().cuda().requires_grad_(True)
    yd = m(xd)
    _close(yd, y, what="UpsampleConv fwd %s" % (case,))
    got = torch.autograd.grad(yd, (xd, m.conv.weight) + ((m.conv.bias,) if has_b else ()), gy.cuda())
    _close(got[0], refs[0], what="UpsampleConv dgrad %s" % (case,))
    _close(got[1], refs[1], what="UpsampleConv wgrad %s" % (case,))
    if has_b:
        _close(got[2], refs[2], what="UpsampleConv bgrad %s" % (case,))
    with torch.no_grad():                    # the cached-fold inference path gives the same output
        _close(m(x.detach().cuda()), y, what="UpsampleConv fwd (no_grad) %s" % (case,))


@pytest.mark.parametrize("kind,N,H,W,C", [("gn", 3, 8, 8, 64), ("gn", 2, 4, 6, 512), ("gn", 2, 3, 5, 96), ("bn", 4, 8, 8, 64), ("bn", 3, 5, 4, 12),
                                          ("bn_eval", 3, 4, 4, 128), ("bn_eval", 2, 7, 7, 20)])
def test_norm_act_depth_to_space_output(kind, N, H, W, C):
    """The normalisation kernels' fused depth-to-space output (y and the raw x in the [N,2H,2W,C/4] layout) equals
    depth_to_space of the plain output; eval-mode BatchNorm uses the running statistics."""
    ops = _ops()
    g = torch.Generator().manual_seed(N * 100 + C)
    x = torch.randn(N, C, H, W, generator=g) * 1.5 + 0.2
    m = torch.nn.GroupNorm(32 if C % 32 == 0 else 4, C) if kind == "gn" else torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        m.weight.copy_(torch.randn(C, generator=g)); m.bias.copy_(torch.randn(C, generator=g) * 0.5)
        if kind != "gn":
            m.running_mean.copy_(torch.randn(C, generator=g)); m.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        m.train(kind != "bn_eval")
        ref = F.relu(m(x))
    xn, gam, bet = _nhwc(x), _dev(m.weight.detach()), _dev(m.bias.detach())
    if kind == "gn":
        plain = ops.groupnorm_act(xn, gam, bet, m.num_groups, eps=m.eps, relu=True)
        ys, xs = ops.groupnorm_act(xn, gam, bet, m.num_groups, eps=m.eps, relu=True, d2s=True, want_raw=True)
    elif kind == "bn":
        plain = ops.batchnorm_act(xn, gam, bet, None, None, eps=m.eps, relu=True)
        ys, xs = ops.batchnorm_act(xn, gam, bet, None, None, eps=m.eps, relu=True, d2s=True, want_raw=True)
    else:
        rm, rv = _dev(m.running_mean), _dev(m.running_var)
        plain = ops.batchnorm_eval_act(xn, gam, bet, rm, rv, eps=m.eps, relu=True)
        ys, xs = ops.batchnorm_eval_act(xn, gam, bet, rm, rv, eps=m.eps, relu=True, d2s=True, want_raw=True)
    _close(plain.permute(0, 3, 1, 2), ref, what="%s plain" % kind)
    # (the statistics are reduced with float atomics: two launches agree to rounding, not bit for bit)
    _close(ys, ops.depth_to_space(plain), rtol=1e-5, what="%s fused vs separate shuffle" % kind)
    assert torch.equal(xs, ops.depth_to_space(xn))
    up = F.pixel_shuffle(torch.cat([ref] * 4, 1), 2)[:, :C // 4]            # the reference's shuffle of the reference's output
    _close(ys.permute(0, 3, 1, 2), up, what="%s shuffled" % kind)


@pytest.mark.parametrize("kind,N,H,C", [("gn", 3, 8, 64), ("gn", 2, 4, 512), ("gn", 2, 3, 96), ("bn", 4, 8, 64), ("bn", 3, 5, 12)])
def test_norm_act_backward(kind, N, H, C):
    ops = _ops()
    g = torch.Generator().manual_seed(N * 100 + C)
    x = (torch.randn(N, C, H, H, generator=g) * 1.5 + 0.2).requires_grad_(True)
    m = torch.nn.GroupNorm(32, C) if kind == "gn" else torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        m.weight.copy_(torch.randn(C, generator=g)); m.bias.copy_(torch.randn(C, generator=g) * 0.5)
    y = F.relu(m(x))
    gy = torch.randn(y.shape, generator=g)
    gx_ref, gg_ref, gb_ref = torch.autograd.grad(y, (x, m.weight, m.bias), gy)
    xn = _nhwc(x.detach())
    if kind == "gn":
        yd, stats = ops.groupnorm_act(xn, _dev(m.weight.detach()), _dev(m.bias.detach()), 32, eps=m.eps, relu=True, return_stats=True)
        rows_per_stat, groups = H * H, 32
    else:
        yd, stats = ops.batchnorm_act(xn, _dev(m.weight.detach()), _dev(m.bias.detach()), None, None, eps=m.eps, relu=True, return_stats=True)
        rows_per_stat, groups = N * H * H, C
    dx, dgam, dbet = ops.norm_act_bwd(xn, _nhwc(gy), yd, _dev(m.weight.detach()), stats, rows_per_stat, groups, m.eps, True)
    _close(dx.permute(0, 3, 1, 2), gx_ref, rtol=2e-4, what="norm bwd dx")
    _close(dgam, gg_ref, rtol=2e-4, what="norm bwd dgamma")
    _close(dbet, gb_ref, rtol=2e-4, what="norm bwd dbeta")


def test_bf16_grad_sample_storage_kernels():
    """bf16-stored per-sample gradients: wgrad epilogue rounding (RNE), norms of the ROUNDED values, and the
    bf16 norm / clip kernels (fp32 accumulate) against torch on the same rounded numbers."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    N, H, C, K, R = 4, 8, 16, 32, 5
    x = torch.randn(N, C, H, H, generator=g)
    gy = torch.randn(N, K, H // 2, H // 2, generator=g)
    w = torch.zeros(K, C, R, R, requires_grad=True)
    refs = []
    for b in range(N):
        y = F.conv2d(x[b:b + 1], w, None, stride=2, padding=2)
        refs.append(torch.autograd.grad(y, w, gy[b:b + 1])[0] * 2.5)
    ref = torch.stack(refs)
    ref_bf = ref.to(torch.bfloat16)                                   # round-to-nearest-even, like the kernel
    out = torch.empty(N, K, R, R, C, device="cuda", dtype=torch.bfloat16)
    sq = torch.zeros(N, device="cuda")
    ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=2, pad=2, group=1, alpha=2.5, out=out, sq=sq)
    got = out.permute(0, 1, 4, 2, 3).float().cpu()
    mism = (got != ref_bf.float()).float().mean().item()
    assert mism < 2e-3, "bf16 rounding differs on %.3f%% of entries" % (100 * mism)   # only fp32 last-bit ties may differ
    _close(got, ref, rtol=8e-3, what="bf16 wgrad")
    _close(sq, got.reshape(N, -1).double().pow(2).sum(1).float(), rtol=1e-4, what="sq of rounded values")
    # norm + clip kernels on mixed bf16 / fp32 segments
    rows, lens = 6, [4803, 64, 1031]
    mats = [torch.randn(rows, L, generator=g) for L in lens]
    dm = [mats[0].to(torch.bfloat16).cuda(), mats[1].cuda(), mats[2].to(torch.bfloat16).cuda()]
    as_f = [d.float().cpu() for d in dm]
    sqn = ops.sample_sqnorm(dm)
    _close(sqn, torch.stack([m.double().pow(2).sum(1).float() for m in as_f]), rtol=1e-4, what="bf16 sqnorm")
    f = torch.rand(3, rows, generator=g)
    outs = [torch.zeros(L, device="cuda") for L in lens]
    ops.clip_accum_noise(dm, outs, factors=f.cuda(), scale=0.5)
    for i in range(3):
        _close(outs[i], 0.5 * (as_f[i] * f[i][:, None]).sum(0), rtol=1e-4, what="bf16 clip_accum %d" % i)


def test_repack_cache_follows_weight_updates():
    """Repacked data-gradient filters and the channel-folded UpsampleConv filters are cached per parameter + version counter: an in-place
    torch update and a HipAdam step (raw-pointer kernel + explicit version bump) must both invalidate them."""
    from csl_gan_amd import nn as hnn, ops, functional as HF
    from csl_gan_amd.engine import HipAdam
    torch.manual_seed(0)
    conv = hnn.to_device_layout(hnn.HipConv2d(8, 16, 5, stride=2, padding=2).cuda())
    from csl_gan_amd.DCResNet_models import UpsampleConv
    upm = hnn.to_device_layout(UpsampleConv(8, 8, 5, bias=False).cuda())
    up = upm.conv
    x = torch.randn(2, 8, 8, 8)

    def run():
        xd = x.clone().cuda().requires_grad_(True)
        y = conv(xd)
        gx, = torch.autograd.grad(y.sum(), xd)
        with torch.no_grad():
            yu = upm(x.cuda())
        return gx.cpu(), yu.cpu()

    def ref():
        xr = x.clone().requires_grad_(True)
        y = F.conv2d(xr, conv.weight.detach().cpu(), conv.bias.detach().cpu(), stride=2, padding=2)
        gx, = torch.autograd.grad(y.sum(), xr)
        yu = F.conv2d(F.pixel_shuffle(torch.cat([x, x, x, x], 1), 2), up.weight.detach().cpu(), None, padding=2)
        return gx, yu
    for step in range(3):
        (g1, u1), (g0, u0) = run(), ref()
        _close(g1, g0, what="dgrad step %d" % step); _close(u1, u0, what="up fwd step %d" % step)
        (g2, u2) = run()                                          # second call: served from the cache
        assert torch.equal(g1, g2) and torch.equal(u1, u2)
        if step == 0:
            with torch.no_grad():
                conv.weight.mul_(1.5); up.weight.add_(0.1)       # in-place torch ops bump the version counter
        elif step == 1:
            opt = HipAdam(list(conv.parameters()) + list(up.parameters()), lr=0.05, betas=(0.0, 0.9))
            for p in list(conv.parameters()) + list(up.parameters()):
                p.grad = torch.ones_like(p, memory_format=torch.preserve_format)
            opt.step()
    assert len(ops.repack_cache.d) >= 2


@pytest.mark.parametrize("case", [
    # N, H, W, C, K, R, stride, pad
    (5, 8, 8, 256, 512, 5, 2, 2),      # critic conv4: 16 output pixels
    (3, 16, 16, 128, 256, 5, 2, 2),    # critic conv3: 64 output pixels
    (7, 1, 1, 64, 32, 1, 1, 0),        # a linear layer: 1 pixel
    (4, 6, 6, 32, 64, 3, 1, 1),        # 36 pixels, stride 1
    (3, 4, 4, 32, 32, 3, 1, 1),
    (2, 7, 5, 64, 96, 5, 2, 2),        # ragged: 4x3 outputs
    # pixel-pair kernel (<= 16 output pixels, <= 16 input pixels per parity class, K % 64 == 0)
    (3, 4, 4, 32, 64, 3, 1, 1),        # stride 1: one class
    (2, 7, 5, 64, 128, 5, 2, 2),       # odd input: four classes of different sizes
    (4, 2, 2, 64, 64, 3, 1, 1),
    (6, 8, 8, 32, 192, 3, 2, 1),
    (2, 1, 1, 64, 64, 1, 1, 0),
    (9, 1, 1, 8192, 1, 1, 1, 0),       # the critic's linear head (norm product)
    (5, 1, 1, 794, 128, 1, 1, 0),
])
def test_wgrad_gram_norms_and_scaled_sum(case):
    """Ghost clipping pieces: per-sample ||gW_b||^2 from the pixel-Gram matrices equals the norm of the materialised
    per-sample gradient; the clip-weighted dense wgrad equals sum_b f_b gW_b."""
    ops = _ops()
    N, H, W, C, K, R, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.zeros(K, C, R, R, requires_grad=True)
    alpha = 2.5
    gy = torch.randn(F.conv2d(x, w, None, stride=s, padding=p).shape, generator=g)
    per = []
    for b in range(N):
        y = F.conv2d(x[b:b + 1], w, None, stride=s, padding=p)
        per.append(torch.autograd.grad(y, w, gy[b:b + 1])[0] * alpha)
    per = torch.stack(per)
    sq_ref = per.double().pow(2).flatten(1).sum(1).float()
    assert ops.gram_norms_eligible(_nhwc(gy).shape, _nhwc(x).shape) or ops.gram_norms_preferred(_nhwc(gy).shape, _nhwc(x).shape, s)
    sq = ops.conv2d_wgrad_sqnorm_gram(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, alpha=alpha)
    _close(sq, sq_ref, rtol=1e-4, what="gram norms %s" % (case,))
    sq2 = torch.full((N,), 3.0, device="cuda")                       # accumulates into the caller's buffer
    ops.conv2d_wgrad_sqnorm_gram(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, alpha=alpha, sq=sq2)
    _close(sq2 - 3.0, sq_ref, rtol=1e-4, what="gram norms accumulate")
    f = torch.rand(N, generator=g)
    ref = (per * f.view(-1, 1, 1, 1, 1)).sum(0)
    got = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=N, alpha=alpha, row_scale=_dev(f))
    _close(got[0].permute(0, 3, 1, 2), ref, what="clip-weighted dense wgrad %s" % (case,))
    with pytest.raises(RuntimeError):
        ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=N, row_scale=_dev(f[:-1]))


_GHOST_REF = {}


def _ghost_ref(case, rounded=False):
    """Operands of tests.ghost_inputs and their fp64 per-sample squared norms, computed once per case and never modified."""
    key = (case, rounded)
    if key not in _GHOST_REF:
        from tests import ghost_inputs as GI
        x, gy = GI.operands(case)
        if rounded:
            x, gy = _bf(x), _bf(gy)
        _GHOST_REF[key] = (x, gy, GI.reference_sq(x, gy, case[5], case[6], case[7], GI.ALPHA))
    return _GHOST_REF[key]


def _ghost_cases():
    from tests.ghost_inputs import CASES
    return [pytest.param(kernel, case, dead, id="%s-%s" % (kernel.replace("gram_sqnorm_", "").replace("_kernel", ""), "x".join(map(str, case))))
            for kernel, case, dead in CASES]


def _per_sample(sq, ref, tol, what):
    """|sq_b - ref_b| <= tol_b for EVERY sample b: a per-sample quantity is judged per sample, not against the batch maximum."""
    sq = sq.detach().cpu().double()
    assert sq.shape == ref.shape, (what, sq.shape, ref.shape)
    err = (sq - ref).abs()
    print("%s: worst per-sample error %.3e of the sample's own norm, %.3e of its tolerance" % (what, (err / ref).max().item(), (err / tol).max().item()))
    bad = (err > tol).nonzero().flatten().tolist()
    assert not bad, "%s: samples %s off: got %s, expected %s" % (what, bad, sq[bad].tolist(), ref[bad].tolist())


@pytest.mark.parametrize("kernel,case,dead", _ghost_cases())
def test_wgrad_gram_norms_per_sample_on_correlated_inputs(kernel, case, dead):
    """Ghost norms on operands whose p != p' Gram terms carry most of the norm (tests/test_ghost_inputs.py: >= 0.49 of it, >= 1.2e-2
    from the least visible tap; white noise: 1e-3 and 1e-5) and whose scale spans six decades over the batch, each sample held to
    1e-4 of ITS OWN squared norm against the fp64 norm of the materialised gradient.  Every kernel of the entry point is named, so a
    routing change cannot drop one from the test."""
    from csl_gan_amd import _lib
    from tests.ghost_inputs import ALPHA, BF16_CASE, reference_weighted_sum
    ops = _ops()
    N, H, W, C, K, R, s, p = case
    x, gy, ref = _ghost_ref(case)
    xd, gd = _nhwc(x), _nhwc(gy)
    run = lambda g_, **kw: ops.conv2d_wgrad_sqnorm_gram(g_, xd, R, R, stride=s, pad=p, alpha=ALPHA, **kw)
    sq = run(gd)
    name = _lib.lib().cslgan_last_kernel().decode()
    assert name == kernel, "case %s ran %s" % (case, name)
    _per_sample(sq, ref, 1e-4 * ref, "%s %s" % (kernel, case))
    # accumulating form: the pre-fill is far above most samples' norms, so each of the `adds` atomic adds into sq[b] (one per
    # workgroup of sample b: one per stride-parity class in cls64, one otherwise) rounds to the fp32 grid at the pre-fill — at most
    # half a spacing each, the spacing anywhere in [fill, fill + max ref] being at most eps * 4 max ref.
    fill = torch.tensor(3.0 * ref.max().item(), dtype=torch.float32)
    sq2 = run(gd, sq=torch.full((N,), fill.item(), device="cuda"))
    adds = s * s if kernel == "gram_sqnorm_cls64_kernel" else 1
    spacing = torch.finfo(torch.float32).eps * 4.0 * ref.max().item()
    _per_sample(sq2.cpu().double() - fill.double(), ref, 1e-4 * ref + adds * 0.5 * spacing, "%s %s accumulate" % (kernel, case))
    if dead:
        # a sample whose output gradient is zero has norm 0.0 exactly, and leaves every other sample's bits alone
        g0 = gy.clone()
        g0[1] = 0
        sq0 = run(_nhwc(g0))
        assert sq0[1].item() == 0.0, sq0
        live = [b for b in range(N) if b != 1]
        if kernel == "gram_sqnorm_cls64_kernel" and s > 1:
            # one workgroup per (sample, class) adds into sq[b] atomically: the order of the s^2 addends is the scheduler's, so
            # two runs may differ in the last bits
            _per_sample(sq0[live], ref[live], 1e-4 * ref[live], "%s %s beside a dead sample" % (kernel, case))
        else:
            assert torch.equal(sq0[live], sq[live]), (sq0, sq)
    # the clip weights these norms imply (C = the median norm), applied by the dense clip-weighted weight gradient
    nrm = ref.sqrt()
    f = (nrm.median() / nrm).clamp(max=1.0).float()
    got = ops.conv2d_wgrad_grouped(gd, xd, R, R, stride=s, pad=p, group=N, alpha=ALPHA, row_scale=_dev(f))
    _close(got[0].permute(0, 3, 1, 2), reference_weighted_sum(x, gy, f, R, s, p, ALPHA), what="clip-weighted dense wgrad %s" % (case,))
    if case == BF16_CASE:
        # bfloat16-stored gy and x: the entry casts them up, so the norms are those of the ROUNDED values, at the same tolerance
        xr, gr, ref_r = _ghost_ref(case, rounded=True)
        sq = ops.conv2d_wgrad_sqnorm_gram(_nhwc(gr).bfloat16(), _nhwc(xr).bfloat16(), R, R, stride=s, pad=p, alpha=ALPHA)
        assert _lib.lib().cslgan_last_kernel().decode() == kernel
        _per_sample(sq, ref_r, 1e-4 * ref_r, "%s %s bf16-stored operands" % (kernel, case))


def test_wgrad_gram_rejects_unsupported_shapes():
    ops = _ops()
    gy, x = torch.zeros(2, 16, 16, 64, device="cuda"), torch.zeros(2, 32, 32, 32, device="cuda")
    assert not ops.gram_norms_eligible(gy.shape, x.shape)
    with pytest.raises(RuntimeError, match="at most 64 output pixels"):
        ops.conv2d_wgrad_sqnorm_gram(gy, x, 5, 5, stride=2, pad=2)
    with pytest.raises(RuntimeError, match="multiples of 32"):
        ops.conv2d_wgrad_sqnorm_gram(torch.zeros(2, 4, 4, 24, device="cuda"), torch.zeros(2, 8, 8, 32, device="cuda"), 5, 5, stride=2, pad=2)


@pytest.mark.parametrize("case", [(2, 16, 16, 3, 3), (3, 8, 16, 1, 3), (2, 8, 8, 4, 3), (5, 64, 64, 3, 3), (2, 8, 8, 2, 1), (130, 8, 8, 3, 3)])
def test_wgrad_dense_skinny(case):
    """Dense weight gradient of a 64 -> K (K <= 4) stride-1 conv on the vector-ALU kernel (G's output conv in train_G)."""
    ops = _ops()
    N, H, W, K, R = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, 64, H, W, generator=g)
    w = torch.zeros(K, 64, R, R, requires_grad=True)
    y = F.conv2d(x, w, None, padding=R // 2)
    gy = torch.randn(y.shape, generator=g)
    ref, = torch.autograd.grad(y, w, gy)
    got = ops.conv2d_wgrad_dense(_nhwc(gy), _nhwc(x), R, R, stride=1, pad=R // 2, alpha=1.5)
    _close(got.permute(0, 3, 1, 2), ref * 1.5, what="skinny dense wgrad %s" % (case,))


# ---- bf16 MFMA compute path (cslgan_conv_t.compute = BF16; BASELINE.json configs[4]) ------------------------------------
def _bf(t):
    """Round-to-nearest-even to bfloat16 and back: what the kernels do to every MFMA operand."""
    return t.to(torch.bfloat16).float()


BF16_FWD = [c for c in FWD_CASES if not c[10]][:24] + [(4, 16, 16, 64, 128, 5, 1, 2, True, 1, False, 0), (130, 4, 4, 48, 72, 3, 1, 1, True, 2, False, None)]


@pytest.mark.parametrize("case", BF16_FWD)
def test_conv2d_fwd_bf16(case):
    """Forward conv on v_mfma_f32_32x32x16_bf16 against torch fp32 math on bf16-ROUNDED operands (so only the fp32 summation
    order differs: 1e-4 of scale), and against the unrounded fp32 conv at the bf16 tolerance 2e-2 of scale."""
    ops = _ops()
    N, H, W, C, K, R, s, p, has_b, act, ups, res = case
    g = torch.Generator().manual_seed(_case_seed(case))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g) if has_b else None

    def ref(xx, ww):
        y = F.conv2d(xx, ww, b, stride=s, padding=p)
        if res is not None:
            y = y + rs
        return F.leaky_relu(y, 0.2) if act == 1 else (F.relu(y) if act == 2 else (torch.tanh(y) if act == 3 else y))
    rs = torch.randn(F.conv2d(x, w, None, stride=s, padding=p).shape, generator=g) if res is not None else None
    with ops.compute_dtype("bf16"):
        y = ops.conv2d_fwd(_nhwc(x), _krsc(w), None if b is None else b.cuda(), stride=s, pad=p,
                           residual=None if rs is None else _nhwc(rs), act=act)
    assert ops.get_compute_dtype() == "fp32"
    # 1..4 output channels (vector-ALU kernel) and the RGB first layer (conv_c3) compute in exact fp32 in every mode
    exact = ((K <= 4 and C == 64 and s == 1) or (C == 3 and K == 64 and R == 5 and s == 2 and H % 16 == 0 and W % 32 == 0 and res is None)
             or (H == 1 and W == 1 and R == 1))           # small linear layers run on the fp32 kernels (ops._conv_desc)
    _close(y.permute(0, 3, 1, 2), ref(x, w) if exact else ref(_bf(x), _bf(w)), rtol=1e-4, what="bf16 fwd vs rounded-operand reference %s" % (case,))
    _close(y.permute(0, 3, 1, 2), ref(x, w), rtol=2e-2, what="bf16 fwd vs fp32 %s" % (case,))


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_conv2d_dgrad_bf16(case):
    ops = _ops()
    N, H, W, C, K, R, s, p, use_mask = case
    g = torch.Generator().manual_seed(sum(case) + 3)
    w = torch.randn(K, C, R, R, generator=g) / (K * R * R) ** 0.5
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    gy = torch.randn(N, K, P, Q, generator=g)
    # 1..4 output channels from 64 input channels on 8x8-patchable class grids: the vector-ALU kernel, exact fp32 in every mode
    exact = (K == 64 and C <= 4 and H % s == 0 and W % s == 0 and (H // s) % 8 == 0 and (W // s) % 8 == 0) or (H == 1 and W == 1 and R == 1)
    rnd = (lambda t: t) if exact else _bf
    ref = F.conv_transpose2d(rnd(gy), rnd(w), None, stride=s, padding=p, output_padding=(H + 2 * p - R - (P - 1) * s, W + 2 * p - R - (Q - 1) * s))
    mask = None
    if use_mask:
        mask = torch.randn(N, C, H, W, generator=g)
        ref = ref * torch.where(mask > 0, 1.0, 0.2)
    with ops.compute_dtype("bf16"):
        gx = ops.conv2d_dgrad(_nhwc(gy), _krsc(w), (H, W), stride=s, pad=p, mask=None if mask is None else _nhwc(mask))
    _close(gx.permute(0, 3, 1, 2), ref, rtol=1e-4, what="bf16 dgrad %s" % (case,))


@pytest.mark.parametrize("case", [(2, 8, 8, 8, 16, 5, 2, 2), (3, 16, 16, 3, 64, 5, 2, 2), (4, 8, 8, 64, 128, 5, 2, 2), (2, 7, 9, 12, 20, 3, 1, 1),
                                  (6, 1, 1, 794, 128, 1, 1, 0), (4, 32, 32, 64, 128, 5, 2, 2), (8, 8, 8, 256, 512, 5, 2, 2), (3, 64, 64, 4, 64, 5, 2, 2),
                                  (2, 16, 16, 128, 256, 5, 2, 2)])
@pytest.mark.parametrize("group", [1, 2, 0])
def test_conv2d_wgrad_grouped_bf16(case, group):
    """Grouped weight gradient (group=1: per-sample gradients) on the bf16 MFMA: gradients, the fused per-group squared norms,
    bf16 storage and the clip-weighted (row_scale) form, against fp32 math on bf16-rounded operands."""
    ops = _ops()
    N, H, W, C, K, R, s, p = case
    grp = N if group == 0 else group
    if N % grp:
        pytest.skip("N not divisible by group")
    g = torch.Generator().manual_seed(sum(case) + 11 * grp)
    x = torch.randn(N, C, H, W, generator=g)
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    gy = torch.randn(N, K, P, Q, generator=g)
    alpha = 1.75
    lin = H == 1 and W == 1 and R == 1               # small linear layers run on the fp32 kernels (ops._conv_desc)
    rnd = (lambda t: t) if lin else _bf
    xr, gr = rnd(x), rnd(gy)
    wz = torch.zeros(K, C, R, R, requires_grad=True)
    refs = []
    for b0 in range(0, N, grp):
        y = F.conv2d(xr[b0:b0 + grp], wz, None, stride=s, padding=p)
        refs.append(torch.autograd.grad(y, wz, gr[b0:b0 + grp])[0] * alpha)
    ref = torch.stack(refs)
    sq = torch.zeros(N // grp, device="cuda")
    with ops.compute_dtype("bf16"):
        gw = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=grp, alpha=alpha, sq=sq)
        sq2 = torch.zeros(N // grp, device="cuda")
        none = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=grp, alpha=alpha, want_gw=False, sq=sq2)
        f = torch.rand(N, generator=g) + 0.1
        gws = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=grp, alpha=alpha, row_scale=f.cuda())
    assert none is None
    _close(gw.permute(0, 1, 4, 2, 3), ref, rtol=1e-4, what="bf16 wgrad %s g%d" % (case, grp))
    exp_sq = ref.reshape(N // grp, -1).double().pow(2).sum(1).float()
    _close(sq, exp_sq, rtol=2e-4, what="bf16 wgrad sq")
    _close(sq2, exp_sq, rtol=2e-4, what="bf16 wgrad sq (norms only)")
    # clip-weighted form: gy rows scaled BEFORE the bf16 rounding (the kernel multiplies on load)
    refs = []
    grs = rnd(gy * f.view(-1, 1, 1, 1))
    for b0 in range(0, N, grp):
        y = F.conv2d(xr[b0:b0 + grp], wz, None, stride=s, padding=p)
        refs.append(torch.autograd.grad(y, wz, grs[b0:b0 + grp])[0] * alpha)
    _close(gws.permute(0, 1, 4, 2, 3), torch.stack(refs), rtol=1e-4, what="bf16 wgrad scaled")


# ---- bf16x3: fp32 emulated from three bfloat16 pieces per operand (cslgan_conv_t.compute = BF16X3) ----------------------
def _err64(got, ref64):
    got = got.detach().cpu().double()
    return ((got - ref64).abs().max() / (ref64.abs().max() + 1e-300)).item()


@pytest.mark.parametrize("case", [(4, 16, 16, 64, 96, 5, 1, 2), (3, 16, 16, 32, 64, 5, 2, 2), (6, 1, 1, 794, 128, 1, 1, 0), (2, 9, 7, 12, 20, 3, 1, 1),
                                  (2, 8, 8, 512, 512, 5, 1, 2), (16, 8, 8, 256, 512, 5, 2, 2), (3, 64, 64, 3, 64, 5, 2, 2)])
def test_bf16x3_is_fp32_accurate(case):
    """x = hi + mid + lo in bfloat16 covers fp32's 24 mantissa bits, and the six kept piece products are exact in fp32: the
    emulated path must be AT LEAST as close to an fp64 reference as the exact-fp32 MFMA kernels (whose k-ordered fmaf chain
    carries ~sqrt(K) roundings), for forward, data gradient and (per-sample) weight gradient — plus an absolute fp32-level
    bound of 2e-6 of scale."""
    ops = _ops()
    N, H, W, C, K, R, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    gy = torch.randn(N, K, P, Q, generator=g)
    x64, w64, gy64 = x.double().requires_grad_(True), w.double().requires_grad_(True), gy.double()
    y64 = F.conv2d(x64, w64, None, stride=s, padding=p)
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), gy64)
    gws64 = []                                                     # per-sample weight gradients
    for b in range(N):
        wz = w.double().requires_grad_(True)
        gws64.append(torch.autograd.grad(F.conv2d(x[b:b + 1].double(), wz, None, stride=s, padding=p), wz, gy64[b:b + 1])[0])
    gws64 = torch.stack(gws64)
    errs = {}
    for mode in ("fp32", "bf16x3"):
        with ops.compute_dtype(mode):
            y = ops.conv2d_fwd(_nhwc(x), _krsc(w), None, stride=s, pad=p).permute(0, 3, 1, 2)
            gx = ops.conv2d_dgrad(_nhwc(gy), _krsc(w), (H, W), stride=s, pad=p).permute(0, 3, 1, 2)
            sq = torch.zeros(N, device="cuda")
            gw = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=1, sq=sq).permute(0, 1, 4, 2, 3)
        errs[mode] = (_err64(y, y64.detach()), _err64(gx, gx64), _err64(gw, gws64),
                      _err64(sq, gws64.reshape(N, -1).pow(2).sum(1)))
    print("bf16x3 vs fp32 kernels, max error / scale against fp64, case %s:" % (case,))
    ratios = []
    for i, what in enumerate(("forward", "data gradient", "per-sample weight gradient", "per-sample squared norm")):
        e32, e3 = errs["fp32"][i], errs["bf16x3"][i]
        print("   %-28s fp32 kernels %.2e   bf16x3 %.2e" % (what, e32, e3))
        # fp32-level for reductions of up to 6400 terms (the exact-fp32 MFMA chain itself reaches 2.6e-6 there)
        assert e3 <= 4e-6, "%s: bf16x3 error %.3e vs fp64 (exact-fp32 kernels: %.3e)" % (what, e3, e32)
        assert e3 <= 3 * e32 + 1e-6, "%s: bf16x3 error %.3e is far above the exact-fp32 kernels' %.3e" % (what, e3, e32)
        ratios.append(e3 / max(e32, 1e-12))
    _X3_RATIOS.extend(ratios)


_X3_RATIOS = []


def test_bf16x3_is_on_average_no_worse_than_fp32_kernels():
    """Over all shapes and ops of the test above (which must have run): the geometric mean of error(bf16x3) / error(fp32
    kernels) against fp64 is <= 1 — the emulated products are as good as the exact-fp32 MFMA's, not merely 'close'."""
    if not _X3_RATIOS:
        pytest.skip("run together with test_bf16x3_is_fp32_accurate")
    gm = float(np.exp(np.mean(np.log(np.maximum(_X3_RATIOS, 1e-6)))))
    print("geometric mean of error ratios bf16x3 / fp32 kernels over %d measurements: %.3f" % (len(_X3_RATIOS), gm))
    assert gm <= 1.0, gm


@pytest.mark.parametrize("case", [c for c in FWD_CASES if not c[10]])
def test_conv2d_fwd_bf16x3(case):
    """Every forward shape / epilogue of test_conv2d_fwd on the three-piece path (gather kernel and LDS-halo kernel), against
    the same fp32 torch reference at the same tolerance as the exact-fp32 kernels."""
    ops = _ops()
    N, H, W, C, K, R, s, p, has_b, act, ups, res = case
    g = torch.Generator().manual_seed(_case_seed(case))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g) if has_b else None
    ref = F.conv2d(x, w, b, stride=s, padding=p)
    resid = None
    if res is not None:
        rs = torch.randn(ref.shape, generator=g)
        ref = ref + rs
        resid = _nhwc(rs)
    ref = F.leaky_relu(ref, 0.2) if act == 1 else (F.relu(ref) if act == 2 else (torch.tanh(ref) if act == 3 else ref))
    with ops.compute_dtype("bf16x3"):
        y = ops.conv2d_fwd(_nhwc(x), _krsc(w), None if b is None else b.cuda(), stride=s, pad=p, residual=resid, act=act)
    _close(y.permute(0, 3, 1, 2), ref, what="bf16x3 fwd %s" % (case,))


@pytest.mark.parametrize("case", DGRAD_CASES + [(4, 32, 32, 64, 128, 5, 2, 2, True), (2, 16, 16, 128, 256, 5, 2, 2, False), (3, 16, 16, 64, 64, 5, 1, 2, False)])
def test_conv2d_dgrad_bf16x3(case):
    ops = _ops()
    N, H, W, C, K, R, s, p, use_mask = case
    g = torch.Generator().manual_seed(sum(case) + 5)
    w = torch.randn(K, C, R, R, generator=g) / (K * R * R) ** 0.5
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    gy = torch.randn(N, K, P, Q, generator=g)
    ref = F.conv_transpose2d(gy, w, None, stride=s, padding=p, output_padding=(H + 2 * p - R - (P - 1) * s, W + 2 * p - R - (Q - 1) * s))
    mask = None
    if use_mask:
        mask = torch.randn(N, C, H, W, generator=g)
        ref = ref * torch.where(mask > 0, 1.0, 0.2)
    with ops.compute_dtype("bf16x3"):
        gx = ops.conv2d_dgrad(_nhwc(gy), _krsc(w), (H, W), stride=s, pad=p, mask=None if mask is None else _nhwc(mask))
    _close(gx.permute(0, 3, 1, 2), ref, what="bf16x3 dgrad %s" % (case,))


@pytest.mark.parametrize("N,H,W", [(6, 64, 64), (3, 128, 128)])
def test_first_layer_dense_wgrad_is_the_sum_of_the_per_image_kernel(N, H, W):
    """conv2d_wgrad_dense on RGB input: per-image gradients from c3_wgrad_kernel + one column sum."""
    ops = _ops()
    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.zeros(64, 3, 5, 5, requires_grad=True)
    y = F.conv2d(x, w, None, stride=2, padding=2)
    gy = torch.randn(y.shape, generator=g)
    ref, = torch.autograd.grad(y, w, gy)
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        got = ops.conv2d_wgrad_dense(_nhwc(gy), _nhwc(x), 5, 5, stride=2, pad=2, alpha=0.5)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_timer(None)
    assert any("c3_wgrad_kernel" in k for k in timer.summary(by_kernel=True)), timer.summary(by_kernel=True).keys()
    _close(got.permute(0, 3, 1, 2), 0.5 * ref, what="dense first-layer wgrad")


def test_mean_sample_gather_jitter_noise():
    """cslgan_mean_sample_f32 = MeanSampler.sample (mean_sampler.py:75-84): the right rows without noise; with noise the per-image
    jitter is one constant per image ~ N(0, s1^2) and the per-pixel residual ~ N(0, s2^2); draws differ between calls."""
    from csl_gan_amd.mean_sampler import MeanSampler
    ops = _ops()
    g = torch.Generator().manual_seed(4)
    ms = MeanSampler(noise_std=0.12, num_samples=32, mean_size=1000, dataset_size=180000, n_classes=2, smallest_class_size=70000, device="cuda")
    ms.mean_samples = torch.randn(2, 32, 3, 16, 16, generator=g).cuda()
    labels = torch.randint(0, 2, (128,), generator=g).cuda()
    r, y = ms.sample(128, noise_std=0, noise_mean_std=0, requested_labels=labels)
    assert torch.equal(y, labels) and r.shape == (128, 3, 16, 16)
    flat = ms.mean_samples.reshape(2, 32, -1)
    for blk in range(4):            # every block of 32 draws is a permutation of the 32 mean samples of the requested classes
        idx = []
        for i in range(32 * blk, 32 * blk + 32):
            match = (flat[labels[i]] == r[i].reshape(1, -1)).all(dim=1).nonzero()
            assert match.numel() == 1
            idx.append(int(match))
        assert sorted(idx) == list(range(32))
    s1, s2 = 0.05, 0.02
    perms = torch.arange(128, device="cuda") % 32
    a = ops.mean_sample(ms.mean_samples, labels, perms, s1, s2, seed=11, offset=1)
    b = ops.mean_sample(ms.mean_samples, labels, perms, s1, s2, seed=11, offset=2)
    a2 = ops.mean_sample(ms.mean_samples, labels, perms, s1, s2, seed=11, offset=1)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    res = (a - ms.mean_samples[labels, perms]).reshape(128, -1)
    jit = res.mean(dim=1)                                   # 768 pixels: the pixel noise averages to s2/sqrt(768) = 7e-4
    assert abs(jit.std().item() - s1) < 0.25 * s1 and abs(jit.mean().item()) < 0.3 * s1
    pix = res - jit.unsqueeze(1)
    assert abs(pix.std().item() - s2) < 0.03 * s2
    # one class: labels may be omitted
    one = ops.mean_sample(ms.mean_samples[:1].contiguous(), None, perms, 0.0, 0.0, seed=1, offset=1)
    assert torch.equal(one, ms.mean_samples[0, perms])
    # in-kernel draws: labels when none are requested (uniform over the classes), new permutations on every call, and the
    # cat-of-randperms structure (mean_sampler.py:76) for a batch that is not a multiple of num_samples
    r1, y1 = ms.sample(128, noise_std=0, noise_mean_std=0)
    r2, y2 = ms.sample(128, noise_std=0, noise_mean_std=0)
    assert y1.shape == (128,) and int(y1.min()) >= 0 and int(y1.max()) <= 1 and 30 < int(y1.sum()) < 98 and not torch.equal(y1, y2)
    assert torch.equal(r1, ms.mean_samples[y1, _match_rows(flat, y1, r1)]) and not torch.equal(r1, r2)
    big = MeanSampler(noise_std=0.12, num_samples=200, mean_size=1000, dataset_size=180000, device="cuda")
    big.mean_samples = torch.randn(1, 200, 1, 4, 4, generator=g).cuda()
    rb, yb = big.sample(450, noise_std=0, noise_mean_std=0)
    assert yb is None
    idx = _match_rows(big.mean_samples.reshape(1, 200, -1), torch.zeros(450, dtype=torch.long, device="cuda"), rb).tolist()
    assert sorted(idx[:200]) == list(range(200)) and sorted(idx[200:400]) == list(range(200)) and len(set(idx[400:])) == 50
    assert idx[:200] != idx[200:400] and idx[:200] != list(range(200))


def _match_rows(flat, labels, r):
    """index of the mean sample each drawn image equals (noise-free draws)."""
    out = []
    for i in range(r.shape[0]):
        m = (flat[labels[i]] == r[i].reshape(1, -1)).all(dim=1).nonzero()
        assert m.numel() == 1
        out.append(int(m))
    return torch.tensor(out, device=r.device)


@pytest.mark.parametrize("case", [(6, 32, 32, 64, 128, 5, 2, 2), (9, 16, 16, 128, 64, 3, 1, 1)])
def test_wgrad_row_blocks_in_one_launch(case):
    """cslgan_conv2d_wgrad_blocks_f32: norms-only / stored / stored+norms blocks of one batch in one launch equal the per-block calls."""
    ops = _ops()
    N, H, W, C, K, R, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = _nhwc(torch.randn(N, C, H, W, generator=g))
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    gy = _nhwc(torch.randn(N, K, P, Q, generator=g))
    assert ops.wgrad_blocks_eligible(gy.shape, x.shape, R, R, s)
    n = N // 3
    L = K * R * R * C
    sq_a, sq_c = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    gw_b, gw_c = torch.empty(n, L, device="cuda"), torch.empty(n, L, device="cuda")
    ops.conv2d_wgrad_blocks(gy, x, R, R, s, p, 1.5, [(n, None, sq_a), (n, gw_b, None), (n, gw_c, sq_c)])
    for i, (gw, sq) in enumerate(((None, sq_a), (gw_b, None), (gw_c, sq_c))):
        sl = slice(i * n, (i + 1) * n)
        rsq = torch.zeros(n, device="cuda")
        ref = ops.conv2d_wgrad_grouped(gy[sl].contiguous(), x[sl].contiguous(), R, R, stride=s, pad=p, group=1, alpha=1.5, sq=rsq)
        if gw is not None:
            assert torch.equal(gw.view_as(ref), ref)
        if sq is not None:
            _close(sq, rsq, rtol=1e-6, what="block %d sq" % i)
    with pytest.raises(RuntimeError):       # a shape the LDS-resident kernel does not take
        ops.conv2d_wgrad_blocks(gy[:, :, :, :3].contiguous(), x, R, R, s, p, 1.0, [(N, None, torch.zeros(N, device="cuda"))])


# ---- round 3: the fused glue kernels of csrc/step_kernels.hip against plain torch -----------------------------------------------
def test_segment_means_forward_backward():
    """cslgan_segment_means_f32 (+ _bwd) = the critic's -mean / +mean losses over row blocks and their sum (DCResNet_models.py:149-153)."""
    from csl_gan_amd import functional as HF
    g = torch.Generator().manual_seed(1)
    sizes, signs = [128, 128, 100], [-1.0, 1.0, -1.0]
    x = torch.randn(sum(sizes), 1, generator=g)
    xr = x.clone().requires_grad_(True)
    parts = torch.split(xr, sizes)
    ref_vec = torch.stack([s * p.mean() for s, p in zip(signs, parts)])
    (ref_vec.sum() + 0.5 * ref_vec[1]).backward()
    xd = x.cuda().requires_grad_(True)
    vec, total = HF.SegmentMeans.apply(xd, sizes, [s / n for s, n in zip(signs, sizes)])
    (total + 0.5 * vec[1]).backward()
    assert torch.allclose(vec.detach().cpu(), ref_vec.detach(), rtol=1e-5, atol=1e-7)
    assert torch.allclose(total.detach().cpu(), ref_vec.detach().sum(), rtol=1e-5, atol=1e-7)
    assert torch.allclose(xd.grad.cpu(), xr.grad, rtol=1e-6, atol=1e-9)


def test_dstep_and_grad_log_statistics():
    """cslgan_dstep_stats_f32 = train.py:488-496; cslgan_grad_log_stats_f32 = train.py:310-329 (per layer and flat); both ADD to their sums."""
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    d_real, d_fake = torch.randn(96, 1, generator=g), torch.randn(128, 1, generator=g)
    rl, fl, pen = torch.tensor(-0.3), torch.tensor(0.7), torch.tensor(9.5)
    acc = torch.full((7,), 1.0).cuda()
    ops.dstep_stats(d_real.cuda(), d_fake.cuda(), rl.cuda(), fl.cuda(), pen.cuda(), acc)
    want = 1.0 + torch.tensor([0.4, 0.4, -0.3, 0.7, 100 * (d_real > 0).float().mean(), 100 * (d_fake < 0).float().mean(), 9.5])
    assert torch.allclose(acc.cpu(), want, rtol=1e-5)
    L, B = 9, 128
    sq = (torch.rand(L, 3 * B, generator=g) * 4).pow(2)
    sq[1] = (1.0 + 1e-4 * torch.rand(3 * B, generator=g)).pow(2)           # nearly equal norms: the std must not cancel away
    C = torch.rand(L, generator=g) * 2 + 0.5
    n = sq[:, 2 * B:].sqrt()
    for per_layer in (True, False):
        nn_ = n if per_layer else sq[:, 2 * B:].sum(dim=0, keepdim=True).sqrt()
        cc = C if per_layer else C[:1]
        rows = L if per_layer else 1
        acc = torch.zeros(5, rows).cuda()
        for _ in range(2):
            ops.grad_log_stats(sq.cuda(), 2 * B, B, cc.cuda().contiguous(), per_layer, 1e-6, acc)
        f = (cc.view(-1, 1) / (nn_ + 1e-6)).clamp(max=1.0)
        want = 2 * torch.stack([nn_.mean(1), nn_.std(1, unbiased=False), nn_.max(1).values, cc, (f < 0.999).float().mean(1)])
        got = acc.cpu()
        assert torch.allclose(got[[0, 2, 3, 4]], want[[0, 2, 3, 4]], rtol=1e-5, atol=1e-7), per_layer
        assert torch.allclose(got[1], want[1], rtol=2e-3, atol=1e-7), (per_layer, got[1], want[1])


@pytest.mark.parametrize("one_sided,per_sample", [(False, False), (True, False), (False, True), (True, True)])
def test_lipschitz_term_and_lerp(one_sided, per_sample):
    """cslgan_lerp_rows_f32 = gradient_penalty.py:36; cslgan_lipschitz_term_f32 (+ _bwd) = :52-54 with the weight and batch mean."""
    from csl_gan_amd import functional as HF
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    B, shape = 24, (3, 16, 16)
    real, fake, alpha = torch.randn((B,) + shape, generator=g), torch.randn((B,) + shape, generator=g), torch.rand(B, generator=g)
    a4 = alpha.view(B, 1, 1, 1)
    for fmt in (torch.contiguous_format, torch.channels_last):
        out = ops.lerp_rows(real.cuda().contiguous(memory_format=fmt), fake.cuda().contiguous(memory_format=fmt), alpha.cuda())
        assert torch.allclose(out.cpu(), a4 * real + (1 - a4) * fake, rtol=1e-6, atol=1e-7)
    t = torch.randn(B, 3 * 16 * 16, generator=g) * torch.linspace(0.01, 0.12, B).view(B, 1)          # norms on both sides of 1
    coef = 10.0 if per_sample else 10.0 / B
    tr_ = t.clone().requires_grad_(True)
    d = tr_.norm(2, dim=1) - 1
    ref = 10.0 * ((d.clamp(min=0) if one_sided else d) ** 2)
    ref = ref if per_sample else ref.mean()
    w = torch.linspace(0.5, 1.5, B)
    ((ref * w).sum() if per_sample else ref * 1.7).backward()
    td = t.cuda().requires_grad_(True)
    got = HF.LipschitzTerm.apply(td, one_sided, coef, per_sample)
    ((got * w.cuda()).sum() if per_sample else got * 1.7).backward()
    nrm = t.norm(2, dim=1)
    assert (nrm < 1).any() and (nrm > 1).any()
    assert torch.allclose(got.detach().cpu(), ref.detach(), rtol=1e-4, atol=1e-6)
    assert torch.allclose(td.grad.cpu(), tr_.grad, rtol=1e-4, atol=1e-7)
    # twice in a row: the kernel's ticket word is left at zero
    got2 = HF.LipschitzTerm.apply(td.detach(), one_sided, coef, per_sample)
    assert torch.allclose(got2.cpu(), got.detach().cpu())


def test_zeroed_accumulators_replay_correctly_in_a_captured_graph():
    """The kernels that accumulate with float atomics zero their output first (csrc/common.h zero_floats).  That zeroing used to be
    hipMemsetAsync, which as a memset node of a captured HIP graph replayed a 128-byte fill with a stale dword in every 16 bytes —
    every fourth per-sample norm of a 32-row batch came back as garbage from the second replay on, once an image-sized eager
    allocation + host-to-device copy had happened between replays.  Same conditions here: 32 x 12288 rows (the immediate-sensitivity
    input-gradient norms at B = 32), per-sample squared norms, GroupNorm statistics, and a split-K convolution."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    rows = (torch.randn(32, 12288, generator=g) * 1e-5).cuda()
    seg = [(torch.randn(32, n, generator=g) * 0.1).cuda() for n in (1728, 64)]
    xg = _nhwc(torch.randn(4, 64, 8, 8, generator=g))
    gam, bet = torch.randn(64, generator=g).cuda(), torch.randn(64, generator=g).cuda()
    xc, wc = _nhwc(torch.randn(2, 512, 4, 4, generator=g)), torch.randn(64, 5, 5, 512, generator=g).cuda() * 0.05     # 32 rows: K is split
    def step():
        return ops.row_l2norm(rows), ops.sample_sqnorm(seg), ops.groupnorm_act(xg, gam, bet, 32, relu=False), ops.conv2d_fwd(xc, wc, stride=1, pad=2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        outs = step()
    for k in range(5):
        fresh = [(torch.rand(32, 3, 64, 64, generator=g) * 2 - 1).cuda() for _ in range(2)]      # eager allocations + H2D between replays
        with torch.no_grad():
            rows.copy_(fresh[0].reshape(32, -1) * 1e-5 * (k + 1))
            seg[0].mul_(1.1)
            xg.add_(0.1)
            xc.mul_(0.9)
        gr.replay()
        torch.cuda.synchronize()
        del fresh
        _close(outs[0], rows.double().norm(dim=1).float(), rtol=1e-5, what="row norms, replay %d" % k)
        _close(outs[1], torch.stack([(t.double() ** 2).sum(1) for t in seg]).float(), rtol=1e-5, what="per-sample squared norms, replay %d" % k)
        _close(outs[2].permute(0, 3, 1, 2), F.group_norm(xg.permute(0, 3, 1, 2), 32, gam, bet), what="groupnorm, replay %d" % k)
        _close(outs[3].permute(0, 3, 1, 2), F.conv2d(xc.permute(0, 3, 1, 2), wc.permute(0, 3, 1, 2), padding=2), rtol=2e-3, what="split-K conv, replay %d" % k)


def test_ragged_column_sums_and_deferred_sums():
    """cslgan_segs_t.rows: one clip_accum_noise launch sums slab sets of DIFFERENT heights (beta accumulates into the destination),
    and ops.deferred_sums queues sum_rows() requests into one such launch at the end of the block."""
    ops = _ops()
    g = torch.Generator().manual_seed(31)
    mats = [torch.randn(n, ln, generator=g) for n, ln in ((128, 4800), (16, 1000), (1, 77), (8, 3_276_800 // 64))]
    outs = [torch.randn(m.shape[1], generator=g) for m in mats]
    dev_outs = [o.clone().cuda() for o in outs]
    ops.clip_accum_noise([m.cuda() for m in mats], dev_outs, beta=1.0, ragged=True)
    for m, o, d in zip(mats, outs, dev_outs):
        _close(d, o + m.double().sum(0).float(), rtol=1e-5, what="ragged column sum, %d rows" % m.shape[0])
    with pytest.raises(RuntimeError, match="ragged"):
        ops.clip_accum_noise([m.cuda() for m in mats], dev_outs, factors=torch.ones(128, device="cuda"), ragged=True)
    res = [torch.full((m.shape[1],), float("nan"), device="cuda") for m in mats]
    with ops.deferred_sums():
        for m, r in zip(mats, res):
            assert ops.sum_rows(m.cuda(), r) is r
        assert all(torch.isnan(r).all() for r in res), "queued, not run"
    for m, r in zip(mats, res):
        _close(r, m.double().sum(0).float(), rtol=1e-5, what="deferred column sum, %d rows" % m.shape[0])
    r2 = torch.empty(mats[1].shape[1], device="cuda")
    ops.sum_rows(mats[1].cuda(), r2)             # outside a block: immediate
    _close(r2, mats[1].double().sum(0).float(), rtol=1e-5, what="immediate column sum")


# ---- round 4: the LDS-halo kernel of the three-piece path (csrc/igemm_x3.hip) on every launch form it has ---------------------------
X3H_CASES = [
    # kind, N, H, W, C, K, R, stride, pad, what the case reaches
    ("fwd", 4, 16, 16, 64, 128, 5, 1, 2, "one class, 128-wide tiles, T = 25 (odd: the filter ring changes parity every chunk)"),
    ("fwd", 3, 16, 16, 16, 64, 5, 1, 2, "a single 16-channel chunk, 64-wide tiles, an odd number of 64-row patches"),
    ("fwd", 2, 8, 8, 48, 160, 3, 1, 1, "three chunks, T = 9, ragged N (160 filters), 8x8 images (halo mostly padding)"),
    ("fwd", 2, 32, 32, 32, 64, 5, 1, 2, "two chunks, 64 filters"),
    ("fwd", 2, 16, 24, 32, 96, 3, 1, 1, "non-square grid"),
    ("fwd", 6, 32, 32, 64, 128, 5, 2, 2, "stride-2 forward = four accumulated parity classes on sub-image views (9/6/6/4 taps)"),
    ("fwd", 128, 8, 8, 128, 192, 5, 2, 2, "stride-2 forward onto 4x4 grids: four-image patches with sub-image views"),
    ("fwd", 6, 16, 16, 32, 64, 5, 2, 2, "stride-2 forward, 64 filters, 8x8 output grids"),
    ("dgrad", 4, 32, 32, 64, 128, 5, 2, 2, "four parity classes in one launch (16x16 class grids)"),
    ("dgrad", 64, 32, 32, 64, 128, 5, 2, 2, "class pairs: 9 + 4 and 6 + 6 taps in one workgroup"),
    ("dgrad", 128, 8, 8, 128, 192, 5, 2, 2, "4x4 class grids: four-image patches"),
    ("dgrad", 3, 16, 16, 64, 64, 5, 1, 2, "stride-1 data gradient: one class with descending taps"),
    ("dgrad", 5, 16, 16, 128, 48, 3, 1, 1, "K = 48 reduction channels: three chunks"),
]


@pytest.mark.parametrize("case", X3H_CASES, ids=[c[-1].split(":")[0][:40].replace(" ", "_") for c in X3H_CASES])
@pytest.mark.parametrize("split", [True, False], ids=["split", "nosplit"])
@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "fp32"])
def test_x3_halo_kernel_forms(case, mode, split, monkeypatch):
    """igemm_x3h_kernel against an fp64 torch reference: fp32-level error (<= 4e-6 of scale, the bound of test_bf16x3_is_fp32_accurate)
    for the three-piece arithmetic, 1e-4 against fp32 math on bf16-ROUNDED operands for the one-piece form, 2e-6 for the exact-fp32
    form (v_mfma_f32_32x32x2_f32 on the same staging; igemm_x3h_kernel<., 0, .>).  Bias, LeakyReLU and the
    LeakyReLU mask ride along; the launch must really be the halo kernel (cslgan_last_kernel).  split: launches of fewer than 512
    tiles divide their reduction channels over workgroups ("/sN" in the kernel note: partial sums + the ordered reduce launch) — the
    strided forward and data-gradient cases here all do when the reduction has >= 64 channels; nosplit keeps the one-launch form covered."""
    from csl_gan_amd import _lib
    ops = _ops()
    monkeypatch.setattr(ops, "_X3_SPLIT", 8 if split else 0)
    kind, N, H, W, C, K, R, s, p, _ = case
    if not split and (kind, s) == ("fwd", 1):
        pytest.skip("stride-1 forward launches never split: covered by the split=True run")
    if mode == "fp32" and s == 2 and H == 8:
        pytest.skip("exact fp32 keeps the round-3 kernels on 4x4 class grids (x3h_eligible)")
    g = torch.Generator().manual_seed(1000 + sum(case[1:9]))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    gy = torch.randn(N, K, P, Q, generator=g)
    b = torch.randn(K, generator=g)
    m = torch.randn(N, C, H, W, generator=g)
    rnd = (lambda t: t.bfloat16().double()) if mode == "bf16" else (lambda t: t.double())
    if kind == "fwd":
        ref = F.leaky_relu(F.conv2d(rnd(x), rnd(w), b.double(), stride=s, padding=p), 0.2)
        with ops.compute_dtype(mode):
            got = ops.conv2d_fwd(_nhwc(x), _krsc(w), b.cuda(), stride=s, pad=p, act=1, wkey=("t", id(w))).permute(0, 3, 1, 2)
    else:
        ref = F.conv_transpose2d(rnd(gy), rnd(w), None, stride=s, padding=p,
                                 output_padding=(H + 2 * p - R - (P - 1) * s, W + 2 * p - R - (Q - 1) * s)) * torch.where(m > 0, 1.0, 0.2).double()
        with ops.compute_dtype(mode):
            got = ops.conv2d_dgrad(_nhwc(gy), _krsc(w), (H, W), stride=s, pad=p, mask=_nhwc(m), wkey=("t", id(w))).permute(0, 3, 1, 2)
    name = _lib.lib().cslgan_last_kernel().decode()
    assert name.startswith("igemm_x3h_kernel"), "case %s dispatched to %s" % (case, name)
    e = _err64(got, ref)
    assert (",0," in name) == (mode == "fp32") and (",3," in name) == (mode == "bf16x3"), name
    red, rows, cols = (C, N * P * Q, K) if kind == "fwd" else (K, N * H * W, C)
    want_split = split and (kind, s) != ("fwd", 1) and red >= 64 and -(-rows // 128) * -(-cols // 128) < 512
    assert ("/s" in name) == want_split, (name, want_split)
    assert e <= {"bf16x3": 4e-6, "bf16": 1e-4, "fp32": 2e-6}[mode], "%s %s: error %.3e of scale vs fp64 (%s)" % (mode, case[:9], e, name)


X3W_CASES = [
    # N, H, W, C, K, stride, group (0 = all), scaled, what
    (6, 32, 32, 64, 128, 2, 1, False, "per-sample gradients of the critic's second conv (four patches per image)"),
    (8, 16, 16, 128, 256, 2, 4, True, "clip-weighted group sums of the third conv (one patch per image)"),
    (8, 16, 16, 128, 256, 2, 0, False, "one dense slab: patches split over workgroups, float atomics"),
    (3, 16, 16, 64, 64, 1, 1, False, "stride 1, 64 x 64 channels"),
    (2, 32, 32, 128, 64, 1, 0, True, "stride 1 generator-side shape, clip weights, dense"),
    (4, 8, 8, 192, 128, 1, 2, False, "8x8 images at stride 1: the slab is mostly padding; three input-channel tiles"),
]


@pytest.mark.parametrize("case", X3W_CASES, ids=[c[-1][:38].replace(" ", "_") for c in X3W_CASES])
def test_x3_weight_gradient_kernel(case):
    """igemm_x3w_kernel (csrc/igemm_wgh.hip): grouped / per-sample / clip-weighted weight gradients and their squared norms on the
    three-piece path against fp64 — the fp32-level bound of test_bf16x3_is_fp32_accurate (4e-6 of scale; 2e-5 where float atomics
    reorder a dense sum), and no worse than 3x the exact-fp32 kernel's own error."""
    from csl_gan_amd import _lib
    ops = _ops()
    N, H, W, C, K, s, group, scaled, _ = case
    R, p = 5, 2
    group = N if group == 0 else group
    g = torch.Generator().manual_seed(77 + sum(case[:7]))
    x = torch.randn(N, C, H, W, generator=g)
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    gy = torch.randn(N, K, P, Q, generator=g)
    f = (torch.rand(N, generator=g) * 0.9 + 0.1) if scaled else torch.ones(N)
    alpha = 1.3
    refs = []
    for gi in range(N // group):
        sl = slice(gi * group, (gi + 1) * group)
        wz = torch.zeros(K, C, R, R, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x[sl].double(), wz, None, stride=s, padding=p)
        refs.append(alpha * torch.autograd.grad(y, wz, gy[sl].double() * f[sl].double().view(-1, 1, 1, 1))[0])
    ref = torch.stack(refs)
    errs = {}
    for mode in ("fp32", "bf16x3"):
        with ops.compute_dtype(mode):
            sq = None if scaled else torch.zeros(N // group, device="cuda")
            gw = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=group, alpha=alpha, sq=sq,
                                          row_scale=f.cuda() if scaled else None)
            name = _lib.lib().cslgan_last_kernel().decode()
        assert name.startswith("igemm_x3w_kernel" if mode == "bf16x3" else "igemm_wgh_kernel"), (mode, name)
        errs[mode] = (_err64(gw.permute(0, 1, 4, 2, 3), ref), None if sq is None else _err64(sq, ref.reshape(ref.shape[0], -1).pow(2).sum(1)))
    e32, e3 = errs["fp32"][0], errs["bf16x3"][0]
    print("x3w %s: error vs fp64 — exact-fp32 kernel %.2e, three-piece kernel %.2e" % (case[:8], e32, e3))
    assert e3 <= 4e-6 and e3 <= 3 * e32 + 1e-6, (e3, e32)
    if errs["bf16x3"][1] is not None:
        assert errs["bf16x3"][1] <= 2e-5, errs["bf16x3"][1]


def test_x3_weight_gradient_row_blocks():
    """cslgan_conv2d_wgrad_blocks_f32 on the three-piece kernel equals the per-block grouped calls in the same arithmetic."""
    ops = _ops()
    N, H, W, C, K, R, s, p = 6, 32, 32, 64, 128, 5, 2, 2
    g = torch.Generator().manual_seed(5)
    x = _nhwc(torch.randn(N, C, H, W, generator=g))
    gy = _nhwc(torch.randn(N, K, 16, 16, generator=g))
    n, L = N // 3, K * R * R * C
    with ops.compute_dtype("bf16x3"):
        assert ops.wgrad_blocks_eligible(gy.shape, x.shape, R, R, s)
        sq_a, sq_c = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        gw_b, gw_c = torch.empty(n, L, device="cuda"), torch.empty(n, L, device="cuda")
        ops.conv2d_wgrad_blocks(gy, x, R, R, s, p, 1.5, [(n, None, sq_a), (n, gw_b, None), (n, gw_c, sq_c)])
        for i, (gw, sq) in enumerate(((None, sq_a), (gw_b, None), (gw_c, sq_c))):
            sl = slice(i * n, (i + 1) * n)
            rsq = torch.zeros(n, device="cuda")
            ref = ops.conv2d_wgrad_grouped(gy[sl].contiguous(), x[sl].contiguous(), R, R, stride=s, pad=p, group=1, alpha=1.5, sq=rsq)
            if gw is not None:
                assert torch.equal(gw.view_as(ref), ref)
            if sq is not None:
                _close(sq, rsq, rtol=1e-6, what="x3 block %d sq" % i)


@pytest.mark.parametrize("group,scaled", [(0, False), (16, True), (2, False)])
def test_x3_weight_gradient_4x4_outputs(group, scaled):
    """igemm_x3w_kernel<2, quad>: the critic's last conv (8x8 -> 4x4, stride 2): dense / clip-weighted group sums over pairs of samples."""
    from csl_gan_amd import _lib
    ops = _ops()
    N, H, W, C, K, R, s, p = 32, 8, 8, 128, 192, 5, 2, 2
    group = N if group == 0 else group
    g = torch.Generator().manual_seed(31 + group)
    x = torch.randn(N, C, H, W, generator=g)
    gy = torch.randn(N, K, 4, 4, generator=g)
    f = (torch.rand(N, generator=g) * 0.9 + 0.1) if scaled else torch.ones(N)
    refs = []
    for gi in range(N // group):
        sl = slice(gi * group, (gi + 1) * group)
        wz = torch.zeros(K, C, R, R, dtype=torch.float64, requires_grad=True)
        refs.append(torch.autograd.grad(F.conv2d(x[sl].double(), wz, None, stride=s, padding=p), wz, gy[sl].double() * f[sl].double().view(-1, 1, 1, 1))[0])
    ref = torch.stack(refs)
    with ops.compute_dtype("bf16x3"):
        sq = None if scaled else torch.zeros(N // group, device="cuda")
        gw = ops.conv2d_wgrad_grouped(_nhwc(gy), _nhwc(x), R, R, stride=s, pad=p, group=group, sq=sq, row_scale=f.cuda() if scaled else None)
        name = _lib.lib().cslgan_last_kernel().decode()
    assert name.startswith("igemm_x3w_kernel<2,quad>"), name
    e = _err64(gw.permute(0, 1, 4, 2, 3), ref)
    assert e <= 4e-6, e
    if sq is not None:
        assert _err64(sq, ref.reshape(ref.shape[0], -1).pow(2).sum(1)) <= 2e-5


GN_FUSE_CASES = [
    # N, H, W, C, K, residual, what
    (3, 8, 8, 32, 512, False, "one patch per image, 16 channels per group, four 128-filter tiles"),
    (2, 16, 16, 64, 256, True, "four patches per image, residual added before the statistics"),
    (2, 32, 32, 32, 128, False, "16 patches per image, groups of 4 = one float4 of a lane"),
    (2, 64, 64, 16, 64, True, "64 patches per image (the limit), 64-filter tiles, groups of 2"),
    (5, 8, 8, 16, 64, False, "odd image count: the last workgroup holds one valid patch"),
]


@pytest.mark.parametrize("case", GN_FUSE_CASES, ids=[c[-1][:36].replace(" ", "_") for c in GN_FUSE_CASES])
@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
def test_groupnorm_statistics_from_the_conv_epilogue(case, mode):
    """cslgan_conv_t.gn_part + cslgan_groupnorm_apply_parts_f32: the halo kernel's epilogue leaves per-patch (sum, centred sum of
    squares) pairs of the values it stores, the apply kernel combines them exactly.  Against GroupNorm on the SAME conv output with
    its own statistics pass (<= 2e-6 of the output's scale: both are fp32 reductions in different orders) and against fp64
    F.group_norm of the fp64 conv (the conv's own error bound); the plain and the depth-to-space output layouts."""
    ops = _ops()
    N, H, W, C, K, with_res, _ = case
    g = torch.Generator().manual_seed(31 + sum(case[:5]))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 5, 5, generator=g) / (C * 25) ** 0.5
    b = torch.randn(K, generator=g) * 3.0                    # means well away from zero: E[x^2] - mean^2 would cancel
    res = torch.randn(N, K, H, W, generator=g) if with_res else None
    gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    with ops.compute_dtype(mode):
        with ops.gn_partials(32) as cell:
            y = ops.conv2d_fwd(_nhwc(x), _krsc(w), b.cuda(), stride=1, pad=2, act=0, residual=None if res is None else _nhwc(res), wkey=("gn", id(w)))
        assert cell.part is not None and cell.part[1] == H * W // 64
        y_plain = ops.conv2d_fwd(_nhwc(x), _krsc(w), b.cuda(), stride=1, pad=2, act=0, residual=None if res is None else _nhwc(res), wkey=("gn", id(w)))
    assert torch.equal(y, y_plain), "the statistics epilogue must not change the stored values"
    own = ops.groupnorm_act(y, gam.cuda(), bet.cuda(), 32, relu=True)
    fused = ops.groupnorm_act(y, gam.cuda(), bet.cuda(), 32, relu=True, part=cell.part)
    scale = own.abs().max().item()
    assert (fused - own).abs().max().item() <= 2e-6 * scale
    o2, r2 = ops.groupnorm_act(y, gam.cuda(), bet.cuda(), 32, relu=True, d2s=True, want_raw=True)
    f2, fr2 = ops.groupnorm_act(y, gam.cuda(), bet.cuda(), 32, relu=True, d2s=True, want_raw=True, part=cell.part)
    assert (f2 - o2).abs().max().item() <= 2e-6 * scale and torch.equal(fr2, r2)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=2) + (0 if res is None else res.double())
    ref = F.relu(F.group_norm(ref, 32, gam.double(), bet.double()))
    assert _err64(fused.permute(0, 3, 1, 2), ref) <= (2e-5 if mode == "bf16x3" else 1e-5)


def test_generator_forward_with_epilogue_statistics_matches_the_two_launch_form(monkeypatch, tmp_path):
    """The frozen DCResNet generator forward (what a D-step runs): every GroupNorm reads the statistics its producing conv left
    (eight statistics launches less per step) — same images as with CSLGAN_GN_FUSE off, to 5e-6 of their range."""
    from csl_gan_amd import init_util, options
    ops = _ops()
    opt = options.parse(["CelebA", "-dpm", "gc", "-nms", "4", "-bs", "4", "-gd", "cuda:0", "-dd", "cuda:0", "-o", str(tmp_path) + "/", "--manual_seed", "3", "--synthetic"])
    G, _ = init_util.init_models(opt)
    z = torch.randn(4, opt.g_latent_dim, device="cuda:0")
    outs = {}
    for fuse in (True, False):
        monkeypatch.setattr(ops, "_GN_FUSE", fuse)
        with torch.no_grad(), ops.compute_dtype("fp32_auto"):
            outs[fuse] = G(z).clone()
    assert (outs[True] - outs[False]).abs().max().item() <= 5e-6 * 2.0


AFFINE_CASES = [
    # N, H, W, C, K, R, residual, what
    (3, 8, 8, 512, 128, 5, False, "32 chunks, one patch per image"),
    (2, 32, 32, 128, 128, 5, True, "the block's second conv: residual epilogue, 16 patches per image"),
    (3, 16, 16, 64, 64, 5, False, "64-filter tiles, an odd image count (a workgroup with one valid patch)"),
    (2, 64, 64, 64, 3, 3, False, "the generator's output conv: the 1..4-output-channel kernel"),
    (5, 16, 16, 64, 2, 3, False, "two output channels, 3x3, odd image count"),
]


@pytest.mark.parametrize("case", AFFINE_CASES, ids=[c[-1][:36].replace(" ", "_") for c in AFFINE_CASES])
@pytest.mark.parametrize("mode", ["fp32_auto", "fp32"])
def test_groupnorm_folded_into_the_consuming_conv(case, mode):
    """cslgan_conv_t.in_scale / in_shift: conv(relu(GroupNorm(x))) with the normalisation applied while the conv stages x, against
    the two-kernel form on the same x (GroupNorm written to HBM, then the conv): <= 4e-6 of the output scale (three-piece / fp32
    products of inputs that differ by one fp32 rounding), zero padding applied AFTER the map (border pixels are the ones that show
    a wrong order), and against fp64."""
    ops = _ops()
    N, H, W, C, K, R, with_res, _ = case
    g = torch.Generator().manual_seed(57 + sum(case[:6]))
    x = torch.randn(N, C, H, W, generator=g) * 2.0 + 1.5
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g)
    res = torch.randn(N, K, H, W, generator=g) if with_res else None
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) + 0.3      # beta != 0: padding must not become relu(beta)
    xd, wd = _nhwc(x), _krsc(w)
    # statistics of x as a producing conv would leave them: per 64-row patch (sum, centred sum of squares)
    xp = x.double().view(N, 32, C // 32, H // 8, 8, W // 8, 8).permute(0, 3, 5, 1, 2, 4, 6).reshape(N, (H // 8) * (W // 8), 32, -1)
    part = torch.stack([xp.sum(-1), ((xp - xp.mean(-1, keepdim=True)) ** 2).sum(-1)], dim=-1).float().contiguous().cuda()
    with ops.compute_dtype(mode):
        assert ops.in_affine_ok(xd, wd, 1, R // 2)
        sc, sh = ops.groupnorm_affine((part, H * W // 64), gam.cuda(), bet.cuda(), 32, 1e-5, N, H * W, C)
        rd = None if res is None else _nhwc(res)
        got = ops.conv2d_fwd(xd, wd, b.cuda(), stride=1, pad=R // 2, act=0, residual=rd, wkey=("af", id(w)), in_affine=(sc, sh, True))
        h = ops.groupnorm_act(xd, gam.cuda(), bet.cuda(), 32, relu=True)
        two = ops.conv2d_fwd(h, wd, b.cuda(), stride=1, pad=R // 2, act=0, residual=rd, wkey=("af", id(w)))
    scale = two.abs().max().item()
    assert (got - two).abs().max().item() <= 4e-6 * scale
    ref = F.conv2d(F.relu(F.group_norm(x.double(), 32, gam.double(), bet.double())), w.double(), b.double(), padding=R // 2)
    ref = ref + (0 if res is None else res.double())
    assert _err64(got.permute(0, 3, 1, 2), ref) <= 1e-5


@pytest.mark.parametrize("per_layer", [True, False])
@pytest.mark.parametrize("stat", ["mean", "max"])
def test_adaptive_clip_in_one_launch(per_layer, stat):
    """cslgan_adaptive_clip_f32 against the chain of small ops it replaces (train.py:233-243 + :324): the adaptive statistic,
    the clip norm(s), the stacked squared norms, the clip factors (1 on the rows before first_private_row), the gathered factor rows
    of the materialised layers and the row-weight jobs."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    L, n_adapt, n_rows, first = 9, 128, 384, 256
    adapt = [(torch.rand(n_adapt, generator=g) * (3.0 + l)).cuda() for l in range(L)]
    rows = [(torch.rand(n_rows, generator=g) * (6.0 + l)).cuda() for l in range(L)]
    mat = [0, 1, 2, 5] if per_layer else []
    dsts = [torch.full((128,), -7.0, device="cuda") for _ in range(3)]
    jobs = [(dsts[0], 3, 256, 1.0 / 128), (dsts[1], 4, 256, 0.5), (dsts[2], 8, 128, 2.0)]
    r, c, sq, f, f_mat = ops.adaptive_clip(adapt, rows, stat == "max", 1.7, per_layer, 1e-6, first, mat_layers=mat, jobs=jobs)
    norms = torch.stack(adapt).sqrt()
    r_ref = norms.mean(dim=1) if stat == "mean" else norms.max(dim=1).values
    c_ref = r_ref * 1.7 if per_layer else (r_ref.norm(2) * 1.7).reshape(1)
    sq_ref = torch.stack(rows)
    f_ref = ops.clip_factors(sq_ref, c_ref.contiguous(), flat=not per_layer, eps=1e-6, first_private_row=first)
    torch.testing.assert_close(r, r_ref, rtol=2e-6, atol=0)
    torch.testing.assert_close(c, c_ref, rtol=2e-6, atol=0)
    assert torch.equal(sq, sq_ref)
    torch.testing.assert_close(f, f_ref, rtol=3e-6, atol=0)
    assert bool((f[..., :first] == 1).all())
    if per_layer:
        assert torch.equal(f_mat, f[torch.tensor(mat, device="cuda")])
    else:
        assert f_mat is None
    for dst, layer, first_row, scale in jobs:
        src = f[layer] if per_layer else f
        torch.testing.assert_close(dst, src[first_row:first_row + dst.numel()] * scale, rtol=1e-6, atol=0)


@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
def test_stride2_forward_workspace_is_packed_when_the_first_call_falls_back(mode):
    """Whether a stride-2 forward takes the halo kernel depends on its batch size (4x4 output grids need >= 2048 rows), and the
    caller's cache marks the filter workspace current after ANY call with repack = 1.  A small batch first (fallback kernel), then
    a large one on the same weight version: the second call reads the workspace with repack = 0, so the first must have packed it
    (the penalty branch's rows before the fused pass at batch sizes between 64 and 127)."""
    from csl_gan_amd import _lib
    ops = _ops()
    g = torch.Generator().manual_seed(77)
    C, K = 32, 64
    w = torch.randn(K, C, 5, 5, generator=g) / (C * 25) ** 0.5
    wd, key = _krsc(w), ("s2pack", mode)
    xs, xb = torch.randn(8, C, 8, 8, generator=g), torch.randn(128, C, 8, 8, generator=g)
    with ops.compute_dtype(mode):
        ops.conv2d_fwd(_nhwc(xs), wd, None, stride=2, pad=2, act=0, wkey=key)
        first = _lib.lib().cslgan_last_kernel().decode()
        got = ops.conv2d_fwd(_nhwc(xb), wd, None, stride=2, pad=2, act=0, wkey=key).permute(0, 3, 1, 2)
        second = _lib.lib().cslgan_last_kernel().decode()
    if mode == "bf16x3":
        assert not first.startswith("igemm_x3h_kernel") and second.startswith("igemm_x3h_kernel"), (first, second)
    ref = F.conv2d(xb.double(), w.double(), None, stride=2, padding=2)
    assert _err64(got, ref) <= 4e-6, (first, second)
