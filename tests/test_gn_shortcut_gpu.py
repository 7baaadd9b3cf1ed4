"""ResBlockUp's bn1 apply + depth-to-space shuffle + 1x1 shortcut conv in one launch (csrc/gn_shortcut.hip, -m gpu).

Kernel cases, as (N, H, W, C, K); groups = 32, bias present and absent in each:
  (2, 8, 8, 128, 64)     C/4 = 32, one statistics slot, two row tiles per image, one filter slice (kept in LDS for the walk)
  (5, 8, 8, 128, 64)     an odd number of images: 10 tiles of 32 source rows (1280 output rows, 10 tiles of the parent's 128-row kernel)
  (2, 16, 16, 128, 192)  four slots, three filter slices, eight tiles per image
  (2, 8, 8, 256, 128)    C/4 = 64
  (2, 8, 8, 512, 256)    C/4 = 128: 16-row tiles, wavefronts split the slice's filters
Block 1 of the generator (4x4 input, statistics of the statistics launch) stays on the two-launch route and has no case.

a_ps and stats_ws must equal bit for bit what cslgan_groupnorm_apply_parts_f32(d2s_W, x_shuffled) writes.  s is held against a
float64 host product of x and wf: its max abs error may be at most twice that of the parent route (apply with x_shuffled, then
cslgan_conv2d_fwd_f32 1x1) on the same inputs — two fp32 summation orders over <= 128 terms differ by an O(1) factor in rounding
error, not more.  Where the parent runs conv1x1_kernel the k-order is the same and s must be bitwise equal.  Every case prints a
`gn-shortcut-fig` line before it asserts.

Route tests (batch-2 frozen forward of the CelebA generator): the launch log shows the new kernel once per eligible block (2, 3, 4)
and one 1x1 conv (block 1) with the switch on, four 1x1 convs and no new kernel with it off or with grad enabled.  The images of the
two routes: the shortcuts differ by fp32 summation order (<= 128 terms: ~1e-6 of the activation scale), which the three remaining
blocks (a 5x5 conv over <= 3200 terms and a GroupNorm of gain <= ~10 each) and tanh (slope <= 1) carry to the image: 1e-4 abs on
values in [-1, 1] bounds it with an order of magnitude to spare; the measured figure is printed (0.0 on an MI355X: s came out
bit-identical to the two-launch route in every kernel case, errors 1.9e-6 .. 4.0e-6 against float64 on both routes).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
GROUPS = 32
CASES = [(2, 8, 8, 128, 64), (5, 8, 8, 128, 64), (2, 16, 16, 128, 192), (2, 8, 8, 256, 128), (2, 8, 8, 512, 256)]
CELEBA = ["CelebA", "-dpm", "gc", "-gcm", "adaptive-pl", "-nms", "8", "--sigma", "0.5"]


def _d2s(x):
    """ps[n][2h+i][2w+j][c'] = x[n][h][w][4c'+2i+j]"""
    N, H, W, C = x.shape
    return x.reshape(N, H, W, C // 4, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(N, 2 * H, 2 * W, C // 4)


def _partials(x, groups):
    """[N][HW/64][groups][2] float32 from float64: per 8x8-pixel slot and group, (sum, sum of squares about the slot's own mean) —
    include/cslgan.h, cslgan_conv_t.gn_part."""
    N, H, W, C = x.shape
    v = x.astype(np.float64).reshape(N, H // 8, 8, W // 8, 8, groups, C // groups)
    s = v.sum(axis=(2, 4, 6))
    m2 = ((v - v.mean(axis=(2, 4, 6), keepdims=True)) ** 2).sum(axis=(2, 4, 6))
    return np.ascontiguousarray(np.stack([s, m2], axis=-1).reshape(N, (H // 8) * (W // 8), groups, 2).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Host inputs of a case and the float64 reference of s without bias; computed once, never written to."""
    import zlib
    N, H, W, C, K = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) % 100000)
    sigma = 0.7
    off = torch.linspace(-0.5, 0.5, C)[torch.randperm(C, generator=g)]           # distinct per-channel offsets
    x = (torch.randn(N, H, W, C, generator=g) * sigma + 3 * sigma + off).contiguous()
    gamma = torch.randn(C, generator=g)
    beta = torch.randn(C, generator=g) * 0.5 + 0.25
    wf = (torch.randn(K, C // 4, generator=g) / (C // 4) ** 0.5).contiguous()
    bias = torch.randn(K, generator=g)
    part = torch.from_numpy(_partials(x.numpy(), GROUPS))
    ref = _d2s(x.numpy().astype(np.float64)) @ wf.numpy().astype(np.float64).T   # [N, 2H, 2W, K]
    return x, gamma, beta, wf, bias, part, ref


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("case", CASES)
def test_fused_equals_two_launch_route(case):
    from csl_gan_amd import _lib, ops
    N, H, W, C, K = case
    x, gamma, beta, wf, bias, part, ref0 = _inputs(case)
    dx, dg, db, dwf, dbias = (t.cuda() for t in (x, gamma, beta, wf, bias))
    dpart = (part.cuda(), part.shape[1])
    for with_bias in (True, False):
        bv = dbias if with_bias else None
        ref = ref0 + (bias.numpy().astype(np.float64) if with_bias else 0.0)
        (y0, xs), st0 = ops.groupnorm_act(dx, dg, db, GROUPS, eps=EPS, relu=True, return_stats=True, d2s=True, want_raw=True, part=dpart)
        s0 = ops.conv2d_fwd(xs, dwf.view(K, 1, 1, C // 4), bv)
        parent_kernel = _lib.lib().cslgan_last_kernel().decode()
        y1, s1, st1 = ops.groupnorm_apply_shortcut(dx, dg, db, GROUPS, dpart, dwf.view(K, 1, 1, C // 4), bv, eps=EPS, relu=True,
                                                   return_stats=True)
        assert _lib.lib().cslgan_last_kernel().decode() == "gn_shortcut_kernel<%d>" % (C // 4)
        torch.cuda.synchronize()
        e_new = float(np.abs(s1.cpu().numpy().astype(np.float64) - ref).max())
        e_par = float(np.abs(s0.cpu().numpy().astype(np.float64) - ref).max())
        same = bool(np.array_equal(_bits(s0), _bits(s1)))
        print("gn-shortcut-fig case %s bias %d: s max abs err new %.3e parent %.3e (%s) ratio %.2f bitwise %s max|s| %.2f"
              % (case, with_bias, e_new, e_par, parent_kernel, e_new / max(e_par, 1e-30), same, float(np.abs(ref).max())))
        assert np.array_equal(_bits(y0), _bits(y1)), "a_ps differs from the apply entry's"
        assert np.array_equal(_bits(st0), _bits(st1)), "stats_ws differs from the apply entry's"
        assert np.array_equal(_bits(xs), _d2s(x.numpy()).view(np.uint32))            # the parent's shortcut input is the shuffled x
        assert e_new <= 2.0 * e_par, "s: max abs error %.3e against the parent route's %.3e" % (e_new, e_par)
        if parent_kernel.startswith("conv1x1_kernel"):
            assert same, "same k-order as conv1x1_kernel, yet s differs"
    # relu off: the activation flag reaches the kernel
    y0 = ops.groupnorm_act(dx, dg, db, GROUPS, eps=EPS, relu=False, d2s=True, part=dpart)
    y1, _ = ops.groupnorm_apply_shortcut(dx, dg, db, GROUPS, dpart, dwf.view(K, 1, 1, C // 4), None, eps=EPS, relu=False)
    assert np.array_equal(_bits(y0), _bits(y1)) and float(y1.min()) < 0.0


def test_host_side_rejections():
    """Argument checks run before any launch: fake pointers are never dereferenced."""
    from csl_gan_amd import _lib
    L = _lib.lib()
    fn, err = L.cslgan_groupnorm_apply_parts_shortcut_f32, L.cslgan_last_error
    ok = dict(x=16, gamma=16, beta=16, N=2, HW=64, C=128, groups=32, eps=1e-5, relu=1, part=16, n_part=1, ws=16, y=16, W=8, wf=16, bias=None,
              K=64, s=16)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["x"], a["gamma"], a["beta"], a["N"], a["HW"], a["C"], a["groups"], a["eps"], a["relu"], a["part"], a["n_part"], a["ws"],
                  a["y"], a["W"], a["wf"], a["bias"], a["K"], a["s"], None)

    for name in ("x", "gamma", "beta", "part", "ws", "y", "wf", "s"):
        assert call(**{name: None}) == -1 and b"null" in err(), name
    assert call(C=130) == -1 and b"C % 4" in err()
    assert call(C=64, groups=16) == -1 and b"32, 64 or 128" in err()
    assert call(K=96) == -1 and b"multiple of 64" in err()
    assert call(n_part=65, HW=64 * 65) == -1 and b"n_part" in err()
    assert call(HW=128) == -1 and b"n_part" in err()
    assert call(W=7) == -1 and b"d2s_W" in err()
    assert call(x=20) == -1 and b"misaligned" in err()
    assert call(s=24) == -1 and b"misaligned" in err()


def _generator():
    from csl_gan_amd import init_util, options
    import tempfile
    opt = options.parse(CELEBA + ["-bs", "2", "-gd", "cuda:0", "-dd", "cuda:0", "-o", tempfile.mkdtemp(), "--manual_seed", "1"])
    G, _ = init_util.init_models(opt)
    return G, opt


def _forward_log(G, z, grad=False):
    """(images, kernel names of the launch log) of one generator forward."""
    from csl_gan_amd import ops
    t = ops.LaunchTimer()
    ops.set_launch_timer(t)
    try:
        with torch.enable_grad() if grad else torch.no_grad():
            img = G(z)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_timer(None)
    # 1x1 convs on an image (the first linear layer is a 1x1 conv on a 1x1 grid)
    one_by_one = sum(1 for name, *_r, tag, kernel in t.records if name == "conv2d_fwd" and tag and " R1" in tag and " 1x1 " not in tag)
    fused = sorted(kernel for name, *_r, tag, kernel in t.records if kernel.startswith("gn_shortcut_kernel"))
    streamed = sum(1 for rec in t.records if rec[7].startswith("conv1x1_kernel"))
    return img.detach(), one_by_one, fused, streamed


def test_generator_routes(monkeypatch):
    from csl_gan_amd import ops
    G, opt = _generator()
    z = torch.randn(2, opt.g_latent_dim, generator=torch.Generator().manual_seed(3)).cuda()
    assert ops._GN_SHORTCUT_FUSE
    img_on, n1_on, fused_on, streamed_on = _forward_log(G, z)
    assert fused_on == ["gn_shortcut_kernel<128>", "gn_shortcut_kernel<32>", "gn_shortcut_kernel<64>"], fused_on
    assert n1_on == 1 and streamed_on == 0, (n1_on, streamed_on)          # block 1's shortcut is the one 1x1 conv left
    _, n1_grad, fused_grad, _ = _forward_log(G, z, grad=True)
    assert fused_grad == [] and n1_grad == 4, (fused_grad, n1_grad)
    monkeypatch.setattr(ops, "_GN_SHORTCUT_FUSE", False)
    img_off, n1_off, fused_off, _ = _forward_log(G, z)
    assert fused_off == [] and n1_off == 4, (fused_off, n1_off)
    diff = float((img_on - img_off).abs().max())
    print("gn-shortcut-fig generator batch 2: max abs image difference fused vs two-launch %.3e (max |img| %.3f)"
          % (diff, float(img_off.abs().max())))
    assert torch.isfinite(img_on).all() and diff <= 1e-4


def _dstep_losses(tmp_path, tag, use_graph):
    """Trainer.last losses of the third D-step (batch 8): eager, or recorded after two eager steps and replayed.  lr = 0 keeps the
    critic bit-identical in both runs."""
    from csl_gan_amd import init_util, ops, options
    from csl_gan_amd.mean_sampler import MeanSampler
    from csl_gan_amd.trainer import GraphedDStep, Trainer
    B, shape = 8, (3, 64, 64)
    out = tmp_path / tag
    opt = options.parse(CELEBA + ["-bs", str(B), "-gd", "cuda:0", "-dd", "cuda:0", "-o", str(out), "--manual_seed", "1"])
    G, D = init_util.init_models(opt)
    ms = MeanSampler(num_samples=opt.num_mean_samples, mean_size=10, device="cuda:0", n_classes=1, res=shape[-1], ch=shape[0])
    ms.mean_samples = (torch.randn((1, opt.num_mean_samples) + shape, generator=torch.Generator().manual_seed(9)) * 0.2).cuda()
    tr = Trainer(opt, G, D, mean_sampler=ms, log_to=str(out / "log.csv"))
    tr.setup_privacy_engine()
    step = GraphedDStep(tr, use_graph=use_graph, warmup=2)
    tr.d_optimizer.param_groups[0]["lr"] = 0.0
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)
    fused = None
    for i in range(3):
        img = (torch.rand((B,) + shape, generator=g) * 2 - 1).cuda()
        if i == 0:                                   # the first eager step's launch log: the step really takes the new route
            t = ops.LaunchTimer()
            ops.set_launch_timer(t)
        step(img, None)
        if i == 0:
            ops.set_launch_timer(None)
            fused = sum(1 for rec in t.records if rec[7].startswith("gn_shortcut_kernel"))
    torch.cuda.synchronize()
    vals = {k: float(tr.last[k]) for k in ("d_real_loss", "d_fake_loss", "penalty")}
    return vals, step.graph is not None, fused


def test_replayed_dstep_equals_eager(tmp_path):
    """One replayed GraphedDStep with the switch on: the route records (no host synchronisation, no allocation the graph's pool
    cannot serve) and the losses are those of the eager step — same kernels on the same inputs, only float atomics reorder: 1e-5 of
    max(1, |value|)."""
    eager, rec_e, fused_e = _dstep_losses(tmp_path, "eager", False)
    graph, rec_g, fused_g = _dstep_losses(tmp_path, "graph", True)
    print("gn-shortcut-fig replay batch 8: eager %s graph %s" % (eager, graph))
    assert rec_g and not rec_e, "the graph was not recorded"
    assert fused_e >= 3 and fused_g >= 3, (fused_e, fused_g)
    for k in eager:
        assert abs(eager[k] - graph[k]) <= 1e-5 * max(1.0, abs(eager[k])), (k, eager[k], graph[k])
