"""The 1..4-output-channel vector-ALU conv (csrc/igemm_skinny.hip) with its filters staged once per workgroup in LDS (-m gpu):
every template form (NJ = 1..4, one class per workgroup and the all-classes form of a stride-2 data gradient) against a float64
host convolution, through the same entry points and at the same tolerance as the skinny cases of tests/test_kernels_gpu.py
(1e-4 of the output scale; 1e-5 with the folded input map, as test_groupnorm_folded_into_the_consuming_conv asks).

The shapes are the smallest that still reach every staging path: one patch whose whole halo edge is padding (8x8), several
patches per image with interior halo edges (16x16, 8x24), every LDS layout of the filter slice (K = 1: the single plane, 2 and
4: one and two pair planes, 3: both kinds), the lane-to-output map of the merged epilogue (K = 4 uses all 16 lanes of a pixel
group), and class slices of 9, 6, 6 and 4 taps replacing one another in LDS (threads past a class's taps store zero rows)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL = 1e-4              # tests/test_kernels_gpu.py::_close, the bound of its igemm_skinny cases
RTOL_AFFINE = 1e-5       # tests/test_kernels_gpu.py::test_groupnorm_folded_into_the_consuming_conv, against fp64


def _ops():
    from csl_gan_amd import ops
    return ops


def _last_kernel():
    from csl_gan_amd import _lib
    return _lib.lib().cslgan_last_kernel().decode()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _krsc(w):
    return w.permute(0, 2, 3, 1).contiguous().cuda()


def _check(got_nchw, ref64, rtol, what):
    got = got_nchw.detach().cpu().double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    scale = ref64.abs().max().item() + 1e-300
    err = (got - ref64).abs().max().item()
    print("skinny-lds %s: max abs err %.3e of scale %.3e (rel %.3e, bound %.0e)" % (what, err, scale, err / scale, rtol))
    assert err <= rtol * scale, "%s: max abs err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale)


def _act64(y, act):
    return {0: y, 1: F.leaky_relu(y, 0.2), 2: F.relu(y), 3: torch.tanh(y)}[act]


FWD_CASES = [
    # N, H, W, K, bias, act (3 = tanh)
    (2, 16, 16, 1, False, 0),
    (2, 16, 16, 2, True, 0),
    (2, 16, 16, 3, True, 3),
    (2, 16, 16, 4, False, 3),
    (1, 8, 8, 3, True, 3),          # one patch: every halo edge is padding
    (2, 8, 24, 3, True, 0),         # non-square
]


@pytest.mark.parametrize("affine", [None, "relu", "no_relu"])
@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_against_float64(case, affine):
    ops = _ops()
    N, H, W, K, has_b, act = case
    C, R = 64, 3
    g = torch.Generator().manual_seed(1000 * K + 10 * H + W + N)
    x = torch.randn(N, C, H, W, generator=g) * 2.0 + 0.5
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g) if has_b else None
    xd, wd = _nhwc(x), _krsc(w)
    bd = None if b is None else b.cuda()
    if affine is None:
        got = ops.conv2d_fwd(xd, wd, bd, stride=1, pad=1, act=act)
        xin, rtol = x.double(), RTOL
    else:
        # a per-(image, channel) map with a shift away from zero: padding applied before the map, or clamped to relu(shift),
        # would show at every border pixel
        relu = affine == "relu"
        sc = torch.rand(N, C, generator=g) + 0.5
        sh = torch.randn(N, C, generator=g) + 0.7
        assert ops.in_affine_ok(xd, wd, 1, 1)
        got = ops.conv2d_fwd(xd, wd, bd, stride=1, pad=1, act=act, in_affine=(sc.cuda(), sh.cuda(), relu))
        xin = sc.double()[:, :, None, None] * x.double() + sh.double()[:, :, None, None]
        xin = F.relu(xin) if relu else xin
        rtol = RTOL_AFFINE
    assert _last_kernel() == "igemm_skinny_kernel<%d>" % K
    ref = _act64(F.conv2d(xin, w.double(), None if b is None else b.double(), padding=1), act)
    _check(got.permute(0, 3, 1, 2), ref, rtol, "fwd %s affine %s" % (case, affine))


def test_forward_bf16_stored_input():
    """a_bf16: the halo is widened from bfloat16 on its way into LDS; the filter slice beside it is fp32 as before."""
    ops = _ops()
    N, H, W, C, K, R = 2, 16, 16, 64, 3, 3
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(N, C, H, W, generator=g)).bfloat16()
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=g)
    got = ops.conv2d_fwd(_nhwc(x), _krsc(w), b.cuda(), stride=1, pad=1, act=3)
    assert got.dtype == torch.float32 and _last_kernel() == "igemm_skinny_kernel<3>"
    ref = torch.tanh(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    _check(got.permute(0, 3, 1, 2), ref, RTOL, "fwd bf16-stored input")


@pytest.mark.parametrize("P,Q", [(8, 8), (16, 8)])
def test_first_layer_data_gradient_all_classes(P, Q):
    """The four parity classes of the 5x5 stride-2 data gradient in one workgroup: their filter slices (9, 6, 6, 4 taps) follow
    one another through the same LDS rows."""
    ops = _ops()
    N, C, K, R = 2, 3, 64, 5
    H, W = 2 * P, 2 * Q
    g = torch.Generator().manual_seed(P * 100 + Q)
    w = torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5
    gy = torch.randn(N, K, P, Q, generator=g)
    m = torch.randn(N, C, H, W, generator=g)
    x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w.double(), None, stride=2, padding=2)
    assert y.shape == (N, K, P, Q)
    ref, = torch.autograd.grad(y, x, gy.double())
    ref = ref * torch.where(m > 0, 1.0, 0.2).double()
    gx = ops.conv2d_dgrad(_nhwc(gy), _krsc(w), (H, W), stride=2, pad=2, mask=_nhwc(m))
    assert _last_kernel() == "igemm_skinny_kernel<3,all>"
    _check(gx.permute(0, 3, 1, 2), ref, RTOL, "first-layer dgrad gy %dx%d" % (P, Q))
