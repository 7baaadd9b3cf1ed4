"""Edge shapes of the normalisation kernels of csrc/norm_kernels.hip and the layout kernels of csrc/layout_kernels.hip (-m gpu): the
GroupNorm / BatchNorm forward family, its backward, the consumers of the conv epilogue's partial statistics, and the depth-to-space /
channel-fold movers, each against float64 host arithmetic written out here from the formula the kernel's comment states.  No expected value comes from
csl_gan_amd itself.

Kernel -> case (shape numbers are those of GN_SHAPES / BN_SHAPES below):
  norm_stats_kernel<true, true, float>    test_groupnorm_forward[1] (two slots, the second of 36 rows: the 4x unrolled loop runs in block 0 only),
                                          [4] (rstep 2), [7] (65535 row groups); test_batchnorm_forward[9] (five slots, tail of 44 rows), [12] (cnt 2)
  norm_stats_kernel<true, false, float>   test_groupnorm_forward[2], test_batchnorm_forward[11] (65 blocks > 64: global atomics, c4n 1 / 2)
  norm_stats_kernel<false, false, float>  test_groupnorm_forward[3] (cpg 3, tail of 17 rows), [5] (C / 4 > 256), [6] (C 8192: 64 KB of LDS),
                                          test_batchnorm_forward[10] (256 % 3 != 0, 7 blocks), test_groupnorm_unaligned (x or y 4 bytes off)
  norm_stats_kernel<true, false, bf16>    test_groupnorm_bf16[1], [2] (no scratch on the bf16 entry: atomics with 2 and 65 blocks)
  norm_stats_kernel<false, false, bf16>   test_groupnorm_bf16_routes[(2, 8, 8, 12, 3), x bf16]
  <float x, bf16 y> of both apply kernels test_groupnorm_bf16_routes[x float32] (no scratch on the bf16 entry: one statistics pass, mean = sum * (1 / n));
                                          the scalar apply kernel with bf16 x: [(2, 8, 8, 12, 3), x bf16], plain and d2s
  norm_stats_finalize_kernel              every <*, false, *> case above; the float cases run it twice (first pass: the mean as the second pass's shift)
  norm_apply_kernel<false, false>         test_groupnorm_forward[3], [5], [6], test_batchnorm_forward[10], test_groupnorm_unaligned, test_batchnorm_eval[10]
  norm_apply_kernel<false, true>          test_norm_d2s[gn 3], [bn 10] (d2s_offset per element)
  norm_apply_kernel<true, *>              not reachable below 2^32 elements per statistic: the launcher prefers norm_apply_rows_kernel
  norm_apply_rows_kernel<false>           part == nullptr: test_groupnorm_forward[2], test_batchnorm_forward[11], test_batchnorm_eval[9];
                                          part, chan 0: test_groupnorm_forward[1], [4], [7], test_batchnorm_forward[9], [12];
                                          part, chan 1: test_apply_parts (n_part 1, 8, 10, 64; groups 32 and 256)
  norm_apply_rows_kernel<true>            test_norm_d2s[gn 1], [gn (2, 3, 5, 64)] (per image, sr > 0, W != H), [bn 9] (d2s_offset branch),
                                          [bn (1, 6, 4, 64)] (BatchNorm with per_image true); chan 1: test_apply_parts[d2s]; bf16: test_groupnorm_bf16[d2s]
  bn_eval_stats_kernel                    test_batchnorm_eval (a running_var entry of exactly 0: rstd = 1 / sqrt(eps))
  bn_running_kernel                       test_batchnorm_forward[running] (momentum 0.1; 1.0 on shape 9; cnt 2: unbiased variance css / 1)
  norm_bwd_stats_kernel<true>             test_norm_backward[gn 1], [gn 4], [bn 9], [bn 12], [gn (1, 4, 4, 64, 2)], [gn (3, 2, 2, 32, 32)]; y == nullptr with relu 0
  norm_bwd_stats_kernel<false>            test_norm_backward[gn 3], [gn (1, 3, 3, 2048, 32)], [gn (1, 1, 2, 4096, 32)] (C cap: 32 KB of LDS), [bn 10],
                                          test_norm_backward_unaligned (dy 4 bytes off)
  norm_bwd_finalize_kernel                nfin = C: [gn (1, 4, 4, 64, 2)] (nrg * groups = 2 < C); nfin = nrg * groups: [gn (3, 2, 2, 32, 32)] (96 > C)
  norm_bwd_apply_kernel                   every test_norm_backward case (y of exactly +0.0 / -0.0 drops the gradient)
  gn_affine_parts_kernel                  test_affine_parts (ways 8; ways 85 with an idle thread, 256 % 3 != 0; ways 1 with groups 256; n_part 10)
  depth_to_space_kernel<false | true>     test_depth_to_space ((1, 64, 64, 516): 528384 float4 > 2048 * 256, a second grid-stride trip)
  fold_channels4_kernel<false | true>     test_fold_channels4 ((129, 5, 5, 660): 532125 > 2048 * 256)

Tolerance (forward and backward): `ref` is float64 arithmetic on the float32 (or bf16-rounded) inputs, e2 the max abs error of a plain
float32 two-pass CPU implementation (mean, centred variance, apply; float32 autograd for the backward) against ref, and the kernel must
satisfy  max |got - ref| <= 4 e2 + 16 * 2^-24 * max(1, max |ref|).  The "atypical shift" inputs (k8, k30) plant the first element k of
every statistic far from its mean and widen the bound by 1 + ((k - mean) / sigma)^2, the a-priori cancellation of S2 - S1^2 / n about
the shift k; mean and sigma are the float64 reference's, k is read from the input.  Every case prints a `norm-fig` line with its error,
e2, bound and ratio before it asserts.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = -7.25
HALF_ULP = 2.0 ** -24


def _case_seed(case):
    """Deterministic per-case seed (crc32 of the case's repr), as tests/test_kernels_gpu.py has it."""
    import zlib
    return zlib.crc32(repr(case).encode()) % 100000


def _gen(*case):
    return torch.Generator().manual_seed(_case_seed(case))


def _ops():
    from csl_gan_amd import ops
    return ops


def _f32(x):
    """The double a C float argument holds after the call: the references use the hyper-parameters the kernels see."""
    return float(np.float32(x))


EPS = _f32(1e-5)


def _dev(t):
    return t.cuda()


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _carve(t, off):
    """A device copy of t as a contiguous view that starts `off` floats into an allocation of its own, guard values on both sides:
    off = 4 is 16-byte aligned, off = 1 sits 4 bytes past a 16-byte boundary.  Returns (view, whole buffer)."""
    n = t.numel()
    buf = torch.full((n + 8,), GUARD, device="cuda", dtype=torch.float32)
    flat = buf[off:off + n]
    flat.copy_(t.reshape(-1))
    view = flat.view(t.shape)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 * off) % 16 and view.is_contiguous()
    return view, buf


def _guards_intact(buf, off, n):
    return torch.equal(buf[:off].cpu(), torch.full((off,), GUARD)) and torch.equal(buf[off + n:].cpu(), torch.full((8 - off,), GUARD))


def _within(family, what, got, ref, f32, widen=1.0):
    """The tolerance rule: max |got - ref| / (widen * (4 e2 + 16 * 2^-24 * max(1, max |ref|))) <= 1 with e2 = max |f32 - ref|; `widen`
    is 1 or the per-element atypical-shift factor.  NaN fails.  Prints the figures, returns the ratio."""
    got = _np64(got) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    f32 = _np64(f32) if torch.is_tensor(f32) else np.asarray(f32, dtype=np.float64)
    assert got.shape == ref.shape == f32.shape, (what, got.shape, ref.shape, f32.shape)
    e2 = float(np.abs(f32 - ref).max())
    plain = 4.0 * e2 + 16.0 * HALF_ULP * max(1.0, float(np.abs(ref).max()))
    err = np.abs(got - ref)
    ratio = float((err / (plain * widen)).max())
    msg = "norm-fig | %s | %s | kernel err %.3e | two-pass e2 %.3e | plain bound %.3e | widened x%.1f | err / bound %.3f" % (
        family, what, float(err.max()), e2, plain, float(np.max(widen)), ratio)
    print(msg)
    assert ratio <= 1.0, msg
    return ratio


# ---- the statistics' geometry and the two references ------------------------------------------------------------------------------
def _view(x, kind, groups):
    """[N, H, W, C] as [row groups, rows per statistic, groups, channels per group]: statistic s = row group * groups + group
    (norm_kernels.hip, "normalisation statistics over NHWC data").  BatchNorm: one row group, a group per channel."""
    N, H, W, Cc = x.shape
    return x.reshape(N, H * W, groups, Cc // groups) if kind == "gn" else x.reshape(1, N * H * W, Cc, 1)


def _moments64(x, kind, groups):
    v = _view(x.astype(np.float64), kind, groups)
    mean = v.mean(axis=(1, 3), keepdims=True)
    var = ((v - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    return mean, var


def _moments32(x, kind, groups):
    v = _view(x, kind, groups)
    mean = v.mean(dim=(1, 3), keepdim=True)
    var = (v - mean).pow(2).mean(dim=(1, 3), keepdim=True)
    return mean, var


def _apply64(x, gamma, beta, mean, var, kind, groups, relu):
    """y = act((x - mean_s) * rstd_s * gamma[c] + beta[c]), the comment above norm_apply_kernel, in float64 numpy."""
    v = _view(x.astype(np.float64), kind, groups)
    G, cpg = v.shape[2], v.shape[3]
    y = (v - mean) / np.sqrt(var + EPS) * gamma.astype(np.float64).reshape(1, 1, G, cpg) + beta.astype(np.float64).reshape(1, 1, G, cpg)
    return (np.maximum(y, 0.0) if relu else y).reshape(x.shape)


def _apply32(x, gamma, beta, mean, var, kind, groups, relu):
    v = _view(x, kind, groups)
    G, cpg = v.shape[2], v.shape[3]
    y = (v - mean) * torch.rsqrt(var + EPS) * gamma.view(1, 1, G, cpg) + beta.view(1, 1, G, cpg)
    return (torch.relu(y) if relu else y).reshape(x.shape)


def _d2s_np(a):
    """ps[n][2h+i][2w+j][c'] = x[n][h][w][4c'+2i+j] (the comment above d2s_offset in device_prims.h)."""
    N, H, W, Cc = a.shape
    out = np.empty((N, 2 * H, 2 * W, Cc // 4), dtype=a.dtype)
    for i in range(2):
        for j in range(2):
            out[:, i::2, j::2, :] = a[:, :, :, 2 * i + j::4]
    return out


KFAM = {"k8": (8.0, 2.9), "k30": (30.0, 10.8)}


def _inputs(kind, shape, groups, fam, *tag):
    """x of a data family, gamma of both signs, beta.  a: randn * 1.5 + 0.2;  b: mean 100, sigma 0.1;  c: one statistic exactly constant
    (the value of its first element), z: one statistic exactly zero, the others as a;  k8 / k30: mean 8 / 30, sigma 1, with the first
    element of every statistic (the kernel's shift) set to 2.9 / 10.8."""
    g = _gen(kind, shape, groups, fam, *tag)
    Cc = shape[-1]
    if fam == "b":
        x = torch.randn(shape, generator=g) * 0.1 + 100.0
    elif fam in KFAM:
        x = torch.randn(shape, generator=g) + KFAM[fam][0]
        _view(x, kind, groups)[:, 0, :, 0] = KFAM[fam][1]
    else:
        x = torch.randn(shape, generator=g) * 1.5 + 0.2
        v = _view(x, kind, groups)
        n_stats = v.shape[0] * v.shape[2]
        if fam == "c":
            sr, gi = divmod(min(1, n_stats - 1), v.shape[2])
            v[sr, :, gi, :] = v[sr, 0, gi, 0].item()
        elif fam == "z":
            sr, gi = divmod(n_stats - 1, v.shape[2])
            v[sr, :, gi, :] = 0.0
    gamma = torch.randn(Cc, generator=g)
    gamma[0], gamma[1] = -gamma[0].abs() - 0.1, gamma[1].abs() + 0.1
    beta = torch.randn(Cc, generator=g) * 0.5
    return g, x.contiguous(), gamma, beta


def _widen(x, mean, var, kind, groups, fam):
    """1 + ((k - mean) / sigma)^2 per statistic for the atypical-shift families, as [row groups, 1, groups, 1]; 1.0 otherwise."""
    if fam not in KFAM:
        return 1.0
    k = _view(x.numpy().astype(np.float64), kind, groups)[:, :1, :, :1]
    return 1.0 + (k - mean) ** 2 / var


def _forward_refs(x, gamma, beta, kind, groups, relu):
    m64, v64 = _moments64(x.numpy(), kind, groups)
    m32, v32 = _moments32(x, kind, groups)
    ref = _apply64(x.numpy(), gamma.numpy(), beta.numpy(), m64, v64, kind, groups, relu)
    two = _apply32(x, gamma, beta, m32, v32, kind, groups, relu)
    return ref, two, (m64, v64), (m32, v32)


def _check_stats(fam, what, stats, cnt, mom64, mom32, widen):
    """The (sum x, sum (x - mean)^2) pairs the kernels publish, as mean and biased variance (the bound scaled by cnt)."""
    st = _np64(stats).reshape(-1, 2) / cnt
    w = widen if np.isscalar(widen) else widen.reshape(-1)
    _within(fam, what + " stats mean", st[:, 0], mom64[0].reshape(-1), mom32[0].reshape(-1), w)
    _within(fam, what + " stats var", st[:, 1], mom64[1].reshape(-1), mom32[1].reshape(-1), w)


# ---- 1. GroupNorm forward -----------------------------------------------------------------------------------------------------------
GN_SHAPES = {1: (2, 10, 10, 64, 32), 2: (1, 65, 64, 4, 1), 3: (2, 9, 9, 96, 32), 4: (3, 4, 4, 512, 32), 5: (1, 3, 3, 2048, 32),
             6: (1, 1, 2, 8192, 32), 7: (65535, 1, 1, 4, 1)}
BN_SHAPES = {9: (3, 10, 10, 64), 10: (5, 9, 9, 12), 11: (1, 65, 64, 8), 12: (2, 1, 1, 4)}
GN_CASES = [(s, f) for s in GN_SHAPES for f in "abcz"] + [(s, f) for s in (1, 2) for f in KFAM]


@pytest.mark.parametrize("shape_no,fam", GN_CASES)
def test_groupnorm_forward(shape_no, fam):
    """ops.groupnorm_act, relu off and on, y and the returned statistics against float64."""
    ops = _ops()
    shape, groups = GN_SHAPES[shape_no][:4], GN_SHAPES[shape_no][4]
    _, x, gamma, beta = _inputs("gn", shape, groups, fam)
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    cnt = shape[1] * shape[2] * (shape[3] // groups)
    for relu in (False, True):
        ref, two, m64, m32 = _forward_refs(x, gamma, beta, "gn", groups, relu)
        widen = _widen(x, m64[0], m64[1], "gn", groups, fam)
        y, stats = ops.groupnorm_act(_dev(x), _dev(gamma), _dev(beta), groups, eps=EPS, relu=relu, return_stats=True)
        we = widen if np.isscalar(widen) else np.broadcast_to(widen, _view(ref, "gn", groups).shape).reshape(ref.shape)
        what = "gn %d relu %d" % (shape_no, relu)
        _within("gn fwd " + fam, what + " y", y, ref, two, we)
        _check_stats("gn fwd " + fam, what, stats, cnt, m64, m32, widen)


def _gn_raw(xv, gamma, beta, shape, groups, relu, yv):
    """cslgan_groupnorm_act_f32 on caller-placed x and y (ops.groupnorm_act allocates y itself, aligned)."""
    ops = _ops()
    from csl_gan_amd import _lib
    N, H, W, Cc = shape
    ws = torch.empty(2 * N * groups, device="cuda", dtype=torch.float32)
    sc = ops._scratch(xv.device, 2 * N * groups)
    ops.check(_lib.lib().cslgan_groupnorm_act_f32(ops._p(xv), ops._p(gamma), ops._p(beta), N, H * W, Cc, groups, EPS, 1 if relu else 0, ops._p(ws),
                                                  ops._p(yv), 0, None, ops._p(sc), ops._stream()), "groupnorm_act")
    return ws


@pytest.mark.parametrize("x_off,y_off", [(1, 4), (4, 1), (1, 1)])
def test_groupnorm_unaligned(x_off, y_off):
    """Shape 1 with x, y or both 4 bytes past a 16-byte boundary: the scalar kernels must be taken; the guard floats around x and y
    are intact after every call."""
    shape, groups = GN_SHAPES[1][:4], GN_SHAPES[1][4]
    _, x, gamma, beta = _inputs("gn", shape, groups, "a", "unaligned")
    dg, db = _dev(gamma), _dev(beta)
    for relu in (False, True):
        ref, two, _, _ = _forward_refs(x, gamma, beta, "gn", groups, relu)
        xv, xbuf = _carve(x, x_off)
        yv, ybuf = _carve(torch.zeros(shape), y_off)
        _gn_raw(xv, dg, db, shape, groups, relu, yv)
        _within("gn fwd unaligned", "x off %d y off %d relu %d" % (x_off, y_off, relu), yv, ref, two)
        assert _guards_intact(xbuf, x_off, x.numel()) and _guards_intact(ybuf, y_off, x.numel())
        assert torch.equal(xv.cpu(), x)


def test_groupnorm_caps_rejected():
    """C = 8196 (past the 64 KB of LDS) and N = 65536 (past grid.y) come back as errors, not launches."""
    ops = _ops()
    for shape, groups in (((1, 1, 1, 8196), 4), ((65536, 1, 1, 4), 1)):
        x = torch.zeros(shape, device="cuda")
        with pytest.raises(RuntimeError, match="too large"):
            ops.groupnorm_act(x, torch.ones(shape[3], device="cuda"), torch.zeros(shape[3], device="cuda"), groups, eps=EPS)
    x = torch.zeros((1, 1, 1, 8196), device="cuda")
    with pytest.raises(RuntimeError, match="bad sizes"):
        ops.batchnorm_act(x, torch.ones(8196, device="cuda"), torch.zeros(8196, device="cuda"))


# ---- 2. BatchNorm forward, training and eval --------------------------------------------------------------------------------------
BN_CASES = [(s, f, r) for s in BN_SHAPES for f in "abcz" for r in (None, 0.1)] + [(9, f, r) for f in KFAM for r in (None, 0.1)] + [(9, "a", 1.0)]


@pytest.mark.parametrize("shape_no,fam,momentum", BN_CASES)
def test_batchnorm_forward(shape_no, fam, momentum):
    """ops.batchnorm_act in training mode, relu off and on, without (momentum None) and with running statistics:
    running = (1 - momentum) running + momentum (mean, css / (cnt - 1))."""
    ops = _ops()
    shape = BN_SHAPES[shape_no]
    Cc = shape[3]
    g, x, gamma, beta = _inputs("bn", shape, Cc, fam, momentum)
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    cnt = shape[0] * shape[1] * shape[2]
    for relu in (False, True):
        ref, two, m64, m32 = _forward_refs(x, gamma, beta, "bn", Cc, relu)
        widen = _widen(x, m64[0], m64[1], "bn", Cc, fam)
        rm, rv = (_dev(rm0), _dev(rv0)) if momentum is not None else (None, None)
        y, stats = ops.batchnorm_act(_dev(x), _dev(gamma), _dev(beta), rm, rv, momentum=0.1 if momentum is None else momentum, eps=EPS,
                                     relu=relu, return_stats=True)
        we = widen if np.isscalar(widen) else np.broadcast_to(widen.reshape(1, 1, 1, Cc), ref.shape)
        what = "bn %d relu %d momentum %s" % (shape_no, relu, momentum)
        _within("bn fwd " + fam, what + " y", y, ref, two, we)
        _check_stats("bn fwd " + fam, what, stats, cnt, m64, m32, widen)
        if momentum is not None:
            mo = _f32(momentum)
            w = widen if np.isscalar(widen) else widen.reshape(-1)
            unb = cnt / (cnt - 1.0)
            _within("bn fwd " + fam, what + " running_mean", rm, (1 - mo) * rm0.numpy().astype(np.float64) + mo * m64[0].reshape(-1),
                    (1 - mo) * rm0 + mo * m32[0].reshape(-1), w)
            _within("bn fwd " + fam, what + " running_var", rv, (1 - mo) * rv0.numpy().astype(np.float64) + mo * unb * m64[1].reshape(-1),
                    (1 - mo) * rv0 + mo * (m32[1].reshape(-1) * cnt / (cnt - 1.0)), w)


@pytest.mark.parametrize("zero_var", [False, True])
@pytest.mark.parametrize("shape_no", [9, 10])
def test_batchnorm_eval(shape_no, zero_var):
    """ops.batchnorm_eval_act: y = act((x - running_mean) rsqrt(running_var + eps) gamma + beta); zero_var: one running_var entry is
    exactly 0, so rstd = 1 / sqrt(eps)."""
    ops = _ops()
    shape = BN_SHAPES[shape_no]
    Cc = shape[3]
    g, x, gamma, beta = _inputs("bn", shape, Cc, "a", "eval", zero_var)
    rm, rv = torch.randn(Cc, generator=g) * 0.5 + 0.2, torch.rand(Cc, generator=g) + 0.5
    if zero_var:
        rv[2] = 0.0
    m64 = (rm.numpy().astype(np.float64).reshape(1, 1, Cc, 1), rv.numpy().astype(np.float64).reshape(1, 1, Cc, 1))
    m32 = (rm.view(1, 1, Cc, 1), rv.view(1, 1, Cc, 1))
    for relu in (False, True):
        ref = _apply64(x.numpy(), gamma.numpy(), beta.numpy(), m64[0], m64[1], "bn", Cc, relu)
        two = _apply32(x, gamma, beta, m32[0], m32[1], "bn", Cc, relu)
        y = ops.batchnorm_eval_act(_dev(x), _dev(gamma), _dev(beta), _dev(rm), _dev(rv), eps=EPS, relu=relu)
        _within("bn eval", "bn eval %d relu %d zero_var %d" % (shape_no, relu, zero_var), y, ref, two)


# ---- 3. the fused depth-to-space output -------------------------------------------------------------------------------------------
D2S_CASES = [("gn",) + GN_SHAPES[1], ("gn",) + GN_SHAPES[3], ("gn", 2, 3, 5, 64, 32),
             ("bn",) + BN_SHAPES[9] + (0,), ("bn",) + BN_SHAPES[10] + (0,), ("bn", 1, 6, 4, 64, 0)]


@pytest.mark.parametrize("case", D2S_CASES)
def test_norm_d2s(case):
    """d2s=True, want_raw=True: y is the float64 output permuted by the index formula, the raw copy is x under the same permutation bit
    for bit."""
    ops = _ops()
    kind, shape = case[0], case[1:5]
    groups = case[5] if kind == "gn" else shape[3]
    _, x, gamma, beta = _inputs(kind, shape, groups, "a", "d2s")
    for relu in (False, True):
        ref, two, _, _ = _forward_refs(x, gamma, beta, kind, groups, relu)
        if kind == "gn":
            y, xs = ops.groupnorm_act(_dev(x), _dev(gamma), _dev(beta), groups, eps=EPS, relu=relu, d2s=True, want_raw=True)
        else:
            y, xs = ops.batchnorm_act(_dev(x), _dev(gamma), _dev(beta), None, None, eps=EPS, relu=relu, d2s=True, want_raw=True)
        assert tuple(y.shape) == (shape[0], 2 * shape[1], 2 * shape[2], shape[3] // 4)
        _within("d2s " + kind, "%s relu %d" % (case, relu), y, _d2s_np(ref), _d2s_np(two.numpy()))
        assert np.array_equal(xs.cpu().numpy().view(np.uint32), _d2s_np(x.numpy()).view(np.uint32))


# ---- 4. bf16 storage ----------------------------------------------------------------------------------------------------------------
def _rne_bf16(a):
    """float64 -> the nearest bfloat16 (ties to even), as float64."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def _check_groupnorm_bf16(what, shape, groups, x_bf16, d2s):
    """ops.groupnorm_act with a bf16 output on x stored as bf16 (x_bf16) or as float32, under test_groupnorm_bf16's rule; the raw
    shuffled copy is x rounded to nearest-even bf16 (x itself where it is stored as bf16), bit for bit."""
    ops = _ops()
    _, x, gamma, beta = _inputs("gn", shape, groups, "a", "bf16")
    xb = x.to(torch.bfloat16)
    if x_bf16:
        x = xb.float()
    for relu in (False, True):
        ref, two, _, _ = _forward_refs(x, gamma, beta, "gn", groups, relu)
        two = two.numpy().astype(np.float64)
        if d2s:
            y, xs = ops.groupnorm_act(_dev(xb if x_bf16 else x), _dev(gamma), _dev(beta), groups, eps=EPS, relu=relu, d2s=True, want_raw=True,
                                      out_dtype=torch.bfloat16)
            ref, two = _d2s_np(ref), _d2s_np(two)
            assert xs.dtype == torch.bfloat16
            assert np.array_equal(xs.float().cpu().numpy().view(np.uint32), _d2s_np(_rne_bf16(x.numpy()).astype(np.float32)).view(np.uint32))
        else:
            y = ops.groupnorm_act(_dev(xb if x_bf16 else x), _dev(gamma), _dev(beta), groups, eps=EPS, relu=relu, out_dtype=torch.bfloat16)
        assert y.dtype == torch.bfloat16
        got = _np64(y)
        e2 = float(np.abs(two - ref).max())
        bound = 4.0 * e2 + 16.0 * HALF_ULP * max(1.0, float(np.abs(ref).max()))
        exact = got == _rne_bf16(ref)
        ok = exact | ((got >= _rne_bf16(ref - bound)) & (got <= _rne_bf16(ref + bound)))
        used = 1.0 - float(exact.mean())
        msg = "norm-fig | gn bf16 | %s d2s %d relu %d | %d of %d outside the allowance | two-pass e2 %.3e | bound %.3e | allowance used by %.4f%%" % (
            what, d2s, relu, int((~ok).sum()), ok.size, e2, bound, 100 * used)
        print(msg)
        assert bool(ok.all()), "%s | first offender: ref %.9e, got %.9e" % (msg, ref[~ok][0], got[~ok][0])
        assert used <= 0.01, msg


@pytest.mark.parametrize("d2s", [False, True])
@pytest.mark.parametrize("shape_no", [1, 2])
def test_groupnorm_bf16(shape_no, d2s):
    """bf16 x and bf16 y: the result is the float64 reference (on the bf16-rounded inputs) rounded to nearest-even bf16; an element
    may sit one bf16 step away only where the reference lies within the float32 bound of a rounding boundary, and at most 1% of the
    elements may use that allowance.

    The allowance is written as an interval: got must be the bf16 rounding of SOME value within the float32 bound of the reference,
    rne(ref - bound) <= got <= rne(ref + bound).  Away from zero a bf16 step is 2^12 bounds wide and this is "one step, next to a
    boundary"; for the few outputs with |y| < 2e-3 the bf16 grid is finer than the float32 bound, and a result inside the float32 bound
    can be several (tiny) bf16 steps from the reference's rounding (shape 1 has one output of 3.9e-6: a bf16 step of 3e-8 there, under
    the float32 ulp of the sum that produces it).  On an MI355X 0 - 0.03% of the elements used the allowance."""
    _check_groupnorm_bf16("gn %d" % shape_no, GN_SHAPES[shape_no][:4], GN_SHAPES[shape_no][4], True, d2s)


BF16_ROUTE_SHAPES = [(2, 8, 8, 8, 2), (2, 8, 8, 12, 3)]


@pytest.mark.parametrize("d2s", [False, True])
@pytest.mark.parametrize("x_bf16", [False, True])
@pytest.mark.parametrize("case", BF16_ROUTE_SHAPES)
def test_groupnorm_bf16_routes(case, x_bf16, d2s):
    """The bf16 entry on the smallest shapes of its two routes, x stored as float32 and as bf16, under test_groupnorm_bf16's rule:
    C = 8 takes the 16-byte kernels, C = 12 (256 % 3 != 0) the scalar ones."""
    _check_groupnorm_bf16("%s x_bf16 %d" % (case, x_bf16), case[:4], case[4], x_bf16, d2s)


# ---- 5. the consumers of the conv epilogue's partial statistics ----------------------------------------------------------------------
def _partials(x3, groups, n_part):
    """[N][n_part][groups][2] float32 from float64: per slot of 64 consecutive rows and group, (sum, sum of squares about the slot's
    own mean) — include/cslgan.h, cslgan_conv_t.gn_part."""
    N, HW, Cc = x3.shape
    v = x3.astype(np.float64).reshape(N, n_part, 64, groups, Cc // groups)
    s = v.sum(axis=(2, 4))
    m2 = ((v - v.mean(axis=(2, 4), keepdims=True)) ** 2).sum(axis=(2, 4))
    return np.stack([s, m2], axis=-1).astype(np.float32)


def _combine(part, cnt, dt):
    """Chan's combination the consumers' comments state: mean = sum_b S_b / cnt, M2 = sum_b M2_b + n_b (S_b / n_b - mean)^2, in `dt`."""
    p = part.astype(dt)
    n_part = p.shape[1]
    nb = dt(cnt) / dt(n_part)
    mean = p[..., 0].sum(axis=1, dtype=dt) / dt(cnt)                       # [N, groups]
    dm = p[..., 0] / nb - mean[:, None, :]
    css = (p[..., 1] + nb * dm * dm).sum(axis=1, dtype=dt)
    return mean, css / dt(cnt)


def _parts_x(N, HW, Cc, fam, g):
    return torch.randn(N, HW, Cc, generator=g) * (0.1 if fam == "b" else 1.5) + (100.0 if fam == "b" else 0.2)


AFFINE_CASES = [(2, 64, 64, 32, 1), (3, 192, 12, 3, 3), (1, 4096, 256, 256, 64), (2, 640, 128, 32, 10)]


@pytest.mark.parametrize("fam", ["a", "b"])
@pytest.mark.parametrize("case", AFFINE_CASES)
def test_affine_parts(case, fam):
    """ops.groupnorm_affine on partials built here: scale = gamma rstd, shift = beta - mean scale; e2 is the float32 host evaluation of
    the same formulas."""
    ops = _ops()
    N, HW, Cc, groups, n_part = case
    g = _gen("affine_parts", case, fam)
    x = _parts_x(N, HW, Cc, fam, g)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.5
    gamma[0], gamma[1] = -gamma[0].abs() - 0.1, gamma[1].abs() + 0.1
    part = _partials(x.numpy(), groups, n_part)
    cpg = Cc // groups
    sc, sh = ops.groupnorm_affine((_dev(torch.from_numpy(part)), n_part), _dev(gamma), _dev(beta), groups, EPS, N, HW, Cc)
    out = {}
    for dt in (np.float64, np.float32):
        mean, var = _combine(part, HW * cpg, dt)
        rstd = dt(1.0) / np.sqrt(var + dt(EPS))
        scale = gamma.numpy().astype(dt)[None, :] * np.repeat(rstd, cpg, axis=1)
        shift = beta.numpy().astype(dt)[None, :] - np.repeat(mean, cpg, axis=1) * scale
        assert scale.dtype == dt and shift.dtype == dt
        out[dt] = (scale, shift)
    _within("affine parts " + fam, "%s scale" % (case,), sc, out[np.float64][0], out[np.float32][0])
    _within("affine parts " + fam, "%s shift" % (case,), sh, out[np.float64][1], out[np.float32][1])


APPLY_CASES = [(2, 8, 8, 64, 32, 1), (1, 64, 64, 256, 256, 64), (2, 20, 32, 128, 32, 10), (1, 16, 32, 1024, 256, 8)]


@pytest.mark.parametrize("d2s", [False, True])
@pytest.mark.parametrize("fam", ["a", "b"])
@pytest.mark.parametrize("case", APPLY_CASES)
def test_apply_parts(case, fam, d2s):
    """ops.groupnorm_act(part=...): the apply launch alone, its statistics combined from partials built here (chan = 1); y, and the
    (sum, centred sum of squares) pairs the first workgroup of every image publishes."""
    ops = _ops()
    N, H, W, Cc, groups, n_part = case
    g = _gen("apply_parts", case, fam)
    x = _parts_x(N, H * W, Cc, fam, g).view(N, H, W, Cc)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.5
    gamma[0], gamma[1] = -gamma[0].abs() - 0.1, gamma[1].abs() + 0.1
    part = _partials(x.numpy().reshape(N, H * W, Cc), groups, n_part)
    cnt = H * W * (Cc // groups)
    m64 = [a.reshape(N, 1, groups, 1) for a in _combine(part, cnt, np.float64)]
    m32 = [torch.from_numpy(a).view(N, 1, groups, 1) for a in _combine(part, cnt, np.float32)]
    dpart = _dev(torch.from_numpy(part))
    for relu in (False, True):
        ref = _apply64(x.numpy(), gamma.numpy(), beta.numpy(), m64[0], m64[1], "gn", groups, relu)
        two = _apply32(x, gamma, beta, m32[0], m32[1], "gn", groups, relu).numpy()
        if d2s:
            (y, xs), stats = ops.groupnorm_act(_dev(x), _dev(gamma), _dev(beta), groups, eps=EPS, relu=relu, return_stats=True, d2s=True,
                                               want_raw=True, part=(dpart, n_part))
            ref, two = _d2s_np(ref), _d2s_np(two)
            assert np.array_equal(xs.cpu().numpy().view(np.uint32), _d2s_np(x.numpy()).view(np.uint32))
        else:
            y, stats = ops.groupnorm_act(_dev(x), _dev(gamma), _dev(beta), groups, eps=EPS, relu=relu, return_stats=True, part=(dpart, n_part))
        what = "%s d2s %d relu %d" % (case, d2s, relu)
        _within("apply parts " + fam, what + " y", y, ref, two)
        _check_stats("apply parts " + fam, what, stats, cnt, m64, [a.numpy() for a in m32], 1.0)


def test_parts_rejected():
    """n_part = 65 (past CSLGAN_NORM_PARTIAL_BLOCKS) and HW != 64 n_part come back as errors from the library's checks."""
    ops = _ops()
    gamma, beta = torch.ones(4, device="cuda"), torch.zeros(4, device="cuda")
    x = torch.zeros(1, 65, 64, 4, device="cuda")
    part = torch.zeros(1, 65, 1, 2, device="cuda")
    with pytest.raises(RuntimeError, match="n_part"):
        ops.groupnorm_act(x, gamma, beta, 1, eps=EPS, part=(part, 65))
    with pytest.raises(RuntimeError, match="n_part"):
        ops.groupnorm_act(x[:, :10].contiguous(), gamma, beta, 1, eps=EPS, part=(part, 9))          # HW = 640 is not 64 * 9
    with pytest.raises(RuntimeError, match="n_part"):
        ops.groupnorm_affine((part, 9), gamma, beta, 1, EPS, 1, 640, 4)


# ---- 6. the backward -----------------------------------------------------------------------------------------------------------------
def _stats32(x, kind, groups):
    """The forward's `stats` output built from float64: (sum x, centred sum of squares) per statistic, rounded to float32."""
    v = _view(x.numpy().astype(np.float64), kind, groups)
    mean = v.mean(axis=(1, 3), keepdims=True)
    return np.stack([v.sum(axis=(1, 3)), ((v - mean) ** 2).sum(axis=(1, 3))], axis=-1).astype(np.float32)        # [row groups, groups, 2]


def _bwd64(x, dy, mask, gamma, stats, kind, groups):
    """The backward's formulas (the comment above norm_bwd_stats_kernel in norm_kernels.hip) in float64 numpy, on the statistics
    the kernel is handed."""
    v = _view(x.numpy().astype(np.float64), kind, groups)
    gp = _view(dy.numpy().astype(np.float64) * mask, kind, groups)
    nrg, R, G, cpg = v.shape
    cnt = float(R * cpg)
    st = stats.astype(np.float64).reshape(nrg, 1, G, 1, 2)
    mean, rstd = st[..., 0] / cnt, 1.0 / np.sqrt(st[..., 1] / cnt + EPS)
    xh = (v - mean) * rstd
    A, Bq = gp.sum(axis=1), (gp * xh).sum(axis=1)                             # [row groups, G, cpg]
    gam = gamma.numpy().astype(np.float64).reshape(1, G, cpg)
    s1, s2 = (gam * A).sum(axis=-1), (gam * Bq).sum(axis=-1)                  # [row groups, G]
    dx = rstd * (gam[:, None] * gp - s1[:, None, :, None] / cnt - xh * s2[:, None, :, None] / cnt)
    return dx.reshape(x.shape), Bq.sum(axis=0).reshape(-1), A.sum(axis=0).reshape(-1)


def _bwd32(x, dy, mask, gamma, beta, kind, groups):
    """float32 CPU autograd through the two-pass forward: the source of e2 only."""
    xt, gt, bt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    mean, var = _moments32(xt, kind, groups)
    out = _apply32(xt, gt, bt, mean, var, kind, groups, False)
    return torch.autograd.grad((out * torch.from_numpy(mask.astype(np.float32)) * dy).sum(), (xt, gt, bt))


def _bwd_inputs(kind, shape, groups, fam, relu, *tag):
    g, x, gamma, beta = _inputs(kind, shape, groups, fam, "bwd", relu, *tag)
    dy = torch.randn(shape, generator=g)
    if not relu:
        return x, gamma, beta, dy, None, np.ones(shape)
    m64, v64 = _moments64(x.numpy(), kind, groups)
    y = torch.from_numpy(_apply64(x.numpy(), gamma.numpy(), beta.numpy(), m64, v64, kind, groups, True).astype(np.float32))
    n = y.numel()
    idx = torch.randperm(n, generator=g)[:max(2, n // 100)]
    y.view(-1)[idx[0::2]] = 0.0                                               # about 1% of the outputs exactly +0.0 / -0.0: no gradient
    y.view(-1)[idx[1::2]] = -0.0
    mask = (y.numpy() > 0)
    assert 0 < mask.sum() < n and not mask.reshape(-1)[idx.numpy()].any()
    return x, gamma, beta, dy, y, mask.astype(np.float64)


def _check_bwd(family, what, got, x, dy, mask, gamma, beta, stats, kind, groups):
    refs = _bwd64(x, dy, mask, gamma, stats, kind, groups)
    twos = _bwd32(x, dy, mask, gamma, beta, kind, groups)
    for name, a, r, t in zip(("dx", "dgamma", "dbeta"), got, refs, twos):
        _within(family, "%s %s" % (what, name), a, r, t)


BWD_CASES = [("gn",) + GN_SHAPES[1], ("gn",) + GN_SHAPES[3], ("gn",) + GN_SHAPES[4], ("gn", 1, 3, 3, 2048, 32), ("gn", 1, 1, 2, 4096, 32),
             ("bn",) + BN_SHAPES[9] + (0,), ("bn",) + BN_SHAPES[10] + (0,), ("bn",) + BN_SHAPES[12] + (0,), ("gn", 1, 4, 4, 64, 2), ("gn", 3, 2, 2, 32, 32)]


@pytest.mark.parametrize("fam", ["a", "b", "c", "z"])
@pytest.mark.parametrize("case", BWD_CASES)
def test_norm_backward(case, fam):
    """ops.norm_act_bwd on statistics and a forward output built here: dx, dgamma, dbeta; relu off passes y = None."""
    ops = _ops()
    kind, shape = case[0], case[1:5]
    groups = case[5] if kind == "gn" else shape[3]
    rps = shape[1] * shape[2] if kind == "gn" else shape[0] * shape[1] * shape[2]
    for relu in (False, True):
        x, gamma, beta, dy, y, mask = _bwd_inputs(kind, shape, groups, fam, relu)
        stats = _stats32(x, kind, groups)
        got = ops.norm_act_bwd(_dev(x), _dev(dy), _dev(y) if relu else None, _dev(gamma), _dev(torch.from_numpy(stats).reshape(-1)), rps, groups, EPS,
                               relu)
        _check_bwd("bwd " + fam, "%s relu %d" % (case, relu), got, x, dy, mask, gamma, beta, stats, kind, groups)


@pytest.mark.parametrize("kind", ["gn", "bn"])
def test_norm_backward_forward_stats(kind):
    """The backward on the statistics the forward kernel returns (shape 1 / 9) meets the same bound."""
    ops = _ops()
    shape, groups = (GN_SHAPES[1][:4], 32) if kind == "gn" else (BN_SHAPES[9], 64)
    rps = shape[1] * shape[2] if kind == "gn" else shape[0] * shape[1] * shape[2]
    x, gamma, beta, dy, y, mask = _bwd_inputs(kind, shape, groups, "a", True, "forward stats")
    if kind == "gn":
        _, stats = ops.groupnorm_act(_dev(x), _dev(gamma), _dev(beta), groups, eps=EPS, relu=True, return_stats=True)
    else:
        _, stats = ops.batchnorm_act(_dev(x), _dev(gamma), _dev(beta), None, None, eps=EPS, relu=True, return_stats=True)
    got = ops.norm_act_bwd(_dev(x), _dev(dy), _dev(y), _dev(gamma), stats, rps, groups, EPS, True)
    _check_bwd("bwd forward stats", kind, got, x, dy, mask, gamma, beta, stats.cpu().numpy(), kind, groups)


@pytest.mark.parametrize("relu", [False, True])
def test_norm_backward_unaligned(relu):
    """Shape 1 with dy 4 bytes past a 16-byte boundary (the scalar statistics kernel) and dx inside guard floats."""
    ops = _ops()
    from csl_gan_amd import _lib
    shape, groups = GN_SHAPES[1][:4], 32
    N, H, W, Cc = shape
    x, gamma, beta, dy, y, mask = _bwd_inputs("gn", shape, groups, "a", relu, "unaligned")
    stats = _stats32(x, "gn", groups)
    dyv, dybuf = _carve(dy, 1)
    dxv, dxbuf = _carve(torch.zeros(shape), 4)
    L = _lib.lib()
    ws = torch.empty(L.cslgan_norm_bwd_ws_floats(N * H * W, H * W, Cc, groups), device="cuda", dtype=torch.float32)
    dgamma, dbeta = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
    xd, yd, gd, sd = _dev(x), (_dev(y) if relu else None), _dev(gamma), _dev(torch.from_numpy(stats).reshape(-1))       # alive over the call
    ops.check(L.cslgan_norm_act_bwd_f32(ops._p(xd), ops._p(dyv), ops._p(yd), ops._p(gd), ops._p(sd), N * H * W, H * W, Cc, groups, EPS,
                                        1 if relu else 0, ops._p(ws), ops._p(dxv), ops._p(dgamma), ops._p(dbeta), ops._stream()), "norm_act_bwd")
    torch.cuda.synchronize()
    _check_bwd("bwd unaligned", "relu %d" % relu, (dxv, dgamma, dbeta), x, dy, mask, gamma, beta, stats, "gn", groups)
    assert _guards_intact(dybuf, 1, dy.numel()) and _guards_intact(dxbuf, 4, dy.numel())


def test_norm_backward_rejects(monkeypatch):
    """C = 4100 (past the backward's cap of 4096) is an error of the library; a non-contiguous y is refused in Python, before the
    library is reached."""
    ops = _ops()
    x = torch.zeros(1, 1, 1, 4100, device="cuda")
    with pytest.raises(RuntimeError, match="bad sizes"):
        ops.norm_act_bwd(x, x, None, torch.ones(4100, device="cuda"), torch.zeros(8, device="cuda"), 1, 4, EPS, False)
    x = torch.zeros(2, 4, 4, 8, device="cuda")
    y = torch.zeros(2, 4, 8, 4, device="cuda").transpose(2, 3)
    assert y.shape == x.shape and not y.is_contiguous()
    reached = []
    monkeypatch.setattr(ops._lib, "lib", lambda: reached.append(1) or pytest.fail("the library was reached"))
    with pytest.raises(RuntimeError, match="y must be contiguous"):
        ops.norm_act_bwd(x, x, y, torch.ones(8, device="cuda"), torch.zeros(8, device="cuda"), 16, 2, EPS, True)
    assert not reached


# ---- 7. the layout movers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 1, 1, 4), (1, 64, 64, 516)])
def test_depth_to_space(shape):
    """ops.depth_to_space forward and inverse against the index formula, bit for bit; the inverse of the forward is the identity."""
    ops = _ops()
    g = _gen("depth_to_space", shape)
    x = torch.randn(shape, generator=g)
    ps = ops.depth_to_space(_dev(x))
    assert np.array_equal(ps.cpu().numpy().view(np.uint32), _d2s_np(x.numpy()).view(np.uint32))
    assert torch.equal(ops.depth_to_space(ps, inverse=True).cpu(), x)
    N, H, W, Cc = shape
    q = torch.randn(N, 2 * H, 2 * W, Cc // 4, generator=g)
    back = ops.depth_to_space(_dev(q), inverse=True).cpu()
    assert back.shape == x.shape
    assert np.array_equal(_d2s_np(back.numpy()).view(np.uint32), q.numpy().view(np.uint32))


@pytest.mark.parametrize("shape", [(3, 5, 5, 8), (1, 1, 1, 4), (129, 5, 5, 660)])
def test_fold_channels4(shape):
    """fold = (b0 + b1) + (b2 + b3) in float32, in that order, bit for bit (with a fresh cache key and without one); unfold copies
    exactly; <unfold(g), w> = <g, fold(w)> up to the three float32 roundings of a folded element."""
    ops = _ops()
    g = _gen("fold_channels4", shape)
    w = torch.randn(shape, generator=g)
    Cq = shape[3] // 4
    b = [w.numpy()[..., q * Cq:(q + 1) * Cq] for q in range(4)]
    want = (b[0] + b[1]) + (b[2] + b[3])
    assert want.dtype == np.float32
    dw = _dev(w)
    for key in (None, object()):
        wf = ops.fold_channels4(dw, wkey=key)
        assert np.array_equal(wf.cpu().numpy().view(np.uint32), want.view(np.uint32))
    gq = torch.randn(shape[:3] + (Cq,), generator=g)
    gw = ops.unfold_channels4(_dev(gq)).cpu()
    assert gw.shape == w.shape
    for q in range(4):
        assert torch.equal(gw[..., q * Cq:(q + 1) * Cq], gq)
    lhs = float((gw.double() * w.double()).sum())
    rhs = float((gq.double() * wf.cpu().double()).sum())
    slack = 3 * HALF_ULP * float((gq.double().abs() * sum(torch.from_numpy(np.abs(p)).double() for p in b)).sum()) + 1e-12 * abs(lhs)
    assert abs(lhs - rhs) <= slack, "adjoint: %.17g vs %.17g, slack %.3e" % (lhs, rhs, slack)
