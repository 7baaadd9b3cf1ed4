"""Edge shapes of the D-step's small kernels (-m gpu): csrc/step_kernels.hip (the Adam kernels among them), the row helpers of
csrc/clip_kernels.hip and the act_bwd kernel of csrc/cast_kernels.hip, each against float64 host arithmetic written out here from the reference line the
kernel's comment cites.  The shapes are the smallest that reach a second loop trip, a second workgroup, the scalar (unaligned or
len % 4 != 0) branches, the grid caps and rows of exactly zero.  No expected value comes from csl_gan_amd itself.

Kernel -> case:
  segment_means_kernel         test_segment_means_forward (blocks of 300 / 257 / 513 / 511 rows: second trip, red[] reused 8 times)
  segment_means_bwd_kernel     test_segment_means_backward (558 .. 1646 rows: 3 .. 7 workgroups; g_total / g_vec / both)
  dstep_stats_kernel           test_dstep_stats (300 real, 257 fake logits, +-0.0 planted, penalty None / tensor, two calls)
  grad_log_stats_kernel        test_grad_log_stats (B 1 / 257 / 300, col0 0 and > 0, L 1 / 9, per layer and flat)
  adaptive_clip_kernel         test_adaptive_clip, test_adaptive_clip_job_without_rows
  lerp_rows_kernel             test_lerp_rows (105 scalar, 768, 66564 second float4 trip, 66565 scalar trips under the 64 cap)
  lipschitz_term_kernel        test_lipschitz_term (1 row, 300 rows, unaligned float4-length rows), test_lipschitz_ticket_sequence
  lipschitz_term_bwd_kernel    test_lipschitz_term (grid cap at 66564, unaligned fallback), test_lipschitz_zero_rows
  sample_sqnorm_kernel<float>  test_sample_sqnorm_unaligned_segments (len % 4 == 0 rows 4 bytes off, 18 segments: two launches)
  clip_factors_kernel          test_clip_factors (129 / 300 rows: 2 / 3 workgroups, first private row 0 / 128 / n_rows, zero norm)
  sqrt_kernel                  test_row_l2norm (300 rows: 3 workgroups)
  row_l2norm_bwd_kernel        test_row_l2norm (66565: five trips under the 64 cap; zero row)
  l2_clip_scale_kernel         test_l2_clip_rows (16388: second trip; 66565; zero row)
  adam_multi_kernel            test_adam_multi (20 tensors: two launches; 4095 / 4096 / 4097 / 8195; g or m 4 bytes off: scalar branch)
  adam_kernel                  test_adam_device_counter (steps 1 .. 4 and 1000, by value and from a device int32)
  act_bwd_kernel               test_act_bwd (g and y 4 bytes off: scalar branch; y == +-0.0)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = -7.25


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


def _close(got, exp, rtol=1e-4, what=""):
    """tests/test_kernels_gpu.py's bound: max abs error relative to the scale of the expected tensor (NaN fails)."""
    got = got.detach().cpu().double()
    exp = exp.detach().cpu().double()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    scale = exp.abs().max().item() + 1e-12
    err = (got - exp).abs().max().item() if got.numel() else 0.0
    assert err <= rtol * scale, "%s: max abs err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale)


def _allclose(got, exp, rtol, atol, what=""):
    """Elementwise |got - exp| <= atol + rtol |exp| against a float64 expectation (NaN fails)."""
    got = got.detach().cpu().double()
    exp = exp.detach().cpu().double()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    err = (got - exp).abs()
    ok = err <= atol + rtol * exp.abs()
    assert bool(ok.all()), "%s: %d of %d off, max abs err %.3e, max rel err %.3e" % (
        what, int((~ok).sum()), ok.numel(), err[~ok].max().item(), (err / (exp.abs() + 1e-300))[~ok].max().item())


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


# ---- 1. segment means (DCResNet_models.py:149-153) ------------------------------------------------------------------------------
SEG_CASES = [([1, 300, 257], [-1.0, 1.0, -1.0]), ([513], [1.0]),
             ([255, 256, 257, 1, 300, 2, 511, 64], [-1.0, 1.0, 1.0, -1.0, -1.0, 1.0, -1.0, 1.0])]


def _seg_inputs(sizes, signs):
    g = _gen("segment_means", sizes, signs)
    x = torch.randn(sum(sizes), generator=g) + 0.5
    scale = [_f32(s / n) for s, n in zip(signs, sizes)]          # +-1/n: the +-mean of a row block
    return g, x, scale


@pytest.mark.parametrize("sizes,signs", SEG_CASES)
def test_segment_means_forward(sizes, signs):
    """vec[s] = +-mean of row block s, total = their sum; blocks longer than the 256 threads and the 4-float scratch reused per block."""
    ops = _ops()
    _, x, scale = _seg_inputs(sizes, signs)
    vec, total = ops.segment_means(x.cuda(), sizes, scale)
    ref = torch.stack([c * p.double().sum() for c, p in zip(scale, torch.split(x, sizes))])
    _allclose(vec, ref, 1e-5, 1e-7, "vec")
    _allclose(total, ref.sum(), 1e-5, 1e-7, "total")


@pytest.mark.parametrize("form", ["total", "vec", "both"])
@pytest.mark.parametrize("sizes,signs", SEG_CASES)
def test_segment_means_backward(sizes, signs, form):
    """gx[i] = (g_total + g_vec[s]) * scale[s] on the rows of block s; more than 256 rows in all, so more than one workgroup."""
    ops = _ops()
    g, _, scale = _seg_inputs(sizes, signs)
    n = sum(sizes)
    assert n > 256
    gt = torch.randn((), generator=g) + 2.0
    gv = torch.randn(len(sizes), generator=g)
    gx = ops.segment_means_bwd(gt.cuda() if form != "vec" else None, gv.cuda() if form != "total" else None, sizes, scale, (n, 1),
                               torch.device("cuda"))
    per_block = (gt.double() if form != "vec" else 0.0) + (gv.double() if form != "total" else torch.zeros(len(sizes), dtype=torch.float64))
    ref = torch.cat([(per_block[s] * scale[s]).expand(sz) for s, sz in enumerate(sizes)]).reshape(n, 1)
    assert gx.shape == (n, 1)
    _allclose(gx, ref, 1e-6, 1e-9, "gx")


def test_segment_means_refuses_bad_roles(monkeypatch):
    """More than 8 row blocks, or sizes and scales of different lengths, raise in Python: the library is never reached."""
    ops = _ops()
    x = torch.zeros(9, device="cuda")
    reached = []
    monkeypatch.setattr(ops._lib, "lib", lambda: reached.append(1) or pytest.fail("the library was reached"))
    with pytest.raises(RuntimeError, match="1..8 row blocks"):
        ops.segment_means(x, [1] * 9, [1.0] * 9)
    with pytest.raises(RuntimeError, match="1..8 row blocks"):
        ops.segment_means(x, [4, 5], [1.0])
    with pytest.raises(RuntimeError, match="1..8 row blocks"):
        ops.segment_means_bwd(x[:1], None, [1] * 9, [1.0] * 9, (9,), x.device)
    with pytest.raises(RuntimeError, match="1..8 row blocks"):
        ops.segment_means_bwd(x[:1], None, [4, 5], [1.0, 1.0, 1.0], (9,), x.device)
    assert not reached


# ---- 2. train_D's logger sums (train.py:488-496) --------------------------------------------------------------------------------
def test_dstep_stats():
    """acc7 += [adv, adv, real loss, fake loss, 100 * mean(d_real > 0), 100 * mean(d_fake < 0), penalty]: more logits than threads,
    logits of exactly +0.0 and -0.0 (neither > 0 nor < 0) in the first and the second trip, penalty absent and present."""
    ops = _ops()
    g = _gen("dstep_stats")
    d_real, d_fake = torch.randn(300, 1, generator=g), torch.randn(257, 1, generator=g)
    for d in (d_real, d_fake):
        d[3], d[17], d[-1], d[-2] = 0.0, -0.0, 0.0, -0.0
    rl, fl, pen = torch.tensor(-0.3), torch.tensor(0.7), torch.tensor(9.5)
    start = torch.linspace(0.5, 2.0, 7)
    acc = start.clone().cuda()
    ops.dstep_stats(d_real.cuda(), d_fake.cuda(), rl.cuda(), fl.cuda(), None, acc)
    r_acc = 100.0 * float((d_real.double() > 0).sum()) / 300
    f_acc = 100.0 * float((d_fake.double() < 0).sum()) / 257
    rl64, fl64 = rl.double().item(), fl.double().item()
    once = torch.tensor([rl64 + fl64, rl64 + fl64, rl64, fl64, r_acc, f_acc, 0.0], dtype=torch.float64)
    _allclose(acc, start.double() + once, 1e-5, 0.0, "first call")
    assert torch.equal(acc[6:].cpu(), start[6:])                  # no penalty: its sum is left alone
    ops.dstep_stats(d_real.cuda(), d_fake.cuda(), rl.cuda(), fl.cuda(), pen.cuda(), acc)
    twice = 2 * once
    twice[6] = pen.double()
    _allclose(acc, start.double() + twice, 1e-5, 0.0, "second call")


# ---- 3. update_grad_logging (train.py:310-329) -----------------------------------------------------------------------------------
def _glog_factors(sq, col0, C, per_layer, eps):
    q = sq[:, col0:].double()
    n = q.sqrt() if per_layer else q.sum(0, keepdim=True).sqrt()
    c = C.double() if per_layer else C[:1].double()
    return n, c, (c.view(-1, 1) / (n + eps)).clamp(max=1.0)


def _glog_inputs(per_layer, L, B, col0):
    g = _gen("grad_log_stats", per_layer, L, B, col0)
    eps = _f32(1e-6)
    sq = (torch.rand(L, col0 + B, generator=g) * 4 + 0.05).pow(2)
    C = torch.rand(L, generator=g) * 2 + 0.5
    if L > 1:
        sq[1, col0:] = (1.0 + 1e-4 * torch.rand(B, generator=g)).pow(2)        # nearly equal norms: the std must not cancel away
        C[1] = 0.7
    # keep every clip factor away from the 0.999 of the "clipped" count: push the few norms that land near it 5% further out
    _, _, f = _glog_factors(sq, col0, C, per_layer, eps)
    near = (f - 0.999).abs() < 2e-3
    cols = sq[:, col0:]
    if per_layer:
        cols[near] *= 1.1
    else:
        cols[:, near[0]] *= 1.1
    sq[:, :col0] = 1e6                                                          # columns before col0 are not the step's
    return sq, C, eps


@pytest.mark.parametrize("col0", [0, 37])
@pytest.mark.parametrize("B", [1, 257, 300])
@pytest.mark.parametrize("L", [1, 9])
@pytest.mark.parametrize("per_layer", [True, False])
def test_grad_log_stats(per_layer, L, B, col0):
    """Per logged row: mean / population std / max of the B norms, the clip norm and the fraction of clip factors below 0.999, ADDED
    to the sums; B beyond the 256 threads (a thread holds two norms), B == 1, columns [col0, col0 + B) ending at the row's end."""
    ops = _ops()
    sq, C, eps = _glog_inputs(per_layer, L, B, col0)
    n, c, f = _glog_factors(sq, col0, C, per_layer, eps)
    assert bool(((f - 0.999).abs() > 1e-5).all()), "input error: a clip factor within 1e-5 of 0.999"
    rows = L if per_layer else 1
    acc = torch.zeros(5, rows).cuda()
    for _ in range(2):
        ops.grad_log_stats(sq.cuda(), col0, B, (C if per_layer else C[:1]).cuda().contiguous(), per_layer, eps, acc)
    want = 2 * torch.stack([n.mean(1), n.std(1, unbiased=False), n.max(1).values, c, (f < 0.999).double().mean(1)])
    got = acc.cpu()
    _allclose(got[[0, 2, 3, 4]], want[[0, 2, 3, 4]], 1e-5, 1e-7, "mean / max / C / clipped")
    loose = torch.zeros(rows, dtype=torch.bool)
    if per_layer and L > 1:
        loose[1] = True                                                         # the nearly-equal layer: test_kernels_gpu.py's 2e-3
        _allclose(got[1][loose], want[1][loose], 2e-3, 1e-7, "std of the nearly equal norms")
    _allclose(got[1][~loose], want[1][~loose], 1e-5, 1e-7, "std")


# ---- 4. adaptive clip in one launch (train.py:233-243 + :324) -------------------------------------------------------------------
def _adaptive_ref(adapt, rows, stat, scalar, per_layer, eps, first):
    norms = torch.stack(adapt).double().sqrt()
    r = norms.mean(1) if stat == "mean" else norms.max(1).values
    c = r * scalar if per_layer else ((r * r).sum().sqrt() * scalar).reshape(1)
    q = torch.stack(rows).double()
    f = (c.view(-1, 1) / (q.sqrt() + eps)) if per_layer else (c / (q.sum(0).sqrt() + eps))
    f = f.clamp(max=1.0)
    f[..., :first] = 1.0
    return r, c, f


@pytest.mark.parametrize("L", [1, 9])
@pytest.mark.parametrize("n_adapt,n_rows", [(1, 5), (257, 300), (300, 255)])
@pytest.mark.parametrize("per_layer", [True, False])
@pytest.mark.parametrize("stat", ["mean", "max"])
def test_adaptive_clip(stat, per_layer, n_adapt, n_rows, L):
    """cslgan_adaptive_clip_f32 against host float64: the statistic over n_adapt norms (one norm, 257, 300: the 256-wide tree with
    idle threads and with a second trip), the clip norm(s), the copied squared norms, the factors (exactly 1 before the first private
    row: none, all, some private), gathered layers with a repeat, a job over more rows than threads that ends at the last row."""
    ops = _ops()
    g = _gen("adaptive_clip", stat, per_layer, n_adapt, n_rows, L)
    scalar, eps = _f32(1.7), _f32(1e-6)
    adapt = [torch.rand(n_adapt, generator=g) * (3.0 + l) + 0.01 for l in range(L)]
    rows = [torch.rand(n_rows, generator=g) * (6.0 + l) for l in range(L)]
    mat = [0, L - 1, 0] if per_layer else []
    for first in (0, n_rows, n_rows // 2 + 1):
        cnt = n_rows - max(1, n_rows // 30)
        bufs = [torch.full((cnt + 2,), GUARD, device="cuda"), torch.full((3,), GUARD, device="cuda")]
        jobs = [(bufs[0][1:1 + cnt], L - 1, n_rows - cnt, _f32(1.0 / 128)), (bufs[1][1:2], 0, 0, 0.5)]
        r, c, sq, f, f_mat = ops.adaptive_clip([a.cuda() for a in adapt], [q.cuda() for q in rows], stat == "max", scalar, per_layer, eps,
                                               first, mat_layers=mat, jobs=jobs)
        r_ref, c_ref, f_ref = _adaptive_ref(adapt, rows, stat, scalar, per_layer, eps, first)
        _allclose(r, r_ref, 2e-6, 0.0, "r")
        _allclose(c, c_ref, 2e-6, 0.0, "C")
        assert torch.equal(sq.cpu(), torch.stack(rows))
        _allclose(f, f_ref, 3e-6, 0.0, "f")
        assert torch.equal(f[..., :first].cpu(), torch.ones_like(f[..., :first].cpu()))
        if per_layer:
            _allclose(f_mat, f_ref[mat], 3e-6, 0.0, "f_mat")
            assert torch.equal(f_mat[0], f_mat[2])
        else:
            assert f_mat is None
        for (dst, layer, first_row, scale), buf in zip(jobs, bufs):
            src = f_ref[layer] if per_layer else f_ref
            _allclose(dst, src[first_row:first_row + dst.numel()] * scale, 3e-6, 0.0, "job")
            assert buf[0].item() == GUARD and buf[-1].item() == GUARD


def test_adaptive_clip_job_without_rows():
    """A row-weight job of count 0 writes nothing (the job's pointer is valid: ops.adaptive_clip takes a count from its tensor, and an
    empty tensor has no address, so this one call fills the C struct itself); the launch's other outputs are as without it."""
    ops = _ops()
    from csl_gan_amd import _lib
    g = _gen("adaptive_clip_empty_job")
    n_adapt, n_rows, scalar, eps = 5, 7, _f32(1.7), _f32(1e-6)
    adapt, rows = (torch.rand(n_adapt, generator=g) + 0.1), torch.rand(n_rows, generator=g) * 6
    da, dr = adapt.cuda(), rows.cuda()
    dst = torch.full((4,), GUARD, device="cuda")
    a = _lib.AdaptiveClipT()
    a.n_layers, a.n_mat, a.n_jobs = 1, 0, 2
    a.sq_adapt[0], a.sq_rows[0] = da.data_ptr(), dr.data_ptr()
    a.job_dst[0], a.job_layer[0], a.job_first[0], a.job_count[0], a.job_scale[0] = dst.data_ptr(), 0, n_rows, 0, 2.0
    a.job_dst[1], a.job_layer[1], a.job_first[1], a.job_count[1], a.job_scale[1] = dst.data_ptr() + 8, 0, n_rows - 1, 1, 2.0
    out = [torch.empty(k, device="cuda") for k in (1, 1, n_rows, n_rows)]
    ops.check(_lib.lib().cslgan_adaptive_clip_f32(ctypes.byref(a), n_adapt, n_rows, 0, scalar, 1, eps, 0, *[ops._p(o) for o in out], None,
                                                  ops._stream()), "adaptive_clip")
    r_ref, c_ref, f_ref = _adaptive_ref([adapt], [rows], "mean", scalar, True, eps, 0)
    _allclose(out[0], r_ref, 2e-6, 0.0, "r")
    _allclose(out[3], f_ref[0], 3e-6, 0.0, "f")
    got = dst.cpu()
    assert got[0].item() == GUARD and got[1].item() == GUARD and got[3].item() == GUARD
    _allclose(got[2], 2.0 * f_ref[0, n_rows - 1], 3e-6, 0.0, "job")


# ---- 5. interpolates (gradient_penalty.py:36) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("length", [105, 768, 66564, 66565])
def test_lerp_rows(length, B):
    """alpha * real + (1 - alpha) * fake per row: the scalar branch (105), the float4 branch in one trip (768) and two (66564 under the
    cap of 64 workgroups), scalar trips under the cap (66565); alpha of exactly 0 / 1 returns fake / real bit for bit."""
    ops = _ops()
    g = _gen("lerp_rows", length, B)
    real, fake = torch.randn(B, length, generator=g), torch.randn(B, length, generator=g)
    alphas = [torch.tensor([0.0, 1.0, 0.37])] if B == 3 else [torch.tensor([a]) for a in (0.0, 1.0, 0.37)]
    for alpha in alphas:
        out = ops.lerp_rows(real.cuda(), fake.cuda(), alpha.cuda())
        a, one_minus_a = alpha.double().view(B, 1), (1 - alpha).double().view(B, 1)      # (1 - alpha) as the fp32 value the kernel forms
        _allclose(out, a * real.double() + one_minus_a * fake.double(), 1e-6, 1e-7, "lerp")
        for b in range(B):
            if alpha[b] == 0.0:
                assert torch.equal(out[b].cpu(), fake[b])
            if alpha[b] == 1.0:
                assert torch.equal(out[b].cpu(), real[b])


def test_lerp_rows_channels_last():
    """A channels-last batch whose C*H*W = 105 is no multiple of 4: rows are the images in memory order, the result keeps the strides."""
    ops = _ops()
    g = _gen("lerp_rows_channels_last")
    real, fake = torch.randn(3, 3, 5, 7, generator=g), torch.randn(3, 3, 5, 7, generator=g)
    alpha = torch.tensor([0.0, 1.0, 0.37])
    dr, df = real.cuda().contiguous(memory_format=torch.channels_last), fake.cuda().contiguous(memory_format=torch.channels_last)
    out = ops.lerp_rows(dr, df, alpha.cuda())
    assert out.stride() == dr.stride()
    a, one_minus_a = alpha.double().view(3, 1, 1, 1), (1 - alpha).double().view(3, 1, 1, 1)
    _allclose(out, a * real.double() + one_minus_a * fake.double(), 1e-6, 1e-7, "lerp")
    assert torch.equal(out[0].cpu(), fake[0]) and torch.equal(out[1].cpu(), real[1])


# ---- 6. the Lipschitz term (gradient_penalty.py:52-54 with the mean and the weight) ---------------------------------------------
def _rows_with_norms(g, rows, length, lo=(0.3, 0.95), hi=(1.05, 1.8)):
    """fp32 rows whose norms are spread over lo (first half) and hi (second half): both sides of 1 and at least 0.05 away from it, so
    (norm - 1) keeps its leading digits in fp32."""
    t = torch.randn(rows, length, generator=g).double()
    k = rows // 2
    target = torch.cat([torch.linspace(lo[0], lo[1], k, dtype=torch.float64), torch.linspace(hi[0], hi[1], rows - k, dtype=torch.float64)])
    return (t * (target / t.norm(2, dim=1)).view(-1, 1)).float()


def _lip_ref(t, one_sided, coef, per_sample, w):
    """float64 autograd of coef * sum or rows of ((t.norm(2, 1) - 1)[.clamp(min=0)] ** 2), weighted as the tests weight the device's."""
    tr = t.double().requires_grad_(True)
    d = tr.norm(2, dim=1) - 1
    per = coef * ((d.clamp(min=0) if one_sided else d) ** 2)
    out = per if per_sample else per.sum()
    loss = (out * w.double()).sum() if per_sample else out * 1.7
    (gr,) = torch.autograd.grad(loss, tr)
    return tr.detach().norm(2, dim=1), per.detach(), out.detach(), gr


def _lip_device(td, one_sided, coef, per_sample, w, create_graph=False):
    from csl_gan_amd import functional as HF
    td = td.requires_grad_(True)
    out = HF.LipschitzTerm.apply(td, one_sided, coef, per_sample)
    loss = (out * w.cuda()).sum() if per_sample else out * 1.7
    (gr,) = torch.autograd.grad(loss, td, create_graph=create_graph)
    return out.detach(), gr.detach()


LIP_CASES = [(1, 105, 0), (300, 12, 0), (300, 12, 1), (5, 768, 0), (5, 768, 1), (3, 66564, 0), (3, 66564, 1)]


@pytest.mark.parametrize("rows,length,off", LIP_CASES)
@pytest.mark.parametrize("one_sided,per_sample", [(False, False), (True, False), (False, True), (True, True)])
def test_lipschitz_term(one_sided, per_sample, rows, length, off):
    """functional.LipschitzTerm forward and backward: one row (the first ticket is the last), 300 rows (the last workgroup sums more
    rows than it has threads), a scalar length, the backward's grid cap, and (off = 1) float4-length rows that start 4 bytes past
    a 16-byte boundary, which both kernels must read with scalar loads."""
    g = _gen("lipschitz_term", one_sided, per_sample, rows, length, off)
    if rows == 1:
        ts = [_rows_with_norms(g, 2, length)[i:i + 1].clone() for i in range(2)]       # a one-row batch on either side of 1
    else:
        ts = [_rows_with_norms(g, rows, length)]
    norms = torch.cat([t.double().norm(2, dim=1) for t in ts])
    assert bool((norms < 1).any()) and bool((norms > 1).any())
    coef = _f32(10.0 if per_sample else 10.0 / rows)
    w = torch.linspace(0.5, 1.5, rows)
    for t in ts:
        td, buf = _carve(t, 4 if off == 0 else 1)
        got, grad = _lip_device(td, one_sided, coef, per_sample, w)
        _, _, ref, gref = _lip_ref(t, one_sided, coef, per_sample, w)
        _allclose(got, ref, 1e-4, 1e-6, "term")
        _allclose(grad, gref, 1e-4, 1e-7, "gradient")
        assert _guards_intact(buf, 4 if off == 0 else 1, t.numel())


def test_lipschitz_ticket_sequence():
    """300 rows, 5, 300 again with other values: the per-device ticket word must be back at 0 after every launch, whatever the grid
    before it — each call's norms, rows and total are checked against the host, not against the previous call."""
    ops = _ops()
    coef = _f32(0.25)
    for i, rows in enumerate((300, 5, 300)):
        t = _rows_with_norms(_gen("lipschitz_ticket", i), rows, 12)
        norm, per, total = ops.lipschitz_term(t.cuda(), False, coef)
        n_ref, per_ref, tot_ref, _ = _lip_ref(t, False, coef, False, None)
        _allclose(norm, n_ref, 1e-4, 1e-6, "norm, call %d" % i)
        _allclose(per, per_ref, 1e-4, 1e-6, "per, call %d" % i)
        _allclose(total, tot_ref, 1e-4, 1e-6, "total, call %d" % i)


@pytest.mark.parametrize("one_sided,per_sample", [(False, False), (True, False), (False, True), (True, True)])
def test_lipschitz_zero_rows(one_sided, per_sample):
    """Rows of exactly zero (one of them the last): norm 0, term coef (two-sided) or 0 (one-sided), and a gradient of exactly 0 on
    those rows — what torch.autograd gives for t.norm(2, 1) at the origin — with every other entry finite and right.  The kernel and
    the differentiable torch form (create_graph=True) both; scalar-length and float4-length rows."""
    ops = _ops()
    rows, zero = 6, [2, 5]
    coef = _f32(10.0 if per_sample else 10.0 / rows)
    w = torch.linspace(0.5, 1.5, rows)
    for length in (105, 768):
        t = _rows_with_norms(_gen("lipschitz_zero_rows", one_sided, per_sample, length), rows, length)
        t[zero] = 0.0
        norm, per, _ = ops.lipschitz_term(t.cuda(), one_sided, coef)
        assert torch.equal(norm[zero].cpu(), torch.zeros(2))
        assert torch.equal(per[zero].cpu(), torch.full((2,), 0.0 if one_sided else coef))
        _, _, ref, gref = _lip_ref(t, one_sided, coef, per_sample, w)
        assert torch.equal(gref[zero], torch.zeros(2, length, dtype=torch.float64))      # the reference itself: torch's norm backward
        for create_graph in (False, True):
            got, grad = _lip_device(t.cuda(), one_sided, coef, per_sample, w, create_graph=create_graph)
            what = "differentiable form" if create_graph else "kernel"
            _allclose(got, ref, 1e-4, 1e-6, what + ": term")
            assert bool(torch.isfinite(grad).all()), "%s: %d non-finite gradient entries" % (what, int((~torch.isfinite(grad)).sum()))
            assert torch.equal(grad[zero].cpu(), torch.zeros(2, length)), what
            _allclose(grad, gref, 1e-4, 1e-7, what + ": gradient")


# ---- 7. row norms and the l2 clip (gradient_penalty.py:52-53, backprop_clip.py:18-22) -------------------------------------------
ROW_CASES = [(1, 1), (300, 7), (3, 66565), (5, 8192 * 2 + 4)]


def _row_inputs(what, rows, length, zero_row):
    g = _gen(what, rows, length, zero_row)
    t = torch.randn(rows, length, generator=g) * torch.linspace(0.2, 3.0, rows).view(-1, 1)
    if zero_row:
        t[rows // 2] = 0.0
    return g, t


@pytest.mark.parametrize("zero_row", [False, True])
@pytest.mark.parametrize("rows,length", ROW_CASES)
def test_row_l2norm(rows, length, zero_row):
    """functional.RowL2Norm: norms and d(sum w_b norm_b)/dt = w_b t_b / norm_b through the kernel and through the differentiable torch
    form; a zero row has norm 0 and gradient 0, as torch's t.norm(2, 1) has.  300 rows: a second workgroup of the root kernel;
    66565 and 16388: grid-stride trips of the backward and a second chunk of the sum of squares."""
    from csl_gan_amd import functional as HF
    g, t = _row_inputs("row_l2norm", rows, length, zero_row)
    w = torch.randn(rows, generator=g)
    tr = t.double().requires_grad_(True)
    n_ref = tr.norm(2, dim=1)
    (g_ref,) = torch.autograd.grad((n_ref * w.double()).sum(), tr)
    for create_graph in (False, True):
        td = t.cuda().requires_grad_(True)
        n = HF.RowL2Norm.apply(td)
        (grad,) = torch.autograd.grad((n * w.cuda()).sum(), td, create_graph=create_graph)
        what = "differentiable form" if create_graph else "kernel"
        _close(n, n_ref, 1e-4, what + ": norm")
        _close(grad, g_ref, 1e-4, what + ": gradient")
        if zero_row:
            z = rows // 2
            assert n[z].item() == 0.0
            assert torch.equal(grad[z].detach().cpu(), torch.zeros(length)), what


@pytest.mark.parametrize("zero_row", [False, True])
@pytest.mark.parametrize("rows,length", ROW_CASES)
def test_l2_clip_rows(rows, length, zero_row):
    """l2_clip: rows inside the ball of radius C (and a zero row) come back unchanged bit for bit, rows outside are scaled onto it;
    the float64 norm of a clipped row is at most C (1 + 1e-5) — the 2e-5 that test_sample_sqnorm allows a squared norm, halved for
    the root.  The first half of the rows lies well inside (0.2 C .. 0.8 C), the rest well outside (1.3 C .. 3 C); a lone row is
    outside, or the zero row."""
    ops = _ops()
    g = _gen("l2_clip_rows", rows, length, zero_row)
    Cn = _f32(1.3)
    k = (rows + 1) // 2 if rows > 1 else 0
    t = torch.randn(rows, length, generator=g).double()
    target = torch.cat([torch.linspace(0.2, 0.8, k, dtype=torch.float64), torch.linspace(1.3, 3.0, rows - k, dtype=torch.float64)]) * Cn
    t = (t * (target / t.norm(2, dim=1)).view(-1, 1)).float()
    if zero_row:
        t[0] = 0.0
    n = t.double().norm(2, dim=1)
    assert bool(((n - Cn).abs() > 1e-5 * Cn).all()), "input error: a row norm within 1e-5 of C"
    inside = n <= Cn
    if rows > 1:
        assert bool((inside & (n > 0)).any()) and bool((~inside).any())
    out = ops.l2_clip_rows(t.cuda(), Cn).cpu()
    assert torch.equal(out[inside], t[inside])
    ref = torch.where(inside.view(-1, 1), t.double(), Cn * t.double() / n.view(-1, 1))
    _close(out, ref, 1e-4, "l2_clip")
    assert bool((out[~inside].double().norm(2, dim=1) <= Cn * (1 + 1e-5)).all())


# ---- 8. per-sample squared norms and clip factors (train.py:311-314, :324) ------------------------------------------------------
SQ_SEGS = [(64, 4), (64, 1), (7, 4), (7, 1), (8196, 1), (8196, 4), (33, 4), (12, 1), (1, 4), (4, 1), (4800, 1), (4800, 4), (16, 1), (20, 4),
           (100, 1), (36, 4), (8, 1), (5, 4)]


def test_sample_sqnorm_unaligned_segments():
    """18 fp32 segments in one call (two launches of at most 16): float4-length rows that start 4 bytes past a 16-byte boundary must
    take the scalar loads, next to aligned ones that take float4 loads, one of each crossing an 8192-float chunk.  Then the
    sensitivity property through clip_factors: factor x float64 norm of every private row is at most C (1 + 1e-5)."""
    ops = _ops()
    rows = 3
    g = _gen("sample_sqnorm_unaligned")
    mats = [torch.randn(rows, ln, generator=g) * (1 + 0.25 * i) for i, (ln, _) in enumerate(SQ_SEGS)]
    assert len(mats) > 16
    dm = [_carve(m, off)[0] for m, (_, off) in zip(mats, SQ_SEGS)]
    sq = ops.sample_sqnorm(dm)
    ref = torch.stack([m.double().pow(2).sum(1) for m in mats])
    assert sq.shape == ref.shape
    for i in range(len(mats)):
        _close(sq[i], ref[i], 2e-5, "sqnorm of segment %d %s" % (i, SQ_SEGS[i]))
    norms = ref.sqrt()
    for flat in (True, False):
        Cn = torch.tensor([_f32(20.0)]) if flat else (norms.median(dim=1).values.float())
        f = ops.clip_factors(sq, Cn.cuda(), flat, eps=_f32(1e-6), first_private_row=1).cpu().double()
        nn_ = ref.sum(0).sqrt() if flat else norms
        bound = Cn.double() * (1 + 1e-5) if flat else Cn.double().view(-1, 1) * (1 + 1e-5)
        assert torch.equal(f[..., :1], torch.ones_like(f[..., :1]))
        assert bool(((f * nn_)[..., 1:] <= bound).all())
        assert bool((f[..., 1:] < 1).any())


@pytest.mark.parametrize("flat", [True, False])
@pytest.mark.parametrize("n_rows", [1, 129, 300])
def test_clip_factors(n_rows, flat):
    """min(1, C / (norm + 1e-6)) flat and per segment, exactly 1 before the first private row (0: all private; 128: the boundary of
    the 128-thread workgroups; n_rows: none private); a row of norm 0 has factor 1; factor x norm never exceeds C (1 + 1e-5)."""
    ops = _ops()
    n_seg, eps = 4, _f32(1e-6)
    for zero_row in ([False, True] if n_rows == 1 else [True]):
        g = _gen("clip_factors", n_rows, flat, zero_row)
        sq = (torch.rand(n_seg, n_rows, generator=g) * 6 + 0.01).pow(2)
        if zero_row:
            sq[:, n_rows - 1] = 0.0
        Cn = torch.tensor([4.0]) if flat else torch.tensor([2.0, 5.0, 0.5, 7.0])
        q = sq.double()
        nrm_ref = q.sum(0).sqrt() if flat else q.sqrt()
        f_all = ((Cn.double() if flat else Cn.double().view(-1, 1)) / (nrm_ref + eps)).clamp(max=1.0)
        for first in (0, 128, n_rows):
            f_ref = f_all.clone()
            f_ref[..., :first] = 1.0
            f, nrm = ops.clip_factors(sq.cuda(), Cn.cuda(), flat, eps=eps, first_private_row=first, want_norms=True)
            _close(f, f_ref, 1e-4, "factors")
            _close(nrm, nrm_ref, 1e-4, "norms")
            f = f.cpu()
            assert torch.equal(f[..., :first], torch.ones_like(f[..., :first]))
            if zero_row:
                assert bool((f[..., n_rows - 1] == 1.0).all())
            bound = (Cn.double() if flat else Cn.double().view(-1, 1)) * (1 + 1e-5)
            assert bool(((f.double() * nrm_ref)[..., first:] <= bound).all())


# ---- 9. Adam (torch.optim.Adam semantics, train.py:76,484) ------------------------------------------------------------------------
def _adam_ref(p, grads, lr, b1, b2, eps, wd, steps):
    """float64 Adam as torch.optim.Adam defines it: L2 weight decay added to the gradient, bias corrections 1 - b^t,
    denom = sqrt(v) / sqrt(bc2) + eps, p -= lr / bc1 * m / denom.  m and v start at 0."""
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for gr, t in zip(grads, steps):
        gr = gr.double()
        if wd != 0:
            gr = gr + wd * p
        m = b1 * m + (1 - b1) * gr
        v = b2 * v + (1 - b2) * gr * gr
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        denom = v.sqrt() / math.sqrt(bc2) + eps
        p = p - lr / bc1 * m / denom
    return p, m, v


ADAM_LENS = [1, 3, 4095, 4096, 4097, 8195, 7, 64, 1280, 4800, 2, 5, 12, 4100, 33, 8192, 100, 257, 16, 8196]
ADAM_UNALIGNED = {1: "g", 2: "g", 3: "m", 5: "g", 6: "p", 9: "m", 12: "v", 13: "m", 19: "g"}     # tensor index -> the buffer 4 bytes off
ADAM_HYPER = [((0.0, 0.9), 0.0), ((0.0, 0.9), 0.01), ((0.5, 0.999), 0.0), ((0.5, 0.999), 0.01)]


def _adam_state(g, lens, unaligned):
    """Per tensor: p, g, m, v carved out of guarded allocations, all 16-byte aligned unless the tensor names one buffer to sit 4 bytes
    off (then the whole tensor must take the scalar branch)."""
    state = []
    for i, n in enumerate(lens):
        p0 = torch.randn(n, generator=g)
        offs = {k: (1 if unaligned.get(i) == k else 4) for k in "pgmv"}
        views, bufs = {}, {}
        for k, init in (("p", p0), ("g", torch.zeros(n)), ("m", torch.zeros(n)), ("v", torch.zeros(n))):
            views[k], bufs[k] = _carve(init, offs[k])
        state.append(dict(n=n, p0=p0, offs=offs, views=views, bufs=bufs, grads=[]))
    return state


def _adam_check(state, lr, b1, b2, eps, wd, steps, what):
    for i, s in enumerate(state):
        p_ref, m_ref, v_ref = _adam_ref(s["p0"], s["grads"], lr, b1, b2, eps, wd, steps)
        tag = "%s, tensor %d (%d floats, off %s)" % (what, i, s["n"], s["offs"])
        _close(s["views"]["p"], p_ref, 1e-5, tag + ": p")
        _close(s["views"]["m"], m_ref, 1e-5, tag + ": m")
        _close(s["views"]["v"], v_ref, 1e-5, tag + ": v")
        for k in "pgmv":
            assert _guards_intact(s["bufs"][k], s["offs"][k], s["n"]), tag + ": guard around " + k


@pytest.mark.parametrize("betas,wd", ADAM_HYPER)
def test_adam_multi(betas, wd):
    """ops.adam_multi over 20 tensors (two launches), four steps, p / m / v against float64 Adam: lengths around the 4096-float chunk,
    a float4 tail, one-element tensors, tensors with every buffer aligned and tensors where p, g, m or v alone starts 4 bytes past a
    16-byte boundary; nothing outside a tensor's floats is written."""
    ops = _ops()
    assert len(ADAM_LENS) == 20 and {1, 3, 4095, 4096, 4097, 8195} <= set(ADAM_LENS)
    g = _gen("adam_multi", betas, wd)
    lr, b1, b2, eps, wd = _f32(0.05), _f32(betas[0]), _f32(betas[1]), _f32(1e-8), _f32(wd)
    state = _adam_state(g, ADAM_LENS, ADAM_UNALIGNED)
    steps = [1, 2, 3, 4]
    for step in steps:
        for s in state:
            gr = torch.randn(s["n"], generator=g)
            s["grads"].append(gr)
            s["views"]["g"].copy_(gr)
        ops.adam_multi(*[[s["views"][k] for s in state] for k in "pgmv"], lr, b1, b2, eps, wd, step)
    _adam_check(state, lr, b1, b2, eps, wd, steps, "adam_multi")


@pytest.mark.parametrize("betas,wd", ADAM_HYPER)
def test_adam_device_counter(betas, wd):
    """The step read from a device int32 (graph-captured steps) against the step passed by value and against float64 Adam, at steps
    1 .. 4 and 1000, for adam_step and adam_multi: the kernels' powf(b, t) stands in for the host's double pow, inside the same
    1e-5 of the output scale that the by-value form is held to."""
    ops = _ops()
    g = _gen("adam_device_counter", betas, wd)
    lr, b1, b2, eps, wd = _f32(0.05), _f32(betas[0]), _f32(betas[1]), _f32(1e-8), _f32(wd)
    lens, unaligned = [5000, 4097, 3, 8195], {1: "g", 3: "m"}
    steps = [1, 2, 3, 4, 1000]
    forms = {}
    for form in ("multi by value", "multi from device", "single by value", "single from device"):
        forms[form] = _adam_state(_gen("adam_device_counter state", betas, wd), lens, unaligned)
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    for step in steps:
        grads = [torch.randn(n, generator=g) for n in lens]
        counter.fill_(step)
        for form, state in forms.items():
            for s, gr in zip(state, grads):
                s["grads"].append(gr)
                s["views"]["g"].copy_(gr)
            st = counter if form.endswith("device") else step
            if form.startswith("multi"):
                ops.adam_multi(*[[s["views"][k] for s in state] for k in "pgmv"], lr, b1, b2, eps, wd, st)
            else:
                for s in state:
                    ops.adam_step(*[s["views"][k] for k in "pgmv"], lr, b1, b2, eps, wd, st)
    for form, state in forms.items():
        _adam_check(state, lr, b1, b2, eps, wd, steps, form)
    for kind in ("multi", "single"):
        for a, b in zip(forms[kind + " by value"], forms[kind + " from device"]):
            for k in "pmv":
                _close(b["views"][k], a["views"][k], 1e-5, "%s: device counter vs by value, %s of %d floats" % (kind, k, a["n"]))


# ---- 10. leaky-ReLU backward (DCResNet_models.py:132) ------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 4])
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_act_bwd(n, off):
    """out = y > 0 ? g : slope * g.  off = 1: g and y start 4 bytes past a 16-byte boundary, so the kernel must take its scalar branch
    (ops.act_bwd allocates out itself, aligned); off = 4: float4 loads and the scalar tail.  An output of +0.0 or -0.0 takes the
    slope, as F.leaky_relu's backward does."""
    ops = _ops()
    slope = _f32(0.2)
    for y0 in (None, 0.0, -0.0):
        g = _gen("act_bwd", n, off, y0)
        gg, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
        planted = []
        if y0 is not None:
            planted = sorted({0, n // 2, n - 1})
            for j, i in enumerate(planted):
                y[i] = y0 if j % 2 == 0 else -y0
                gg[i] = 1.5
        (dg, bg), (dy, by) = _carve(gg, off), _carve(y, off)
        out = ops.act_bwd(dg, dy, slope).cpu()
        pos = y > 0
        assert not bool(pos[planted].any())
        ref = torch.where(pos, gg.double(), slope * gg.double())
        _close(out, ref, 1e-4, "act_bwd")
        assert torch.equal(out[pos], gg[pos])
        _allclose(out[planted], ref[planted], 1e-6, 0.0, "entries with y == +-0")
        assert _guards_intact(bg, off, n) and _guards_intact(by, off, n)
