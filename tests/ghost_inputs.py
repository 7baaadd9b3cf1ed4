"""Operands for the ghost-norm tests (imported as tests.ghost_inputs): spatially smooth, channel-shared, post-ReLU activations and
output gradients whose scale spans six decades over the batch, plus fp64 references of the per-sample weight-gradient norm.

For white Gaussian operands both Gram matrices of
    ||gW_b||^2 = alpha^2 * sum_{p,p'} (GY GY^T)[p,p'] * (XU XU^T)[p,p']
are diagonal to within 1/sqrt(K) and 1/sqrt(C): the p != p' terms — the only ones that use the pixel-pair location tables, the border
validity of a tap for a PAIR of pixels and the symmetric tile handling — are then a 1e-4 .. 1e-7 share of the norm and a kernel that
got them wrong would pass a 1e-4 test.  offdiag_shares measures that share; tests/test_ghost_inputs.py holds the operands below to it.
Plain torch on the CPU.  Test infrastructure only.
"""
import torch
import torch.nn.functional as F

ALPHA = 2.5

# (kernel cslgan_last_kernel() must report, (N, H, W, C, K, R, stride, pad), run the dead-sample check on this case)
CASES = [
    ("gram_sqnorm_small_kernel", (5, 8, 8, 256, 512, 5, 2, 2), True),       # critic conv4
    ("gram_sqnorm_small_kernel", (3, 4, 4, 32, 64, 3, 1, 1), False),
    ("gram_sqnorm_small_kernel", (2, 7, 5, 64, 128, 5, 2, 2), False),
    ("gram_sqnorm_small_kernel", (4, 2, 2, 64, 64, 3, 1, 1), False),
    ("gram_sqnorm_small_kernel", (6, 8, 8, 32, 192, 3, 2, 1), False),
    ("gram_sqnorm_small_kernel", (130, 4, 4, 32, 64, 3, 1, 1), False),      # more samples than a wave of workgroups
    ("gram_sqnorm_cls64_kernel", (3, 16, 16, 128, 256, 5, 2, 2), True),     # critic conv3
    ("gram_sqnorm_cls64_kernel", (4, 6, 6, 32, 64, 3, 1, 1), False),
    ("gram_sqnorm_cls64_kernel", (3, 4, 4, 32, 32, 3, 1, 1), False),        # K % 64 != 0
    ("gram_sqnorm_cls64_kernel", (2, 7, 5, 64, 96, 5, 2, 2), False),
    ("gram_sqnorm_cls64_kernel", (2, 15, 13, 32, 64, 5, 2, 2), False),      # 8x7 outputs, four classes of different sizes
    ("gram_sqnorm_kernel<1>", (3, 9, 9, 32, 64, 5, 1, 0), True),            # 25 outputs, 81 input pixels
    ("gram_sqnorm_kernel<1>", (2, 12, 12, 32, 32, 3, 3, 0), False),         # stride 3
    ("gram_sqnorm_kernel<4>", (3, 10, 10, 32, 64, 3, 1, 0), True),          # 64 outputs
    ("gram_sqnorm_kernel<4>", (2, 12, 9, 32, 96, 5, 1, 0), False),          # 40 outputs
    ("sample_sqnorm_kernel<float>", (9, 1, 1, 8192, 1, 1, 1, 0), True),     # linear layers: the product of the two row norms
    ("sample_sqnorm_kernel<float>", (5, 1, 1, 794, 128, 1, 1, 0), False),
]
BF16_CASE = (5, 8, 8, 256, 512, 5, 2, 2)      # also run with both operands stored as bfloat16


def out_size(case):
    N, H, W, C, K, R, s, p = case
    return (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1


def correlated(N, C, H, W, g, rho=0.7):
    """A smooth field per channel (bilinear from a quarter-resolution grid) plus one offset per sample shared by every channel and
    pixel, mixed with white noise."""
    coarse = torch.randn(N, C, max(H // 4, 1), max(W // 4, 1), generator=g)
    field = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)
    return rho * (torch.randn(N, 1, 1, 1, generator=g) + field) + (1 - rho) * torch.randn(N, C, H, W, generator=g)


def operands(case):
    """(x [N,C,H,W] >= 0 with exact zeros, gy [N,K,P,Q] of mixed sign, six decades between the first and the last sample)."""
    N, H, W, C, K, R, s, p = case
    P, Q = out_size(case)
    g = torch.Generator().manual_seed(sum(case))
    x = torch.relu(correlated(N, C, H, W, g) + 0.5)
    gy = correlated(N, K, P, Q, g) * (10.0 ** torch.linspace(-3, 3, N))[:, None, None, None]
    return x, gy


def gaussian_operands(case):
    """The white-noise draw of test_wgrad_gram_norms_and_scaled_sum."""
    N, H, W, C, K, R, s, p = case
    P, Q = out_size(case)
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, C, H, W, generator=g)
    return x, torch.randn(N, K, P, Q, generator=g)


def _unfolded(x, R, stride, pad):
    """[N, C, T, PQ] in float64."""
    N, C = x.shape[:2]
    xu = F.unfold(x.double(), R, padding=pad, stride=stride)
    return xu.view(N, C, R * R, xu.shape[-1])


def reference_sq(x, gy, R, stride, pad, alpha):
    """fp64 [N]: squared norm of the materialised per-sample weight gradient alpha * GY_b^T XU_b (one matmul per sample)."""
    xu = _unfolded(x, R, stride, pad).flatten(1, 2)                  # [N, C*T, PQ]
    gm = gy.double().flatten(2)                                      # [N, K, PQ]
    return torch.stack([(gm[b] @ xu[b].t()).pow(2).sum() for b in range(x.shape[0])]) * float(alpha) ** 2


def reference_weighted_sum(x, gy, f, R, stride, pad, alpha):
    """fp64 [K, C, R, R]: sum_b f_b * alpha * gW_b, as one matmul over the (sample, pixel) rows."""
    N, C = x.shape[:2]
    K = gy.shape[1]
    xu = _unfolded(x, R, stride, pad).flatten(1, 2)                  # [N, C*T, PQ]
    gm = gy.double().flatten(2) * f.double().view(N, 1, 1)           # [N, K, PQ]
    gw = gm.permute(1, 0, 2).reshape(K, -1) @ xu.permute(1, 0, 2).reshape(C * R * R, -1).t()
    return gw.view(K, C, R, R) * float(alpha)


def offdiag_shares(x, gy, R, stride, pad):
    """Per sample, in fp64, of the terms G1[p,p'] * G2_t[p,p'] (G1 = GY GY^T, G2_t = tap t's part of XU XU^T):
    total: the share of sum_{p != p'} in the whole sum;
    tap:   the smallest |share| of one tap's p != p' terms, over the taps that have at least two output pixels whose input pixel is in
           range (a tap with fewer has no pair to get wrong);
    kappa: sum |terms| / sum terms, the condition number of the summation."""
    N, _, H, W = x.shape
    xu = _unfolded(x, R, stride, pad)                                # [N, C, T, PQ]
    gm = gy.double().flatten(2)                                      # [N, K, PQ]
    g1 = torch.einsum("bkp,bkq->bpq", gm, gm)
    g2 = torch.einsum("bctp,bctq->btpq", xu, xu)
    terms = g1[:, None] * g2                                         # [N, T, PQ, PQ]
    total = terms.sum((1, 2, 3))
    off_t = terms.sum((2, 3)) - torch.diagonal(terms, dim1=2, dim2=3).sum(2)        # [N, T]
    in_range = F.unfold(torch.ones(1, 1, H, W, dtype=torch.float64), R, padding=pad, stride=stride)[0]          # [T, PQ]
    pairs = in_range.sum(1) >= 2
    tap = (off_t.abs() / total[:, None])[:, pairs].min(1).values if pairs.any() else torch.zeros(N, dtype=torch.float64)
    return off_t.sum(1) / total, tap, terms.abs().sum((1, 2, 3)) / total
