"""The operands of the ghost-norm tests make the p != p' terms of the Gram formula visible (CPU, fp64 reference only).

A 1e-4 per-sample norm tolerance tests what contributes well over 1e-4 of the norm.  For every case of tests.ghost_inputs.CASES with more
than one output pixel, each sample must have
  - an off-diagonal share of at least 0.4 of its squared norm,
  - at least 1e-2 (100 x the tolerance) from the off-diagonal terms of its LEAST visible tap,
  - kappa = sum |terms| / sum terms <= 2, so the tolerance is not eaten by cancellation;
and white Gaussian operands on the critic's conv3 / conv4 shapes have a least-visible-tap share below 1e-4, which is why they do not
serve."""
import pytest
import torch

from tests.ghost_inputs import ALPHA, CASES, gaussian_operands, offdiag_shares, operands, out_size, reference_sq

CONV_CASES = [c for _, c, _ in CASES if out_size(c)[0] * out_size(c)[1] > 1]
CONV3, CONV4 = (3, 16, 16, 128, 256, 5, 2, 2), (5, 8, 8, 256, 512, 5, 2, 2)


def test_case_list_covers_every_route():
    assert CONV3 in CONV_CASES and CONV4 in CONV_CASES and len(CONV_CASES) == len(CASES) - 2
    assert {k for k, _, _ in CASES} == {"gram_sqnorm_small_kernel", "gram_sqnorm_cls64_kernel", "gram_sqnorm_kernel<1>",
                                        "gram_sqnorm_kernel<4>", "sample_sqnorm_kernel<float>"}
    for kernel in {k for k, _, _ in CASES}:
        assert sum(dead for k, _, dead in CASES if k == kernel) == 1, kernel        # one dead-sample run per kernel family


@pytest.mark.parametrize("case", CONV_CASES)
def test_correlated_operands_make_the_pixel_pairs_visible(case):
    N, H, W, C, K, R, s, p = case
    x, gy = operands(case)
    zeros = (x == 0).double().mean().item()
    total, tap, kappa = offdiag_shares(x, gy, R, s, p)
    print("%s: zeros %.3f  off-diagonal share >= %.3f  least visible tap >= %.2e  kappa <= %.3f"
          % (case, zeros, total.min().item(), tap.min().item(), kappa.max().item()))
    assert x.min().item() == 0.0 and 0.01 <= zeros <= 0.5, zeros                     # post-ReLU: exact zeros, most entries alive
    assert (gy > 0).any() and (gy < 0).any()
    sq = reference_sq(x, gy, R, s, p, ALPHA)
    assert sq.min().item() > 0 and sq.max().item() / sq.min().item() >= 1e6          # per-sample norms span decades
    assert total.min().item() >= 0.4, total
    assert tap.min().item() >= 1e-2, tap
    assert kappa.max().item() <= 2.0, kappa


@pytest.mark.parametrize("case", [CONV3, CONV4])
def test_white_gaussian_operands_hide_them(case):
    N, H, W, C, K, R, s, p = case
    total, tap, _ = offdiag_shares(*gaussian_operands(case), R, s, p)
    print("%s, Gaussian: off-diagonal share <= %.2e  least visible tap <= %.2e" % (case, total.abs().max().item(), tap.max().item()))
    assert tap.max().item() < 1e-4, tap


def test_reference_agrees_with_autograd():
    """reference_sq restates the per-sample gradient through F.unfold; autograd of F.conv2d is the independent statement."""
    import torch.nn.functional as F
    case = (2, 7, 5, 64, 96, 5, 2, 2)
    N, H, W, C, K, R, s, p = case
    x, gy = operands(case)
    w = torch.zeros(K, C, R, R, dtype=torch.float64, requires_grad=True)
    sq = []
    for b in range(N):
        y = F.conv2d(x[b:b + 1].double(), w, None, stride=s, padding=p)
        sq.append((torch.autograd.grad(y, w, gy[b:b + 1].double())[0] * ALPHA).pow(2).sum())
    torch.testing.assert_close(reference_sq(x, gy, R, s, p, ALPHA), torch.stack(sq), rtol=1e-12, atol=0)
