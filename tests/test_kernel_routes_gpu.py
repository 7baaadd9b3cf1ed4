"""The dispatch layer sends every launch to the same device kernel as the recorded fixture says.

tests/kernel_routes.json maps the cases of scripts/kernel_routes.py to the name cslgan_last_kernel() reported after the call, recorded
on the commit BEFORE the A/B environment switches were folded into constants (and unchanged by it).  The cases sit on both sides of
every numeric threshold of the conv dispatch — "<x>_at" exactly on it, "<x>_below" one tile or row block (a sample, or the four samples
of a 4x4-grid row block) under it — and on both sides of every shape rule that used to be a boolean switch.  Each threshold pair
resolves to two different names, with one exception the names cannot show: the x3 halo kernel's class pairing (256 paired
workgroups) changes the grid, not the kernel, so x3_pair_* record one name on both sides (the fp32 halo kernel's pairing, the same
helper, is visible as halo_pair_*).  The 128-wide rule of the stride-2 fp32 halo launches (>= 256 tiles) cannot be undercut either:
those launches start at 512 tiles (s2_halo_wide_*).

The thresholds decided in Python are integer functions; they are pinned without a GPU at the end of this file."""
import importlib.util
import json
import os

import pytest

from csl_gan_amd import ops

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_routes", os.path.join(_ROOT, "scripts", "kernel_routes.py"))
kernel_routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_routes)

with open(os.path.join(_ROOT, "tests", "kernel_routes.json")) as _f:
    ROUTES = json.load(_f)


def test_fixture_covers_every_case():
    assert set(ROUTES) == set(kernel_routes.CASES)


# threshold pairs whose two sides must be different kernels (the pair tests nothing otherwise)
_PAIRS = [("kc_t128_at", "kc_t128_below"), ("kc_t64_at", "kc_t64_below"), ("kc_tmc_at", "kc_tmc_below"), ("s2_halo_at", "s2_halo_below"),
          ("s2_halo_wide_at", "s2_halo_wide_below"), ("x3_quad_at", "x3_quad_below"), ("x3_quad_bf16_at", "x3_quad_bf16_below"),
          ("x3_quad_dgrad_at", "x3_quad_dgrad_below"), ("halo_quad_at", "halo_quad_below"), ("halo_pair_at", "halo_pair_below"),
          ("x3_wide_at", "x3_wide_below"), ("x3_wide_x3_at", "x3_wide_x3_below"), ("mc_wide64_at", "mc_wide64_below"),
          ("mc_wide64_at", "mc_wide64_ndim_below"), ("kcs_t128_at", "kcs_t128_below"),
          # shape rules: the default route against its ineligible neighbour
          ("c3_fwd", "c3_fwd_padded_rgb"), ("c3_wgrad", "c3_wgrad_padded_rgb"), ("conv1x1_c32", "conv1x1_c48"), ("conv1x1s_c32", "conv1x1s_c48"),
          ("linear_k1_fwd", "linear_k1_fwd_c128"), ("linear_k1_dgrad", "linear_k1_dgrad_c128"), ("skinny_k3", "skinny_k3_c32"),
          ("skinny_all_dgrad_s2", "skinny_dgrad_s1"), ("f32_halo_fwd", "f32_halo_fwd_off"), ("f32_halo_fwd_off", "f32_halo_fwd_off_c16"),
          ("f32_halo_fwd", "f32_halo_fwd_6x6"), ("x3_halo_fwd", "x3_halo_fwd_6x6"), ("bf16_halo_fwd", "bf16_halo_fwd_6x6"),
          ("x3_s2_fwd", "x3_s2_fwd_r4"), ("x3_dgrad_s1", "x3_dgrad_s1_c32"), ("wgh_s5", "wgh_s5_6x6"), ("x3w_s5", "x3w_s3"),
          ("x3w_quad", "x3w_quad_group1"), ("gram_small", "gram_cls64"), ("gram_cls64", "gram_100_pixels"), ("halos_fwd", "halos_fwd_8x8")]


@pytest.mark.parametrize("a,b", _PAIRS)
def test_fixture_pairs_resolve_differently(a, b):
    assert ROUTES[a] != ROUTES[b]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(kernel_routes.CASES))
def test_kernel_route(name):
    got, out = kernel_routes.run_case(kernel_routes.CASES[name])
    assert got == ROUTES[name]
    assert out.isfinite().all()


# ---- thresholds decided in Python (no GPU) ---------------------------------------------------------------------------------------------

def test_fp32_auto_forward_thresholds():
    """_kc_compute: the three-piece path from 32 tiles of 128x128, a reduction of 512 and 64 output channels on."""
    with ops.compute_dtype("fp32_auto"):
        assert ops._kc_compute(32 * 128, 128, 512) == ops.COMPUTE_BF16X3
        assert ops._kc_compute(31 * 128, 128, 512) == ops.COMPUTE_F32             # 31 tiles
        assert ops._kc_compute(16 * 128, 256, 512) == ops.COMPUTE_BF16X3           # 16 x 2 tiles
        assert ops._kc_compute(16 * 128, 129, 512) == ops.COMPUTE_BF16X3
        assert ops._kc_compute(16 * 128, 128, 512) == ops.COMPUTE_F32             # 16 x 1 tiles
        assert ops._kc_compute(32 * 128, 128, 511) == ops.COMPUTE_F32             # reduction one short
        assert ops._kc_compute(64 * 128, 64, 512) == ops.COMPUTE_BF16X3
        assert ops._kc_compute(64 * 128, 63, 512) == ops.COMPUTE_F32
    for mode, comp in (("fp32", ops.COMPUTE_F32), ("bf16", ops.COMPUTE_BF16), ("bf16x3", ops.COMPUTE_BF16X3)):
        with ops.compute_dtype(mode):       # outside fp32_auto the mode decides alone
            assert ops._kc_compute(32 * 128, 128, 512) == comp and ops._kc_compute(128, 64, 64) == comp


def test_fp32_auto_wgrad_threshold():
    """_conv_desc's weight-gradient clause: a 5x5 64 -> 64 conv on an 8x8 grid is 13,107,200 FLOP per sample, so 39 samples are the
    first batch at or above 0.5 GFLOP (no batch of such a layer lands on it exactly: K and C carry 2^12, 0.5e9 / 50 only 2^7)."""
    def comp(N, **kw):
        a = dict(H=8, W=8, Cc=64, K=64, R=5, S=5, stride=1, pad=2)
        a.update(kw)
        return ops._conv_desc(N, a["H"], a["W"], a["Cc"], a["K"], a["R"], a["S"], a["stride"], a["pad"], kind="wgrad", group=a.get("group"))[0].compute

    with ops.compute_dtype("fp32_auto"):
        assert 2.0 * 39 * 64 * 64 * 25 * 64 >= 0.5e9 > 2.0 * 38 * 64 * 64 * 25 * 64
        assert comp(39) == ops.COMPUTE_BF16X3
        assert comp(38) == ops.COMPUTE_F32
        assert comp(64, R=3, S=3, pad=1) == ops.COMPUTE_F32                        # three filter columns: exact fp32
        assert comp(64, Cc=32) == ops.COMPUTE_F32
        assert comp(64, H=6, W=6) == ops.COMPUTE_F32                               # 6x6 output: not 8x8-patchable
        assert comp(160, H=8, W=8, stride=2, group=2) == ops.COMPUTE_BF16X3        # the 4x4-output form needs an even group
        assert comp(160, H=8, W=8, stride=2, group=1) == ops.COMPUTE_F32
    with ops.compute_dtype("fp32"):
        assert comp(64) == ops.COMPUTE_F32


def test_gram_norms_preferred_pixel_limit():
    """Ghost clipping up to 64 output pixels and 64 input pixels per stride-parity class."""
    assert ops.gram_norms_preferred((8, 8, 8, 64), (8, 8, 8, 32), 1)                 # 64 / 64
    assert not ops.gram_norms_preferred((8, 5, 13, 64), (8, 8, 8, 32), 1)            # 65 output pixels
    assert not ops.gram_norms_preferred((8, 8, 8, 64), (8, 5, 13, 32), 1)            # 65 input pixels
    assert ops.gram_norms_preferred((8, 8, 8, 64), (8, 16, 16, 32), 2)               # 256 input pixels, 64 per parity class
    assert not ops.gram_norms_preferred((8, 8, 8, 64), (8, 17, 16, 32), 2)           # 9 x 8 = 72 per class
