"""What does the conv dispatch layer of csl_gan_amd.ops ask the library to do?  A call log, taken without a GPU.

The layer is host logic: it picks a C entry point, a descriptor, a workspace size, an output dtype and a timer tag.  Here it runs on
small zero-filled CPU tensors against a stand-in for the library that records every call and launches nothing:

  _lib.lib                 returns the recorder (any cslgan_* attribute appends a record and returns 0)
  ops._stream              returns None
  torch.Tensor.is_cuda     reads True, which switches the "must be a device tensor" test off
  ops.repack_cache.get     logs (kind, numel, wkey given, version given), then runs the original with wkey=None (no stream is asked for)
  ops._timer               a stand-in with only = None that logs (name, flop, nbytes, exec_flop, tag)

A record holds the entry name, every int and float argument, the scalar fields of a byref(ConvT) (its pointer fields as null / set) and,
for each pointer, where it points: null, "<input name>+offset", "ws+offset" (a workspace the wrapped get returned) or "new".

    python scripts/conv_dispatch_log.py                         # entry names per case
    python scripts/conv_dispatch_log.py --case fwd_s1_r3_fp32   # the full log of one case
    python scripts/conv_dispatch_log.py --time                  # host time of the whole list, no timer installed
    python scripts/conv_dispatch_log.py --root ../parent --record tests/conv_dispatch_calls.json

tests/conv_dispatch_calls.json holds, per case, the ordered entry names and a SHA-1 of the canonical JSON of the full log, recorded
with --root pointing at a checkout of the commit BEFORE the dispatch layer was rewritten around one geometry record;
tests/test_conv_dispatch.py asserts them.  Only names both sides have are patched, so the script runs unchanged on that commit.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The conv entry points the layer can reach: every case list must reach all of them (tests/test_conv_dispatch.py).
CONV_ENTRIES = sorted("cslgan_" + n for n in (
    "conv2d_fwd_f32", "conv2d_fwd_x3_f32", "conv2d_s2_fwd_f32", "conv2d_s2_fwd_x3_f32", "conv2d_fwd_bf16s", "conv2d_fwd_skinny_bf16in",
    "conv2d_c3_fwd_bf16out", "conv2d_dgrad_f32", "conv2d_dgrad_x3_f32", "conv2d_dgrad_bf16s", "conv2d_dgrad_skinny_bf16in",
    "linear_k1_dgrad_bf16s", "conv2d_wgrad_grouped_f32", "conv2d_wgrad_grouped_bf16out_f32", "conv2d_wgrad_scaled_f32",
    "conv2d_wgrad_grouped_bf16s", "conv2d_wgrad_scaled_bf16s", "conv2d_c3_wgrad_bf16gy", "linear_k1_wgrad_bf16s",
    "conv2d_wgrad_blocks_f32", "conv2d_wgrad_skinny_f32", "conv2d_wgrad_sqnorm_gram_f32"))


def is_conv_entry(name):
    return name.startswith(("cslgan_conv2d_", "cslgan_linear_k1_"))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

def T(*shape, dt="f32"):
    """A zero-filled tensor argument ("f32", "bf16", "f64"; "f32t": fp32 with its last two dimensions transposed, so not contiguous)."""
    return ("T", shape, dt)


def B(*shape):
    return T(*shape, dt="bf16")


KEY = dict(wkey="k", wversion=3)        # a dummy module token and version: the log shows that they reach repack_cache.get


def _fwd(x, w, **kw):
    kw.setdefault("pad", w[1][1] // 2)
    if "wkey" not in kw:
        kw.update(KEY)
    return ("conv2d_fwd", dict(x=x, w=w, **kw))


def _dgrad(gy, w, in_hw, **kw):
    kw.setdefault("pad", w[1][1] // 2)
    kw.setdefault("wkey", "k")
    return ("conv2d_dgrad", dict(gy=gy, w=w, in_hw=in_hw, **kw))


def _wg(fn, gy, x, R, **kw):
    kw.setdefault("pad", R // 2)
    return (fn, dict(gy=gy, x=x, R=R, S=R, **kw))


def _grouped(gy, x, R, **kw):
    return _wg("conv2d_wgrad_grouped", gy, x, R, **kw)


def _dense(gy, x, R, **kw):
    return _wg("conv2d_wgrad_dense", gy, x, R, **kw)


def _gram(gy, x, R, **kw):
    return _wg("conv2d_wgrad_sqnorm_gram", gy, x, R, **kw)


def _blocks(gy, x, R, blocks, **kw):
    kw.setdefault("stride", 1)
    return _wg("conv2d_wgrad_blocks", gy, x, R, alpha=0.5, blocks=blocks, **kw)


MODES = ("fp32", "bf16", "bf16x3", "fp32_auto")
AFF = (T(2, 16), T(2, 16), True)

# name -> (ops function, arguments).  Arguments that start with "_" are settings: _mode (compute dtype), _halo (set_f32_halo),
# _split (ops._X3_SPLIT), _gn (a pending gn_partials request of that many groups), _gn_fuse (ops._GN_FUSE).
CASES = {}


def _add(name, case):
    assert name not in CASES, name
    CASES[name] = case


# ---- forward
for m in MODES:
    _add("fwd_s1_r3_" + m, _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), _mode=m))
    _add("fwd_s1_r5_" + m, _fwd(T(2, 8, 8, 16), T(64, 5, 5, 16), _mode=m, bias=T(64), act=1))
    _add("fwd_s1_r1_" + m, _fwd(T(2, 8, 8, 16), T(64, 1, 1, 16), _mode=m))
    _add("fwd_s2_r3_" + m, _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), stride=2, _mode=m))
    _add("fwd_s2_r5_" + m, _fwd(T(2, 8, 8, 16), T(64, 5, 5, 16), stride=2, _mode=m, bias=T(64), act=2))
    _add("fwd_s2_r4_" + m, _fwd(T(2, 8, 8, 16), T(64, 4, 4, 16), stride=2, pad=1, _mode=m))
_add("fwd_s1_r4", _fwd(T(2, 8, 8, 16), T(64, 4, 4, 16), pad=1))
_add("fwd_s1_r3_halo_off", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), _halo=False))
_add("fwd_s2_r5_halo_off_c32", _fwd(T(2, 8, 8, 32), T(64, 5, 5, 32), stride=2, _halo=False))
_add("fwd_s2_r5_halo_off_c16", _fwd(T(2, 8, 8, 16), T(64, 5, 5, 16), stride=2, _halo=False))
_add("fwd_s2_r3_halo_off_c32_residual", _fwd(T(2, 8, 8, 32), T(64, 3, 3, 32), stride=2, _halo=False, residual=T(2, 4, 4, 64)))
_add("fwd_auto_at", _fwd(T(8, 16, 16, 64), T(256, 3, 3, 64), _mode="fp32_auto"))            # 16 x 2 tiles of 128x128, reduction 576
_add("fwd_auto_below", _fwd(T(7, 16, 16, 64), T(256, 3, 3, 64), _mode="fp32_auto"))         # 14 x 2 tiles
_add("fwd_auto_short_k", _fwd(T(8, 16, 16, 32), T(256, 3, 3, 32), _mode="fp32_auto"))       # reduction 288
_add("fwd_auto_at_halo_off", _fwd(T(8, 16, 16, 64), T(256, 3, 3, 64), _mode="fp32_auto", _halo=False))
_add("fwd_auto_below_halo_off", _fwd(T(7, 16, 16, 64), T(256, 3, 3, 64), _mode="fp32_auto", _halo=False))
_add("fwd_s1_all_extras",_fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), bias=T(64), residual=T(2, 8, 8, 64), out=T(2, 8, 8, 64), act=1))
_add("fwd_generic_all_extras", _fwd(T(2, 8, 8, 16), T(64, 1, 1, 16), bias=T(64), residual=T(2, 8, 8, 64), out=T(2, 8, 8, 64), act=3))
_add("fwd_s2_residual", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), stride=2, residual=T(2, 4, 4, 64)))
_add("fwd_no_wkey", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), wkey=None))
_add("fwd_alg_scale", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), alg_scale=4.0))
_add("fwd_out_bf16", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), out_dtype="bf16"))
_add("fwd_out_bf16_into_out", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), out_dtype="bf16", out=B(2, 8, 8, 64), bias=T(64)))
_add("fwd_residual_bf16", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), residual=B(2, 8, 8, 64)))
_add("fwd_in_affine_halo", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), in_affine=AFF))
_add("fwd_in_affine_x3", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), in_affine=(T(2, 16), T(2, 16), False), _mode="bf16x3"))
_add("fwd_in_affine_k3", _fwd(T(2, 8, 8, 64), T(3, 3, 3, 64), in_affine=(T(2, 64), T(2, 64), True), bias=T(3), act=3))
_add("fwd_gn_accepted", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), _gn=32))
_add("fwd_gn_accepted_k128", _fwd(T(2, 16, 16, 16), T(128, 3, 3, 16), _gn=32, bias=T(128)))
_add("fwd_gn_refused_act", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), _gn=32, act=2))
_add("fwd_gn_refused_k96", _fwd(T(2, 8, 8, 16), T(96, 3, 3, 16), _gn=32))
_add("fwd_gn_other_route", _fwd(T(2, 8, 8, 16), T(64, 1, 1, 16), _gn=32))                   # not the stride-1 halo kernel: stays pending
_add("fwd_gn_fuse_off", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), _gn=32, _gn_fuse=False))
_add("fwd_bf16_x", _fwd(B(2, 8, 8, 16), T(64, 3, 3, 16)))
_add("fwd_bf16_x_extras", _fwd(B(2, 8, 8, 16), T(64, 3, 3, 16), bias=T(64), residual=B(2, 8, 8, 64), out=B(2, 8, 8, 64), act=1, alg_scale=4.0))
_add("fwd_bf16_x_residual_f32", _fwd(B(2, 8, 8, 16), T(64, 3, 3, 16), residual=T(2, 8, 8, 64), stride=1))
_add("fwd_bf16_x_out_f32", _fwd(B(2, 8, 8, 16), T(64, 3, 3, 16), out_dtype="f32"))
_add("fwd_bf16_x_s2", _fwd(B(2, 8, 8, 16), T(64, 5, 5, 16), stride=2))
_add("fwd_bf16_x_c12", _fwd(B(2, 8, 8, 12), T(64, 3, 3, 12)))
_add("fwd_bf16_x_c12_into_out", _fwd(B(2, 8, 8, 12), T(64, 3, 3, 12), out=B(2, 8, 8, 64)))
_add("fwd_bf16_x_head", _fwd(B(4, 1, 1, 64), T(1, 1, 1, 64)))
_add("fwd_bf16_x_k3_c64", _fwd(B(2, 8, 8, 64), T(3, 3, 3, 64), bias=T(3), act=3))
_add("fwd_bf16_x_k3_c32", _fwd(B(2, 8, 8, 32), T(3, 3, 3, 32)))
_add("fwd_bf16_x_k3_c64_out", _fwd(B(2, 8, 8, 64), T(3, 3, 3, 64), out=T(2, 8, 8, 3)))
_add("fwd_k3_c64", _fwd(T(2, 8, 8, 64), T(3, 3, 3, 64)))
_add("fwd_k3_c32", _fwd(T(2, 8, 8, 32), T(3, 3, 3, 32)))
_add("fwd_rgb_first_layer", _fwd(T(2, 32, 32, 3), T(64, 5, 5, 3), stride=2, bias=T(64)))
_add("fwd_rgb_24x24", _fwd(T(2, 24, 24, 3), T(64, 5, 5, 3), stride=2, bias=T(64)))
_add("fwd_rgb_first_layer_residual", _fwd(T(2, 32, 32, 3), T(64, 5, 5, 3), stride=2, residual=T(2, 16, 16, 64)))
_add("fwd_rgb_1x1", _fwd(T(2, 8, 8, 3), T(64, 1, 1, 3)))
_add("fwd_rgb_first_layer_bf16_out", _fwd(T(2, 32, 32, 3), T(64, 5, 5, 3), stride=2, out_dtype="bf16", bias=T(64), act=1))
_add("fwd_rgb_24x24_bf16_out", _fwd(T(2, 24, 24, 3), T(64, 5, 5, 3), stride=2, out_dtype="bf16"))
_add("fwd_split8_s2", _fwd(T(2, 8, 8, 64), T(64, 5, 5, 64), stride=2, _split=8))
_add("fwd_split8_s2_c16", _fwd(T(2, 8, 8, 16), T(64, 5, 5, 16), stride=2, _split=8))         # one 16-channel chunk: nothing to split
_add("err_fwd_channels", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 32)))
_add("err_fwd_residual_shape", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), residual=T(2, 8, 8, 32)))
_add("err_fwd_stored_out_dtype", _fwd(B(2, 8, 8, 16), T(64, 3, 3, 16), out=T(2, 8, 8, 64)))
_add("err_fwd_in_affine_shape", _fwd(T(2, 8, 8, 16), T(64, 3, 3, 16), in_affine=(T(2, 8), T(2, 16), True)))
_add("err_fwd_x_f64", _fwd(T(2, 8, 8, 16, dt="f64"), T(64, 3, 3, 16)))
_add("err_fwd_w_not_contiguous", _fwd(T(2, 8, 8, 16), T(64, 3, 16, 3, dt="f32t")))

# ---- data gradient
for m in MODES:
    _add("dgrad_s1_r3_" + m, _dgrad(T(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), _mode=m))
    _add("dgrad_s2_r3_" + m, _dgrad(T(2, 4, 4, 64), T(64, 3, 3, 64), (8, 8), stride=2, _mode=m, mask=T(2, 8, 8, 64)))
    _add("dgrad_s2_r5_" + m, _dgrad(T(2, 4, 4, 64), T(64, 5, 5, 64), (8, 8), stride=2, _mode=m))
    _add("dgrad_c32_" + m, _dgrad(T(2, 8, 8, 64), T(64, 3, 3, 32), (8, 8), _mode=m, mask=T(2, 8, 8, 32)))
_add("dgrad_s1_r3_halo_off", _dgrad(T(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), _halo=False))
_add("dgrad_auto_at", _dgrad(T(8, 16, 16, 64), T(64, 3, 3, 256), (16, 16), _mode="fp32_auto"))
_add("dgrad_auto_below", _dgrad(T(7, 16, 16, 64), T(64, 3, 3, 256), (16, 16), _mode="fp32_auto"))
_add("dgrad_auto_at_halo_off", _dgrad(T(8, 16, 16, 64), T(64, 3, 3, 256), (16, 16), _mode="fp32_auto", _halo=False))
_add("dgrad_auto_below_halo_off", _dgrad(T(7, 16, 16, 64), T(64, 3, 3, 256), (16, 16), _mode="fp32_auto", _halo=False))
_add("dgrad_split8",_dgrad(T(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), _split=8, mask=T(2, 8, 8, 64)))
_add("dgrad_r1", _dgrad(T(2, 8, 8, 64), T(64, 1, 1, 64), (8, 8), wkey=None))
_add("dgrad_bf16_gy", _dgrad(B(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8)))
_add("dgrad_bf16_gy_s2_mask_f32", _dgrad(B(2, 4, 4, 64), T(64, 5, 5, 64), (8, 8), stride=2, mask=T(2, 8, 8, 64)))
_add("dgrad_bf16_gy_mask_bf16", _dgrad(B(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), mask=B(2, 8, 8, 64)))
_add("dgrad_bf16_gy_out_f32", _dgrad(B(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), out_dtype="f32", mask=B(2, 8, 8, 64)))
_add("dgrad_bf16_gy_k12", _dgrad(B(2, 8, 8, 12), T(12, 3, 3, 64), (8, 8)))
_add("dgrad_out_bf16", _dgrad(T(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), out_dtype="bf16"))
_add("dgrad_mask_bf16", _dgrad(T(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), mask=B(2, 8, 8, 64)))
_add("dgrad_head", _dgrad(T(4, 1, 1, 1), T(1, 1, 1, 64), (1, 1), out_dtype="bf16"))
_add("dgrad_head_mask", _dgrad(T(4, 1, 1, 1), T(1, 1, 1, 64), (1, 1), out_dtype="bf16", mask=T(4, 1, 1, 64)))
_add("dgrad_head_c12", _dgrad(T(4, 1, 1, 1), T(1, 1, 1, 12), (1, 1), out_dtype="bf16"))
_add("dgrad_image_bf16_gy_s2", _dgrad(B(2, 8, 8, 64), T(64, 5, 5, 3), (16, 16), stride=2))
_add("dgrad_image_bf16_gy_s1", _dgrad(B(2, 8, 8, 64), T(64, 3, 3, 3), (8, 8)))
_add("dgrad_image_bf16_gy_s1_r5", _dgrad(B(2, 8, 8, 64), T(64, 5, 5, 3), (8, 8)))
_add("dgrad_image_bf16_gy_mask", _dgrad(B(2, 8, 8, 64), T(64, 5, 5, 3), (16, 16), stride=2, mask=T(2, 16, 16, 3)))
_add("dgrad_image_f32", _dgrad(T(2, 8, 8, 64), T(64, 5, 5, 3), (16, 16), stride=2))
_add("err_dgrad_inconsistent", _dgrad(T(2, 8, 8, 64), T(64, 3, 3, 64), (16, 16)))
_add("err_dgrad_mask_shape", _dgrad(T(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), mask=T(2, 8, 8, 32)))
_add("err_dgrad_stored_mask_shape", _dgrad(B(2, 8, 8, 64), T(64, 3, 3, 64), (8, 8), mask=B(2, 8, 8, 32)))

# ---- weight gradient
GY, X = (4, 8, 8, 64), (4, 8, 8, 64)
for m in MODES:
    _add("wgrad_g1_" + m, _grouped(T(*GY), T(*X), 3, _mode=m))
    _add("wgrad_g2_r5_" + m, _grouped(T(*GY), T(*X), 5, group=2, alpha=0.5, sq=T(2), _mode=m))
_add("wgrad_linear_bf16_mode", _grouped(T(4, 1, 1, 64), T(4, 1, 1, 32), 1, _mode="bf16"))         # small linear layer: exact fp32
_add("wgrad_auto_at", _grouped(T(39, 8, 8, 64), T(39, 8, 8, 64), 5, _mode="fp32_auto"))           # 0.511 GFLOP
_add("wgrad_auto_below", _grouped(T(38, 8, 8, 64), T(38, 8, 8, 64), 5, _mode="fp32_auto"))        # 0.498 GFLOP
_add("wgrad_auto_quad_g2", _grouped(T(160, 4, 4, 64), T(160, 8, 8, 64), 5, stride=2, group=2, _mode="fp32_auto"))
_add("wgrad_auto_quad_g1", _grouped(T(160, 4, 4, 64), T(160, 8, 8, 64), 5, stride=2, group=1, _mode="fp32_auto"))
_add("wgrad_normonly_scratch", _grouped(T(8, 8, 8, 64), T(8, 8, 8, 16), 3, group=8, want_gw=False, sq=T(1)))      # 8 x 64 = 512 pixels per group
_add("wgrad_normonly_no_scratch", _grouped(T(8, 8, 8, 64), T(8, 8, 8, 16), 3, group=4, want_gw=False, sq=T(2)))   # 256 pixels per group
_add("wgrad_nothing_wanted", _grouped(T(*GY), T(*X), 3, want_gw=False))
_add("wgrad_out_f32", _grouped(T(*GY), T(*X), 3, out=T(4, 64, 3, 3, 64), sq=T(4)))
_add("wgrad_out_bf16", _grouped(T(*GY), T(*X), 3, group=2, out=B(2, 64, 3, 3, 64)))
_add("wgrad_row_scale", _grouped(T(*GY), T(*X), 3, group=4, row_scale=T(4)))
_add("wgrad_row_scale_out", _grouped(T(*GY), T(*X), 3, group=2, row_scale=T(4), out=T(2, 64, 3, 3, 64)))
_add("wgrad_s2", _grouped(T(4, 4, 4, 64), T(*X), 3, stride=2))
_add("wgrad_stored", _grouped(B(*GY), B(*X), 3))
_add("wgrad_stored_g2_sq", _grouped(B(*GY), B(*X), 3, group=2, sq=T(2), alpha=0.5))
_add("wgrad_stored_normonly", _grouped(B(*GY), B(*X), 3, want_gw=False, sq=T(4)))
_add("wgrad_stored_out_bf16", _grouped(B(*GY), B(*X), 3, out=B(4, 64, 3, 3, 64)))
_add("wgrad_stored_out_f32", _grouped(B(*GY), B(*X), 3, out=T(4, 64, 3, 3, 64)))
_add("wgrad_stored_row_scale", _grouped(B(*GY), B(*X), 3, group=4, row_scale=T(4)))
_add("wgrad_stored_row_scale_16px", _grouped(B(4, 4, 4, 64), B(4, 4, 4, 64), 3, group=4, row_scale=T(4)))       # a K tile would span samples
_add("err_wgrad_stored_row_scale_out_bf16", _grouped(B(*GY), B(*X), 3, group=4, row_scale=T(4), out=B(1, 64, 3, 3, 64)))
_add("wgrad_stored_nothing_wanted", _grouped(B(*GY), B(*X), 3, want_gw=False))
_add("wgrad_stored_c12", _grouped(B(*GY), B(4, 8, 8, 12), 3))
_add("wgrad_bf16_gy_f32_x", _grouped(B(*GY), T(*X), 3))
_add("wgrad_head", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1))
_add("wgrad_head_g8_sq", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, group=8, sq=T(1), alpha=2.0))
_add("wgrad_head_normonly", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, want_gw=False, sq=T(8)))
_add("wgrad_head_out", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, group=2, out=T(4, 1, 1, 1, 64)))
_add("wgrad_head_row_scale", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, group=8, row_scale=T(8)))
_add("wgrad_head_out_bf16", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, out=B(8, 1, 1, 1, 64)))
_add("wgrad_head_c12", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 12), 1))
_add("wgrad_rgb_layer_mixed", _grouped(B(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2))
_add("wgrad_rgb_layer_mixed_sq", _grouped(B(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, want_gw=False, sq=T(2), alpha=0.5))
_add("wgrad_rgb_layer_mixed_out", _grouped(B(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, out=T(2, 64, 5, 5, 3), sq=T(2)))
_add("wgrad_rgb_layer_mixed_g2", _grouped(B(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, group=2))
_add("wgrad_rgb_layer_mixed_row_scale", _grouped(B(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, row_scale=T(2)))
_add("wgrad_rgb_layer_mixed_24x24", _grouped(B(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2))
_add("wgrad_rgb_layer", _grouped(T(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, sq=T(2)))
_add("wgrad_rgb_layer_normonly", _grouped(T(8, 16, 16, 64), T(8, 32, 32, 3), 5, stride=2, want_gw=False, sq=T(8)))
_add("wgrad_rgb_layer_out_bf16", _grouped(T(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, out=B(2, 64, 5, 5, 3)))
_add("wgrad_rgb_24x24", _grouped(T(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2))
_add("wgrad_rgb_24x24_out_sq", _grouped(T(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2, out=T(2, 64, 5, 5, 3), sq=T(2)))
_add("wgrad_rgb_24x24_normonly", _grouped(T(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2, want_gw=False, sq=T(2)))
_add("wgrad_rgb_24x24_g2", _grouped(T(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2, group=2))
_add("wgrad_rgb_24x24_row_scale", _grouped(T(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2, row_scale=T(2)))
_add("wgrad_rgb_1x1", _grouped(T(2, 8, 8, 16), T(2, 8, 8, 3), 1))
_add("err_wgrad_inconsistent", _grouped(T(*GY), T(4, 16, 16, 64), 3))
_add("err_wgrad_batch", _grouped(T(2, 8, 8, 64), T(*X), 3))
_add("err_wgrad_group", _grouped(T(*GY), T(*X), 3, group=3))
_add("err_wgrad_row_scale_sq", _grouped(T(*GY), T(*X), 3, row_scale=T(4), sq=T(4)))
_add("err_wgrad_row_scale_size", _grouped(T(*GY), T(*X), 3, row_scale=T(3)))
_add("err_wgrad_stored_inconsistent", _grouped(B(*GY), B(4, 16, 16, 64), 3))
_add("err_wgrad_stored_group", _grouped(B(*GY), B(*X), 3, group=3))
_add("err_wgrad_stored_row_scale_size", _grouped(B(*GY), B(*X), 3, row_scale=T(3)))
_add("err_wgrad_head_row_scale_size", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, row_scale=T(4)))
_add("err_wgrad_head_row_scale_sq", _grouped(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, row_scale=T(8), sq=T(8)))

_add("blocks_mixed", _blocks(T(*GY), T(*X), 3, [(2, T(2, 64 * 9 * 64), None), (1, None, T(1)), (1, None, None)]))
_add("blocks_both_s2_r5", _blocks(T(4, 4, 4, 64), T(*X), 5, [(3, T(3, 64 * 25 * 64), T(3)), (1, T(1, 64 * 25 * 64), T(1))], stride=2))
_add("err_blocks_rows", _blocks(T(*GY), T(*X), 3, [(2, None, None), (1, None, None)]))
_add("err_blocks_gw_size", _blocks(T(*GY), T(*X), 3, [(4, T(4, 64), None)]))
_add("err_blocks_sq_size", _blocks(T(*GY), T(*X), 3, [(4, None, T(3))]))

_add("dense", _dense(T(*GY), T(*X), 3))
_add("dense_rows", _dense(T(*GY), T(*X), 3, want_rows=True, alpha=0.5))
_add("dense_rows_and_out", _dense(T(*GY), T(*X), 3, want_rows=True, out=T(64 * 9 * 64)))
_add("dense_out", _dense(T(*GY), T(*X), 3, out=T(64 * 9 * 64)))
_add("dense_row_scale", _dense(T(*GY), T(*X), 3, row_scale=T(4)))
_add("dense_one_sample", _dense(T(1, 8, 8, 64), T(1, 8, 8, 64), 3))
_add("dense_one_sample_out", _dense(T(1, 8, 8, 64), T(1, 8, 8, 64), 3, out=T(64 * 9 * 64)))
_add("dense_c32_s2", _dense(T(8, 4, 4, 64), T(8, 8, 8, 32), 5, stride=2))
_add("dense_bf16_mode", _dense(T(*GY), T(*X), 3, _mode="bf16"))
_add("dense_k3", _dense(T(2, 8, 8, 3), T(2, 8, 8, 64), 3, alpha=0.5))
_add("dense_k3_out", _dense(T(2, 8, 8, 3), T(2, 8, 8, 64), 3, out=T(3 * 9 * 64)))
_add("dense_k3_r1", _dense(T(2, 8, 8, 3), T(2, 8, 8, 64), 1))
_add("dense_k3_c32", _dense(T(2, 8, 8, 3), T(2, 8, 8, 32), 3))
_add("dense_k3_row_scale", _dense(T(2, 8, 8, 3), T(2, 8, 8, 64), 3, row_scale=T(2)))
_add("dense_k3_bf16_x", _dense(T(2, 8, 8, 3), B(2, 8, 8, 64), 3))
_add("dense_head", _dense(T(8, 1, 1, 1), B(8, 1, 1, 64), 1))
_add("dense_head_n6_out", _dense(T(6, 1, 1, 1), B(6, 1, 1, 64), 1, out=T(64), alpha=0.5))
_add("dense_head_row_scale", _dense(T(8, 1, 1, 1), B(8, 1, 1, 64), 1, row_scale=T(8)))
_add("dense_head_c12", _dense(T(8, 1, 1, 1), B(8, 1, 1, 12), 1))
_add("dense_rgb_layer_mixed", _dense(B(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2))
_add("dense_rgb_layer_mixed_row_scale", _dense(B(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, row_scale=T(2)))
_add("dense_rgb_layer", _dense(T(2, 16, 16, 64), T(2, 32, 32, 3), 5, stride=2, out=T(64 * 25 * 3)))
_add("dense_rgb_24x24", _dense(T(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2))
_add("dense_rgb_24x24_mixed", _dense(B(2, 12, 12, 64), T(2, 24, 24, 3), 5, stride=2))
_add("dense_stored", _dense(B(*GY), B(*X), 3))
_add("dense_stored_row_scale", _dense(B(*GY), B(*X), 3, row_scale=T(4), want_rows=True))
_add("dense_stored_row_scale_16px", _dense(B(4, 4, 4, 64), B(4, 4, 4, 64), 3, row_scale=T(4)))
_add("dense_stored_c12", _dense(B(*GY), B(4, 8, 8, 12), 3))
_add("err_dense_k3_inconsistent", _dense(T(2, 8, 8, 3), T(2, 8, 8, 64), 3, pad=0))

_add("gram_linear", _gram(T(4, 1, 1, 64), T(4, 1, 1, 32), 1, alpha=0.5))
_add("gram_16px", _gram(T(4, 4, 4, 64), T(4, 4, 4, 32), 3))
_add("gram_16px_s2", _gram(T(4, 4, 4, 64), T(4, 8, 8, 32), 3, stride=2, sq=T(4), alpha=0.5))
_add("gram_64px", _gram(T(4, 8, 8, 64), T(4, 8, 8, 32), 3))
_add("gram_64px_s2", _gram(T(4, 8, 8, 64), T(4, 16, 16, 32), 5, stride=2))
_add("gram_100px", _gram(T(4, 10, 10, 32), T(4, 10, 10, 32), 3))
_add("gram_bf16", _gram(B(4, 4, 4, 64), B(4, 4, 4, 32), 3))
_add("gram_bf16_mode", _gram(T(4, 4, 4, 64), T(4, 4, 4, 32), 3, _mode="bf16"))
_add("err_gram_inconsistent", _gram(T(4, 4, 4, 64), T(4, 8, 8, 32), 3))
_add("err_gram_sq_size", _gram(T(4, 4, 4, 64), T(4, 4, 4, 32), 3, sq=T(3)))

# ---- the other wrappers of the section, and the shape rules other modules ask about
_add("depth_to_space", ("depth_to_space", dict(x=T(2, 4, 4, 16))))
_add("depth_to_space_inverse_bf16", ("depth_to_space", dict(x=B(2, 8, 8, 4), inverse=True)))
_add("fold_channels4", ("fold_channels4", dict(w=T(8, 3, 3, 16), wkey="k")))
_add("unfold_channels4", ("unfold_channels4", dict(gwf=T(8, 3, 3, 4))))
_add("cast_bf16", ("cast_bf16", dict(t=T(2, 4, 4, 8))))
_add("cast_bf16_any_order", ("cast_bf16", dict(t=T(2, 4, 8, 4, dt="f32t"))))           # dense, not contiguous: the casts take it
_add("cast_f32", ("cast_f32", dict(t=B(2, 4, 4, 8))))
_add("cast_f32_to_u8", ("f32_to_u8", dict(src=T(2, 4, 8, 4, dt="f32t"), scale=0.5, bias=0.5)))
_add("err_cast_bf16_f64", ("cast_bf16", dict(t=T(2, 4, dt="f64"))))
_add("err_depth_to_space_channels", ("depth_to_space", dict(x=T(2, 4, 4, 6))))
_add("err_depth_to_space_odd", ("depth_to_space", dict(x=T(2, 5, 4, 4), inverse=True)))
_add("err_fold_channels4", ("fold_channels4", dict(w=T(8, 3, 3, 6))))
for m in MODES:
    _add("rule_in_affine_ok_" + m, ("in_affine_ok", dict(x=T(2, 8, 8, 16), w=T(64, 3, 3, 16), stride=1, pad=1, _mode=m)))
    _add("rule_blocks_s5_" + m, ("wgrad_blocks_eligible", dict(gy_shape=GY, x_shape=X, R=5, S=5, stride=1, _mode=m)))
    _add("rule_blocks_s3_" + m, ("wgrad_blocks_eligible", dict(gy_shape=GY, x_shape=X, R=3, S=3, stride=2, _mode=m)))
    _add("rule_dense_group_" + m, ("dense_wgrad_group", dict(N=64, K=128, Cc=64, R=5, S=5, PQ=64, stride=1, out_hw=(8, 8), _mode=m)))
_add("rule_in_affine_ok_halo_off", ("in_affine_ok", dict(x=T(2, 8, 8, 16), w=T(64, 3, 3, 16), stride=1, pad=1, _halo=False)))
_add("rule_in_affine_ok_s2", ("in_affine_ok", dict(x=T(2, 8, 8, 16), w=T(64, 3, 3, 16), stride=2, pad=1)))
_add("rule_in_affine_ok_6x6", ("in_affine_ok", dict(x=T(2, 6, 6, 16), w=T(64, 3, 3, 16), stride=1, pad=1)))
_add("rule_in_affine_ok_fuse_off", ("in_affine_ok", dict(x=T(2, 8, 8, 16), w=T(64, 3, 3, 16), stride=1, pad=1, _gn_fuse=False)))
_add("rule_in_affine_ok_k3", ("in_affine_ok", dict(x=T(2, 8, 8, 64), w=T(3, 3, 3, 64), stride=1, pad=1)))
_add("rule_in_affine_ok_k3_r1", ("in_affine_ok", dict(x=T(2, 8, 8, 64), w=T(3, 1, 1, 64), stride=1, pad=0)))
_add("rule_in_affine_ok_k3_c32", ("in_affine_ok", dict(x=T(2, 8, 8, 32), w=T(3, 3, 3, 32), stride=1, pad=1)))
_add("rule_in_affine_ok_bf16_x", ("in_affine_ok", dict(x=B(2, 8, 8, 16), w=T(64, 3, 3, 16), stride=1, pad=1)))
_add("rule_blocks_6x6", ("wgrad_blocks_eligible", dict(gy_shape=(4, 6, 6, 64), x_shape=(4, 6, 6, 64), R=5, S=5, stride=1)))
_add("rule_blocks_c32", ("wgrad_blocks_eligible", dict(gy_shape=GY, x_shape=(4, 8, 8, 32), R=5, S=5, stride=1)))
_add("rule_blocks_s1x1", ("wgrad_blocks_eligible", dict(gy_shape=GY, x_shape=X, R=1, S=1, stride=1)))
_add("rule_dense_group_big", ("dense_wgrad_group", dict(N=512, K=128, Cc=128, R=5, S=5, PQ=4096, stride=1, out_hw=(64, 64))))
_add("rule_dense_group_no_hw", ("dense_wgrad_group", dict(N=64, K=128, Cc=64, R=5, S=5, PQ=64)))
_add("rule_dense_group_k3", ("dense_wgrad_group", dict(N=64, K=64, Cc=3, R=5, S=5, PQ=1024, stride=2, out_hw=(32, 32))))
_add("rule_dense_group_6x6", ("dense_wgrad_group", dict(N=256, K=64, Cc=64, R=3, S=3, PQ=36, stride=1, out_hw=(6, 6))))
_add("rule_gram_eligible", ("gram_norms_eligible", dict(gy_shape=(4, 8, 8, 64), x_shape=(4, 8, 8, 32))))
_add("rule_gram_eligible_k48", ("gram_norms_eligible", dict(gy_shape=(4, 8, 8, 48), x_shape=(4, 8, 8, 32))))
_add("rule_gram_eligible_100px", ("gram_norms_eligible", dict(gy_shape=(4, 10, 10, 64), x_shape=(4, 10, 10, 32))))
_add("rule_gram_preferred_linear", ("gram_norms_preferred", dict(gy_shape=(4, 1, 1, 1), x_shape=(4, 1, 1, 100), stride=1)))
_add("rule_gram_preferred_64px", ("gram_norms_preferred", dict(gy_shape=(4, 8, 8, 64), x_shape=(4, 16, 16, 32), stride=2)))
_add("rule_gram_preferred_72px", ("gram_norms_preferred", dict(gy_shape=(4, 8, 8, 64), x_shape=(4, 17, 16, 32), stride=2)))
_add("rule_gram_preferred_k32", ("gram_norms_preferred", dict(gy_shape=(4, 8, 8, 32), x_shape=(4, 8, 8, 32), stride=1)))


# ---- harness --------------------------------------------------------------------------------------------------------------------------

class Patches:
    """setattr with an undo list (the script's stand-in for pytest's monkeypatch.setattr)."""

    def __init__(self):
        self.saved = []

    def setattr(self, obj, name, value):
        self.saved.append((obj, name, obj.__dict__.get(name, self), getattr(obj, name)))
        setattr(obj, name, value)

    def undo(self):
        for obj, name, own, old in reversed(self.saved):
            if own is self:             # the attribute came from a base class: drop the override
                delattr(obj, name)
            else:
                setattr(obj, name, old)
        self.saved = []


class Harness:
    """The recording stand-ins, installed through `setattr(obj, name, value)` (monkeypatch.setattr in the test)."""

    def __init__(self, setattr_fn, root=ROOT, timer=True):
        if root not in sys.path:
            sys.path.insert(0, root)
        import torch
        from csl_gan_amd import _lib, ops
        self.torch, self.ops, self.setattr = torch, ops, setattr_fn
        self.calls, self.repack, self.timed, self.spans, self.keep = [], [], [], [], []
        setattr_fn(_lib, "lib", lambda: self)
        setattr_fn(ops, "_stream", lambda: None)
        setattr_fn(torch.Tensor, "is_cuda", property(lambda t: True))
        orig_get = ops.repack_cache.get

        def get(kind, w, numel, wkey=None, version=None):
            self.repack.append([kind, numel, wkey is not None, version is not None])
            ws, fresh = orig_get(kind, w, numel, None, version=version)
            self.keep.append(ws)
            self.spans.append((ws.data_ptr(), ws.data_ptr() + ws.numel() * ws.element_size(), "ws"))
            return ws, fresh

        setattr_fn(ops.repack_cache, "get", get)
        setattr_fn(ops, "_timer", self if timer else None)

    # -- the library
    def __getattr__(self, name):
        if not name.startswith("cslgan_"):
            raise AttributeError(name)
        if name == "cslgan_last_kernel":
            return lambda: b"recorded_kernel"

        def entry(*args):
            self.calls.append({"entry": name, "args": [self._arg(a) for a in args]})
            return 0
        return entry

    def _where(self, addr):
        if not addr:
            return "null"
        for lo, hi, name in self.spans:
            if lo <= addr < hi:
                return name if addr == lo else "%s+%d" % (name, addr - lo)
        return "new"

    # struct -> {prefix of an array field's name: the field that counts its entries} (anything else: n_seg)
    _ARRAY_LEN = {"AdaptiveClipT": {"sq": "n_layers", "mat": "n_mat", "job": "n_jobs"}}

    def _arg(self, a):
        if a is None or isinstance(a, C.c_void_p):
            return self._where(a.value if a is not None else 0)
        if isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, C.Array):
            return [self._where(v) if a._type_ is C.c_void_p else v for v in a]
        obj = a._obj                                # byref(...)
        out = {"struct": type(obj).__name__}
        for field, ctype in obj._fields_:
            v = getattr(obj, field)
            if field.startswith("_"):
                continue
            if ctype is C.c_void_p:
                out[field] = "set" if v else "null"
            elif isinstance(v, C.Array):            # the entries in use: SegsT's first n_seg, AdaptiveClipT's by the field's own count
                n = getattr(obj, self._ARRAY_LEN.get(type(obj).__name__, {}).get(field.split("_")[0], "n_seg"))
                out[field] = [self._where(e) if ctype._type_ is C.c_void_p else e for e in list(v)[:n]]
            else:
                out[field] = v
        return out

    # -- the launch timer
    only = None

    def begin(self):
        return None

    def end(self, name, flop, nbytes, start, exec_flop=None, tag=None, kernel=None):
        self.timed.append([name, flop, nbytes, exec_flop, tag, kernel])

    # -- cases
    def tensor(self, spec, name):
        torch = self.torch
        _, shape, dt = spec
        t = torch.zeros(shape, dtype={"f32": torch.float32, "f32t": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[dt])
        if dt == "f32t":
            t = t.transpose(-1, -2)
        self.spans.append((t.data_ptr(), t.data_ptr() + max(1, t.numel()) * t.element_size(), name))
        return t

    def build(self, v, name):
        if isinstance(v, tuple) and v and v[0] == "T":
            return self.tensor(v, name)
        if isinstance(v, (tuple, list)) and any(isinstance(e, (tuple, list)) for e in v):
            return type(v)(self.build(e, "%s.%d" % (name, i)) for i, e in enumerate(v))
        if v in ("bf16", "f32") and name == "out_dtype":
            return self.torch.bfloat16 if v == "bf16" else self.torch.float32
        return v

    def prepare(self, case):
        """(function, settings, arguments) of a case with its tensors made and their address ranges noted."""
        self.spans, self.keep = [], []
        fn, spec = case
        args = {k: self.build(v, k) for k, v in spec.items() if not k.startswith("_")}
        return getattr(self.ops, fn), {k: v for k, v in spec.items() if k.startswith("_")}, args

    def call(self, fn, settings, args):
        """Run one prepared case under its settings; returns (result or None, exception or None, gn_partials cell or None)."""
        ops = self.ops
        self.setattr(ops, "_X3_SPLIT", settings.get("_split", 0))
        self.setattr(ops, "_GN_FUSE", settings.get("_gn_fuse", True))
        prev_halo = ops.set_f32_halo(settings.get("_halo", True))
        ops.set_compute_dtype(settings.get("_mode", "fp32"))
        cell = ops.gn_partials(settings["_gn"]) if "_gn" in settings else None
        try:
            if cell is not None:
                cell.__enter__()
            try:
                return fn(**args), None, cell
            except RuntimeError as e:
                return None, e, cell
            finally:
                if cell is not None:
                    cell.pending = ops.gn_partials._req is not None
                    cell.__exit__()
        finally:
            ops.set_compute_dtype("fp32")
            ops.set_f32_halo(prev_halo)

    def describe(self, r, out):
        if isinstance(r, self.torch.Tensor):
            return {"shape": list(r.shape), "dtype": str(r.dtype), "is_out": r is out, "at": self._where(r.data_ptr()),
                    "contiguous": r.is_contiguous()}
        return r

    def log(self, name):
        """The full log of one case."""
        self.calls, self.repack, self.timed = [], [], []
        fn, settings, args = self.prepare(CASES[name])
        r, err, cell = self.call(fn, settings, args)
        log = {"calls": self.calls, "repack": self.repack, "timed": self.timed, "result": self.describe(r, args.get("out")),
               "error": type(err).__name__ if err is not None else None}
        if cell is not None:
            log["gn_part"] = None if cell.part is None else [self.describe(cell.part[0], None), cell.part[1]]
            log["gn_pending"] = cell.pending
        return log


def digest(log):
    return hashlib.sha1(json.dumps(log, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def entries(log):
    return [c["entry"] for c in log["calls"]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=ROOT, help="checkout whose csl_gan_amd is driven (default: this one)")
    ap.add_argument("--case", help="print the full log of this case")
    ap.add_argument("--record", metavar="JSON", help="write {case: {entries, sha1}} to this file")
    ap.add_argument("--time", action="store_true", help="host seconds for the whole case list, no timer installed")
    ap.add_argument("--passes", type=int, default=20, help="--time: passes over the list (per case the fastest counts)")
    a = ap.parse_args()
    p = Patches()
    h = Harness(p.setattr, root=os.path.abspath(a.root), timer=not a.time)
    try:
        if a.time:
            h.log(next(iter(CASES)))              # imports and first-call costs stay off the clock
            best = dict.fromkeys(CASES, float("inf"))     # per case the fastest of the passes: scheduling noise only ever adds time
            for _ in range(a.passes):
                for name in CASES:
                    prepared = h.prepare(CASES[name])
                    h.calls, h.repack = [], []
                    t0 = time.perf_counter()
                    h.call(*prepared)
                    best[name] = min(best[name], time.perf_counter() - t0)
            print("%.2f ms for %d cases, each the fastest of %d passes (%s)" % (1e3 * sum(best.values()), len(CASES), a.passes, h.ops.__file__))
            return
        if a.case:
            print(json.dumps(h.log(a.case), indent=1, sort_keys=True))
            return
        fixture, reached = {}, set()
        for name in CASES:
            log = h.log(name)
            fixture[name] = {"entries": entries(log), "sha1": digest(log)}
            reached.update(e for e in entries(log) if is_conv_entry(e))
            print("%-36s %s %s" % (name, log["error"] or "", " ".join(e[len("cslgan_"):] for e in entries(log))))
        print("%d cases, %d of %d conv entries reached%s" % (len(CASES), len(reached), len(CONV_ENTRIES),
                                                             "" if sorted(reached) == CONV_ENTRIES else " — MISSING / EXTRA: %s" % sorted(reached ^ set(CONV_ENTRIES))))
        if a.record:
            with open(a.record, "w") as f:
                json.dump(fixture, f, indent=0, sort_keys=True)
                f.write("\n")
    finally:
        p.undo()


if __name__ == "__main__":
    main()
