"""Which device kernel does each dispatch decision of csl_gan_amd.ops / libcslgan_hip.so pick?

One small launch per case, on either side of every tile-count threshold and every shape rule of the conv dispatch; after the call the
name cslgan_last_kernel() reports is the case's route.  tests/kernel_routes.json holds the names recorded with this script and
tests/test_kernel_routes_gpu.py asserts them, so a refactor of the dispatch layer cannot move a launch to another kernel unnoticed.

    python scripts/kernel_routes.py                 # name per case
    python scripts/kernel_routes.py --checksum      # ... and a hash of the output bytes (cases that accumulate with float atomics
                                                    #     differ between two runs of the same build: compare those by name only)
    python scripts/kernel_routes.py --checksum --epilogue   # the same launches with a bias and an activation (forward) or a mask
                                                    #     (data gradient), so the hashes cover every routed kernel's epilogue
    python scripts/kernel_routes.py --record tests/kernel_routes.json

Only public entry points are used (ops.conv2d_fwd / conv2d_dgrad / conv2d_wgrad_grouped / conv2d_wgrad_sqnorm_gram, ops.compute_dtype,
ops.storage_dtype, ops.set_f32_halo), so the script runs unchanged on older commits.  (The normalisation launches note no kernel name
and their statistics are summed with LDS atomics, so neither a name nor a checksum pins them; tests/test_kernels_gpu.py does.)
"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _c(op, mode="fp32", bf16s=False, f32_halo=True, **shape):
    return dict(op=op, mode=mode, bf16s=bf16s, f32_halo=f32_halo, **shape)


def _fwd(N, H, W, C, K, R, stride=1, pad=None, **kw):
    return _c("fwd", N=N, H=H, W=W, C=C, K=K, R=R, stride=stride, pad=R // 2 if pad is None else pad, **kw)


def _dgrad(N, H, W, C, K, R, stride=1, pad=None, **kw):
    return _c("dgrad", N=N, H=H, W=W, C=C, K=K, R=R, stride=stride, pad=R // 2 if pad is None else pad, **kw)


def _wgrad(N, H, W, C, K, R, stride=1, pad=None, group=1, **kw):
    return _c("wgrad", N=N, H=H, W=W, C=C, K=K, R=R, stride=stride, pad=R // 2 if pad is None else pad, group=group, **kw)


def _gram(N, H, W, C, K, R, stride=1, pad=None, **kw):
    return _c("gram", N=N, H=H, W=W, C=C, K=K, R=R, stride=stride, pad=R // 2 if pad is None else pad, **kw)


# name -> case.  "<threshold>_at" sits exactly on a tile / row threshold, "<threshold>_below" one tile or row block under it.
CASES = {
    # ---- gather kernel (igemm_kc), one class: 1x1 convs with 16 input channels run on no other kernel ----------------------------------
    "kc_t128_at": _fwd(300, 8, 16, 16, 128, 1),              # 300 tiles of 128x128
    "kc_t128_below": _fwd(299, 8, 16, 16, 128, 1),
    "kc_t64_at": _fwd(192, 8, 8, 16, 128, 1),                # 192 tiles of 64x128
    "kc_t64_below": _fwd(191, 8, 8, 16, 128, 1),
    # ---- gather kernel, four classes: 3x3 stride-2 data gradient (its one-tap class keeps it off the halo kernels) --------------------
    "kc_tmc_at": _dgrad(130, 16, 16, 128, 16, 3, stride=2),      # 4 x 130 = 520 tiles of 64x128
    "kc_tmc_below": _dgrad(129, 16, 16, 128, 16, 3, stride=2),
    # ---- stride-2 forward conv on the fp32 halo kernel (parity classes): 512 tiles of 128x128 ----------------------------------------
    "s2_halo_at": _fwd(256, 32, 32, 32, 64, 5, stride=2, f32_halo=False),
    "s2_halo_below": _fwd(255, 32, 32, 32, 64, 5, stride=2, f32_halo=False),
    "s2_halo_wide_at": _fwd(256, 32, 32, 32, 128, 5, stride=2, f32_halo=False),      # 128 filters: the 128-wide form (>= 256 tiles always holds here)
    "s2_halo_wide_below": _fwd(255, 32, 32, 32, 128, 5, stride=2, f32_halo=False),
    # ---- 4x4 grids on the x3 halo kernel in a bf16 mode: 2048 rows (a row block = four images) ----------------------------------------
    "x3_quad_at": _fwd(128, 8, 8, 16, 64, 5, stride=2, mode="bf16x3"),
    "x3_quad_below": _fwd(124, 8, 8, 16, 64, 5, stride=2, mode="bf16x3"),
    "x3_quad_bf16_at": _fwd(128, 8, 8, 16, 64, 5, stride=2, mode="bf16"),
    "x3_quad_bf16_below": _fwd(124, 8, 8, 16, 64, 5, stride=2, mode="bf16"),
    "x3_quad_dgrad_at": _dgrad(128, 8, 8, 64, 16, 5, stride=2, mode="bf16x3"),
    "x3_quad_dgrad_below": _dgrad(124, 8, 8, 64, 16, 5, stride=2, mode="bf16x3"),
    # ---- 4x4 grids on the fp32 halo kernel: 4096 rows -------------------------------------------------------------------------------------
    "halo_quad_at": _dgrad(256, 8, 8, 64, 32, 5, stride=2),
    "halo_quad_below": _dgrad(252, 8, 8, 64, 32, 5, stride=2),
    # ---- heaviest-with-lightest class pairing: 256 paired workgroups -------------------------------------------------------------------
    "halo_pair_at": _dgrad(256, 16, 16, 64, 32, 5, stride=2, f32_halo=False),
    "halo_pair_below": _dgrad(254, 16, 16, 64, 32, 5, stride=2, f32_halo=False),
    "x3_pair_at": _dgrad(256, 16, 16, 64, 32, 5, stride=2),              # (the x3 kernel's name does not show the pairing: same name both sides)
    "x3_pair_below": _dgrad(254, 16, 16, 64, 32, 5, stride=2),
    "x3_pair_x3_at": _dgrad(256, 16, 16, 64, 32, 5, stride=2, mode="bf16x3"),
    "x3_pair_x3_below": _dgrad(254, 16, 16, 64, 32, 5, stride=2, mode="bf16x3"),
    # ---- x3 halo kernel, 128-wide tiles from 192 tiles on ---------------------------------------------------------------------------------
    "x3_wide_at": _fwd(384, 8, 8, 16, 128, 3),
    "x3_wide_below": _fwd(382, 8, 8, 16, 128, 3),
    "x3_wide_x3_at": _fwd(384, 8, 8, 16, 128, 3, mode="bf16x3"),
    "x3_wide_x3_below": _fwd(382, 8, 8, 16, 128, 3, mode="bf16x3"),
    # ---- weight gradient on igemm_mc, 64 output channels: 64x256 tiles when Ndim >= 1024 and groups x n-tiles >= 256 -------------------
    "mc_wide64_at": _wgrad(64, 5, 5, 256, 64, 2, pad=0),                 # Ndim 1024, 64 x 4 = 256
    "mc_wide64_below": _wgrad(63, 5, 5, 256, 64, 2, pad=0),              # 63 x 4 = 252
    "mc_wide64_ndim_below": _wgrad(64, 5, 5, 252, 64, 2, pad=0),         # Ndim 1008, 64 x 4 = 256
    "mc_k128": _wgrad(8, 5, 5, 64, 128, 2, pad=0),
    # ---- shape rules that used to sit behind boolean switches: the default route and an ineligible neighbour ----------------------------
    "c3_fwd": _fwd(4, 32, 32, 3, 64, 5, stride=2),
    "c3_fwd_padded_rgb": _fwd(4, 24, 24, 3, 64, 5, stride=2),
    "c3_wgrad": _wgrad(4, 32, 32, 3, 64, 5, stride=2),
    "c3_wgrad_padded_rgb": _wgrad(4, 24, 24, 3, 64, 5, stride=2),
    "conv1x1_c32": _fwd(16, 64, 64, 32, 64, 1),
    "conv1x1_c48": _fwd(16, 64, 64, 48, 64, 1),
    "conv1x1s_c32": _fwd(16, 64, 64, 32, 64, 1, bf16s=True),
    "conv1x1s_c48": _fwd(16, 64, 64, 48, 64, 1, bf16s=True),
    "linear_k1_fwd": _fwd(8, 1, 1, 256, 1, 1),
    "linear_k1_fwd_c128": _fwd(8, 1, 1, 128, 1, 1),
    "linear_k1_dgrad": _dgrad(8, 1, 1, 256, 1, 1),
    "linear_k1_dgrad_c128": _dgrad(8, 1, 1, 128, 1, 1),
    "skinny_k3": _fwd(4, 16, 16, 64, 3, 3),
    "skinny_k3_c32": _fwd(4, 16, 16, 32, 3, 3),
    "skinny_all_dgrad_s2": _dgrad(4, 16, 16, 3, 64, 5, stride=2),
    "skinny_dgrad_s1": _dgrad(4, 16, 16, 3, 64, 3),
    "f32_halo_fwd": _fwd(8, 16, 16, 16, 64, 3),
    "f32_halo_fwd_off": _fwd(8, 16, 16, 32, 64, 3, f32_halo=False),
    "f32_halo_fwd_off_c16": _fwd(8, 16, 16, 16, 64, 3, f32_halo=False),
    "f32_halo_fwd_6x6": _fwd(8, 6, 6, 16, 64, 3),
    "x3_halo_fwd": _fwd(8, 16, 16, 16, 64, 3, mode="bf16x3"),
    "x3_halo_fwd_6x6": _fwd(8, 6, 6, 16, 64, 3, mode="bf16x3"),
    "bf16_halo_fwd": _fwd(8, 16, 16, 16, 64, 3, mode="bf16"),
    "bf16_halo_fwd_6x6": _fwd(8, 6, 6, 16, 64, 3, mode="bf16"),
    "x3_s2_fwd": _fwd(8, 32, 32, 16, 64, 5, stride=2, mode="bf16x3"),
    "x3_s2_fwd_r4": _fwd(8, 32, 32, 16, 64, 4, stride=2, pad=1, mode="bf16x3"),
    "x3_dgrad_s1": _dgrad(8, 16, 16, 64, 16, 3, mode="bf16x3"),
    "x3_dgrad_s1_c32": _dgrad(8, 16, 16, 32, 16, 3, mode="bf16x3"),
    "wgh_s5": _wgrad(8, 8, 8, 64, 64, 5),
    "wgh_s5_6x6": _wgrad(8, 6, 6, 64, 64, 5),
    "x3w_s5": _wgrad(8, 8, 8, 64, 64, 5, mode="bf16x3"),
    "x3w_s3": _wgrad(8, 8, 8, 64, 64, 3, mode="bf16x3"),
    "x3w_quad": _wgrad(8, 8, 8, 64, 64, 5, stride=2, group=2, mode="bf16x3"),
    "x3w_quad_group1": _wgrad(8, 8, 8, 64, 64, 5, stride=2, group=1, mode="bf16x3"),
    "gram_small": _gram(8, 4, 4, 64, 64, 3),
    "gram_cls64": _gram(8, 8, 8, 32, 32, 3),
    "gram_100_pixels": _gram(8, 10, 10, 32, 32, 3, pad=0),
    "halos_fwd": _fwd(4, 16, 16, 16, 64, 3, bf16s=True),
    "halos_fwd_8x8": _fwd(4, 8, 8, 16, 64, 3, bf16s=True),
    "kcs_dgrad_s2": _dgrad(4, 32, 32, 64, 64, 5, stride=2, bf16s=True),
    "kcs_dgrad_s1": _dgrad(4, 16, 16, 64, 64, 3, bf16s=True),
    "mcs_wgrad": _wgrad(8, 8, 8, 64, 64, 3, bf16s=True),
    # ---- bf16-stored gather kernel above 64 filters: 128x128 tiles from 256 row blocks x column tiles on (48 channels: not the 1x1 stream) --
    "kcs_t128_at": _fwd(256, 8, 16, 48, 128, 1, bf16s=True),             # 32768 rows = 256 row blocks of 128, one column tile
    "kcs_t128_below": _fwd(255, 8, 16, 48, 128, 1, bf16s=True),
    # ---- the critic's head on bf16 features (fp32 loss cotangent) and the clip-weighted weight gradient ------------------------------
    "linear_k1s_fwd": _fwd(8, 1, 1, 256, 1, 1, bf16s=True),
    "linear_k1s_dgrad": _dgrad(8, 1, 1, 256, 1, 1, bf16s=True, gy_f32=True),
    "linear_k1s_wgrad": _wgrad(8, 1, 1, 256, 1, 1, group=2, bf16s=True, gy_f32=True),
    "mcs_wgrad_scaled": _wgrad(8, 8, 8, 64, 64, 3, group=2, bf16s=True, row_scale=True),     # 8x8 output: a 64-pixel K tile per sample
}


def run_case(case, seed=0, epilogue=False, act=None):
    """Launch one case; returns (kernel name, output tensor).

    epilogue: forward cases also pass a random bias and the activation `act` (main() passes 1 + case index % 3, so the three
    activations alternate over the cases; default 1 + seed % 3); data-gradient cases pass a random mask.  No residual: it changes routes (and an
    activation keeps K from being split, so those launches hash reproducibly).
    Optional case keys: gy_f32 (the output gradient stays fp32 in a bf16s case: the head's loss cotangent; a data gradient then asks
    for a bf16 result), row_scale (a weight gradient gets random [N] fp32 per-sample weights)."""
    import torch
    from csl_gan_amd import _lib, ops

    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        t = torch.randn(*shape, generator=g).cuda()
        return ops.cast_bf16(t) if case["bf16s"] else t

    def rnd_gy(*shape):
        return torch.randn(*shape, generator=g).cuda() if case.get("gy_f32") else rnd(*shape)

    op = case["op"]
    N, H, W, Cc = case["N"], case["H"], case["W"], case["C"]
    prev = ops.set_f32_halo(case["f32_halo"])
    try:
        with ops.compute_dtype(case["mode"]), ops.storage_dtype("bf16" if case["bf16s"] else "fp32"):
            K, R, stride, pad = case["K"], case["R"], case["stride"], case["pad"]
            P, Q = ops.conv_out_size(H, R, stride, pad), ops.conv_out_size(W, R, stride, pad)
            w = torch.randn(K, R, R, Cc, generator=g).cuda() * 0.1
            if op == "fwd":
                extra = dict(bias=torch.randn(K, generator=g).cuda(), act=1 + seed % 3 if act is None else act) if epilogue else {}
                out = ops.conv2d_fwd(rnd(N, H, W, Cc), w, stride=stride, pad=pad, **extra)
            elif op == "dgrad":
                extra = dict(mask=rnd(N, H, W, Cc)) if epilogue else {}
                if case.get("gy_f32"):
                    extra["out_dtype"] = torch.bfloat16
                out = ops.conv2d_dgrad(rnd_gy(N, P, Q, K), w, (H, W), stride=stride, pad=pad, **extra)
            elif op == "wgrad":
                extra = dict(row_scale=torch.rand(N, generator=g).cuda()) if case.get("row_scale") else {}
                out = ops.conv2d_wgrad_grouped(rnd_gy(N, P, Q, K), rnd(N, H, W, Cc), R, R, stride=stride, pad=pad, group=case["group"], **extra)
            elif op == "gram":
                out = ops.conv2d_wgrad_sqnorm_gram(rnd(N, P, Q, K), rnd(N, H, W, Cc), R, R, stride=stride, pad=pad)
            else:
                raise ValueError(op)
            name = _lib.lib().cslgan_last_kernel().decode()
    finally:
        ops.set_f32_halo(prev)
    torch.cuda.synchronize()
    return name, out


def checksum(t):
    import torch
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha1(raw.cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checksum", action="store_true", help="also print a hash of each case's output bytes")
    ap.add_argument("--epilogue", action="store_true", help="forward cases with a bias and an activation, data-gradient cases with a mask")
    ap.add_argument("--record", metavar="JSON", help="write {case: kernel name} to this file")
    a = ap.parse_args()
    names = {}
    for i, (key, case) in enumerate(CASES.items()):
        name, out = run_case(case, seed=i, epilogue=a.epilogue, act=1 + i % 3)
        names[key] = name
        print("%-24s %-44s %s" % (key, name, checksum(out) if a.checksum else ""), flush=True)
    if a.record:
        with open(a.record, "w") as f:
            json.dump(names, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
