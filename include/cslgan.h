/*
 * cslgan.h — C-ABI of libcslgan_hip.so: the MI355X (gfx950) kernels behind the csl-gan
 * DP discriminator step.
 *
 * The reference (twosixlabs/csl-gan) is pure Python and has no FFI layer: the boundary a
 * maintainer binds is the set of PyTorch / Opacus-fork calls its D-step makes.  Every entry
 * point below names the reference call (file:line under /root/reference) whose device work
 * it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C types only: device pointers are void* / float*, sizes are int / int64_t,
 *     the stream is the raw hipStream_t handle passed as void* (0 = default stream);
 *   - every function returns 0 on success or a negative cslgan_status; the message of the
 *     last failure on the calling thread is returned by cslgan_last_error();
 *   - all work is enqueued asynchronously on the given stream; the library never allocates,
 *     frees or synchronises (graph-capturable).  Workspaces are caller-owned;
 *   - activations are NHWC fp32 ("channels last"): x[n][h][w][c]; conv weights are
 *     KRSC: w[cout][kh][kw][cin] (the memory of a torch channels_last [cout,cin,kh,kw] tensor).
 */
#ifndef CSLGAN_H
#define CSLGAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSLGAN_ABI_VERSION 7

typedef enum {
    CSLGAN_OK = 0,
    CSLGAN_ERR_INVALID_ARG = -1,   /* bad shape / null pointer / unsupported configuration */
    CSLGAN_ERR_LAUNCH = -2,        /* hipLaunchKernel / hipMemsetAsync reported an error */
    CSLGAN_ERR_NO_DEVICE = -3      /* no gfx950 device visible */
} cslgan_status;

/* activation / epilogue codes for cslgan_conv2d_* */
enum { CSLGAN_ACT_NONE = 0, CSLGAN_ACT_LRELU02 = 1, CSLGAN_ACT_RELU = 2, CSLGAN_ACT_TANH = 3 };

#define CSLGAN_MAX_SEGS 16
#define CSLGAN_MAX_ROLES 8      /* row blocks of one fused critic pass (adaptive / generated / private / penalty rows) */

/* A batch of row-major [n_rows, len[i]] matrices (one per parameter tensor): the materialised
 * per-sample gradients p.grad_sample viewed as [passes*B, numel(p)]  (train.py:233,311-315). */
typedef struct {
    int32_t n_seg;
    int32_t _pad;
    const float* in[CSLGAN_MAX_SEGS];      /* device, [n_rows, len] with row stride row_stride */
    float* out[CSLGAN_MAX_SEGS];           /* device, [len]            (clip_accum only)       */
    const float* noise[CSLGAN_MAX_SEGS];   /* device, [len] pre-drawn N(0,1) or NULL -> Philox  */
    int64_t len[CSLGAN_MAX_SEGS];
    int64_t row_stride[CSLGAN_MAX_SEGS];   /* in elements */
    int64_t rows[CSLGAN_MAX_SEGS];         /* clip_accum only: > 0 = this segment has its OWN row count (column sums of slab sets of
                                            * different heights in one launch; needs factors == NULL), 0 = the call's n_rows */
    const uint64_t* call_counter;          /* device, nullable (clip_accum only): the Philox offset used is
                                            * offset + 64 * *call_counter — a step captured in a HIP graph passes its
                                            * noise-call counter here instead of by value, so every replay draws new noise */
} cslgan_segs_t;

int cslgan_version(void);
const char* cslgan_last_error(void);
/* Name of the device kernel most recently launched by the calling thread through a conv / clip / norm entry, as rocprofv3
 * --kernel-trace lists it (e.g. "igemm_halo_kernel<128,false>"); "" before the first launch.  Measurement aid: bench.py
 * tags its per-launch HIP-event timings with it. */
const char* cslgan_last_kernel(void);
/* number of visible HIP devices (>=0) or a negative status */
int cslgan_device_count(void);

/* ---- per-sample norm / clip / noise  (the fused DP kernel family) ------------------------ */

/* out_sq[s * n_rows + r] = sum_j in[s][r][j]^2.  Replaces
 * opacus.utils.tensor_utils.calc_sample_norms (train.py:311-314) and the norm half of
 * privacy_engine.clip() (train.py:399).  out_sq is overwritten (zeroed on-stream first). */
int cslgan_sample_sqnorm_f32(const cslgan_segs_t* segs, int64_t n_rows, float* out_sq, void* stream);

/* bfloat16 storage of the materialised per-sample gradients (fp32 accumulate): segs->in[] point to bf16
 * elements, everything else as the _f32 form.  Halves the HBM bytes of the norm / clip passes
 * (17.3 MB/img/clipped pass for D64); BASELINE.json config 5. */
int cslgan_sample_sqnorm_bf16(const cslgan_segs_t* segs, int64_t n_rows, float* out_sq, void* stream);

/* Clip factors from squared norms:  f = min(1, C / (sqrt(sq) + eps)).
 *   flat != 0 : one factor per row from the all-segment norm; max_norm[0] is C; out_f is [n_rows]
 *   flat == 0 : per segment; max_norm[s] is C_s; out_f is [n_seg, n_rows]
 * rows < first_private_row get factor 1 (split mode: the generated-data pass is not clipped,
 * train.py:112-113).  out_norm (nullable) receives the norms ([1 or n_seg, n_rows]).
 * Replaces norm_clipper.calc_clipping_factors (train.py:324). max_norm is a DEVICE pointer. */
int cslgan_clip_factors_f32(const float* sq, int n_seg, int64_t n_rows, const float* max_norm, int flat,
                            float eps, int64_t first_private_row, float* out_f, float* out_norm, void* stream);

/* out[s][j] = beta*out[s][j] + scale * ( sum_r f(s,r) * in[s][r][j] + noise_std[s] * z[s][j] )
 *   factors: device [n_rows] (factors_per_seg==0) or [n_seg,n_rows] (factors_per_seg!=0), NULL -> 1
 *   noise_std: DEVICE [n_seg] or NULL (no noise); z from segs->noise[s] when given, else
 *   Philox4x32-10 + Box-Muller keyed by (seed, offset, s, j):
 *
 * Device random streams (restated on the host by oracle/noise_streams.py; tests/test_noise_streams*.py hold both to it).
 *   Philox4x32-10 as in Random123 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1), four 32-bit words out.
 *   Box-Muller on a word pair (a, b): u1 = (a >> 8) 2^-24 + 2^-25, u2 = (b >> 8) 2^-24, r = sqrt(-2 ln u1),
 *   (r cos 2 pi u2, r sin 2 pi u2), in fp32 with the fast log / sincos.  u1 lies on a 2^-24 grid inside (0, 1), so
 *   |z| <= sqrt(-2 ln 2^-25) = 5.89; the fp32 sum rounds u1 to even above 1/2 (at most 2.5e-4 on z, reached where u1 -> 1).
 *   Column j of segment s:  q = j >> 2;  off64 = offset + 64 * *call_counter (mod 2^64);
 *       counter = (q lo, q hi, (s + (off64 << 8)) mod 2^32, off64 >> 24),  key = (seed lo, seed hi);
 *       words 0, 1 -> columns 4q, 4q+1; words 2, 3 -> columns 4q+2, 4q+3.
 *   Every (off64, s, q) has a counter of its own for s < 256 (a launch has s < 16), off64 < 2^56, len < 2^34 (above, q hi != 0
 *   still separates).  The CALLER keeps off64 unique per launch: csl_gan_amd.ops.clip_accum_noise passes
 *   offset = 64 * (its own offset argument) + first_index, first_index = the position in its tensor list of the launch's first
 *   tensor, so one call may hold at most 64 tensors (it refuses more: position 64 would be position 0 of the next call); the
 *   engines pass offset 0 and count their steps in *call_counter, which their checkpoints carry.
 *   The mean sampler (cslgan_mean_sample_f32 below) draws from the same generator with counters that can coincide with
 *   these: the two are kept apart by their SEEDS alone (engine: manual_seed + 7919 * rank; sampler: the process seed xor
 *   0x6D65616E73616D70), as are ranks.
 *   The indexed latent stream (cslgan_latent_normal_f32 below; ABI v7), sample g = first_index + *first_index_dev + i of row i:
 *       key = the two halves of (seed xor 0x6C6174656E747A73),  counter = (q, g lo, g hi, 0x7A6C6174) -> columns 4q .. 4q+3 of row i
 *   (words 0, 1 -> 4q, 4q+1; words 2, 3 -> 4q+2, 4q+3; a row's last counter is partly used when dim % 4 != 0).  It is kept apart from
 *   the two streams above by its seed tag; inside it every (g, q) has a counter of its own for dim < 2^34.
 * Replaces privacy_engine.clip() + accum_grads_across_passes() (train.py:399-402) and, with
 * noise/scale, the engine-wrapped d_optimizer.step() noise + 1/B (train.py:484). */
int cslgan_clip_accum_noise_f32(const cslgan_segs_t* segs, int64_t n_rows, const float* factors,
                                int factors_per_seg, const float* noise_std, uint64_t seed, uint64_t offset,
                                float scale, float beta, void* stream);

int cslgan_clip_accum_noise_bf16(const cslgan_segs_t* segs, int64_t n_rows, const float* factors,
                                 int factors_per_seg, const float* noise_std, uint64_t seed, uint64_t offset,
                                 float scale, float beta, void* stream);

/* backprop_clip.py:18-22 l2_clip: rows with ||t_r|| > C are scaled to norm C (no epsilon).
 * in/out may alias.  norms_ws: caller workspace [n_rows] floats. */
int cslgan_l2_clip_rows_f32(const float* in, float* out, int64_t n_rows, int64_t len, float C,
                            float* norms_ws, void* stream);

/* MeanSampler.sample (mean_sampler.py:75-84; called from train.py:200-202, 214-216) on device-resident mean samples:
 *   out[i][:] = mean_samples[labels[i]][perms[i]][:] + noise_mean_std * z_i + noise_std * z_{i,:}
 * mean_samples [n_classes][num_samples][len], labels (nullable when n_classes == 1) and perms [n] int64, out [n][len];
 * z ~ N(0,1) from Philox4x32-10 keyed (seed, offset): the caller advances offset per call (MeanSampler: 1, 2, ... per draw,
 * checkpointed).  Key = (seed lo, seed hi) and, with off lo / off hi the 32-bit halves of offset, the counters of image i are
 *     permutation keys  (j, i / num_samples, off lo, 0x7065726D ^ off hi)   word 0 for j < num_samples; the image takes the j whose
 *                                                                           key has rank i mod num_samples (equal keys: lower j first)
 *     label             (i, 0x6C61626C, off lo, off hi)                      (word 0 * n_classes) >> 32
 *     jitter z_i        (i, 0xFFFFFFFF, off lo, off hi)                      first Box-Muller output of words 0, 1
 *     pixels 4q .. 4q+3 (q, i, off lo, off hi)                               Box-Muller of words 0, 1 and of words 2, 3
 * (Box-Muller as under cslgan_clip_accum_noise_f32 "Device random streams").  No two of them coincide for n <= 65535 (below
 * both tags), offset < 2^60 (then 0x7065726D ^ off hi >= 2^28 is no off hi in use) and len < 2^34.
 * perms == NULL (num_samples <= 1024): the kernel draws them — image i takes entry i mod num_samples of the (i / num_samples)-th
 * uniform random permutation (torch.cat of randperms, mean_sampler.py:76).  labels == NULL with n_classes > 1: uniform labels
 * are drawn (mean_sampler.py:77).  labels_out (nullable, [n] int64) receives the labels used. */
int cslgan_mean_sample_f32(const float* mean_samples, int n_classes, int num_samples, int64_t len, const int64_t* labels,
                           const int64_t* perms, int64_t n, float noise_mean_std, float noise_std, uint64_t seed, uint64_t offset,
                           float* out, int64_t* labels_out, void* stream);

/* The generator's latent batch (gensamples.py:36, train.py:256: torch normal_ on the process RNG) as an INDEXED stream (ABI v7):
 * z[i][:] (row-major [n, dim]) holds the dim unit normals of sample g = first_index + *first_index_dev + i, a function of
 * (seed, g) alone — not of the batch size, of where a run was cut, or of how an index range is split between calls ("Device random
 * streams" above; csl_gan_amd.generate.latent_normals_host restates it on the host).  first_index_dev (nullable, device): its value
 * is ADDED to first_index inside the kernel, as call_counter is for the gradient noise — a recorded graph draws new rows on every
 * replay.  labels (nullable, [n] int64) receives fixed_label when fixed_label >= 0, else g mod n_classes: class-balanced over any
 * contiguous range, no draw needed.  n_classes >= 1, fixed_label < n_classes; dim need not be a multiple of 4. */
int cslgan_latent_normal_f32(uint64_t seed, uint64_t first_index, const unsigned long long* first_index_dev, int64_t n, int dim, float* z,
                             int n_classes, int fixed_label, int64_t* labels, void* stream);

/* Row L2 norms of a [n_rows, len] matrix (gradient_penalty.py:52-53) and the backward of
 * norm: gin[r][j] = gnorm[r] * in[r][j] / norm[r].  A row whose norm is exactly 0 gets a gradient of 0, as torch's 2-norm
 * backward gives it, not 0 / 0. */
int cslgan_row_l2norm_f32(const float* in, int64_t n_rows, int64_t len, float* out_norm, void* stream);
int cslgan_row_l2norm_bwd_f32(const float* in, const float* norm, const float* gnorm, int64_t n_rows,
                              int64_t len, float* gin, void* stream);

/* ---- convolution family: fp32 MFMA implicit GEMM ------------------------------------------ */

/* cslgan_conv_t.compute.  All tensors are fp32 in HBM either way.
 *   CSLGAN_COMPUTE_F32 : v_mfma_f32_32x32x2_f32 — bit-for-bit an fp32 fmaf chain; the default and the headline path.
 *   CSLGAN_COMPUTE_BF16: operands rounded to bfloat16 (round-to-nearest-even) on their way into LDS, v_mfma_f32_32x32x16_bf16
 *                        with fp32 accumulate (BASELINE.json configs[4]; `--compute_dtype bf16`).  Honoured by conv2d_fwd,
 *                        conv2d_s2_fwd, conv2d_dgrad, conv2d_wgrad_grouped(_bf16out), conv2d_wgrad_scaled; the vector-ALU
 *                        (1..4 channel) kernels, the RGB first layer (3 -> 64, 5x5, stride 2), single-output linear layers and the
 *                        Gram-norm entries compute in fp32 regardless (a fraction of a per cent of the FLOP).
 *   CSLGAN_COMPUTE_BF16X3: fp32 emulated on the bf16 matrix cores — every operand is split into three bfloat16 pieces
 *                        (x = hi + mid + lo, 3 x 8 mantissa bits = fp32's 24), a product is the sum of the six largest of the nine
 *                        piece products (each exact in fp32), fp32 accumulate: per-product error about one fp32 ulp at 2.67x the
 *                        fp32 MFMA rate.  Same entries as BF16. */
enum { CSLGAN_COMPUTE_F32 = 0, CSLGAN_COMPUTE_BF16 = 1, CSLGAN_COMPUTE_BF16X3 = 2 };

typedef struct {
    int32_t N, H, W, C;          /* input  x[N][H][W][C]                                     */
    int32_t K, R, S;             /* filter w[K][R][S][C]                                     */
    int32_t stride, pad;
    int32_t compute;             /* CSLGAN_COMPUTE_F32 (exact fp32 MFMA) or CSLGAN_COMPUTE_BF16 (see below) */
    int32_t P, Q;                /* output y[N][P][Q][K]                                     */
    /* ABI v6: optional device scratch for launches that would leave most of the chip idle (the critic's last convs: 64-384
     * workgroups on 256 CUs).  When given, the LDS-halo kernel of csrc/igemm_x3.hip may divide the REDUCTION channels over up to
     * split_ws_floats / (output floats) workgroups per output tile, each writing its partial sums here, and a second launch adds
     * the partials in a fixed order and applies bias / activation / mask (deterministic: no atomics).  NULL / 0: never split. */
    void* split_ws;
    int64_t split_ws_floats;
    /* ABI v6: GroupNorm statistics from the conv's epilogue (cslgan_conv2d_fwd_x3_f32 only).  When gn_part is given, every
     * workgroup of the halo kernel also leaves, for each of its 64-row patches and each of the gn_groups channel groups it covers,
     * the pair (sum, centred sum of squares about the patch's own mean) of the values it stores:
     *   gn_part[((n * (P*Q/64) + patch) * gn_groups + g) * 2 + {0, 1}]
     * cslgan_groupnorm_apply_parts_f32 combines the P*Q/64 pairs of an image exactly (Chan et al.) — the statistics pass over the
     * activation (one launch and one read of the tensor per normalisation) is gone.  Needs stride 1, P % 8 == Q % 8 == 0, act ==
     * NONE, K % gn_groups == 0 with K / gn_groups in {1, 2, 4, 8, 16, 32} and a shape the halo kernel takes; anything else is an
     * error (the caller then normalises with cslgan_groupnorm_act_f32). */
    float* gn_part;
    int32_t gn_groups;
    int32_t in_relu;
    /* ABI v6: a per-(sample, channel) affine map (+ ReLU when in_relu != 0) applied to x while it is staged —
     *   x'[n][h][w][c] = max(in_scale[n*C + c] * x[n][h][w][c] + in_shift[n*C + c], in_relu ? 0 : -inf), zero padding AFTER the map —
     * i.e. GroupNorm + ReLU folded into the consuming conv (cslgan_groupnorm_affine_parts_f32 makes the two tables from the
     * producing conv's statistics): the normalised activation is never written to HBM.  Taken by cslgan_conv2d_fwd_x3_f32 on the
     * shapes the LDS-halo kernel runs and by the 1..4-output-channel kernel behind cslgan_conv2d_fwd_f32 (64 input channels);
     * anything else is an error.  NULL: x is used as it is. */
    const float* in_scale;
    const float* in_shift;
} cslgan_conv_t;

/* y = act(conv(x, w) + bias [+ residual]).  Replaces torch.nn.Conv2d / nn.Linear forward at
 * DCResNet_models.py:131-132,145 (D), :16 (the conv inside UpsampleConv, run on the depth-to-space tensor with
 * channel-folded filters, see cslgan_depth_to_space_f32), :26,:36,:85,:95-104 (G), MNIST_models.py:17-23,41-46.
 *   bias      : [K] or NULL
 *   residual  : NULL or r[N][P][Q][K], added before act (ResBlockUp's "o + s", DCResNet_models.py:38)
 * A Linear layer is the 1x1 case H=W=P=Q=R=S=1. */
int cslgan_conv2d_fwd_f32(const cslgan_conv_t* p, const float* x, const float* w, const float* bias,
                          const float* residual, int act, float* y, void* stream);

/* cslgan_conv2d_fwd_f32 with compute == CSLGAN_COMPUTE_BF16X3 and the filter pre-split into its three bfloat16 pieces
 * (or compute == CSLGAN_COMPUTE_BF16 and the filter pre-rounded: one piece, the same layout):
 * w3_ws is a caller workspace of 3 * K*R*S*C bfloat16 (= 1.5 * K*R*S*C floats), rebuilt from w when repack != 0 and reused
 * otherwise (the caller knows when w changed).  Stride-1 convs on 8x8-patchable grids with C % 16 == 0 and K >= 64 then run on
 * the LDS-halo kernel whose filter operand goes straight from that workspace to registers; other shapes ignore it.
 * compute == CSLGAN_COMPUTE_F32 is accepted too (round 4): the workspace then holds an fp32 copy of the filter in the same
 * step-major order (K*R*S*C floats of the same allocation) and the kernel runs v_mfma_f32_32x32x2_f32 on the same staging —
 * exact fp32 products, the result of cslgan_conv2d_fwd_f32 up to summation order. */
int cslgan_conv2d_fwd_x3_f32(const cslgan_conv_t* p, const float* x, const float* w, void* w3_ws, int repack,
                             const float* bias, const float* residual, int act, float* y, void* stream);
/* The workspace of cslgan_conv2d_fwd_x3_f32 on its own (ABI v5): w[rows][taps][red] fp32 -> w3_ws[pieces][(red/16)*taps + tap][rows][16]
 * bfloat16 (pieces = 3: hi / mid / lo; 1: the rounded filter; 0: an fp32 copy, [step][rows][16] floats).  Lets a caller that replays a recorded graph refresh the pieces of a
 * FROZEN filter in place only when the filter has changed, instead of inside every replay; red % 16 != 0 writes nothing. */
int cslgan_split_filter_x3_f32(const float* w, int rows, int taps, int red, void* w3_ws, int pieces, void* stream);

/* gx = conv_transpose(gy, w) [* lrelu'(mask)]: the data gradient (autograd of the conv above;
 * "conv_transpose2d" in the north star).  wt_ws: caller workspace of K*R*S*C floats receiving
 * the repacked filters (rebuilt when repack != 0, reused otherwise).  mask (nullable) has gx's shape:
 * gx *= (mask > 0 ? 1 : 0.2). */
int cslgan_conv2d_dgrad_f32(const cslgan_conv_t* p, const float* gy, const float* w, float* wt_ws, int repack,
                            const float* mask, float* gx, void* stream);

/* cslgan_conv2d_dgrad_f32 with compute == CSLGAN_COMPUTE_BF16X3 (fp32 from three bfloat16 pieces) or CSLGAN_COMPUTE_BF16 on the
 * LDS-halo kernel of csrc/igemm_x3.hip (ABI v5): w3_ws is a second caller workspace of 3 * K*R*S*C bfloat16 receiving the
 * repacked parity-class matrices split into their pieces in step-major order (rebuilt with wt_ws when repack != 0).  Takes
 * stride 1-2, K % 16 == 0, C >= 64, class grids 8x8-patchable or 4x4; other shapes run the gather kernels in the same
 * arithmetic and ignore w3_ws.  compute == CSLGAN_COMPUTE_F32: w3_ws receives fp32 step-major class matrices and the launch is the
 * exact-fp32 form of the same kernel (8x8-patchable class grids only).  Same call it replaces: the autograd data gradient of nn.Conv2d (DCResNet_models.py:131-132)
 * and its use inside the penalty's double backward (gradient_penalty.py:48-54). */
int cslgan_conv2d_dgrad_x3_f32(const cslgan_conv_t* p, const float* gy, const float* w, float* wt_ws, void* w3_ws, int repack,
                               const float* mask, float* gx, void* stream);

/* Grouped weight gradient:  gw[g][k][r][s][c] = alpha * sum_{n in group g} sum_{p,q} gy[n,p,q,k] x[n,..,c]
 * with groups of `group` consecutive samples (N % group == 0).
 *   group == 1 -> per-sample gradients p.grad_sample (Opacus hook, train.py:387)
 *   gw == NULL -> norms only ("ghost" mode)
 *   sq (nullable): [N/group] += sum of squares of alpha*gw[g]  (caller zeroes)
 * The dense gradient is group == N, or any group followed by cslgan_clip_accum_noise_f32. */
int cslgan_conv2d_wgrad_grouped_f32(const cslgan_conv_t* p, const float* gy, const float* x, int group,
                                    float alpha, float* gw, float* sq, void* stream);

/* Per-sample weight gradients of a batch made of consecutive ROW BLOCKS with their own outputs, in one launch — the fused
 * discriminator pass of train.py:204-245 + 382-389 carries the adaptive-clipping rows (norms only), the generated rows (only
 * their sum is used) and the private rows (materialised) in one batch, and three launches of 640 workgroups each fill
 * 512 slots 62 % where one launch of 1920 fills them 94 %.  Block b covers samples [block_first[b], block_first[b+1]) (the last
 * one ends at N); sample n of block b writes gw[b] + (n - block_first[b]) * K*R*S*C (nothing when gw[b] is NULL) and adds
 * ||alpha * g_n||^2 into sq[b][n - block_first[b]] (skipped when sq[b] is NULL; the caller zeroes).  gw and sq are HOST arrays of
 * n_blocks device pointers.  fp32 only, on the shapes igemm_wgh takes (stride 1-2, 2..5 filter columns, K % 64 == 0,
 * C % 64 == 0, P % 8 == 0, Q % 8 == 0); other shapes return CSLGAN_ERR_INVALID_ARG and the caller uses one
 * cslgan_conv2d_wgrad_grouped_f32 call per block. */
#define CSLGAN_MAX_WGRAD_BLOCKS 4
int cslgan_conv2d_wgrad_blocks_f32(const cslgan_conv_t* p, const float* gy, const float* x, float alpha, int n_blocks,
                                   const int32_t* block_first, float* const* gw, float* const* sq, void* stream);

/* Stride-2 forward conv (the critic's convs, DCResNet_models.py:131) through the LDS-halo kernel: the four parity
 * sub-images of x are convolved at stride 1 and accumulated in one workgroup.  wcls_ws: K*R*R*C floats receiving the
 * filters regrouped by parity class (rebuilt when repack != 0).  Same result as cslgan_conv2d_fwd_f32, to which it falls
 * back for shapes the halo kernel does not take (C % 32, K >= 64, 8x8-patchable or 4x4 output grid). */
int cslgan_conv2d_s2_fwd_f32(const cslgan_conv_t* p, const float* x, const float* w, float* wcls_ws, int repack,
                             const float* bias, int act, float* y, void* stream);

/* The same stride-2 forward conv with compute == CSLGAN_COMPUTE_BF16X3 / CSLGAN_COMPUTE_BF16 on the LDS-halo kernel of
 * csrc/igemm_x3.hip (ABI v5): w3_ws = 3 * K*R*R*C bfloat16 receiving the parity-class matrices split into their pieces
 * (rebuilt with wcls_ws when repack != 0).  C % 16 == 0, K >= 64, 8x8-patchable or 4x4 output grid; other shapes fall back
 * to cslgan_conv2d_fwd_f32 in the same arithmetic.  compute == CSLGAN_COMPUTE_F32: as for cslgan_conv2d_dgrad_x3_f32. */
int cslgan_conv2d_s2_fwd_x3_f32(const cslgan_conv_t* p, const float* x, const float* w, float* wcls_ws, void* w3_ws, int repack,
                                const float* bias, int act, float* y, void* stream);

/* Clip-weighted grouped weight gradient: as cslgan_conv2d_wgrad_grouped_f32 with gy of sample n multiplied by
 * row_scale[n] on load.  With row_scale = the per-sample clip factors f_b and group = N this is the clipped sum
 * sum_b f_b g_b (privacy_engine.clip() + accumulate, train.py:399-417) without materialising p.grad_sample. */
int cslgan_conv2d_wgrad_scaled_f32(const cslgan_conv_t* p, const float* gy, const float* x, const float* row_scale,
                                   int group, float alpha, float* gw, void* stream);

/* Dense weight gradient of a stride-1 conv with 1..4 output channels and 64 input channels (G's output conv in
 * train_G, train.py:502-511), on the vector ALU.  Each of the n_blocks workgroups writes one partial [K][R*S][64]
 * row into partial[n_blocks][K*R*S*64]; the caller sums the rows (cslgan_clip_accum_noise_f32).  Needs P, Q
 * multiples of 8 and at most 9 taps. */
int cslgan_conv2d_wgrad_skinny_f32(const cslgan_conv_t* p, const float* gy, const float* x, float alpha, float* partial,
                                   int n_blocks, void* stream);

/* Per-sample squared norms of the weight gradient WITHOUT forming it:  sq[n] += alpha^2 * sum_{p,p'}
 * (GY_n GY_n^T)[p,p'] (XU_n XU_n^T)[p,p']  — the same value cslgan_conv2d_wgrad_grouped_f32(group=1, gw=NULL)
 * accumulates (opacus calc_sample_norms, train.py:311-314), 30x fewer FLOP for the critic's last conv.
 * Needs P*Q <= 64, K % 32 == 0, C % 32 == 0.  sq: [N], caller zeroes. */
int cslgan_conv2d_wgrad_sqnorm_gram_f32(const cslgan_conv_t* p, const float* gy, const float* x, float alpha, float* sq,
                                        void* stream);

/* Same, storing gw as bfloat16 (round-to-nearest-even); sq is the norm of the ROUNDED values, i.e. of what
 * the clip kernels will read back. */
int cslgan_conv2d_wgrad_grouped_bf16out_f32(const cslgan_conv_t* p, const float* gy, const float* x, int group,
                                            float alpha, void* gw_bf16, float* sq, void* stream);

/* Per-group bias gradient gb[g][k] = alpha * sum_{n in g, p, q} gy[n,p,q,k]; sq as above. */
int cslgan_bias_grad_grouped_f32(const float* gy, int N, int PQ, int K, int group, float alpha,
                                 float* gb, float* sq, void* stream);

/* ---- bf16 STORAGE (BASELINE.json configs[4]; csrc/igemm_bf16s.hip) -------------------------------------------------
 * The entries above read fp32 tensors whatever cslgan_conv_t.compute says.  These read and write ACTIVATIONS and ACTIVATION
 * GRADIENTS stored as bfloat16 in HBM (NHWC, the same index maps), with a bfloat16 copy of the fp32 master filter; sums are
 * fp32 (v_mfma_f32_32x32x16_bf16), weight gradients / norms are fp32.  `*_bf16` flags give the element type of the tensor
 * named before them (0 = float, 1 = bfloat16).  Replaces the same reference calls as the fp32 entries: nn.Conv2d / nn.Linear
 * forward and data gradient (DCResNet_models.py:131-132,145), per-sample weight gradients (train.py:373,387). */

/* y = act(conv(x, w) + bias [+ residual]); x bf16 [N,H,W,C] with C % 8 == 0; w the fp32 KRSC filter, wb_ws a caller-owned
 * bf16 workspace of K*R*S*C elements holding bf16(w) (written here when repack != 0: once per parameter version);
 * residual (nullable) and y are bf16 or fp32 as flagged. */
int cslgan_conv2d_fwd_bf16s(const cslgan_conv_t* p, const void* x, const float* w, void* wb_ws, int repack, const float* bias,
                            const void* residual, int res_bf16, int act, void* y, int y_bf16, void* stream);

/* gx = conv_transpose(gy, w) (* lrelu'(mask)); gy bf16 [N,P,Q,K] with K % 8 == 0; wt_ws: bf16 workspace of K*R*S*C elements for
 * the per-parity-class filter matrices (written when repack != 0); mask (nullable) has gx's shape AND element type. */
int cslgan_conv2d_dgrad_bf16s(const cslgan_conv_t* p, const void* gy, const float* w, void* wt_ws, int repack, const void* mask,
                              void* gx, int gx_bf16, void* stream);

/* cslgan_conv2d_wgrad_grouped_f32 on bf16 gy [N,P,Q,K] and bf16 x [N,H,W,C] (K % 8 == 0, C % 8 == 0): gw fp32 (bf16 when
 * gw_bf16; nullable) and / or sq[N/group] += ||alpha gw_g||^2. */
int cslgan_conv2d_wgrad_grouped_bf16s(const cslgan_conv_t* p, const void* gy, const void* x, int group, float alpha, void* gw,
                                      int gw_bf16, float* sq, void* stream);

/* The critic's head nn.Linear(C, 1) (DCResNet_models.py:145) on bf16 features x [N, C], C % 8 == 0 (its forward is
 * cslgan_conv2d_fwd_bf16s with K == 1): data gradient gx[n,:] = bf16(gy[n] * bf16(w) (* lrelu'(mask[n,:]))) from fp32 gy [N], with
 * bf16 mask / gx [N, C]; grouped weight gradient gw[N/group, C] = alpha * sum_{n in g} gy[n] x[n,:] (fp32, nullable) and / or
 * sq[N/group] += ||gw_g||^2. */
int cslgan_linear_k1_dgrad_bf16s(const float* gy, const float* w, const void* mask_bf16, int N, int64_t C, void* gx_bf16, void* stream);
int cslgan_linear_k1_wgrad_bf16s(const float* gy, const void* x_bf16, const float* row_scale, int N, int64_t C, int group, float alpha,
                                 float* gw, float* sq, void* stream);   /* row_scale (nullable, [N]): gy[n] is weighted by row_scale[n] */

/* The critic's RGB first layer (3 -> 64 channels, 5x5, stride 2; csrc/conv_c3.hip) at the edge of the bf16-stored chain: fp32 image
 * and fp32 arithmetic as in cslgan_conv2d_fwd_f32 / cslgan_conv2d_wgrad_grouped_f32(group = 1), with the OUTPUT stored as bfloat16 /
 * the output gradient read as bfloat16.  Only the shapes the first-layer kernels take (even image, P % 8 == 0, Q % 16 == 0 forward;
 * Q in {16, 32, 64} with whole-row strips for the weight gradient); anything else is an error. */
int cslgan_conv2d_c3_fwd_bf16out(const cslgan_conv_t* p, const float* x, const float* w, const float* bias, int act, void* y_bf16,
                                 void* stream);
int cslgan_conv2d_c3_wgrad_bf16gy(const cslgan_conv_t* p, const void* gy_bf16, const float* x, float alpha, float* gw, float* sq,
                                  void* stream);

/* nn.GroupNorm(groups, C) + ReLU (DCResNet_models.py:55-57) writing bf16-stored activations: x fp32 or bfloat16 (x_bf16), y and
 * x_shuffled bfloat16; everything else as cslgan_groupnorm_act_f32 (fp32 statistics, d2s_W > 0 = depth-to-space output layout). */
int cslgan_groupnorm_act_bf16s(const void* x, int x_bf16, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                               float eps, int relu, float* stats_ws, void* y_bf16, int d2s_W, void* x_shuffled_bf16, void* stream);

/* The two 1..4-channel ends of the bf16-stored chain on the vector-ALU kernel (csrc/igemm_skinny.hip), reading bfloat16, computing and
 * writing fp32: the generator's output conv (64 -> 3 channels, stride 1; DCResNet_models.py:85) on a bf16 input, and the data gradient
 * of the critic's RGB first layer (the image gradient of gradient_penalty.py:48-50) from a bf16 output gradient.  Shapes the
 * vector-ALU kernel does not take are an error. */
int cslgan_conv2d_fwd_skinny_bf16in(const cslgan_conv_t* p, const void* x_bf16, const float* w, const float* bias, int act, float* y,
                                    void* stream);
int cslgan_conv2d_dgrad_skinny_bf16in(const cslgan_conv_t* p, const void* gy_bf16, const float* w, float* wt_ws, int repack, float* gx,
                                      void* stream);

/* cslgan_conv2d_wgrad_scaled_f32 on bf16 gy / x: gw[N/group] = alpha * sum_{n in g} row_scale[n] * (weight gradient of sample n) —
 * clip() + accumulate of ghost-clipped layers (train.py:399-402).  The fp32 weight is applied to each sample's ACCUMULATED product,
 * never to a bfloat16 operand, so every summed contribution is row_scale[n] times exactly the gradient
 * cslgan_conv2d_wgrad_grouped_bf16s(group = 1) would store.  Needs P*Q % 64 == 0. */
int cslgan_conv2d_wgrad_scaled_bf16s(const cslgan_conv_t* p, const void* gy, const void* x, const float* row_scale, int group, float alpha,
                                     float* gw, void* stream);

/* Element-type conversions at the edges of the bf16-stored chain (round-to-nearest-even / exact widening). */
int cslgan_cast_f32_bf16(const float* in, void* out_bf16, int64_t n, void* stream);
int cslgan_cast_bf16_f32(const void* in_bf16, float* out, int64_t n, void* stream);

/* cslgan_act_bwd_f32 / cslgan_bias_grad_grouped_f32 on bf16 tensors (fp32 sums; n % 8 == 0; K % 8 == 0, 256 % (K/8) == 0). */
int cslgan_act_bwd_bf16(const void* g, const void* y, int64_t n, float slope, void* out, void* stream);
int cslgan_bias_grad_grouped_bf16(const void* gy, int N, int PQ, int K, int group, float alpha, float* gb, float* sq, void* stream);

/* ---- pointwise / normalisation ------------------------------------------------------------- */

/* out = g * (y > 0 ? 1 : slope)   (LeakyReLU / ReLU backward from the OUTPUT y) */
int cslgan_act_bwd_f32(const float* g, const float* y, int64_t n, float slope, float* out, void* stream);

/* UpsampleConv's data movement (DCResNet_models.py:13-15): torch.cat([x]*4, 1) followed by F.pixel_shuffle(., 2).
 * pixel_shuffle is channel-major, so up[c][2h+i][2w+j] = x[(4c + 2i + j) mod C][h][w]: for C % 4 == 0 the C channels of
 * `up` are the C/4 channels of the plain depth-to-space tensor
 *       ps[n][2h+i][2w+j][c'] = x[n][h][w][4c' + 2i + j]                         (NHWC, [N][2H][2W][C/4])
 * repeated four times, and the conv that follows (DCResNet_models.py:16) equals a conv of ps with the filter summed over
 * the four channel groups — a quarter of the multiply-adds, the sums only re-associate the reference arithmetic.
 *   cslgan_depth_to_space_f32 : inverse == 0: ps from x[N][H][W][C];  inverse != 0: x[N][H][W][C] from ps (its gradient)
 *   cslgan_fold_channels4_f32 : unfold == 0: wf[row][c'] = sum_q w[row][c' + q*C/4], rows = K*R*S of a KRSC filter;
 *                               unfold != 0: gw[row][c' + q*C/4] = gwf[row][c']  (the gradient of w from that of wf)
 * The normalisation entries below can write their output (and the raw input) directly in the ps layout. */
int cslgan_depth_to_space_f32(const float* in, int N, int H, int W, int C, int inverse, float* out, void* stream);
int cslgan_fold_channels4_f32(const float* in, int64_t rows, int C, int unfold, float* out, void* stream);

/* GroupNorm(groups) + optional ReLU on NHWC x[N][HW][C] (DCResNet_models.py:55-57,63-67,101-102).
 * stats_ws: caller workspace [2*N*groups] floats (sum, centred sum of squares per statistic).
 * d2s_W > 0: the image is HW/d2s_W rows of d2s_W pixels and y is written depth-to-space shuffled,
 * y[n][2h+i][2w+j][c'] = act(norm(x))[n][h][w][4c'+2i+j] (C % 4 == 0); x_shuffled (nullable) receives the raw x in the
 * same layout — the inputs of ResBlockUp's convUp and shortcut (DCResNet_models.py:29-34) from one read of x.
 * d2s_W == 0: y has x's layout and x_shuffled must be NULL.
 * scratch (nullable; ABI v5 meaning): caller workspace of 2*N*groups*CSLGAN_NORM_PARTIAL_BLOCKS floats (no initialisation needed)
 * for per-workgroup partial statistics: the normalisation then runs as TWO launches (statistics, apply — the apply kernel adds the
 * partials in its prologue and publishes the final pairs to stats_ws) instead of four (zero, statistics with atomics, finalize,
 * apply).  The routes with global atomics (more than CSLGAN_NORM_PARTIAL_BLOCKS workgroups per statistic, or the scalar
 * kernels) use scratch too: its first N*groups floats carry the means of a first statistics pass, the shift of a second one.  One scratch must not be shared by launches on different streams. */
#define CSLGAN_NORM_PARTIAL_BLOCKS 64
/* The apply half of cslgan_groupnorm_act_f32 on statistics a conv epilogue left behind (cslgan_conv_t.gn_part): part holds
 * n_part = HW/64 (sum, centred sum of squares) pairs per image and group; everything else as cslgan_groupnorm_act_f32
 * (stats_ws receives the final pairs).  n_part <= CSLGAN_NORM_PARTIAL_BLOCKS. */
/* The same statistics as a per-(sample, channel) affine map for cslgan_conv_t.in_scale / in_shift:
 * scale[n*C + c] = gamma[c] * rstd(n, group of c), shift[n*C + c] = beta[c] - mean(n, group of c) * scale[n*C + c]. */
int cslgan_groupnorm_affine_parts_f32(const float* part, int n_part, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                                      float eps, float* scale, float* shift, void* stream);
int cslgan_groupnorm_apply_parts_f32(const float* x, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                                     float eps, int relu, const float* part, int n_part, float* stats_ws, float* y, int d2s_W,
                                     float* x_shuffled, void* stream);
int cslgan_groupnorm_act_f32(const float* x, const float* gamma, const float* beta, int N, int HW, int C,
                             int groups, float eps, int relu, float* stats_ws, float* y, int d2s_W, float* x_shuffled,
                             float* scratch, void* stream);
/* cslgan_groupnorm_apply_parts_f32 with d2s_W > 0 and ResBlockUp's 1x1 shortcut conv in ONE launch (csrc/gn_shortcut.hip; a new
 * entry under ABI v7: no existing entry or struct changes):
 * y receives the shuffled activation exactly as the apply entry writes it, stats_ws the final pairs, and instead of the raw
 * x_shuffled (never written) the kernel leaves the conv that would have read it,
 *   s[n][2h+i][2w+j][k] = bias[k] + sum_c' wf[k][c'] * x[n][h][w][4c'+2i+j]
 * wf[K][C/4]: the shortcut filter folded over the four channel groups (cslgan_fold_channels4_f32); bias[K] nullable.
 * Needs C / 4 in {32, 64, 128}, K % 64 == 0, HW == 64 * n_part (n_part <= CSLGAN_NORM_PARTIAL_BLOCKS), d2s_W dividing HW,
 * N <= 65535, 4 * HW * K < 2^31 and x, y, wf, s aligned to 16 bytes; anything else is an error before any launch. */
int cslgan_groupnorm_apply_parts_shortcut_f32(const float* x, const float* gamma, const float* beta, int N, int HW, int C, int groups,
                                              float eps, int relu, const float* part, int n_part, float* stats_ws, float* y,
                                              int d2s_W, const float* wf, const float* bias, int K, float* s, void* stream);

/* Training-mode BatchNorm2d (+ optional ReLU) on NHWC x[rows][C], rows = N*H*W: batch statistics per channel,
 * running_mean / running_var (nullable pair) updated with `momentum` and the unbiased variance — the bn=True
 * generator of the non-per-sample modes (init_util.py:46, DCResNet_models.py:23,25,84).
 * stats_ws: caller workspace [2*C] floats.  rows_per_image / d2s_W / x_shuffled: as for GroupNorm (rows_per_image
 * = H*W is only read when d2s_W > 0). */
int cslgan_batchnorm_act_f32(const float* x, const float* gamma, const float* beta, int64_t rows, int C, float eps,
                             int relu, float momentum, float* running_mean, float* running_var, float* stats_ws,
                             float* y, int64_t rows_per_image, int d2s_W, float* x_shuffled, float* scratch /* as above, 2*C floats + 1 ticket */,
                             void* stream);

/* Eval-mode BatchNorm2d (+ optional ReLU): y = act((x - running_mean) / sqrt(running_var + eps) * gamma + beta) — the
 * generator in eval() when images are sampled (train.py:298-308, gensamples.py:26-41). */
int cslgan_batchnorm_eval_act_f32(const float* x, const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, int64_t rows, int C, float eps, int relu, float* stats_ws,
                                  float* y, int64_t rows_per_image, int d2s_W, float* x_shuffled, void* stream);

/* Backward of GroupNorm / BatchNorm (+ReLU): dx, dgamma, dbeta from the forward's x, y (ReLU mask) and the
 * stats workspace the forward filled.  rows_per_stat = H*W (GroupNorm) or rows (BatchNorm, groups = C).
 * ws: caller workspace of cslgan_norm_bwd_ws_floats(...) floats. */
int cslgan_norm_act_bwd_f32(const float* x, const float* dy, const float* y, const float* gamma, const float* stats,
                            int64_t rows, int64_t rows_per_stat, int C, int groups, float eps, int relu, float* ws,
                            float* dx, float* dgamma, float* dbeta, void* stream);
int64_t cslgan_norm_bwd_ws_floats(int64_t rows, int64_t rows_per_stat, int C, int groups);

/* Adam (torch.optim.Adam semantics, train.py:76): in-place on p, m, v.  step is 1-based. */
int cslgan_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1,
                         float b2, float eps, float weight_decay, int step, void* stream);
/* Same with the (1-based) step count read from device memory: a step captured in a HIP graph must not bake it in. */
int cslgan_adam_step_dev_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1,
                             float b2, float eps, float weight_decay, const int32_t* step_dev, void* stream);

/* Adam over n_seg <= CSLGAN_MAX_SEGS tensors in ONE launch (the optimizer's per-parameter loop, train.py:76,484).  step_dev
 * (nullable): device int32 holding the 1-based step — when given, `step` is ignored (HIP-graph replay). */
int cslgan_adam_multi_f32(int n_seg, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                          float lr, float b1, float b2, float eps, float weight_decay, int step, const int32_t* step_dev,
                          void* stream);

/* ---- fused glue of the D-step (csrc/step_kernels.hip): each replaces a run of 4-us elementwise / reduction launches ---- */
/* The critic's losses over the row blocks of one pass (DCResNet_models.py:149-153: real_loss = -mean, fake_loss = +mean):
 * vec[s] = scale[s] * sum(x[block s]), total = sum_s vec[s].  sizes / scale: HOST arrays of n_seg <= CSLGAN_MAX_ROLES entries. */
int cslgan_segment_means_f32(const float* x, int n_seg, const int32_t* sizes, const float* scale, float* vec, float* total,
                             void* stream);
/* gx[i] = (g_total + g_vec[s(i)]) * scale[s(i)]; either gradient (device scalar / [n_seg]) may be NULL, not both. */
int cslgan_segment_means_bwd_f32(const float* g_total, const float* g_vec, int n_seg, const int32_t* sizes, const float* scale,
                                 float* gx, void* stream);
/* train.py:488-496, the logger.stats[...] += lines of train_D: acc7 += {adv loss (G gate), D Adv Loss, D Real Loss, D Fake Loss,
 * D Real Acc = 100*mean(d_real > 0), D Fake Acc = 100*mean(d_fake < 0), D Penalty (penalty may be NULL)}. */
int cslgan_dstep_stats_f32(const float* d_real, int n_real, const float* d_fake, int n_fake, const float* real_loss,
                           const float* fake_loss, const float* penalty, float* acc7, void* stream);
/* update_grad_logging (train.py:310-329) from the squared norms the clip already holds: sq[n_layers, ld], logged columns
 * [col0, col0 + B).  per_layer: one row of statistics per layer against max_norm[layer]; else ONE row from the flat norm
 * sqrt(sum_l sq) against max_norm[0].  Adds mean / population std / max of the norms, the clip norm and the fraction of
 * samples with min(1, C/(norm+eps)) < 0.999 to the five accumulators (each [n_layers] or [1]). */
int cslgan_grad_log_stats_f32(const float* sq, int n_layers, int64_t ld, int64_t col0, int B, const float* max_norm, int per_layer,
                              float eps, float* acc_mean, float* acc_std, float* acc_max, float* acc_c, float* acc_clipped,
                              void* stream);
/* Adaptive clipping of one fused critic pass in ONE launch (train.py:233-243 update_adaptive_clipping_params + :324
 * calc_clipping_factors; the device form ran stack, sqrt, mean, mul, stack, clip-factor, gather and three row-scale launches):
 *   r[l]   = mean_i (stat_max: max_i) sqrt(sq_adapt[l][i])                     over the n_adapt adaptive rows of layer l
 *   C      = scalar * r[l] per layer (per_layer) | scalar * ||r||_2 (one flat clip norm)
 *   sq_out = the layers' sq_rows stacked [n_layers][n_rows];  f = min(1, C / (norm + eps)), 1 for rows < first_private_row:
 *            per_layer [n_layers][n_rows] from each layer's own norm, else [n_rows] from the flat norm sqrt(sum_l sq)
 *   f_mat  (nullable, per_layer) [n_mat][n_rows] = f[mat_layer[m]];  jobs: job_dst[j][i] = job_scale[j] * f[job_layer[j]][job_first[j] + i]
 *            (flat: f[job_first[j] + i]) for i < job_count[j] — the row weights of the clip-weighted weight-gradient launches.
 * Pointers inside the struct are DEVICE pointers; the struct itself is read on the host. */
#define CSLGAN_MAX_CLIP_LAYERS 32
#define CSLGAN_MAX_CLIP_JOBS 16
typedef struct {
    int32_t n_layers, n_mat, n_jobs, _pad;
    const float* sq_adapt[CSLGAN_MAX_CLIP_LAYERS];
    const float* sq_rows[CSLGAN_MAX_CLIP_LAYERS];
    int32_t mat_layer[CSLGAN_MAX_CLIP_LAYERS];
    float* job_dst[CSLGAN_MAX_CLIP_JOBS];
    int64_t job_first[CSLGAN_MAX_CLIP_JOBS];
    int32_t job_layer[CSLGAN_MAX_CLIP_JOBS];
    int32_t job_count[CSLGAN_MAX_CLIP_JOBS];
    float job_scale[CSLGAN_MAX_CLIP_JOBS];
} cslgan_adaptive_clip_t;
int cslgan_adaptive_clip_f32(const cslgan_adaptive_clip_t* a, int64_t n_adapt, int64_t n_rows, int stat_max, float scalar, int per_layer,
                             float eps, int64_t first_private_row, float* r_out, float* c_out, float* sq_out, float* f_out, float* f_mat,
                             void* stream);
/* gradient_penalty.py:36: out[b,:] = alpha[b] * real[b,:] + (1 - alpha[b]) * fake[b,:]. */
int cslgan_lerp_rows_f32(const float* real, const float* fake, const float* alpha, int64_t n_rows, int64_t len, float* out,
                         void* stream);
/* gradient_penalty.py:52-54 (+ the weight and batch mean of :41,:65) in one launch: norm[b] = ||t[b,:]||, per[b] = coef *
 * (norm-1)^2 (one_sided: max(norm-1,0)^2), total (nullable) = sum_b per[b].  ticket: one zero-initialised device uint32 the
 * kernel uses to find its last workgroup and leaves at zero. */
int cslgan_lipschitz_term_f32(const float* t, int64_t n_rows, int64_t len, int one_sided, float coef, float* norm, float* per,
                              float* total, uint32_t* ticket, void* stream);
/* gt[b,:] = (g_total + g_per[b]) * coef * 2 (norm_b - 1)[clamped] * t[b,:] / norm_b; either gradient may be NULL, not both.
 * A row with norm_b == 0 gets a gradient of 0 (torch's 2-norm backward at the origin), not 0 * inf. */
int cslgan_lipschitz_term_bwd_f32(const float* t, const float* norm, const float* g_total, const float* g_per, int64_t n_rows,
                                  int64_t len, int one_sided, float coef, float* gt, void* stream);


/* ---- input pipeline (ABI v5) ----------------------------------------------------------------------------------------------------
 * out[n][h][w][c] = src[n][h][flip[n] ? W-1-w : w][c] * scale + bias: a batch of uint8 NHWC images (the preprocessed-tensor cache of
 * csl_gan_amd/pipeline.py, uploaded as 1 byte per element) becomes the normalised fp32 channels-last batch the critic reads.
 * Replaces the per-image ToTensor / RandomHorizontalFlip / Normalize of datasets.py:41-47 (flip: nullable [N] bytes drawn by the host
 * with p = 0.5; scale = 1/127.5, bias = -1 for Normalize(0.5, 0.5)). */
int cslgan_u8_to_f32_nhwc(const void* src_u8, const void* flip_u8, int N, int H, int W, int C, float scale, float bias, float* out, void* stream);

/* The inverse (ABI v7): n fp32 values in memory order (NHWC images) -> n bytes,
 *   t = clamp(src * scale + bias, 0, 1);  dst = (uint8) clamp(t * 255 + 0.5, 0, 255)      (truncation; NaN -> 0)
 * — util.denorm_celeba followed by the quantisation of util.save_image (train.py:303-306, gensamples.py:37-41) for
 * (scale, bias) = (0.5, 0.5), MNIST's [0, 1] images for (1, 0).  Every product and sum is rounded on its own, in this order: the bytes
 * equal the host's fp32 expression bit for bit.  16-byte loads / 4-byte stores where src is 16-byte and dst 4-byte aligned, element
 * by element otherwise. */
int cslgan_f32_to_u8(const float* src, int64_t n, float scale, float bias, void* dst_u8, void* stream);

/* ---- membership-inference audit (attack_kernels.hip; backward-compatible additions, ABI stays 7) ---------------------------------
 * All three validate on the host before any launch, never allocate and never synchronise.
 *
 * Audit sampler.  Trial T = first_trial + t (mod 2^64) draws n of the N train scores and m of the M non-train scores without
 * replacement: element j of a side's subset is v[pi(j)], j < k, with pi a keyed permutation of [0, N) built by the swap-or-not shuffle
 * (Hoang, Morris, Rogaway, CRYPTO'12) on Philox4x32-10 ("Device random streams" above):
 *     key     = the two halves of (seed xor 0x6D656D696E666174)
 *     tag     = 0x7472616E for the train side, 0x6E6F6E74 for the non-train side;  T lo / T hi = the 32-bit halves of T
 *     rounds  R = 8 * max(1, ceil(log2 N));  round r = 0 .. R-1, on x (starting at x = j):
 *         K_r = mulhi32(word 0 of Philox(0xFFFFFFFF, r, T lo, T hi ^ tag), N)         (one per round; x < 2^31 is never 0xFFFFFFFF)
 *         x'  = (K_r + N - x) mod N;   xh = max(x, x');   x <- x' iff word 0 of Philox(xh, r, T lo, T hi ^ tag) is odd
 * Every round is an involution of [0, N), so pi is a permutation for every N: no cycle walking, no rejection, and pi(j) is computed
 * by one lane without reference to any other.  csl_gan_amd.audit.subset_indices restates it in numpy.
 *
 * cslgan_attack_trials — attack() + _get_random_subset(), mem_inf_attack.py:29-66.  hits[t] (t < trials) = the number of train
 * elements among the n best of trial first_trial + t.  The pool is the n train values followed by the m non-train values;
 *     rank(i) = #{j : v[j] > v[i]} + #{j < i : v[j] == v[i]}        (Python's stable sorted(..., reverse=True): ties go to the train
 *     hits    = #{i < n : rank(i) < n}                               sample, which precedes every non-train sample in the pool)
 * 1 <= n <= N < 2^31, 0 <= m <= M < 2^31 (vn may be NULL when m == 0), n + m <= 4096 (the pool lives in LDS), trials < 2^31.
 * One workgroup runs one trial, so a call may be cut into chunks of trials at will. */
int cslgan_attack_trials(const float* vt, int64_t N, const float* vn, int64_t M, int n, int m, uint64_t seed, uint64_t first_trial,
                         int64_t trials, uint32_t* hits, void* stream);

/* Exact rank counts (an addition of this build; nothing in the reference): for i < na over b[nb],
 *     gt[i] = #{j : a[i] > b[j]},   eq[i] = #{j : a[i] == b[j]}         (IEEE comparisons: -0 == +0; a NaN counts nowhere)
 * from which the host derives AUC = sum(gt + eq / 2) / (na nb) and the TPR at an FPR budget.  na, nb < 2^31. */
int cslgan_rank_counts(const float* a, int64_t na, const float* b, int64_t nb, uint32_t* gt, uint32_t* eq, void* stream);

/* softmax(logits, 1).max(1)[0], mem_inf_attack.py:80:  out[b] = 1 / sum_j exp(l[b][j] - max_j l[b][j])  for [B, n_classes] fp32
 * logits, 1 <= n_classes <= 64.  The sum runs in fp64: out is the rounded fp32 of the formula on the fp32 logits. */
int cslgan_softmax_max_rows_f32(const float* logits, int64_t B, int n_classes, float* out, void* stream);

/* ---- downstream classifier (logreg_kernels.hip; backward-compatible additions, ABI stays 7) ---------------------------------------
 * One-vs-rest logistic regression over K <= 16 classes, as downstream.py:71-72 builds it (OneVsRestClassifier over
 * LogisticRegression(solver='lbfgs', multi_class='multinomial'), C = 1): handed a binary target, the multinomial form is a two-class
 * softmax, i.e. a binary logistic regression with C = 2.  With t_ik = [labels[i] == k], s = 2 t - 1 and U [D + 1, K] row-major (row
 * d < D: the weights of feature d; row D: the intercepts), class k minimises
 *     f_k(U) = sum_i log(1 + exp(-s_ik z_ik)) + sum_{d < D} U[d][k]^2 / 4,      z_ik = sum_{d < D} X[i][d] U[d][k] + U[D][k]
 * (no penalty on the intercept).  All entries validate on the host before any launch, never allocate and never synchronise;
 * 2 <= K <= 16, 1 <= D <= 895 (a 16-row tile of X lives in LDS), 1 <= N, M < 2^31.  D need not be a multiple of 4.
 *
 * cslgan_ovr_logreg_eval_f32 — one loss-and-gradient evaluation of all K problems, the inner call of the L-BFGS that replaces
 * .fit() of downstream.py:87:  loss[k] = f_k(U),  grad[d][k] = d f_k / d U[d][k]  ([D + 1, K] row-major like U).  Both products run
 * on the exact fp32 matrix instruction; X is read from HBM once; the softplus is the stable form (finite for every finite z);
 * workgroup partials are added in a fixed order in double, so two calls on the same inputs return the same bits.  labels outside
 * 0 .. K-1 belong to no class (t = 0 everywhere).  ws: caller workspace of cslgan_ovr_logreg_ws_floats(N, D) floats, 8-byte aligned. */
int64_t cslgan_ovr_logreg_ws_floats(int64_t N, int D);
int cslgan_ovr_logreg_eval_f32(const float* X, const int32_t* labels, const float* U, int64_t N, int D, int K, float* loss, float* grad,
                               float* ws, int64_t ws_floats, void* stream);

/* cslgan_ovr_logreg_proba_f32 — .predict_proba() of downstream.py:87 on the test matrix of :103-106:
 *     P[i][k] = sigmoid(z_ik) / sum_k' sigmoid(z_ik')          ([M, K] row-major)
 * Xtest: [M, D] fp32 (is_u8 = 0), or [M, D] bytes (is_u8 = 1) that become floats times 1/255 in the load (:106). */
int cslgan_ovr_logreg_proba_f32(const void* Xtest, int is_u8, const float* U, int64_t M, int D, int K, float* P, void* stream);

/* The same estimator on cache BYTES, for any row size (csl_gan_amd.tstr; backward-compatible additions, ABI stays 7).
 * The objective, U, loss, grad and P are those above with x_id = byte_id / 255, whatever scale the cache header records:
 *     z_ik = (sum_{d < D} byte_id U[d][k]) / 255 + U[D][k]
 * X / Xtest: uint8 [N, D] row-major, base 16-byte aligned, 1 <= D <= 65536 (as in the nearest-neighbour audit); D need not be a
 * multiple of 4 or 16 — rows are then unaligned and are assembled from aligned 16-byte words; no byte beyond X + N D is read.
 * 2 <= K <= 16, 1 <= N, M < 2^31; labels outside 0 .. K-1 belong to no class.  A 16-row tile of such rows does not fit in LDS, so
 * cslgan_ovr_logreg_eval_u8 makes two passes over X: a forward pass (Z = X U, the loss terms, the residuals R = sigmoid(Z) - T
 * [N, 16] into the workspace, the intercept gradient) and a gradient pass (G = X^T R, one partial [256, 16] per workgroup), then a
 * reduction of the partials in index order in double.  Both products run on the exact fp32 matrix instruction with the bytes as
 * the exact floats 0 .. 255 and 1 / 255 applied once to each sum; softplus and sigmoid are the stable forms (finite for every
 * finite z).  All entries validate on the host before any launch, never allocate and never synchronise; no atomics, no memset:
 * two calls on the same inputs return the same bits.  ws: caller workspace of cslgan_ovr_logreg_u8_ws_floats(N, D) floats (0 for
 * sizes the evaluation refuses), 8-byte aligned.  csl_gan_amd.classify.objective_host_bytes is the host model. */
int64_t cslgan_ovr_logreg_u8_ws_floats(int64_t N, int D);
int cslgan_ovr_logreg_eval_u8(const void* X, const int32_t* labels, const float* U, int64_t N, int D, int K, float* loss, float* grad,
                              float* ws, int64_t ws_floats, void* stream);
int cslgan_ovr_logreg_proba_u8(const void* Xtest, const float* U, int64_t M, int D, int K, float* P, void* stream);

/* ---- One-vs-rest MLP on cache bytes (mlp_kernels.hip; csl_gan_amd.tstr --classifier mlp; backward-compatible additions,
 * ABI stays 7).  downstream.py:82's OneVsRestClassifier(MLPClassifier(alpha=1)): class k owns a network with H hidden ReLU units on
 * x_id = byte_id / 255.  U [P, K] row-major, P = (D + 2) H + 1: row d H + h holds W1[d][h], rows D H + h hold b1, rows (D + 1) H + h
 * hold w2, the last row holds b2 — a column of U is one class.  With t_ik = [labels[i] == k] and s = 2 t - 1
 *     Z1_ihk = (sum_d byte_id W1[d][h][k]) / 255 + b1[h][k],     A = max(Z1, 0),     z_ik = sum_h A_ihk w2[h][k] + b2[k]
 *     f_k    = sum_i log(1 + exp(-s_ik z_ik)) + (alpha / 2) (||W1_k||^2 + ||w2_k||^2)                (intercepts unpenalised)
 * which is N times scikit-learn's MLPClassifier loss on a binary target.  With R = sigmoid(z) - T and dZ1 = [Z1 > 0] w2 R (the
 * derivative at exactly 0 is 0):  dW1 = X^T dZ1 + alpha W1,  db1 = sum_i dZ1,  dw2 = sum_i A R + alpha w2,  db2 = sum_i R.
 * X / Xtest: uint8 [N, D] row-major, base 16-byte aligned, 1 <= D <= 65536, rows need not be aligned; no byte beyond X + N D is read.
 * 2 <= K <= 16, 1 <= H <= 128, 1 <= N, M < 2^31; labels outside 0 .. K-1 belong to no class.
 *
 * cslgan_ovr_mlp_eval_u8 — loss[k] = f_k(U), grad [P, K] like U.  A forward pass (Z1 = X W1 tiled 64 x 64 over the H K columns, the
 * logits, the loss terms, dZ1 [N, H K] into the workspace, per-workgroup partials of the loss, dw2, db1, db2), a gradient pass
 * (X^T dZ1, one partial per chunk of rows) and a reduction of all partials in index order in double.  Both products run on the exact
 * fp32 matrix instruction with the bytes as the exact floats 0 .. 255 and 1 / 255 applied once to each sum.  alpha >= 0.  All entries
 * validate on the host before any launch, never allocate and never synchronise; no atomics, no memset: two calls on the same
 * inputs return the same bits.  ws: caller workspace of cslgan_ovr_mlp_u8_ws_floats(N, D, K, H) floats (0 for sizes the evaluation
 * refuses), 8-byte aligned.  cslgan_ovr_mlp_proba_u8 — P[i][k] = sigmoid(z_ik) / sum_k' sigmoid(z_ik') ([M, K] row-major).
 * csl_gan_amd.classify.objective_mlp_host_bytes / proba_mlp_host_bytes are the host model. */
int64_t cslgan_ovr_mlp_u8_ws_floats(int64_t N, int D, int K, int H);
int cslgan_ovr_mlp_eval_u8(const void* X, const int32_t* labels, const float* U, int64_t N, int D, int K, int H, float alpha, float* loss,
                           float* grad, float* ws, void* stream);
int cslgan_ovr_mlp_proba_u8(const void* Xtest, const float* U, int64_t M, int D, int K, int H, float* P, void* stream);

/* ---- naive Bayes on cache bytes (nb_kernels.hip; csl_gan_amd.tstr --classifier gnb / bnb; backward-compatible additions,
 * ABI stays 7).  GaussianNB() and BernoulliNB(alpha=.01) of downstream.py:76-78 on x = byte / 255 are closed forms of per-class,
 * per-feature moments, and on bytes those are integers.  X / Xtest: uint8 [N, D] row-major, base 16-byte aligned, 1 <= D <= 65536, rows
 * need not be aligned; no byte beyond X + N D is read.  2 <= K <= 16, 1 <= N, M < 2^31, 0 <= binarize <= 254.  All entries validate
 * on the host before any launch (null pointers, D, K, N / M, binarize, alignment), never allocate and never synchronise.
 *
 * cslgan_class_moments_u8 — one pass over the N D bytes.  With b = X[i][j] and the sums over the rows i with labels[i] == k (a label
 * outside 0 .. K-1 belongs to no class):  n[k] = the number of rows,  s1[k][j] = sum b,  s2[k][j] = sum b^2,  cnt[k][j] = the number
 * of rows with b > binarize;  int64, [K] and [K, D] row-major, 8-byte aligned.  The result is EXACT — equal to
 * csl_gan_amd.classify.class_moments_host_bytes for every N — and does not depend on scheduling: a workgroup keeps 32-bit partials
 * in LDS for a chunk of at most 2048 rows (sum b^2 <= 2048 * 65025 < 2^28; a 32-bit sum would wrap after 66 051 rows of 255) and adds
 * them to the outputs at the end of its chunk with 64-bit integer vector atomics, whose order cannot change an integer sum.  The
 * outputs are zeroed by the library's own kernel on the stream before that launch, whatever they held.  ws: unused by this form
 * (reserved for a two-stage reduction), may be NULL.
 *
 * cslgan_nb_score_gauss_u8 — S[i][k] = sum_j w[k][j] (b_ij - m[k][j])^2, the subtraction first (the expanded quadratic cancels at
 * small variances and is never formed).  cslgan_nb_score_bern_u8 — S[i][k] = sum_j [b_ij > binarize] delta[k][j].  m, w, delta:
 * fp32 [K, D] row-major; S: fp32 [M, K] row-major, every entry written.  One pass over the M D bytes (16-byte loads), every table
 * element reused over the rows of a tile through LDS.  No atomics: thread-strided partials and a butterfly in a fixed order, so the
 * same inputs return the same bits, and no sum passes through more than s = 275 fp32 additions at any D:
 *     |S - S_float64| <= (s + 3) 2^-24 T <= 2e-5 T,      T[i][k] = the float64 sum of the absolute terms (for gauss S itself).
 * The joint log-likelihoods are c_k - S (gauss) and c_k + S (bern) with the float64 constants c_k added by the caller
 * (csl_gan_amd.classify.NaiveBayes holds the derivation of m, w, delta and c from the moments). */
int cslgan_class_moments_u8(const void* X, const int32_t* labels, int64_t N, int D, int K, int binarize, int64_t* n, int64_t* s1, int64_t* s2,
                            int64_t* cnt, void* ws, void* stream);
int cslgan_nb_score_gauss_u8(const void* Xtest, const float* m, const float* w, int64_t M, int D, int K, float* S, void* stream);
int cslgan_nb_score_bern_u8(const void* Xtest, const float* delta, int64_t M, int D, int K, int binarize, float* S, void* stream);

/* ---- decision trees on cache bytes (tree_kernels.hip; csl_gan_amd.tstr --classifier dt / rf; backward-compatible
 * additions, ABI stays 7).  OneVsRestClassifier(DecisionTreeClassifier()) and (RandomForestClassifier()) of downstream.py:69-74 on the
 * bytes themselves: a threshold is one of 255 byte values and a node's sufficient statistic a 256-bin integer histogram per feature, so
 * the fit is integer-exact.  X / Xtest: uint8 [N, D] row-major, base 16-byte aligned, 1 <= D <= 65536, rows need not be aligned; no
 * byte beyond X + N D is read.  2 <= K <= 16, 1 <= N < 2^24, 1 <= M < 2^31.  Both entries validate on the host before any launch (null
 * pointers, D, K, N / M, S, T, Q, the workspace size, alignment), never allocate and never synchronise.
 *
 * cslgan_tree_best_split_u8 — the split search of one tree level.  rows: int32 [R] row indices into X, grouped into S segments,
 * segment s being rows[seg_off[s] .. seg_off[s + 1]) (seg_off: int32 [S + 1], non-decreasing, within 0 .. R): the rows of one open node
 * of one tree.  Per segment: seg_class[s], the class k whose one-vs-rest targets t_i = [labels[i] == k] the node counts (a label outside
 * 0 .. K-1 is negative for every class); seg_wrow[s], the row of weights (int32 [n_wrows, N], w >= 0) that holds its row weights, or
 * -1 for w = 1 (weights == NULL: w = 1 everywhere, seg_wrow may be NULL); and, when mask_thr != 0, its mask key (seg_tree[s],
 * seg_node[s]).  The weights of a segment's rows must add up to less than 2^31; a row of weight 0 is not there.
 *   With n = sum w, p = sum w t over the segment, a candidate is (feature j, byte v), v in 0 .. 254 present in the segment, with
 * nL = sum w [b_ij <= v] >= 1 and nR = n - nL >= 1; its score is s = fl(pL pL / nL) + fl(pR pR / nR) in float64 — the products exact
 * integers converted once, two IEEE divisions, one addition, nothing fused (computed by the score routine of the boosted stumps below,
 * (a a) / fl(nL) + (c c) / fl(nR) on the converted counts: below 2^32 they convert exactly and both forms round the exact product once —
 * the same bits).  Feature j is a candidate feature iff mask_thr == 0 or
 * word 0 of Philox4x32-10(counter (j, seg_node, seg_tree, 0x74726565), key = seed ^ 0x7472656573706C74) < mask_thr.  The segment's
 * result is the candidate of the largest s, ties to the smallest j, then the smallest v:
 *     out[s] = (j, v, v_hi, nL, pL, n, p)   int32 [S, 7],  v_hi the next larger byte present;   score[s] = the bits of s   int64 [S]
 * and (-1, -1, -1, 0, 0, n, p) with score 0 where no candidate is valid.  Every entry of out and score is written.  EXACT: equal to
 * csl_gan_amd.classify.best_split_host_bytes in every output and in the bits of the score, the same on every call.
 *   A workgroup owns a (segment, tile of 16 features) pair, builds the tile's 256-bin (n, p) histograms in LDS with 64-bit LDS atomics
 * (n in the low half, p in the high half: sum w < 2^31 keeps both from wrapping, one bin may hold it all), scans them and writes one
 * candidate per (segment, tile) into ws; a second kernel reduces the tiles with the tie rule.  No global histogram exists.  The
 * histogram scatter, the scan, the score and the reductions are byte_split.h's, shared with cslgan_boost_stump_u8.
 * ws: cslgan_tree_best_split_ws_bytes(S, D) bytes, 8-byte aligned (0: S < 1, D outside 1 .. 65536, or S ceil(D / 16) >= 2^31 — split the
 * level into several calls then).
 *
 * cslgan_tree_apply_u8 — leaf[t][i], int32 [T, M]: the tree-local number of the leaf that row i of Xtest reaches in tree t.  The T trees
 * are flat tables of Q nodes in all, tree t being the nodes tree_off[t] .. tree_off[t + 1] - 1 (int32 [T + 1]) with its root first:
 * feature[q] (-1: a leaf), threshold[q], child[q] (the tree-local number of the left child; the right one follows it; children lie
 * behind their parent).  A row goes left when its byte <= threshold.  A table that breaks these rules gives leaf -1 for the rows that
 * meet the broken node; nothing outside the tables or Xtest is read.  1 <= T <= 65535. */
int64_t cslgan_tree_best_split_ws_bytes(int64_t S, int D);
int cslgan_tree_best_split_u8(const void* X, const int32_t* labels, const int32_t* weights, int n_wrows, int64_t N, int D, int K, const int32_t* rows,
                              int64_t R, const int32_t* seg_off, const int32_t* seg_class, const int32_t* seg_wrow, const int32_t* seg_tree,
                              const int32_t* seg_node, int64_t S, uint32_t mask_thr, uint64_t seed, int32_t* out, int64_t* score, void* ws,
                              int64_t ws_bytes, void* stream);
int cslgan_tree_apply_u8(const void* Xtest, int64_t M, int D, const int32_t* feature, const int32_t* threshold, const int32_t* child,
                         const int32_t* tree_off, int T, int64_t Q, int32_t* leaf, void* stream);

/* ---- boosted stumps on cache bytes (boost_kernels.hip; csl_gan_amd.tstr --classifier ab; backward-compatible additions,
 * ABI stays 7).  OneVsRestClassifier(AdaBoostClassifier()) of downstream.py:79-80: rounds of depth-1 trees under row weights that are
 * rewritten every round.  The weights are fixed-point integers 0 .. W1 = 2^28, so every sum is an exact integer below 2^52 and the
 * search is the same bits on the host and on a device.
 *
 * cslgan_boost_stump_u8 — the stump search of one round, all K classes over all N rows in one launch.  X: uint8 [N, D] row-major, base
 * 16-byte aligned, rows need not be aligned, no byte beyond X + N D is read; labels: int32 [N], class k counts t_i = [labels[i] == k]
 * (a label outside 0 .. K-1 is negative for every class); weights: int32 [K, N], row k the weights of class k — a weight outside
 * 0 .. 2^28 is clamped into that range, a row of weight 0 is not there.  2 <= K <= 16, 1 <= D <= 65536, 1 <= N < 2^24.
 *   With n = sum w, p = sum w t, a candidate is (feature j, byte v), v in 0 .. 254 present among the rows of weight > 0, with
 * nL = sum w [b_ij <= v] >= 1 and nR = n - nL >= 1; its score is s = (a a) / fl(nL) + (c c) / fl(nR), a = fl(pL), c = fl(p - pL), in
 * float64 — the conversions are exact, each of the five operations is rounded once, nothing is fused.  The largest s wins, ties to the
 * smallest j, then the smallest v:
 *     out[k] = (j, v, v_hi, nL, pL, n, p)   int64 [K, 7],  v_hi the next larger byte present;   score[k] = the bits of s   int64 [K]
 * and (-1, -1, -1, 0, 0, n, p) with score 0 where no candidate is valid.  Every entry of out and score is written.  EXACT: equal to
 * csl_gan_amd.classify.boost_stump_host_bytes in every output and in the bits of the score, the same on every call.
 *   A workgroup owns a (class, tile of 16 features) pair — the K workgroups of a tile are neighbours in the grid — and builds per feature
 * two 256-bin histograms of 64-bit LDS counters, the weights of the negative and of the positive rows: one 64-bit LDS atomic per byte.
 * It scans them and writes one candidate into ws; a second kernel reduces the tiles with the tie rule — the frame and the score routine of
 * cslgan_tree_best_split_u8 (byte_split.h), on 64-bit counts: with every weight 1 a class's result equals that entry's on all rows.
 * ws: cslgan_boost_stump_ws_bytes(K, D) = 64 K ceil(D / 16) bytes, 8-byte aligned (0: K or D out of range).  The entry validates on the
 * host before any launch (null pointers, N, D, K, the workspace size, alignment), never allocates and never synchronises. */
int64_t cslgan_boost_stump_ws_bytes(int K, int D);
int cslgan_boost_stump_u8(const void* X, const int32_t* labels, const int32_t* weights /* [K, N] */, int64_t N, int D, int K,
                          int64_t* out /* [K, 7] */, int64_t* score /* [K] */, void* ws, int64_t ws_bytes, void* stream);

/* ---- Nearest-neighbour audit (nn_kernels.hip; backward-compatible additions, ABI stays 7) -----------------------------------------
 * Exact nearest neighbour of every row of Q [nq, D] among the rows of R [nr, D], both uint8, D = H W C with 1 <= D <= 65536
 * (so 255^2 D < 2^32):
 *     d2(q, r) = sum_i (Q[q][i] - R[r][i])^2                                   an integer in [0, 65025 D]
 *     key(q)   = min over r of (d2(q, r) << 32 | (index_base + r))             as uint64
 * The neighbour's index is the low word of the key and its squared distance the high word; TIES GO TO THE SMALLEST INDEX.  The key
 * is a minimum over a set: it does not depend on tiling, launch order or the number of calls that R is cut into.  The all-ones
 * key means "nothing seen yet"; index_base + nr <= 2^32 - 1 keeps it out of reach.  The device works on a = Q - 128, b = R - 128
 * as int8 (byte ^ 0x80): d2 = |a|^2 + |b|^2 - 2 a.b with |a.b| <= 2^14 D <= 2^30 in the int32 accumulator of the int8 matrix
 * instruction, |a|^2 <= 2^30 in int32, and d2 (up to 4.26e9) formed in uint32 — never int32.  All entries validate on the host
 * before any launch, never allocate and never synchronise.  csl_gan_amd.neighbours.nearest_host is the host model.
 *
 * cslgan_nn_padded_dim — the row pitch Dp of the prepared operands: D rounded up to the kernel's K tile, a multiple of 64
 * (0 for a D outside 1 .. 65536). */
int cslgan_nn_padded_dim(int D);

/* cslgan_nn_prepare_u8 — x: uint8 [rows, D] (16-byte aligned base; D need not be a multiple of 16) becomes xs: int8 [rows, Dp]
 * holding x - 128 with ZERO in bytes D .. Dp-1 of every row (zero in the shifted domain adds nothing to dots or norms), and
 * sqnorm[row] = sum_i (x[row][i] - 128)^2 as int32.  One pass over x; 16-byte aligned loads and stores; no byte beyond
 * x + rows * D is read.  1 <= rows < 2^31, Dp = cslgan_nn_padded_dim(D), xs 16-byte aligned. */
int cslgan_nn_prepare_u8(const void* x, int64_t rows, int D, int Dp, void* xs, int32_t* sqnorm, void* stream);

/* cslgan_nn_min_i8 — best[q] = min(best[q], key(q)) for q < nq over the nr rows of r, by unsigned 64-bit atomicMin: best is IN/OUT
 * and the caller fills it with all-ones once (a torch int64 tensor of -1), then may call any number of times with different
 * blocks of R and their index_base.  q / r: prepared int8 [nq, Dp] / [nr, Dp], qn / rn: their int32 squared norms.  An
 * nq x nr x Dp product on v_mfma_i32_32x32x32_i8 whose nq x nr result never reaches memory: a workgroup owns 128 rows of q and a
 * range of 128-row tiles of r, keeps the running minimum per row in registers and issues one atomicMin per row.  Rows past nq
 * and nr never win, whatever lies behind them.  Dp a multiple of 64 in 64 .. 65536, 1 <= nq, nr < 2^31,
 * 0 <= index_base, index_base + nr <= 2^32 - 1, q / r 16-byte, qn / rn 4-byte and best 8-byte aligned. */
int cslgan_nn_min_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp,
                     int64_t index_base, uint64_t* best, void* stream);

/* cslgan_nn_count_i8 — counts[q][j] += #{r < nr : d2(q, r) <= thresholds[j]} for q < nq, j < n_thr, d2 as above and the compare on
 * UNSIGNED 32-bit values (d2 reaches 4.26e9): the black-box membership scores of csl_gan_amd.blackbox, whose count_within_host is
 * the host model.  q / r / qn / rn / Dp / nq / nr as for cslgan_nn_min_i8.  thresholds: a HOST array of n_thr in 1 .. 4 values in
 * [0, 2^32 - 1], any order, read before the entry returns and passed to the kernel by value.  counts: device uint32 [nq, n_thr],
 * IN/OUT: the caller zeroes it once (no memset here) and may call any number of times with different blocks of R; the sums are
 * integer adds, so they do not depend on tiling, launch order or the number of calls.  A count must stay below 2^32 (2^31 where
 * the caller reads it as int32).  Same tile loop as nn_min with a counting epilogue: a workgroup owns 128 rows of q and at most
 * 127 128-row tiles of r, keeps the n_thr counters of a row as the bytes of one register (<= 2 columns per lane, row and tile, so
 * <= 254 per byte), sums them over the lanes and waves of the row once at the end and issues ONE atomicAdd per (row, threshold)
 * that counted anything.  Columns past nr are masked by their index, never by their data (zero padding has d2 = |a|^2, which a
 * threshold may reach); rows past nq issue nothing.  nr <= 65535 * 127 * 128 per call; counts 4-byte aligned. */
int cslgan_nn_count_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp,
                       const uint32_t* thresholds, int n_thr, uint32_t* counts, void* stream);

/* The k smallest keys and the counts inside per-row radii (csl_gan_amd.manifold: precision / recall / density / coverage; backward-
 * compatible additions, ABI stays 7).  For 1 <= k <= 8, kth(q) is the ascending list of the k smallest keys
 * d2(q, r) << 32 | (index_base + r) of row q over the candidate set {r < nr}, minus — when self_base >= 0 — the ONE column with
 * index_base + r == self_base + q: a row is excluded by its INDEX, never by its distance, so another row with the same bytes
 * stays in, at d2 = 0.  Keys are distinct (they carry the index): ties in d2 are ordered by index and the list is a function of
 * the set alone, not of tiling, launch order, block size or the number of calls.  csl_gan_amd.neighbours.kth_host is the host
 * model.
 *
 * cslgan_nn_kth_workspace_bytes — bytes of workspace that cslgan_nn_kth_i8 needs for these sizes: one list of k keys per row of q
 * and per column range of the launch.  0 for arguments the search would refuse. */
int64_t cslgan_nn_kth_workspace_bytes(int64_t nq, int64_t nr, int k);

/* cslgan_nn_kth_i8 — best: device uint64 [nq, k], IN/OUT: the caller fills it with all-ones once; after a call row q holds the k
 * smallest of (what it held) and (this call's candidates), ascending, all-ones entries last while fewer than k candidates have
 * been seen.  Successive calls must present DISJOINT index ranges (a key met twice would be kept twice).  q / r / qn / rn / Dp /
 * nq / nr / index_base as for cslgan_nn_min_i8; self_base = -1 excludes nothing, else 0 <= self_base, self_base + nq <= 2^32 - 1.
 * Same tile loop as nn_min.  Per row and wave a running bound (the d2 of the wave's k-th key, seeded from best) turns a candidate
 * that cannot enter into one compare; one that can is inserted by the whole wave into the wave's own sorted list of the row in
 * LDS (a ballot, then one uniform loop over its set bits).  No lock, no loop that waits for another wave, no scratch.  After the
 * last tile the two waves of a row merge their lists and the workgroup writes k keys per row to its slice of `workspace`
 * ([column range][nq][k] uint64, written in full: it needs no clearing); a second small kernel folds the slices and best.  Columns
 * past nr and the excluded column never enter a list, whatever bytes lie behind them; rows past nq write nothing.  k in 1 .. 8;
 * best and workspace 8-byte aligned; workspace_bytes >= cslgan_nn_kth_workspace_bytes(nq, nr, k). */
int cslgan_nn_kth_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp,
                     int64_t index_base, int64_t self_base, int k, uint64_t* best, void* workspace, int64_t workspace_bytes, void* stream);

/* cslgan_nn_count_radius_i8 — counts[q] += #{r < nr : d2(q, r) <= radius[r]} for q < nq: the counting epilogue with the threshold
 * of the COLUMN, compared as UNSIGNED 32-bit values and with <= (Kynkaanniemi et al.; the `prdc` package uses <, which differs on
 * exact ties only).  radius: device uint32 [nr], read beside rn; counts: device uint32 [nq], IN/OUT, zeroed by the caller once.
 * One plain uint32 counter per row and lane (no cap on the tiles of a workgroup), summed over the lanes and waves of the row
 * once, ONE atomicAdd per row and workgroup that counted anything.  Columns past nr are masked by their index, whatever radius
 * or bytes lie behind them; rows past nq issue nothing.  csl_gan_amd.manifold.count_within_radii_host is the host model.
 * q / r / qn / rn / Dp / nq / nr as for cslgan_nn_min_i8; radius and counts 4-byte aligned. */
int cslgan_nn_count_radius_i8(const void* q, const int32_t* qn, int64_t nq, const void* r, const int32_t* rn, int64_t nr, int Dp,
                              const uint32_t* radius, uint32_t* counts, void* stream);

/* ---- linear SVC (svm_kernels.hip; csl_gan_amd.svm and csl_gan_amd.tstr_svm; backward-compatible additions, ABI stays 7).
 * OneVsRestClassifier(SVC(kernel='linear', probability=True)) of downstream.py:67 on byte rows, x = byte / 255: the kernel matrix is
 *     K_ij = <b_i, b_j> / 65025,   <b_i, b_j> = (s_i + s_j - d2_ij) / 2   an exact integer below 2^53,
 * s the squared norms of the BYTE rows (int64; not the norms of the shifted rows that nn_prepare_u8 leaves) and d2 the squared distance.
 *
 * cslgan_gram_d2_u8 — the stored matrix.  xs / sqnorm: the prepared rows [n, Dp] and norms of cslgan_nn_prepare_u8, taken against
 * themselves by the tile loop of the nearest-neighbour kernels (nn_tile.h).  out: uint32 [n, pitch], 128-byte aligned, pitch a multiple
 * of 32 with n <= pitch <= 65536, so every row starts on 128 bytes and is written in whole 128-byte stores; out[i, j] = d2(i, j) for
 * j < n, the columns n .. pitch - 1 are written with values that mean nothing.  1 <= n <= 65536 (a 16 GiB matrix): a larger set is
 * refused with a message that says so.  EXACT.
 *
 * cslgan_svc_smo_f64 — LIBSVM's SMO on n_problems <= 96 dual problems over the same n rows, one workgroup per problem:
 *     minimise 1/2 a'Qa - e'a,  0 <= a <= C,  y'a = 0 over the rows of active[p],  Q_ij = y_i y_j K_ij
 * with y: int8 [P, n] of +1 / -1 and active: uint8 [P, n].  State per problem, kept in global memory between calls: alpha and grad
 * (float64 [P, n]; the caller starts them at 0 and -1), iters (int64 [P], from 0) and done (int32 [P], from 0).  A call runs at most
 * `chunk` iterations per problem and never past max_iter in total; it leaves done[p] = 1 where m(a) - M(a) < tol or no pair is left, and
 * a problem that is done is not touched again.  The caller repeats the call until every problem is done or at max_iter.
 *   One iteration: i = argmax of -y G over I_up; j = argmin of -b^2 / a over the rows of I_low with b = m + y G > 0, a = K_ii + K_jj -
 * 2 K_ij (TAU = 1e-12 where a <= 0), second-order selection of Fan, Chen and Lin; LIBSVM's clipped two-variable update; G += (Q_i da_i)
 * + (Q_j da_j) over ALL rows, the inactive ones included (so y_t (G_t + 1) is the held-out decision value of row t).  Both selections
 * resolve ties to the lowest row index.  Every operation is a single IEEE float64 operation in the order of csl_gan_amd.svm.smo_host
 * (no fused multiply-add, IEEE division): alpha, grad and iters equal the host's bit for bit, whatever `chunk` is.
 * 2 <= n <= 65536; d2 / pitch as written by cslgan_gram_d2_u8; C and tol finite and > 0; chunk >= 1; max_iter >= 0.
 * Both entries validate on the host before any launch (null pointers, n, Dp, pitch, the problem count, alignment), never allocate and
 * never synchronise. */
int cslgan_gram_d2_u8(const void* xs, const int32_t* sqnorm, int64_t n, int Dp, uint32_t* out /* [n, pitch] */, int64_t pitch, void* stream);
int cslgan_svc_smo_f64(const uint32_t* d2 /* [n, pitch] */, int64_t pitch, const int64_t* s /* [n] */, int64_t n, const int8_t* y /* [P, n] */,
                       const uint8_t* active /* [P, n] */, int n_problems, double C, double tol, int64_t chunk, int64_t max_iter,
                       double* alpha /* [P, n] */, double* grad /* [P, n] */, int64_t* iters /* [P] */, int32_t* done /* [P] */, void* stream);

/* ---- Sliced Wasserstein audit (swd_kernels.hip; csl_gan_amd.sliced and csl_gan_amd.swd; backward-compatible additions,
 * ABI stays 7).  Two sets A [Na, D] and B [Nb, D] of uint8 rows, D = H W C with 1 <= D <= 65536, and P directions s_p in {-1, +1}^D:
 *     y_p(x)  = sum_j s_p[j] (x[j] - 128)                                      an integer, |y| <= 128 D <= 2^23
 *     num_p   = sum_i sum_j |a[i] - b[j]| * |[i Nb, (i + 1) Nb) n [j Na, (j + 1) Na)|     a, b: the ascending sorted y_p of A and B
 *     W1_p    = num_p / (Na Nb)                                                the exact 1-D Wasserstein-1 distance, quantile form
 * and the sliced distance is the mean of W1_p over p divided by sqrt(D), the norm of EVERY direction.  Every num_p is an exact int64
 * (Na Nb 2^25 < 2^63 is required) and does not depend on tiling, blocking or the device; csl_gan_amd.sliced holds the host models.
 *
 * The direction stream: one Philox4x32-10 call gives the 128 signs of the columns 128 b .. 128 b + 127 of direction p, counter
 * (b, p, 0, 0x73776464 "swdd"), key = seed ^ 0x7377647369676E73 ("swdsigns": low word k0, high word k1).  Bit t of the 128 is bit
 * t & 31 of output word t >> 5: set is +1, clear is -1.  A direction depends on (seed, p, column) only.
 *
 * cslgan_swd_directions_i8 — dirs: int8 [P, Dp], Dp = cslgan_nn_padded_dim(D), 16-byte aligned: +1 / -1 in the columns < D and ZERO in
 * D .. Dp - 1, the shape of the prepared operands of cslgan_nn_prepare_u8.  1 <= P < 2^31. */
int cslgan_swd_directions_i8(uint64_t seed, int64_t P, int D, int Dp, void* dirs, void* stream);

/* cslgan_swd_project_i8 — Y[p, col0 + i] = dirs[p] . xs[i] as int32 for p < P, i < n.  dirs: int8 [P, Dp] as above; xs: a prepared block
 * of cslgan_nn_prepare_u8 with n rows (its norms are not needed); Y: int32 [P, ldy] row-major, so the projections of one direction are
 * contiguous; col0 lets a walk over blocks of a set fill one matrix.  The P x n x Dp product on v_mfma_i32_32x32x32_i8 through the tile
 * loop of the nearest-neighbour kernels (nn_tile.h), directions as the row operand, with an epilogue that stores the accumulator: every
 * element of Y[:, col0 .. col0 + n) has exactly one writer and nothing else of Y is touched.  1 <= P, n < 2^31, ldy >= col0 + n, Dp a
 * multiple of 64 in 64 .. 65536, dirs / xs 16-byte and Y 4-byte aligned. */
int cslgan_swd_project_i8(const void* dirs, int64_t P, const void* xs, int64_t n, int Dp, int32_t* Y /* [P, ldy] */, int64_t ldy, int64_t col0,
                          void* stream);

/* cslgan_sort_rows_i32 — the first n entries of every row of x: int32 [P, ld] are sorted ascending as SIGNED values, in place; the
 * entries n .. ld - 1 are neither read nor written.  Keys only, so the result is unique.  An LSD radix sort segmented by row: the key is
 * value + 2^(key_bits - 1) as uint32 — with key_bits = 32 the flipped sign bit; with fewer bits every value must lie in
 * [-2^(key_bits - 1), 2^(key_bits - 1)), and ceil(key_bits / 8) passes run (the sliced distance needs 25).  A pass is three launches
 * — histogram per (row, tile of 4096, digit) in LDS, exclusive scan per row, stable scatter — between x and a workspace of the same
 * size; no kernel waits for another workgroup.  workspace: 16-byte aligned, at least cslgan_sort_rows_ws_bytes(P, n) bytes (0 for
 * sizes that the sort refuses); nothing of it needs clearing.  1 <= P, n < 2^31, P ceil(n / 4096) < 2^31, ld >= n. */
int64_t cslgan_sort_rows_ws_bytes(int64_t P, int64_t n);
int cslgan_sort_rows_i32(int32_t* x /* [P, ld] */, int64_t P, int64_t n, int64_t ld, int key_bits, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* cslgan_swd_w1_i64 — num[p] = num_p as above from the SORTED rows a: int32 [P, lda] (Na entries each) and b: int32 [P, ldb] (Nb entries).
 * One workgroup per direction walks the longer row; products and sums in int64, reduced over the lanes and waves of the workgroup,
 * one plain 8-byte store per direction, no atomics: exact and order-free.  Refused when Na Nb 2^25 >= 2^63 (values within +-2^24
 * then cannot overflow the sum).  1 <= P, Na, Nb < 2^31, lda >= Na, ldb >= Nb, a / b 4-byte and num 8-byte aligned.
 * All entries of this section validate on the host before any launch, never allocate and never synchronise. */
int cslgan_swd_w1_i64(const int32_t* a, int64_t lda, int64_t Na, const int32_t* b, int64_t ldb, int64_t Nb, int64_t P, int64_t* num /* [P] */,
                      void* stream);

/* ---- Byte moments (moment_kernels.hip; csl_gan_amd.moments and csl_gan_amd.frechet; backward-compatible additions, ABI
 * stays 7).  A set of N uint8 rows of D = H W C bytes, 1 <= D <= 65536, and y = x - 128, the shift of cslgan_nn_prepare_u8:
 *     s1[j]    = sum_n y[n][j]                     int64, |s1| <= N 2^7
 *     s2[i][j] = sum_n y[n][i] y[n][j]             int64, |s2| <= N 2^14
 *     M        = N s2 - s1 (x) s1                  an exact int64 on the host for N < 2^24 (N^2 2^14 < 2^62)
 *     C        = M / (N (N - 1))                   the unbiased covariance, float64 on the host
 * and the Frechet distance of two sets is |dmu|^2 + tr CA + tr CB - 2 tr (CA^1/2 CB CA^1/2)^1/2 from these integers, on the host in
 * float64 whoever computed them.  s1 and s2 are exact and do not depend on tiling, blocking, chunking or the device;
 * csl_gan_amd.moments.byte_moments_host is the host model.  A set is walked in chunks of at most 65536 rows: the Gram product sums over
 * the rows of the chunk in an int32 accumulator, |acc| <= 65536 * 2^14 = 2^30 < 2^31, and adds it to the int64 matrix.
 *
 * cslgan_mom_transpose_u8 — the transposed operand image of a chunk.  x: uint8 [n, D], 1 <= n <= 65536, any D in range, no alignment
 * asked of x.  xt: int8 [D, np], np = n rounded up to 64, 16-byte aligned: xt[j][i] = x[i][j] - 128 for i < n and ZERO in the columns
 * n .. np - 1, which therefore add nothing to a sum.  Rows of xt are K-contiguous, the shape the tile loop of nn_tile.h wants.  No byte
 * beyond x + n D is read and nothing outside [D, np] is written. */
int cslgan_mom_transpose_u8(const void* x, int64_t n, int D, int64_t np, void* xt /* [D, np] */, void* stream);

/* cslgan_mom_colsum_i64 — s1[j] += sum_i xt[j][i] for j < D.  s1: int64 [D], in/out, zeroed by the caller once.  ONE WRITER PER COLUMN:
 * one wave sums a row of xt and its first lane adds the total by a plain 8-byte load / add / store; no atomics.  np a multiple of 64
 * in 64 .. 65536, xt 16-byte and s1 8-byte aligned. */
int cslgan_mom_colsum_i64(const void* xt, int D, int64_t np, int64_t* s1 /* [D] */, void* stream);

/* cslgan_mom_gram_i64 — S2[i][j] += xt[i] . xt[j] for every element of the 128 x 128 tiles ON AND BELOW the diagonal (tile row
 * i / 128 >= tile column j / 128; a diagonal tile is written whole).  S2: int64 [D, ld] row-major, ld >= D, in/out, zeroed by the caller
 * once; successive calls add further chunks of rows.  The D x D x np product on v_mfma_i32_32x32x32_i8 through the tile loop of
 * nn_tile.h with xt as BOTH operands; the epilogue adds the int32 accumulator by a plain 8-byte load / add / store: every element has one
 * writer per launch and the launches of one stream are ordered.  THE TILES STRICTLY ABOVE THE DIAGONAL, and the columns D .. ld - 1,
 * ARE NEITHER READ NOR WRITTEN; cslgan_mom_mirror_i64 fills them once at the end.
 *
 * cslgan_mom_mirror_i64 — S2[i][j] = S2[j][i] for every element of the tiles strictly above the diagonal; nothing else is written.
 * All entries of this section validate on the host before any launch, never allocate and never synchronise. */
int cslgan_mom_gram_i64(const void* xt, int D, int64_t np, int64_t* S2 /* [D, ld] */, int64_t ld, void* stream);
int cslgan_mom_mirror_i64(int64_t* S2 /* [D, ld] */, int D, int64_t ld, void* stream);

/* ---- Kernel two-sample test (mmd_kernels.hip; csl_gan_amd.kernel_test and csl_gan_amd.mmd; backward-compatible
 * additions, ABI stays 7).  Z: n synthetic rows followed by m real rows, N = n + m <= 65536, and d2 the stored matrix of
 * cslgan_gram_d2_u8 over Z.  med: the lower median of the entries above the diagonal, an integer; bandwidth b has den_b = 2 med c_b.  The
 * host builds two float64 tables per bandwidth, hi_b[h] = exp(-65536 h / den_b) and lo_b[l] = exp(-l / den_b), 65536 entries each, and
 *     Kq[i][j] = sum_b rint(2^28 (hi_b[d2 >> 16] lo_b[d2 & 65535]))   for i != j,     Kq[i][i] = 0:
 * one IEEE float64 product, one exact scaling, round-half-even, then integers: no transcendental and no fused operation on either path,
 * so Kq is the same bit for bit on the host and the device; Kq < 2^31 for B <= 7.  For a partition p, member[p][j] != 0 marking its
 * first side,
 *     r[i][p] = sum_j Kq[i][j] member[p][j],   sxx2[p] = sum_{i in p} r[i][p],   sxy[p] = sum_{i not in p} r[i][p]
 * are exact int64 (N (N - 1) 2^31 < 2^63), and the unbiased MMD^2 of every relabelling follows from them and the total of Kq on the host
 * in Python integers.  csl_gan_amd.kernel_test holds the host model of every entry.  All three validate on the host before any launch,
 * never allocate and never synchronise; d2 / kq: 128-byte aligned, pitch a multiple of 32 in n .. 65536, 1 <= n <= 65536.
 *
 * cslgan_tri_hist_u32 — hist[v] += the number of entries d2[i][j], i < j < n, whose top prefix_bits (0, 8, 16 or 24) bits equal those
 * of `prefix` and whose next 8 bits are v.  hist: int64 [256], in/out, zeroed by the caller.  Four calls are an exact radix select of
 * any rank.  Nothing on or below the diagonal and nothing in the columns n .. pitch - 1 is counted. */
int cslgan_tri_hist_u32(const uint32_t* d2, int64_t pitch, int64_t n, uint32_t prefix, int prefix_bits, int64_t* hist /* [256] */, void* stream);

/* cslgan_mmd_kernel_u32 — rewrites d2 in place as Kq: both triangles, zero on the diagonal.  hi, lo: float64 [B, 65536], 1 <= B <= 7.
 * The columns n .. pitch - 1 hold anything afterwards. */
int cslgan_mmd_kernel_u32(uint32_t* d2, int64_t pitch, int64_t n, const double* hi, const double* lo, int B, void* stream);

/* cslgan_mmd_partition_sums_i64 — sxx2[p] += sum_{i : member[p][i] != 0} r[i][p] and sxy[p] += sum_{i : member[p][i] == 0} r[i][p] over
 * the rows i < n, for p < P.  kq: ANY uint32 matrix with entries below 2^31, not necessarily symmetric, its diagonal as stored.  member:
 * int8 [P, ldm], 16-byte aligned, ldm a multiple of 64 in n .. 65536; the columns n .. of member and of kq are not used.  sxx2, sxy:
 * int64 [P], in/out, zeroed by the caller; 1 <= P <= 2^20.  The n x P x n product runs on v_mfma_i32_32x32x32_i8: the four bytes of an
 * entry, each minus 128, are four int8 limb planes (the A operand, cut while a stage is written to LDS) against member (the B operand,
 * K-contiguous as stored), int32 accumulators per limb (|acc| <= 2^30), recombined to int64 once per 64-row tile with the correction
 * 0x80808080 sum_j member[p][j]; the results leave by 64-bit integer atomic adds, exact and so independent of their order. */
int cslgan_mmd_partition_sums_i64(const uint32_t* kq, int64_t pitch, int64_t n, const int8_t* member /* [P, ldm] */, int64_t ldm, int64_t P,
                                  int64_t* sxx2 /* [P] */, int64_t* sxy /* [P] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CSLGAN_H */
