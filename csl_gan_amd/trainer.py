"""The training step functions of the reference's train.py as methods of one object.

The reference keeps these as closures over script globals (train.py:95-546); here `Trainer` owns
opt / G / D / optimizers / privacy_engine / logger / mean_sampler and exposes the same function
names with the same argument meaning: setup_privacy_engine, gen_z, gen_y, eval_G_D,
get_penalty_data, update_adaptive_clipping_params, update_grad_logging, calc_d_fake_loss,
calc_d_real_loss, train_D, train_G, train.

MI355X-first host changes (results identical):
  * per-step statistics stay on the device and are folded into the Logger only when a line is
    printed — the reference forces >= 8 device->host syncs per D-step (train.py:233-238, 315, 328,
    488-493); this path forces none outside log/gating iterations;
  * grad-norm logging reuses the norms/factors the clip kernels already produced instead of
    recomputing them (train.py:397 duplicates train.py:399's norm pass);
  * the generator forward for fakes runs under no_grad when G is frozen (train.py:362).
"""
from __future__ import annotations

import contextlib
import gc
import inspect
import os
import warnings

import numpy as np
import torch
from torch import autograd

from . import distributed as Dist
from . import engine as E
from . import functional as HF
from . import nn as hnn
from . import ops
from . import util
from .backprop_clip import BackpropClipper
from .gradient_penalty import calc_penalty
from .is_engine import ISPrivacyEngine
from .logger import Logger


class Trainer:
    def __init__(self, opt, G, D, dataset=None, public_dataloader=None, public_dataset=None, mean_sampler=None,
                 log_to=None, world_size=1, rank=0, grad_reducer=None):
        self.opt, self.G, self.D = opt, G, D
        if any(p.is_cuda for p in D.parameters()):
            ops.set_compute_dtype(getattr(opt, "compute_dtype", "fp32"))     # process-wide: one process drives one run
            ops.set_storage_dtype(getattr(opt, "storage_dtype", "fp32"))
        self.dataset, self.public_dataloader, self.public_dataset = dataset, public_dataloader, public_dataset
        self.mean_sampler = mean_sampler
        self.world_size, self.rank, self.grad_reducer = world_size, rank, grad_reducer
        self.privacy_engine = None
        self.prop_grad_clipper = None      # BackpropClipper, created by setup_backprop_clip when --backprop_clip is set
        self.g_optimizer, self.d_optimizer = self.init_optimizers()
        self.logger = self._make_logger(log_to)
        self.dev_stats = {}
        self._pending_stats = []
        self.batches_per_epoch = opt.train_set_size / opt.batch_size
        self.fixed_z = self.fixed_y = None  # set by init_fixed_samples (train.py:256-261); sample() is a no-op until then
        self.graphed = None                # GraphedDStep, created by setup_privacy_engine when --hip_graph is set
        self.last = {}                     # observables of the most recent D-step (device tensors), for tests
        self.explicit = {}                 # optional explicit random inputs (alpha / noise / mean-sample batches) for parity tests
        self._fused_buf = None             # the fused critic batch (_fused_batch)
        self._g_out_kw = None              # whether G.forward takes out= (_g_takes_out)
        self._g_flat = None                # the flat bucket of G's gradients (_average_G_grads)
        self._stat_bufs = {}               # persistent statistic buffers whose rows dev_stats holds (_stat_rows)
        self._gp_stream = None             # the penalty's side stream (_launch_penalty)
        self._pending_penalty = None       # (penalty, grads) launched on it and not yet joined
        self._gp_joined = False            # joined early, at a segment boundary
        self._warn_ps_pen = True           # the per-sample-penalty warning has not been printed yet

    # ---- train.py:75-77 -----------------------------------------------------------------------
    def init_optimizers(self):
        o = self.opt
        return (E.HipAdam(self.G.parameters(), lr=o.g_lr, betas=(o.adam_b1, o.adam_b2)),
                E.HipAdam(self.D.parameters(), lr=o.d_lr, betas=(o.adam_b1, o.adam_b2), weight_decay=o.weight_decay))

    # ---- train.py:84-92 -----------------------------------------------------------------------
    def setup_backprop_clip(self):
        """Experimental in the reference (options.py:243-244).  Hangs the per-layer input / output-gradient clips on D and turns the
        analytic per-sample gradient bounds into the engine's per-layer clip norms (x batch_size: the losses are batch means)."""
        o = self.opt
        if not o.backprop_clip:
            return None
        with torch.no_grad():
            p = ((o.bpc_back_clip_param_pl, o.bpc_forward_clip_param_pl) if o.grad_clip_mode[-3:] == "-pl"
                 else (o.bpc_back_clip_param, o.bpc_forward_clip_param))
            self.prop_grad_clipper = BackpropClipper(self.D, *p, o.bpc_auto_activation_scale, o.bpc_auto_weight_grad_scale, device=o.d_device)
            clip_params = [c * o.batch_size for c in self.prop_grad_clipper.grad_l2_bounds]
            o.clipping_param_per_layer = clip_params
            o.clipping_param = np.linalg.norm(clip_params, ord=2)
        return self.prop_grad_clipper

    # ---- train.py:95-138 ----------------------------------------------------------------------
    def setup_privacy_engine(self):
        o = self.opt
        if o.backprop_clip and self.prop_grad_clipper is None:
            self.setup_backprop_clip()
        params = dict(batch_size=o.batch_size, sample_size=o.train_set_size,
                      alphas=[1 + x / 10.0 for x in range(1, 100)] + list(range(12, 400)), noise_multiplier=o.sigma,
                      world_size=self.world_size)
        if o.dp_mode == "gc":
            if o.clipping_param_per_layer is None:
                o.clipping_param_per_layer = [1 for _ in self.D.parameters()]
            per_layer = o.grad_clip_mode.endswith("-pl")
            pe = E.PrivacyEngine(self.D, **params, accum_passes=not o.grad_clip_split,
                                 num_private_passes=1 if o.grad_clip_split else None, auto_clip_and_accum_on_step=False,
                                 max_grad_norm=list(o.clipping_param_per_layer) if per_layer else o.clipping_param,
                                 materialize=getattr(o, "materialize", "private"),
                                 grad_sample_dtype=getattr(o, "grad_sample_dtype", "fp32"))
            pe.disable_hooks()
        elif o.dp_mode == "is":
            pe = ISPrivacyEngine(self.D, **params, per_param=o.imm_sens_per_param,
                                 scaling_vec=None if o.imm_sens_scaling_mode == "standard" else o.imm_sens_scaling_vec)
        else:
            raise NotImplementedError("dp_mode=%s: the trimmed-mean / smooth-vote engines are experimental in the reference "
                                      "(README.md:11) and out of scope" % o.dp_mode)
        pe.grad_reducer = self.grad_reducer
        pe.attach(self.d_optimizer)
        pe._set_seed(o.manual_seed + 7919 * self.rank)
        self.privacy_engine = pe
        # Recorded: gc, and immediate sensitivity except moving-avg-pl (its host reads gradient norms inside the step); never with
        # --backprop_clip.  One rank records the whole step.  N > 1 ranks record it as SEGMENTS — the capture ends at each collective
        # (the flat gradient all-reduce, the 9-float adaptive statistics, the immediate-sensitivity maxima), which is issued eagerly
        # between the replays of the graphs on either side (GraphedDStep._capture_segments); with CSLGAN_GRAPH_DIST=1 over RCCL the
        # collectives are stream-ordered launches and are recorded with the step, whole.  N > 1 with CSLGAN_GRAPH_SEGMENTS=0 and
        # collectives that are not recorded steps eagerly.
        # (Replayed fills: the library never uses hipMemsetAsync, whose graph node replays wrongly — csrc/common.h zero_floats.)
        if (getattr(o, "hip_graph", False) and (self.world_size == 1 or Dist.collectives_capturable() or Dist.segments_enabled()) and not o.backprop_clip
                and (o.dp_mode == "gc" or (o.dp_mode == "is" and o.imm_sens_scaling_mode != "moving-avg-pl"))):
            self.graphed = GraphedDStep(self)
        return pe

    # ---- train.py:150-161 ---------------------------------------------------------------------
    def gen_z(self, size):
        return torch.empty((size, self.opt.g_latent_dim), device=self.opt.g_device).normal_(0.0, 1.0)

    def gen_y(self, size):
        o = self.opt
        if not o.conditional:
            return None
        if o.n_classes < 3:
            p1 = 0.5
            if o.dataset == "CelebA" and self.dataset is not None and hasattr(self.dataset, "label_true_count"):
                p1 = self.dataset.label_true_count / o.train_set_size
            return (torch.empty(size).random_(0, 2) < p1).long()
        return torch.empty(size).random_(0, o.n_classes).long()

    # ---- train.py:163-184 ---------------------------------------------------------------------
    def eval_G_D(self, z, y=None, g_kwarg={}, d_kwarg={}):
        """G then D.  (The reference's micro-batch G/D software pipeline for split devices,
        train.py:168-184, is dead at its defaults and calls torch.cat on a generator; not carried.)"""
        o = self.opt
        yg = None if y is None else y.to(o.g_device)
        frozen = not any(p.requires_grad for p in self.G.parameters())
        with torch.no_grad() if frozen else contextlib.nullcontext():
            img = self.G(z, yg, **g_kwarg)
        img = img.to(o.d_device)
        d_out, d_aux = self.D(img, None if y is None else y.to(o.d_device), **d_kwarg)
        return d_out, d_aux, img

    # ---- train.py:186-202 ---------------------------------------------------------------------
    def get_penalty_data(self, data_in, labels_in):
        o = self.opt
        data, labels = data_in, labels_in
        n = data_in.size(0)
        if "pen_real" in self.explicit:
            return self.explicit["pen_real"].to(o.d_device), labels_in
        if o.penalty_use_public_data:
            if o.public_set_size > 0:
                if labels_in is None:
                    reps = (n - 1) // o.batch_size + 1
                    data = torch.cat([next(iter(self.public_dataloader))[0] for _ in range(reps)], dim=0)[:n]
                else:
                    pairs = [self.public_dataset.get_item_with_label(l) for l in labels_in]
                    data = torch.stack([p[0] for p in pairs])
                    labels = torch.tensor([p[1] for p in pairs])
            elif o.num_mean_samples > 0:
                data, labels = self.mean_sampler.sample(n, requested_labels=labels_in)
        return data.to(o.d_device), None if labels is None else labels.to(o.d_device)

    # ---- train.py:204-245 ---------------------------------------------------------------------
    def update_adaptive_clipping_params(self):
        o, D, pe = self.opt, self.D, self.privacy_engine
        util.zero_grad(D)
        img, labels = self._adaptive_batch()
        if "ms_adapt" not in self.explicit and o.public_set_size > 0:      # the public loader's batch: this pass keeps its own copy
            img, labels = img.clone(), (None if labels is None else labels.clone())
        img = img.to(o.d_device)
        labels = None if labels is None else labels.to(o.d_device)
        if o.grad_clip_split:
            d_fake_loss = d_fake_aux_loss = 0
        else:
            z = self.explicit["z_adapt"] if "z_adapt" in self.explicit else self.gen_z(o.batch_size)
            _, _, d_fake_loss, d_fake_aux_loss, _ = self.calc_d_fake_loss(img, labels, z, labels)
        _, _, d_real_loss, d_real_aux_loss = self.calc_d_real_loss(img, labels)
        pe.norms_only = pe.lean      # this pass only feeds the per-sample norms below
        try:
            (d_real_loss + d_fake_loss + d_real_aux_loss + d_fake_aux_loss).backward()
        finally:
            pe.norms_only = False
        with torch.no_grad():
            B = img.size(0)
            # per-layer per-sample norms of pass 0: produced by the wgrad epilogue, never re-read from HBM
            self._set_adaptive_clip_norm(pe.sample_sqnorms()[:, :B].sqrt())
        self.d_optimizer.zero_grad()

    def _adaptive_batch(self):
        """The batch the adaptive clip norm is estimated on (train.py:206-212): an explicit one, else the public loader's next batch,
        else mean samples."""
        o = self.opt
        if "ms_adapt" in self.explicit:
            return self.explicit["ms_adapt"], self.explicit.get("ms_adapt_labels")
        if o.public_set_size > 0:
            img, labels = next(iter(self.public_dataloader))
            return img, (labels if o.conditional else None)
        return self.mean_sampler.sample(o.batch_size)

    def _adaptive_clip_norm(self, r):
        """train.py:233-243: the statistic r [n_params] times adaptive_scalar per layer, or its 2-norm times adaptive_scalar flat."""
        o = self.opt
        return r * o.adaptive_scalar if o.use_grad_clip_per_layer else (r.norm(2) * o.adaptive_scalar).reshape(1)

    def _set_adaptive_clip_norm(self, norms, join_penalty=False):
        """train.py:225-243 on the device: per-sample norms [n_params, B] -> their mean or max per layer -> the engine's clip norm.
        join_penalty: the fused pass has work on the penalty stream, which a segment boundary at the collective must join first."""
        o = self.opt
        r = norms.mean(dim=1) if o.adaptive_stat == "mean" else norms.max(dim=1).values
        if self.world_size > 1:            # every rank must clip and noise with the same C
            if join_penalty:
                self._join_penalty_stream_at_boundary()
            r = Dist.average_across_ranks(r.contiguous(), use_max=o.adaptive_stat == "max")
        self.last["adaptive_stats"] = r
        self.privacy_engine.set_max_grad_norm_device(self._adaptive_clip_norm(r))

    # ---- train.py:310-329 ---------------------------------------------------------------------
    def update_grad_logging(self):
        """Uses the norms / factors of the clip that just ran (same numbers the reference recomputes)."""
        o, pe = self.opt, self.privacy_engine
        B = o.batch_size
        per_layer = pe.clipper.norm_clipper.is_per_layer
        keep = bool(self.explicit.get("keep"))
        C = pe.max_grad_norm_device()
        if o.grad_clip_split:
            sq, f = pe.last_sq, pe.last_factors
            col = 1 if sq.shape[1] >= 2 * B else 0
        else:
            # the reference logs column 0 = the first (generated-data) pass when passes are accumulated
            # (train.py:315); those norms come from the wgrad epilogue, the factors from the same formula
            sq, f, col = pe.sample_sqnorms()[:, :B], None, 0
        one_launch = o.grad_clip_split and sq.is_cuda and sq.dtype == torch.float32 and sq.is_contiguous()
        if one_launch:
            # mean / std / max of the logged column's norms, the clip norms and the clipped fraction in ONE launch, added in place
            rows = sq.shape[0] if per_layer else 1
            ops.grad_log_stats(sq, col * B, B, C, per_layer, E.CLIP_EPS, self._stat_rows(self._GLOG_NAMES, (5, rows), sq.device))
            if not keep:
                return
        norms = sq.sqrt() if per_layer else sq.sum(dim=0, keepdim=True).sqrt()
        if f is None:
            f = (C.reshape(-1, 1) / (norms + E.CLIP_EPS)).clamp(max=1.0)
        if not one_launch:
            nm = norms[:, col * B:(col + 1) * B]
            fac = (f if per_layer else f.reshape(1, -1))[:, col * B:(col + 1) * B]
            self._acc("D Layer Grad Norm Means", nm.mean(dim=1))
            self._acc("D Layer Grad Norm Stds", nm.std(dim=1, unbiased=False))
            self._acc("D Layer Grad Norm Maxes", nm.max(dim=1).values)
            self._acc("Clipping Params", C.clone())
            self._acc("Grads Clipped", (fac < 0.999).float().mean(dim=1))
        self.last.update(norms=norms, clip_factors=f, clip_params=C.clone())

    # ---- train.py:247-249 ---------------------------------------------------------------------
    def update_sens_moving_avg(self):
        """--imm_sens_scaling_mode moving-avg-pl: scaling_vec <- beta * scaling_vec + (1 - beta) * ||p.grad||_2 per tensor.
        The reference reads opt.moving_avg_beta, which options.py never defines (train.py:249 raises AttributeError), so the
        mode cannot run there; here --moving_avg_beta (a build extension) supplies it and its absence is reported as such."""
        o, pe = self.opt, self.privacy_engine
        beta = getattr(o, "moving_avg_beta", None)
        if beta is None:
            raise AttributeError("imm_sens_scaling_mode=moving-avg-pl needs opt.moving_avg_beta, which the reference's options.py "
                                 "never defines (train.py:249 fails the same way); pass --moving_avg_beta")
        vec = pe.scaling_vec
        norms = [0.0 if p.grad is None else float(p.grad.reshape(-1).norm(2)) for p in self.D.parameters()]
        pe.set_scaling_vec([vec[i] * beta + n * (1 - beta) for i, n in enumerate(norms)])

    def update_is_logging(self):
        """train.py:332-338 without the per-step host read: the mean accumulates on the device, the running minimum / maximum of
        the interval too; flush_stats folds them into the Logger with the reference's conventions (values scaled by the logging
        interval because the Logger divides by it; _fold_is_extrema)."""
        pe = self.privacy_engine
        s = getattr(pe, "batch_sensitivity_device", None)
        if s is None:                      # a foreign engine without the device view: the reference's host arithmetic
            self.logger.stats["IS Mean"] += pe.batch_sensitivity
            self._fold_is_extrema(pe.batch_sensitivity, pe.batch_sensitivity)
            return
        s = s.detach().reshape(-1)
        self._acc("IS Mean", s.clone() if self.opt.imm_sens_per_param else s.reshape(()).clone())
        # running extrema of the logging interval in PERSISTENT buffers updated in place (a replayed step keeps updating the same
        # memory); +-inf marks "nothing seen since the last flush"
        for key, op, init in self._IS_EXTREMA:
            cur = self.dev_stats.get(key)
            if cur is None or cur.shape != s.shape:
                cur = self.dev_stats[key] = torch.full_like(s, init)
            op(cur, s, out=cur)

    _IS_EXTREMA = (("_is_min", torch.minimum, float("inf")), ("_is_max", torch.maximum, float("-inf")))

    def _fold_is_extrema(self, mn, mx):
        """train.py:334-338: a (min, max) pair of sensitivities, floats or per-parameter arrays, into the Logger.  Values are scaled
        by the logging interval because the Logger divides by it; a minimum the Logger has reset to 0.0 restarts from the reference's
        large constant (a float) or from the incoming array (per parameter)."""
        lg = self.logger
        mn, mx = mn * lg.interval, mx * lg.interval
        if self.opt.imm_sens_per_param:
            lg.stats["IS Min"] = mn if isinstance(lg.stats["IS Min"], float) else np.minimum(lg.stats["IS Min"], mn)
            lg.stats["IS Max"] = np.maximum(lg.stats["IS Max"], mx)
        else:
            lg.stats["IS Min"] = min(99999 if lg.stats["IS Min"] < 1e-8 else lg.stats["IS Min"], mn)
            lg.stats["IS Max"] = max(lg.stats["IS Max"], mx)

    def _flush_is_extrema(self):
        """The device-side extrema of the interval into the Logger; the buffers go back to "nothing seen"."""
        mn, mx = (self.dev_stats.get(key) for key, _, _ in self._IS_EXTREMA)
        if mn is None:
            return
        mn_h, mx_h = mn.cpu().numpy().astype(np.float64), mx.cpu().numpy().astype(np.float64)
        self._reset_is_extrema()
        if np.isfinite(mn_h).all():              # else: no immediate-sensitivity step since the last flush
            self._fold_is_extrema(*((mn_h, mx_h) if self.opt.imm_sens_per_param else (float(mn_h[0]), float(mx_h[0]))))

    def _reset_is_extrema(self):
        for key, _, init in self._IS_EXTREMA:
            if key in self.dev_stats:
                self.dev_stats[key].fill_(init)

    # ---- train.py:345-358 ---------------------------------------------------------------------
    def calc_d_fake_loss(self, img, labels, z, y):
        o, D = self.opt, self.D
        d_fake, d_fake_aux, fake_img = self.eval_G_D(z, y, d_kwarg={"aux": o.d_fake_aux_loss})
        fake_img = fake_img.detach()
        d_fake_loss = D.fake_loss(d_fake, o.d_device)
        aux = D.aux_loss(d_fake_aux, y.to(o.d_device), o.d_device, fake=True) if (o.use_aux_loss and o.d_fake_aux_loss) else 0
        return d_fake, d_fake_aux, d_fake_loss, aux, fake_img

    def calc_d_real_loss(self, img, labels):
        o, D = self.opt, self.D
        d_real, d_real_aux = D(img, labels)
        d_real_loss = D.real_loss(d_real, o.d_device)
        aux = D.aux_loss(d_real_aux, labels, o.d_device, fake=False) if o.use_aux_loss else 0
        return d_real, d_real_aux, d_real_loss, aux

    # ---- fused form of train.py:378-402 ---------------------------------------------------------
    def _can_fuse(self, use_dp):
        o, pe = self.opt, self.privacy_engine
        return (use_dp and o.dp_mode == "gc" and o.grad_clip_split and getattr(pe, "lean", False)
                and getattr(o, "fuse_passes", True) and not o.backprop_clip)

    # ---- gradient penalty on a second stream ---------------------------------------------------------
    def _penalty_overlap_ok(self, use_dp):
        """The public-data gradient penalty (train.py:423-431) depends only on the generated batch and on mean samples — not on
        the critic pass over the private batch — and its 128-row launches (64-256 workgroups) leave most of the 256 CUs idle.  It
        runs on a second stream beside the fused 384-row pass and joins before its gradients are added to summed_grad.  Order of
        the activation-mask recordings differs, so parity tests with a recorder installed keep the serial order."""
        o = self.opt
        return (os.environ.get("CSLGAN_GP_STREAM", "1") == "1" and use_dp and o.dp_mode == "gc" and o.per_sample_grad
                and len(o.penalty) > 0 and o.penalty_use_public_data and hnn._mask_recorder is None and self.D is not None
                and next(self.D.parameters()).is_cuda)

    def _join_penalty_stream_at_boundary(self):
        """A segmented recording (distributed._boundary) ends the graph being captured at the next collective: work forked onto the
        penalty stream must be joined into the capturing stream first.  train_D's own join is then skipped (waiting, inside the NEXT
        capture, on an event of a finished one is not allowed)."""
        if Dist._boundary is not None and self._pending_penalty is not None and not self._gp_joined:
            torch.cuda.current_stream().wait_stream(self._gp_stream)
            self._gp_joined = True

    def _launch_penalty(self, img, labels, fake_img, y):
        D, pe = self.D, self.privacy_engine
        if self._gp_stream is None:
            self._gp_stream = torch.cuda.Stream(device=next(D.parameters()).device)
        side, cur = self._gp_stream, torch.cuda.current_stream()
        ops.repack_cache.multi_stream = True
        was_enabled = pe.enabled
        pe.disable_hooks()                      # the penalty's critic passes are ordinary autograd, not per-sample passes
        side.wait_stream(cur)
        try:
            with torch.cuda.stream(side):
                self._pending_penalty = self._public_penalty(img, labels, fake_img, y)
        finally:
            if was_enabled:
                pe.enable_hooks()

    def _penalty_kw(self):
        o = self.opt
        return dict(device=o.d_device, aux_penalty=o.aux_penalty, alpha=self.explicit.get("alpha"))

    def _public_penalty(self, img, labels, fake_img, y):
        """train.py:423-427: (penalty, its parameter gradients) on public data or mean samples, on the current stream."""
        pen_real, pen_labels = self.get_penalty_data(img, labels)
        penalty = calc_penalty(self.D, self.opt.penalty, pen_real, pen_labels, fake_img, y, **self._penalty_kw())
        return penalty, self._penalty_param_grads(penalty)

    def _penalty_param_grads(self, penalty):
        """autograd.grad(penalty, D.parameters()) (train.py:427).  With ONE penalty term every critic weight receives exactly one
        dense second-order weight gradient and nothing reads it before this call returns, so the column sums over the gradients'
        slabs are queued and run as one multi-segment launch (ops.deferred_sums; instead of five latency-sized launches).  Several
        terms (an auxiliary-logit penalty, two penalty types) make autograd ADD contributions inside the call: those run undeferred."""
        o, D = self.opt, self.D
        params = list(D.parameters())
        single_term = len(o.penalty) == 1 and not (o.aux_penalty and getattr(D, "linOutAux", None) is not None)
        if single_term and penalty.is_cuda:
            with ops.deferred_sums():
                return autograd.grad(penalty, params, grad_outputs=ops.ones_like_const(penalty), create_graph=False, retain_graph=False,
                                     allow_unused=True)
        return autograd.grad(penalty, params, create_graph=False, retain_graph=False, allow_unused=True)

    def _fused_passes(self, img, labels, z, y, on_fake=None):
        """[adaptive mean-sample pass] + generated pass + real pass as ONE discriminator forward/backward over the
        concatenated batch.  D has no batch-coupled layer, every block keeps its own mean-reduced loss and the
        engine treats the row blocks by role, so every number equals the three separate passes of the reference
        (train.py:204-245, 382-389); the small layers simply see 3x more rows per launch."""
        o, D, pe = self.opt, self.D, self.privacy_engine
        B = img.size(0)
        adaptive = o.grad_clip_mode.startswith("adaptive")
        blocks, roles, lab = [], [], []
        if adaptive:
            xa, ya = self._adaptive_batch()
            xa = xa.to(o.d_device)
            blocks.append(xa); roles.append(("norms", xa.size(0))); lab.append(None if ya is None else ya.to(o.d_device))
        yg = None if y is None else y.to(o.g_device)
        with torch.no_grad():
            # the generated rows' slice of the fused critic batch, when that buffer exists: the generator's output conv writes the
            # images there (channels-last) and _assemble_fused finds them in place
            g_out, r0 = None, blocks[0].size(0) if blocks else 0
            if img.dim() == 4 and img.is_cuda and str(o.g_device) == str(o.d_device) and self._g_takes_out():
                buf = self._fused_batch(r0 + 2 * B, img.shape[1:], img.device, make=False)
                if buf is not None:
                    g_out = buf[r0:r0 + B].permute(0, 2, 3, 1)
            fake_img = (self.G(z, yg, out=g_out) if g_out is not None else self.G(z, yg)).to(o.d_device)
        if on_fake is not None:
            on_fake(fake_img.detach())
        blocks += [fake_img, img]
        roles += [("dense", B), ("private", B)]
        lab += [None if y is None else y.to(o.d_device), labels]
        x_all = self._assemble_fused(blocks)
        y_all = None if labels is None else torch.cat(lab, dim=0)
        pe.enable_hooks()
        pe.row_roles = roles
        out_all, aux_all = D(x_all, y_all)
        outs = torch.split(out_all, [n for _, n in roles])
        auxs = [None] * len(roles) if aux_all is None else list(torch.split(aux_all, [n for _, n in roles]))
        i0 = 1 if adaptive else 0
        d_fake, d_real = outs[i0], outs[i0 + 1]
        d_fake_aux, d_real_aux = auxs[i0], auxs[i0 + 1]
        if getattr(D, "linear_critic_losses", False) and not o.use_aux_loss and out_all.is_cuda:
            # real_loss = -mean, fake_loss = +mean (DCResNet_models.py:149-153) of every row block and their sum in ONE launch,
            # the constant cotangent in one more (csl_gan_amd.functional.SegmentMeans)
            sizes = [n for _, n in roles]
            scale = [(1.0 if role == "dense" else -1.0) / n for role, n in roles]
            vec, total = HF.SegmentMeans.apply(out_all, sizes, scale)
            vd = vec.detach()
            d_fake_loss, d_real_loss = vd[i0], vd[i0 + 1]
            d_fake_aux_loss = d_real_aux_loss = 0
        else:
            d_fake_loss = D.fake_loss(d_fake, o.d_device)
            d_real_loss = D.real_loss(d_real, o.d_device)
            d_fake_aux_loss = D.aux_loss(d_fake_aux, y.to(o.d_device), o.d_device, fake=True) if (o.use_aux_loss and o.d_fake_aux_loss) else 0
            d_real_aux_loss = D.aux_loss(d_real_aux, labels, o.d_device, fake=False) if o.use_aux_loss else 0
            total = d_real_loss + d_fake_loss + d_real_aux_loss + d_fake_aux_loss
            if adaptive:
                total = total + D.real_loss(outs[0], o.d_device)
                if o.use_aux_loss:
                    total = total + D.aux_loss(auxs[0], lab[0], o.d_device, fake=False)
        if total.is_cuda:
            total.backward(gradient=ops.ones_like_const(total))     # the constant cotangent: no fill launch per step
        else:
            total.backward()
        pe.disable_hooks()
        if adaptive:
            with torch.no_grad():
                r = None
                if self.world_size == 1:
                    # one launch: the statistic, the clip norms, and the clip factors clip() is about to ask for
                    r = pe.adaptive_clip_fused(o.adaptive_stat, o.adaptive_scalar, bool(o.use_grad_clip_per_layer))
                if r is None:
                    self._set_adaptive_clip_norm(pe.norms_rows_sqnorms().sqrt(), join_penalty=True)
                else:
                    self.last["adaptive_stats"] = r
        pe.row_roles = None
        return d_fake, d_fake_aux, d_fake_loss, d_fake_aux_loss, fake_img.detach(), d_real, d_real_aux, d_real_loss, d_real_aux_loss

    def _g_takes_out(self):
        if self._g_out_kw is None:
            self._g_out_kw = "out" in inspect.signature(self.G.forward).parameters
        return self._g_out_kw

    def _fused_batch(self, rows, shape, device, make=True):
        """The persistent channels-last fp32 batch [rows, *shape] of the fused critic pass, allocated here and nowhere else.
        make=False: None unless it already exists with that shape on that device."""
        shp = (rows,) + tuple(shape)
        buf = self._fused_buf
        if buf is None or tuple(buf.shape) != shp or buf.device != torch.device(device):
            if not make:
                return None
            buf = self._fused_buf = torch.empty(shp, device=device, dtype=torch.float32).contiguous(memory_format=torch.channels_last)
        return buf

    def _assemble_fused(self, blocks):
        """The row blocks of the fused critic pass as ONE channels-last batch, without torch.cat's NCHW copy that the critic's first
        conv would re-lay out again: blocks that already ARE slices of the persistent buffer (the generator's output, the mean-sample
        and real batches GraphedDStep hands out as views of it) cost nothing, every other block is one copy_ straight into its
        slice (a layout change, where there is one, rides in that copy)."""
        if not blocks[0].is_cuda or blocks[0].dim() != 4:
            return torch.cat(blocks, dim=0)
        buf = self._fused_batch(sum(b.shape[0] for b in blocks), blocks[0].shape[1:], blocks[0].device)
        r0 = 0
        with torch.no_grad():
            for b in blocks:
                dst = buf[r0:r0 + b.shape[0]]
                if not (b.data_ptr() == dst.data_ptr() and b.stride() == dst.stride() and b.dtype == dst.dtype):
                    dst.copy_(b)
                r0 += b.shape[0]
        return buf

    def fused_slices(self, B, shape, device):
        """(mean-sample slice, real-batch slice) of the fused buffer for a [B, *shape] batch in an adaptive-clipping run: views a
        caller may fill in place so that _assemble_fused finds them already where they belong."""
        buf = self._fused_batch(3 * B, shape, device)
        return buf[0:B], buf[2 * B:3 * B]

    # ---- train.py:360-500 ---------------------------------------------------------------------
    def train_D(self, img, labels, z, y, use_dp=False):
        o, D, G, pe = self.opt, self.D, self.G, self.privacy_engine
        util.zero_grad(D)
        util.freeze(G)
        use_grad_clip = o.dp_mode == "gc" and use_dp
        use_imm_sens = o.dp_mode == "is" and use_dp
        if o.backprop_clip and use_dp:
            self.prop_grad_clipper.enable_hooks()
        if o.per_sample_grad and use_dp:
            pe.enable_hooks()
        if use_imm_sens:
            img.requires_grad = True
        fused = self._can_fuse(use_dp)
        self._pending_penalty, self._gp_joined = None, False
        if fused:
            pe.zero_grad()
            on_fake = (lambda f: self._launch_penalty(img, labels, f, y)) if self._penalty_overlap_ok(use_dp) else None
            (d_fake, d_fake_aux, d_fake_loss, d_fake_aux_loss, fake_img,
             d_real, d_real_aux, d_real_loss, d_real_aux_loss) = self._fused_passes(img, labels, z, y, on_fake)
            d_loss = None           # already differentiated; the gc branch below never reads it again
        else:
            if use_grad_clip and o.grad_clip_mode.startswith("adaptive"):
                self.update_adaptive_clipping_params()
            d_fake, d_fake_aux, d_fake_loss, d_fake_aux_loss, fake_img = self.calc_d_fake_loss(img, labels, z, y)
            d_real, d_real_aux, d_real_loss, d_real_aux_loss = self.calc_d_real_loss(img, labels)
            d_loss = d_real_loss + d_fake_loss + d_real_aux_loss + d_fake_aux_loss

        if o.per_sample_grad and use_dp and not fused:
            d_loss.backward()
            pe.disable_hooks()
        if o.backprop_clip and use_dp:
            if not o.per_sample_grad:
                d_loss.backward()
            self.prop_grad_clipper.disable_hooks()
        if use_grad_clip:
            pe.clip()
            if o.grad_clip_split:
                pe.accum_grads_across_passes()
            with torch.no_grad():
                self.update_grad_logging()     # after clip(): reuses its norms (the reference logs first, train.py:397)
                self.last["summed_clipped"] = [p.summed_grad.clone() for p in D.parameters()] if self.explicit.get("keep") else None

        # ---- the penalty and what finishes the gradient (train.py:419-479): one route per step
        pending, self._pending_penalty = self._pending_penalty, None
        have_penalty, per_sample = len(o.penalty) > 0, use_dp and o.per_sample_grad
        if pending is not None:
            # overlapped: launched on the second stream right after the generator forward (_launch_penalty); join, then train.py:429-431
            if not self._gp_joined:
                torch.cuda.current_stream().wait_stream(self._gp_stream)
            if use_grad_clip:
                pe.accumulate_batch()
            penalty, penalty_grad = pending
            self._add_penalty_grads(penalty_grad)
        else:
            penalty = torch.zeros((), device=o.d_device)
            if have_penalty and per_sample and o.penalty_use_public_data:
                # public penalty beside per-sample gradients (train.py:419-431): its dense gradients join the clipped sum
                if use_grad_clip:
                    pe.accumulate_batch()
                penalty, penalty_grad = self._public_penalty(img, labels, fake_img, y)
                self._add_penalty_grads(penalty_grad)
            elif have_penalty and per_sample:
                # private per-sample penalty (train.py:433-450): clips and accumulates again itself
                penalty = self._per_sample_penalty(*self.get_penalty_data(img, labels), fake_img, y, use_grad_clip)
                self._add_penalty_grads([])
            elif have_penalty:
                # plain penalty (train.py:451-462): part of d_loss
                pen_real, pen_labels = self.get_penalty_data(img, labels)
                penalty = calc_penalty(D, o.penalty, pen_real, pen_labels, fake_img, y, **self._penalty_kw())
                d_loss = d_loss + penalty
                if use_imm_sens:
                    self._finish_imm_sens(d_loss, img, with_penalty=True)
                else:
                    d_loss.backward()
            elif use_grad_clip:                # no penalty (train.py:464-479)
                pe.accumulate_batch()
            elif use_imm_sens:
                self._finish_imm_sens(d_loss, img, with_penalty=False)
            else:
                d_loss.backward()

        if self.explicit.get("keep") and use_grad_clip:
            self.last["summed_grad"] = [p.summed_grad.clone() for p in D.parameters()]
        if o.bpc_during_g_train and o.backprop_clip and use_dp:
            self.prop_grad_clipper.enable_hooks()
        self.d_optimizer.step()
        util.unfreeze(G)

        with torch.no_grad():
            if d_real.is_cuda and d_real.dtype == torch.float32 and torch.is_tensor(d_real_loss) and d_real_loss.dim() == 0:
                # train.py:488-496 in one launch, added in place to the persistent device-side sums
                names = self._DSTAT_NAMES if have_penalty else self._DSTAT_NAMES[:-1]
                ops.dstep_stats(d_real.detach().contiguous(), d_fake.detach().contiguous(), d_real_loss.detach(), d_fake_loss.detach(),
                                penalty.detach().reshape(()) if have_penalty else None, self._stat_rows(names, (7,), d_real.device))
            else:
                adv = d_real_loss.detach() + d_fake_loss.detach()
                self._acc("_d_adv_gate", adv)
                self._acc("D Adv Loss", adv)
                self._acc("D Real Loss", d_real_loss.detach())
                self._acc("D Fake Loss", d_fake_loss.detach())
                self._acc("D Real Acc", 100 * (d_real.detach() > 0).float().mean())
                self._acc("D Fake Acc", 100 * (d_fake.detach() < 0).float().mean())
                if have_penalty:
                    self._acc("D Penalty", penalty.detach().reshape(()))
            if o.use_aux_loss:
                self._acc("D Real Aux Loss", d_real_aux_loss.detach().reshape(()))
                self._acc("D Real Aux Acc", 100 * (d_real_aux.detach().argmax(dim=1) == labels).float().mean())
            self.last.update(d_real_loss=d_real_loss.detach(), d_fake_loss=d_fake_loss.detach(), penalty=penalty.detach(),
                             d_real=d_real.detach(), d_fake=d_fake.detach(), fake_img=fake_img)
            self._commit_stats()

    def _finish_imm_sens(self, d_loss, img, with_penalty):
        """The immediate-sensitivity backward and what follows it in the reference."""
        o, pe = self.opt, self.privacy_engine
        pe.backward(d_loss, img)
        moving_avg = o.imm_sens_scaling_mode == "moving-avg-pl"
        if moving_avg:
            self.update_sens_moving_avg()
        # Reference parity, not an oversight: with a penalty (train.py:456-460) update_is_logging follows the moving-average update
        # unconditionally; without one (train.py:468-473) it is the `elif` of that update, so moving-avg-pl does not log there.
        if with_penalty or not moving_avg:
            self.update_is_logging()
        if with_penalty and self.explicit.get("keep"):
            self.last["is_param_grads"] = [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in self.D.parameters()]

    def _add_penalty_grads(self, penalty_grad):
        """train.py:429-431: the penalty's parameter gradients join summed_grad — a sum, not a mean, hence x batch_size; one
        multi-tensor launch."""
        with torch.no_grad():
            pairs = [(p.summed_grad, g) for p, g in zip(self.D.parameters(), penalty_grad) if g is not None]
            if pairs:
                torch._foreach_add_([t for t, _ in pairs], [g for _, g in pairs], alpha=self.opt.batch_size)
            if self.explicit.get("keep"):
                self.last["penalty_grads"] = [None if g is None else g.clone() for g in penalty_grad]

    # ---- train.py:433-450 ---------------------------------------------------------------------
    def _per_sample_penalty(self, pen_real, pen_labels, fake_img, y, use_grad_clip):
        """Gradient penalty evaluated on PRIVATE data (--penalty_use_public_data False): the penalty of sample i is part of that
        sample's loss, so its parameter gradient is added to p.grad_sample[0, i] (train.py:447 — pass index 0 as the reference
        writes it) and the batch is clipped again (train.py:449-450).  The reference takes B separate autograd.grad calls, each
        through the whole batch graph; penalties[i] depends on row i only, so ONE second-order sweep of sum_i penalties[i] with
        per-sample (group = 1) weight-gradient kernels gives the same B gradients (csl_gan_amd.functional.per_sample_param_grads).
        The first-order bias terms of the penalty are identically zero."""
        o, D, pe = self.opt, self.D, self.privacy_engine
        if not use_grad_clip:
            raise NotImplementedError("per-sample gradient penalties are defined for dp_mode=gc (train.py:433-450)")
        if not all(hasattr(p, "grad_sample") for p in D.parameters()):
            raise RuntimeError("--penalty_use_public_data False edits p.grad_sample of every parameter: run with --materialize all")
        if self._warn_ps_pen:              # the reference prints this every step (train.py:436); once is enough here
            print("WARNING: Per sample penalty currently causes a memory leak.")
            self._warn_ps_pen = False
        penalties = calc_penalty(D, o.penalty, pen_real, pen_labels, fake_img, y, per_sample=True, **self._penalty_kw())
        seen = set()

        def sink(p, rows):
            seen.add(id(p))
            pe.add_to_grad_sample(p, rows, 0)
        with HF.per_sample_param_grads(sink, list(D.parameters())):
            dense = autograd.grad(penalties.sum(), list(D.parameters()), create_graph=False, retain_graph=False, allow_unused=True)
        # every weight the penalty depends on must have gone through the per-sample sink (a layer whose filter is not a zero-copy
        # view of its parameter would have produced a dense gradient instead, which this branch cannot use)
        stray = [n for (n, p), g in zip(D.named_parameters(), dense) if g is not None and id(p) not in seen]
        if stray:
            raise RuntimeError("per-sample penalty: parameters %s received a dense instead of a per-sample gradient" % stray)
        pe.clip(recompute_norms=True)
        pe.accumulate_batch()
        with torch.no_grad():
            if self.explicit.get("keep"):
                self.last["summed_clipped_with_penalty"] = [p.summed_grad.clone() for p in D.parameters()]
        return penalties.detach().mean(dim=0)

    # ---- train.py:502-517 ---------------------------------------------------------------------
    def train_G(self, z, y):
        o, G, D = self.opt, self.G, self.D
        util.zero_grad(G)
        # The reference lets D's parameters collect (stale, later discarded) gradients here (train.py:505-510,
        # cleared at train.py:361).  Freezing D for the G step skips those weight-gradient kernels; G's
        # gradients are unchanged.
        util.freeze(D)
        try:
            d_fake, d_fake_aux, _ = self.eval_G_D(z, y)
            g_adv_loss = G.loss(d_fake, o.d_device)
            g_aux_loss = D.aux_loss(d_fake_aux, y.to(o.d_device), o.d_device) if o.is_acgan else 0
            (g_adv_loss + g_aux_loss).backward()
        finally:
            util.unfreeze(D)
        if self.world_size > 1:
            self._average_G_grads()
        self.g_optimizer.step()
        self._acc("G Adv Loss", g_adv_loss.detach())
        if o.is_acgan:
            self._acc("G Aux Loss", g_aux_loss.detach())
            self._acc("G Aux Acc", 100 * (d_fake_aux.detach().argmax(dim=1) == y.to(o.d_device)).float().mean())
        self._commit_stats()

    def _average_G_grads(self):
        """G is replicated; its (non-private) gradients are averaged over ranks with ONE flat
        all-reduce (G64: 84 MB).  p.grad tensors are re-pointed at slices of the bucket, like the D side."""
        ps = [p for p in self.G.parameters() if p.grad is not None]
        flat = self._g_flat
        n = sum(p.numel() for p in ps)
        if flat is None or flat.numel() != n or flat.device != ps[0].device:
            flat = self._g_flat = torch.empty(n, device=ps[0].device, dtype=torch.float32)
        off = 0
        for p in ps:
            v = torch.as_strided(flat, p.size(), p.stride(), storage_offset=off)
            v.copy_(p.grad)
            p.grad = v
            off += p.numel()
        Dist.average_across_ranks(flat)

    # ---- train.py:521-546 ---------------------------------------------------------------------
    def train(self, epoch, batch_i, real_images_batch, real_labels_batch, use_dp=False):
        o, lg = self.opt, self.logger
        img = real_images_batch.to(o.d_device)
        labels = real_labels_batch.to(o.d_device) if o.conditional else None
        n = img.size(0)
        if self.graphed is not None and use_dp and n == o.batch_size:
            self.graphed(img, labels)          # recorded once, replayed afterwards (z and the mean-sample draws happen inside)
        else:
            self.train_D(img, labels, self.gen_z(n), labels, use_dp=use_dp)
        if batch_i % o.n_d_steps == 0:
            acc = self.dev_stats.get("_d_adv_gate")
            gate = None if acc is None else acc.detach().reshape(1).clone()
            if acc is not None:
                acc.zero_()
            if gate is not None and self.world_size > 1:           # every rank must take the same branch
                gate = Dist.average_across_ranks(gate)
            d_adv = 0.0 if gate is None else float(gate)           # the one host sync, every n_d_steps iterations
            if d_adv / o.n_d_steps < o.train_d_until_threshold:
                lg.log_g_iter += 1
                self.train_G(self.gen_z(n), self.gen_y(n))
        if ((batch_i + 1) * o.batch_size) % o.log_every == 0:
            self.flush_stats()
            for stat in [k for k in lg.stats if k.startswith("G ")]:
                lg.stats[stat] *= 0 if lg.log_g_iter == 0 else lg.interval / lg.log_g_iter
            lg.log_g_iter = 0
            self.log(epoch, 100 * batch_i / self.batches_per_epoch, print_dp=use_dp)
        if ((batch_i + 1) * o.batch_size) % o.sample_every == 0:
            self.sample(epoch, batch_i)

    # ---- train.py:256-261, 298-308 ------------------------------------------------------------
    def init_fixed_samples(self):
        o = self.opt
        self.fixed_z = self.gen_z(o.sample_num)
        if o.conditional:
            self.fixed_y = torch.cat([torch.arange(o.n_classes) for _ in range(o.sample_num // o.n_classes)]).to(o.g_device)
            self.fixed_z = self.fixed_z[:len(self.fixed_y)]
        else:
            self.fixed_y = self.gen_y(o.sample_num)

    def sample(self, epoch, batch):
        """G.eval() on the fixed latents -> samples/<epoch+1>-<batch>.png, n_classes images per row (rank 0 only under --dist)."""
        o, G = self.opt, self.G
        if self.fixed_z is None or self.rank != 0:
            return None
        G.eval()
        with torch.no_grad():
            fake = G(self.fixed_z, self.fixed_y).to("cpu")
            if o.dataset == "CelebA":
                fake = util.denorm_celeba(fake)
            path = os.path.join(o.output_dir + "samples/", "%d-%d.png" % (epoch + 1, batch))
            util.save_image(fake, path, nrow=o.n_classes)
        G.train()
        return path

    def log(self, epoch, epoch_progress, print_dp=False):
        self.flush_stats()
        if self.rank != 0:          # --dist: every rank keeps its own CSV (log_rank<r>.csv); only rank 0 prints
            with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
                self.logger.log(epoch, epoch_progress)
            return
        self.logger.log(epoch, epoch_progress)
        pe = self.privacy_engine
        if print_dp and pe is not None and pe.steps > 0:
            eps, best_alpha = pe.get_privacy_spent(self.opt.delta)
            print("({}, {})-DP for alpha={}".format(eps, self.opt.delta, best_alpha))

    # ---- device-side statistics ----------------------------------------------------------------
    _DSTAT_NAMES = ("_d_adv_gate", "D Adv Loss", "D Real Loss", "D Fake Loss", "D Real Acc", "D Fake Acc", "D Penalty")
    _GLOG_NAMES = ("D Layer Grad Norm Means", "D Layer Grad Norm Stds", "D Layer Grad Norm Maxes", "Clipping Params", "Grads Clipped")

    def _stat_rows(self, names, shape, dev):
        """A persistent zeroed device buffer whose leading rows dev_stats holds under `names`, as views: a kernel adds to the whole
        buffer in one launch, and flush / reset / the G gate see the same memory.  The [7] sums train_D's closing lines update
        (train.py:488-496, cslgan_dstep_stats_f32; without a penalty the last row, "D Penalty", stays unregistered) and the
        [5, rows] sums of update_grad_logging (cslgan_grad_log_stats_f32).  Made again, and registered again, when the device or the
        shape changes or a caller has cleared dev_stats."""
        a = self._stat_bufs.get(names[0])
        if a is None or a.device != dev or tuple(a.shape) != tuple(shape) or self.dev_stats.get(names[0]) is None:
            a = self._stat_bufs[names[0]] = torch.zeros(shape, device=dev, dtype=torch.float32)
            for i, n in enumerate(names):
                self.dev_stats[n] = a[i]
        return a

    def _acc(self, name, value):
        """Running sums live in persistent device tensors updated IN PLACE (a step recorded in a HIP graph keeps accumulating
        into the same memory on replay)."""
        cur = self.dev_stats.get(name)
        if cur is None or cur.shape != value.shape:
            self.dev_stats[name] = value.detach().clone()
        elif value.is_cuda:
            self._pending_stats.append((cur, value.detach()))     # folded in by _commit_stats: one multi-tensor add per step
        else:
            cur.add_(value.detach())

    def _commit_stats(self):
        """The step's statistic updates as ONE multi-tensor launch (instead of a dozen 4-us kernels)."""
        if self._pending_stats:
            torch._foreach_add_([c for c, _ in self._pending_stats], [v for _, v in self._pending_stats])
            self._pending_stats = []

    def reset_stats(self):
        """logger.reset_stats() of the reference (train.py:566, 576): the statistics live partly on the device here, so the
        pending device-side sums (everything accumulated since the last log line) must be dropped with them — otherwise the
        tail of one epoch leaks into the first log line of the next."""
        self.logger.reset_stats()
        self._commit_stats()
        self._reset_is_extrema()
        for k, v in self.dev_stats.items():
            if not k.startswith("_"):
                v.zero_()

    def flush_stats(self):
        """Fold device-side sums into the Logger (this is where the host synchronises)."""
        self._commit_stats()
        self._flush_is_extrema()
        for k, v in list(self.dev_stats.items()):
            if k.startswith("_"):
                continue
            val = v.detach().cpu()
            val = float(val) if val.dim() == 0 else val.numpy().astype(np.float64)
            if k in self.logger.stats:
                self.logger.stats[k] = self.logger.stats[k] + val
            v.zero_()

    # ---- train.py:263-278 ---------------------------------------------------------------------
    def _make_logger(self, log_to):
        o = self.opt
        aux, pen, gc, im = o.use_aux_loss, len(o.penalty) > 0, o.dp_mode == "gc", o.dp_mode == "is"
        fmt = "G " + ("Adv " if aux else "") + "Loss: {:4.4f}" + (", G Aux: {:4.4f} / {:3.1f}%\n" if aux else " | ")
        fmt += "D Adv Loss: {:4.4f} (Real: {:4.4f} / {:3.1f}%, Fake: {:4.4f} / {:3.1f}%"
        fmt += (", Real Aux: {:4.4f} / {:3.1f}%" if aux else "") + (", Penalty: {:4.4f}" if pen else "") + ")"
        if gc:
            fmt += "\n=== Grad Norms ===\nMean Per Layer: {}\nStd Per Layer: {}\nMax Per Layer: {}\nClipping Params: {}\nGrads Clipped: {}"
        if im:
            fmt += "\nIS - Mean: {} - Min: {} - Max: {}"
        names = ["G Adv Loss"] + (["G Aux Loss", "G Aux Acc"] if aux else [])
        names += ["D Adv Loss", "D Real Loss", "D Real Acc", "D Fake Loss", "D Fake Acc"]
        names += (["D Real Aux Loss", "D Real Aux Acc"] if aux else []) + (["D Penalty"] if pen else [])
        if gc:
            names += ["D Layer Grad Norm Means", "D Layer Grad Norm Stds", "D Layer Grad Norm Maxes", "Clipping Params", "Grads Clipped"]
        if im:
            names += ["IS Mean", "IS Min", "IS Max"]
        every = o.log_every_epochs * o.train_set_size if o.log_every_epochs > 0 else o.log_every
        path = log_to if log_to is not None else o.output_dir + "log.csv"
        lg = Logger(fmt, names, max(every // o.batch_size, 1), path)
        lg.log_g_iter = 0
        return lg


class _StepCounters:
    """The host-side counters one D-step advances, which the accountant and checkpoints read: the engine's steps and its noise-call
    mirror, and every Adam state's step.  A replay runs no Python, so GraphedDStep advances them itself; a failed recording ran the
    Python without the device work, so it puts them back."""

    def __init__(self, engine, optimizer):
        self.pe, self.optimizer = engine, optimizer

    def snapshot(self):
        return self.pe.steps, self.pe._noise_calls, {id(st): st["step"] for st in self.optimizer.state.values()}

    def restore(self, snap):
        self.pe.steps, self.pe._noise_calls, adam = snap
        for st in self.optimizer.state.values():       # (a state made since the snapshot keeps its count)
            st["step"] = adam.get(id(st), st["step"])

    def advance(self):
        self.pe.steps += 1
        self.pe._noise_calls += 1
        for st in self.optimizer.state.values():
            st["step"] += 1


@contextlib.contextmanager
def _no_gc():
    """No cyclic garbage collection while the stream is capturing.  A dead cycle that owns device resources — an earlier
    GraphedDStep's graph and its private pool, most of all — is finalised wherever the collector happens to run, which can be an
    autograd worker thread in the middle of the recording; releasing a pool calls hipFree, which is not permitted during a
    (global-mode) capture, and the failure surfaces inside a destructor: the process aborts.  (torch 2.10 no longer collects in
    torch.cuda.graph.__enter__.)  So: collect now, on this thread, then keep the collector off until the capture has ended.  The
    double backward of an is-mode step makes enough cycles to trip it within one recording."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


class GraphedDStep:
    """One `Trainer.train_D` recorded in a HIP graph and replayed (fixed batch size and configuration).

    The D-step of the small models is bound by the host: BASELINE configs[1] (MNIST conditional vanilla GAN, bs=600) issues
    ~100 launches for 0.6 ms of kernel work.  Every C-ABI entry enqueues on the caller's stream, never allocates or
    synchronises, and takes its per-step scalars either from device memory (the Philox call counter, Adam's step count, the
    adaptive clip norms) or as constants of the configuration — so the whole step, torch's autograd bookkeeping included,
    can be captured once (torch.cuda.CUDAGraph on the same stream) and replayed with one host call.

    Per step, OUTSIDE the graph: the batch is copied into static buffers, z / penalty alpha / mean-sample batches are drawn
    into static buffers (torch's device generator), the graph is replayed, and the host-side counters the accountant and
    checkpoints read (engine.steps, the noise-call mirror, Adam's step) are advanced.  use_graph=False runs the identical
    sequence eagerly (the parity reference in tests/test_graph_gpu.py)."""

    def __init__(self, trainer, use_graph=True, warmup=2):
        self.tr, self.use_graph, self.warmup = trainer, use_graph, warmup
        o = trainer.opt
        if not (o.use_dp and o.dp_mode in ("gc", "is")) or (o.dp_mode == "is" and o.imm_sens_scaling_mode == "moving-avg-pl"):
            raise NotImplementedError("GraphedDStep covers the DP D-steps whose host never reads the device inside the step: dp_mode=gc "
                                      "and dp_mode=is (not the moving-average scaling mode, which reads gradient norms on the host)")
        self.graph, self.bufs, self.capture_error = None, None, None
        # the recording: graphs and the collectives issued between them; a whole-step recording is one graph (`graph` is the first)
        self.graphs, self.between, self.segmented = [], [], False
        self._pinned = []                  # generator filter workspaces pinned in ops.repack_cache for the recorded graph
        self._prev = (trainer.d_optimizer.capturable, trainer.explicit)
        trainer.d_optimizer.capturable = True

    def release(self):
        """Give the trainer back to plain eager stepping (bench.py times other variants on the same trainer afterwards)."""
        self.tr.d_optimizer.capturable, self.tr.explicit = self._prev
        self.graph, self.graphs, self.between = None, [], []
        if self._pinned:
            ops.repack_cache.unpin(self._pinned)
            self._pinned = []

    def _alloc(self, img, labels):
        o, dev, B = self.tr.opt, self.tr.opt.d_device, img.shape[0]
        b = dict(img=torch.empty_like(img, device=dev), z=torch.empty((B, o.g_latent_dim), device=o.g_device),
                 labels=None if labels is None else torch.empty_like(labels, device=dev))
        need_ms = self.tr.mean_sampler is not None
        fused_views = (need_ms and img.dim() == 4 and o.dp_mode == "gc" and o.grad_clip_mode.startswith("adaptive") and o.public_set_size == 0
                       and self.tr._can_fuse(True) and torch.device(dev).type == "cuda")
        if fused_views:
            # the mean-sample batch of the adaptive pass and the real batch ARE the first and the last row block of the fused critic
            # batch (Trainer._assemble_fused): the sampler and the input copy write them in place, channels-last
            ms_view, img_view = self.tr.fused_slices(B, img.shape[1:], dev)
            b["img"] = img_view
        if need_ms and (len(o.penalty) > 0 or o.grad_clip_mode.startswith("adaptive")):
            cl = lambda: torch.empty(tuple(img.shape), device=dev, dtype=torch.float32).contiguous(memory_format=torch.channels_last) \
                if img.dim() == 4 else torch.empty_like(img, device=dev)
            b["ms_adapt"], b["pen_real"] = (ms_view if fused_views else cl()), cl()
            if labels is not None:
                b["ms_labels"] = torch.empty_like(b["labels"])
        if len(o.penalty) > 0:
            b["alpha"] = torch.empty(B, device=dev)
        self.bufs = b
        self.tr.explicit = {k: b[s] for k, s in (("ms_adapt", "ms_adapt"), ("pen_real", "pen_real"), ("alpha", "alpha"),
                                                 ("ms_adapt_labels", "ms_labels")) if s in b}

    @torch.no_grad()
    def _fill(self, img, labels):
        b = self.bufs                  # (no_grad: in is mode the static image buffer is a leaf that requires grad, train.py:375)
        b["img"].copy_(img, non_blocking=True)
        if labels is not None:
            b["labels"].copy_(labels, non_blocking=True)
        b["z"].normal_(0.0, 1.0)
        if "ms_adapt" in b:
            ms = self.tr.mean_sampler
            direct = b["ms_adapt"].is_cuda and b["ms_adapt"].dim() == 4 and ms.mean_samples.is_cuda and ms.mean_samples.dim() == 5
            req = b.get("labels") if labels is not None else None
            drawn_labels = []
            for key in ("ms_adapt", "pen_real"):
                x, yl = ms.sample(img.shape[0], requested_labels=req, out=b[key] if direct else None)
                if not direct:
                    b[key].copy_(x)
                drawn_labels.append(yl)
            if "ms_labels" in b:
                b["ms_labels"].copy_(drawn_labels[0])
        if "alpha" in b:
            b["alpha"].uniform_(0.0, 1.0)

    def _eager(self):
        b = self.bufs
        self.tr.train_D(b["img"], b["labels"], b["z"], b["labels"], use_dp=True)

    def _replay(self):
        for i, g in enumerate(self.graphs):      # graph, collective, graph, ... : the collectives are ordinary stream-ordered calls
            g.replay()
            if i < len(self.between):
                self.between[i]()

    def _capture_segments(self):
        """Record the step as several graphs that END at each collective (distributed._boundary): nothing of RCCL / gloo is inside a
        graph.  All graphs share the first one's memory pool (a tensor made in one segment is read in the next); the closures kept
        in self.between hold the tensors their collectives run on, so those addresses stay reserved."""
        graphs, between, cur = [], [], [None]
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())

        def begin():
            g = torch.cuda.CUDAGraph()
            if graphs:
                g.capture_begin(pool=graphs[0].pool())
            else:
                g.capture_begin()
            cur[0] = g

        def boundary(fn):
            g, cur[0] = cur[0], None
            g.capture_end()
            graphs.append(g)
            out = fn()                           # issued for real (on whatever the unexecuted graph left in memory): keeps the ranks in step
            between.append(fn)
            begin()
            return out

        with torch.cuda.stream(cap):
            begin()
            Dist._boundary = boundary
            try:
                self._eager()
                g, cur[0] = cur[0], None
                g.capture_end()
                graphs.append(g)
            except BaseException:
                if cur[0] is not None:           # leave capture mode before the error travels on
                    try:
                        cur[0].capture_end()
                    except Exception:
                        pass
                raise
            finally:
                Dist._boundary = None
        torch.cuda.current_stream().wait_stream(cap)
        self.graphs, self.between = graphs, between

    def _record(self):
        """Record the step the static buffers hold; its host-side bookkeeping runs once, here.  False when the capture failed: the
        host state is back where it was and the run goes on eagerly."""
        tr, pe = self.tr, self.tr.privacy_engine
        # state a replay must find in HBM exists BEFORE the capture (created inside it, torch.full would be re-run by every
        # replay: a constant Adam step and a constant noise offset)
        tr.d_optimizer.prepare_capture()
        pe.ensure_noise_counter()
        # every repacked / folded filter of the CRITIC must be RECORDED: a cache hit at capture time would bake in "no repack"
        # plus a pointer to an eager buffer — stale weights (and freed memory) on every replay once a replayed Adam has moved the
        # parameters.  The GENERATOR is frozen during D-steps: its folded / pre-split filters (made by the eager warm-up steps) are
        # PINNED instead — the recording hits them, no replay re-makes them, and refresh_pinned() rebuilds them in place before a
        # replay when a train_G step has changed the weights.
        torch.cuda.synchronize()
        self._pinned = ops.repack_cache.pin({m._wtoken for m in tr.G.modules() if hasattr(m, "_wtoken")})
        ops.repack_cache.clear()
        torch.cuda.synchronize()
        counters = _StepCounters(pe, tr.d_optimizer)
        snap = counters.snapshot()
        self.segmented = tr.world_size > 1 and not Dist.collectives_capturable()
        try:
            with _no_gc():
                if self.segmented:
                    self._capture_segments()
                else:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        self._eager()            # RECORDED, not executed
                    self.graphs = [graph]
        except Exception as e:                   # e.g. a collective this backend cannot record
            warnings.warn("HIP-graph capture of the D-step failed (%s: %s); stepping eagerly from here on" % (type(e).__name__, str(e)[:200]))
            torch.cuda.synchronize()
            ops.repack_cache.clear()
            # A whole-step recording executed nothing on the device.  A segmented one has issued, for real, the collectives it
            # reached (boundary() in _capture_segments) on whatever the unexecuted graphs left in memory; no kernel of the step ran.
            # Either way the host-side bookkeeping goes back and the half-built per-sample state is dropped; the caller then runs
            # this step eagerly.
            counters.restore(snap)
            pe._reset_samples()
            for p in pe.params:
                if hasattr(p, "summed_grad"):
                    del p.summed_grad
            self.use_graph, self.capture_error = False, repr(e)[:300]
            return False
        self.graph = self.graphs[0]
        ops.repack_cache.clear()                 # entries made during capture point into the graph's private pool (pinned ones stay)
        return True

    def __call__(self, img, labels=None):
        tr = self.tr
        if self.bufs is None:
            self._alloc(img, labels)
        elif img.shape != self.bufs["img"].shape:
            raise RuntimeError("GraphedDStep was recorded for batch shape %s, got %s" % (tuple(self.bufs["img"].shape), tuple(img.shape)))
        self._fill(img, labels)
        if not self.use_graph:
            return self._eager()
        if self.graph is None:
            if self.warmup > 0:
                self.warmup -= 1
                return self._eager()             # first steps run eagerly: allocator pools, caches and accumulators settle
            if not self._record():
                return self._eager()
            self._replay()                       # the step itself; the recording has advanced the host counters
        else:
            if self._pinned:
                ops.repack_cache.refresh_pinned()    # a train_G step since the last replay: the generator's filter workspaces, in place
            self._replay()
            _StepCounters(tr.privacy_engine, tr.d_optimizer).advance()     # what the recorded python would have done on the host
        tr.d_optimizer.bump_versions()           # the replayed Adam wrote D's weights: eager code (train_G) must re-pack them
