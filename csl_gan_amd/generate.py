"""A saved generator as a synthetic DATASET (reference gensamples.py:26-41; mem_inf_attack.py:353-402 repeats the loop).

Two properties the reference's script does not have:

  * sample g is a function of (checkpoint, seed, g) alone.  The latent rows come from an indexed Philox stream (include/cslgan.h
    "Device random streams": key = seed xor a tag, counter = (q, g lo, g hi, tag) -> columns 4q..4q+3 of row g), so the output does
    not depend on the batch size, on where a run was cut, or on how an index range is split between processes; labels of a
    conditional generator are g mod n_classes (balanced over any contiguous range).  `latent_normals_host` restates the stream in
    numpy for CPU runs; the device draws it with cslgan_latent_normal_f32;
  * the output is the uint8 NHWC cache of csl_gan_amd.pipeline (`<path>.u8`, `.labels.npy`, `.json`), which CachedImages,
    DevicePrefetcher and `--data_cache` read as it is: synthetic data can be fed straight back into the trainer.

On a HIP device one batch is three steps, latent kernel -> frozen G(z, y) (NHWC, GroupNorm statistics from the conv epilogues,
eval-mode BatchNorm on cslgan_batchnorm_eval_act_f32) -> cslgan_f32_to_u8 into a device [B, H, W, C] byte buffer.  Full batches are
recorded once in a HIP graph on one stream; the first index lives in HBM and the host rewrites it between replays.  The bytes leave
through two pinned buffers on a side stream, and a writer thread moves finished buffers into the sink.
"""
from __future__ import annotations

import json
import os
import queue
import threading

import numpy as np
import torch

from . import pipeline

LATENT_SEED_TAG = 0x6C6174656E747A73          # include/cslgan.h: xor-ed into the seed (keeps the stream apart from the noise streams)
LATENT_COUNTER_TAG = 0x7A6C6174               # word 3 of every counter of the stream
_M64 = 0xFFFFFFFFFFFFFFFF


def latent_seed(seed):
    """The 64-bit Philox key of the latent stream of `seed`."""
    return (int(seed) ^ LATENT_SEED_TAG) & _M64


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays of 32-bit words."""
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & m32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bit: no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _box_muller(a, b):
    u1 = (a >> np.uint64(8)).astype(np.float64) * (1.0 / 16777216.0) + (0.5 / 16777216.0)
    u2 = (b >> np.uint64(8)).astype(np.float64) * (1.0 / 16777216.0)
    r, t = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    return r * np.cos(t), r * np.sin(t)


def latent_normals_host(seed, first, n, dim):
    """Rows first .. first+n-1 of the latent stream, [n, dim] float32: the formula in float64, cast once."""
    key = latent_seed(seed)
    g = (np.arange(n, dtype=np.uint64) + np.uint64(int(first) & _M64))[:, None]          # wraps mod 2^64 like the device
    q = np.arange((dim + 3) // 4, dtype=np.uint64)[None, :]
    w = _philox4x32_10(q, g, g >> np.uint64(32), LATENT_COUNTER_TAG, key & 0xFFFFFFFF, key >> 32)
    z0, z1 = _box_muller(w[0], w[1])
    z2, z3 = _box_muller(w[2], w[3])
    return np.stack([z0, z1, z2, z3], axis=-1).reshape(n, -1)[:, :dim].astype(np.float32)


def labels_host(first, n, n_classes, fixed_label=-1):
    """Labels of samples first .. first+n-1: the fixed label, else g mod n_classes."""
    if fixed_label >= 0:
        return np.full(n, int(fixed_label), dtype=np.int64)
    g = np.arange(n, dtype=np.uint64) + np.uint64(int(first) & _M64)                     # wraps mod 2^64 like the device
    return (g % np.uint64(max(int(n_classes), 1))).astype(np.int64)


def quantise_host(x, scale, bias):
    """util.denorm_celeba + util.save_image's quantisation, elementwise in fp32 (what cslgan_f32_to_u8 computes bit for bit)."""
    t = x * scale + bias
    return t.clamp(0, 1).mul(255).add(0.5).clamp(0, 255).to(torch.uint8)


def image_geometry(train_opt):
    """(H, W, C, signed) of the generator's images: CelebA lives in [-1, 1] (tanh), MNIST in [0, 1]."""
    if train_opt.dataset == "MNIST":
        return 28, 28, 1, False
    s = int(getattr(train_opt, "im_size", 64) or 64)
    return s, s, 3, True


class SampleGenerator:
    """Rows of the synthetic dataset of one generator: `generate(first, count, sink)`.

    sink(start, rows_u8 [b, H, W, C] uint8 ndarray, labels [b] int64 ndarray) receives consecutive row blocks, start counted from 0
    at `first`; the arrays are only valid during the call.  keep_float: `generate(..., float_sink=...)` also hands over the
    generator's own fp32 NHWC output of every block (tests and measurements; one more copy per batch)."""

    def __init__(self, G, train_opt, device, seed, batch_size, hip_graph=True, compute_dtype=None, fixed_label=-1, keep_float=False):
        self.G, self.opt, self.device = G, train_opt, torch.device(device)
        self.seed, self.B, self.fixed_label, self.keep_float = int(seed), int(batch_size), int(fixed_label), bool(keep_float)
        if self.B < 1:
            raise ValueError("batch_size must be positive")
        self.conditional = bool(train_opt.conditional)
        self.n_classes = int(train_opt.n_classes) if self.conditional else 1
        if self.fixed_label >= self.n_classes:
            raise ValueError("label %d is no class of %d" % (self.fixed_label, self.n_classes))
        self.dim = int(train_opt.g_latent_dim)
        self.H, self.W, self.C, self.signed = image_geometry(train_opt)
        self.scale, self.bias = (0.5, 0.5) if self.signed else (1.0, 0.0)
        self.on_gpu = self.device.type == "cuda"
        self.compute_dtype = compute_dtype or getattr(train_opt, "compute_dtype", None) or "fp32"
        G.eval()
        for p in G.parameters():
            p.requires_grad_(False)
        self.use_graph = bool(hip_graph) and self.on_gpu
        self.graph, self._pinned_ws, self._static = None, [], None
        self._prev_compute = None
        if self.on_gpu:
            from . import ops
            self._prev_compute = ops.get_compute_dtype()      # process-wide switch: release() puts it back
            ops.set_compute_dtype(self.compute_dtype)

    # ---- one batch ---------------------------------------------------------------------------------------------------------------
    def _nhwc(self, img):
        """The generator's logical-NCHW output as the NHWC tensor it is in memory (a copy only for a layout that is not)."""
        x = img.permute(0, 2, 3, 1)
        return x if x.is_contiguous() else x.contiguous()

    def _batch_cpu(self, first, n):
        z = torch.from_numpy(latent_normals_host(self.seed, first, n, self.dim)).to(self.device)
        lab = labels_host(first, n, self.n_classes, self.fixed_label)
        with torch.no_grad():
            x = self._nhwc(self.G(z, torch.from_numpy(lab).to(self.device) if self.conditional else None)).float()
        return quantise_host(x, self.scale, self.bias).cpu().numpy(), (x.cpu().numpy() if self.keep_float else None)

    def _buffers(self, n):
        dev = self.device
        b = dict(z=torch.empty((n, self.dim), device=dev), y=torch.empty(n, device=dev, dtype=torch.int64),
                 u8=torch.empty((n, self.H, self.W, self.C), device=dev, dtype=torch.uint8), first=torch.zeros(1, device=dev, dtype=torch.int64))
        if self.keep_float:
            b["f32"] = torch.empty((n, self.H, self.W, self.C), device=dev, dtype=torch.float32)
        return b

    def _steps(self, b, first_value):
        """latent kernel -> G -> quantisation on the current stream; the first index is first_value + *b["first"]."""
        from . import ops
        n = b["z"].shape[0]
        ops.latent_normal(self.seed, first_value, n, self.dim, first_index_dev=b["first"], n_classes=self.n_classes, fixed_label=self.fixed_label,
                          out=b["z"], labels_out=b["y"])
        with torch.no_grad():
            x = self._nhwc(self.G(b["z"], b["y"] if self.conditional else None))
        if tuple(x.shape) != tuple(b["u8"].shape):
            raise RuntimeError("generator output %s, expected %s" % (tuple(x.shape), tuple(b["u8"].shape)))
        ops.f32_to_u8(x, self.scale, self.bias, out=b["u8"])
        if self.keep_float:
            b["f32"].copy_(x)

    def _record(self):
        """Full batches as ONE recorded graph.  Two eager batches first (allocator pools, filter workspaces and scratch caches
        settle); the generator's filter workspaces are pinned so the recording reads them where they are; nothing created under
        capture is kept except what the graph writes into the static buffers."""
        from . import ops
        import gc
        b = self._static = self._buffers(self.B)
        for _ in range(2):
            self._steps(b, 0)
        torch.cuda.synchronize(self.device)
        self._pinned_ws = ops.repack_cache.pin({m._wtoken for m in self.G.modules() if hasattr(m, "_wtoken")})
        ops.repack_cache.clear()
        graph = torch.cuda.CUDAGraph()
        gc.collect()                        # no cyclic collection while the stream captures (trainer.GraphedDStep: a dead graph's
        gc_was_on = gc.isenabled()          # pool freed inside a capture aborts the process)
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                self._steps(b, 0)
        finally:
            if gc_was_on:
                gc.enable()
        ops.repack_cache.clear()            # entries made under capture point into the graph's pool (pinned ones stay)
        self.graph = graph

    def release(self):
        """Drop the recorded graph, its pool and the pins it held; the compute-dtype switch goes back to what it was."""
        self.graph, self._static = None, None
        if self._pinned_ws:
            from . import ops
            ops.repack_cache.unpin(self._pinned_ws)
            self._pinned_ws = []
        if self._prev_compute is not None:
            from . import ops
            ops.set_compute_dtype(self._prev_compute)
            self._prev_compute = None

    def device_batch(self, first, n=None):
        """The device work of one batch of n rows (default: a full batch) starting at sample `first`, enqueued on the current stream:
        a replay of the recorded graph for full batches (recorded on first use), the same three steps eagerly for a ragged one or
        with hip_graph=False.  Returns the buffers (z, y, u8, and f32 with keep_float); a full batch's are overwritten by the next."""
        n = self.B if n is None else int(n)
        full = n == self.B
        if full and self.use_graph and self.graph is None:
            self._record()
        if full and self._static is None:
            self._static = self._buffers(self.B)
        b = self._static if full else self._buffers(n)
        g0 = int(first) & _M64                      # the graph reads the index from HBM: nothing else changes between replays
        b["first"].fill_(g0 - (1 << 64) if g0 >= (1 << 63) else g0)
        if full and self.graph is not None:
            self.graph.replay()
        else:
            self._steps(b, 0)
        return b

    # ---- the loop ----------------------------------------------------------------------------------------------------------------
    def generate(self, first, count, sink, float_sink=None):
        first, count = int(first), int(count)
        if count <= 0:
            return
        if float_sink is not None and not self.keep_float:
            raise RuntimeError("float_sink needs keep_float=True")
        blocks = [(s, min(self.B, count - s)) for s in range(0, count, self.B)]
        if not self.on_gpu:
            for s, n in blocks:
                u8, f32 = self._batch_cpu(first + s, n)
                sink(s, u8, labels_host(first + s, n, self.n_classes, self.fixed_label))
                if float_sink is not None:
                    float_sink(s, f32)
            return
        with torch.cuda.device(self.device):
            self._generate_gpu(first, blocks, sink, float_sink)

    def _generate_gpu(self, first, blocks, sink, float_sink):
        main = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(device=self.device)
        shape = (self.B, self.H, self.W, self.C)
        host = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        host_free = [threading.Event() for _ in range(2)]
        for e in host_free:
            e.set()
        work, failed = queue.Queue(), []

        def writer():
            while True:
                item = work.get()
                if item is None:
                    return
                slot, done, s, n = item
                try:
                    if not failed:
                        done.synchronize()
                        sink(s, host[slot].numpy()[:n], labels_host(first + s, n, self.n_classes, self.fixed_label))
                except BaseException as e:          # surfaced in the caller
                    failed.append(e)
                finally:
                    host_free[slot].set()

        th = threading.Thread(target=writer, daemon=True)
        th.start()
        copied = None                               # the D2H copy of the batch before: the next batch overwrites the device bytes
        try:
            for k, (s, n) in enumerate(blocks):
                if failed:
                    break
                if copied is not None:
                    main.wait_event(copied)
                b = self.device_batch(first + s, n)
                ready = torch.cuda.Event()
                ready.record(main)
                if float_sink is not None:          # measurement aid: a blocking copy
                    float_sink(s, b["f32"].cpu().numpy())
                slot = k % 2
                host_free[slot].wait()              # the writer has emptied this pinned buffer (batch k - 2)
                host_free[slot].clear()
                with torch.cuda.stream(side):
                    side.wait_event(ready)
                    host[slot][:n].copy_(b["u8"], non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(side)
                work.put((slot, copied, s, n))
        finally:
            work.put(None)
            th.join()
            torch.cuda.synchronize(self.device)
        if failed:
            raise failed[0]


# ---- sinks ---------------------------------------------------------------------------------------------------------------------------

class CacheWriter:
    """The cache of pipeline.build_cache, written block by block: `<path>.u8` (open_memmap [n, H, W, C] uint8), `<path>.labels.npy`,
    `<path>.json` with the usual header plus a "generator" block that says where the rows came from."""

    def __init__(self, path, n, H, W, C, signed, generator_info):
        self.path, self.n = path, int(n)
        self.u8p, self.labp, self.hdrp = pipeline.cache_paths(path)
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        self.mm = np.lib.format.open_memmap(self.u8p, mode="w+", dtype=np.uint8, shape=(self.n, H, W, C))
        self.labels = np.zeros(self.n, dtype=np.int64)
        self.hdr = {"version": pipeline.CACHE_VERSION, "n": self.n, "H": H, "W": W, "C": C, "signed": bool(signed), "dtype": "uint8",
                    "layout": "NHWC", "generator": dict(generator_info)}

    def __call__(self, start, rows, labels):
        self.mm[start:start + len(rows)] = rows
        self.labels[start:start + len(rows)] = labels

    def close(self):
        self.mm.flush()
        del self.mm
        np.save(self.labp, self.labels)
        with open(self.hdrp, "w") as f:
            json.dump(self.hdr, f)
        return self.hdr


class PngWriter:
    """One PNG per sample, `<dir>/<k>.png` with k = number_from + row (gensamples.py:40-41): the row's bytes as an H x W RGB image,
    a single channel repeated three times (what torchvision's save_image writes for one image: make_grid leaves it unpadded).
    limit: only rows < limit are written (None: all)."""

    def __init__(self, out_dir, number_from=1, limit=None):
        os.makedirs(out_dir, exist_ok=True)
        self.dir, self.number_from, self.limit = out_dir, int(number_from), limit

    def __call__(self, start, rows, labels):
        from PIL import Image
        for i, row in enumerate(rows):
            if self.limit is not None and start + i >= self.limit:
                return
            a = np.repeat(row, 3, axis=2) if row.shape[2] == 1 else row
            Image.fromarray(np.ascontiguousarray(a)).save(os.path.join(self.dir, "%d.png" % (self.number_from + start + i)), format="PNG")


def tee(*sinks):
    sinks = [s for s in sinks if s is not None]
    return lambda start, rows, labels: [s(start, rows, labels) for s in sinks] and None
