"""The command line on one MI355X (-m gpu): the reference's smoke matrix (test_configs.sh: {MNIST, CelebA} x {gc, is} x
{unconditional, conditional}) on synthetic data with the DEFAULT launch mode (HIP-graph replay of the gc D-step, eager generator
steps in between), and checkpoint + resume of a graph-replayed run."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(tmp_path, argv):
    from csl_gan_amd import train
    return train.main(argv + ["-gd", "cuda:0", "-dd", "cuda:0", "-o", str(tmp_path), "--synthetic", "--manual_seed", "7"])


@pytest.mark.parametrize("dataset", ["MNIST", "CelebA"])
@pytest.mark.parametrize("mode", ["gc", "is"])
@pytest.mark.parametrize("cond", [False, True])
def test_cli_smoke_matrix(tmp_path, dataset, mode, cond):
    bs, iters = 32, 9
    tr = _run(tmp_path, [dataset, "-tss", "1000", "-dpm", mode, "-nms", "1", "--mean_sample_size", "10", "-bs", str(bs), "--max_iters", str(iters),
                         "--log_every", str(bs * 3)] + (["--conditional"] if cond else []))
    torch.cuda.synchronize()
    assert tr.privacy_engine.steps == iters
    assert tr.graphed is not None and tr.graphed.graph is not None, "the D-step should have been recorded and replayed"
    for p in list(tr.D.parameters()) + list(tr.G.parameters()):
        assert torch.isfinite(p).all()
    rows = open(os.path.join(str(tmp_path), "log.csv")).read().strip().splitlines()
    assert len(rows) >= 3 and "nan" not in rows[-1].lower()      # header + one line per 3 iterations


def test_cli_checkpoint_and_resume_with_graph_replay(tmp_path):
    """resuming a --hip_graph run raised at the first D-step (the device step counter came back from the checkpoint as a
    float).  Train one epoch with replayed D-steps, save, resume for another epoch: the optimizer state has torch's Adam layout, the
    engine's step count and Philox counter and the mean sampler's draw stream continue."""
    base = ["MNIST", "--model", "DeepConvResNet", "--penalty", "WGAN-GP", "-tss", "256", "-dpm", "gc", "-nms", "2", "--mean_sample_size", "10",
            "-bs", "32", "--save_every", "1", "--log_every", "64", "--g_latent_dim", "16"]
    tr = _run(tmp_path, base + ["-ne", "1"])
    assert tr.graphed is not None and tr.graphed.graph is not None
    steps1, draws1 = tr.privacy_engine.steps, tr.mean_sampler._draws
    assert steps1 == 8 and draws1 > 0
    ck = torch.load(os.path.join(str(tmp_path), "saves", "D-1"), weights_only=True)
    for st in ck["optimizer_state_dict"]["state"].values():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
    with open(os.path.join(str(tmp_path), "saves", "PE-1.json")) as f:
        pe_state = json.load(f)
    assert pe_state["steps"] == steps1 and pe_state["mean_sampler"]["draws"] == draws1
    from csl_gan_amd import train
    tr2 = train.main(["MNIST", "-rp", str(tmp_path), "-re", "1", "-gd", "cuda:0", "-dd", "cuda:0", "-ne", "2", "-ka", "n_epochs"])
    torch.cuda.synchronize()
    assert tr2.privacy_engine.steps == 2 * steps1 and tr2.mean_sampler._draws > draws1
    assert tr2.graphed is not None and tr2.graphed.graph is not None
    # the reference re-creates both optimizers after the warm-up loop (train.py:572), i.e. AFTER load_model restored their state
    # (train.py:79-82): Adam's moments restart on resume there and here (the optimizer round trip itself is
    # test_graph_gpu.py::test_capturable_adam_checkpoint_roundtrip)
    assert all(st["step"] == steps1 for st in tr2.d_optimizer.state.values())
    assert all(torch.isfinite(p).all() for p in tr2.D.parameters())


@pytest.mark.parametrize("extra", [["--im_size", "128"], ["--conditional"], ["-dpm", "is"]])
def test_cli_bf16_storage(tmp_path, extra):
    """BASELINE configs[4] from the command line: --compute_dtype bf16 --storage_dtype bf16 (bf16-stored activations of the critic and of
    the frozen generator, eager generator steps differentiating through them) — the 128x128 extension, the conditional (ACGAN) critic
    whose first layer sees label planes, and the immediate-sensitivity engine's double backward."""
    bs, iters = 16, 7
    argv = ["CelebA", "-tss", "1000", "-nms", "1", "--mean_sample_size", "10", "-bs", str(bs), "--max_iters", str(iters), "--log_every", str(bs * 3),
            "--compute_dtype", "bf16", "--storage_dtype", "bf16"]
    if "-dpm" not in extra:
        argv += ["-dpm", "gc"]
    tr = _run(tmp_path, argv + extra)
    torch.cuda.synchronize()
    from csl_gan_amd import ops
    assert ops.get_storage_dtype() == "bf16" and tr.privacy_engine.steps == iters
    for p in list(tr.D.parameters()) + list(tr.G.parameters()):
        assert torch.isfinite(p).all()
    rows = open(os.path.join(str(tmp_path), "log.csv")).read().strip().splitlines()
    assert len(rows) >= 3 and "nan" not in rows[-1].lower()


def test_storage_dtype_needs_bf16_compute(tmp_path):
    from csl_gan_amd import options
    with pytest.raises(Exception, match="needs --compute_dtype bf16"):
        options.parse(["CelebA", "-dpm", "gc", "-nms", "1", "-bs", "4", "-gd", "cuda:0", "-dd", "cuda:0", "-o", str(tmp_path), "--storage_dtype", "bf16"])


def test_bench_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`, a plain run: one JSON line with the headline fields and none of
    --full's, its figures from exactly K replayed steps; DIR holds what the last timed step computed as float32 .npy files within
    64 MB, and a second run with the same arguments computes the same numbers from the same inputs.

    "The same" to the step's own reproducibility: the generated images depend on the seeded draws alone and come out bitwise equal;
    the critic's reductions (per-sample norms, split-K sums) add with floating-point atomics, so its scores, losses and clip
    statistics agree to rounding (measured <= 8e-5 of each array's scale), and Adam's per-coordinate normalisation magnifies such
    differences in its parameters step by step (measured <= 6.2e-4 after the 7 critic steps of this run, 2 eager + recording +
    4 replays)."""
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines, dumps = [], []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        ls = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(ls) == 1, r.stdout[-2000:]
        lines.append(json.loads(ls[0]))
        dumps.append(d)
    line = lines[0]
    assert (line["steps"], line["warmup"], line["n_gpus"], line["unit"], line["dtype"]) == (3, 2, 1, "images/sec", "f32"), line
    assert line["higher_is_better"] is True and line["config"]["launch"] == "hip_graph" and line["graph_error"] is None, line
    assert abs(line["value"] - 128 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"], line
    for k in ("cpu_baseline", "variants", "secondary", "roofline", "kernels_ms_per_step"):
        assert k not in line, k
    files = sorted(os.listdir(dumps[0]))
    assert files == sorted(os.listdir(dumps[1])) and {"last.fake_img.npy", "last.d_real_loss.npy"} <= set(files), files
    assert any(f.startswith("D.") for f in files) and sum(os.path.getsize(dumps[0] / f) for f in files) <= 64 << 20
    assert np.load(dumps[0] / "last.fake_img.npy").shape == (128, 3, 64, 64)
    for f in files:
        x, y = np.load(dumps[0] / f), np.load(dumps[1] / f)
        assert x.dtype == np.float32 and x.shape == y.shape and np.isfinite(x).all(), f
        tol = 1e-6 if f == "last.fake_img.npy" else 1e-2 if f.startswith("D.") else 1e-3
        assert np.abs(x.astype(np.float64) - y).max() <= tol * max(float(np.abs(x).max()), 1e-6), f
