"""What the membership-inference audit costs on one MI355X, two measurements in ONE process:

  (1) images/s of csl_gan_amd.audit.CriticScorer on the CelebA-64 critic at -bs 1000, recorded graph against eager, alternated
      A/B/A/B.  "end to end" is a host clock around score(cache) — uint8 gather into pinned memory, H2D, cslgan_u8_to_f32_nhwc, D,
      the values back on the host; "device only" is what HIP events see for the same number of batches over the static buffers with
      nothing crossing the bus (launch gaps of the eager path are inside it: an upper bound of kernel time, not kernel time).
  (2) the attack-success-rate estimate: --trials trials at N = 60000, M = 10000, n = 100, m = 900 in cslgan_attack_trials (HIP events,
      warm-up first, median and min of --reps launches), against the reference's host estimator on the same box.  The reference's
      attack() / _get_random_subset() (mem_inf_attack.py:29-66) are restated below as `host_attack`: per trial a list -> array
      conversion of all N values, np.random.choice(range(N), size=k, replace=False) — a permutation of all N indices — for either
      side, and a Python sort of the 1000 (value, flag) pairs.  It is timed over --host_trials trials and scaled to --trials.

    python scripts/attack_bench.py [--images 16000] [--rounds 2] [--trials 10000] [--reps 5] [--host_trials 100] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import audit, init_util, ops, options  # noqa: E402
from csl_gan_amd.pipeline import CachedImages  # noqa: E402


def host_attack(values_train, values_nontrain, data_prop=0.1):
    """One trial of the reference's estimator, written the way it works: lists in, a fresh subset of either side through
    np.random.choice over range(len), pairs sorted by value (descending, stable), the share of train flags among the first n."""
    n, m = int(1000 * data_prop), int(1000 * (1 - data_prop))

    def subset(collection, k):
        idx = np.random.choice(range(len(collection)), size=k, replace=False)
        return np.array(collection)[idx].tolist()

    pairs = [(v, 1) for v in subset(values_train, n)] + [(v, 0) for v in subset(values_nontrain, m)]
    best = sorted(pairs, key=lambda p: p[0], reverse=True)[:n]
    return float(np.mean([flag for _, flag in best]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=1000)
    ap.add_argument("--images", type=int, default=16000, help="images per timed window")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--trials", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host_trials", type=int, default=100)
    ap.add_argument("--compute_dtype", default="fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("attack_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="attack_bench_") + "/"
    opt = options.parse(["CelebA", "-dpm", "gc", "-gcm", "adaptive-pl", "-nms", "4", "-gd", "cuda:0", "-dd", "cuda:0", "-o", tmp, "--manual_seed", "1",
                         "--synthetic", "--compute_dtype", a.compute_dtype])
    _, D = init_util.init_models(opt, init_G=False)
    say("attack_bench: CelebA-64 critic (%.1f M parameters), compute_dtype %s, -bs %d, %d images per window, %d rounds, %s"
        % (sum(p.numel() for p in D.parameters()) / 1e6, a.compute_dtype, a.bs, a.images, a.rounds, torch.cuda.get_device_name(0)))

    # ---- (1) scoring -----------------------------------------------------------------------------------------------------------------
    nb = max(a.images // a.bs, 2)
    rng = np.random.default_rng(0)
    cache = CachedImages.from_arrays(rng.integers(0, 256, size=(nb * a.bs, 64, 64, 3), dtype=np.uint8), np.zeros(nb * a.bs, np.int64), True)
    scorers = {"graph": audit.CriticScorer(D, opt, dev, a.bs, hip_graph=True, compute_dtype=a.compute_dtype),
               "eager": audit.CriticScorer(D, opt, dev, a.bs, hip_graph=False, compute_dtype=a.compute_dtype)}

    def device_only(sc):
        b = sc._static
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(nb):
            if sc.graph is not None:
                sc.graph.replay()
            else:
                sc._steps(b, cache.scale, cache.bias)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3

    res = {k: {"e2e": [], "dev": []} for k in scorers}
    values = {}
    for k, sc in scorers.items():                                # warm-up: allocator, workspaces, the recording
        values[k] = sc.score(cache)
        device_only(sc)
    for _ in range(a.rounds):
        for k, sc in scorers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.score(cache)
            res[k]["e2e"].append(nb * a.bs / (time.perf_counter() - t0))
            res[k]["dev"].append(nb * a.bs / device_only(sc))
    say("(1) CriticScorer, %d batches (%d images) per window" % (nb, nb * a.bs))
    for k in scorers:
        e, d = res[k]["e2e"], res[k]["dev"]
        say("  %-5s end to end %s images/s (mean %.0f)   device only %s images/s (mean %.0f, %.3f ms per batch)"
            % (k, " / ".join("%.0f" % v for v in e), np.mean(e), " / ".join("%.0f" % v for v in d), np.mean(d), 1e3 * a.bs / np.mean(d)))
    say("  graph / eager: end to end %.2fx, device only %.2fx;  largest score difference %.2e of max |score| %.3f"
        % (np.mean(res["graph"]["e2e"]) / np.mean(res["eager"]["e2e"]), np.mean(res["graph"]["dev"]) / np.mean(res["eager"]["dev"]),
           float(np.abs(values["graph"] - values["eager"]).max()) / float(np.abs(values["eager"]).max()), float(np.abs(values["eager"]).max())))
    for sc in scorers.values():
        sc.release()

    # ---- (2) the estimate ------------------------------------------------------------------------------------------------------------
    N, M, n, m = 60000, 10000, 100, 900
    vt, vn = (rng.standard_normal(N) + 0.5).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    dt, dn = torch.from_numpy(vt).to(dev), torch.from_numpy(vn).to(dev)
    hits = torch.empty(a.trials, device=dev, dtype=torch.int32)
    for _ in range(2):
        ops.attack_trials(dt, dn, n, m, 1, 0, a.trials, out=hits)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.attack_trials(dt, dn, n, m, 1, 0, a.trials, out=hits)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    h = hits.cpu().numpy()
    say("(2) %d trials at N=%d M=%d n=%d m=%d (%d + %d swap-or-not rounds per element)" % (a.trials, N, M, n, m, audit.shuffle_rounds(N), audit.shuffle_rounds(M)))
    say("  cslgan_attack_trials: median %.3f ms, min %.3f ms of %d launches (%.2f us per trial);  ASR %.4f +- %.4f"
        % (np.median(times), np.min(times), a.reps, 1e3 * np.median(times) / a.trials, h.mean() / n, h.std(ddof=1) / (n * np.sqrt(a.trials))))
    lt, ln = vt.tolist(), vn.tolist()
    np.random.seed(1)
    host_attack(lt, ln)
    t0 = time.perf_counter()
    rates = [host_attack(lt, ln) for _ in range(a.host_trials)]
    per = (time.perf_counter() - t0) / a.host_trials
    say("  reference estimator on the host: %.2f ms per trial over %d trials = %.1f s per %d trials (scaled);  ASR %.4f +- %.4f"
        % (1e3 * per, a.host_trials, per * a.trials, a.trials, np.mean(rates), np.std(rates, ddof=1) / np.sqrt(a.host_trials)))
    say("  host / device: %.0fx" % (per * a.trials * 1e3 / np.median(times)))
    t0 = time.perf_counter()
    audit.trial_hits(vt, vn, n, m, 1, 0, 8)
    say("  host model of the device sampler (numpy, csl_gan_amd.audit.trial_hits): %.0f ms per trial" % (1e3 * (time.perf_counter() - t0) / 8))
    assert np.array_equal(h[:8], audit.trial_hits(vt, vn, n, m, 1, 0, 8))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
