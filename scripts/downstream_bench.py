"""What `python -m csl_gan_amd.downstream` costs per checkpoint on one MI355X, and what its fit reaches, in ONE process:

  (1) one cslgan_ovr_logreg_eval_f32 call at N = --n, D = 784, K = 10: HIP events around --calls back-to-back calls (both kernels and
      the launch gap between them are inside), on one X (which then lives in the 256 MB Infinity Cache) and rotating over enough
      copies of X that every call reads it from HBM; set against the time to stream X once at the 6.29 TB/s the float4 copy reaches
      (MI355X_MICROARCH.md);
  (2) generate / fit / predict / AUROC of one checkpoint on the device (host clock around work that ends in a synchronise), the solver's
      report, and max|P - P_host| against the float64 host path of csl_gan_amd.classify on the same features;
  (3) the reference's estimator on the host — OneVsRestClassifier(LogisticRegression(solver='lbfgs', multi_class='multinomial',
      random_state=30)), downstream.py:71-72 — fitted on the same features at its default stop and converged (tol=1e-12), with
      predict_proba and roc_curve + auc as downstream.py:48-62 runs them.  Skipped with a note where scikit-learn is absent.

The generator is the conditional MNIST network with perturbed initial weights (no trained run travels with the repository); the test
set is 10000 further samples of it, quantised to bytes like the idx file's.

    python scripts/downstream_bench.py [--n 10000] [--calls 200] [--bs 500] [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csl_gan_amd import classify, downstream, generate, init_util, ops, options  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def timed_calls(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--bs", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", type=options.str2bool, default=True, help="run the float64 host path and scikit-learn too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("downstream_bench.py measures on an MI355X; no device is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="downstream_bench_") + "/"
    opt = options.parse(["MNIST", "-cond", "-o", tmp, "--manual_seed", "77", "--synthetic", "-gd", "cuda:0"])
    G, _ = init_util.init_models(opt, init_D=False)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in G.parameters():
            p.mul_(1.5).add_(torch.randn(p.shape, generator=g).to(p.device) * 0.05)
    say("downstream_bench: %s, N = %d generated samples, D = 784, K = 10, -bs %d" % (torch.cuda.get_device_name(0), a.n, a.bs))

    # ---- (2a) generation ---------------------------------------------------------------------------------------------------------------
    gen = generate.SampleGenerator(G, opt, dev, 77, a.bs, hip_graph=True, keep_float=True)
    downstream.generated_features(gen, a.n)                        # warm-up: the recording
    t_gen = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X, labels = downstream.generated_features(gen, a.n)
        t_gen.append(time.perf_counter() - t0)
    test_u8 = torch.empty((a.n, 784), device=dev, dtype=torch.uint8)          # the test set: samples n .. 2n-1, as bytes
    for s in range(0, a.n, a.bs):
        k = min(a.bs, a.n - s)
        test_u8[s:s + k].copy_(gen.device_batch(a.n + s, k)["u8"].reshape(k, 784))
    test_y = generate.labels_host(a.n, a.n, 10)
    torch.cuda.synchronize()
    gen.release()
    N, D, K = a.n, 784, 10
    yd = torch.from_numpy(labels).to(dev).to(torch.int32)

    # ---- (1) one evaluation ------------------------------------------------------------------------------------------------------------
    U = (torch.randn(D + 1, K, generator=g) * 0.02).to(dev)
    ws = torch.empty(ops.ovr_logreg_ws_floats(N, D), device=dev, dtype=torch.float32)
    loss, grad = ops.ovr_logreg_eval(X, yd, U, ws=ws)
    copies = [X.clone() for _ in range(max(2, int(2 * 256e6 / (N * D * 4)) + 1))]          # twice the Infinity Cache
    same = lambda i: ops.ovr_logreg_eval(X, yd, U, out_loss=loss, out_grad=grad, ws=ws)
    rot = lambda i: ops.ovr_logreg_eval(copies[i % len(copies)], yd, U, out_loss=loss, out_grad=grad, ws=ws)
    for f in (same, rot):
        timed_calls(f, a.calls)
    t_same = [timed_calls(same, a.calls) for _ in range(a.reps)]
    t_rot = [timed_calls(rot, a.calls) for _ in range(a.reps)]
    stream_us = N * D * 4 / HBM_BYTES_PER_S * 1e6
    say("(1) cslgan_ovr_logreg_eval_f32, %d back-to-back calls per window (eval kernel + reduce kernel, launch gap included)" % a.calls)
    say("  same X every call:       %s us per call" % " / ".join("%.1f" % v for v in t_same))
    say("  %2d copies of X in turn:  %s us per call" % (len(copies), " / ".join("%.1f" % v for v in t_rot)))
    say("  X once at 6.29 TB/s: %.1f us (%.1f MB);  ratio %.1fx (rotating), %.1fx (same X)" % (stream_us, N * D * 4 / 1e6, np.median(t_rot) / stream_us,
                                                                                        np.median(t_same) / stream_us))
    del copies

    # ---- (2b) fit, predict, AUROC ------------------------------------------------------------------------------------------------------
    t_fit, t_pred, t_auc = [], [], []
    for _ in range(a.reps):
        clf = classify.OvrLogReg(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = clf.fit(X, yd)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        P = clf.predict_proba(test_u8)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        au = classify.auroc(P, test_y)
        t3 = time.perf_counter()
        t_fit.append(t1 - t0), t_pred.append(t2 - t1), t_auc.append(t3 - t2)
    say("(2) one checkpoint on the device (host clock, synchronised), %d runs" % a.reps)
    say("  generate %s s   fit %s s   predict %s ms   AUROC %s s" % (" / ".join("%.3f" % v for v in t_gen), " / ".join("%.3f" % v for v in t_fit),
                                                                   " / ".join("%.2f" % (1e3 * v) for v in t_pred), " / ".join("%.3f" % v for v in t_auc)))
    say("  solver at gtol_rel %.1e: iterations %s  evaluations %s  stalled %s  max|g| %.3g (stop at %.3g)"
        % (rep["gtol_rel"], rep["iterations"], rep["evaluations"], [k for k, v in enumerate(rep["stalled"]) if v] or "none", max(rep["grad_norm"]), rep["gtol"]))
    say("  micro AUROC %.6f   per class %s" % (au["micro"], " ".join("%.4f" % v for v in au["per_class"])))
    if not a.host:
        return finish(a, lines)

    # ---- the float64 host path on the same features ---------------------------------------------------------------------------------------
    Xh, th = X.cpu().numpy(), test_u8.cpu().numpy()
    t0 = time.perf_counter()
    hclf = classify.OvrLogReg(K)
    hrep = hclf.fit(Xh, labels)
    Ph = hclf.predict_proba(th).numpy()
    t_host = time.perf_counter() - t0
    hau = classify.auroc(Ph, test_y)
    say("  float64 host path: %.1f s, iterations %s;  max|P_device - P_host| = %.3g;  micro AUROC %.6f (device - host %.2e)"
        % (t_host, hrep["iterations"], float(np.abs(P.cpu().numpy().astype(np.float64) - Ph).max()), hau["micro"], au["micro"] - hau["micro"]))

    # ---- (3) the reference's estimator -------------------------------------------------------------------------------------------------
    try:
        from sklearn.linear_model import LogisticRegression
        from sklearn.metrics import auc, roc_curve
        from sklearn.multiclass import OneVsRestClassifier
        from sklearn.preprocessing import label_binarize
    except ImportError:
        say("(3) scikit-learn is not installed: the reference's estimator was not measured")
        return finish(a, lines)
    hot = label_binarize(test_y, classes=list(range(K)))
    tf = th.astype(float) / 255.0
    say("(3) the reference's estimator on the host (scikit-learn, %d threads visible)" % (os.cpu_count() or 0))
    for name, kw in (("default stop", {}), ("converged (tol=1e-12, max_iter=20000)", {"tol": 1e-12, "max_iter": 20000})):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est = OneVsRestClassifier(LogisticRegression(solver="lbfgs", multi_class="multinomial", random_state=30, **kw))
            t0 = time.perf_counter()
            est.fit(Xh, labels)
            t1 = time.perf_counter()
            Ps = est.predict_proba(tf)
            t2 = time.perf_counter()
            fpr, tpr, _ = roc_curve(hot.ravel(), Ps.ravel())
            micro = auc(fpr, tpr)
            for k in range(K):
                f, t, _ = roc_curve(hot[:, k], Ps[:, k])
                auc(f, t)
            t3 = time.perf_counter()
        say("  %-38s fit %.2f s  predict %.3f s  AUROC %.3f s  iterations %s  micro AUROC %.6f  max|P - P_host| %.3g  max|P - P_device| %.3g"
            % (name, t1 - t0, t2 - t1, t3 - t2, [int(e.n_iter_[0]) for e in est.estimators_], micro, float(np.abs(Ps - Ph).max()),
               float(np.abs(Ps - P.cpu().numpy()).max())))
        say("  %-38s device fit + predict + AUROC %.3f s: %.1fx" % ("", np.median(t_fit) + np.median(t_pred) + np.median(t_auc),
                                                                  (t3 - t0) / (np.median(t_fit) + np.median(t_pred) + np.median(t_auc))))
    return finish(a, lines)


def finish(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
