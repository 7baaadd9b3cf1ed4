"""The downstream classifier of a conditional MNIST run (reference downstream.py:48-88): a one-vs-rest logistic regression fitted
on generated samples, its probabilities on a real test set, and their micro-averaged and per-class AUROC.

  * the objective.  downstream.py:71-72 builds OneVsRestClassifier(LogisticRegression(solver='lbfgs', multi_class='multinomial')):
    every estimator gets a binary target, for which the multinomial form is a two-class softmax — a binary logistic regression
    with C = 2.  Class k minimises  f_k = sum_i log(1 + exp(-s_ik z_ik)) + ||u_k||^2 / 4,  z = X u_k + b_k,  s = +-1, the intercept
    unpenalised (include/cslgan.h "downstream classifier").  `objective_host` is THE definition, in float64;
  * the fit.  f_k is strictly convex, so its minimiser is unique and `OvrLogReg.fit` looks for that, not for the point at which
    SciPy's L-BFGS happens to stop with the reference's tol=1e-4 / max_iter=100.  One L-BFGS (10 pairs) drives all K columns at
    once: own history, step and backtracking per column, one objective evaluation — on a HIP device one cslgan_ovr_logreg_eval_f32
    call, one pass over X — for all columns per trial point; a column that has converged is frozen;
  * the probabilities, P[i, k] = sigmoid(z_ik) / sum_k' sigmoid(z_ik') (OneVsRestClassifier.predict_proba), and
  * `auroc`: auc(roc_curve(...)) of downstream.py:48-62 is the Mann-Whitney statistic with ties counted half, which
    csl_gan_amd.audit.rank_metrics computes exactly from integer rank counts (cslgan_rank_counts on a device).

Every piece has a host path (float64 torch) and a device path (fp32, csrc/logreg_kernels.hip) with the same definition.

The `*_bytes` forms (csl_gan_amd.tstr) are the same estimator on uint8 cache rows, x = byte / 255, for any row size
1 .. 65536: `objective_host_bytes` is THE definition, `OvrLogReg.fit_bytes` / `predict_proba_bytes` run it through
cslgan_ovr_logreg_eval_u8 / cslgan_ovr_logreg_proba_u8 on a device, and `accuracy` is the argmax hit count.

`OvrMlp` is the reference's second classifier, OneVsRestClassifier(MLPClassifier(alpha=1)) of downstream.py:82, on the
same byte rows: one hidden ReLU layer per class, `objective_mlp_host_bytes` / `proba_mlp_host_bytes` THE definition, the same
`lbfgs_columns`, cslgan_ovr_mlp_eval_u8 / cslgan_ovr_mlp_proba_u8 (csrc/mlp_kernels.hip) on a device.

`NaiveBayes` is GaussianNB() and BernoulliNB(alpha=.01) of downstream.py:76-78 on the same byte rows: closed forms of
per-class, per-feature moments, which on bytes are integers — `class_moments_host_bytes` THE definition, equalled exactly by
cslgan_class_moments_u8 — and one derivation of the tables on the host for both paths (`gnb_tables`, `bnb_tables`), so a host fit
and a device fit are the same bits; `jll_host_bytes` is the float64 model of cslgan_nb_score_gauss_u8 / _bern_u8 (csrc/nb_kernels.hip).

`Trees` is DecisionTreeClassifier() and RandomForestClassifier(n_estimators=100) of downstream.py:69-74, one-vs-rest, on
the same byte rows: a threshold is a byte and a node's statistic a 256-bin integer histogram per feature, so the fit is integer-exact
— `best_split_host_bytes` THE definition of the split search, equalled in every integer and in the score's bits by
cslgan_tree_best_split_u8 (csrc/tree_kernels.hip), `tree_apply_host_bytes` that of cslgan_tree_apply_u8 — and one level loop in torch for
both paths, so a host fit and a device fit are the same trees.

`AdaBoost` is AdaBoostClassifier() of downstream.py:79-80, one-vs-rest, on the same byte rows: rounds of depth-1 trees
under fixed-point row weights 0 .. 2^28, so every sum of a round is an exact integer — `boost_stump_host_bytes` THE definition of the
stump search, equalled in every integer and in the score's bits by cslgan_boost_stump_u8 (csrc/boost_kernels.hip) — and one round loop
in torch for both paths; the stumps score test rows through the tree apply path.

The linear support-vector classifier of downstream.py:67 lives in csl_gan_amd.svm (`OvrSvc`): it scores through
`proba_host_bytes` / cslgan_ovr_logreg_proba_u8 here, Platt's sigmoid of a linear score being a logistic model.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

from . import audit, ops

MAX_CLASSES = 16                   # the 16 columns of the matrix instruction (include/cslgan.h)
MEMORY = 10                        # L-BFGS pairs (SciPy's default maxcor, what the reference's solver keeps)
ARMIJO_C1 = 1e-4
MAX_BACKTRACKS = 30
GTOL_REL_DEVICE = 2e-8             # fp32: max|g_k| <= 2e-8 N.  5e-7 passes the golden test too but leaves 2e-3 in probability on an
                                   # ill-conditioned fit (512 samples of 784 features); DESIGN.md §6f has the runs
GTOL_REL_HOST = 1e-8               # float64: the model the device is held to
MAX_HIDDEN = 128                   # hidden units per class of OvrMlp: H K <= 2048 first-layer columns (include/cslgan.h)


def _check_classes(n_classes):
    n_classes = int(n_classes)
    if not 2 <= n_classes <= MAX_CLASSES:
        raise ValueError("n_classes must lie in 2 .. %d, got %d" % (MAX_CLASSES, n_classes))
    return n_classes


def objective_host(X, labels, U):
    """(loss [K], grad [D + 1, K]) of the K objectives at U [D + 1, K] (last row: the intercepts), float64 torch on the CPU."""
    X, U = torch.as_tensor(X).double(), torch.as_tensor(U).double()
    y = torch.as_tensor(labels).long()
    D, K = X.shape[1], U.shape[1]
    T = (y[:, None] == torch.arange(K)[None, :]).double()
    Z = X @ U[:D] + U[D]
    sz = (2 * T - 1) * Z
    loss = (torch.clamp(-sz, min=0) + torch.log1p(torch.exp(-sz.abs()))).sum(0) + 0.25 * (U[:D] ** 2).sum(0)
    R = torch.sigmoid(Z) - T
    grad = torch.cat([X.t() @ R + 0.5 * U[:D], R.sum(0, keepdim=True)], 0)
    return loss, grad


def _bytes_rows(Xu8):
    X = torch.as_tensor(Xu8)
    if X.dtype != torch.uint8 or X.dim() != 2:
        raise ValueError("need uint8 rows [N, D], got %s %s" % (X.dtype, tuple(X.shape)))
    return X


def objective_host_bytes(Xu8, labels, U, block=2048):
    """(loss [K], grad [D + 1, K]) of the K objectives on byte features x = byte / 255, float64 torch on the CPU, in row blocks of
    `block` (a CelebA-sized cache never becomes one float64 matrix) — THE definition for byte features; equal to
    objective_host(Xu8.double() / 255, labels, U)."""
    X, U = _bytes_rows(Xu8).cpu(), torch.as_tensor(U).double().cpu()
    y = torch.as_tensor(labels).long().reshape(-1).cpu()
    N, D = X.shape
    K = U.shape[1]
    block = max(1, int(block))
    cls = torch.arange(K)[None, :]
    loss = 0.25 * (U[:D] ** 2).sum(0)
    G = torch.zeros((D, K), dtype=torch.float64)
    gb = torch.zeros(K, dtype=torch.float64)
    for r0 in range(0, N, block):
        Xb = X[r0:r0 + block].double() / 255.0
        T = (y[r0:r0 + block, None] == cls).double()
        Z = Xb @ U[:D] + U[D]
        sz = (2 * T - 1) * Z
        loss = loss + (torch.clamp(-sz, min=0) + torch.log1p(torch.exp(-sz.abs()))).sum(0)
        R = torch.sigmoid(Z) - T
        G += Xb.t() @ R
        gb += R.sum(0)
    return loss, torch.cat([G + 0.5 * U[:D], gb[None, :]], 0)


def proba_host_bytes(Xu8, U, block=2048):
    """P [M, K] in float64 of uint8 rows, x = byte / 255, in row blocks."""
    X, U = _bytes_rows(Xu8).cpu(), torch.as_tensor(U).double().cpu()
    out = torch.empty((X.shape[0], U.shape[1]), dtype=torch.float64)
    block = max(1, int(block))
    for r0 in range(0, X.shape[0], block):
        S = torch.sigmoid((X[r0:r0 + block].double() / 255.0) @ U[:-1] + U[-1])
        out[r0:r0 + block] = S / S.sum(1, keepdim=True)
    return out


def _mlp_split(U, D, H):
    """(W1 [D, C], b1 [C], w2 [C], b2 [K]) views of U [(D + 2) H + 1, K], C = H K with column c = h K + k."""
    K = U.shape[1]
    if U.dim() != 2 or H < 1 or U.shape[0] != (D + 2) * H + 1:
        raise ValueError("need U [(D + 2) H + 1, K] with D = %d, H = %d, got %s" % (D, H, tuple(U.shape)))
    C = H * K
    return U[:D * H].reshape(D, C), U[D * H:(D + 1) * H].reshape(C), U[(D + 1) * H:(D + 2) * H].reshape(C), U[-1]


def objective_mlp_host_bytes(Xu8, labels, U, hidden, alpha=1.0, block=2048):
    """(loss [K], grad like U) of K one-vs-rest networks with `hidden` ReLU units each on byte features x = byte / 255, float64
    torch on the CPU, in row blocks of `block` — THE definition of csl_gan_amd.classify.OvrMlp.

    U [(D + 2) H + 1, K]: row d H + h is W1[d][h], rows D H + h are b1, rows (D + 1) H + h are w2, the last row is b2; a column is
    one class.  Z1 = (bytes W1) / 255 + b1 (the bytes enter as the integers 0 .. 255 and 1 / 255 is applied once to each sum, so a sum
    that is exactly zero stays exactly zero), A = max(Z1, 0), z = sum_h A w2 + b2, t = [label == k] (labels outside 0 .. K-1
    belong to no class), s = 2 t - 1,
        f_k = sum_i log(1 + exp(-s z)) + (alpha / 2) (||W1_k||^2 + ||w2_k||^2)
    — N times scikit-learn's MLPClassifier loss on a binary target, intercepts unpenalised.  R = sigmoid(z) - T,
    dZ1 = [Z1 > 0] w2 R (the derivative at exactly 0 is 0), dW1 = X^T dZ1 + alpha W1, db1 = sum_i dZ1, dw2 = sum_i A R + alpha w2,
    db2 = sum_i R."""
    X, U = _bytes_rows(Xu8).cpu(), torch.as_tensor(U).double().cpu()
    y = torch.as_tensor(labels).long().reshape(-1).cpu()
    N, D = X.shape
    H, K, alpha = int(hidden), U.shape[1], float(alpha)
    W1, b1, w2, b2 = _mlp_split(U, D, H)
    C = H * K
    block = max(1, int(block))
    cls = torch.arange(K)[None, :]
    loss = 0.5 * alpha * ((W1 ** 2).reshape(D * H, K).sum(0) + (w2 ** 2).reshape(H, K).sum(0))
    G1 = torch.zeros((D, C), dtype=torch.float64)
    gb1, gw2 = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    gb2 = torch.zeros(K, dtype=torch.float64)
    for r0 in range(0, N, block):
        Xb = X[r0:r0 + block].double()                                    # the integers 0 .. 255
        T = (y[r0:r0 + block, None] == cls).double()
        Z1 = (Xb @ W1) / 255.0 + b1
        A = torch.clamp(Z1, min=0)
        Z = (A * w2).reshape(-1, H, K).sum(1) + b2
        sz = (2 * T - 1) * Z
        loss = loss + (torch.clamp(-sz, min=0) + torch.log1p(torch.exp(-sz.abs()))).sum(0)
        R = torch.sigmoid(Z) - T
        Rc = R.repeat(1, H)                                               # [n, C]: column c = h K + k holds R[:, k]
        dZ1 = (Z1 > 0).double() * w2 * Rc
        G1 += Xb.t() @ dZ1
        gb1 += dZ1.sum(0)
        gw2 += (A * Rc).sum(0)
        gb2 += R.sum(0)
    grad = torch.cat([(G1 / 255.0 + alpha * W1).reshape(D * H, K), gb1.reshape(H, K), (gw2 + alpha * w2).reshape(H, K), gb2[None, :]], 0)
    return loss, grad


def proba_mlp_host_bytes(Xu8, U, hidden, block=2048):
    """P [M, K] in float64 of uint8 rows under the networks of objective_mlp_host_bytes: sigmoid(z) / sum_k sigmoid(z), in row blocks."""
    X, U = _bytes_rows(Xu8).cpu(), torch.as_tensor(U).double().cpu()
    H, K = int(hidden), U.shape[1]
    W1, b1, w2, b2 = _mlp_split(U, X.shape[1], H)
    out = torch.empty((X.shape[0], K), dtype=torch.float64)
    block = max(1, int(block))
    for r0 in range(0, X.shape[0], block):
        A = torch.clamp((X[r0:r0 + block].double() @ W1) / 255.0 + b1, min=0)
        S = torch.sigmoid((A * w2).reshape(-1, H, K).sum(1) + b2)
        out[r0:r0 + block] = S / S.sum(1, keepdim=True)
    return out


def accuracy(P, y):
    """{"hits", "n", "accuracy"} of scores P [M, K] against labels y [M]: the prediction is the argmax over the classes, ties to the
    smallest class index; hits is the integer numerator."""
    P = (P.detach().cpu() if torch.is_tensor(P) else torch.from_numpy(np.asarray(P)))
    y = torch.as_tensor(y).reshape(-1).long().cpu()
    if P.dim() != 2 or y.numel() != P.shape[0] or P.shape[0] < 1:
        raise ValueError("need P [M, K] and y [M], got %s and %s" % (tuple(P.shape), tuple(y.shape)))
    best = P.max(1, keepdim=True)[0]
    cls = torch.arange(P.shape[1])[None, :].expand_as(P)
    pred = torch.where(P == best, cls, torch.full_like(cls, P.shape[1])).min(1)[0]      # the first maximum
    hits, n = int((pred == y).sum()), int(P.shape[0])
    return {"hits": hits, "n": n, "accuracy": hits / n}


def proba_host(Xtest, U):
    """P [M, K] in float64; uint8 rows are bytes / 255 (downstream.py:106)."""
    Xtest = torch.as_tensor(Xtest)
    X = Xtest.double() / 255.0 if Xtest.dtype == torch.uint8 else Xtest.double()
    U = torch.as_tensor(U).double()
    S = torch.sigmoid(X @ U[:-1] + U[-1])
    return S / S.sum(1, keepdim=True)


def lbfgs_columns(evaluate, U0, n_rows, gtol_rel, max_iter, memory=MEMORY):
    """Minimise K independent objectives that share one evaluation.  evaluate(U [P, K]) -> (loss [K], grad [P, K]), fresh tensors of
    U0's dtype and device.  Column k: own history of `memory` pairs, own step, own Armijo backtracking (halving from t = 1; the first
    iteration starts from 1 / max(1, ||g_k||)); it stops when max|g_k| <= gtol_rel * n_rows, after max_iter iterations, or when its
    line search finds no decrease within MAX_BACKTRACKS halvings — then it is `stalled` and stays where it was.  Next to the Armijo
    test a trial point is accepted when its loss equals the old one to within two units of the dtype's rounding of the loss AND the
    slope along the direction has shrunk (|g_new . p| <= 0.9 |g . p|): close to the minimiser of an fp32 objective the decrease of
    a good step is below what the loss can show, and the gradient still can.  Every trial point of every active column goes into
    ONE evaluate call.  Returns (U, report)."""
    U = U0.clone()
    P, K = U.shape
    dev, dt = U.device, U.dtype
    eps = torch.finfo(dt).eps
    f, g = evaluate(U)
    gtol = float(gtol_rel) * float(n_rows)
    S = torch.zeros((memory, P, K), device=dev, dtype=dt)
    Y = torch.zeros((memory, P, K), device=dev, dtype=dt)
    rho = torch.zeros((memory, K), device=dev, dtype=dt)
    gamma = torch.ones(K, device=dev, dtype=dt)
    active = g.abs().amax(0) > gtol
    stalled = torch.zeros(K, device=dev, dtype=torch.bool)
    iters = torch.zeros(K, device=dev, dtype=torch.int64)
    evals = torch.ones(K, device=dev, dtype=torch.int64)
    n_pairs, it = 0, 0
    while it < max_iter and bool(active.any()):
        # two-loop recursion, all columns at once; slot order: oldest .. newest = 0 .. n_pairs - 1
        q = g.clone()
        alphas = []
        for i in range(n_pairs - 1, -1, -1):
            a = rho[i] * (S[i] * q).sum(0)
            q -= a * Y[i]
            alphas.append(a)
        r = gamma * q
        for i in range(n_pairs):
            b = rho[i] * (Y[i] * r).sum(0)
            r += S[i] * (alphas[n_pairs - 1 - i] - b)
        p = -r
        gp = (g * p).sum(0)
        bad = active & ~(gp < 0)                       # no descent direction (rounding): steepest descent for that column
        if bool(bad.any()):
            p = torch.where(bad, -g, p)
            gp = (g * p).sum(0)
        t = torch.ones(K, device=dev, dtype=dt)
        if it == 0:
            t = 1.0 / torch.clamp(g.norm(dim=0), min=1.0)
        t = torch.where(active, t, torch.zeros_like(t))
        todo = active.clone()                          # columns whose trial point is not accepted yet
        Un, fn, gn = U, f, g
        for _ in range(MAX_BACKTRACKS + 1):
            Ut = U + t * p
            ft, gt_ = evaluate(Ut)
            evals += active.long()
            armijo = ft <= f + ARMIJO_C1 * t * gp
            flat = (ft <= f + 2 * eps * f.abs()) & ((gt_ * p).sum(0).abs() <= 0.9 * gp.abs())
            ok = todo & (armijo | flat)
            Un = torch.where(ok, Ut, Un)
            fn = torch.where(ok, ft, fn)
            gn = torch.where(ok, gt_, gn)
            todo = todo & ~ok
            if not bool(todo.any()):
                break
            t = torch.where(todo, 0.5 * t, torch.where(active, t, torch.zeros_like(t)))
            # accepted columns are evaluated again at their accepted point: Ut = U + t p with their t unchanged
        moved = active & ~todo
        stalled |= todo
        s, y = Un - U, gn - g
        sy, yy = (s * y).sum(0), (y * y).sum(0)
        good = moved & (sy > eps * yy) & (yy > 0)
        if n_pairs == memory:
            S, Y, rho = S.roll(-1, 0), Y.roll(-1, 0), rho.roll(-1, 0)
            n_pairs -= 1
        S[n_pairs], Y[n_pairs] = torch.where(good, s, torch.zeros_like(s)), torch.where(good, y, torch.zeros_like(y))
        rho[n_pairs] = torch.where(good, 1.0 / torch.where(good, sy, torch.ones_like(sy)), torch.zeros_like(sy))
        gamma = torch.where(good, sy / torch.where(good, yy, torch.ones_like(yy)), gamma)
        n_pairs += 1
        U, f, g = Un, fn, gn
        iters += moved.long()
        active = moved & (g.abs().amax(0) > gtol)
        it += 1
    gmax = g.abs().amax(0)
    report = {"iterations": iters.tolist(), "evaluations": evals.tolist(), "grad_norm": [float(v) for v in gmax.tolist()],
              "stalled": [bool(v) for v in stalled.tolist()], "converged": [bool(v) for v in (gmax <= gtol).tolist()],
              "gtol": gtol, "loss": [float(v) for v in f.tolist()]}
    return U, report


def _check_rows(K, X, y):
    """What a fit on rows refuses: shapes that do not match, and a class of 0 .. K-1 without a training sample."""
    if X.dim() != 2 or y.numel() != X.shape[0]:
        raise ValueError("need X [N, D] and y [N], got %s and %s" % (tuple(X.shape), tuple(y.shape)))
    counts = np.bincount(y.detach().cpu().numpy().astype(np.int64).reshape(-1), minlength=K)
    if len(counts) > K or (counts[:K] == 0).any():
        raise ValueError("every class 0 .. %d needs a training sample; counts: %s" % (K - 1, counts.tolist()))


def _fit(est, X, y, host_objective, device_objective, ws_floats, start):
    """The fit of both estimators on rows X [N, D] and labels y from U0 = start(D), float64 on the host; stores est.coef and
    est.report and returns the report.  X on a HIP device: fp32 — int32 labels, ONE workspace of ws_floats(N, D) floats for all
    evaluations, U0 rounded to float32, device_objective(X, labels, U, ws) per trial point, GTOL_REL_DEVICE unless the estimator
    has its own gtol_rel.  Anything else: float64 — host_objective(X, labels, U) and GTOL_REL_HOST."""
    y = torch.as_tensor(y)
    _check_rows(est.K, X, y)
    N, D = X.shape
    U0 = start(D)
    if X.is_cuda:
        with torch.cuda.device(X.device):
            yd = y.to(X.device).reshape(-1).to(torch.int32).contiguous()
            ws = torch.empty(ws_floats(N, D), device=X.device, dtype=torch.float32)
            ev = lambda U: device_objective(X, yd, U.contiguous(), ws)
            gtol_rel = GTOL_REL_DEVICE if est.gtol_rel is None else est.gtol_rel
            U, rep = lbfgs_columns(ev, U0.to(X.device, torch.float32), N, gtol_rel, est.max_iter)
    else:
        yh = y.long().reshape(-1)
        gtol_rel = GTOL_REL_HOST if est.gtol_rel is None else est.gtol_rel
        U, rep = lbfgs_columns(lambda U: host_objective(X, yh, U), U0, N, gtol_rel, est.max_iter)
    rep["gtol_rel"] = float(gtol_rel)
    est.coef, est.report = U, rep
    return rep


def _proba(est, X, host_proba, device_proba):
    """P [M, K] of a fitted estimator: device_proba(X, its coefficients in fp32 on X's device) for rows on a HIP device,
    host_proba(X, its coefficients on the host) for anything else."""
    if est.coef is None:
        raise RuntimeError("fit first")
    if X.is_cuda:
        with torch.cuda.device(X.device):
            return device_proba(X, est.coef.to(X.device, torch.float32).contiguous())
    return host_proba(X, est.coef.cpu())


def solver_line(report):
    """The "solver:" line that tstr and downstream print under a fit's figures."""
    return "   solver: iterations %s  evaluations %s  max|g| %.3g (stop at %.3g)  stalled %s" % (
        report["iterations"], report["evaluations"], max(report["grad_norm"]), report["gtol"],
        [k for k, v in enumerate(report["stalled"]) if v] or "none")


class OvrLogReg:
    """`OvrLogReg(n_classes).fit(X, y)` then `.predict_proba(Xtest)`.

    fit: X [N, D] floats, y [N] integer labels.  X on a HIP device selects the device path (fp32, ops.ovr_logreg_eval); anything
    else — numpy, CPU tensors — the host path (float64).  Returns the solver's report: per column the iteration count, the
    evaluation count, the final max|g| and the stall flag.  `coef` is U [D + 1, K], the intercepts in the last row.
    predict_proba: Xtest [M, D] floats or uint8 bytes (scaled by 1 / 255); the path follows Xtest's device; float32 [M, K] on a device,
    float64 on the host."""

    def __init__(self, n_classes, gtol_rel=None, max_iter=2000):
        self.K = _check_classes(n_classes)
        self.gtol_rel, self.max_iter = gtol_rel, int(max_iter)
        self.coef, self.report = None, None

    def _start(self, D):
        return torch.zeros((D + 1, self.K), dtype=torch.float64)

    def fit(self, X, y):
        X = torch.as_tensor(X)
        X = X.float().contiguous() if X.is_cuda else X.double()
        return _fit(self, X, y, objective_host, lambda X, y, U, ws: ops.ovr_logreg_eval(X, y, U, ws=ws),
                    lambda N, D: max(ops.ovr_logreg_ws_floats(N, D), 2), self._start)

    def fit_bytes(self, Xu8, y):
        """fit on uint8 rows [N, D] with x = byte / 255, any D in 1 .. 65536.  On a HIP device the rows stay bytes and every
        evaluation is one ops.ovr_logreg_eval_u8 call; elsewhere objective_host_bytes.  Same solver, same default gtol_rel per
        path, same report as fit."""
        return _fit(self, _bytes_rows(Xu8).contiguous(), y, objective_host_bytes, lambda X, y, U, ws: ops.ovr_logreg_eval_u8(X, y, U, ws=ws),
                    lambda N, D: max(ops.ovr_logreg_u8_ws_floats(N, D), 2), self._start)

    def predict_proba_bytes(self, Xu8):
        """P [M, K] of uint8 rows, x = byte / 255, any D: ops.ovr_logreg_proba_u8 on a device (float32), the row-blocked float64
        formula on the host."""
        return _proba(self, _bytes_rows(Xu8), proba_host_bytes, lambda X, U: ops.ovr_logreg_proba_u8(X.contiguous(), U))

    def predict_proba(self, Xtest):
        return _proba(self, torch.as_tensor(Xtest), proba_host,
                      lambda X, U: ops.ovr_logreg_proba(X.contiguous() if X.dtype == torch.uint8 else X.float().contiguous(), U))


class OvrMlp:
    """`OvrMlp(n_classes, hidden).fit_bytes(Xu8, y)` then `.predict_proba_bytes(Xu8)`: OneVsRestClassifier(MLPClassifier(alpha=1)) of
    downstream.py:82 on uint8 rows with x = byte / 255 — per class one hidden layer of `hidden` ReLU units (1 .. 128) and the
    objective of objective_mlp_host_bytes, minimised by lbfgs_columns (max_iter 200 is scikit-learn's default).  The objective is
    not convex: the fit is a local minimiser that depends on the initial point, which depends on `seed` alone.

    Initial point, as scikit-learn's Glorot-uniform with the intercepts at zero: ONE draw of (D hidden + hidden) K float64 uniforms
    from torch.Generator().manual_seed(seed) on the host, taken in the row-major order of U's rows — the D hidden rows of W1, then
    the `hidden` rows of w2 (the b1 rows between them and the b2 row stay zero) — and mapped to (2 u - 1) bound with
    bound = sqrt(6 / (D + hidden)) for W1 and sqrt(6 / (hidden + 1)) for w2.  Both paths start from these numbers (the device from
    their float32 rounding).

    Rows on a HIP device select the device path (fp32, one ops.ovr_mlp_eval_u8 call per trial point); anything else the host path
    (float64).  `coef` is U [(D + 2) hidden + 1, K], `report` the solver's report."""

    def __init__(self, n_classes, hidden=100, alpha=1.0, seed=0, gtol_rel=None, max_iter=200):
        self.K = _check_classes(n_classes)
        self.H, self.alpha, self.seed = int(hidden), float(alpha), int(seed)
        if not 1 <= self.H <= MAX_HIDDEN:
            raise ValueError("hidden must lie in 1 .. %d, got %d" % (MAX_HIDDEN, self.H))
        if not 0 <= self.alpha < float("inf"):
            raise ValueError("alpha must be a finite number >= 0, got %r" % (alpha,))
        self.gtol_rel, self.max_iter = gtol_rel, int(max_iter)
        self.coef, self.report = None, None

    def initial_point(self, D):
        """U0 [(D + 2) hidden + 1, K] in float64 on the host (the class docstring has the order of the draw)."""
        H, K = self.H, self.K
        g = torch.Generator().manual_seed(self.seed)
        u = 2.0 * torch.rand(((D + 1) * H, K), dtype=torch.float64, generator=g) - 1.0
        U0 = torch.zeros(((D + 2) * H + 1, K), dtype=torch.float64)
        U0[:D * H] = u[:D * H] * float(np.sqrt(6.0 / (D + H)))
        U0[(D + 1) * H:(D + 2) * H] = u[D * H:] * float(np.sqrt(6.0 / (H + 1)))
        return U0

    def fit_bytes(self, Xu8, y):
        return _fit(self, _bytes_rows(Xu8).contiguous(), y, lambda X, y, U: objective_mlp_host_bytes(X, y, U, self.H, self.alpha),
                    lambda X, y, U, ws: ops.ovr_mlp_eval_u8(X, y, U, self.H, self.alpha, ws=ws),
                    lambda N, D: ops.ovr_mlp_u8_ws_floats(N, D, self.K, self.H), self.initial_point)

    def predict_proba_bytes(self, Xu8):
        """P [M, K]: ops.ovr_mlp_proba_u8 on a device (float32), proba_mlp_host_bytes on the host (float64)."""
        return _proba(self, _bytes_rows(Xu8), lambda X, U: proba_mlp_host_bytes(X, U, self.H),
                      lambda X, U: ops.ovr_mlp_proba_u8(X.contiguous(), U, self.H))


# ---- naive Bayes on cache bytes -----------------------------------------------------------------------------------------

NB_KINDS = ("gnb", "bnb")


def _check_binarize(binarize):
    b = int(binarize)
    if b != binarize or not 0 <= b <= 254:
        raise ValueError("binarize must be a byte threshold in 0 .. 254, got %r" % (binarize,))
    return b


def _check_row_size(X):
    if X.dim() != 2 or not 1 <= X.shape[1] <= 65536:
        raise ValueError("need rows of 1 .. 65536 bytes, got %s" % (tuple(X.shape),))
    return X


def class_moments_host_bytes(Xu8, labels, K, binarize=0, block=2048):
    """{"n": [K], "s1": [K, D], "s2": [K, D], "cnt": [K, D]}, int64 torch on the CPU: per class k the number of rows with that label, and
    per feature sum b, sum b^2 and the number of those rows with b > binarize (a byte threshold in 0 .. 254; 0 is scikit-learn's
    binarize=0.0 on x = b / 255).  A label outside 0 .. K-1 belongs to no class.  In row blocks of `block`; a block's sums are
    products of small integers in float64 (exact below 2^53) and are added in int64 — THE definition of the moments."""
    X = _check_row_size(_bytes_rows(Xu8)).cpu()
    y = torch.as_tensor(labels).long().reshape(-1).cpu()
    K, thr = _check_classes(K), _check_binarize(binarize)
    N, D = X.shape
    if y.numel() != N:
        raise ValueError("need X [N, D] and labels [N], got %s and %s" % (tuple(X.shape), tuple(y.shape)))
    block = max(1, min(int(block), 1 << 20))                         # 2^20 rows of 255^2 stay far below 2^53
    cls = torch.arange(K)[None, :]
    out = {"n": torch.zeros(K, dtype=torch.int64), "s1": torch.zeros((K, D), dtype=torch.int64),
           "s2": torch.zeros((K, D), dtype=torch.int64), "cnt": torch.zeros((K, D), dtype=torch.int64)}
    for r0 in range(0, N, block):
        Xb = X[r0:r0 + block]
        T = (y[r0:r0 + block, None] == cls).double().t()             # [K, n]
        Xd = Xb.double()
        out["n"] += T.sum(1).long()
        out["s1"] += (T @ Xd).long()
        out["s2"] += (T @ (Xd * Xd)).long()
        out["cnt"] += (T @ (Xb > thr).double()).long()
    return out


def _variance_times_n2(n, s1, s2):
    """n s2 - s1^2 as exact integers in a float64 array: int64 where it cannot overflow (n^2 255^2 < 2^62), Python ints elsewhere."""
    n, s1, s2 = np.asarray(n, dtype=np.int64), np.asarray(s1, dtype=np.int64), np.asarray(s2, dtype=np.int64)
    if int(n.max()) ** 2 * 65025 < 2 ** 62:
        return (n * s2 - s1 * s1).astype(np.float64)
    return (n.astype(object) * s2.astype(object) - s1.astype(object) * s1.astype(object)).astype(np.float64)


def gnb_tables(mom, var_smoothing=1e-9):
    """(m [K, D] float32, w [K, D] float32, c [K] float64, eps) of GaussianNB on x = b / 255, in byte units, from the moments:
    m = s1 / n_k,  v = (n_k s2 - s1^2) / n_k^2 (the numerator in exact integers),  eps = var_smoothing max_j V_j with V the same
    expression on the moments summed over the classes,  w = 1 / (2 (v + eps)),  c_k = log(n_k / N) - 1/2 sum_j log(2 pi (v + eps) / 255^2);
    jll[i, k] = c_k - sum_j w (b_ij - m)^2.  Derived in float64; m and w are rounded to float32 ONCE, here, for both paths."""
    n = mom["n"].numpy().astype(np.int64)
    s1, s2 = mom["s1"].numpy(), mom["s2"].numpy()
    if not float(var_smoothing) >= 0 or (n < 1).any():
        raise ValueError("need var_smoothing >= 0 and a row in every class, got %r and counts %s" % (var_smoothing, n.tolist()))
    N = int(n.sum())
    nf = n.astype(np.float64)[:, None]
    m = s1.astype(np.float64) / nf
    v = _variance_times_n2(n[:, None], s1, s2) / (nf * nf)
    V = _variance_times_n2(np.int64(N), s1.sum(0), s2.sum(0)) / (float(N) * float(N))
    eps = float(var_smoothing) * float(V.max())
    if not eps > 0:
        raise ValueError("var_smoothing times the largest feature variance is %r: every feature is constant (or var_smoothing is 0), "
                         "the Gaussian model has no variance to work with" % eps)
    w = 1.0 / (2.0 * (v + eps))
    c = np.log(nf[:, 0] / N) - 0.5 * np.log(2.0 * np.pi * (v + eps) / 65025.0).sum(1)
    m32, w32 = m.astype(np.float32), w.astype(np.float32)
    if not np.isfinite(w32).all():
        raise ValueError("var_smoothing = %r leaves 1 / (2 (variance + eps)) beyond float32: eps = %.3g" % (var_smoothing, eps))
    return m32, w32, c, eps


def bnb_tables(mom, alpha=0.01):
    """(delta [K, D] float32, c [K] float64) of BernoulliNB(alpha) on the features [b > binarize], from the moments:
    lp = log(cnt + alpha) - log(n_k + 2 alpha),  ln = log1p(-exp(lp)),  delta = lp - ln,  c_k = log(n_k / N) + sum_j ln;
    jll[i, k] = c_k + sum_j [b_ij > binarize] delta.  Derived in float64; delta is rounded to float32 ONCE, here, for both paths."""
    alpha = float(alpha)
    n = mom["n"].numpy().astype(np.float64)
    if not 0 < alpha < float("inf") or (n < 1).any():
        raise ValueError("need a finite alpha > 0 and a row in every class, got %r and counts %s" % (alpha, n.tolist()))
    lp = np.log(mom["cnt"].numpy().astype(np.float64) + alpha) - np.log(n + 2.0 * alpha)[:, None]
    ln = np.log1p(-np.exp(lp))
    c = np.log(n / n.sum()) + ln.sum(1)
    return (lp - ln).astype(np.float32), c


def jll_host_bytes(Xu8, kind, tables, c, binarize=0, block=2048):
    """jll [M, K] in float64 of uint8 rows under the float32 tables of gnb_tables / bnb_tables and the float64 constants c, in row
    blocks — the model of the device scores: gnb c_k - sum_j w (b - m)^2, bnb c_k + sum_j [b > binarize] delta, the sums in float64."""
    X = _bytes_rows(Xu8).cpu()
    tabs = [torch.from_numpy(np.asarray(t, dtype=np.float32)).double() for t in tables]
    c = torch.from_numpy(np.asarray(c, dtype=np.float64))
    K = tabs[0].shape[0]
    out = torch.empty((X.shape[0], K), dtype=torch.float64)
    block = max(1, int(block))
    for r0 in range(0, X.shape[0], block):
        Xb = X[r0:r0 + block]
        if kind == "gnb":
            Xd = Xb.double()
            for k in range(K):
                out[r0:r0 + block, k] = c[k] - (tabs[1][k] * (Xd - tabs[0][k]) ** 2).sum(1)
        else:
            out[r0:r0 + block] = c + (Xb > int(binarize)).double() @ tabs[0].t()
    return out


def log_odds(jll):
    """L[i, k] = jll[i, k] - logsumexp_{l != k} jll[i, l]: the log-odds of class k, a strictly increasing function of the posterior
    that keeps its order where the posterior has saturated to exactly 0 or 1."""
    J = torch.as_tensor(jll).double()
    K = J.shape[1]
    L = torch.empty_like(J)
    for k in range(K):
        L[:, k] = J[:, k] - torch.logsumexp(J[:, [l for l in range(K) if l != k]], 1)
    return L


class NaiveBayes:
    """`NaiveBayes(n_classes, kind).fit_bytes(Xu8, y)` then `.jll_bytes(Xu8)`, `.predict_proba_bytes(Xu8)`, `.log_odds_bytes(Xu8)`:
    kind "gnb" is GaussianNB(var_smoothing) and "bnb" BernoulliNB(alpha, binarize) of downstream.py:76-78 on uint8 rows with
    x = byte / 255 (binarize is a byte threshold, 0 .. 254: the feature is [byte > binarize]).  The fit is a closed form of integer
    moments: rows on a HIP device select ops.class_moments_u8, anything else class_moments_host_bytes — the same integers — and the
    tables come from them by the same host code, so `coef` is the same bits on both paths.  Scores: rows on a HIP device select
    ops.nb_score_gauss_u8 / nb_score_bern_u8 (fp32 sums), anything else jll_host_bytes (float64 sums); the constants c_k are added
    in float64 on the host and every result is a float64 CPU tensor [M, K].
    `coef` (float64): gnb [2 D + 1, K] — D rows of m, D rows of w (both the float32 values used), then c; bnb [D + 1, K] — delta, c.
    fit_bytes returns the report {"kind", "n_per_class", "eps" (gnb) | "binarize" (bnb)}."""

    def __init__(self, n_classes, kind, var_smoothing=1e-9, alpha=0.01, binarize=0):
        self.K = _check_classes(n_classes)
        if kind not in NB_KINDS:
            raise ValueError("kind must be one of %s, got %r" % (NB_KINDS, kind))
        self.kind, self.var_smoothing, self.alpha = kind, float(var_smoothing), float(alpha)
        if not 0 <= self.var_smoothing < float("inf"):
            raise ValueError("var_smoothing must be a finite number >= 0, got %r" % (var_smoothing,))
        if not 0 < self.alpha < float("inf"):
            raise ValueError("alpha must be a finite number > 0, got %r" % (alpha,))
        self.binarize = _check_binarize(binarize)
        self.coef, self.report, self.tables, self.c = None, None, None, None

    def fit_bytes(self, Xu8, y):
        X, y = _check_row_size(_bytes_rows(Xu8)).contiguous(), torch.as_tensor(y)
        _check_rows(self.K, X, y)
        if X.is_cuda:
            with torch.cuda.device(X.device):
                yd = y.to(X.device).reshape(-1).to(torch.int32).contiguous()
                mom = {k: v.cpu() for k, v in ops.class_moments_u8(X, yd, self.K, self.binarize).items()}
        else:
            mom = class_moments_host_bytes(X, y, self.K, self.binarize)
        rep = {"kind": self.kind, "n_per_class": [int(v) for v in mom["n"].tolist()]}
        if self.kind == "gnb":
            m, w, c, eps = gnb_tables(mom, self.var_smoothing)
            self.tables, rep["eps"] = (m, w), eps
        else:
            delta, c = bnb_tables(mom, self.alpha)
            self.tables, rep["binarize"] = (delta,), self.binarize
        self.c = c
        self.coef = torch.from_numpy(np.concatenate([t.astype(np.float64).T for t in self.tables] + [c[None, :]], 0))
        self.report = rep
        return rep

    def jll_bytes(self, Xu8):
        """jll [M, K], float64 on the CPU."""
        if self.coef is None:
            raise RuntimeError("fit first")
        X = _bytes_rows(Xu8)
        if X.dim() != 2 or X.shape[1] != self.tables[0].shape[1]:
            raise ValueError("need uint8 rows [M, %d], got %s" % (self.tables[0].shape[1], tuple(X.shape)))
        if not X.is_cuda:
            return jll_host_bytes(X, self.kind, self.tables, self.c, self.binarize)
        with torch.cuda.device(X.device):
            tabs = [torch.from_numpy(t).to(X.device) for t in self.tables]
            if self.kind == "gnb":
                S = -ops.nb_score_gauss_u8(X.contiguous(), tabs[0], tabs[1]).cpu().double()
            else:
                S = ops.nb_score_bern_u8(X.contiguous(), tabs[0], self.binarize).cpu().double()
        return torch.from_numpy(self.c) + S

    def predict_proba_bytes(self, Xu8):
        """P [M, K] = softmax_k(jll), float64 on the CPU."""
        return torch.softmax(self.jll_bytes(Xu8), 1)

    def log_odds_bytes(self, Xu8):
        """L [M, K] = log_odds(jll): what AUROC ranks."""
        return log_odds(self.jll_bytes(Xu8))


def _auc(pos, neg):
    if torch.is_tensor(pos) and pos.is_cuda:
        with torch.cuda.device(pos.device):
            gt, eq = (t.cpu().numpy().astype(np.int64) for t in ops.rank_counts(pos.contiguous(), neg.contiguous()))
    else:
        gt, eq = audit.rank_counts_host(pos, neg)
    return audit.rank_metrics(gt, eq, int(neg.numel() if torch.is_tensor(neg) else len(neg)))["auc"]


def auroc(P, y):
    """{"micro": ..., "per_class": [...]} of scores P [M, K] (rounded to float32 first: the rank counts compare fp32 values) against
    labels y [M] — roc_auc["micro"] and roc_auc[k] of downstream.py:48-62.  Micro: the M entries P[i, y_i] against the M (K - 1)
    others; class k: P[y == k, k] against P[y != k, k]; ties count half.  P on a HIP device: the counts come from cslgan_rank_counts;
    elsewhere from the host model; the integers, hence the figures, are the same.  A class without a test sample gives nan."""
    on_dev = torch.is_tensor(P) and P.is_cuda
    P = (P if torch.is_tensor(P) else torch.from_numpy(np.asarray(P))).to(torch.float32)
    M, K = P.shape
    y = torch.as_tensor(y).reshape(-1).long().to(P.device)
    hot = y[:, None] == torch.arange(K, device=P.device)[None, :]
    conv = (lambda t: t.contiguous()) if on_dev else (lambda t: t.contiguous().numpy())
    out = {"micro": _auc(conv(P[hot]), conv(P[~hot])), "per_class": []}
    for k in range(K):
        pos, neg = P[hot[:, k], k], P[~hot[:, k], k]
        out["per_class"].append(_auc(conv(pos), conv(neg)) if pos.numel() and neg.numel() else float("nan"))
    return out


# ---- decision trees and forests on cache bytes --------------------------------------------------------------------------

TREE_KINDS = ("dt", "rf")
TREE_SEED_TAG = 0x7472656573706C74   # include/cslgan.h "decision trees": xor-ed into the seed of the feature-mask stream
TREE_COUNTER_TAG = 0x74726565        # word 3 of every counter of that stream
TREE_MAX_ROWS = 1 << 24
TREE_LAUNCH_TILES = 1 << 20          # (segment, 16-feature tile) pairs of one split-search call: 40 MiB of workspace at most
_TREE_HOST_BLOCK = 1 << 22           # entries of a host model's sort block (rows x features)
_HOST_SORT_ROWS = 64                 # a host search sorts a feature's bytes up to this many rows and builds its histograms beyond


def tree_mask_threshold(max_features, D):
    """The 32-bit threshold of the keyed feature mask: floor(max_features / D 2^32); 0 — every feature — when max_features >= D."""
    mf, D = int(max_features), int(D)
    if mf < 1:
        raise ValueError("max_features must be >= 1, got %r" % (max_features,))
    return 0 if mf >= D else (mf << 32) // D


def tree_feature_mask(seed, tree, node, D, mask_thr):
    """bool [D]: feature j is a candidate at node `node` of tree `tree` iff mask_thr == 0 or word 0 of Philox4x32-10 at counter
    (j, node, tree, TREE_COUNTER_TAG) under the key seed ^ TREE_SEED_TAG is below mask_thr — the host form of the device's mask."""
    if int(mask_thr) == 0:
        return np.ones(int(D), dtype=bool)
    key = (int(seed) ^ TREE_SEED_TAG) & 0xFFFFFFFFFFFFFFFF
    w = audit.philox4x32_10(np.arange(int(D), dtype=np.uint64), int(node) & 0xFFFFFFFF, int(tree) & 0xFFFFFFFF, TREE_COUNTER_TAG,
                            key & 0xFFFFFFFF, key >> 32)[0]
    return w < np.uint64(int(mask_thr))


def _best_byte_split(Xs, w, wt, cols):
    """(j, v, v_hi, nL, pL, score) of one node on the host — the one search behind best_split_host_bytes and boost_stump_host_bytes:
    Xs [n, D] uint8 rows of weight w >= 1 (int64), wt = w t, over the candidate features `cols` (ascending); (-1, -1, -1, 0, 0, -1.0)
    without a candidate.  Two ways to the same integers: up to _HOST_SORT_ROWS rows are sorted per feature (the candidates lie where
    the sorted byte changes, the cumulative sums there are (nL, pL)), more rows go into 256-bin histograms — np.bincount with float64
    weights, every partial sum an integer below 2^53, so the sums are exact.  The score is (a a) / fl(nL) + (c c) / fl(nR) with
    a = fl(pL), c = fl(p - pL): five float64 operations rounded once each.  In blocks of features; the first maximum of a block is
    the smallest j, then the smallest v, and a later block wins only with a strictly larger score."""
    n_rows = Xs.shape[0]
    best = (-1, -1, -1, 0, 0, -1.0)
    if n_rows < 2 or len(cols) == 0:
        return best
    n, p = int(w.sum()), int(wt.sum())
    few = n_rows <= _HOST_SORT_ROWS
    step = max(1, _TREE_HOST_BLOCK // (n_rows if few else 256))
    for c0 in range(0, len(cols), step):
        cc = cols[c0:c0 + step]
        if few:
            A = np.ascontiguousarray(Xs[:, cc].T)                    # [c, n]: a feature's bytes lie together
            order = np.argsort(A, axis=1, kind="stable")
            vs = np.take_along_axis(A, order, 1)
            valid = vs[:, :-1] != vs[:, 1:]                          # [c, n - 1]: a candidate between sorted places i and i + 1
            nL, pL = np.cumsum(w[order], 1)[:, :-1], np.cumsum(wt[order], 1)[:, :-1]
        else:
            c = len(cc)
            idx = (Xs[:, cc].astype(np.int64) + 256 * np.arange(c)[None, :]).reshape(-1)
            hn = np.bincount(idx, weights=np.repeat(w.astype(np.float64), c), minlength=256 * c).reshape(c, 256).astype(np.int64)
            hp = np.bincount(idx, weights=np.repeat(wt.astype(np.float64), c), minlength=256 * c).reshape(c, 256).astype(np.int64)
            nL, pL = np.cumsum(hn, 1), np.cumsum(hp, 1)
            valid = (hn > 0) & (nL < n)
        if not valid.any():
            continue
        a, b = pL.astype(np.float64), (p - pL).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (a * a) / nL.astype(np.float64) + (b * b) / (n - nL).astype(np.float64)
        s = np.where(valid, s, -1.0)
        ci, i = divmod(int(np.argmax(s)), s.shape[1])
        if s[ci, i] > best[5]:
            v, vh = (int(vs[ci, i]), int(vs[ci, i + 1])) if few else (i, i + 1 + int(np.nonzero(hn[ci, i + 1:])[0][0]))
            best = (int(cc[ci]), v, vh, int(nL[ci, i]), int(pL[ci, i]), float(s[ci, i]))
    return best


def best_split_host_bytes(Xu8, labels, rows, seg_off, seg_class, seg_wrow=None, weights=None, seg_key=None, mask_thr=0, seed=0):
    """(out int32 [S, 7] = (j, v, v_hi, nL, pL, n, p), score int64 [S]: the bits of the float64 score), CPU tensors — THE definition of the
    split search (include/cslgan.h "decision trees" has the arguments).  Segment s is the rows rows[seg_off[s] ..
    seg_off[s + 1]) of X with the targets t = [label == seg_class[s]] and the weights weights[seg_wrow[s]] (1 without; a row of
    weight 0 is not there).  A candidate (j, v): byte v <= 254 present, nL = sum w [b <= v] >= 1, nR >= 1, feature j let through by
    tree_feature_mask(seed, *seg_key[s], D, mask_thr); score fl(pL pL / nL) + fl(pR pR / nR) in float64, the products exact integers
    converted once — computed as boost_stump_host_bytes' (a a) / fl(nL) + (c c) / fl(nR), the same bits: the counts are below 2^31, so
    the factors convert exactly and the product of the two is the exact integer rounded once.  The largest score wins, ties to the smallest j, then the smallest v; v_hi is the next larger byte present.
    No valid candidate: (-1, -1, -1, 0, 0, n, p) and score 0."""
    X = _check_row_size(_bytes_rows(Xu8)).cpu().numpy()
    N, D = X.shape
    if not 1 <= N < TREE_MAX_ROWS:
        raise ValueError("need 1 <= N < 2^24 rows, got %d" % N)
    tonp = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.int64)
    y, rows, seg_off, seg_class = tonp(labels).reshape(-1), tonp(rows).reshape(-1), tonp(seg_off).reshape(-1), tonp(seg_class).reshape(-1)
    S = len(seg_class)
    if len(y) != N or len(seg_off) != S + 1:
        raise ValueError("need labels [N] and seg_off [S + 1], got %d labels for %d rows and %d offsets for %d segments" % (len(y), N, len(seg_off), S))
    if (weights is None) != (seg_wrow is None):
        raise ValueError("weights and seg_wrow go together")
    if int(mask_thr) and seg_key is None:
        raise ValueError("a feature mask needs seg_key = (seg_tree, seg_node)")
    W = None if weights is None else tonp(weights)
    wrow = None if seg_wrow is None else tonp(seg_wrow).reshape(-1)
    key = None if seg_key is None else (tonp(seg_key[0]).reshape(-1), tonp(seg_key[1]).reshape(-1))
    out = np.zeros((S, 7), dtype=np.int32)
    score = np.zeros(S, dtype=np.float64)
    every = np.arange(D)
    for s in range(S):
        r = rows[seg_off[s]:seg_off[s + 1]]
        w = np.ones(len(r), dtype=np.int64) if W is None or wrow[s] < 0 else W[wrow[s]][r]
        r, w = r[w > 0], w[w > 0]
        wt = w * (y[r] == seg_class[s])
        n, p = int(w.sum()), int(wt.sum())
        if n >= 1 << 31:
            raise ValueError("the weights of segment %d add up to %d; the counters take less than 2^31" % (s, n))
        cols = every if int(mask_thr) == 0 else np.nonzero(tree_feature_mask(seed, key[0][s], key[1][s], D, mask_thr))[0]
        j, v, vh, nL, pL, sc = _best_byte_split(X[r], w, wt, cols)
        out[s] = (j, v, vh, nL, pL, n, p)
        score[s] = sc if j >= 0 else 0.0
    return torch.from_numpy(out), torch.from_numpy(score.view(np.int64).copy())


def tree_tables(coef):
    """(feature, threshold, child int32 [Q], tree_off int32 [T + 1]) numpy views of node tables coef [Q, 6] = (tree, feature, threshold,
    first child, n, p) sorted by (tree, node): what the apply entries take."""
    c = (coef.detach().cpu().numpy() if torch.is_tensor(coef) else np.asarray(coef)).astype(np.int32)
    T = int(c[:, 0].max()) + 1
    off = np.concatenate([[0], np.cumsum(np.bincount(c[:, 0], minlength=T))]).astype(np.int32)
    return np.ascontiguousarray(c[:, 1]), np.ascontiguousarray(c[:, 2]), np.ascontiguousarray(c[:, 3]), off


def tree_apply_host_bytes(Xu8, feature, threshold, child, tree_off):
    """leaf int32 [T, M], a CPU tensor: the tree-local number of the leaf each row of Xu8 reaches — from the root, left (child) when
    byte <= threshold, right (child + 1) otherwise, until feature == -1.  A walk that leaves its tree's table, or a child that does not
    lie behind its parent, gives -1 (the device's rule for a malformed table)."""
    X = _bytes_rows(Xu8).cpu().numpy()
    f, t, c, off = (np.asarray(a).astype(np.int64).reshape(-1) for a in (feature, threshold, child, tree_off))
    M, D, T = X.shape[0], X.shape[1], len(off) - 1
    leaf = np.full((T, M), -1, dtype=np.int32)
    ar = np.arange(M)
    for k in range(T):
        q0, nq = int(off[k]), int(off[k + 1] - off[k])
        if nq < 1 or q0 < 0 or q0 + nq > len(f):
            continue
        node, live = np.zeros(M, dtype=np.int64), np.ones(M, dtype=bool)
        for _ in range(nq):
            if not live.any():
                break
            fi = f[q0 + node]
            done = live & (fi < 0)
            leaf[k, done] = node[done]
            live &= fi >= 0
            ci = c[q0 + node]
            live &= (fi < D) & (ci > node) & (ci + 1 < nq)
            b = X[ar, np.where(live, fi, 0)]
            node = np.where(live, ci + (b > t[q0 + node]), node)
    return torch.from_numpy(leaf)


class Trees:
    """`Trees(n_classes, kind).fit_bytes(Xu8, y)` then `.apply_bytes(Xu8)`, `.predict_proba_bytes(Xu8)`: kind "dt" is
    OneVsRestClassifier(DecisionTreeClassifier()) and "rf" OneVsRestClassifier(RandomForestClassifier(n_trees)) of downstream.py:69-74,
    grown on the uint8 rows themselves by the definition of DESIGN.md §6m — exact histogram splits, Gini, ties to the smallest
    (feature, byte), nodes numbered level by level.  Class k has n_trees trees (one for dt), tree number k n_trees + b.

    rf: tree b weighs the rows by the multiplicities of N draws with replacement from numpy's default_rng([seed, b]) (drawn on the
    host, shared by the K classes), and at node q feature j is a candidate iff tree_feature_mask(seed, b, q, D, thr)[j] with
    thr = tree_mask_threshold(max_features, D); max_features defaults to max(1, floor(sqrt(D))).  Two deviations from Breiman /
    scikit-learn: the subset is drawn per feature, so its size is binomial(D, max_features / D), not fixed; and a node whose subset
    holds no valid split becomes a leaf, where scikit-learn keeps drawing features until it has found one.

    Rows on a HIP device select ops.tree_best_split_u8 / ops.tree_apply_u8, anything else best_split_host_bytes /
    tree_apply_host_bytes — the same integers and score bits, so `coef` is the same on both paths.  The level loop around the split
    search is one piece of torch code that runs where the rows are.
    `coef`: the node tables, int32 [Q, 6] on the CPU = (tree, feature or -1, threshold, first child or -1, n, p) sorted by (tree, node).
    fit_bytes returns the report {"kind", "n_per_class", "nodes", "leaves", "depth" (per tree), "levels" (split-search levels)}."""

    def __init__(self, n_classes, kind="dt", n_trees=100, max_features=None, max_depth=0, min_samples_split=2, seed=0):
        self.K = _check_classes(n_classes)
        if kind not in TREE_KINDS:
            raise ValueError("kind must be one of %s, got %r" % (TREE_KINDS, kind))
        self.kind = kind
        self.B = 1 if kind == "dt" else int(n_trees)
        if not 1 <= self.B <= 4095:
            raise ValueError("n_trees must lie in 1 .. 4095, got %r" % (n_trees,))
        if max_features is not None and int(max_features) < 1:
            raise ValueError("max_features must be >= 1, got %r" % (max_features,))
        self.max_features = None if max_features is None else int(max_features)
        self.max_depth, self.min_samples_split, self.seed = int(max_depth), int(min_samples_split), int(seed)
        if self.max_depth < 0:
            raise ValueError("max_depth must be >= 0 (0: unlimited), got %r" % (max_depth,))
        if self.min_samples_split < 2:
            raise ValueError("min_samples_split must be >= 2, got %r" % (min_samples_split,))
        if not 0 <= self.seed < 2 ** 63:
            raise ValueError("seed must lie in 0 .. 2^63 - 1, got %r" % (seed,))
        self.coef, self.report = None, None

    def bootstrap_weights(self, N):
        """int32 [n_trees, N]: row b holds the multiplicities of N draws with replacement from default_rng([seed, b])."""
        return np.stack([np.bincount(np.random.default_rng([self.seed, b]).integers(0, N, N), minlength=N) for b in range(self.B)]).astype(np.int32)

    def mask_threshold(self, D):
        if self.kind == "dt":
            return 0
        return tree_mask_threshold(max(1, int(np.sqrt(D))) if self.max_features is None else self.max_features, D)

    def _search(self, X, lab, rows, seg_off, seg_tree, seg_node, W, thr):
        """The split search of one level, in calls of at most TREE_LAUNCH_TILES (segment, tile) pairs: int64 numpy [S, 7]."""
        S, D, B = len(seg_tree), X.shape[1], self.B
        per = max(1, TREE_LAUNCH_TILES // ((D + 15) // 16))
        outs = []
        for s0 in range(0, S, per):
            s1 = min(S, s0 + per)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(X.device)
            args = (dev(seg_off[s0:s1 + 1]), dev(seg_tree[s0:s1] // B))
            kw = dict(seg_wrow=None if W is None else dev(seg_tree[s0:s1] % B), weights=W,
                      seg_key=(dev(seg_tree[s0:s1] % B), dev(seg_node[s0:s1])), mask_thr=thr, seed=self.seed)
            if X.is_cuda:
                out, _ = ops.tree_best_split_u8(X, lab, self.K, rows, *args, **kw)
            else:
                out, _ = best_split_host_bytes(X, lab, rows, *args, **kw)
            outs.append(out.cpu().numpy().astype(np.int64))
        return np.concatenate(outs, 0)

    def fit_bytes(self, Xu8, y, weights=None, mask_thr=None):
        """Grow the K n_trees trees.  weights (int [n_trees, N], >= 0) replaces the bootstrap multiplicities (dt: the unit weights) and
        mask_thr the feature-mask threshold — what the tests use to tie rf to dt."""
        X, y = _check_row_size(_bytes_rows(Xu8)).contiguous(), torch.as_tensor(y)
        _check_rows(self.K, X, y)
        N, D = X.shape
        if not N < TREE_MAX_ROWS:
            raise ValueError("need fewer than 2^24 rows, got %d" % N)
        K, B, dev = self.K, self.B, X.device
        T = K * B
        thr = self.mask_threshold(D) if mask_thr is None else int(mask_thr)
        Wn = weights if weights is not None else (self.bootstrap_weights(N) if self.kind == "rf" else None)
        if Wn is not None:
            Wn = np.ascontiguousarray(np.asarray(Wn), dtype=np.int64).reshape(B, N)
            if (Wn < 0).any() or int(Wn.sum(1).max()) >= 1 << 31 or int(Wn.sum(1).min()) < 1:
                raise ValueError("weights must be >= 0 and add up to 1 .. 2^31 - 1 per tree")
        with torch.cuda.device(dev) if X.is_cuda else contextlib.nullcontext():
            lab = y.to(dev).reshape(-1).to(torch.int32).contiguous()
            W = None if Wn is None else torch.from_numpy(Wn.astype(np.int32)).to(dev)
            # the roots: per tree the rows of weight >= 1, in row order; trees in the order k B + b
            per_b = [np.arange(N) if Wn is None else np.nonzero(Wn[b])[0] for b in range(B)]
            rows = torch.from_numpy(np.concatenate(per_b * K).astype(np.int32)).to(dev)
            sizes = np.array([len(r) for r in per_b] * K, dtype=np.int64)
            seg_tree, seg_node = np.arange(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
            next_node = np.ones(T, dtype=np.int64)
            depth = np.zeros(T, dtype=np.int64)
            records, level = [], 0
            while len(seg_tree):
                S = len(seg_tree)
                seg_off = np.concatenate([[0], np.cumsum(sizes)])
                o = self._search(X, lab, rows, seg_off, seg_tree, seg_node, W, thr)
                j, v, vh, n, p = o[:, 0], o[:, 1], o[:, 2], o[:, 5], o[:, 6]
                split = ~((p == 0) | (p == n) | (n < self.min_samples_split) | (j < 0))
                if self.max_depth and level >= self.max_depth:
                    split[:] = False
                # children: per tree the next free numbers, in the order of the parents, left before right
                rank = np.cumsum(split) - split                                          # among all splitting segments
                first = np.searchsorted(seg_tree, seg_tree, side="left")                 # the tree's first segment of this level
                child = np.where(split, next_node[seg_tree] + 2 * (rank - rank[first]), -1)
                next_node += 2 * np.bincount(seg_tree[split], minlength=T)
                depth[seg_tree] = level
                records.append(np.stack([seg_tree, seg_node, np.where(split, j, -1), np.where(split, (v + vh) // 2, 0), child, n, p], 1))
                level += 1
                if not split.any():
                    break
                # the next level's segments: gather the chosen byte per row, stable sort by (segment, side)
                seg_of_row = torch.repeat_interleave(torch.arange(S, device=dev), torch.from_numpy(sizes).to(dev))
                keep = torch.from_numpy(split).to(dev)[seg_of_row]
                r, sg = rows[keep], seg_of_row[keep]
                byte = X[r.long(), torch.from_numpy(np.where(split, j, 0)).to(dev)[sg]]
                side = (byte.to(torch.int64) > torch.from_numpy(v).to(dev)[sg]).to(torch.int64)
                key = 2 * torch.from_numpy(rank).to(dev)[sg] + side
                rows = r[torch.sort(key, stable=True).indices].contiguous()
                n_split = int(split.sum())
                sizes = torch.bincount(key, minlength=2 * n_split).cpu().numpy().astype(np.int64)
                seg_tree = np.repeat(seg_tree[split], 2)
                seg_node = np.stack([child[split], child[split] + 1], 1).reshape(-1)
        rec = np.concatenate(records, 0)
        rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
        self.coef = torch.from_numpy(np.ascontiguousarray(rec[:, [0, 2, 3, 4, 5, 6]]).astype(np.int32))
        counts = np.bincount(y.detach().cpu().numpy().astype(np.int64).reshape(-1), minlength=K)
        self.report = {"kind": self.kind, "n_per_class": [int(c) for c in counts[:K]], "nodes": [int(c) for c in next_node],
                       "leaves": [int(c) for c in np.bincount(rec[rec[:, 2] < 0, 0], minlength=T)], "depth": [int(c) for c in depth], "levels": level}
        return self.report

    def apply_bytes(self, Xu8):
        """leaf int32 [K n_trees, M] on the CPU: ops.tree_apply_u8 for rows on a HIP device, tree_apply_host_bytes elsewhere."""
        if self.coef is None:
            raise RuntimeError("fit first")
        X = _check_row_size(_bytes_rows(Xu8))
        tabs = tree_tables(self.coef)
        if not X.is_cuda:
            return tree_apply_host_bytes(X, *tabs)
        with torch.cuda.device(X.device):
            return ops.tree_apply_u8(X.contiguous(), *(torch.from_numpy(t).to(X.device) for t in tabs)).cpu()

    def predict_proba_bytes(self, Xu8):
        """P [M, K] float64 on the CPU: the mean over the class's trees, added in tree order, of the reached leaf's p / n — computed
        here, on the host, from the integer leaf tables for both paths."""
        leaf = self.apply_bytes(Xu8).numpy().astype(np.int64)
        c = self.coef.numpy().astype(np.int64)
        off = tree_tables(self.coef)[3].astype(np.int64)
        value = c[:, 5].astype(np.float64) / c[:, 4].astype(np.float64)
        P = np.zeros((leaf.shape[1], self.K), dtype=np.float64)
        for k in range(self.K):
            for b in range(self.B):
                t = k * self.B + b
                P[:, k] += value[off[t] + leaf[t]]
            P[:, k] /= float(self.B)
        return torch.from_numpy(P)



# ---- boosted stumps on cache bytes ----------------------------------------------------------------------------------------

BOOST_W1 = 1 << 28                   # the largest fixed-point row weight (include/cslgan.h "boosted stumps")
BOOST_MAX_ROUNDS = 4095              # K n_rounds stumps go through the tree apply path as trees: at most 65535
_BOOST_APPLY_ENTRIES = 1 << 24       # (stump, test row) pairs of one apply call


def boost_stump_host_bytes(Xu8, labels, weights, K):
    """(out int64 [K, 7] = (j, v, v_hi, nL, pL, n, p), score int64 [K]: the bits of the float64 score), CPU tensors — THE definition of
    the stump search of a boosting round (include/cslgan.h "boosted stumps").  Class k has the targets t = [label == k]
    and the weights weights[k] (int [K, N], 0 .. BOOST_W1; a row of weight 0 is not there).  A candidate (j, v): byte v <= 254 present
    among the rows of weight > 0, nL = sum w [b <= v] >= 1, nR = n - nL >= 1; score (a a) / fl(nL) + (c c) / fl(nR) with a = fl(pL),
    c = fl(p - pL), five float64 operations rounded once each (every integer is below 2^52: the conversions are exact).  The largest
    score wins, ties to the smallest j, then the smallest v; v_hi is the next larger byte present.  No valid candidate:
    (-1, -1, -1, 0, 0, n, p) and score 0.
    The search is best_split_host_bytes' (_best_byte_split); for counts below 2^32 its form of the score, the exact integer pL pL
    converted once, rounds the same real number once and gives the same bits."""
    X = _check_row_size(_bytes_rows(Xu8)).cpu().numpy()
    N, D = X.shape
    K = _check_classes(K)
    if not 1 <= N < TREE_MAX_ROWS:
        raise ValueError("need 1 <= N < 2^24 rows, got %d" % N)
    tonp = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.int64)
    y, W = tonp(labels).reshape(-1), tonp(weights)
    if len(y) != N or W.shape != (K, N):
        raise ValueError("need labels [N] and weights [K, N], got %d labels and weights %s for %d rows, %d classes" % (len(y), W.shape, N, K))
    if (W < 0).any() or (W > BOOST_W1).any():
        raise ValueError("weights must lie in 0 .. 2^28")
    out = np.zeros((K, 7), dtype=np.int64)
    score = np.zeros(K, dtype=np.float64)
    every = np.arange(D)
    for k in range(K):
        live = W[k] > 0
        w = W[k][live]
        wt = w * (y[live] == k)
        j, v, vh, nL, pL, sc = _best_byte_split(X[live], w, wt, every)
        out[k] = (j, v, vh, nL, pL, int(w.sum()), int(wt.sum()))
        score[k] = sc if j >= 0 else 0.0
    return torch.from_numpy(out), torch.from_numpy(score.view(np.int64).copy())


class AdaBoost:
    """`AdaBoost(n_classes, n_rounds, learning_rate).fit_bytes(Xu8, y)` then `.decision_bytes(Xu8)`, `.predict_proba_bytes(Xu8)`:
    OneVsRestClassifier(AdaBoostClassifier()) of downstream.py:79-80 on the uint8 rows themselves by the definition of DESIGN.md §6n —
    per class up to n_rounds stumps (depth-1 trees with exact byte thresholds), SAMME for two classes, under fixed-point row weights
    0 .. 2^28 whose largest is 2^28 after every round.  A round: the stump (boost_stump_host_bytes), its weighted error e (an exact
    int64); e == 0 keeps it with alpha 1 and stops the class, 2 e >= n discards it and stops; else alpha = learning_rate log((n - e) / e),
    the missed rows are multiplied by exp(alpha) and all by 2^28 / the largest, rounded down.

    Rows on a HIP device select ops.boost_stump_u8 / ops.tree_apply_u8, anything else boost_stump_host_bytes / tree_apply_host_bytes —
    the same integers, so `coef` and P are the same bits on both paths.  Everything around the stump search — the predictions on the
    training rows, e, the largest weight, the reweighting — is one piece of torch int64 / float64 code that runs where the rows are;
    alpha and exp(alpha) are computed on the host for both paths.
    `coef`: float64 [Q, 7] on the CPU = (class, round, feature or -1, threshold, left prediction, right prediction, alpha) sorted by
    (class, round); a stump without a split has feature -1 and two equal predictions.  fit_bytes returns the report {"kind": "ab",
    "n_per_class", "rounds", "alpha_sum", "first_err"}, the last three per class (first_err: e / n of the first round)."""

    def __init__(self, n_classes, n_rounds=50, learning_rate=1.0):
        self.K = _check_classes(n_classes)
        self.n_rounds, self.learning_rate = int(n_rounds), float(learning_rate)
        if not 1 <= self.n_rounds <= BOOST_MAX_ROUNDS or self.n_rounds != n_rounds:
            raise ValueError("n_rounds must lie in 1 .. %d, got %r" % (BOOST_MAX_ROUNDS, n_rounds))
        if not 0 < self.learning_rate < float("inf"):
            raise ValueError("learning_rate must be a finite number > 0, got %r" % (learning_rate,))
        self.coef, self.report = None, None

    def fit_bytes(self, Xu8, y, on_round=None):
        """on_round(round, weights int32 [K, N]) is called after every round with the weights of the next one (a stopped class: zeros)."""
        X, y = _check_row_size(_bytes_rows(Xu8)).contiguous(), torch.as_tensor(y).reshape(-1)
        N, D = X.shape
        K, dev = self.K, X.device
        if y.numel() != N or not 1 <= N < TREE_MAX_ROWS:
            raise ValueError("need X [N, D] and y [N] with 1 <= N < 2^24, got %s and %s" % (tuple(X.shape), tuple(y.shape)))
        counts = np.bincount(np.clip(y.cpu().numpy().astype(np.int64), -1, K) + 1, minlength=K + 2)[1:K + 1]      # labels outside: no class
        if (counts == 0).any():
            raise ValueError("every class 0 .. %d needs a training sample; counts: %s" % (K - 1, counts.tolist()))
        records = [[] for _ in range(K)]
        first_err = [0.0] * K
        with torch.cuda.device(dev) if X.is_cuda else contextlib.nullcontext():
            lab = y.to(dev).to(torch.int32).contiguous()
            T = lab[None, :] == torch.arange(K, device=dev, dtype=torch.int32)[:, None]          # [K, N]
            w = torch.full((K, N), BOOST_W1, dtype=torch.int32, device=dev)
            active = np.ones(K, dtype=bool)
            todev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
            ws = torch.empty(ops.boost_stump_ws_bytes(K, D), device=dev, dtype=torch.uint8) if X.is_cuda else None
            for rnd in range(self.n_rounds):
                if X.is_cuda:
                    out, _ = ops.boost_stump_u8(X, lab, K, w, ws=ws)
                else:
                    out, _ = boost_stump_host_bytes(X, lab, w, K)
                o = out.cpu().numpy()
                j, v, vh, nL, pL, n, p = (o[:, i] for i in range(7))
                thr = np.where(j >= 0, (v + vh) // 2, 0)
                left = np.where(j >= 0, 2 * pL > nL, 2 * p > n)                                 # a tie predicts negative
                right = np.where(j >= 0, 2 * (p - pL) > n - nL, 2 * p > n)
                byte = X[:, todev(np.maximum(j, 0), torch.int64)].t().to(torch.int64)           # [K, N]
                h = torch.where(byte > todev(thr, torch.int64)[:, None], todev(right, torch.bool)[:, None], todev(left, torch.bool)[:, None])
                miss = h != T
                e = (w.to(torch.int64) * miss).sum(1).cpu().numpy()
                mult = np.ones(K, dtype=np.float64)
                for k in np.nonzero(active)[0]:
                    ek, nk = int(e[k]), int(n[k])
                    if rnd == 0:
                        first_err[k] = ek / nk
                    if ek == 0:
                        alpha, active[k] = 1.0, False
                    elif 2 * ek >= nk:
                        active[k] = False
                        continue
                    else:
                        alpha = self.learning_rate * math.log(float(nk - ek) / float(ek))
                        mult[k] = math.exp(alpha)
                    records[k].append((float(k), float(rnd), float(j[k]), float(thr[k]), float(left[k]), float(right[k]), float(alpha)))
                # u = w (m where missed), the largest becomes 2^28: one multiplication, one division, an exact scaling, floor
                u = w.to(torch.float64) * torch.where(miss, todev(mult, torch.float64)[:, None], torch.ones((), dtype=torch.float64, device=dev))
                umax = u.max(1, keepdim=True)[0]
                keep = todev(active, torch.bool)[:, None]
                scaled = torch.floor(u / torch.where(keep, umax, torch.ones_like(umax)) * float(BOOST_W1))
                w = torch.where(keep, scaled, torch.zeros_like(scaled)).to(torch.int32)
                if on_round is not None:
                    on_round(rnd, w)
                if not active.any():
                    break
        rec = [r for k in range(K) for r in records[k]]
        self.coef = torch.tensor(rec, dtype=torch.float64).reshape(-1, 7)
        self.report = {"kind": "ab", "n_per_class": [int(c) for c in counts], "rounds": [len(r) for r in records],
                       "alpha_sum": [float(sum(q[6] for q in r)) for r in records], "first_err": [float(f) for f in first_err]}
        return self.report

    def stump_tables(self):
        """(feature, threshold, child int32 [Q'], tree_off int32 [Q + 1]): the Q stumps as trees for the tree apply path — a split is a
        3-node tree (left leaf 1, right leaf 2), a stump without one a single node (leaf 0)."""
        c = self.coef.numpy()
        f, t, ch, off = [], [], [], [0]
        for q in range(len(c)):
            if c[q, 2] >= 0:
                f += [int(c[q, 2]), -1, -1]; t += [int(c[q, 3]), 0, 0]; ch += [1, -1, -1]
            else:
                f += [-1]; t += [0]; ch += [-1]
            off.append(len(f))
        return tuple(np.array(a, dtype=np.int32) for a in (f, t, ch, off))

    def decision_bytes(self, Xu8):
        """F [M, K] float64 on the CPU: F_k = sum_m alpha_m sigma_m / sum_m alpha_m, sigma = +-1 the stump's prediction, added in round
        order on the host from the integer leaf numbers of the tree apply path, for both paths; 0 for a class without a stump."""
        if self.coef is None:
            raise RuntimeError("fit first")
        X = _check_row_size(_bytes_rows(Xu8))
        M = X.shape[0]
        c = self.coef.numpy()
        F = np.zeros((M, self.K), dtype=np.float64)
        if len(c) == 0:
            return torch.from_numpy(F)
        tabs = self.stump_tables()
        if X.is_cuda:
            X = X.contiguous()
            dtabs = [torch.from_numpy(t).to(X.device) for t in tabs]
        step = max(1, _BOOST_APPLY_ENTRIES // len(c))
        for m0 in range(0, M, step):
            xb = X[m0:m0 + step]
            if X.is_cuda:
                with torch.cuda.device(X.device):
                    leaf = ops.tree_apply_u8(xb, *dtabs).cpu().numpy()
            else:
                leaf = tree_apply_host_bytes(xb, *tabs).numpy()
            for q in range(len(c)):
                sigma = np.where(np.where(leaf[q] == 2, c[q, 5], c[q, 4]) > 0, 1.0, -1.0)
                F[m0:m0 + step, int(c[q, 0])] += c[q, 6] * sigma
        for k in range(self.K):
            tot = 0.0
            for a in c[c[:, 0] == k, 6]:
                tot += float(a)
            if tot > 0:
                F[:, k] /= tot
        return torch.from_numpy(F)

    def predict_proba_bytes(self, Xu8):
        """P [M, K] float64 on the CPU: 1 / (1 + exp(-2 F)), column 1 of scikit-learn's AdaBoostClassifier.predict_proba per class."""
        return torch.from_numpy(1.0 / (1.0 + np.exp(-2.0 * self.decision_bytes(Xu8).numpy())))
