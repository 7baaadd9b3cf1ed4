"""One-vs-rest linear support-vector classifier with Platt scaling on cache bytes: the last line of the reference's
classifier panel, `OneVsRestClassifier(SVC(kernel='linear', probability=True))` of downstream.py:67, with x = byte / 255.

The kernel matrix is K_ij = <b_i, b_j> / 65025 with the exact integer dot product <b_i, b_j> = (s_i + s_j - d2_ij) / 2 of the byte rows:
s their squared norms, d2 their squared distance (below 2^32 for rows of at most 65536 bytes).  Per class k and labels y = +1 / -1 the dual

    minimise 1/2 a'Qa - e'a   subject to 0 <= a <= C and y'a = 0,   Q_ij = y_i y_j K_ij

is solved by LIBSVM's SMO (`smo_host`): second-order working-set selection, the clipped two-variable update, no shrinking, ties in both
selections to the lowest row index.  Every floating-point operation of the loop is elementwise or an exact maximum / minimum with its
index; there is no sum inside it.  That is what lets cslgan_svc_smo_f64 (csrc/svm_kernels.hip) return the same bits.

Platt scaling costs no extra pass: per class there are 1 + folds problems over the SAME rows, each with an `active` mask.  Inactive rows are
never selected but their gradient entries are updated like all others, so y_t (G_t + 1) - rho is the held-out decision value of row t.
`sigmoid_train` is LIBSVM's Newton fit of P = 1 / (1 + exp(A f + B)) to those values.  The sigmoid of a linear score is a logistic model,
so the fitted estimator is a coefficient matrix U [D + 1, K] of csl_gan_amd.classify.proba_host_bytes / cslgan_ovr_logreg_proba_u8.
"""
import numpy as np
import torch

from . import classify, ops

TAU = 1e-12                 # replaces a curvature that is not positive
SCALE = 65025.0             # K = <b_i, b_j> / 255^2
MAX_ROWS = ops.SVM_MAX_ROWS  # the stored matrix: 65536 rows are 16 GiB
MAX_PROBLEMS = 96           # 16 classes x (1 + 5 folds) workgroups
_HOST_MATRIX_ROWS = 4096    # smo_host keeps K as one float64 matrix up to here and forms its rows on demand beyond
_DEVICE_CHUNK = 1 << 22     # row updates of one launch: chunk = _DEVICE_CHUNK / n iterations, 64 .. 4096, so no launch runs for long


def byte_sqnorms(X, block=4096):
    """s [n] int64: the exact squared norms of uint8 rows X [n, D], numpy."""
    X = np.asarray(X)
    return np.concatenate([(X[r0:r0 + block].astype(np.int64) ** 2).sum(1) for r0 in range(0, len(X), block)])


def gram_d2_host(X, block=1024):
    """(d2 [n, n] uint32, s [n] int64) of uint8 rows X [n, D]: the definition of cslgan_gram_d2_u8.  The dot products are float64 matrix
    products of integers below 2^53, hence exact in any order."""
    X = np.ascontiguousarray(X, dtype=np.uint8)
    n, D = X.shape
    if not 1 <= D <= 65536:
        raise ValueError("rows of %d bytes; the squared distance takes 1 .. 65536" % D)
    s = byte_sqnorms(X)
    Xf = X.astype(np.float64)
    d2 = np.empty((n, n), dtype=np.uint32)
    for r0 in range(0, n, block):
        dot = (Xf[r0:r0 + block] @ Xf.T).astype(np.int64)
        d2[r0:r0 + block] = (s[r0:r0 + block, None] + s[None, :] - 2 * dot).astype(np.uint32)
    return d2, s


def kernel_rows(d2, s, rows):
    """K[rows, :] in float64: ((s_i + s_j - d2_ij) / 2) / 65025, an exact integer, one conversion and one division per entry."""
    rows = np.atleast_1d(rows)
    return ((s[rows, None] + s[None, :] - d2[rows, :s.shape[0]].astype(np.int64)) // 2).astype(np.float64) / SCALE


def smo_start(n):
    """The state of a problem before its first iteration: alpha = 0, gradient = -1."""
    return {"alpha": np.zeros(n), "grad": np.full(n, -1.0), "iterations": 0, "done": False}


def smo_host(d2, s, y, active, C=1.0, tol=1e-3, max_iter=10_000_000, state=None, chunk=None, on_pair=None):
    """THE definition of cslgan_svc_smo_f64: LIBSVM's SMO on one dual problem.  d2 [n, >= n] uint32 and s [n] int64 as gram_d2_host returns
    them, y [n] of +1 / -1, active [n] bool.  Runs from `state` (smo_start(n) when absent; updated in place and returned) for at most
    `chunk` iterations and never past max_iter in total.  state["done"] turns True where m(a) - M(a) < tol or no pair is left; a problem
    that stops at max_iter stays not done.  The result does not depend on how the iterations are cut into chunks.
    on_pair(i, j, quad) is called with every working pair and its curvature, TAU where it was not positive.
    Every floating-point operation below is elementwise or an exact max / min / argmax / argmin (first index on ties)."""
    s = np.asarray(s, dtype=np.int64)
    n = s.shape[0]
    y = np.asarray(y, dtype=np.int64)
    pos = y > 0
    active = np.asarray(active, dtype=bool)
    state = smo_start(n) if state is None else state
    alpha, G = state["alpha"], state["grad"]
    Kd = s.astype(np.float64) / SCALE
    Kall = kernel_rows(d2, s, np.arange(n)) if n <= _HOST_MATRIX_ROWS else None
    row = (lambda r: Kall[r]) if Kall is not None else (lambda r: kernel_rows(d2, s, r)[0])
    inf = np.inf
    budget = max_iter - state["iterations"]
    budget = budget if chunk is None else min(budget, chunk)
    for _ in range(max(0, budget)):
        if state["done"]:
            break
        val = np.where(pos, -G, G)                                             # -y G
        up = active & np.where(pos, alpha < C, alpha > 0.0)
        low = active & np.where(pos, alpha > 0.0, alpha < C)
        if not up.any():
            state["done"] = True
            break
        vu = np.where(up, val, -inf)
        i = int(np.argmax(vu))
        gmax = vu[i]
        Ki = row(i)
        gmin = np.where(low, val, inf).min()
        b = gmax - val
        cand = low & (b > 0.0)
        if not cand.any() or gmax - gmin < tol:
            state["done"] = True
            break
        quad = (Kd[i] + Kd) - 2.0 * Ki
        quad = np.where(quad > 0.0, quad, TAU)
        obj = np.where(cand, -(b * b) / quad, inf)
        j = int(np.argmin(obj))
        Kj = row(j)

        q = float(quad[j])
        if on_pair is not None:
            on_pair(i, j, q)
        gi, gj, ai, aj = float(G[i]), float(G[j]), float(alpha[i]), float(alpha[j])
        ai_old, aj_old = ai, aj
        if y[i] != y[j]:
            delta = (-gi - gj) / q
            diff = ai - aj
            ai += delta
            aj += delta
            if diff > 0.0:
                if aj < 0.0:
                    aj, ai = 0.0, diff
            elif ai < 0.0:
                ai, aj = 0.0, -diff
            if diff > 0.0:
                if ai > C:
                    ai, aj = C, C - diff
            elif aj > C:
                aj, ai = C, C + diff
        else:
            delta = (gi - gj) / q
            total = ai + aj
            ai -= delta
            aj += delta
            if total > C:
                if ai > C:
                    ai, aj = C, total - C
            elif aj < 0.0:
                aj, ai = 0.0, total
            if total > C:
                if aj > C:
                    aj, ai = C, total - C
            elif ai < 0.0:
                ai, aj = 0.0, total
        dai, daj = ai - ai_old, aj - aj_old
        Qi = np.where(y == y[i], Ki, -Ki)
        Qj = np.where(y == y[j], Kj, -Kj)
        G += (Qi * dai) + (Qj * daj)
        alpha[i], alpha[j] = ai, aj
        state["iterations"] += 1
    return state


def rho_host(alpha, G, y, active, C):
    """LIBSVM's calculate_rho over the active rows, in row order: the mean of y G over the free rows (a running sum from the first free row
    to the last), else the midpoint of the bounds that the rows at 0 and at C leave."""
    ub, lb, total, free = np.inf, -np.inf, 0.0, 0
    for t in np.nonzero(active)[0]:
        yg = float(y[t]) * float(G[t])
        if alpha[t] >= C:
            if y[t] < 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        elif alpha[t] <= 0.0:
            if y[t] > 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        else:
            total += yg
            free += 1
    return total / free if free else (ub + lb) / 2.0


def fold_assignment(y, folds, seed):
    """fold [n] in 0 .. folds - 1: round-robin along one permutation of the rows drawn from `seed`, dealt separately within the positives
    and the negatives of y (+1 / -1).  A side of at least 2 rows is never all in one fold, so every fold's training set keeps both signs."""
    y = np.asarray(y)
    perm = np.random.default_rng(seed).permutation(len(y))
    fold = np.empty(len(y), dtype=np.int64)
    for side in (perm[y[perm] > 0], perm[y[perm] < 0]):
        fold[side] = np.arange(len(side)) % folds
    return fold


def problems_of(labels, K, folds, seed):
    """(Y int8 [P, n], active bool [P, n], fold int64 [K, n]) with P = K (1 + folds): problem k (1 + folds) is class k on all rows, problem
    k (1 + folds) + 1 + f the same class without the rows of its fold f.  Refuses a class with fewer than 2 rows on either side."""
    labels = np.asarray(labels).reshape(-1)
    n = len(labels)
    Y = np.empty((K * (1 + folds), n), dtype=np.int8)
    active = np.ones((K * (1 + folds), n), dtype=bool)
    fold = np.empty((K, n), dtype=np.int64)
    for k in range(K):
        yk = np.where(labels == k, 1, -1)
        n_pos = int((yk > 0).sum())
        if n_pos < 2 or n - n_pos < 2:
            raise ValueError("class %d has %d rows against %d; the %d-fold Platt scaling needs at least 2 on each side" % (k, n_pos, n - n_pos, folds))
        fold[k] = fold_assignment(yk, folds, seed)
        p0 = k * (1 + folds)
        Y[p0:p0 + 1 + folds] = yk
        for f in range(folds):
            active[p0 + 1 + f] = fold[k] != f
    return Y, active, fold


def platt_targets(y):
    """(t [n], A0, B0) of LIBSVM's sigmoid_train: the targets (N+ + 1) / (N+ + 2) and 1 / (N- + 2), and the starting point (0, log((N- + 1) /
    (N+ + 1)))."""
    y = np.asarray(y)
    n_pos, n_neg = float((y > 0).sum()), float((y < 0).sum())
    t = np.where(y > 0, (n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0))
    return t, 0.0, float(np.log((n_neg + 1.0) / (n_pos + 1.0)))


def platt_objective(f, t, A, B):
    """(value, dA, dB) of LIBSVM's regularised cross-entropy sum t (A f + B) + log(1 + exp(-(A f + B))) in float64, the overflow-free form."""
    z = f * A + B
    value = float(np.where(z >= 0, t * z + np.log1p(np.exp(-np.abs(z))), (t - 1.0) * z + np.log1p(np.exp(-np.abs(z)))).sum())
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    d = t - p
    return value, float((f * d).sum()), float(d.sum())


def sigmoid_train(f, y, max_iter=100, min_step=1e-10, sigma=1e-12, eps=1e-5):
    """(A, B) of P(y = +1 | f) = 1 / (1 + exp(A f + B)): LIBSVM's sigmoid_train, Newton with backtracking, float64, on the host."""
    f = np.asarray(f, dtype=np.float64)
    t, A, B = platt_targets(y)
    fval, g1, g2 = platt_objective(f, t, A, B)
    for _ in range(max_iter):
        z = f * A + B
        e = np.exp(-np.abs(z))
        p = np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        d2 = p * (1.0 - p)
        h11, h22, h21 = sigma + float((f * f * d2).sum()), sigma + float(d2.sum()), float((f * d2).sum())
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA, dB = -(h22 * g1 - h21 * g2) / det, -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= min_step:
            newf, n1, n2 = platt_objective(f, t, A + step * dA, B + step * dB)
            if newf < fval + 0.0001 * step * gd:
                A, B, fval, g1, g2 = A + step * dA, B + step * dB, newf, n1, n2
                break
            step /= 2.0
        else:
            break                                                              # the line search failed: LIBSVM keeps the point too
    return A, B


def _solve_host(d2, s, Y, active, C, tol, max_iter):
    states = [smo_host(d2, s, Y[p], active[p], C, tol, max_iter) for p in range(len(Y))]
    return (np.stack([st["alpha"] for st in states]), np.stack([st["grad"] for st in states]),
            np.array([st["iterations"] for st in states], dtype=np.int64), np.array([st["done"] for st in states]))


def device_chunk(n):
    return max(64, min(4096, _DEVICE_CHUNK // max(int(n), 1)))


def solve_device(d2, s, Y, active, C, tol, max_iter, chunk=None):
    """(alpha [P, n], grad [P, n], iterations [P], done [P]) as numpy from repeated cslgan_svc_smo_f64 launches of `chunk` iterations on
    d2 (ops.gram_d2's device matrix) and s (int64 on the device), all P problems per launch."""
    dev = d2.device
    P, n = Y.shape
    chunk = device_chunk(n) if chunk is None else int(chunk)
    Yd = torch.from_numpy(np.ascontiguousarray(Y, dtype=np.int8)).to(dev)
    Md = torch.from_numpy(np.ascontiguousarray(active, dtype=np.uint8)).to(dev)
    alpha = torch.zeros((P, n), dtype=torch.float64, device=dev)
    grad = torch.full((P, n), -1.0, dtype=torch.float64, device=dev)
    iters = torch.zeros(P, dtype=torch.int64, device=dev)
    done = torch.zeros(P, dtype=torch.int32, device=dev)
    while True:
        ops.svc_smo(d2, s, Yd, Md, C, tol, chunk, max_iter, alpha, grad, iters, done)
        it, dn = iters.cpu().numpy(), done.cpu().numpy() != 0
        if (dn | (it >= max_iter)).all():
            return alpha.cpu().numpy(), grad.cpu().numpy(), it, dn


def _byte_sqnorms_device(X, block=4096):
    return torch.cat([(X[r0:r0 + block].to(torch.int32) ** 2).sum(1, dtype=torch.int64) for r0 in range(0, X.shape[0], block)])


class OvrSvc:
    """`OvrSvc(n_classes).fit_bytes(Xu8, y)` then `.predict_proba_bytes(Xu8)`.  Rows on a HIP device: the matrix by cslgan_gram_d2_u8 and
    all K (1 + folds) problems by cslgan_svc_smo_f64; anything else: gram_d2_host and smo_host.  Everything after the solve (rho, the
    held-out decision values, the sigmoids, w) is the same float64 host code for both, and the solves agree bit for bit, so `coef` does
    too: U [D + 1, K] float64 on the host with U[:D, k] = -A_k w_k and U[D, k] = A_k rho_k - B_k, the logistic form of Platt's sigmoid."""

    def __init__(self, n_classes, C=1.0, tol=1e-3, folds=5, seed=0, max_iter=10_000_000):
        self.K = classify._check_classes(n_classes)
        self.C, self.tol, self.folds, self.seed, self.max_iter = float(C), float(tol), int(folds), int(seed), int(max_iter)
        if not (0 < self.C < np.inf and 0 < self.tol < np.inf):
            raise ValueError("C and tol must be finite numbers > 0, got %r and %r" % (C, tol))
        if not 2 <= self.folds or self.K * (1 + self.folds) > MAX_PROBLEMS:
            raise ValueError("folds = %d: %d classes take 2 .. %d folds" % (self.folds, self.K, MAX_PROBLEMS // self.K - 1))
        if self.max_iter < 0:
            raise ValueError("max_iter = %d must be >= 0" % self.max_iter)
        self.coef, self.report, self.solution = None, None, None

    def fit_bytes(self, Xu8, y):
        X = classify._bytes_rows(Xu8).contiguous()
        y = torch.as_tensor(y)
        classify._check_rows(self.K, X, y)
        classify._check_row_size(X)
        n, D = X.shape
        if n > MAX_ROWS:
            raise ValueError("%d rows; the stored kernel matrix takes at most %d (16 GiB): a larger set needs shrinking and a row cache" % (n, MAX_ROWS))
        labels = y.detach().cpu().numpy().astype(np.int64).reshape(-1)
        Y, active, fold = problems_of(labels, self.K, self.folds, self.seed)
        if X.is_cuda:
            with torch.cuda.device(X.device):
                xs, sq = ops.nn_prepare(X)
                d2 = ops.gram_d2(xs, sq)
                del xs
                alpha, G, iters, done = solve_device(d2, _byte_sqnorms_device(X), Y, active, self.C, self.tol, self.max_iter)
                del d2
            Xh = X.cpu().numpy()
        else:
            Xh = X.numpy()
            d2, s = gram_d2_host(Xh)
            alpha, G, iters, done = _solve_host(d2, s, Y, active, self.C, self.tol, self.max_iter)
        self.solution = {"alpha": alpha, "grad": G, "iterations": iters, "done": done, "Y": Y, "active": active, "fold": fold}
        return self._finish(Xh, labels)

    def _finish(self, Xh, labels):
        """rho, held-out decision values, sigmoids and w from the solved problems: float64 on the host, one order."""
        sol, K, F = self.solution, self.K, self.folds
        n, D = Xh.shape
        U = np.zeros((D + 1, K))
        rep = {"n_per_class": np.bincount(labels, minlength=K).tolist(), "iterations": [], "converged": [], "n_sv": [], "n_bsv": [], "rho": [],
               "A": [], "B": []}
        for k in range(K):
            p0 = k * (1 + F)
            yk = sol["Y"][p0].astype(np.float64)
            dec = np.empty(n)
            for f in range(F):
                p = p0 + 1 + f
                held = ~sol["active"][p]
                dec[held] = yk[held] * (sol["grad"][p][held] + 1.0) - rho_host(sol["alpha"][p], sol["grad"][p], sol["Y"][p], sol["active"][p], self.C)
            A, B = sigmoid_train(dec, sol["Y"][p0])
            a = sol["alpha"][p0]
            rho = rho_host(a, sol["grad"][p0], sol["Y"][p0], sol["active"][p0], self.C)
            sv = np.nonzero(a > 0.0)[0]
            w = np.zeros(D)
            for r0 in range(0, len(sv), 2048):                                  # w = sum a_i y_i x_i over the support vectors, in row blocks
                rows = sv[r0:r0 + 2048]
                w += (a[rows] * yk[rows]) @ (Xh[rows].astype(np.float64) / 255.0)
            U[:D, k], U[D, k] = -A * w, A * rho - B
            rep["iterations"].append(int(sol["iterations"][p0]))
            rep["converged"].append(bool(sol["done"][p0]))
            rep["n_sv"].append(int(len(sv)))
            rep["n_bsv"].append(int((a >= self.C).sum()))
            rep["rho"].append(float(rho))
            rep["A"].append(float(A))
            rep["B"].append(float(B))
        rep["iterations_total"] = int(sol["iterations"].sum())
        self.coef, self.report = torch.from_numpy(U), rep
        return rep

    def predict_proba_bytes(self, Xu8):
        """P [M, K] of uint8 rows: the normalised sigmoids, OneVsRestClassifier.predict_proba's rule — ops.ovr_logreg_proba_u8 on a device
        (float32), classify.proba_host_bytes on the host (float64)."""
        return classify._proba(self, classify._bytes_rows(Xu8), classify.proba_host_bytes, lambda X, U: ops.ovr_logreg_proba_u8(X.contiguous(), U))
