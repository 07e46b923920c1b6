"""float64 model of liblinear's L2R_L2LOSS_SVC as liblinear::LibLinearClassifier trains it: the objective l2r_l2_svc_fun
(fun / grad / Hv) and the trust-region Newton method TRON (tron / trcg), restated step for step in numpy.

Rows are positives (+1) first, then negatives (-1); x is float32 and widened (liblinear stores double(float)); with bias a
constant-1 column is appended and regularised like any weight.  Sums run in numpy's order, not liblinear's: the result differs
from liblinear's by rounding only as long as both take the same branches, which is what `margin` is for -- the smallest relative
distance |a - b| / max(|a|, |b|) over every comparison the run took."""
import numpy as np

STOP_GRADIENT, STOP_MAX_ITER, STOP_ACTRED_ZERO, STOP_ACTRED_SMALL, STOP_CG_CAP, STOP_NONFINITE = 1, 2, 3, 4, 5, 6


def design(x, bias):
    X = np.asarray(x, np.float32).astype(np.float64)
    if bias:
        X = np.hstack([X, np.ones((X.shape[0], 1))])
    return X


def labels_and_c(n_pos, n_neg, C=1.0, weight_pos=1.0, weight_neg=1.0):
    y = np.concatenate([np.ones(n_pos), -np.ones(n_neg)])
    c = np.concatenate([np.full(n_pos, C * weight_pos), np.full(n_neg, C * weight_neg)])
    return y, c


class Objective:
    """l2r_l2_svc_fun: fun leaves z, grad the active set of that z, Hv works on the active set of the last grad"""

    def __init__(self, X, y, c):
        self.X, self.y, self.c = X, y, c
        self.z = None
        self.active = None
        self.tie_margin = np.inf

    def fun(self, w):
        self.z = self.y * (self.X @ w)
        d = 1.0 - self.z
        pos = d > 0
        return 0.5 * float(w @ w) + float(np.sum(self.c[pos] * d[pos] * d[pos]))

    def grad(self, w):
        z = self.z
        if len(z):
            self.tie_margin = min(self.tie_margin, float(np.min(np.abs(z - 1.0) / np.maximum(np.abs(z), 1.0))))
        self.active = z < 1
        a = self.active
        coef = self.c[a] * self.y[a] * (z[a] - 1.0)
        return w + 2.0 * (self.X[a].T @ coef)

    def hv(self, s):
        a = self.active
        return s + 2.0 * (self.X[a].T @ (self.c[a] * (self.X[a] @ s)))


class _Margin:
    def __init__(self):
        self.v = np.inf

    def cmp(self, a, b):
        m = max(abs(a), abs(b))
        if m > 0 and np.isfinite(m):
            self.v = min(self.v, abs(a - b) / m)


def _trcg(obj, delta, g, mg, cg_budget):
    """returns s, r, cg steps, whether the boundary was hit, whether the CG cap ended it"""
    s = np.zeros_like(g)
    r = -g
    d = r.copy()
    cgtol = 0.1 * np.sqrt(g @ g)
    cg = 0
    rtr = r @ r
    while True:
        rn = np.sqrt(r @ r)
        mg.cmp(rn, cgtol)
        if rn <= cgtol:
            return s, r, cg, 0, False
        if cg >= cg_budget:
            return s, r, cg, 0, True
        cg += 1
        hd = obj.hv(d)
        alpha = rtr / (d @ hd)
        s = s + alpha * d
        sn = np.sqrt(s @ s)
        mg.cmp(sn, delta)
        if sn > delta:
            s = s + (-alpha) * d
            std, sts, dtd = s @ d, s @ s, d @ d
            dsq = delta * delta
            rad = np.sqrt(std * std + dtd * (dsq - sts))
            alpha = (dsq - sts) / (std + rad) if std >= 0 else (rad - std) / dtd
            s = s + alpha * d
            r = r + (-alpha) * hd
            return s, r, cg, 1, False
        r = r + (-alpha) * hd
        rnew = r @ r
        beta = rnew / rtr
        d = d * beta + r
        rtr = rnew


def solver_tolerance(n_pos, n_neg, eps=0.01):
    """train_one's primal_solver_tol"""
    return eps * max(min(n_pos, n_neg), 1) / (n_pos + n_neg)


def tron(x, n_pos, n_neg, C=1.0, bias=False, eps=0.01, solver_tol=0.0, weight_pos=1.0, weight_neg=1.0, max_iter=1000,
         max_cg_steps=0):
    """dict with w, f, gnorm, gnorm0, delta, iterations, cg_steps, trace [(cg, boundary, accepted)], stop, converged, n_active,
    margin"""
    X = design(x, bias)
    y, c = labels_and_c(n_pos, n_neg, C, weight_pos, weight_neg)
    obj = Objective(X, y, c)
    tol = solver_tol if solver_tol > 0 else solver_tolerance(n_pos, n_neg, eps if eps > 0 else 0.01)
    m = X.shape[1]
    if max_cg_steps == 0:
        max_cg_steps = 100 * m + 1000
    eta0, eta1, eta2 = 1e-4, 0.25, 0.75
    sigma1, sigma2, sigma3 = 0.25, 0.5, 4.0
    mg = _Margin()
    w = np.zeros(m)
    trace = []
    cg_total = 0
    stop = 0
    with np.errstate(all="ignore"):
        f = obj.fun(w)
        g = obj.grad(w)
        delta = np.sqrt(g @ g)
        gnorm0 = gnorm = delta
        it = 1
        if not (np.isfinite(f) and np.isfinite(gnorm)):
            stop = STOP_NONFINITE
        else:
            mg.cmp(gnorm, tol * gnorm0)
            if gnorm <= tol * gnorm0:
                stop = STOP_GRADIENT
        while not stop:
            if it > max_iter:
                stop = STOP_MAX_ITER
                break
            s, r, cg, boundary, capped = _trcg(obj, delta, g, mg, max_cg_steps - cg_total)
            cg_total += cg
            if capped:
                stop = STOP_CG_CAP
                break
            w_new = w + s
            gs = g @ s
            prered = -0.5 * (gs - s @ r)
            fnew = obj.fun(w_new)
            if not np.isfinite(fnew):
                stop = STOP_NONFINITE
                break
            actred = f - fnew
            snorm = np.sqrt(s @ s)
            if it == 1:
                delta = min(delta, snorm)
            if fnew - f - gs <= 0:
                alpha = sigma3
            else:
                alpha = max(sigma1, -0.5 * (gs / (fnew - f - gs)))
            mg.cmp(actred, eta0 * prered)
            if actred < eta0 * prered:
                delta = min(max(alpha, sigma1) * snorm, sigma2 * delta)
            else:
                mg.cmp(actred, eta1 * prered)
                if actred < eta1 * prered:
                    delta = max(sigma1 * delta, min(alpha * snorm, sigma2 * delta))
                else:
                    mg.cmp(actred, eta2 * prered)
                    if actred < eta2 * prered:
                        delta = max(sigma1 * delta, min(alpha * snorm, sigma3 * delta))
                    else:
                        delta = max(delta, min(alpha * snorm, sigma3 * delta))
            accepted = actred > eta0 * prered
            trace.append((cg, boundary, int(accepted)))
            if accepted:
                it += 1
                w = w_new
                f = fnew
                g = obj.grad(w)
                gnorm = np.sqrt(g @ g)
                if not np.isfinite(gnorm):
                    stop = STOP_NONFINITE
                    break
                mg.cmp(gnorm, tol * gnorm0)
                if gnorm <= tol * gnorm0:
                    stop = STOP_GRADIENT
                    break
            if abs(actred) <= 0 and prered <= 0:
                stop = STOP_ACTRED_ZERO
                break
            if abs(actred) <= 1.0e-12 * abs(f) and abs(prered) <= 1.0e-12 * abs(f):
                stop = STOP_ACTRED_SMALL
                break
    return dict(w=w, f=float(f), gnorm=float(gnorm), gnorm0=float(gnorm0), delta=float(delta), iterations=it - 1, cg_steps=cg_total,
                trace=np.array(trace, np.int32).reshape(-1, 3), stop=stop, converged=int(stop == STOP_GRADIENT),
                n_active=int(np.count_nonzero(obj.active)) if obj.active is not None else 0,
                margin=float(min(mg.v, obj.tie_margin)))


def evaluate(x, n_pos, n_neg, w, s=None, C=1.0, bias=False, weight_pos=1.0, weight_neg=1.0):
    """f, g and (with s) Hs at w"""
    X = design(x, bias)
    y, c = labels_and_c(n_pos, n_neg, C, weight_pos, weight_neg)
    obj = Objective(X, y, c)
    w = np.asarray(w, np.float64)
    with np.errstate(all="ignore"):
        f = obj.fun(w)
        g = obj.grad(w)
        hs = obj.hv(np.asarray(s, np.float64)) if s is not None else None
    return f, g, hs


def bounds(x, n_pos, n_neg, w, s=None, C=1.0, bias=False, weight_pos=1.0, weight_neg=1.0):
    """Componentwise rounding bounds for a double evaluation in any summation order: with u = 2^-53 and
    gamma = (n + d + 8) u, |f - f'| <= gamma (w.w + 2 sum_I C_i (1 + |x_i| |w|)^2) and, while no row changes sides of z = 1,
    |g - g'| <= gamma (|w| + 2 |X_I|^T (C (1 + 2 |X_I| |w|))), |Hs - Hs'| <= gamma (|s| + 2 |X_I|^T (C |X_I| |s|)).
    Returns (Bf, Bg, Bhs)."""
    X = design(x, bias)
    y, c = labels_and_c(n_pos, n_neg, C, weight_pos, weight_neg)
    w = np.asarray(w, np.float64)
    n, m = X.shape
    gamma = (n + m + 8) * 2.0 ** -53
    A = np.abs(X)
    a = y * (X @ w) < 1
    zb = A @ np.abs(w)
    bf = gamma * (float(w @ w) + 2.0 * float(np.sum(c[a] * (1.0 + zb[a]) ** 2)))
    bg = gamma * (np.abs(w) + 2.0 * (A[a].T @ (c[a] * (1.0 + 2.0 * zb[a]))))
    bh = None
    if s is not None:
        s = np.abs(np.asarray(s, np.float64))
        bh = gamma * (s + 2.0 * (A[a].T @ (c[a] * (A[a] @ s))))
    return bf, bg, bh
