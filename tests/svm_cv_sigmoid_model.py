"""float64 restatement of libsvm's sigmoid fit for a C-SVC (libSvm/src/svm.cpp: svm_binary_svc_probability :1940-2024,
svm_predict_values for two classes, Kernel::k_function :342-420, sigmoid_train :1752-1863), on top of
tests/svm_kernel_train_model.py.  The permutation is libc's: srand(seed), then j = i + rand() % (l - i).  k_function sums in
feature order without fusing -- x y, (x - y)^2 (not the xs_i + xs_j - 2 dot form of the Gram), min -- and the decision value adds
coef_s K_s in the model's order, then subtracts rho.  exp and log are libm's (math.exp, math.log; not numpy's)."""
import ctypes as C
import math
import time

import numpy as np

import svm_kernel_train_model as K
import svm_one_class_model as OC
import svm_train_model as M

FOLDS = 5
CONVERGED, MAX_ITERATIONS, LINE_SEARCH_FAILED = 0, 1, 2
_libc = None
last_train_seconds = 0.0


def libc():
    global _libc
    if _libc is None:
        _libc = C.CDLL("libc.so.6")
        _libc.srand.argtypes = [C.c_uint]
        _libc.srand.restype = None
        _libc.rand.restype = C.c_int
    return _libc


def libc_perm(seed, n):
    """the shuffle of svm_binary_svc_probability after srand(seed)"""
    lc = libc()
    lc.srand(seed)
    perm = list(range(n))
    for i in range(n):
        j = i + lc.rand() % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm, np.int32)


def folds(perm, n_pos):
    """per fold: (the training part's examples, positives in permuted order first; how many of them are positive; the held-out
    examples)"""
    n = len(perm)
    out = []
    for f in range(FOLDS):
        begin, end = f * n // FOLDS, (f + 1) * n // FOLDS
        rest = [int(p) for p in perm[:begin]] + [int(p) for p in perm[end:]]
        pos = [p for p in rest if p < n_pos]
        neg = [p for p in rest if p >= n_pos]
        out.append((np.array(pos + neg, np.int64), len(pos), np.array(perm[begin:end], np.int64)))
    return out


def constant_of(n_train_pos, n_train_neg):
    """None for a fold that trains; else the decision value of its held-out examples (:1987-1995)"""
    if n_train_pos > 0 and n_train_neg > 0:
        return None
    return 1.0 if n_train_pos > 0 else (-1.0 if n_train_neg > 0 else 0.0)


def k_function(x, sv, kernel):
    """K(x_h, sv_s) as k_function gives it: sums over the features in index order, one rounded operation at a time"""
    kind, p0, p1, p2 = kernel
    x = np.asarray(x, np.float32).astype(np.float64)
    sv = np.asarray(sv, np.float32).astype(np.float64)
    s = np.zeros((x.shape[0], sv.shape[0]))
    for c in range(x.shape[1]):
        a, b = x[:, c][:, None], sv[:, c][None, :]
        if kind == K.HIK:
            s = s + np.minimum(a, b)
        elif kind == K.RBF:
            diff = a - b
            s = s + diff * diff
        else:
            s = s + a * b
    if kind == K.POLY:
        return np.array([[K.powi(p0 * v + p1, int(p2)) for v in row] for row in s.tolist()]).reshape(s.shape)
    if kind == K.RBF:
        return np.array([[math.exp(-p0 * v) for v in row] for row in s.tolist()]).reshape(s.shape)
    return s


def decision(kmat, coef, rho):
    """svm_predict_values for two classes: sum += coef_s * K_s in the model's order (positives first), then - rho"""
    dec = np.zeros(kmat.shape[0])
    for s in range(kmat.shape[1]):
        dec = dec + float(coef[s]) * kmat[:, s]
    return dec - rho


def sigmoid_train(dec, n_pos):
    """sigmoid_train; labels_i > 0 for i < n_pos.  Returns A, B, the Newton iterations and the status."""
    dec = [float(v) for v in dec]
    l = len(dec)
    exp, log = math.exp, math.log
    prior1, prior0 = float(n_pos), float(l - n_pos)
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    hi, lo = (prior1 + 1.0) / (prior1 + 2.0), 1 / (prior0 + 2.0)
    t = [hi if i < n_pos else lo for i in range(l)]
    A, B = 0.0, log((prior0 + 1.0) / (prior1 + 1.0))

    def fun(a, b):
        f = 0.0
        for i in range(l):
            v = dec[i] * a + b
            if v >= 0:
                f += t[i] * v + log(1 + exp(-v))
            else:
                f += (t[i] - 1) * v + log(1 + exp(v))
        return f

    fval = fun(A, B)
    status = CONVERGED
    it = 0
    while it < max_iter:
        h11, h22, h21, g1, g2 = sigma, sigma, 0.0, 0.0, 0.0
        for i in range(l):
            v = dec[i] * A + B
            if v >= 0:
                p = exp(-v) / (1.0 + exp(-v))
                q = 1.0 / (1.0 + exp(-v))
            else:
                p = 1.0 / (1.0 + exp(v))
                q = exp(v) / (1.0 + exp(v))
            d2 = p * q
            h11 += dec[i] * dec[i] * d2
            h22 += d2
            h21 += dec[i] * d2
            d1 = t[i] - p
            g1 += dec[i] * d1
            g2 += d1
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= min_step:
            nA, nB = A + step * dA, B + step * dB
            nf = fun(nA, nB)
            if nf < fval + 0.0001 * step * gd:
                A, B, fval = nA, nB, nf
                break
            step = step / 2.0
        if step < min_step:
            status = LINE_SEARCH_FAILED
            break
        it += 1
    if it >= max_iter:
        status = MAX_ITERATIONS
    return A, B, it, status


def cross_validate(x, n_pos, kernel, perm, C_=1.0, weight_pos=1.0, weight_neg=1.0, eps=1e-4, fold_models=None):
    """svm_binary_svc_probability.  fold_models: per fold None or (alpha over the fold's rows, rho) to use in place of the float64
    training (the device's).  Returns dec (n, example order), probA, probB, Newton iterations, status, and per fold the trained
    model (None for a constant fold)."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    dec = np.zeros(n)
    models = []
    for f, (rows, npf, held) in enumerate(folds(perm, n_pos)):
        const = constant_of(npf, len(rows) - npf)
        if const is not None:
            dec[held] = const
            models.append(None)
            continue
        if fold_models is not None:
            alpha, rho = fold_models[f]
        else:
            r = K.train(x[rows], npf, kernel, 1.0, C_ * weight_pos, C_ * weight_neg, eps)
            alpha, rho = r["alpha"], r["rho"]
        models.append((np.asarray(alpha), rho))
        sv = np.flatnonzero(np.asarray(alpha) > 0)
        coef = np.where(sv < npf, 1.0, -1.0) * np.asarray(alpha)[sv]
        if len(held):
            dec[held] = decision(k_function(x[held], x[rows[sv]], kernel), coef, rho)
    A, B, it, status = sigmoid_train(dec, n_pos)
    return dec, A, B, it, status, models


# ---------------- the compiled reference ----------------
def _c_svc_parameter(kernel, C_, weight_pos, weight_neg, eps, probability, keep):
    wl = (C.c_int * 2)(1, -1)
    ww = (C.c_double * 2)(weight_pos, weight_neg)
    keep.extend([wl, ww])
    return M._Parameter(svm_type=0, cache_size=100.0, eps=eps, C=C_, nr_weight=2, weight_label=wl, weight=ww, nu=0.0, p=0.0, shrinking=0,
                        probability=probability, **OC.kernel_fields(kernel))


def libsvm_prob(ref, x, n_pos, kernel, seed, C_=1.0, weight_pos=1.0, weight_neg=1.0, eps=1e-4):
    """svm_train with probability = 1 directly behind srand(seed): libsvm's probA, probB"""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    keep, rows = OC.dense_nodes(x)
    ys = (C.c_double * n)(*M.labels(n_pos, n - n_pos).tolist())
    prob = M._Problem(n, ys, rows)
    held = []
    prm = _c_svc_parameter(kernel, C_, weight_pos, weight_neg, eps, 1, held)
    OC.bind(ref)
    global last_train_seconds
    libc().srand(seed)
    t0 = time.perf_counter()
    m = ref.svm_train(C.byref(prob), C.byref(prm))
    last_train_seconds = time.perf_counter() - t0   # svm_train alone: the five folds, the fit and the final model
    a, b = float(m.contents.probA[0]), float(m.contents.probB[0])
    ref.svm_free_and_destroy_model(C.byref(m))
    return a, b


def libsvm_cv_dec(ref, x, n_pos, kernel, perm, C_=1.0, weight_pos=1.0, weight_neg=1.0, eps=1e-4):
    """the decision values svm_binary_svc_probability hands to sigmoid_train, from libsvm's own svm_train and svm_predict_values
    fold by fold (libsvm does not return them)"""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    OC.bind(ref)
    keep_all, rows_all = OC.dense_nodes(x)
    dec = np.zeros(n)
    for rows, npf, held in folds(perm, n_pos):
        const = constant_of(npf, len(rows) - npf)
        if const is not None:
            dec[held] = const
            continue
        m_rows = (C.POINTER(M._Node) * len(rows))(*[rows_all[int(r)] for r in rows])
        ys = (C.c_double * len(rows))(*M.labels(npf, len(rows) - npf).tolist())
        prob = M._Problem(len(rows), ys, m_rows)
        held_keep = []
        prm = _c_svc_parameter(kernel, 1.0, C_ * weight_pos, C_ * weight_neg, eps, 0, held_keep)
        m = ref.svm_train(C.byref(prob), C.byref(prm))
        assert int(m.contents.label[0]) == 1
        for h in held:
            v = C.c_double()
            ref.svm_predict_values(m, rows_all[int(h)], C.byref(v))
            dec[int(h)] = v.value
        ref.svm_free_and_destroy_model(C.byref(m))
    return dec


# ---------------- the cases of the tests ----------------
HIK_KERNEL, LINEAR_KERNEL = (K.HIK, 0.0, 0.0, 0.0), (K.LINEAR, 0.0, 0.0, 0.0)
POLY_KERNEL, RBF_KERNEL = (K.POLY, 0.25, 1.0, 2.0), (K.RBF, 2.0, 0.0, 0.0)
# name: (rows, n_pos, n_neg, d, data seed, kernels, srand seed, C, weight_pos, weight_neg)
CASES = {
    "int65": ("integer", 20, 45, 12, 2, (HIK_KERNEL, LINEAR_KERNEL), 7, 2.0, 1.5, 0.75),
    "float55": ("float", 15, 40, 9, 3, (POLY_KERNEL, RBF_KERNEL), 9, 10.0, 1.0, 1.0),
    "one_pos": ("integer", 1, 11, 6, 4, (HIK_KERNEL,), 3, 1.0, 1.0, 1.0),     # fold 2 trains on no positive: -1
    "one_neg": ("integer", 11, 1, 6, 5, (HIK_KERNEL,), 3, 1.0, 1.0, 1.0),     # fold 4 trains on no negative: +1
    "pair": ("integer", 1, 1, 4, 6, (HIK_KERNEL,), 1, 1.0, 1.0, 1.0),         # folds 2 and 4 constant, 0, 1 and 3 hold nothing out
    "large": ("integer", 300, 990, 8, 7, (HIK_KERNEL,), 7, 1.0, 1.0, 1.0),    # folds of 1032 rows: the large solver
}
_case_cache = {}


def case(name):
    """(x, n_pos, kernels, perm, C, weight_pos, weight_neg) of a case"""
    if name not in _case_cache:
        rows, n_pos, n_neg, d, data_seed, kernels, seed, c, wp, wn = CASES[name]
        x = (OC.integer_rows if rows == "integer" else OC.float_rows)(n_pos, n_neg, d, data_seed)
        _case_cache[name] = (x, n_pos, kernels, libc_perm(seed, n_pos + n_neg), c, wp, wn)
    return _case_cache[name]
