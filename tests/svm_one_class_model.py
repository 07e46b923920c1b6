"""numpy float64 restatement of libsvm's one-class training (libSvm/src/svm.cpp: solve_one_class :1577-1607, the gradient
Solver::Solve builds from the start state :571-588, its loop with every label +1, calculate_rho, ONE_CLASS_Q), on top of
tests/svm_train_model.py and tests/svm_kernel_train_model.py, and a ctypes caller of the compiled reference's svm_train with
svm_type ONE_CLASS.  Every operation is one IEEE double operation in libsvm's order: the element-wise numpy expressions below
round each product and each sum once, as the scalar loops of libsvm do."""
import ctypes as C
import time

import numpy as np

import svm_kernel_train_model as K
import svm_train_model as M

NUS = [0.02, 0.26, 0.5, 1.0]   # on 40 rows: nu n < 1, fractional, integral, every alpha at its bound (rho = inf)
INF = float("inf")
last_train_seconds = 0.0


def integer_rows(n_pos, n_neg, d, seed):
    """rows whose histogram intersections and dot products are exact in float: Q is libsvm's own bits for HIK and LINEAR"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(3, 16, (n_pos, d)), rng.integers(0, 12, (n_neg, d))]).astype(np.float32)


def float_rows(n_pos, n_neg, d, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(0.3, 0.2, (n_pos, d)), rng.normal(0.0, 0.2, (n_neg, d))]).astype(np.float32)


def q_one_class(k):
    """ONE_CLASS_Q: Q_ij = (Qfloat)K_ij, QD_i = K_ii"""
    return k.astype(np.float32), np.diag(k).copy()


def start_alpha(n, nu):
    """solve_one_class :1586-1593"""
    nb = int(nu * n)
    alpha = np.zeros(n)
    alpha[:nb] = 1.0
    if nb < n:
        alpha[nb] = nu * n - nb
    return alpha


def start_gradient(q, alpha):
    """Solve :571-588 with p = 0: G[j] += alpha_i * Q_i[j] over the i with alpha_i > 0, ascending"""
    qf = np.asarray(q, np.float32).astype(np.float64)
    G = np.zeros(len(alpha))
    for i in range(len(alpha)):
        if alpha[i] > 0:
            G = G + float(alpha[i]) * qf[i]
    return G


def _last(mask_values, target):
    """the highest index whose value equals target (a scan in index order with >= / <=)"""
    hit = np.flatnonzero(mask_values == target)
    return int(hit[-1]) if len(hit) else -1


def smo(q, qd, alpha, G, eps=1e-4, max_iterations=0):
    """Solver::Solve's loop without shrinking for y = +1 and C = 1 throughout, from the given state"""
    n = len(alpha)
    if max_iterations <= 0:
        max_iterations = M.default_max_iterations(n)
    Q = np.asarray(q, np.float32).astype(np.float64)
    QD = np.asarray(qd, np.float64)
    alpha, G = np.array(alpha, np.float64), np.array(G, np.float64)
    it, converged = 0, 0
    while it < max_iterations:
        up = alpha < 1.0
        i, gmax = -1, -INF
        if up.any():
            cand = np.where(up, -G, -INF)
            gmax = float(cand.max())
            i = _last(cand, gmax)
        low = alpha > 0.0
        j, gmax2 = -1, -INF
        if low.any():
            gmax2 = float(np.where(low, G, -INF).max())
        if i >= 0 and low.any():
            gd = gmax + G
            ok = low & (gd > 0)
            if ok.any():
                quad = QD[i] + QD - 2.0 * Q[i]
                with np.errstate(divide="ignore", invalid="ignore"):
                    od = np.where(quad > 0, -(gd * gd) / quad, -(gd * gd) / M.TAU)
                od = np.where(ok, od, INF)
                j = _last(od, float(od.min()))
        if gmax + gmax2 < eps or i < 0 or j < 0:
            converged = 1
            break
        it += 1
        oi, oj = float(alpha[i]), float(alpha[j])
        quad = float(QD[i]) + float(QD[j]) - 2 * float(Q[i, j])
        if quad <= 0:
            quad = M.TAU
        delta = (float(G[i]) - float(G[j])) / quad
        s = oi + oj
        ai, aj = oi - delta, oj + delta
        if s > 1.0:
            if ai > 1.0:
                ai, aj = 1.0, s - 1.0
        elif aj < 0:
            aj, ai = 0.0, s
        if s > 1.0:
            if aj > 1.0:
                aj, ai = 1.0, s - 1.0
        elif ai < 0:
            ai, aj = 0.0, s
        alpha[i], alpha[j] = ai, aj
        G = G + (Q[i] * (ai - oi) + Q[j] * (aj - oj))
    return alpha, G, it, converged


def finish(alpha, G):
    """calculate_rho and the counts as for a problem of positives with C = 1; the objective with the linear term 0"""
    rho, _, nsv, nb = M.finish(alpha, G, len(alpha), 1.0, 1.0)
    obj = 0.0
    for a, g in zip(alpha.tolist(), G.tolist()):
        obj += a * (g + 0.0)
    return rho, obj / 2, nsv, nb


def train(x, kernel, nu, eps=1e-4, max_iterations=0, q=None, qd=None):
    """the whole path; q / qd: a Gram the caller supplies (the device's) in place of the float64 one"""
    x = np.asarray(x, np.float32)
    if q is None:
        q, qd = q_one_class(K.kernel64(x, kernel))
    a0 = start_alpha(x.shape[0], nu)
    g0 = start_gradient(q, a0)
    alpha, G, it, conv = smo(q, qd, a0, g0, eps, max_iterations)
    rho, obj, nsv, nb = finish(alpha, G)
    sv_index = np.flatnonzero(alpha > 0).astype(np.int32)
    return dict(alpha=alpha, G=G, G0=g0, iterations=it, converged=conv, rho=rho, objective=obj, n_sv=nsv, n_bounded=nb, sv_index=sv_index,
                coefficients=alpha[sv_index].astype(np.float32), support_vectors=x[sv_index])


def dense_nodes(x):
    """(keep-alive, row pointers) of dense svm_node lists"""
    x = np.asarray(x, np.float32)
    n, d = x.shape
    nodes = (M._Node * ((d + 1) * n))()
    rows = (C.POINTER(M._Node) * n)()
    for i in range(n):
        base = i * (d + 1)
        for k in range(d):
            nodes[base + k].index = k + 1
            nodes[base + k].value = float(x[i, k])
        nodes[base + d].index = -1
        rows[i] = C.cast(C.byref(nodes, base * C.sizeof(M._Node)), C.POINTER(M._Node))
    return nodes, rows


def bind(ref):
    ref.svm_set_print_string_function.argtypes = [M._PRINT]
    ref.svm_set_print_string_function.restype = None
    ref.svm_set_print_string_function(M._quiet)
    ref.svm_train.restype = C.POINTER(M._Model)
    ref.svm_train.argtypes = [C.POINTER(M._Problem), C.POINTER(M._Parameter)]
    ref.svm_free_and_destroy_model.argtypes = [C.POINTER(C.POINTER(M._Model))]
    ref.svm_free_and_destroy_model.restype = None
    ref.svm_predict_values.argtypes = [C.POINTER(M._Model), C.POINTER(M._Node), C.POINTER(C.c_double)]
    ref.svm_predict_values.restype = C.c_double


def kernel_fields(kernel):
    kind, p0, p1, p2 = kernel
    return dict(kernel_type=K.LIBSVM_KERNEL_TYPE[kind], degree=int(p2) if kind == K.POLY else 0,
                gamma=float(p0) if kind in (K.POLY, K.RBF) else 0.0, coef0=float(p1) if kind == K.POLY else 0.0)


def libsvm_train(ref, x, kernel, nu, eps=1e-4):
    """svm_train of the compiled reference with svm_type ONE_CLASS (2) and LibSvmClassifier's other parameters.
    Returns alpha (n), rho, the model's sv_indices (0-based)."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    keep, rows = dense_nodes(x)
    ys = (C.c_double * n)(*([1.0] * n))
    prob = M._Problem(n, ys, rows)
    prm = M._Parameter(svm_type=2, cache_size=100.0, eps=eps, C=1.0, nr_weight=0, weight_label=None, weight=None, nu=float(nu), p=0.0,
                       shrinking=0, probability=0, **kernel_fields(kernel))
    bind(ref)
    global last_train_seconds
    t0 = time.perf_counter()
    m = ref.svm_train(C.byref(prob), C.byref(prm))
    last_train_seconds = time.perf_counter() - t0
    mm = m.contents
    alpha = np.zeros(n)
    sv_index = np.array([mm.sv_indices[s] - 1 for s in range(mm.l)], np.int32)
    alpha[sv_index] = [mm.sv_coef[0][s] for s in range(mm.l)]
    rho = float(mm.rho[0])
    ref.svm_free_and_destroy_model(C.byref(m))
    return alpha, rho, sv_index


# ---------------- the cases of the tests ----------------
HIK_KERNEL, LINEAR_KERNEL = (K.HIK, 0.0, 0.0, 0.0), (K.LINEAR, 0.0, 0.0, 0.0)
_case_cache = {}


def case_x(name):
    """int40: 40 x 10 integer rows; float55: 55 x 9; mem200: 200 x 12 (Q in memory); large: 1040 x 8 integer (the large solver)"""
    if name not in _case_cache:
        _case_cache[name] = {"int40": lambda: integer_rows(40, 0, 10, 1), "float55": lambda: float_rows(55, 0, 9, 8),
                             "mem200": lambda: float_rows(200, 0, 12, 9), "large": lambda: integer_rows(1040, 0, 8, 10)}[name]()
    return _case_cache[name]
