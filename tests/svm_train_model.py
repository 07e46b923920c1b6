"""numpy float64 restatement of libsvm's C-SVC training for a linear kernel, as the tracker uses it (libSvm/src/svm.cpp:
Solver::Solve :551-830, select_working_set :833-930, calculate_rho :1013-1049, SVC_Q; LibSvmUtils::extractSupportVectors
LibSvmUtils.cpp:105-118) -- and the seeded problem generator, the cases of the tests and a ctypes caller of the compiled
reference's svm_train.  A problem is n_pos positive rows followed by n_neg negative rows (LibSvmClassifier::createProblem), so
libsvm's class grouping is the identity.  No shrinking: there is no G_bar and no reconstruct_gradient.  Every operation is one
IEEE double operation in libsvm's order (Python floats), so that "the same model" means the same bits."""
import ctypes as C
import time

import numpy as np

TAU = 1e-12
last_train_seconds = 0.0
INF = float("inf")
LDS_BYTES = 160 * 1024   # one gfx950 workgroup


def labels(n_pos, n_neg):
    return np.concatenate([np.ones(n_pos), -np.ones(n_neg)])


def gram64(x):
    """Kernel::dot over dense svm_node lists: a float64 sum of the products (exact for float32 inputs) in index order"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, d = x.shape
    k = np.zeros((n, n))
    for c in range(d):   # one column at a time keeps libsvm's summation order for every pair
        k += np.outer(x[:, c], x[:, c])
    return k


def q_from_gram(k, n_pos):
    """SVC_Q::get_Q: Qfloat is float; QD stays double"""
    n = k.shape[0]
    y = labels(n_pos, n - n_pos)
    return (np.outer(y, y) * k).astype(np.float32), np.diag(k).copy()


def default_max_iterations(n):
    return max(10000000, 100 * n)


def padded(n):
    return (n + 15) // 16 * 16


def smo_lds_bytes(n, with_q):
    """dynamic LDS of the solver's workgroup: alpha, G and QD (double), the reduction slots, and Q when it fits"""
    n_pad = padded(n)
    return 3 * 8 * n_pad + 512 + (4 * n_pad * n_pad if with_q else 0)


def q_in_lds(n):
    return smo_lds_bytes(n, True) <= LDS_BYTES


def smo(q, qd, n_pos, c_pos=1.0, c_neg=1.0, eps=1e-4, max_iterations=0):
    """Solver::Solve without shrinking on a given Q (float32 n x n, rows as SVC_Q returns them) and QD (float64).
    Returns alpha, G, iterations, converged."""
    n = q.shape[0]
    if max_iterations <= 0:
        max_iterations = default_max_iterations(n)
    qf = np.asarray(q, np.float32).astype(np.float64)
    Q = [row.tolist() for row in qf]
    QD = [float(v) for v in qd]
    y = [1 if i < n_pos else -1 for i in range(n)]
    Cs = [float(c_pos) if i < n_pos else float(c_neg) for i in range(n)]
    alpha = [0.0] * n
    G = [-1.0] * n
    it = 0
    converged = 0
    while it < max_iterations:
        # select_working_set
        gmax, gmax2, i, j, obj_min = -INF, -INF, -1, -1, INF
        for t in range(n):
            if y[t] == 1:
                if alpha[t] < Cs[t] and -G[t] >= gmax:
                    gmax, i = -G[t], t
            elif alpha[t] > 0 and G[t] >= gmax:
                gmax, i = G[t], t
        if i >= 0:
            Qi = Q[i]
            for t in range(n):
                if y[t] == 1:
                    if alpha[t] > 0:
                        gd = gmax + G[t]
                        if G[t] >= gmax2:
                            gmax2 = G[t]
                        if gd > 0:
                            quad = QD[i] + QD[t] - 2.0 * y[i] * Qi[t]
                            od = -(gd * gd) / quad if quad > 0 else -(gd * gd) / TAU
                            if od <= obj_min:
                                j, obj_min = t, od
                elif alpha[t] < Cs[t]:
                    gd = gmax - G[t]
                    if -G[t] >= gmax2:
                        gmax2 = -G[t]
                    if gd > 0:
                        quad = QD[i] + QD[t] + 2.0 * y[i] * Qi[t]
                        od = -(gd * gd) / quad if quad > 0 else -(gd * gd) / TAU
                        if od <= obj_min:
                            j, obj_min = t, od
        if gmax + gmax2 < eps or i < 0 or j < 0:
            converged = 1
            break
        it += 1
        Qi, Qj = Q[i], Q[j]
        Ci, Cj = Cs[i], Cs[j]
        oi, oj = alpha[i], alpha[j]
        if y[i] != y[j]:
            quad = QD[i] + QD[j] + 2 * Qi[j]
            if quad <= 0:
                quad = TAU
            delta = (-G[i] - G[j]) / quad
            diff = alpha[i] - alpha[j]
            alpha[i] += delta
            alpha[j] += delta
            if diff > 0:
                if alpha[j] < 0:
                    alpha[j] = 0.0
                    alpha[i] = diff
            elif alpha[i] < 0:
                alpha[i] = 0.0
                alpha[j] = -diff
            if diff > Ci - Cj:
                if alpha[i] > Ci:
                    alpha[i] = Ci
                    alpha[j] = Ci - diff
            elif alpha[j] > Cj:
                alpha[j] = Cj
                alpha[i] = Cj + diff
        else:
            quad = QD[i] + QD[j] - 2 * Qi[j]
            if quad <= 0:
                quad = TAU
            delta = (G[i] - G[j]) / quad
            s = alpha[i] + alpha[j]
            alpha[i] -= delta
            alpha[j] += delta
            if s > Ci:
                if alpha[i] > Ci:
                    alpha[i] = Ci
                    alpha[j] = s - Ci
            elif alpha[j] < 0:
                alpha[j] = 0.0
                alpha[i] = s
            if s > Cj:
                if alpha[j] > Cj:
                    alpha[j] = Cj
                    alpha[i] = s - Cj
            elif alpha[i] < 0:
                alpha[i] = 0.0
                alpha[j] = s
        dai, daj = alpha[i] - oi, alpha[j] - oj
        for t in range(n):
            G[t] += Qi[t] * dai + Qj[t] * daj
    return np.array(alpha), np.array(G), it, converged


def finish(alpha, G, n_pos, c_pos=1.0, c_neg=1.0):
    """calculate_rho, the objective and the support-vector counts"""
    n = len(alpha)
    ub, lb, nfree, sfree = INF, -INF, 0, 0.0
    obj = 0.0
    nsv = nb = 0
    for i in range(n):
        yi = 1.0 if i < n_pos else -1.0
        Ci = c_pos if i < n_pos else c_neg
        a, g = float(alpha[i]), float(G[i])
        yg = yi * g
        if a >= Ci:
            if yi < 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        elif a <= 0:
            if yi > 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        else:
            nfree += 1
            sfree += yg
        obj += a * (g + -1.0)
        if a > 0:
            nsv += 1
            if a >= Ci:
                nb += 1
    rho = sfree / nfree if nfree > 0 else (ub + lb) / 2
    return rho, obj / 2, nsv, nb


def weights_f32(x, alpha, n_pos):
    """extractSupportVectors for CV_32F: values[k] += (float)(sv_coef_i * (double)x_ik) over the support vectors in index order"""
    x = np.asarray(x, np.float32)
    w = np.zeros(x.shape[1], np.float32)
    for i in range(x.shape[0]):
        a = float(alpha[i])
        if a > 0:
            coef = a if i < n_pos else -a
            w = w + (coef * x[i].astype(np.float64)).astype(np.float32)   # float32 + float32
    return w


def train(x, n_pos, C=1.0, weight_pos=1.0, weight_neg=1.0, eps=1e-4, max_iterations=0, q=None, qd=None):
    """the whole path; q / qd: a Gram the caller supplies (the device's) in place of the float64 one"""
    x = np.asarray(x, np.float32)
    if q is None:
        q, qd = q_from_gram(gram64(x), n_pos)
    cp, cn = C * weight_pos, C * weight_neg
    alpha, G, it, conv = smo(q, qd, n_pos, cp, cn, eps, max_iterations)
    rho, obj, nsv, nb = finish(alpha, G, n_pos, cp, cn)
    return dict(alpha=alpha, G=G, iterations=it, converged=conv, rho=rho, objective=obj, n_sv=nsv, n_bounded=nb,
                weights=weights_f32(x, alpha, n_pos))


# ---------------- problems ----------------
def ehog_like(n_pos, n_neg, d, seed):
    """ehog-like features: non-negative, each 13-channel block normalised to unit length and clipped at 0.48; the positives
    share a pattern so that the classes are separable only with some support vectors at the bound"""
    rng = np.random.default_rng(seed)
    n = n_pos + n_neg
    x = rng.random((n, d))
    pattern = rng.random(d)
    x[:n_pos] = 0.6 * x[:n_pos] + 0.4 * pattern
    for b in range(0, d, 13):
        blk = x[:, b:b + 13]
        blk /= np.sqrt((blk * blk).sum(axis=1, keepdims=True)) + 1e-9
    return np.minimum(x, 0.48).astype(np.float32)


def case_x(name):
    """(x, n_pos, n_neg) of the cases a..f"""
    if name == "a":
        return ehog_like(1, 1, 13, 11), 1, 1
    if name == "b":
        return ehog_like(5, 18, 117, 12), 5, 18
    if name == "c":   # b with rows 7 and 9 copies of row 1 (opposite class) and row 2 a copy of row 1: quad_coef = 0 -> TAU
        x = ehog_like(5, 18, 117, 12)
        x[7] = x[1]
        x[9] = x[1]
        x[2] = x[1]
        return x, 5, 18
    if name == "d":
        return ehog_like(20, 100, 455, 14), 20, 100
    if name == "e":
        return ehog_like(20, 180, 52, 15), 20, 180
    if name == "f":
        return ehog_like(30, 290, 39, 16), 30, 290
    raise KeyError(name)


def params_of(name):
    """the parameter sets a case runs with: (C, weight_pos, weight_neg)"""
    if name in ("b", "c"):
        return [(c, wp, wn) for c in (0.01, 1.0, 100.0) for (wp, wn) in ((1.0, 1.0), (18.0 / 5.0, 5.0 / 18.0))]
    return [(1.0, 1.0, 1.0)]


CASES = [(name, p) for name in "abcdef" for p in params_of(name)]
SMALL_CASES = [(name, p) for (name, p) in CASES if name in "abc"]   # n <= 24: recorded under tests/golden


def case_id(case):
    name, (c, wp, wn) = case
    return "%s-C%g-%s" % (name, c, "w" if wp != 1.0 else "u")


# ---------------- the compiled reference (oracle/_ref/libfdref.so exports libsvm's C interface) ----------------
class _Node(C.Structure):
    _fields_ = [("index", C.c_int), ("value", C.c_double)]


class _Problem(C.Structure):
    _fields_ = [("l", C.c_int), ("y", C.POINTER(C.c_double)), ("x", C.POINTER(C.POINTER(_Node)))]


class _Parameter(C.Structure):
    _fields_ = [("svm_type", C.c_int), ("kernel_type", C.c_int), ("degree", C.c_int), ("gamma", C.c_double), ("coef0", C.c_double),
                ("cache_size", C.c_double), ("eps", C.c_double), ("C", C.c_double), ("nr_weight", C.c_int),
                ("weight_label", C.POINTER(C.c_int)), ("weight", C.POINTER(C.c_double)), ("nu", C.c_double), ("p", C.c_double),
                ("shrinking", C.c_int), ("probability", C.c_int)]


class _Model(C.Structure):
    _fields_ = [("param", _Parameter), ("nr_class", C.c_int), ("l", C.c_int), ("SV", C.POINTER(C.POINTER(_Node))),
                ("sv_coef", C.POINTER(C.POINTER(C.c_double))), ("rho", C.POINTER(C.c_double)), ("probA", C.POINTER(C.c_double)),
                ("probB", C.POINTER(C.c_double)), ("sv_indices", C.POINTER(C.c_int)), ("label", C.POINTER(C.c_int)),
                ("nSV", C.POINTER(C.c_int)), ("free_sv", C.c_int)]


_PRINT = C.CFUNCTYPE(None, C.c_char_p)
_quiet = _PRINT(lambda s: None)


def libsvm_train(ref, x, n_pos, C_=1.0, weight_pos=1.0, weight_neg=1.0, eps=1e-4):
    """svm_train of the compiled reference with LibSvmClassifier's parameters (LibSvmClassifier.cpp:56-85: C_SVC, LINEAR,
    cache 100 MB, no shrinking, no probability; the class weights as weight_label / weight) on dense nodes.
    Returns alpha (n, from sv_coef / sv_indices), rho, the support-vector count."""
    x = np.asarray(x, np.float32)
    n, d = x.shape
    nodes = (_Node * ((d + 1) * n))()
    rows = (C.POINTER(_Node) * n)()
    for i in range(n):
        base = i * (d + 1)
        for k in range(d):
            nodes[base + k].index = k + 1
            nodes[base + k].value = float(x[i, k])
        nodes[base + d].index = -1
        rows[i] = C.cast(C.byref(nodes, base * C.sizeof(_Node)), C.POINTER(_Node))
    ys = (C.c_double * n)(*labels(n_pos, n - n_pos).tolist())
    prob = _Problem(n, ys, rows)
    wl = (C.c_int * 2)(1, -1)
    ww = (C.c_double * 2)(weight_pos, weight_neg)
    prm = _Parameter(svm_type=0, kernel_type=0, degree=0, gamma=0.0, coef0=0.0, cache_size=100.0, eps=eps, C=C_, nr_weight=2,
                     weight_label=wl, weight=ww, nu=0.0, p=0.0, shrinking=0, probability=0)
    ref.svm_set_print_string_function.argtypes = [_PRINT]
    ref.svm_set_print_string_function.restype = None
    ref.svm_set_print_string_function(_quiet)
    ref.svm_train.restype = C.POINTER(_Model)
    ref.svm_train.argtypes = [C.POINTER(_Problem), C.POINTER(_Parameter)]
    ref.svm_free_and_destroy_model.argtypes = [C.POINTER(C.POINTER(_Model))]
    ref.svm_free_and_destroy_model.restype = None
    global last_train_seconds
    t0 = time.perf_counter()
    m = ref.svm_train(C.byref(prob), C.byref(prm))
    last_train_seconds = time.perf_counter() - t0   # svm_train alone, without building the nodes (tools/svm_train_probe.py)
    mm = m.contents
    alpha = np.zeros(n)
    for s in range(mm.l):
        alpha[mm.sv_indices[s] - 1] = abs(mm.sv_coef[0][s])
    rho, nsv = float(mm.rho[0]), int(mm.l)
    ref.svm_free_and_destroy_model(C.byref(m))
    return alpha, rho, nsv
