"""numpy float64 restatement of libsvm's C-SVC training with a polynomial, RBF or histogram-intersection kernel (libSvm/src/
svm.cpp: Kernel::kernel_poly / kernel_rbf / kernel_hik :235-273, powi :26, SVC_Q, svm_train's two-class model;
LibSvmUtils::extractCoefficients), on top of tests/svm_train_model.py, whose solver (smo, finish) reads nothing of a problem but Q
and QD.  A kernel is a tuple (FD_KERNEL_*, p0, p1, p2) with the parameters of fd_svm_model: rbf gamma; poly alpha (libsvm's gamma),
constant (coef0), degree.  Every operation is one IEEE double operation in libsvm's order: dot sums the products in index order,
exp is libm's (math.exp, not numpy's), powi is restated, the histogram intersection is summed column by column."""
import ctypes as C
import math
import time

import numpy as np

import svm_train_model as M

LINEAR, POLY, RBF, HIK = 0, 1, 2, 3          # FD_KERNEL_*
LIBSVM_KERNEL_TYPE = {LINEAR: 0, POLY: 1, RBF: 2, HIK: 5}   # svm.h: LINEAR, POLY, RBF, SIGMOID, PRECOMPUTED, HIK

KERNELS = [(RBF, 0.5, 0.0, 0.0), (RBF, 8.0, 0.0, 0.0), (POLY, 0.25, 1.0, 2.0), (POLY, 0.05, 0.5, 3.0), (HIK, 0.0, 0.0, 0.0)]
last_train_seconds = 0.0


def kernel_id(kernel):
    kind, p0, p1, p2 = kernel
    return {LINEAR: "linear", POLY: "poly%g_%g_%d" % (p0, p1, p2), RBF: "rbf%g" % p0, HIK: "hik"}[kind]


def powi(base, times):
    """svm.cpp:26"""
    tmp, ret = base, 1.0
    t = times
    while t > 0:
        if t % 2 == 1:
            ret *= tmp
        tmp = tmp * tmp
        t //= 2
    return ret


def hik64(x, z=None):
    """kernel_hik: minSum += min<double>(x_k, z_k) over k in index order"""
    x = np.asarray(x, np.float32).astype(np.float64)
    z = x if z is None else np.asarray(z, np.float32).astype(np.float64)
    k = np.zeros((x.shape[0], z.shape[0]))
    for c in range(x.shape[1]):
        k += np.minimum.outer(x[:, c], z[:, c])
    return k


def dot64(x, z):
    """Kernel::dot between the rows of x and those of z, products summed in index order"""
    x = np.asarray(x, np.float32).astype(np.float64)
    z = np.asarray(z, np.float32).astype(np.float64)
    k = np.zeros((x.shape[0], z.shape[0]))
    for c in range(x.shape[1]):
        k += np.outer(x[:, c], z[:, c])
    return k


def _apply(kernel, dot, xs_rows, xs_cols):
    kind, p0, p1, p2 = kernel
    if kind == LINEAR:
        return dot
    out = np.empty_like(dot)
    if kind == POLY:
        degree = int(p2)
        for i in range(dot.shape[0]):
            out[i] = [powi(p0 * v + p1, degree) for v in dot[i].tolist()]
        return out
    assert kind == RBF
    for i in range(dot.shape[0]):
        xi = float(xs_rows[i])
        out[i] = [math.exp(-p0 * (xi + xj - 2 * v)) for v, xj in zip(dot[i].tolist(), xs_cols)]
    return out


def kernel64(x, kernel):
    """K (n x n, float64) as Kernel's kernel_function gives it; for rbf x_square is dot(x_i, x_i), the diagonal of the same sums"""
    if kernel[0] == HIK:
        return hik64(x)
    dot = M.gram64(x)
    xs = np.diag(dot).tolist()
    return _apply(kernel, dot, xs, xs)


def kernel64_between(sv, x, kernel):
    """K(sv_i, x_j) in float64, for decision values"""
    if kernel[0] == HIK:
        return hik64(sv, x)
    return _apply(kernel, dot64(sv, x), np.diag(dot64(sv, sv)).tolist() if kernel[0] == RBF else None,
                  np.diag(dot64(x, x)).tolist() if kernel[0] == RBF else None)


def train(x, n_pos, kernel, C=1.0, weight_pos=1.0, weight_neg=1.0, eps=1e-4, max_iterations=0, q=None, qd=None):
    """the whole path; q / qd: a Gram the caller supplies (the device's) in place of the float64 one.  The model is svm_train's:
    the examples with alpha > 0 in ascending index, coefficient (float)(alpha_i y_i)"""
    x = np.asarray(x, np.float32)
    if q is None:
        q, qd = M.q_from_gram(kernel64(x, kernel), n_pos)
    cp, cn = C * weight_pos, C * weight_neg
    alpha, G, it, conv = M.smo(q, qd, n_pos, cp, cn, eps, max_iterations)
    rho, obj, nsv, nb = M.finish(alpha, G, n_pos, cp, cn)
    sv_index = np.flatnonzero(alpha > 0).astype(np.int32)
    y = M.labels(n_pos, x.shape[0] - n_pos)
    return dict(alpha=alpha, G=G, iterations=it, converged=conv, rho=rho, objective=obj, n_sv=nsv, n_bounded=nb, sv_index=sv_index,
                coefficients=(alpha * y)[sv_index].astype(np.float32), support_vectors=x[sv_index])


def libsvm_train(ref, x, n_pos, kernel, C_=1.0, weight_pos=1.0, weight_neg=1.0, eps=1e-4):
    """svm_train of the compiled reference with LibSvmClassifier's parameters and the kernel's kernel_type, degree, gamma, coef0
    (LibSvmKernelParamSetter.hpp:36-51).  Returns alpha (n), rho, the model's sv_indices (0-based, in the model's order), its sv_coef and
    its labels."""
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
    ys = (C.c_double * n)(*M.labels(n_pos, n - n_pos).tolist())
    prob = M._Problem(n, ys, rows)
    wl = (C.c_int * 2)(1, -1)
    ww = (C.c_double * 2)(weight_pos, weight_neg)
    kind, p0, p1, p2 = kernel
    prm = M._Parameter(svm_type=0, kernel_type=LIBSVM_KERNEL_TYPE[kind], degree=int(p2) if kind == POLY else 0,
                       gamma=float(p0) if kind in (POLY, RBF) else 0.0, coef0=float(p1) if kind == POLY else 0.0, cache_size=100.0, eps=eps,
                       C=C_, nr_weight=2, weight_label=wl, weight=ww, nu=0.0, p=0.0, shrinking=0, probability=0)
    ref.svm_set_print_string_function.argtypes = [M._PRINT]
    ref.svm_set_print_string_function.restype = None
    ref.svm_set_print_string_function(M._quiet)
    ref.svm_train.restype = C.POINTER(M._Model)
    ref.svm_train.argtypes = [C.POINTER(M._Problem), C.POINTER(M._Parameter)]
    ref.svm_free_and_destroy_model.argtypes = [C.POINTER(C.POINTER(M._Model))]
    ref.svm_free_and_destroy_model.restype = None
    global last_train_seconds
    t0 = time.perf_counter()
    m = ref.svm_train(C.byref(prob), C.byref(prm))
    last_train_seconds = time.perf_counter() - t0   # svm_train alone, without building the nodes (tools/svm_kernel_train_probe.py)
    mm = m.contents
    alpha = np.zeros(n)
    sv_index = np.array([mm.sv_indices[s] - 1 for s in range(mm.l)], np.int32)
    sv_coef = np.array([mm.sv_coef[0][s] for s in range(mm.l)], np.float64)
    alpha[sv_index] = np.abs(sv_coef)
    rho, label = float(mm.rho[0]), (int(mm.label[0]), int(mm.label[1]))
    ref.svm_free_and_destroy_model(C.byref(m))
    return alpha, rho, sv_index, sv_coef, label
