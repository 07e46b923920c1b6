"""One-class SVM training on the device (fd_one_class_svm_gram / _train / _train_model) against tests/svm_one_class_model.py, the
float64 restatement that tests/test_svm_prob_model.py pins to libsvm itself.

The shapes are the smallest at which the kernels can still go wrong (svm_one_class_model.case_x):
  int40    40 x 10 integer rows   Q in LDS; with the histogram-intersection and the linear kernel Q is libsvm's own bits
  float55  55 x 9                 n and d no multiples of 16 or 4
  mem200   200 x 12               Q from memory
  large    1040 x 8 integer       the large solver, more than one block of the start-state kernel
nu on the first two: nu n < 1, fractional, integral, and 1 (every alpha at its bound, rho = inf)."""
import ctypes as C
import os

import numpy as np
import pytest

import svm_kernel_train_model as K
import svm_one_class_model as OC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-4
KERNELS = K.KERNELS + [OC.LINEAR_KERNEL]
CASES = [(name, kernel, nu) for name in ("int40", "float55") for kernel in KERNELS for nu in OC.NUS] + \
        [("mem200", kernel, 0.26) for kernel in KERNELS] + [("large", OC.HIK_KERNEL, 0.1)]
_cache = {}


def _id(v):
    return v if isinstance(v, str) else (K.kernel_id(v) if isinstance(v, tuple) else "nu%g" % v)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _gram(capi, ctx, name, kernel, nu):
    key = ("q", name, kernel, nu)
    if key not in _cache:
        _cache[key] = capi.one_class_svm_gram(ctx, OC.case_x(name), kernel, nu)
    return _cache[key]


def _model(capi, ctx, name, kernel, nu):
    """the float64 model on the device's Q"""
    key = ("m", name, kernel, nu)
    if key not in _cache:
        q, qd, _ = _gram(capi, ctx, name, kernel, nu)
        _cache[key] = OC.train(OC.case_x(name), kernel, nu, EPS, q=q, qd=qd)
    return _cache[key]


def _assert_same_bits(got, want, x):
    sv_index, coef, sv, bias, alpha, info = got
    assert _bits(alpha) == _bits(want["alpha"]), "alpha: max |d| = %g" % np.abs(alpha - want["alpha"]).max()
    assert info["iterations"] == want["iterations"] and info["converged"] == want["converged"]
    assert _bits(np.float64(info["rho"])) == _bits(np.float64(want["rho"])), (info["rho"], want["rho"])
    assert _bits(np.float64(info["objective"])) == _bits(np.float64(want["objective"])), (info["objective"], want["objective"])
    assert (info["n_sv"], info["n_bounded"]) == (want["n_sv"], want["n_bounded"])
    assert sv_index.dtype == np.int32 and np.array_equal(sv_index, want["sv_index"])
    assert coef.dtype == np.float32 and _bits(coef) == _bits(want["coefficients"])
    assert sv.dtype == np.float32 and _bits(sv) == _bits(x[sv_index])
    assert _bits(np.float32(bias)) == _bits(np.float32(want["rho"]))


@pytest.mark.parametrize("name,kernel,nu", CASES, ids=_id)
def test_gram_and_start_gradient(capi, ctx, name, kernel, nu):
    """Q and QD are fd_kernel_svm_gram's for a problem of positives; G0 is the model's start gradient on this Q, bit for bit"""
    x = OC.case_x(name)
    q, qd, g0 = _gram(capi, ctx, name, kernel, nu)
    if ("kq", name, kernel) not in _cache:
        _cache[("kq", name, kernel)] = capi.kernel_svm_gram(ctx, np.concatenate([x, x[:1]]), len(x), kernel)
    kq, kqd = _cache[("kq", name, kernel)]
    assert _bits(q) == _bits(kq[:-1, :-1]) and _bits(qd) == _bits(kqd[:-1])
    assert _bits(g0) == _bits(OC.start_gradient(q, OC.start_alpha(len(x), nu)))
    if name == "int40" and kernel[0] in (K.HIK, K.LINEAR):
        want_q, want_qd = OC.q_one_class(K.kernel64(x, kernel))
        assert _bits(q) == _bits(want_q) and _bits(qd) == _bits(want_qd)


@pytest.mark.parametrize("name,kernel,nu", CASES, ids=_id)
def test_train_equals_model_on_device_q(capi, ctx, name, kernel, nu):
    x = OC.case_x(name)
    want = _model(capi, ctx, name, kernel, nu)
    got = capi.one_class_svm_train(ctx, x, kernel, nu=nu, eps=EPS)
    _assert_same_bits(got, want, x)
    alpha, info, n = got[4], got[5], len(x)
    assert want["converged"] == 1 and info["launches"] == 1
    # model-independent: the equality constraint, the nu-property, the box
    assert abs(alpha.sum() - nu * n) <= 1e-12 * nu * n
    assert info["n_sv"] >= nu * n - 1e-9 and (alpha == 1.0).sum() <= nu * n + 1e-9
    assert (alpha >= 0.0).all() and (alpha <= 1.0).all()
    assert np.isinf(info["rho"]) == (nu == 1.0)
    if nu == 1.0:
        assert info["rho"] == np.inf and info["iterations"] == 0 and (alpha == 1.0).all()


@pytest.mark.parametrize("nu", OC.NUS)
@pytest.mark.parametrize("kernel", [OC.HIK_KERNEL, OC.LINEAR_KERNEL], ids=K.kernel_id)
def test_integer_rows_give_libsvm_bits(capi, ctx, kernel, nu):
    g = np.load(os.path.join(GOLDEN, "svm_one_class_int40.npz"))
    x = OC.case_x("int40")
    assert float(g["xsum"]) == float(x.astype(np.float64).sum())
    ki, ni = KERNELS.index(kernel), OC.NUS.index(nu)
    assert tuple(g["kernels"][ki]) == kernel and g["nus"][ni] == nu
    _, _, _, _, alpha, info = capi.one_class_svm_train(ctx, x, kernel, nu=nu, eps=float(g["eps"]))
    assert _bits(alpha) == _bits(g["alpha"][ki, ni]) and _bits(np.float64(info["rho"])) == _bits(g["rho"][ki, ni])


@pytest.mark.parametrize("name,kernel,nu", [("int40", OC.HIK_KERNEL, 0.26), ("float55", K.KERNELS[0], 0.5), ("mem200", K.KERNELS[2], 0.26),
                                            ("large", OC.HIK_KERNEL, 0.1)], ids=_id)
def test_relaunches_give_the_bits_of_one_launch(capi, ctx, name, kernel, nu):
    x = OC.case_x(name)
    want = _model(capi, ctx, name, kernel, nu)
    got = capi.one_class_svm_train(ctx, x, kernel, nu=nu, eps=EPS, launch_iterations=7)
    _assert_same_bits(got, want, x)
    assert got[5]["launches"] == want["iterations"] // 7 + 1 and want["iterations"] > 7


def test_max_iterations_returns_the_current_model(capi, ctx):
    x, kernel, nu = OC.case_x("float55"), K.KERNELS[0], 0.26
    q, qd, _ = _gram(capi, ctx, "float55", kernel, nu)
    want = OC.train(x, kernel, nu, EPS, 5, q=q, qd=qd)
    got = capi.one_class_svm_train(ctx, x, kernel, nu=nu, eps=EPS, max_iterations=5)
    assert want["converged"] == 0 and want["iterations"] == 5
    _assert_same_bits(got, want, x)


@pytest.mark.parametrize("name,kernel,nu", [("int40", OC.HIK_KERNEL, 0.26), ("float55", K.KERNELS[0], 0.5), ("float55", K.KERNELS[3], 0.02),
                                            ("mem200", OC.LINEAR_KERNEL, 0.26)], ids=_id)
def test_train_model_scores_the_training_rows(capi, ctx, name, kernel, nu):
    """fd_svm_distance_batch of the created f32 model against sum alpha K64 - rho, within DESIGN.md 4.10's bound"""
    x = OC.case_x(name)
    want = _model(capi, ctx, name, kernel, nu)
    svm, info = capi.one_class_svm_train_model(ctx, x, kernel, nu=nu, eps=EPS)
    assert info["n_sv"] == want["n_sv"] and _bits(np.float64(info["rho"])) == _bits(np.float64(want["rho"]))
    k = K.kernel64_between(x[want["sv_index"]], x, kernel)
    ref = want["alpha"][want["sv_index"]] @ k - want["rho"]
    got = svm.distance(x)
    bound = 1e-4 * max(1.0, np.abs(want["alpha"]).sum() * np.abs(k).max())
    print("one-class %s %s: max |d| = %g, bound %g" % (name, K.kernel_id(kernel), np.abs(got - ref).max(), bound))
    assert np.abs(got - ref).max() <= bound


def test_nu_one_is_infinite_rho_and_no_model(capi, ctx):
    x = OC.case_x("int40")
    _, _, _, bias, alpha, info = capi.one_class_svm_train(ctx, x, OC.HIK_KERNEL, nu=1.0)
    assert info["rho"] == np.inf and bias == np.inf and (alpha == 1.0).all() and info["n_sv"] == info["n_bounded"] == 40
    with pytest.raises(capi.FdError) as e:
        capi.one_class_svm_train_model(ctx, x, OC.HIK_KERNEL, nu=1.0)
    assert e.value.code == capi.FD_ERR_RUNTIME and "rho" in str(e.value)


def test_single_example(capi, ctx):
    x = OC.case_x("int40")[:1]
    for nu in (0.3, 1.0):
        q, qd, _ = capi.one_class_svm_gram(ctx, x, OC.HIK_KERNEL, nu)
        _assert_same_bits(capi.one_class_svm_train(ctx, x, OC.HIK_KERNEL, nu=nu), OC.train(x, OC.HIK_KERNEL, nu, EPS, q=q, qd=qd), x)


def test_device_input(capi, ctx):
    import torch
    for name, kernel, nu in (("float55", K.KERNELS[0], 0.26), ("large", OC.HIK_KERNEL, 0.1)):
        x = OC.case_x(name)
        xd = torch.from_numpy(x).cuda()
        _assert_same_bits(capi.one_class_svm_train(ctx, xd, kernel, nu=nu, eps=EPS), _model(capi, ctx, name, kernel, nu), x)
        q, qd, g0 = capi.one_class_svm_gram(ctx, xd, kernel, nu)
        assert all(_bits(a) == _bits(b) for a, b in zip((q, qd, g0), _gram(capi, ctx, name, kernel, nu)))


def test_two_calls_give_the_same_bits_and_c_svc_is_unchanged_between(capi, ctx):
    """the one-class start state does not leak into a C-SVC run on the same scratch"""
    x = OC.case_x("float55")
    a = capi.one_class_svm_train(ctx, x, K.KERNELS[0], nu=0.26)
    c1 = capi.kernel_svm_train(ctx, x, 15, K.KERNELS[0])
    b = capi.one_class_svm_train(ctx, x, K.KERNELS[0], nu=0.26)
    c2 = capi.kernel_svm_train(ctx, x, 15, K.KERNELS[0])
    assert _bits(a[4]) == _bits(b[4]) and a[5] == b[5]
    assert _bits(c1[4]) == _bits(c2[4]) and c1[5] == c2[5]
    q, qd = capi.kernel_svm_gram(ctx, x, 15, K.KERNELS[0])
    want = K.train(x, 15, K.KERNELS[0], eps=EPS, q=q, qd=qd)
    assert _bits(c1[4]) == _bits(want["alpha"]) and _bits(np.float64(c1[5]["objective"])) == _bits(np.float64(want["objective"]))


@pytest.mark.parametrize("nu", [0.0, -0.5, 1.0000001, float("nan"), float("inf")])
def test_invalid_nu(capi, ctx, nu):
    x = OC.case_x("int40")
    for call in (lambda: capi.one_class_svm_train(ctx, x, OC.HIK_KERNEL, nu=nu), lambda: capi.one_class_svm_train_model(ctx, x, OC.HIK_KERNEL, nu=nu),
                 lambda: capi.one_class_svm_gram(ctx, x, OC.HIK_KERNEL, nu)):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "nu" in str(e.value)


def test_invalid_arguments(capi, ctx):
    x = OC.case_x("int40")
    L = capi.lib()
    k, prm, info, bias = capi.svm_kernel(K.HIK), capi.svm_one_class_params(nu=0.5), capi.fd_svm_train_info(), C.c_float()
    svi, coef, q, qd = np.zeros(40, np.int32), np.zeros(40, np.float32), np.zeros((40, 40), np.float32), np.zeros(40)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    train = lambda xp, n, d, kk, pp, s, c, b, i: L.fd_one_class_svm_train(ctx.h, xp, n, d, 0, kk, pp, s, c, None, b, None, i)
    ok = (p(x), 40, 10, C.byref(k), C.byref(prm), p(svi), p(coef), C.byref(bias), C.byref(info))
    assert train(*ok) == capi.FD_OK
    for pos in (0, 3, 4, 5, 6, 7, 8):   # each required pointer
        args = list(ok)
        args[pos] = None
        assert train(*args) == capi.FD_ERR_INVALID_ARGUMENT, pos
    for n, d in ((0, 10), (-3, 10), (40, 0), (16385, 10)):
        assert train(p(x), n, d, *ok[3:]) == capi.FD_ERR_INVALID_ARGUMENT
    for bad in (capi.svm_one_class_params(nu=0.5, eps=-1.0), capi.svm_one_class_params(nu=0.5, max_iterations=-1),
                capi.svm_one_class_params(nu=0.5, launch_iterations=-1)):
        assert train(*ok[:4], C.byref(bad), *ok[5:]) == capi.FD_ERR_INVALID_ARGUMENT
    for badk in (capi.svm_kernel(7), capi.svm_kernel(K.RBF, -1.0), capi.svm_kernel(K.POLY, 0.5, 0.0, 1.5)):
        assert train(*ok[:3], C.byref(badk), *ok[4:]) == capi.FD_ERR_INVALID_ARGUMENT
    assert L.fd_one_class_svm_gram(ctx.h, p(x), 40, 10, 0, C.byref(k), 0.5, p(q), p(qd), None) == capi.FD_OK   # G0 is optional
    assert L.fd_one_class_svm_gram(ctx.h, p(x), 40, 10, 0, C.byref(k), 0.5, None, p(qd), None) == capi.FD_ERR_INVALID_ARGUMENT
    assert L.fd_one_class_svm_gram(ctx.h, None, 40, 10, 0, C.byref(k), 0.5, p(q), p(qd), None) == capi.FD_ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert L.fd_one_class_svm_train_model(ctx.h, p(x), 40, 10, 0, C.byref(k), C.byref(prm), 0.0, 1.0, 0.0, None, C.byref(info)) == \
        capi.FD_ERR_INVALID_ARGUMENT
    assert L.fd_one_class_svm_train_model(ctx.h, p(x), 0, 10, 0, C.byref(k), C.byref(prm), 0.0, 1.0, 0.0, C.byref(h), C.byref(info)) == \
        capi.FD_ERR_INVALID_ARGUMENT and not h.value
