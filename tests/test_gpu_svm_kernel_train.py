"""Kernel C-SVC training on the device (fd_kernel_svm_gram / _train / _train_model / _train_batch) against
tests/svm_kernel_train_model.py, the float64 restatement that tests/test_svm_kernel_train_model.py pins to libsvm itself.

The shapes are the smallest at which the kernels can still go wrong (svm_train_model.case_x):
  a      1 + 1 x 13      one iteration
  b      5 + 18 x 117    n and d no multiples of 16 or 4; d spans two LDS chunks of the histogram-intersection Gram
  c      b with duplicated rows of either class (quad_coef = 0 -> TAU)
  e      20 + 180 x 52   Q from memory
  large  40 + 1000 x 20  n = 1040: the large solver, Q in the training scratch
"""
import ctypes as C
import os

import numpy as np
import pytest

import svm_kernel_train_model as K
import svm_train_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-4
LINEAR = (K.LINEAR, 0.0, 0.0, 0.0)
HIK = (K.HIK, 0.0, 0.0, 0.0)
RBF = K.KERNELS[0]
SMALL = list("abce")
_cache = {}


def _case_x(name):
    if name == "large":
        return M.ehog_like(40, 1000, 20, 21), 40, 1000
    return M.case_x(name)


def _params(name):
    """weighted and unweighted, C = 0.01, 1, 100; the weights are compensateImbalance's"""
    _, n_pos, n_neg = _problem(name)
    return [(c, wp, wn) for c in (0.01, 1.0, 100.0) for (wp, wn) in ((1.0, 1.0), (n_neg / n_pos, n_pos / n_neg))]


def _problem(name):
    if ("x", name) not in _cache:
        _cache[("x", name)] = _case_x(name)
    return _cache[("x", name)]


def _k64(name, kernel):
    if ("k", name, kernel) not in _cache:
        _cache[("k", name, kernel)] = K.kernel64(_problem(name)[0], kernel)
    return _cache[("k", name, kernel)]


def _device_gram(capi, ctx, name, kernel):
    if ("q", name, kernel) not in _cache:
        x, n_pos, _ = _problem(name)
        _cache[("q", name, kernel)] = capi.kernel_svm_gram(ctx, x, n_pos, kernel)
    return _cache[("q", name, kernel)]


def _model_on_device_q(capi, ctx, name, kernel, prm, max_iterations=0):
    key = ("m", name, kernel, prm, max_iterations)
    if key not in _cache:
        x, n_pos, _ = _problem(name)
        q, qd = _device_gram(capi, ctx, name, kernel)
        _cache[key] = K.train(x, n_pos, kernel, prm[0], prm[1], prm[2], EPS, max_iterations, q=q, qd=qd)
    return _cache[key]


def _device_train(capi, ctx, name, kernel, prm, **kw):
    x, n_pos, _ = _problem(name)
    return capi.kernel_svm_train(ctx, x, n_pos, kernel, C=prm[0], weight_pos=prm[1], weight_neg=prm[2], **kw)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


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


def _ulps32(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ---------------- Gram ----------------
GRAM_CASES = [(name, kernel) for name in SMALL for kernel in K.KERNELS + [LINEAR]] + [("large", RBF), ("large", HIK)]


@pytest.mark.parametrize("name,kernel", GRAM_CASES, ids=lambda v: v if isinstance(v, str) else K.kernel_id(v))
def test_gram(capi, ctx, name, kernel):
    """hik: libsvm's own bits (minimum exact, the sum in libsvm's order).  rbf: QD = 1 exactly, Q within one float ulp.  poly and
    linear: Q within one float ulp, QD within 4 d max(1, degree) double ulp (a reordered f64 sum of non-negative exact products,
    then powi).  Q is symmetric."""
    x, n_pos, n_neg = _problem(name)
    q, qd = _device_gram(capi, ctx, name, kernel)
    want_q, want_qd = M.q_from_gram(_k64(name, kernel), n_pos)
    dq = _ulps32(q, want_q)
    dqd = np.abs(qd - want_qd) / np.spacing(want_qd)
    print("gram %s %s: max |dQ| / ulp = %g, max |dQD| / ulp = %g" % (name, K.kernel_id(kernel), dq.max(), dqd.max()))
    assert q.shape == (n_pos + n_neg,) * 2 and np.array_equal(q, q.T)
    if kernel[0] == K.HIK:
        assert _bits(q) == _bits(want_q) and _bits(qd) == _bits(want_qd)
    elif kernel[0] == K.RBF:
        assert (qd == 1.0).all() and (dq <= 1.0).all()
    else:
        assert (dq <= 1.0).all()
        assert (dqd <= 4 * x.shape[1] * max(1, int(kernel[3]))).all()


# ---------------- solver: the model's bits ----------------
@pytest.mark.parametrize("kernel", K.KERNELS, ids=K.kernel_id)
@pytest.mark.parametrize("pi", range(6), ids=["C0.01-u", "C0.01-w", "C1-u", "C1-w", "C100-u", "C100-w"])
@pytest.mark.parametrize("name", SMALL)
def test_solver_equals_model_bit_for_bit(capi, ctx, name, pi, kernel):
    prm = _params(name)[pi]
    want = _model_on_device_q(capi, ctx, name, kernel, prm)
    got = _device_train(capi, ctx, name, kernel, prm)
    assert want["converged"] == 1 and got[5]["launches"] == want["iterations"] // 16384 + 1   # the default budget of a launch
    _assert_same_bits(got, want, _problem(name)[0])


@pytest.mark.parametrize("kernel", [RBF, HIK], ids=K.kernel_id)
def test_large_solver_equals_model_bit_for_bit(capi, ctx, kernel):
    assert capi.kernel_svm_train_limits(40, 1000, 20)[1]
    prm = (1.0, 1.0, 1.0)
    want = _model_on_device_q(capi, ctx, "large", kernel, prm)
    got = _device_train(capi, ctx, "large", kernel, prm)
    assert want["converged"] == 1
    _assert_same_bits(got, want, _problem("large")[0])


@pytest.mark.parametrize("name", ["b", "e"])
def test_linear_kernel_equals_the_weight_vector_trainer(capi, ctx, name):
    x, n_pos, n_neg = _problem(name)
    for prm in _params(name)[2:4]:
        w, bias, alpha, info = capi.linear_svm_train(ctx, x, n_pos, C=prm[0], weight_pos=prm[1], weight_neg=prm[2])
        sv_index, coef, sv, kbias, kalpha, kinfo = _device_train(capi, ctx, name, LINEAR, prm)
        assert _bits(kalpha) == _bits(alpha) and kinfo == info and _bits(np.float32(kbias)) == _bits(np.float32(bias))
        assert np.array_equal(sv_index, np.flatnonzero(alpha > 0))
    q, qd = capi.linear_svm_gram(ctx, x, n_pos)
    kq, kqd = _device_gram(capi, ctx, name, LINEAR)
    assert _bits(q) == _bits(kq) and _bits(qd) == _bits(kqd)


@pytest.mark.parametrize("name", list("abc"))
def test_hik_equals_recorded_libsvm(capi, ctx, name):
    """Q is libsvm's own for this kernel, so no device Gram stands between the device's alpha and libsvm's"""
    g = np.load(os.path.join(GOLDEN, "svm_kernel_train_%s.npz" % name))
    ki = K.KERNELS.index(HIK)
    for pi, prm in enumerate(M.params_of(name)):
        sv_index, coef, sv, bias, alpha, info = _device_train(capi, ctx, name, HIK, prm)
        c = prm[0] * max(prm[1], prm[2])
        print("hik %s %r: max |alpha - libsvm| = %g, |rho - libsvm| = %g" % (name, prm, np.abs(alpha - g["alpha"][ki, pi]).max(),
                                                                            abs(info["rho"] - g["rho"][ki, pi])))
        assert np.abs(alpha - g["alpha"][ki, pi]).max() <= 1e-12 * c
        assert abs(info["rho"] - g["rho"][ki, pi]) <= 1e-12 and info["n_sv"] == g["n_sv"][ki, pi]
        assert np.array_equal(sv_index, g["sv_index"][ki, pi, :info["n_sv"]])


# ---------------- independent of the model ----------------
@pytest.mark.parametrize("kernel", K.KERNELS, ids=K.kernel_id)
@pytest.mark.parametrize("name", SMALL)
def test_solution_is_optimal(capi, ctx, name, kernel):
    """With G recomputed in float64 from the returned alpha and the float64 K: m(alpha) - M(alpha) < eps + s, rho between -m and -M
    up to s (s = n C_max 2^-24 max|K|, the effect of rounding Q to float), the box and the equality constraint"""
    x, n_pos, n_neg = _problem(name)
    n = n_pos + n_neg
    y = M.labels(n_pos, n_neg)
    k = _k64(name, kernel)
    for prm in _params(name):
        Cs = np.where(y > 0, prm[0] * prm[1], prm[0] * prm[2])
        sv_index, coef, sv, bias, alpha, info = _device_train(capi, ctx, name, kernel, prm)
        assert (alpha >= 0).all() and (alpha <= Cs).all() and abs(float(alpha @ y)) <= 1e-12 * Cs.max() * n
        G = (np.outer(y, y) * k) @ alpha - 1.0
        up = ((y > 0) & (alpha < Cs)) | ((y < 0) & (alpha > 0))
        low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < Cs))
        m, Mm = (-y * G)[up].max(), (-y * G)[low].min()
        s = n * Cs.max() * 2.0 ** -24 * np.abs(k).max()
        print("%s %s %r: m - M = %g, eps + s = %g, rho = %r in [%r, %r]" % (name, K.kernel_id(kernel), prm, m - Mm, EPS + s, info["rho"], -m, -Mm))
        assert m - Mm < EPS + s
        assert min(-m, -Mm) - s <= info["rho"] <= max(-m, -Mm) + s


# ---------------- closure with the scorer ----------------
@pytest.mark.parametrize("kernel", K.KERNELS, ids=K.kernel_id)
@pytest.mark.parametrize("name", SMALL)
def test_trained_model_scores_its_examples(capi, ctx, name, kernel):
    """kernel_svm_train_model(...).distance(x) against sum coef_f32 K64 - rho in float64, within the project's 1e-4 for SVM distances
    scaled by what multiplies a kernel value's f32 error; beyond that tolerance the sign is that of y_i (G_i + 1) - rho"""
    x, n_pos, n_neg = _problem(name)
    y = M.labels(n_pos, n_neg)
    k = _k64(name, kernel)
    for prm in (_params(name)[2], _params(name)[5]):
        sv_index, coef, sv, bias, alpha, info = _device_train(capi, ctx, name, kernel, prm)
        svm, minfo = capi.kernel_svm_train_model(ctx, x, n_pos, kernel, C=prm[0], weight_pos=prm[1], weight_neg=prm[2])
        assert minfo == info
        got = svm.distance(x)
        svm.close()
        want = coef.astype(np.float64) @ K.kernel64_between(sv, x, kernel) - info["rho"]
        tol = 1e-4 * max(1.0, float(np.abs(coef.astype(np.float64)).sum()) * float(np.abs(k).max()))
        print("%s %s %r: max |distance - float64| = %g, tolerance %g" % (name, K.kernel_id(kernel), prm, np.abs(got - want).max(), tol))
        assert np.abs(got - want).max() <= tol
        G = (np.outer(y, y) * k) @ alpha - 1.0
        value = y * (G + 1.0) - info["rho"]
        sure = np.abs(value) > tol
        assert (np.sign(got[sure]) == np.sign(value[sure])).all()


# ---------------- relaunch, iteration limit ----------------
@pytest.mark.parametrize("name,kernel", [("b", RBF), ("c", K.KERNELS[3]), ("e", HIK), ("large", RBF)], ids=lambda v: v if isinstance(v, str) else K.kernel_id(v))
def test_relaunch_gives_the_same_bits(capi, ctx, name, kernel):
    prm = (1.0, 1.0, 1.0)
    want = _model_on_device_q(capi, ctx, name, kernel, prm)
    got = _device_train(capi, ctx, name, kernel, prm, launch_iterations=7)
    assert got[5]["launches"] == want["iterations"] // 7 + 1 > 1
    _assert_same_bits(got, want, _problem(name)[0])


@pytest.mark.parametrize("kernel", [RBF, HIK], ids=K.kernel_id)
def test_max_iterations_is_not_an_error(capi, ctx, kernel):
    prm = (1.0, 1.0, 1.0)
    want = _model_on_device_q(capi, ctx, "e", kernel, prm, max_iterations=3)
    assert want["iterations"] == 3 and want["converged"] == 0
    got = _device_train(capi, ctx, "e", kernel, prm, max_iterations=3)   # FD_OK: no FdError
    _assert_same_bits(got, want, _problem("e")[0])


# ---------------- batch, device input ----------------
@pytest.mark.parametrize("kernel", [RBF, K.KERNELS[2], HIK], ids=K.kernel_id)
def test_batch_equals_single_calls(capi, ctx, kernel):
    prm = (1.0, 1.0, 1.0)
    got = capi.kernel_svm_train_batch(ctx, [(_problem(name)[0], _problem(name)[1]) for name in SMALL], kernel)
    assert len(got) == len(SMALL)
    for name, g in zip(SMALL, got):
        _assert_same_bits(g, _model_on_device_q(capi, ctx, name, kernel, prm), _problem(name)[0])
    # with relaunches: every problem keeps its state until the last one is done
    got = capi.kernel_svm_train_batch(ctx, [(_problem(name)[0], _problem(name)[1]) for name in "ecb"], kernel, launch_iterations=16)
    for name, g in zip("ecb", got):
        _assert_same_bits(g, _model_on_device_q(capi, ctx, name, kernel, prm), _problem(name)[0])


@pytest.mark.parametrize("name,kernel", [("b", RBF), ("e", HIK), ("large", HIK)], ids=lambda v: v if isinstance(v, str) else K.kernel_id(v))
def test_device_input_equals_host_input(capi, ctx, name, kernel):
    import torch
    x, n_pos, _ = _problem(name)
    dev = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    host = _device_train(capi, ctx, name, kernel, (1.0, 1.0, 1.0))
    got = capi.kernel_svm_train(ctx, dev, n_pos, kernel)
    for a, b in zip(got[:3] + got[4:5], host[:3] + host[4:5]):
        assert _bits(a) == _bits(b)
    assert got[3] == host[3] and got[5] == host[5]
    q, qd = capi.kernel_svm_gram(ctx, dev, n_pos, kernel)
    hq, hqd = _device_gram(capi, ctx, name, kernel)
    assert _bits(q) == _bits(hq) and _bits(qd) == _bits(hqd)
    assert torch.equal(dev.cpu(), torch.from_numpy(x))   # the input is only read


# ---------------- argument errors ----------------
@pytest.mark.parametrize("n_pos,n_rows,kernel,kw", [
    (0, 6, RBF, {}), (6, 6, RBF, {}), (3, 16390, HIK, {}),
    (3, 6, (7, 0.0, 0.0, 0.0), {}), (3, 6, (-1, 0.0, 0.0, 0.0), {}),
    (3, 6, (K.RBF, -0.5, 0.0, 0.0), {}), (3, 6, (K.RBF, float("nan"), 0.0, 0.0), {}), (3, 6, (K.POLY, -0.25, 1.0, 2.0), {}),
    (3, 6, (K.POLY, 0.25, 1.0, -1.0), {}), (3, 6, (K.POLY, 0.25, 1.0, 2.5), {}),
    (3, 6, RBF, {"C": 0.0}), (3, 6, RBF, {"weight_pos": 0.0}), (3, 6, HIK, {"weight_neg": -2.0}), (3, 6, HIK, {"eps": -1e-3}),
    (3, 6, RBF, {"max_iterations": -1}), (3, 6, RBF, {"launch_iterations": -1}), (3, 6, HIK, {"C": float("nan")})])
def test_invalid_arguments(capi, ctx, n_pos, n_rows, kernel, kw):
    x = np.ones((n_rows, 2), np.float32)
    with pytest.raises(capi.FdError) as e:
        capi.kernel_svm_train(ctx, x, n_pos, kernel, **kw)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and len(str(e.value)) > len("fd_hip error 1: ")
    with pytest.raises(capi.FdError) as e:
        capi.kernel_svm_train_model(ctx, x, n_pos, kernel, **kw)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    if not kw:
        with pytest.raises(capi.FdError) as e:
            capi.kernel_svm_gram(ctx, x, n_pos, kernel)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    if n_rows <= 1024 or kw:
        with pytest.raises(capi.FdError) as e:
            capi.kernel_svm_train_batch(ctx, [(np.ones((4, 2), np.float32), 2), (x, n_pos)], kernel, **kw)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_the_batch_keeps_its_limit_of_1024(capi, ctx):
    x = np.ones((1030, 2), np.float32)
    with pytest.raises(capi.FdError) as e:
        capi.kernel_svm_train_batch(ctx, [(x, 3)], HIK)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_null_pointers(capi, ctx):
    L = capi.lib()
    x = np.ones((6, 5), np.float32) + np.arange(6, dtype=np.float32)[:, None]
    svi, coef, sv, q, qd = np.zeros(6, np.int32), np.zeros(6, np.float32), np.zeros((6, 5), np.float32), np.zeros((6, 6), np.float32), np.zeros(6)
    bias, info, prm, kern, h = C.c_float(), capi.fd_svm_train_info(), capi.svm_train_params(), capi.svm_kernel(*RBF), C.c_void_p()
    P, R = capi._ptr, C.byref
    train = L.fd_kernel_svm_train
    calls = [lambda: train(ctx.h, None, 3, 3, 5, 0, R(kern), R(prm), P(svi), P(coef), P(sv), R(bias), None, R(info)),
             lambda: train(ctx.h, P(x), 3, 3, 5, 0, None, R(prm), P(svi), P(coef), P(sv), R(bias), None, R(info)),
             lambda: train(ctx.h, P(x), 3, 3, 5, 0, R(kern), None, P(svi), P(coef), P(sv), R(bias), None, R(info)),
             lambda: train(ctx.h, P(x), 3, 3, 5, 0, R(kern), R(prm), None, P(coef), P(sv), R(bias), None, R(info)),
             lambda: train(ctx.h, P(x), 3, 3, 5, 0, R(kern), R(prm), P(svi), None, P(sv), R(bias), None, R(info)),
             lambda: train(ctx.h, P(x), 3, 3, 5, 0, R(kern), R(prm), P(svi), P(coef), P(sv), None, None, R(info)),
             lambda: train(ctx.h, P(x), 3, 3, 5, 0, R(kern), R(prm), P(svi), P(coef), P(sv), R(bias), None, None),
             lambda: train(ctx.h, P(x), 3, 3, 0, 0, R(kern), R(prm), P(svi), P(coef), P(sv), R(bias), None, R(info)),
             lambda: L.fd_kernel_svm_gram(ctx.h, P(x), 3, 3, 5, 0, R(kern), None, P(qd)),
             lambda: L.fd_kernel_svm_gram(ctx.h, P(x), 3, 3, 5, 0, R(kern), P(q), None),
             lambda: L.fd_kernel_svm_gram(ctx.h, P(x), 3, 3, 5, 0, None, P(q), P(qd)),
             lambda: L.fd_kernel_svm_train_model(ctx.h, P(x), 3, 3, 5, 0, R(kern), R(prm), 0.0, 0.0, -1.0, None, R(info)),
             lambda: L.fd_kernel_svm_train_model(ctx.h, P(x), 3, 3, 5, 0, R(kern), R(prm), 0.0, 0.0, -1.0, R(h), None),
             lambda: L.fd_kernel_svm_train_model(ctx.h, P(x), 3, 3, 5, 0, None, R(prm), 0.0, 0.0, -1.0, R(h), R(info)),
             lambda: L.fd_kernel_svm_train_batch(ctx.h, 1, None, R(kern), R(prm), R(info)),
             lambda: L.fd_kernel_svm_train_batch(ctx.h, 0, None, R(kern), R(prm), R(info))]
    for i, call in enumerate(calls):
        assert call() == capi.FD_ERR_INVALID_ARGUMENT, i
        assert L.fd_last_error(ctx.h), i
    assert not h.value
    # the support vectors' rows and alpha are optional
    assert train(ctx.h, P(x), 3, 3, 5, 0, R(kern), R(prm), P(svi), P(coef), None, R(bias), None, R(info)) == capi.FD_OK
    assert info.n_sv >= 2 and (np.diff(svi[:info.n_sv]) > 0).all()
