"""Linear C-SVC training for up to 16384 examples on the device (fd_linear_svm_gram_large / _train_large) against
tests/svm_train_model.py, bit for bit on the device's Q, on the problems of tests/svm_train_large_cases.py."""
import os

import numpy as np
import pytest

import svm_train_large_cases as L
import svm_train_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-4
_cache = {}


def case_id(case):
    name, (c, wp, wn) = case
    return "%s-C%g-%s" % (name, c, "w" if wp != 1.0 else "u")


def _problem(name):
    if ("x", name) not in _cache:
        x, n_pos, n_neg = L.case_x(name)
        _cache[("x", name)] = (x, n_pos, n_neg, M.gram64(x))
    return _cache[("x", name)]


def _device_gram(capi, ctx, name):
    if ("q", name) not in _cache:
        x, n_pos, _, _ = _problem(name)
        _cache[("q", name)] = capi.linear_svm_gram_large(ctx, x, n_pos)
    return _cache[("q", name)]


def _model_on_device_q(capi, ctx, case, max_iterations=0):
    key = ("m", case, max_iterations)
    if key not in _cache:
        name, (c, wp, wn) = case
        x, n_pos, _, _ = _problem(name)
        q, qd = _device_gram(capi, ctx, name)
        _cache[key] = M.train(x, n_pos, c, wp, wn, EPS, max_iterations, q=q, qd=qd)
    return _cache[key]


def _device_train(capi, ctx, case, **kw):
    name, (c, wp, wn) = case
    x, n_pos, _, _ = _problem(name)
    return capi.linear_svm_train_large(ctx, x, n_pos, C=c, weight_pos=wp, weight_neg=wn, **kw)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_same_bits(got, want):
    w, bias, alpha, info = got
    assert _bits(alpha) == _bits(want["alpha"]), "alpha: max |d| = %g" % np.abs(alpha - want["alpha"]).max()
    assert info["iterations"] == want["iterations"] and info["converged"] == want["converged"]
    assert _bits(np.float64(info["rho"])) == _bits(np.float64(want["rho"])), (info["rho"], want["rho"])
    assert _bits(np.float64(info["objective"])) == _bits(np.float64(want["objective"])), (info["objective"], want["objective"])
    assert (info["n_sv"], info["n_bounded"]) == (want["n_sv"], want["n_bounded"])
    assert w.dtype == np.float32 and _bits(w) == _bits(want["weights"]), "w: max |d| = %g" % np.abs(w - want["weights"]).max()
    assert _bits(np.float32(bias)) == _bits(np.float32(want["rho"]))


@pytest.mark.parametrize("name", list("pqrg"))
def test_gram(capi, ctx, name):
    """the bounds of test_gpu_svm_train.test_gram: Q within one float ulp of float32(float64 Gram), QD within 4 d double ulp, Q
    symmetric"""
    x, n_pos, n_neg, k = _problem(name)
    q, qd = _device_gram(capi, ctx, name)
    want_q, want_qd = M.q_from_gram(k, n_pos)
    dq = np.abs(q.astype(np.float64) - want_q.astype(np.float64))
    print("gram %s: max |dQ| / ulp = %g, max |dQD| / ulp = %g" % (name, (dq / np.spacing(np.abs(want_q)).astype(np.float64)).max(),
                                                                 (np.abs(qd - want_qd) / np.spacing(want_qd)).max()))
    assert (dq <= np.spacing(np.abs(want_q)).astype(np.float64)).all()
    assert (np.abs(qd - want_qd) <= 4 * x.shape[1] * np.spacing(want_qd)).all()
    assert np.array_equal(q, q.T)


@pytest.mark.parametrize("case", L.CASES, ids=case_id)
def test_solver_equals_model_bit_for_bit(capi, ctx, case):
    want = _model_on_device_q(capi, ctx, case)
    got = _device_train(capi, ctx, case)
    assert want["converged"] == 1 and got[3]["launches"] == 1
    _assert_same_bits(got, want)


@pytest.mark.parametrize("case", [("p", (0.5, 8.0, 0.25)), ("q", (1.0, 1.0, 1.0))], ids=case_id)
def test_relaunch_gives_the_same_bits(capi, ctx, case):
    want = _model_on_device_q(capi, ctx, case)
    got = _device_train(capi, ctx, case, launch_iterations=61)
    assert got[3]["launches"] == want["iterations"] // 61 + 1 >= 3
    _assert_same_bits(got, want)


def test_max_iterations_is_not_an_error(capi, ctx):
    case = ("q", (1.0, 1.0, 1.0))
    want = _model_on_device_q(capi, ctx, case, max_iterations=5)
    assert want["iterations"] == 5 and want["converged"] == 0
    got = _device_train(capi, ctx, case, max_iterations=5)   # FD_OK: no FdError
    _assert_same_bits(got, want)
    got = _device_train(capi, ctx, case, max_iterations=5, launch_iterations=2)
    assert got[3]["launches"] == 3
    _assert_same_bits(got, want)


@pytest.mark.parametrize("case", L.CASES, ids=case_id)
def test_solution_is_optimal(capi, ctx, case):
    """independent of the model, as test_gpu_svm_train does: with G recomputed in float64 from the returned alpha and the exact
    Gram, m(alpha) - M(alpha) < eps + s and rho between -m and -M up to s (s = n C_max 2^-24 max|K|, the effect of rounding Q to
    float)"""
    name, (c, wp, wn) = case
    x, n_pos, n_neg, k = _problem(name)
    n = n_pos + n_neg
    y = M.labels(n_pos, n_neg)
    Cs = np.where(y > 0, c * wp, c * wn)
    w, bias, alpha, info = _device_train(capi, ctx, case)
    assert (alpha >= 0).all() and (alpha <= Cs).all() and abs(float(alpha @ y)) <= 1e-12 * Cs.max() * n
    G = (np.outer(y, y) * k) @ alpha - 1.0
    up = ((y > 0) & (alpha < Cs)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < Cs))
    m, Mm = (-y * G)[up].max(), (-y * G)[low].min()
    s = n * Cs.max() * 2.0 ** -24 * np.abs(k).max()
    print("%s: m - M = %g, eps + s = %g, rho = %r in [%r, %r]" % (case_id(case), m - Mm, EPS + s, info["rho"], -m, -Mm))
    assert m - Mm < EPS + s
    assert min(-m, -Mm) - s <= info["rho"] <= max(-m, -Mm) + s


def _rho64(alpha, G, y, Cs):
    free = (alpha > 0) & (alpha < Cs)
    if free.any():
        return float((y * G)[free].mean())
    up = ((y > 0) & (alpha < Cs)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < Cs))
    return float((-(-y * G)[up].max() - (-y * G)[low].min()) / 2)


def _gap(x64, y, Cs, alpha, w, rho):
    margins = y * (x64 @ w - rho)
    primal = 0.5 * float(w @ w) + float((Cs * np.maximum(0.0, 1.0 - margins)).sum())
    v = (alpha * y) @ x64
    dual = float(alpha.sum()) - 0.5 * float(v @ v)
    return primal - dual


def test_solution_is_near_recorded_libsvm(capi, ctx):
    """libsvm's recorded alpha for case g, compared the way test_gpu_svm_train compares its cases d to f:
    |w - w_libsvm| <= sqrt(2 gap) + sqrt(2 gap_libsvm) (strong convexity of the primal), both gaps non-negative up to 1e-9 of
    the objective"""
    case = ("g", (1.0, 1.0, 1.0))
    x, n_pos, n_neg, k = _problem("g")
    g = np.load(os.path.join(GOLDEN, "svm_train_large.npz"))
    assert float(g["xsum"]) == float(x.astype(np.float64).sum())
    a_ref = g["alpha"]
    y = M.labels(n_pos, n_neg)
    Cs = np.ones(n_pos + n_neg)
    w, bias, alpha, info = _device_train(capi, ctx, case)
    x64 = x.astype(np.float64)
    w_ref = (a_ref * y) @ x64
    G_ref = (np.outer(y, y) * k) @ a_ref - 1.0
    gap_ref = _gap(x64, y, Cs, a_ref, w_ref, _rho64(a_ref, G_ref, y, Cs))
    gap = _gap(x64, y, Cs, alpha, w.astype(np.float64), info["rho"])
    dist = float(np.linalg.norm(w.astype(np.float64) - w_ref))
    print("|w - w_libsvm| = %g, gaps %g %g" % (dist, gap, gap_ref))
    assert gap >= -1e-9 * max(1.0, abs(info["objective"])) and gap_ref >= -1e-9 * max(1.0, abs(info["objective"]))
    assert dist <= np.sqrt(2 * max(gap, 0.0)) + np.sqrt(2 * max(gap_ref, 0.0))


@pytest.mark.parametrize("n_pos,n_rows,kw", [
    (0, 1100, {}), (1100, 1100, {}),
    (3, 1100, {"C": 0.0}), (3, 1100, {"weight_pos": 0.0}), (3, 1100, {"weight_neg": -2.0}), (3, 1100, {"eps": -1e-3}),
    (3, 1100, {"max_iterations": -1}), (3, 1100, {"launch_iterations": -1}), (3, 1100, {"C": float("nan")})])
def test_invalid_arguments(capi, ctx, n_pos, n_rows, kw):
    x = np.ones((n_rows, 5), np.float32)
    with pytest.raises(capi.FdError) as e:
        capi.linear_svm_train_large(ctx, x, n_pos, **kw)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and len(str(e.value)) > len("fd_hip error 1: ")
    if not kw:
        with pytest.raises(capi.FdError) as e:
            capi.linear_svm_gram_large(ctx, x, n_pos)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_too_many_examples_and_null_pointers(capi, ctx):
    import ctypes as C
    lib = capi.lib()
    x = np.ones((6, 5), np.float32)
    w, q, qd = np.zeros(5, np.float32), np.zeros((6, 6), np.float32), np.zeros(6)
    bias, info, prm = C.c_float(), capi.fd_svm_train_info(), capi.svm_train_params()
    P = capi._ptr
    calls = [lambda: lib.fd_linear_svm_train_large(ctx.h, None, 3, 3, 5, 0, C.byref(prm), P(w), C.byref(bias), None, C.byref(info)),
             lambda: lib.fd_linear_svm_train_large(ctx.h, P(x), 3, 3, 5, 0, None, P(w), C.byref(bias), None, C.byref(info)),
             lambda: lib.fd_linear_svm_train_large(ctx.h, P(x), 3, 3, 5, 0, C.byref(prm), None, C.byref(bias), None, C.byref(info)),
             lambda: lib.fd_linear_svm_train_large(ctx.h, P(x), 3, 3, 5, 0, C.byref(prm), P(w), None, None, C.byref(info)),
             lambda: lib.fd_linear_svm_train_large(ctx.h, P(x), 3, 3, 5, 0, C.byref(prm), P(w), C.byref(bias), None, None),
             lambda: lib.fd_linear_svm_train_large(ctx.h, P(x), 3, 3, 0, 0, C.byref(prm), P(w), C.byref(bias), None, C.byref(info)),
             # 16385 examples: refused before any row is read
             lambda: lib.fd_linear_svm_train_large(ctx.h, P(x), 3, 16382, 5, 0, C.byref(prm), P(w), C.byref(bias), None, C.byref(info)),
             lambda: lib.fd_linear_svm_gram_large(ctx.h, P(x), 3, 16382, 5, 0, P(q), P(qd)),
             lambda: lib.fd_linear_svm_gram_large(ctx.h, P(x), 3, 3, 5, 0, None, P(qd)),
             lambda: lib.fd_linear_svm_gram_large(ctx.h, P(x), 3, 3, 5, 0, P(q), None)]
    for i, call in enumerate(calls):
        assert call() == capi.FD_ERR_INVALID_ARGUMENT, i
        assert lib.fd_last_error(ctx.h), i
    # alpha is optional, and a small problem is a valid large one
    assert lib.fd_linear_svm_train_large(ctx.h, P(x + np.arange(6, dtype=np.float32)[:, None]), 3, 3, 5, 0, C.byref(prm), P(w), C.byref(bias),
                                         None, C.byref(info)) == capi.FD_OK


def test_small_problem_gives_the_small_trainers_bits(capi, ctx):
    """the two solvers run the same arithmetic: on a problem both accept, the same model"""
    x, n_pos, _ = M.case_x("f")
    a = capi.linear_svm_train(ctx, x, n_pos)
    b = capi.linear_svm_train_large(ctx, x, n_pos)
    assert _bits(a[0]) == _bits(b[0]) and a[1] == b[1] and _bits(a[2]) == _bits(b[2])
    assert {k: v for k, v in a[3].items()} == {k: v for k, v in b[3].items()}


def test_the_small_entry_points_still_refuse_1025(capi, ctx):
    x, n_pos, _, _ = _problem("p")
    for call in (lambda: capi.linear_svm_train(ctx, x, n_pos), lambda: capi.linear_svm_gram(ctx, x, n_pos),
                 lambda: capi.linear_svm_train_batch(ctx, [(x, n_pos)])):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
