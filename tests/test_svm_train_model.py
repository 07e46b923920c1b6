"""The float64 restatement of libsvm's linear C-SVC training (tests/svm_train_model.py) against libsvm itself -- recorded
results (tests/golden/svm_train_*.npz) and, where the compiled reference is present, live svm_train on every case -- and the
host-only part of the training ABI (fd_linear_svm_train_limits)."""
import os

import numpy as np
import pytest

import svm_train_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same_model(r, alpha, rho, n_sv, C):
    assert np.abs(r["alpha"] - alpha).max() <= 1e-12 * C
    assert abs(r["rho"] - rho) <= 1e-12
    assert np.array_equal(r["alpha"] > 0, alpha > 0)   # the same support vectors
    assert r["n_sv"] == n_sv


@pytest.mark.parametrize("name", list("abc"))
def test_model_equals_recorded_libsvm(name):
    g = np.load(os.path.join(GOLDEN, "svm_train_%s.npz" % name))
    x, n_pos, n_neg = M.case_x(name)
    assert np.array_equal(g["x"], x) and int(g["n_pos"]) == n_pos and int(g["n_neg"]) == n_neg   # the generator is pinned too
    assert [tuple(p) for p in g["params"]] == M.params_of(name)
    for k, (c, wp, wn) in enumerate(g["params"]):
        r = M.train(g["x"], n_pos, c, wp, wn, float(g["eps"]))
        assert r["converged"] == 1
        _same_model(r, g["alpha"][k], g["rho"][k], g["n_sv"][k], c * max(wp, wn))


def test_recorded_cases_exercise_the_bounds_and_tau():
    """what the small cases are for: a has both alpha at the bound after one iteration; c has duplicated rows of either class"""
    x, n_pos, _ = M.case_x("a")
    r = M.train(x, n_pos)
    assert r["iterations"] == 1 and r["n_bounded"] == 2 and np.array_equal(r["alpha"], [1.0, 1.0])
    x, n_pos, _ = M.case_x("c")
    k = M.gram64(x)
    assert k[1, 1] + k[7, 7] - 2 * k[1, 7] == 0.0 and k[1, 1] + k[2, 2] - 2 * k[1, 2] == 0.0   # quad_coef = 0 -> TAU


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_model_equals_live_libsvm(case, oracle):
    ref = oracle.ref()
    if ref is None:
        pytest.skip("oracle/_ref is absent (the reference tree is not on this machine)")
    name, (c, wp, wn) = case
    x, n_pos, _ = M.case_x(name)
    alpha, rho, n_sv = M.libsvm_train(ref, x, n_pos, c, wp, wn)
    _same_model(M.train(x, n_pos, c, wp, wn), alpha, rho, n_sv, c * max(wp, wn))


def test_q_is_float_and_qd_double():
    x, n_pos, _ = M.case_x("b")
    k = M.gram64(x)
    q, qd = M.q_from_gram(k, n_pos)
    assert q.dtype == np.float32 and qd.dtype == np.float64
    assert np.array_equal(qd, np.diag(k)) and np.array_equal(np.abs(q), np.abs(k).astype(np.float32))
    assert (q[:n_pos, n_pos:] <= 0).all() and (q[:n_pos, :n_pos] >= 0).all()   # non-negative features


# ---------------- host-only ABI ----------------
def test_train_limits(capi):
    for n_pos, n_neg, d in [(1, 1, 13), (5, 18, 117), (20, 100, 455), (20, 172, 455), (20, 173, 455), (20, 180, 52), (30, 290, 39),
                            (1, 1023, 1), (512, 512, 1085)]:
        q, m = capi.linear_svm_train_limits(n_pos, n_neg, d)
        n = n_pos + n_neg
        assert q == M.q_in_lds(n), (n_pos, n_neg)
        assert m == M.default_max_iterations(n) == 10000000
    # the flag is the LDS budget of one workgroup: Q padded to the tile beside alpha, G and QD
    assert M.q_in_lds(192) and not M.q_in_lds(193)
    assert capi.linear_svm_train_limits(20, 100, 455)[0] and not capi.linear_svm_train_limits(20, 180, 52)[0]


@pytest.mark.parametrize("n_pos,n_neg,d", [(0, 5, 13), (5, 0, 13), (-1, 5, 13), (5, 5, 0), (5, 5, -3), (1000, 25, 13), (1, 1024, 13),
                                           (2 ** 31 - 1, 2 ** 31 - 1, 13)])
def test_train_limits_invalid(capi, n_pos, n_neg, d):
    with pytest.raises(capi.FdError) as e:
        capi.linear_svm_train_limits(n_pos, n_neg, d)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_train_limits_optional_outputs(capi):
    import ctypes as C
    m = C.c_int()
    assert capi.lib().fd_linear_svm_train_limits(20, 100, 455, None, C.byref(m)) == capi.FD_OK and m.value == 10000000
    assert capi.lib().fd_linear_svm_train_limits(20, 100, 455, None, None) == capi.FD_OK
