"""The float64 restatement of libsvm's kernel C-SVC training (tests/svm_kernel_train_model.py) against libsvm itself -- recorded
results (tests/golden/svm_kernel_train_*.npz) and, where the compiled reference is present, live svm_train -- and the host-only
part of the kernel training ABI (fd_kernel_svm_train_limits)."""
import os

import numpy as np
import pytest

import svm_kernel_train_model as K
import svm_train_model as M
from test_svm_train_model import _same_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIVE_CASES = [(name, p) for name in "abce" for p in M.params_of(name)]
_cache = {}


def _golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, "svm_kernel_train_%s.npz" % name))
        x, n_pos, n_neg = M.case_x(name)
        assert float(g["xsum"]) == float(x.astype(np.float64).sum())   # the generator is pinned
        assert [tuple(k) for k in g["kernels"]] == K.KERNELS and [tuple(p) for p in g["params"]] == M.params_of(name)
        _cache[name] = (g, x, n_pos, n_neg)
    return _cache[name]


@pytest.mark.parametrize("kernel", K.KERNELS, ids=K.kernel_id)
@pytest.mark.parametrize("name", list("abc"))
def test_model_equals_recorded_libsvm(name, kernel):
    g, x, n_pos, _ = _golden(name)
    ki = K.KERNELS.index(kernel)
    q, qd = M.q_from_gram(K.kernel64(x, kernel), n_pos)
    for pi, (c, wp, wn) in enumerate(M.params_of(name)):
        r = K.train(x, n_pos, kernel, c, wp, wn, float(g["eps"]), q=q, qd=qd)
        assert r["converged"] == 1
        _same_model(r, g["alpha"][ki, pi], g["rho"][ki, pi], g["n_sv"][ki, pi], c * max(wp, wn))
        # the model's own list is what train() returns: the same examples in the same order, the same coefficients
        m = int(g["n_sv"][ki, pi])
        assert np.array_equal(r["sv_index"], g["sv_index"][ki, pi, :m])
        assert np.abs(r["coefficients"].astype(np.float64) - g["sv_coef"][ki, pi, :m]).max() <= 1e-12 * c * max(wp, wn) + np.spacing(np.float32(c * max(wp, wn)))


@pytest.mark.parametrize("name", list("abc"))
def test_recorded_sv_order_is_ascending_positives_first(name):
    """svm_train groups the classes in order of first appearance (label = {+1, -1}) and keeps the examples' order inside a class;
    with the positives first that is ascending example index, positive coefficients first"""
    g, x, n_pos, _ = _golden(name)
    for ki in range(len(K.KERNELS)):
        for pi in range(len(M.params_of(name))):
            m = int(g["n_sv"][ki, pi])
            idx, coef = g["sv_index"][ki, pi, :m], g["sv_coef"][ki, pi, :m]
            assert tuple(g["label"][ki, pi]) == (1, -1)
            assert m >= 2 and (np.diff(idx) > 0).all() and (g["sv_index"][ki, pi, m:] == -1).all()
            assert ((coef > 0) == (idx < n_pos)).all() and (coef != 0).all()


@pytest.mark.parametrize("kernel", K.KERNELS, ids=K.kernel_id)
@pytest.mark.parametrize("case", LIVE_CASES, ids=M.case_id)
def test_model_equals_live_libsvm(case, kernel, oracle):
    ref = oracle.ref()
    if ref is None:
        pytest.skip("oracle/_ref is absent (the reference tree is not on this machine)")
    name, (c, wp, wn) = case
    x, n_pos, _ = M.case_x(name)
    if ("q", name, kernel) not in _cache:
        _cache[("q", name, kernel)] = M.q_from_gram(K.kernel64(x, kernel), n_pos)
    q, qd = _cache[("q", name, kernel)]
    alpha, rho, sv_index, sv_coef, label = K.libsvm_train(ref, x, n_pos, kernel, c, wp, wn)
    r = K.train(x, n_pos, kernel, c, wp, wn, q=q, qd=qd)
    _same_model(r, alpha, rho, len(sv_index), c * max(wp, wn))
    assert np.array_equal(r["sv_index"], sv_index) and label == (1, -1)


@pytest.mark.parametrize("name", list("abce"))
def test_rbf_qd_is_one_and_q_is_float(name):
    """x_square and dot are one function in libsvm, so K_ii = exp(-gamma * 0) = 1 exactly"""
    x, n_pos, _ = M.case_x(name)
    for kernel in K.KERNELS:
        if kernel[0] != K.RBF:
            continue
        k = K.kernel64(x, kernel)
        q, qd = M.q_from_gram(k, n_pos)
        assert q.dtype == np.float32 and qd.dtype == np.float64 and (qd == 1.0).all()
        assert np.array_equal(k, k.T) and (k > 0).all() and (k <= 1.0).all()


def test_kernel_functions():
    assert K.powi(3.0, 0) == 1.0 and K.powi(3.0, 1) == 3.0 and K.powi(1.5, 5) == 1.5 ** 5 and K.powi(-2.0, 3) == -8.0
    x, n_pos, _ = M.case_x("b")
    x64 = x.astype(np.float64)
    assert np.allclose(K.kernel64(x, (K.HIK, 0, 0, 0)), np.minimum(x64[:, None, :], x64[None, :, :]).sum(axis=2), rtol=1e-14, atol=0)
    d = x64 @ x64.T
    assert np.allclose(K.kernel64(x, (K.POLY, 0.05, 0.5, 3.0)), (0.05 * d + 0.5) ** 3, rtol=1e-13, atol=0)
    sq = ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(axis=2)
    assert np.allclose(K.kernel64(x, (K.RBF, 8.0, 0, 0)), np.exp(-8.0 * sq), rtol=1e-12, atol=0)
    assert np.array_equal(K.kernel64(x, (K.LINEAR, 0, 0, 0)), M.gram64(x))
    for kernel in K.KERNELS:   # K between two sets, as the decision values use it, is the same function
        assert np.array_equal(K.kernel64_between(x[:7], x, kernel), K.kernel64(x, kernel)[:7])


# ---------------- host-only ABI ----------------
def test_kernel_train_limits(capi):
    for n_pos, n_neg, d in [(1, 1, 13), (5, 18, 117), (20, 172, 455), (20, 173, 455), (20, 180, 52), (1, 1023, 1), (1, 1024, 1), (40, 1000, 20),
                            (8192, 8192, 3)]:
        q, large, m = capi.kernel_svm_train_limits(n_pos, n_neg, d)
        n = n_pos + n_neg
        assert large == (n > 1024) and q == (n <= 1024 and M.q_in_lds(n)), (n_pos, n_neg)
        assert m == M.default_max_iterations(n) == 10000000
    assert capi.kernel_svm_train_limits(20, 172, 455)[0] and not capi.kernel_svm_train_limits(20, 173, 455)[0]   # n = 192 | 193
    assert not capi.kernel_svm_train_limits(1, 1023, 1)[1] and capi.kernel_svm_train_limits(1, 1024, 1)[1]       # n = 1024 | 1025


@pytest.mark.parametrize("n_pos,n_neg,d", [(0, 5, 13), (5, 0, 13), (-1, 5, 13), (5, 5, 0), (5, 5, -3), (16000, 385, 13), (1, 16384, 13),
                                           (2 ** 31 - 1, 2 ** 31 - 1, 13)])
def test_kernel_train_limits_invalid(capi, n_pos, n_neg, d):
    with pytest.raises(capi.FdError) as e:
        capi.kernel_svm_train_limits(n_pos, n_neg, d)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_kernel_train_limits_optional_outputs(capi):
    import ctypes as C
    m = C.c_int()
    assert capi.lib().fd_kernel_svm_train_limits(20, 100, 455, None, None, C.byref(m)) == capi.FD_OK and m.value == 10000000
    assert capi.lib().fd_kernel_svm_train_limits(20, 100, 455, None, None, None) == capi.FD_OK


def test_the_new_symbols_are_declared_and_bound(capi):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fd_hip.h")).read()
    for name in ("fd_kernel_svm_gram", "fd_kernel_svm_train", "fd_kernel_svm_train_model", "fd_kernel_svm_train_batch", "fd_kernel_svm_train_limits"):
        assert "int %s(" % name in hdr and name in capi._SIGS and hasattr(capi.lib(), name)
