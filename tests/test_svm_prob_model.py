"""The float64 restatements of libsvm's one-class training (tests/svm_one_class_model.py) and of its sigmoid fit
(tests/svm_cv_sigmoid_model.py) against libsvm itself -- recorded results (tests/golden/svm_one_class_*.npz, svm_cv_sigmoid_*.npz,
made by tests/golden/make_svm_prob_golden.py) and, where the compiled reference is present, live svm_train -- and the host-only
part of the ABI: fd_svm_sigmoid_train, fd_one_class_svm_train_limits.

Both models restate libsvm's own Kernel functions, so their Q is libsvm's for every kernel and the comparison is bit for bit
throughout (the integer rows with the histogram-intersection and the linear kernel are the cases whose Q the device reproduces
too)."""
import ctypes as C
import os

import numpy as np
import pytest

import svm_cv_sigmoid_model as CV
import svm_kernel_train_model as K
import svm_one_class_model as OC
import svm_train_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OC_KERNELS = K.KERNELS + [OC.LINEAR_KERNEL]
CV_CASES = [(name, ki) for name in CV.CASES for ki in range(len(CV.CASES[name][5]))]
CV_SMALL = [(name, ki) for name, ki in CV_CASES if name != "large"]   # the float64 solver needs minutes on the large case
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _cv_id(v):
    return v if isinstance(v, str) else str(v)


def _oc_golden():
    if "oc" not in _cache:
        g = np.load(os.path.join(GOLDEN, "svm_one_class_int40.npz"))
        x = OC.case_x("int40")
        assert float(g["xsum"]) == float(x.astype(np.float64).sum())   # the generator is pinned
        assert [tuple(k) for k in g["kernels"]] == OC_KERNELS and g["nus"].tolist() == OC.NUS
        _cache["oc"] = g
    return _cache["oc"]


def _cv_golden(name):
    if ("cv", name) not in _cache:
        g = np.load(os.path.join(GOLDEN, "svm_cv_sigmoid_%s.npz" % name))
        x, n_pos, kernels, perm, c, wp, wn = CV.case(name)
        assert float(g["xsum"]) == float(x.astype(np.float64).sum())
        assert [tuple(k) for k in g["kernels"]] == list(kernels)
        assert np.array_equal(g["perm"], perm)   # libc's rand() is the recorded one
        _cache[("cv", name)] = g
    return _cache[("cv", name)]


def _cv_model(name, ki):
    if ("cvm", name, ki) not in _cache:
        x, n_pos, kernels, perm, c, wp, wn = CV.case(name)
        _cache[("cvm", name, ki)] = CV.cross_validate(x, n_pos, kernels[ki], perm, c, wp, wn)
    return _cache[("cvm", name, ki)]


# ---------------- one-class ----------------
@pytest.mark.parametrize("nu", OC.NUS)
@pytest.mark.parametrize("kernel", OC_KERNELS, ids=K.kernel_id)
def test_one_class_model_equals_recorded_libsvm(kernel, nu):
    g = _oc_golden()
    ki, ni = OC_KERNELS.index(kernel), OC.NUS.index(nu)
    r = OC.train(OC.case_x("int40"), kernel, nu, float(g["eps"]))
    assert r["converged"] == 1
    assert _bits(r["alpha"]) == _bits(g["alpha"][ki, ni]) and _bits(np.float64(r["rho"])) == _bits(g["rho"][ki, ni])
    assert np.isinf(r["rho"]) == (nu == 1.0)


@pytest.mark.parametrize("nu", OC.NUS)
@pytest.mark.parametrize("kernel", OC_KERNELS, ids=K.kernel_id)
@pytest.mark.parametrize("name", ["int40", "float55"])
def test_one_class_model_equals_live_libsvm(name, kernel, nu, oracle):
    ref = oracle.ref()
    if ref is None:
        pytest.skip("oracle/_ref is absent (the reference tree is not on this machine)")
    x = OC.case_x(name)
    alpha, rho, sv_index = OC.libsvm_train(ref, x, kernel, nu)
    r = OC.train(x, kernel, nu)
    assert _bits(r["alpha"]) == _bits(alpha) and _bits(np.float64(r["rho"])) == _bits(np.float64(rho))
    assert np.array_equal(r["sv_index"], sv_index)


@pytest.mark.parametrize("n,nu,full,frac", [(40, 0.02, 0, 0.8), (40, 0.26, 10, 0.4), (40, 0.5, 20, 0.0), (40, 1.0, 40, None), (1, 1.0, 1, None),
                                            (1, 0.3, 0, 0.3)])
def test_one_class_start_state(n, nu, full, frac):
    a = OC.start_alpha(n, nu)
    assert (a[:full] == 1.0).all() and (a[full + 1:] == 0.0).all()
    if frac is not None:
        assert a[full] == nu * n - full and abs(a[full] - frac) < 1e-12
    assert abs(a.sum() - nu * n) <= 1e-12 * nu * n
    q = np.arange(n * n, dtype=np.float32).reshape(n, n) / 7
    g = OC.start_gradient(q, a)
    assert np.allclose(g, a @ q.astype(np.float64), rtol=1e-14)


# ---------------- the sigmoid fit ----------------
@pytest.mark.parametrize("name,ki", CV_SMALL, ids=_cv_id)
def test_cv_model_equals_recorded_libsvm(name, ki):
    g = _cv_golden(name)
    dec, a, b, it, status, models = _cv_model(name, ki)
    assert _bits(dec) == _bits(g["dec"][ki]), np.abs(dec - g["dec"][ki]).max()
    assert _bits(np.float64(a)) == _bits(g["prob_a"][ki]) and _bits(np.float64(b)) == _bits(g["prob_b"][ki])
    assert status == CV.CONVERGED and 1 <= it <= 10


@pytest.mark.parametrize("name,ki", CV_CASES, ids=_cv_id)
def test_cv_equals_live_libsvm(name, ki, oracle):
    """svm_train with probability = 1 behind srand(seed) gives the recorded probA, probB; the restated fit on libsvm's own
    fold-by-fold decision values gives them too; and (small cases) so does the whole model"""
    ref = oracle.ref()
    if ref is None:
        pytest.skip("oracle/_ref is absent (the reference tree is not on this machine)")
    x, n_pos, kernels, perm, c, wp, wn = CV.case(name)
    g = _cv_golden(name)
    a, b = CV.libsvm_prob(ref, x, n_pos, kernels[ki], CV.CASES[name][6], c, wp, wn)
    assert (a, b) == (float(g["prob_a"][ki]), float(g["prob_b"][ki]))
    dec = CV.libsvm_cv_dec(ref, x, n_pos, kernels[ki], perm, c, wp, wn)
    assert _bits(dec) == _bits(g["dec"][ki])
    assert CV.sigmoid_train(dec, n_pos)[:2] == (a, b)
    if name != "large":
        assert _bits(_cv_model(name, ki)[0]) == _bits(dec)


def test_cv_degenerate_folds():
    """one_pos: fold 2 trains on no positive and its three held-out rows get -1; one_neg: fold 4 gets +1; pair: folds 2 and 4 are
    constant, the others hold nothing out"""
    for name, fold, value, count in (("one_pos", 2, -1.0, 3), ("one_neg", 4, 1.0, 3)):
        x, n_pos, kernels, perm, c, wp, wn = CV.case(name)
        dec, a, b, it, status, models = _cv_model(name, 0)
        assert [m is None for m in models] == [f == fold for f in range(5)]
        held = CV.folds(perm, n_pos)[fold][2]
        assert len(held) == count and (dec[held] == value).all()
    dec, a, b, it, status, models = _cv_model("pair", 0)
    assert [m is None for m in models] == [False, False, True, False, True]
    assert [len(f[2]) for f in CV.folds(CV.case("pair")[3], 1)] == [0, 0, 1, 0, 1]
    assert a == 0.6931471784024834 and sorted(dec.tolist()) == [-1.0, 1.0]


def test_libc_permutation_is_a_permutation():
    for seed, n in ((7, 65), (9, 55), (1, 2), (3, 12)):
        p = CV.libc_perm(seed, n)
        assert sorted(p.tolist()) == list(range(n)) and np.array_equal(p, CV.libc_perm(seed, n))


@pytest.mark.parametrize("name,ki", CV_CASES, ids=_cv_id)
def test_fd_svm_sigmoid_train_equals_the_restatement(capi, name, ki):
    """bit for bit, with the iteration count and the status, on the recorded decision values"""
    g = _cv_golden(name)
    n_pos = CV.case(name)[1]
    dec = g["dec"][ki]
    a, b, it, status = capi.svm_sigmoid_train(dec, n_pos)
    assert (a, b, it, status) == CV.sigmoid_train(dec, n_pos)
    assert (a, b) == (float(g["prob_a"][ki]), float(g["prob_b"][ki])) and status == capi.FD_SVM_SIGMOID_CONVERGED


def test_fd_svm_sigmoid_train_other_exits(capi):
    """values the fit cannot separate and constant ones; a single value; every label on one side"""
    rng = np.random.default_rng(5)
    for dec, n_pos in ((rng.normal(0, 1, 37), 11), (np.zeros(9), 4), (np.array([2.5]), 1), (np.array([-1.0, 3.0, 0.5]), 0),
                       (np.array([-1.0, 3.0, 0.5]), 3), (np.concatenate([np.full(20, 1e3), np.full(20, -1e3)]), 20)):
        assert capi.svm_sigmoid_train(dec, n_pos) == CV.sigmoid_train(dec, n_pos)


def test_fd_svm_sigmoid_train_invalid(capi):
    dec = np.zeros(4)
    for d, n_pos in ((dec[:0], 0), (dec, -1), (dec, 5)):
        with pytest.raises(capi.FdError) as e:
            capi.svm_sigmoid_train(d, n_pos)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    a, b = C.c_double(), C.c_double()
    p = dec.ctypes.data_as(C.c_void_p)
    assert capi.lib().fd_svm_sigmoid_train(4, None, 2, C.byref(a), C.byref(b), None, None) == capi.FD_ERR_INVALID_ARGUMENT
    assert capi.lib().fd_svm_sigmoid_train(4, p, 2, None, C.byref(b), None, None) == capi.FD_ERR_INVALID_ARGUMENT
    assert capi.lib().fd_svm_sigmoid_train(4, p, 2, C.byref(a), None, None, None) == capi.FD_ERR_INVALID_ARGUMENT
    assert capi.lib().fd_svm_sigmoid_train(4, p, 2, C.byref(a), C.byref(b), None, None) == capi.FD_OK   # the counts are optional


# ---------------- host-only limits ----------------
def test_one_class_train_limits(capi):
    for n, d in [(1, 13), (40, 10), (192, 455), (193, 455), (1024, 1), (1025, 1), (1040, 8), (16384, 3)]:
        q, large, m = capi.one_class_svm_train_limits(n, d)
        assert large == (n > 1024) and q == (n <= 1024 and M.q_in_lds(n)), n
        assert m == M.default_max_iterations(n) == 10000000
        if n >= 2:   # kernel_svm_train_limits' rules for the same number of examples
            assert (q, large, m) == capi.kernel_svm_train_limits(1, n - 1, d)
    assert capi.lib().fd_one_class_svm_train_limits(40, 10, None, None, None) == capi.FD_OK


@pytest.mark.parametrize("n,d", [(0, 13), (-1, 13), (5, 0), (5, -3), (16385, 13), (2 ** 31 - 1, 13)])
def test_one_class_train_limits_invalid(capi, n, d):
    with pytest.raises(capi.FdError) as e:
        capi.one_class_svm_train_limits(n, d)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_the_new_symbols_are_declared_and_bound(capi):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fd_hip.h")).read()
    for name in ("fd_one_class_svm_gram", "fd_one_class_svm_train", "fd_one_class_svm_train_model", "fd_one_class_svm_train_limits",
                 "fd_kernel_svm_cv_sigmoid", "fd_svm_sigmoid_train"):
        assert "int %s(" % name in hdr and name in capi._SIGS and hasattr(capi.lib(), name)
