"""libsvm's sigmoid fit on the device (fd_kernel_svm_cv_sigmoid) against tests/svm_cv_sigmoid_model.py, the float64 restatement
that tests/test_svm_prob_model.py pins to libsvm itself, and against libsvm's recorded results (tests/golden/svm_cv_sigmoid_*.npz).

The cases (svm_cv_sigmoid_model.CASES):
  int65    (20 + 45) x 12 integer rows, HIK and linear, C = 2, weights 1.5 / 0.75: Q and every k_function value are exact, so the
           decision values, probA and probB are libsvm's bits
  float55  (15 + 40) x 9, poly and RBF (gamma = 2), C = 10: folds of 44 rows, held-out tiles of 11 rows
  one_pos, one_neg, pair   folds that train nothing
  large    (300 + 990) x 8 integer rows, HIK: folds of 1032 rows, five problems in one launch of the large solver
"""
import ctypes as C
import os

import numpy as np
import pytest

import svm_cv_sigmoid_model as CV
import svm_kernel_train_model as K

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-4
# max_h |dec_device - dec_model| / (2^-52 sum_s |coef_s| K_hs) of the RBF kernel, whose device exp is not libm's (at most 2 ulp apart,
# DESIGN.md 4.7): measured on an MI355X as RBF_R_MEASURED; the bound is twice that, rounded up to an integer, and at most 8.  A
# larger ratio is an error of the summation order, not of exp.
RBF_R_MEASURED = 0.578
RBF_R_CAP = min(8, int(np.ceil(2 * RBF_R_MEASURED)))
INFO_FIELDS = ("iterations", "converged", "n_sv", "n_bounded", "rho", "objective")
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _golden(name):
    g = np.load(os.path.join(GOLDEN, "svm_cv_sigmoid_%s.npz" % name))
    x, n_pos, kernels, perm, c, wp, wn = CV.case(name)
    assert float(g["xsum"]) == float(x.astype(np.float64).sum()) and np.array_equal(g["perm"], perm)
    return g


def _device(capi, ctx, name, ki, perm=None):
    key = (name, ki) if perm is None else None
    if key is None or key not in _cache:
        x, n_pos, kernels, p, c, wp, wn = CV.case(name)
        r = capi.kernel_svm_cv_sigmoid(ctx, x, n_pos, kernels[ki], p if perm is None else perm, C=c, weight_pos=wp, weight_neg=wn, eps=EPS)
        if key is None:
            return r
        _cache[key] = r
    return _cache[key]


def _fold_models(capi, ctx, name, ki, perm=None):
    """fd_kernel_svm_train on every fold's rows: [(alpha, rho) or None], [info or None]"""
    x, n_pos, kernels, p, c, wp, wn = CV.case(name)
    models, infos = [], []
    for rows, npf, held in CV.folds(p if perm is None else perm, n_pos):
        if CV.constant_of(npf, len(rows) - npf) is not None:
            models.append(None)
            infos.append(None)
            continue
        _, _, _, _, alpha, info = capi.kernel_svm_train(ctx, x[rows], npf, kernels[ki], want_support_vectors=False, C=1.0, weight_pos=c * wp,
                                                        weight_neg=c * wn, eps=EPS)
        models.append((alpha, info["rho"]))
        infos.append(info)
    return models, infos


def _assert_fold_infos(got, infos):
    for f in range(5):
        fold = got[3]["folds"][f]
        assert fold["trained"] == (infos[f] is not None)
        if infos[f] is not None:
            for name in INFO_FIELDS:
                assert _bits(np.float64(fold[name])) == _bits(np.float64(infos[f][name])), (f, name, fold[name], infos[f][name])


def _assert_fit_of_own_dec(capi, got, n_pos):
    """fd_svm_sigmoid_train and the restatement on the device's decision values give the device's probA, probB"""
    a, b, dec, info = got
    assert capi.svm_sigmoid_train(dec, n_pos) == (a, b, info["newton_iterations"], info["status"])
    assert CV.sigmoid_train(dec, n_pos) == (a, b, info["newton_iterations"], info["status"])


@pytest.mark.parametrize("ki", [0, 1], ids=["hik", "linear"])
def test_integer_rows_give_libsvm_bits(capi, ctx, ki):
    g = _golden("int65")
    x, n_pos, kernels, perm, c, wp, wn = CV.case("int65")
    got = _device(capi, ctx, "int65", ki)
    a, b, dec, info = got
    print("int65 %s: probA %.17g probB %.17g, %d Newton iterations" % (K.kernel_id(kernels[ki]), a, b, info["newton_iterations"]))
    assert _bits(dec) == _bits(g["dec"][ki]), np.abs(dec - g["dec"][ki]).max()
    assert (a, b) == (float(g["prob_a"][ki]), float(g["prob_b"][ki]))
    assert info["status"] == capi.FD_SVM_SIGMOID_CONVERGED
    models, infos = _fold_models(capi, ctx, "int65", ki)
    _assert_fold_infos(got, infos)
    _assert_fit_of_own_dec(capi, got, n_pos)


def test_poly_equals_model_on_device_alpha(capi, ctx):
    x, n_pos, kernels, perm, c, wp, wn = CV.case("float55")
    got = _device(capi, ctx, "float55", 0)
    models, infos = _fold_models(capi, ctx, "float55", 0)
    _assert_fold_infos(got, infos)
    dec, a, b, it, status, _ = CV.cross_validate(x, n_pos, kernels[0], perm, c, wp, wn, EPS, fold_models=models)
    assert _bits(got[2]) == _bits(dec), np.abs(got[2] - dec).max()
    assert (got[0], got[1]) == (a, b) and (got[3]["newton_iterations"], got[3]["status"]) == (it, status)
    _assert_fit_of_own_dec(capi, got, n_pos)


def test_rbf_within_the_exp_bound(capi, ctx):
    """the float64 model (k_function's order, math.exp) on the device's fold alpha"""
    x, n_pos, kernels, perm, c, wp, wn = CV.case("float55")
    kernel = kernels[1]
    got = _device(capi, ctx, "float55", 1)
    models, infos = _fold_models(capi, ctx, "float55", 1)
    _assert_fold_infos(got, infos)
    dec = CV.cross_validate(x, n_pos, kernel, perm, c, wp, wn, EPS, fold_models=models)[0]
    scale = np.zeros(len(x))
    for (rows, npf, held), m in zip(CV.folds(perm, n_pos), models):
        sv = np.flatnonzero(m[0] > 0)
        scale[held] = CV.k_function(x[held], x[rows[sv]], kernel) @ np.abs(m[0][sv])
    r = (np.abs(got[2] - dec) / (2.0 ** -52 * scale)).max()
    print("float55 rbf: r = %.3f (cap %d), max |d dec| = %g" % (r, RBF_R_CAP, np.abs(got[2] - dec).max()))
    assert r <= RBF_R_CAP
    _assert_fit_of_own_dec(capi, got, n_pos)


@pytest.mark.parametrize("name,fold,value", [("one_pos", 2, -1.0), ("one_neg", 4, 1.0)])
def test_a_fold_without_a_class_is_constant(capi, ctx, name, fold, value):
    g = _golden(name)
    x, n_pos, kernels, perm, c, wp, wn = CV.case(name)
    got = _device(capi, ctx, name, 0)
    a, b, dec, info = got
    assert _bits(dec) == _bits(g["dec"][0]) and (a, b) == (float(g["prob_a"][0]), float(g["prob_b"][0]))
    assert [f["trained"] for f in info["folds"]] == [f != fold for f in range(5)]
    assert info["folds"][fold]["constant"] == value and info["folds"][fold]["n_sv"] == 0
    held = CV.folds(perm, n_pos)[fold][2]
    assert len(held) == 3 and (dec[held] == value).all()
    _assert_fold_infos(got, _fold_models(capi, ctx, name, 0)[1])


def test_two_examples(capi, ctx):
    """1 + 1: folds 2 and 4 are constant, folds 0, 1 and 3 hold nothing out"""
    g = _golden("pair")
    a, b, dec, info = _device(capi, ctx, "pair", 0)
    assert a == 0.6931471784024834 == float(g["prob_a"][0]) and b == float(g["prob_b"][0]) and _bits(dec) == _bits(g["dec"][0])
    assert [f["trained"] for f in info["folds"]] == [True, True, False, True, False]
    assert sorted(f["constant"] for f in info["folds"] if not f["trained"]) == [-1.0, 1.0]


def test_large_folds_in_one_launch(capi, ctx):
    g = _golden("large")
    x, n_pos, kernels, perm, c, wp, wn = CV.case("large")
    got = _device(capi, ctx, "large", 0)
    a, b, dec, info = got
    print("large hik: probA %.17g probB %.17g" % (a, b))
    assert [len(f[0]) for f in CV.folds(perm, n_pos)] == [1032] * 5
    assert _bits(dec) == _bits(g["dec"][0]), np.abs(dec - g["dec"][0]).max()
    assert (a, b) == (float(g["prob_a"][0]), float(g["prob_b"][0]))
    assert all(f["trained"] and f["converged"] == 1 and f["launches"] == info["folds"][0]["launches"] for f in info["folds"])
    _assert_fold_infos(got, _fold_models(capi, ctx, "large", 0)[1])


def test_folds_on_either_solver(capi, ctx):
    """1281 rows: the training parts have 1025 rows (folds 0 to 3: the large solver) and 1024 rows (fold 4)"""
    x, n_pos, kernels, _, c, wp, wn = CV.case("large")
    x = x[:1281]
    perm = CV.libc_perm(11, 1281)
    assert [len(f[0]) for f in CV.folds(perm, n_pos)] == [1025, 1025, 1025, 1025, 1024]
    got = capi.kernel_svm_cv_sigmoid(ctx, x, n_pos, kernels[0], perm, eps=EPS)
    models, infos = [], []
    for rows, npf, held in CV.folds(perm, n_pos):
        _, _, _, _, alpha, info = capi.kernel_svm_train(ctx, x[rows], npf, kernels[0], want_support_vectors=False, eps=EPS)
        models.append((alpha, info["rho"]))
        infos.append(info)
    _assert_fold_infos(got, infos)
    dec = CV.cross_validate(x, n_pos, kernels[0], perm, eps=EPS, fold_models=models)[0]
    assert _bits(got[2]) == _bits(dec)
    _assert_fit_of_own_dec(capi, got, n_pos)


def test_identity_permutation(capi, ctx):
    """the last fold then holds out negatives only, the first one positives only"""
    x, n_pos, kernels, _, c, wp, wn = CV.case("int65")
    perm = np.arange(len(x), dtype=np.int32)
    got = _device(capi, ctx, "int65", 0, perm)
    models, infos = _fold_models(capi, ctx, "int65", 0, perm)
    _assert_fold_infos(got, infos)
    dec, a, b, it, status, _ = CV.cross_validate(x, n_pos, kernels[0], perm, c, wp, wn, EPS, fold_models=models)
    assert _bits(got[2]) == _bits(dec) and (got[0], got[1]) == (a, b)
    assert _bits(dec) == _bits(CV.cross_validate(x, n_pos, kernels[0], perm, c, wp, wn, EPS)[0])   # and the float64 training


def test_two_calls_give_the_same_bits(capi, ctx):
    for name, ki in (("int65", 0), ("float55", 1)):
        a = _device(capi, ctx, name, ki, CV.case(name)[3])
        b = _device(capi, ctx, name, ki, CV.case(name)[3])
        assert a[:2] == b[:2] and _bits(a[2]) == _bits(b[2]) and a[3] == b[3]


def test_device_input(capi, ctx):
    import torch
    x, n_pos, kernels, perm, c, wp, wn = CV.case("float55")
    got = capi.kernel_svm_cv_sigmoid(ctx, torch.from_numpy(x).cuda(), n_pos, kernels[1], perm, C=c, weight_pos=wp, weight_neg=wn, eps=EPS)
    want = _device(capi, ctx, "float55", 1)
    assert got[:2] == want[:2] and _bits(got[2]) == _bits(want[2]) and got[3] == want[3]


@pytest.mark.parametrize("bad", ["repeat", "negative", "too_large"])
def test_a_non_permutation_is_rejected(capi, ctx, bad):
    x, n_pos, kernels, perm, c, wp, wn = CV.case("int65")
    p = perm.copy()
    p[5] = {"repeat": p[6], "negative": -1, "too_large": len(x)}[bad]
    with pytest.raises(capi.FdError) as e:
        capi.kernel_svm_cv_sigmoid(ctx, x, n_pos, kernels[0], p)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "permutation" in str(e.value)


def test_invalid_arguments(capi, ctx):
    x, n_pos, kernels, perm, c, wp, wn = CV.case("int65")
    L = capi.lib()
    k, prm, a, b = capi.svm_kernel(K.HIK), capi.svm_train_params(), C.c_double(), C.c_double()
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    call = lambda xp, npos, nneg, d, kk, pp, perm_, pa, pb: L.fd_kernel_svm_cv_sigmoid(ctx.h, xp, npos, nneg, d, 0, kk, pp, perm_, pa, pb, None, None)
    ok = (p(x), 20, 45, 12, C.byref(k), C.byref(prm), p(perm), C.byref(a), C.byref(b))
    assert call(*ok) == capi.FD_OK   # dec_values and cv_info are optional
    for pos in (0, 4, 5, 6, 7, 8):
        args = list(ok)
        args[pos] = None
        assert call(*args) == capi.FD_ERR_INVALID_ARGUMENT, pos
    for npos, nneg, d in ((0, 45, 12), (20, 0, 12), (20, 45, 0), (16000, 385, 12)):
        assert call(p(x), npos, nneg, d, *ok[4:]) == capi.FD_ERR_INVALID_ARGUMENT
    for bad in (capi.svm_train_params(C=0.0), capi.svm_train_params(weight_neg=-1.0), capi.svm_train_params(eps=-1.0)):
        assert call(*ok[:5], C.byref(bad), *ok[6:]) == capi.FD_ERR_INVALID_ARGUMENT
    badk = capi.svm_kernel(9)
    assert call(*ok[:4], C.byref(badk), *ok[5:]) == capi.FD_ERR_INVALID_ARGUMENT
