"""The large training problems (tests/svm_train_large_cases.py) on the float64 restatement of libsvm (tests/svm_train_model.py):
the model equals libsvm's compiled svm_train on a problem with more than 1024 examples (recorded by
tests/golden/make_svm_train_large_golden.py), and the host-only part of the large trainer's ABI."""
import os

import numpy as np
import pytest

import svm_train_large_cases as L
import svm_train_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_model_equals_recorded_libsvm_beyond_1024_examples():
    g = np.load(os.path.join(GOLDEN, "svm_train_large.npz"))
    x, n_pos, n_neg = L.case_x("g")
    assert n_pos + n_neg > 1024 and float(g["xsum"]) == float(x.astype(np.float64).sum())   # the generator is pinned
    r = M.train(x, n_pos, 1.0, 1.0, 1.0, 1e-4)
    assert r["converged"] == 1 and r["iterations"] == int(g["iterations"])
    assert np.abs(r["alpha"] - g["alpha"]).max() <= 1e-12
    assert abs(r["rho"] - float(g["rho"])) <= 1e-12
    assert np.array_equal(r["alpha"] > 0, g["alpha"] > 0) and r["n_sv"] == int(g["n_sv"])


def test_the_cases_are_what_they_are_for():
    """p is the first size the small trainer refuses, q has three elements per thread of a 1024-thread workgroup, r has
    duplicated rows of both classes (quad_coef = 0 -> TAU), and one parameter set per weighted case differs from 1"""
    shapes = {name: L.case_x(name)[1:] for name in "pqrg"}
    assert shapes["p"] == (1, 1024) and sum(shapes["q"]) == 2 * 1024 + 37 and all(sum(s) > 1024 for s in shapes.values())
    x, n_pos, _ = L.case_x("r")
    k = M.gram64(x[[1, 3, 700, 1139, 800, 900]])
    assert k[0, 0] + k[1, 1] - 2 * k[0, 1] == 0.0 and k[0, 0] + k[2, 2] - 2 * k[0, 2] == 0.0 and k[4, 4] + k[5, 5] - 2 * k[4, 5] == 0.0
    assert 3 < n_pos <= 700
    assert any(wp != 1.0 and wn != 1.0 for _, (_, wp, wn) in L.CASES)


def test_large_train_limits(capi):
    assert capi.SVM_LARGE_MAX_N == 16384
    for n_pos, n_neg, d in [(1, 1, 13), (1, 1024, 5), (150, 1935, 7), (8192, 8192, 1), (1, 16383, 496), (16383, 1, 3)]:
        lds, m = capi.linear_svm_train_large_limits(n_pos, n_neg, d)
        n = n_pos + n_neg
        assert lds == 9 * M.padded(n) + 1024 <= M.LDS_BYTES   # G (double) and a status byte per padded row, the slots
        assert m == M.default_max_iterations(n)
    assert capi.linear_svm_train_large_limits(1, 16383, 1)[0] == 9 * 16384 + 1024


@pytest.mark.parametrize("n_pos,n_neg,d", [(0, 5, 13), (5, 0, 13), (-1, 5, 13), (5, 5, 0), (5, 5, -3), (1, 16384, 13), (16384, 1, 13),
                                           (8193, 8192, 1), (2 ** 31 - 1, 2 ** 31 - 1, 13)])
def test_large_train_limits_invalid(capi, n_pos, n_neg, d):
    with pytest.raises(capi.FdError) as e:
        capi.linear_svm_train_large_limits(n_pos, n_neg, d)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_the_small_limits_are_unchanged(capi):
    assert capi.linear_svm_train_limits(1, 1023, 1)
    with pytest.raises(capi.FdError):
        capi.linear_svm_train_limits(1, 1024, 5)
