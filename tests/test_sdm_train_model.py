"""tests/sdm_train_model.py (the float64 model of supervised descent training) on the CPU oracle's descriptors:
N = 24 faces, K = 5 perturbed samples + the aligned mean, S = 3, UoCTTI, desc_params (2,8,4) (2,8,4) (1,8,4): M = 144 rows with
D = 321, 321, 81 columns -- fewer rows than columns in two steps, so lambda carries the solve."""
import numpy as np
import pytest

import sdm_train_model as T


def oracle_desc(oracle):
    return lambda gray, px, py, nc, cs, nb, variant: oracle.sdm_descriptors(gray, px, py, 0, variant, nc, cs, nb)


@pytest.fixture(scope="module")
def trained(oracle):
    ts = T.make_set(20261019, T.N_TRAIN, T.K_SAMPLES)
    rows = [ts["images"][r // ts["samples"]] for r in range(len(ts["x0"]))]
    out = T.train(oracle_desc(oracle), rows, ts["x0"], ts["gt"], T.DESC_PARAMS, T.VARIANT, T.AUTOMATIC, 0.5, False)
    return ts, out


def test_dimensions(trained):
    ts, out = trained
    assert ts["x0"].shape == (144, 10)
    assert [r.shape for r in out["R"]] == [(321, 10), (321, 10), (81, 10)]
    assert all(np.isfinite(r).all() for r in out["R"])


def test_training_error_never_increases(trained):
    """ridge guarantees ||A R - b|| <= ||b||; the float update may add sqrt(M 2L) 2^-23 max|x|"""
    ts, out = trained
    fro = [i["err_fro"] for i in out["info"]]
    slack = np.sqrt(ts["x0"].size) * 2.0 ** -23 * max(np.abs(s).max() for s in out["shapes"])
    print("train L1", [round(i["err_l1"], 3) for i in out["info"]], "fro", fro, "slack", slack)
    for a, b in zip(fro, fro[1:]):
        assert b <= a + slack
    assert fro[-1] < 0.5 * fro[0]


def test_held_out_faces_improve(oracle, trained):
    _, out = trained
    hs = T.make_set(77, T.N_HELDOUT, 0)
    before, after = [], []
    for img, x0, gt in zip(hs["images"], hs["x0"], hs["gt"]):
        x = T.fit(oracle_desc(oracle), img, x0, out["R"], T.DESC_PARAMS, T.VARIANT)
        before.append(T.errors(gt, x0)[0])
        after.append(T.errors(gt, x)[0])
    print("held-out L1 %.3f -> %.3f" % (np.mean(before), np.mean(after)))
    assert np.mean(after) < np.mean(before)


def test_cholesky_agrees_with_lapack_solve(trained):
    _, out = trained
    for lr in out["steps"]:
        ref = np.linalg.solve(lr["Mreg"], lr["Atb"])
        assert np.abs(lr["R64"] - ref).max() <= 1e-10 * np.abs(ref).max()
        assert np.array_equal(lr["AtA"], lr["AtA"].T)


def test_linear_regression_lambda_rules():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((20, 7)).astype(np.float32)
    b = rng.standard_normal((20, 3)).astype(np.float32)
    AtA = A.astype(np.float64).T @ A.astype(np.float64)
    lr = T.linear_regression(A, b, T.AUTOMATIC, 0.5, True)
    assert abs(lr["lam"] - 0.5 * np.linalg.norm(AtA) / 20) <= 1e-14 * lr["lam"]
    assert np.allclose(np.diag(lr["Mreg"]) - np.diag(AtA), lr["lam"])
    lr = T.linear_regression(A, b, T.MANUAL, 0.25, False)
    d = np.diag(lr["Mreg"]) - np.diag(AtA)
    assert lr["lam"] == 0.25 and np.allclose(d[:-1], 0.25, rtol=0, atol=1e-12) and d[-1] == 0.0
    assert np.abs(lr["Mreg"] @ lr["R64"] - lr["Atb"]).max() < 1e-12 * np.abs(lr["Atb"]).max()


def test_train_limits_host_only(capi):
    """fd_sdm_train_limits needs no device: bytes the trainer keeps resident and the largest D of the steps"""
    nbytes, dmax = capi.sdm_train_limits(T.L, T.DESC_PARAMS, 144, T.VARIANT)
    assert dmax == 321
    lda, ldb, mpad = 384, 64, 160
    assert nbytes >= 4 * mpad * lda + 8 * (lda + ldb) * lda
    with pytest.raises(capi.FdError):
        capi.sdm_train_limits(T.L, ((9, 8, 4),), 144, T.VARIANT)
