"""tests/liblinear_model.py, the float64 restatement of l2r_l2_svc_fun and TRON, against what the reference's own linear.cpp +
tron.cpp gave on the recorded problems of tests/golden/liblinear_tron.npz (DESIGN.md 4.13 describes the recording).  No GPU."""
import os

import numpy as np
import pytest

import liblinear_cases as L
import liblinear_model as M


@pytest.mark.parametrize("name", L.golden_names())
def test_model_reproduces_the_recorded_w(name):
    """Both take the same branches (the smallest margin of a comparison is far above rounding) and differ by the order of their
    sums only: 1e-6 |w|_inf leaves room for other libm and numpy builds; the value measured at the recording is in the file."""
    g = L.golden()
    m = L.model(name)
    w_ref = g[name + "_w"]
    err = np.abs(m["w"] - w_ref).max() / np.abs(w_ref).max()
    print("%s: |w - w_ref|_inf / |w_ref|_inf = %.3g (recorded %.3g), margin %.3g, trace %s" %
          (name, err, float(g[name + "_measured"]), m["margin"], m["trace"].tolist()))
    assert m["margin"] >= 1e-6
    assert m["stop"] == M.STOP_GRADIENT and m["converged"] == 1
    assert err <= 1e-6


def test_the_recorded_cases_are_the_ones_the_trainer_is_held_to():
    shapes = {name: L.case(name)[1:3] + (L.case(name)[0].shape[1], L.case(name)[4]) for name in L.golden_names()}
    assert shapes == {"tiny": (5, 7, 3, False), "bias39": (40, 90, 39, True), "c100": (64, 64, 17, True), "onepos": (1, 200, 31, False),
                      "fewneg": (500, 3, 65, True), "wide": (30, 30, 200, False)}
    traces = np.concatenate([L.model(name)["trace"] for name in L.golden_names()])
    assert (traces[:, 1] == 1).any() and (traces[:, 2] == 0).any(), "no case hits the boundary / rejects a step"
    assert os.path.getsize(L.GOLDEN) < 300 * 1024


def test_objective_pieces_in_closed_form():
    """at w = 0: f = sum C_i, g = -2 sum C_i y_i x_i; far outside every margin: g = w and Hs = s exactly"""
    x, n_pos, n_neg, _, _ = L.case("bias39")
    X = M.design(x, True)
    y, c = M.labels_and_c(n_pos, n_neg, 2.0, 3.0, 0.5)
    f, g, hs = M.evaluate(x, n_pos, n_neg, np.zeros(40), s=np.ones(40), C=2.0, bias=True, weight_pos=3.0, weight_neg=0.5)
    assert f == pytest.approx(c.sum(), rel=1e-14)
    np.testing.assert_allclose(g, -2 * (X.T @ (c * y)), rtol=1e-12)
    np.testing.assert_allclose(hs, np.ones(40) + 2 * X.T @ (c * (X @ np.ones(40))), rtol=1e-12)
    w = L.model("bias39")["w"] * 1e6
    if np.all(y * (X @ w) > 1):
        f2, g2, hs2 = M.evaluate(x, n_pos, n_neg, w, s=np.ones(40), bias=True)
        assert np.array_equal(g2, w) and np.array_equal(hs2, np.ones(40))


def test_stops_of_the_model():
    x, n_pos, n_neg, c, bias = L.case("onepos")
    assert M.tron(x, n_pos, n_neg, C=c, bias=bias, max_iter=1)["stop"] == M.STOP_MAX_ITER
    assert M.tron(x, n_pos, n_neg, C=c, bias=bias, max_cg_steps=2)["stop"] == M.STOP_CG_CAP
    z = M.tron(np.zeros((4, 3), np.float32), 2, 2)
    assert z["stop"] == M.STOP_GRADIENT and z["iterations"] == 0 and not z["w"].any()


def test_the_new_symbols_are_declared_and_bound(capi):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fd_hip.h")).read()
    for name in ("fd_liblinear_train", "fd_liblinear_train_batch", "fd_liblinear_objective", "fd_liblinear_train_limits"):
        assert "int %s(" % name in hdr and name in capi._SIGS and hasattr(capi.lib(), name)


def test_limits_report_the_selection_rule(capi, monkeypatch):
    monkeypatch.delenv("FD_LIBLINEAR_SMALL_ROWS", raising=False)
    single, rows, scratch, lds = capi.liblinear_train_limits(100, 100, 64)
    assert single and rows == 200 and 0 < lds <= 64 * 1024 and scratch > 0
    assert not capi.liblinear_train_limits(100, 900, 1116)[0]            # more than 40960 elements
    assert not capi.liblinear_train_limits(1000, 1049, 4)[0]             # more than FD_LIBLINEAR_SMALL_MAX_N rows
    assert capi.liblinear_train_limits(320, 320, 64)[0] and not capi.liblinear_train_limits(320, 321, 64)[0]
    assert capi.liblinear_train_limits(4000, 16000, 64)[1] == 64         # 313 slabs
    single, rows, scratch, lds = capi.liblinear_train_limits(4, 1048572, 8191, True)
    assert not single and rows == 2048 and lds <= 64 * 1024 and scratch >= 512 * 8192 * 8
    monkeypatch.setenv("FD_LIBLINEAR_SMALL_ROWS", "0")
    assert capi.liblinear_train_limits(100, 100, 64)[:2] == (False, 64)
    for bad in ((0, 5, 3, 0), (5, 0, 3, 0), (5, 5, 0, 0), (5, 5, 8192, 1), (5, 1048572, 3, 0), (5, 5, 3, 2)):
        with pytest.raises(capi.FdError):
            capi.liblinear_train_limits(*bad)
