"""liblinear's L2-loss SVC trained with TRON on the device (fd_liblinear_*) against tests/liblinear_model.py.

fun / grad / Hv are held to the componentwise rounding bound of a double evaluation in any order (liblinear_model.bounds: no
measured constant); a training run at the reference's eps must take the model's path step for step, which the model's smallest
comparison margin licenses; at a tight tolerance the returned w is certified by its own float64 gradient, f being 1-strongly
convex.  Every case runs through both forms: the single-workgroup kernel and, with FD_LIBLINEAR_SMALL_ROWS=0, the
multi-workgroup pair."""
import numpy as np
import pytest

import liblinear_cases as L
import liblinear_model as M

pytestmark = pytest.mark.gpu

FORMS = ["single", "multi"]


@pytest.fixture(params=FORMS)
def form(request, monkeypatch):
    if request.param == "multi":
        monkeypatch.setenv("FD_LIBLINEAR_SMALL_ROWS", "0")
    else:
        monkeypatch.delenv("FD_LIBLINEAR_SMALL_ROWS", raising=False)
    return request.param


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(a, b):
    """two results of liblinear_train, bit for bit"""
    return (_bits(a[0]) == _bits(b[0]) and np.float32(a[1]).tobytes() == np.float32(b[1]).tobytes() and _bits(a[2]) == _bits(b[2])
            and np.array_equal(a[3], b[3]) and a[4] == b[4])


def _check_objective(capi, ctx, x, n_pos, w, s, **kw):
    """device fun / grad / Hv at w against the model within the rounding bound; returns the device's triple"""
    n_neg = x.shape[0] - n_pos
    f, g, hs = capi.liblinear_objective(ctx, x, n_pos, w, s, **kw)
    mk = dict(C=kw.get("C", 1.0), bias=kw.get("bias", False), weight_pos=kw.get("weight_pos", 1.0), weight_neg=kw.get("weight_neg", 1.0))
    f64, g64, hs64 = M.evaluate(x, n_pos, n_neg, w, s, **mk)
    bf, bg, bh = M.bounds(x, n_pos, n_neg, w, s, **mk)
    print("f %.17g model %.17g bound %.3g | max |g - g64| / B %.3g | max |Hs - Hs64| / B %.3g" % (
        f, f64, bf, np.max(np.abs(g - g64) / np.maximum(bg, 1e-300)), np.max(np.abs(hs - hs64) / np.maximum(bh, 1e-300)) if s is not None else 0))
    assert abs(f - f64) <= bf
    assert np.all(np.abs(g - g64) <= bg)
    if s is not None:
        assert np.all(np.abs(hs - hs64) <= bh)
    return f, g, hs


# ---- 1. start values in closed form ----

@pytest.mark.parametrize("bias", [False, True])
def test_start_values_in_closed_form(capi, ctx, form, bias):
    x, n_pos, n_neg, _, _ = L.case("bias39")
    kw = dict(C=2.0, weight_pos=3.0, weight_neg=0.5, bias=bias)
    m = x.shape[1] + int(bias)
    f, g, _ = capi.liblinear_objective(ctx, x, n_pos, np.zeros(m), **kw)
    X = M.design(x, bias)
    y, c = M.labels_and_c(n_pos, n_neg, 2.0, 3.0, 0.5)
    bf, bg, _ = M.bounds(x, n_pos, n_neg, np.zeros(m), **kw)
    assert abs(f - c.sum()) <= bf
    want = -2.0 * (X.T @ (c * y))
    assert np.all(np.abs(g - want) <= bg)
    if bias:
        assert abs(g[-1] - -2.0 * np.sum(c * y)) <= bg[-1]


# ---- 2. fun / grad / Hv at the edges ----

EDGE_SHAPES = [(1, 1, 1, False), (1, 1, 3, True), (20, 43, 63, False), (32, 32, 64, True), (30, 35, 65, False), (64, 65, 129, True),
               (3, 5, 8191, True), (4, 4, 8192, False)]   # n = 2, 63, 64, 65 (a slab and one row either way), 129 (a last slab of one row)


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "%d+%dx%d%s" % (s[0], s[1], s[2], "b" if s[3] else ""))
def test_objective_at_the_edges(capi, ctx, form, shape):
    n_pos, n_neg, d, bias = shape
    n, m = n_pos + n_neg, d + int(bias)
    rng = np.random.default_rng(n * 10007 + d)
    x = L.make_x(n * 31 + d, n_pos, n_neg, d)
    kw = dict(C=1.5, weight_neg=0.75, bias=bias)
    s = rng.normal(size=m)
    # a mixed active set
    _check_objective(capi, ctx, x, n_pos, rng.normal(size=m) / np.sqrt(m), s, **kw)
    # the full active set: every z_i = 0
    f, g, hs = _check_objective(capi, ctx, x, n_pos, np.zeros(m), s, **kw)
    # the empty one: rows y_i u with w a large multiple of u, so that every z_i > 1; g = w and Hs = s exactly
    u = np.sign(rng.normal(size=d)).astype(np.float32)
    xs = np.concatenate([np.ones(n_pos), -np.ones(n_neg)]).astype(np.float32)[:, None] * u[None, :]
    w = np.zeros(m)
    w[:d] = 4.0 * u
    f, g, hs = capi.liblinear_objective(ctx, xs, n_pos, w, s, **kw)
    assert np.array_equal(g, w) and np.array_equal(hs, s)
    assert abs(f - 0.5 * w @ w) <= M.bounds(xs, n_pos, n_neg, w, **kw)[0]


@pytest.mark.parametrize("bias", [False, True])
def test_a_row_on_the_margin_is_inactive(capi, ctx, form, bias):
    """row t is e_0 with label +1, no other row has anything in coordinate 0, w_0 = 1 (and no bias weight): z_t = 1 exactly in
    double, so the row is outside grad's set (z < 1) and adds nothing to fun (1 - z > 0)"""
    n_pos, n_neg, d = 40, 90, 39
    x = np.array(L.case("bias39")[0])
    x[:, 0] = 0
    t = 17
    x[t] = 0
    x[t, 0] = 1
    m = d + int(bias)
    rng = np.random.default_rng(3)
    w = rng.normal(size=m) / 8
    w[0] = 1.0
    if bias:
        w[-1] = 0.0
    s = rng.normal(size=m)
    f, g, hs = _check_objective(capi, ctx, x, n_pos, w, s, bias=bias)
    # the same problem without the row, its coordinate kept: the sums must not change by a bit of the row's making
    keep = np.arange(n_pos + n_neg) != t
    f2, g2, hs2 = M.evaluate(x[keep], n_pos - 1, n_neg, w, s, bias=bias)
    bf, bg, bh = M.bounds(x[keep], n_pos - 1, n_neg, w, s, bias=bias)
    assert abs(f - f2) <= bf and np.all(np.abs(g - g2) <= bg) and np.all(np.abs(hs - hs2) <= bh)
    assert g[0] == w[0] and hs[0] == s[0]   # coordinate 0 sees no active row at all


# ---- 3. training at the reference's eps ----

def _train(capi, ctx, name, **kw):
    x, n_pos, n_neg, c, bias = L.case(name)
    return capi.liblinear_train(ctx, x, n_pos, C=c, bias=bias, **kw)


@pytest.mark.parametrize("name", L.all_names())
def test_training_takes_the_model_s_path(capi, ctx, form, name):
    x, n_pos, n_neg, c, bias = L.case(name)
    m = L.model(name)
    assert m["margin"] >= 1e-6, "the case does not license a step-for-step comparison"
    weights, b, w, trace, info = _train(capi, ctx, name)
    print(name, form, info, "model: it %d cg %d margin %.3g |w - w_model|_inf %.3g" % (
        m["iterations"], m["cg_steps"], m["margin"], np.abs(w - m["w"]).max()))
    assert capi.liblinear_train_limits(n_pos, n_neg, x.shape[1], bias)[0] == (form == "single" and x.shape[0] * len(w) <= 40960)
    assert info["iterations"] == m["iterations"] and info["cg_steps"] == m["cg_steps"]
    assert info["trace_len"] == len(m["trace"]) and np.array_equal(trace, m["trace"])
    assert info["converged"] == 1 and info["stop"] == capi.FD_LL_STOP_GRADIENT
    assert info["n_active"] == m["n_active"]
    # gnorm0 at w = 0, objective and gnorm at the returned w: against the float64 evaluation at that very point
    _, g0, _ = M.evaluate(x, n_pos, n_neg, np.zeros_like(w), C=c, bias=bias)
    assert abs(info["gnorm0"] - np.linalg.norm(g0)) <= np.linalg.norm(M.bounds(x, n_pos, n_neg, np.zeros_like(w), C=c, bias=bias)[1])
    f64, g64, _ = M.evaluate(x, n_pos, n_neg, w, C=c, bias=bias)
    bf, bg, _ = M.bounds(x, n_pos, n_neg, w, C=c, bias=bias)
    assert abs(info["objective"] - f64) <= bf
    assert abs(info["gnorm"] - np.linalg.norm(g64)) <= np.linalg.norm(bg)
    d = x.shape[1]
    assert _bits(weights) == _bits(w[:d].astype(np.float32))
    assert np.float32(b).tobytes() == (np.float32(-w[d]) if bias else np.float32(0)).tobytes()
    if name in L.golden_names():
        w_ref = L.golden()[name + "_w"]
        print("against the recorded w of the reference: %.3g |w|_inf" % (np.abs(w - w_ref).max() / np.abs(w_ref).max()))


# ---- 4. the certificate at a tight tolerance ----

def _certify(x, n_pos, n_neg, c, bias, w, info, w_model=None):
    f64, g64, _ = M.evaluate(x, n_pos, n_neg, w, C=c, bias=bias)
    bg = np.linalg.norm(M.bounds(x, n_pos, n_neg, w, C=c, bias=bias)[1])
    gn = np.linalg.norm(g64)
    print("|g64(w_dev)| %.3g <= 1e-6 |g|_0 %.3g + |B| %.3g" % (gn, 1e-6 * info["gnorm0"], bg))
    assert info["converged"] == 1
    assert gn <= 1e-6 * info["gnorm0"] + bg
    if w_model is not None:
        _, gm, _ = M.evaluate(x, n_pos, n_neg, w_model, C=c, bias=bias)
        dist = np.linalg.norm(w - w_model)
        print("|w_dev - w_model| %.3g <= %.3g" % (dist, gn + np.linalg.norm(gm) + bg))
        assert dist <= gn + np.linalg.norm(gm) + bg


@pytest.mark.parametrize("name", [n for n in L.all_names() if n != "wide"])   # (30+30) x 200 with C = 10 is left out
def test_certificate_at_a_tight_tolerance(capi, ctx, form, name):
    x, n_pos, n_neg, c, bias = L.case(name)
    m = L.model(name, 1e-6)
    assert m["converged"] == 1
    weights, b, w, trace, info = _train(capi, ctx, name, solver_tol=1e-6)
    _certify(x, n_pos, n_neg, c, bias, w, info, m["w"])


# ---- 5. stops ----

def test_stops(capi, ctx, form):
    _, _, _, trace, info = _train(capi, ctx, "onepos", max_iterations=1)
    assert (info["iterations"], info["converged"], info["stop"]) == (1, 0, capi.FD_LL_STOP_MAX_ITER)
    _, _, _, trace, info = _train(capi, ctx, "onepos", max_cg_steps=2)
    assert (info["cg_steps"], info["converged"], info["stop"]) == (2, 0, capi.FD_LL_STOP_CG_CAP)
    weights, b, w, trace, info = capi.liblinear_train(ctx, np.zeros((12, 5), np.float32), 5)
    assert info["gnorm0"] == 0 and info["iterations"] == 0 and info["converged"] == 1 and not w.any() and not weights.any() and b == 0
    x = np.array(L.case("bias39")[0])
    x[3, 7] = np.inf
    _, _, _, _, info = capi.liblinear_train(ctx, x, 40, bias=True)
    assert (info["converged"], info["stop"]) == (0, capi.FD_LL_STOP_NONFINITE)
    assert _train(capi, ctx, "tiny")[4]["converged"] == 1   # the context is usable afterwards


# ---- 6. sameness ----

@pytest.mark.parametrize("name", ["c100", "n1280"])
def test_two_calls_and_every_budget_give_the_same_bits(capi, ctx, form, name):
    import torch
    x, n_pos, n_neg, c, bias = L.case(name)
    first = _train(capi, ctx, name)
    assert _same(first, _train(capi, ctx, name))
    assert _same(first, capi.liblinear_train(ctx, torch.from_numpy(np.array(x)).cuda(), n_pos, C=c, bias=bias))
    for steps in (1, 7):
        assert _same(first, _train(capi, ctx, name, launch_steps=steps))


def test_a_batch_equals_its_single_calls(capi, ctx, monkeypatch):
    monkeypatch.delenv("FD_LIBLINEAR_SMALL_ROWS", raising=False)
    for bias in (False, True):
        problems = [(L.make_x(40 + k, p, q, d), p) for k, (p, q, d) in enumerate([(5, 7, 3), (40, 90, 39), (64, 64, 17), (100, 157, 129)])]
        batch = capi.liblinear_train_batch(ctx, problems, C=2.0, bias=bias)
        for (x, p), got in zip(problems, batch):
            assert capi.liblinear_train_limits(p, x.shape[0] - p, x.shape[1], bias)[0]
            weights, b, w, _, info = capi.liblinear_train(ctx, x, p, C=2.0, bias=bias)
            info.pop("trace_len")
            got[3].pop("trace_len")
            assert _bits(got[0]) == _bits(weights) and np.float32(got[1]).tobytes() == np.float32(b).tobytes() and _bits(got[2]) == _bits(w)
            assert got[3] == info


def test_a_batch_takes_the_longest_feature_vector(capi, ctx):
    """d + bias = FD_LIBLINEAR_MAX_D on the single-workgroup kernel, which a single call of this size does not select"""
    n_pos, n_neg, d = 4, 4, 8191
    x = L.make_x(5, n_pos, n_neg, d)
    m = M.tron(x, n_pos, n_neg, bias=True)
    assert m["margin"] >= 1e-6
    (weights, b, w, info), = capi.liblinear_train_batch(ctx, [(x, n_pos)], bias=True)
    assert (info["iterations"], info["cg_steps"], info["converged"], info["n_active"]) == (m["iterations"], m["cg_steps"], 1, m["n_active"])
    f64, g64, _ = M.evaluate(x, n_pos, n_neg, w, bias=True)
    bf, bg, _ = M.bounds(x, n_pos, n_neg, w, bias=True)
    assert abs(info["objective"] - f64) <= bf and abs(info["gnorm"] - np.linalg.norm(g64)) <= np.linalg.norm(bg)
    assert _bits(weights) == _bits(w[:d].astype(np.float32)) and np.float32(b).tobytes() == np.float32(-w[d]).tobytes()


# ---- 7. beyond the dual trainers' limit ----

def test_twenty_thousand_rows(capi, ctx):
    n_pos, n_neg, d = 4000, 16000, 64
    assert n_pos + n_neg > capi.SVM_LARGE_MAX_N
    x = L.make_x(11, n_pos, n_neg, d)
    assert capi.liblinear_train_limits(n_pos, n_neg, d)[:2] == (False, 64)
    weights, b, w, trace, info = capi.liblinear_train(ctx, x, n_pos, solver_tol=1e-6)
    print(info)
    _certify(x, n_pos, n_neg, 1.0, False, w, info, M.tron(x, n_pos, n_neg, solver_tol=1e-6)["w"])


# ---- 8. argument errors ----

def test_argument_errors(capi, ctx):
    x = np.array(L.case("tiny")[0])
    for kw in (dict(C=0.0), dict(C=-1.0), dict(weight_pos=0.0), dict(weight_neg=float("nan")), dict(eps=-1e-3), dict(solver_tol=-1.0),
               dict(max_iterations=-1), dict(max_cg_steps=-1), dict(launch_steps=-1), dict(bias=2)):
        with pytest.raises(capi.FdError) as e:
            capi.liblinear_train(ctx, x, 5, **kw)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "fd_liblinear_train" in str(e.value), kw
    for n_pos in (0, 12):
        with pytest.raises(capi.FdError) as e:
            capi.liblinear_train(ctx, x, n_pos)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError) as e:
        capi.liblinear_train(ctx, np.zeros((4, 8192), np.float32), 2, bias=True)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "8193" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        capi.liblinear_train_batch(ctx, [(np.zeros((2049, 2), np.float32), 5)])
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "2049" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        capi.liblinear_train_batch(ctx, [])
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError) as e:
        capi.liblinear_objective(ctx, x, 0, np.zeros(3))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    p = capi.liblinear_params()
    info = capi.fd_liblinear_info()
    w = np.zeros(3, np.float32)
    assert capi.lib().fd_liblinear_train(ctx.h, None, 5, 7, 3, 0, p, capi._ptr(w), None, None, None, 0, info) == capi.FD_ERR_INVALID_ARGUMENT
    assert _train(capi, ctx, "tiny")[4]["converged"] == 1
