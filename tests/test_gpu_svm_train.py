"""Linear C-SVC training on the device (fd_linear_svm_gram / _train / _train_batch, fd_ehog_tracker_train_svm) against
tests/svm_train_model.py, the float64 restatement of libsvm that tests/test_svm_train_model.py pins to libsvm itself.

The cases are the smallest shapes at which the kernels can still go wrong (svm_train_model.case_x):
  a  1 + 1 x 13      one iteration, both alpha at the bound
  b  5 + 18 x 117    n not a tile multiple, d = 1 (mod 4); C = 0.01 / 1 / 100, weights 1 : 1 and 18/5 : 5/18
  c  b with duplicated rows of either class (quad_coef = 0 -> TAU)
  d  20 + 100 x 455  the tracker's shape, Q in LDS
  e  20 + 180 x 52   Q in memory, one element per thread
  f  30 + 290 x 39   more than one element per thread
"""
import os

import numpy as np
import pytest

import svm_train_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-4
_cache = {}


def _problem(name):
    """x, n_pos, n_neg and the float64 Gram of a case -- computed once"""
    if ("x", name) not in _cache:
        x, n_pos, n_neg = M.case_x(name)
        _cache[("x", name)] = (x, n_pos, n_neg, M.gram64(x))
    return _cache[("x", name)]


def _device_gram(capi, ctx, name):
    if ("q", name) not in _cache:
        x, n_pos, _, _ = _problem(name)
        _cache[("q", name)] = capi.linear_svm_gram(ctx, x, n_pos)
    return _cache[("q", name)]


def _model_on_device_q(capi, ctx, case, max_iterations=0):
    """the model run on the Q the device returned"""
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
    return capi.linear_svm_train(ctx, x, n_pos, C=c, weight_pos=wp, weight_neg=wn, **kw)


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


# ---------------- Gram ----------------
@pytest.mark.parametrize("name", list("abcdef"))
def test_gram(capi, ctx, name):
    """Q within one float ulp of float32(float64 Gram), QD within 4 d double ulp: a reordered f64 sum before one rounding"""
    x, n_pos, n_neg, k = _problem(name)
    q, qd = _device_gram(capi, ctx, name)
    want_q, want_qd = M.q_from_gram(k, n_pos)
    dq = np.abs(q.astype(np.float64) - want_q.astype(np.float64))
    print("gram %s: max |dQ| / ulp = %g, max |dQD| / ulp = %g" % (name, (dq / np.spacing(np.abs(want_q)).astype(np.float64)).max(),
                                                                 (np.abs(qd - want_qd) / np.spacing(want_qd)).max()))
    assert (dq <= np.spacing(np.abs(want_q)).astype(np.float64)).all()
    assert (np.abs(qd - want_qd) <= 4 * x.shape[1] * np.spacing(want_qd)).all()
    assert np.array_equal(q, q.T)   # libsvm reads rows of a symmetric Q


# ---------------- solver: the model's bits ----------------
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_solver_equals_model_bit_for_bit(capi, ctx, case):
    want = _model_on_device_q(capi, ctx, case)
    got = _device_train(capi, ctx, case)
    assert want["converged"] == 1 and got[3]["launches"] == 1
    _assert_same_bits(got, want)


def test_q_placement_of_the_cases(capi):
    """d runs with Q in LDS, e and f read it from memory; f has more than one element per thread"""
    assert capi.linear_svm_train_limits(20, 100, 455)[0]
    assert not capi.linear_svm_train_limits(20, 180, 52)[0] and not capi.linear_svm_train_limits(30, 290, 39)[0]


# ---------------- independent of the model ----------------
def _libsvm_alpha(case):
    """libsvm's recorded alpha (tests/golden/make_svm_train_golden.py): with X for the small cases, alpha alone for d..f, whose X
    the seeded generator reproduces (pinned by its sum)"""
    name, (c, wp, wn) = case
    if name in "abc":
        g = np.load(os.path.join(GOLDEN, "svm_train_%s.npz" % name))
        return g["alpha"][M.params_of(name).index((c, wp, wn))]
    g = np.load(os.path.join(GOLDEN, "svm_train_def.npz"))
    assert (c, wp, wn) == (1.0, 1.0, 1.0) and float(g["xsum_" + name]) == float(_problem(name)[0].astype(np.float64).sum())
    return g["alpha_" + name]


def _rho64(alpha, G, y, Cs):
    free = (alpha > 0) & (alpha < Cs)
    if free.any():
        return float((y * G)[free].mean())
    up = ((y > 0) & (alpha < Cs)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < Cs))
    return float((-(-y * G)[up].max() - (-y * G)[low].min()) / 2)


def _gap(x64, y, Cs, alpha, w, rho):
    """duality gap of (w, rho) and alpha in float64: primal - dual >= 0, and 1/2 |w - w*|^2 <= primal - primal* <= gap"""
    margins = y * (x64 @ w - rho)
    primal = 0.5 * float(w @ w) + float((Cs * np.maximum(0.0, 1.0 - margins)).sum())
    v = (alpha * y) @ x64
    dual = float(alpha.sum()) - 0.5 * float(v @ v)
    return primal - dual


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_solution_is_optimal_and_near_libsvm(capi, ctx, oracle, case):
    """With G recomputed in float64 from the returned alpha and the exact Gram: m(alpha) - M(alpha) < eps + s, rho between -m and
    -M up to s (s = n C_max 2^-24 max|K|, the effect of rounding Q to float), and |w - w_libsvm| <= sqrt(2 gap) + sqrt(2 gap_libsvm)
    (strong convexity of the primal).  The rho interval is [min(-m, -M) - s, max(-m, -M) + s]: without a free alpha and without
    any violating pair m < M, calculate_rho returns the midpoint (-m - M) / 2 and the interval's ends swap (case a)."""
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
    print("%s: m - M = %g, eps + s = %g, rho = %r in [%r, %r]" % (M.case_id(case), m - Mm, EPS + s, info["rho"], -m, -Mm))
    assert m - Mm < EPS + s
    assert min(-m, -Mm) - s <= info["rho"] <= max(-m, -Mm) + s
    x64 = x.astype(np.float64)
    a_ref = _libsvm_alpha(case)
    w_ref = (a_ref * y) @ x64
    G_ref = (np.outer(y, y) * k) @ a_ref - 1.0
    gap_ref = _gap(x64, y, Cs, a_ref, w_ref, _rho64(a_ref, G_ref, y, Cs))
    gap = _gap(x64, y, Cs, alpha, w.astype(np.float64), info["rho"])
    dist = float(np.linalg.norm(w.astype(np.float64) - w_ref))
    print("   |w - w_libsvm| = %g, gaps %g %g" % (dist, gap, gap_ref))
    assert gap >= -1e-9 * max(1.0, abs(info["objective"])) and gap_ref >= -1e-9 * max(1.0, abs(info["objective"]))
    assert dist <= np.sqrt(2 * max(gap, 0.0)) + np.sqrt(2 * max(gap_ref, 0.0))


# ---------------- relaunch ----------------
@pytest.mark.parametrize("case", [("b", (1.0, 1.0, 1.0)), ("d", (1.0, 1.0, 1.0)), ("f", (1.0, 1.0, 1.0))], ids=M.case_id)
def test_relaunch_gives_the_same_bits(capi, ctx, case):
    want = _model_on_device_q(capi, ctx, case)
    got = _device_train(capi, ctx, case, launch_iterations=7)
    assert got[3]["launches"] == want["iterations"] // 7 + 1 > 1
    _assert_same_bits(got, want)


def test_max_iterations_is_not_an_error(capi, ctx):
    case = ("d", (1.0, 1.0, 1.0))
    want = _model_on_device_q(capi, ctx, case, max_iterations=5)
    assert want["iterations"] == 5 and want["converged"] == 0
    got = _device_train(capi, ctx, case, max_iterations=5)   # FD_OK: no FdError
    _assert_same_bits(got, want)
    got = _device_train(capi, ctx, case, max_iterations=5, launch_iterations=2)
    assert got[3]["launches"] == 3
    _assert_same_bits(got, want)


# ---------------- batch ----------------
def test_batch_equals_single_calls(capi, ctx):
    """a..f in one call: one workgroup per problem, Q in LDS and in memory side by side"""
    cases = [(name, (1.0, 1.0, 1.0)) for name in "abcdef"]
    got = capi.linear_svm_train_batch(ctx, [(_problem(name)[0], _problem(name)[1]) for name, _ in cases])
    assert len(got) == len(cases)
    for case, g in zip(cases, got):
        _assert_same_bits(g, _model_on_device_q(capi, ctx, case))
    # weighted, with relaunches: every problem keeps iterating until the last one is done
    p = (1.0, 18.0 / 5.0, 5.0 / 18.0)
    got = capi.linear_svm_train_batch(ctx, [(_problem(name)[0], _problem(name)[1]) for name in "cbf"], C=p[0], weight_pos=p[1], weight_neg=p[2],
                                      launch_iterations=16)
    for name, g in zip("cb", got):
        _assert_same_bits(g, _model_on_device_q(capi, ctx, (name, p)))
    single = capi.linear_svm_train(ctx, _problem("f")[0], _problem("f")[1], C=p[0], weight_pos=p[1], weight_neg=p[2])
    assert _bits(got[2][2]) == _bits(single[2]) and _bits(got[2][0]) == _bits(single[0]) and got[2][3]["iterations"] == single[3]["iterations"]
    assert got[2][3]["launches"] == single[3]["iterations"] // 16 + 1


# ---------------- argument errors ----------------
@pytest.mark.parametrize("n_pos,n_rows,kw", [
    (0, 6, {}), (6, 6, {}), (3, 1030, {}),
    (3, 6, {"C": 0.0}), (3, 6, {"C": -1.0}), (3, 6, {"weight_pos": 0.0}), (3, 6, {"weight_neg": -2.0}), (3, 6, {"eps": -1e-3}),
    (3, 6, {"max_iterations": -1}), (3, 6, {"launch_iterations": -1}), (3, 6, {"C": float("nan")})])
def test_invalid_arguments(capi, ctx, n_pos, n_rows, kw):
    x = np.ones((n_rows, 5), np.float32)
    with pytest.raises(capi.FdError) as e:
        capi.linear_svm_train(ctx, x, n_pos, **kw)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and len(str(e.value)) > len("fd_hip error 1: ")
    if not kw:
        with pytest.raises(capi.FdError) as e:
            capi.linear_svm_gram(ctx, x, n_pos)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
        with pytest.raises(capi.FdError) as e:
            capi.linear_svm_train_batch(ctx, [(np.ones((4, 5), np.float32), 2), (x, n_pos)])
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_null_pointers_and_empty_feature(capi, ctx):
    import ctypes as C
    L = capi.lib()
    x = np.ones((6, 5), np.float32)
    w, q, qd = np.zeros(5, np.float32), np.zeros((6, 6), np.float32), np.zeros(6)
    bias, info, prm = C.c_float(), capi.fd_svm_train_info(), capi.svm_train_params()
    P = capi._ptr
    calls = [lambda: L.fd_linear_svm_train(ctx.h, None, 3, 3, 5, 0, C.byref(prm), P(w), C.byref(bias), None, C.byref(info)),
             lambda: L.fd_linear_svm_train(ctx.h, P(x), 3, 3, 5, 0, None, P(w), C.byref(bias), None, C.byref(info)),
             lambda: L.fd_linear_svm_train(ctx.h, P(x), 3, 3, 5, 0, C.byref(prm), None, C.byref(bias), None, C.byref(info)),
             lambda: L.fd_linear_svm_train(ctx.h, P(x), 3, 3, 5, 0, C.byref(prm), P(w), None, None, C.byref(info)),
             lambda: L.fd_linear_svm_train(ctx.h, P(x), 3, 3, 5, 0, C.byref(prm), P(w), C.byref(bias), None, None),
             lambda: L.fd_linear_svm_train(ctx.h, P(x), 3, 3, 0, 0, C.byref(prm), P(w), C.byref(bias), None, C.byref(info)),
             lambda: L.fd_linear_svm_gram(ctx.h, P(x), 3, 3, 5, 0, None, P(qd)),
             lambda: L.fd_linear_svm_gram(ctx.h, P(x), 3, 3, 5, 0, P(q), None),
             lambda: L.fd_linear_svm_train_batch(ctx.h, 1, None, C.byref(prm), C.byref(info)),
             lambda: L.fd_linear_svm_train_batch(ctx.h, 0, None, C.byref(prm), C.byref(info))]
    for i, call in enumerate(calls):
        assert call() == capi.FD_ERR_INVALID_ARGUMENT, i
        assert L.fd_last_error(ctx.h), i
    # alpha is optional
    assert L.fd_linear_svm_train(ctx.h, P(x + np.arange(6, dtype=np.float32)[:, None]), 3, 3, 5, 0, C.byref(prm), P(w), C.byref(bias), None,
                                 C.byref(info)) == capi.FD_OK


# ---------------- tracker ----------------
TW, TH, TCELL = 160, 120, 4
TCOLS, TROWS = 5, 7


@pytest.fixture(scope="module")
def tracker_scene(capi, ctx, synth):
    fp = capi.cehog_params(cell_size=TCELL, bin_count=18, signed_gradients=True, unsigned_gradients=True, interpolate_bins=False,
                           interpolate_cells=True, alpha=0.2)
    prm = capi.ehog_tracker_params(fp, TCOLS, TROWS, 2, TCOLS * TCELL, 100)
    frame = synth.make_frame(TW, TH, seed=41)
    trackers = [capi.EhogTracker(ctx, prm) for _ in range(2)]
    for t in trackers:
        t.update(frame)
    # the target's patch and 12 windows around it
    rng = np.random.default_rng(7)
    target = (80, 60, 40, 56)
    boxes = [target] + [(int(rng.integers(40, 121)), int(rng.integers(45, 76)), int(w), int(w) * TROWS // TCOLS)
                        for w in rng.integers(24, 41, 12)]
    valid, feats = trackers[0].extract_patches(boxes)
    assert valid.all()
    return trackers, feats.reshape(len(boxes), -1), boxes


def test_tracker_train_svm_equals_set_svm(capi, ctx, tracker_scene):
    (trained, given), x, boxes = tracker_scene
    assert x.shape == (13, TROWS * TCOLS * 31)
    w, bias, alpha, info = capi.linear_svm_train(ctx, x, 1)
    tinfo = trained.train_svm(x, 1)
    assert tinfo == info and info["converged"] == 1 and info["n_sv"] >= 2
    tw, tb = trained.get_svm()   # the handle's host copy of what the kernel wrote into its device weights
    assert _bits(tw.reshape(-1)) == _bits(w) and _bits(np.float32(tb)) == _bits(np.float32(bias))
    given.set_svm(w.reshape(TROWS, TCOLS, -1), bias)
    assert len(trained.layers()) >= 3
    for li in range(len(trained.layers())):
        a, b = trained.heat_layer(li), given.heat_layer(li)
        assert a.shape == b.shape and _bits(a) == _bits(b), li
    samples = boxes + [(40, 40, 30, 42), (100, 70, 55, 77), (5, 5, 20, 28)]
    va, sa = trained.evaluate_samples(samples)
    vb, sb = given.evaluate_samples(samples)
    assert np.array_equal(va, vb) and va.any() and _bits(sa) == _bits(sb)
    # the handle's host copy was refreshed: the patch scores (decision values in double) agree as well
    _, _, pa = trained.extract_patches(boxes, want_score=True)
    _, _, pb = given.extract_patches(boxes, want_score=True)
    assert _bits(pa) == _bits(pb) and pa[0] > 0 and (pa[1:] < 0).sum() >= 10


def test_tracker_train_svm_checks_its_arguments(capi, ctx, tracker_scene):
    (trained, _), x, _ = tracker_scene
    with pytest.raises(capi.FdError) as e:
        trained.train_svm(x, len(x))   # no negative
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        trained.train_svm(x[:, :-1], 1)
