"""csrc/rvm.hip through its public entry points (capi.Rvm.eval, capi.detect_rvm) against the numpy model of tests/rvm_score_model.py,
on thresholds that make a window leave at EVERY level: inside each pass of k_rvm_pass, on every lane of k_rvm_deep's 64-level blocks and
across the hand-over between two blocks, at the pass boundaries (num_used 2, 3, 6, 7, 16, 17, 80, 81, 144, 145), past both grid-stride
limits, on every u8 load path of rvm_kernel_value<true>, with and without the per-window outputs, on empty and full queues, and on
rows with a NaN or an infinity.  Which kernel runs which level follows from num_used alone (rvm_score_model.PASS_CUTS, DEEP_FROM).

Levels are compared exactly on every row (the model proves every row sure: tests/test_rvm_score_model.py), HIK / linear / polynomial
distances bit for bit, RBF distances against the bound derived in the model's docstring."""
import numpy as np
import pytest

import rvm_score_model as M

pytestmark = pytest.mark.gpu

_RVMS, _PYR = {}, {}


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _handle(capi, ctx, m, key):
    if key not in _RVMS:
        _RVMS[key] = capi.Rvm(ctx, m)
    return _RVMS[key]


def _rvm(capi, ctx, name, nu=None, num_cus=256):
    """the case's model on the device, created once"""
    return _handle(capi, ctx, M.model(name, nu, num_cus), (name, nu, num_cus))


def _compare(m, r, lg, dg, what, rows=slice(None)):
    """levels exact; distances: the model's bits, or for RBF within the model's bound at the row's exit level"""
    level, dist, bound = r.level[rows], r.dist[rows], r.bound[rows]
    assert lg.shape == level.shape and dg.shape == dist.shape, what
    assert r.sure[rows].all(), what   # no row's level may depend on the last bits of an exp
    bad = np.nonzero(lg != level)[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], lg[bad[:5]], level[bad[:5]])
    if m["kernel"] == M.RBF:
        err = np.abs(dg - dist)
        w = int(np.argmax(err / bound))
        print("%s: max err / bound = %.3g (row %d of %d, level %d, err %.3g)" % (what, err[w] / bound[w], w, len(dist), level[w], err[w]))
        assert np.all(err <= bound), (what, w, err[w], bound[w])
    else:
        bad = np.nonzero(dg.view(np.uint64) != dist.view(np.uint64))[0]
        assert len(bad) == 0, (what, len(bad), bad[:5], dg[bad[:5]], dist[bad[:5]])


def _eval_case(capi, ctx, name, nu=None, num_cus=256):
    c, m, r = M.case(name, num_cus), M.model(name, nu, num_cus), M.reference(name, nu, num_cus)
    h = _rvm(capi, ctx, name, nu, num_cus)
    lg, dg = h.eval(c.rows)
    _compare(m, r, lg, dg, "%s num_used=%d" % (name, M.num_used(m)))
    lg2, dg2 = h.eval(c.rows)   # the handle's queues, counters and outputs are reused
    assert lg2.tobytes() == lg.tobytes() and dg2.tobytes() == dg.tobytes(), name
    return c, m, r, h


# ---- f32 rows, every level boundary -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", M.LEVELS_NUM_USED)
@pytest.mark.parametrize("name", M.names("levels-"))
def test_levels(capi, ctx, name, nu):
    """145 filters, an exit at every level: num_used 1 .. 16 end inside or at the end of a pass (16: no deep launch), 17 is a deep block
    with one valid lane, 79 / 80 / 81 end before, at and one lane past the first block, 144 / 145 the same for the second"""
    _eval_case(capi, ctx, name, nu)


@pytest.mark.parametrize("name", M.names("wrap-"))
def test_grid_stride_loops_wrap(capi, ctx, num_cus, name):
    c, m, r, _ = _eval_case(capi, ctx, name, None, num_cus)
    assert len(c.rows) > M.pass_rows_to_wrap(num_cus), "k_rvm_pass must walk its grid-stride loop twice"
    assert r.reached[M.DEEP_FROM] > M.deep_rows_to_wrap(num_cus), "k_rvm_deep must walk its grid-stride loop twice"


# ---- u8 windows through the detector ----------------------------------------------------------------------------------------------------
def _pyramid(capi, ctx):
    """the one-layer pyramid at scale 1 of the model's image; gray in, so layer 0 is a copy"""
    if "p" not in _PYR:
        p = capi.Pyramid(ctx, octave_layers=1, min_scale=1.0, max_scale=1.0)
        p.update(M.image())
        info = p.layers()
        assert len(info) == 1 and info[0]["scale"] == 1.0 and (info[0]["w"], info[0]["h"]) == (M.IMAGE_W, M.IMAGE_H)
        _PYR["p"], _PYR["layer"] = p, p.layer(0)
    return _PYR["p"], _PYR["layer"]


def _detect(capi, ctx, pyr, layer, h, m, r, c, what):
    pw, ph = c.pw, c.ph
    wins = pyr.windows(pw, ph, 1, 1)
    assert np.array_equal(wins[:, 0], np.zeros(len(wins), np.int32)) and np.array_equal(wins[:, 1:3], c.origins)
    gray = c.gray if hasattr(c, "gray") else c.patches
    got = np.stack([layer[ly:ly + ph, lx:lx + pw].reshape(-1) for _, lx, ly, *_ in wins])
    assert np.array_equal(got, gray), "the window bytes of the device pyramid are the case's"
    kw = dict(feature_space=c.space, conv_scale=c.conv[0], conv_shift=c.conv[1], sx=1, sy=1)
    dets, lg, dg = capi.detect_rvm(ctx, pyr, h, **kw)
    _compare(m, r, lg, dg, what)
    pos = np.nonzero(r.positive)[0]
    assert len(dets) == len(pos) >= 2, (what, len(dets), len(pos))
    geometry = np.stack([dets[f] for f in ("layer", "lx", "ly", "cx", "cy", "w", "h")], 1)
    assert np.array_equal(geometry, wins[pos]), what            # exactly the model's positives, in window order
    assert np.all(dets["level"] == M.num_used(m) - 1)
    assert np.all(np.abs(dets["probability"] - M.probability(m, r.dist[pos])) <= 1e-12), what
    dets = dets.copy()
    d2, l2, dd2 = capi.detect_rvm(ctx, pyr, h, want_all=False, **kw)   # null all_level / all_dist in both kernels
    assert l2 is None and dd2 is None and d2.tobytes() == dets.tobytes(), what
    with pytest.raises(capi.FdError) as e:
        capi.detect_rvm(ctx, pyr, h, cap=len(pos) - 1, **kw)
    assert e.value.code == capi.FD_ERR_CAPACITY, e.value
    d3, l3, dd3 = capi.detect_rvm(ctx, pyr, h, **kw)
    assert d3.tobytes() == dets.tobytes() and l3.tobytes() == lg.tobytes() and dd3.tobytes() == dg.tobytes(), what
    return dets


@pytest.mark.parametrize("name", M.names("u8-") + ["bench-shape"])
def test_u8_windows(capi, ctx, name):
    """gray patches of 2x2 .. 32x32 (one dword; one, two and nine 16-byte chunks; nine dwords; bytes only; the LDS slab full) under each
    kernel's conversion, and the benchmark's shape (20x20 hq64, 100 filters, conv_scale 1/255)"""
    c, m, r = M.case(name), M.model(name), M.reference(name)
    pyr, layer = _pyramid(capi, ctx)
    _detect(capi, ctx, pyr, layer, _rvm(capi, ctx, name), m, r, c, name)


# ---- degenerate queues ------------------------------------------------------------------------------------------------------------------
def test_every_row_leaves_at_level_0(capi, ctx):
    """thresholds +inf: the three later passes and the deep kernel see an empty queue"""
    name = "levels-rbf"
    m, r = M.with_thresholds(name, np.inf)
    assert np.all(r.level == 0) and not r.positive.any()
    h = _handle(capi, ctx, m, (name, "+inf"))
    lg, dg = h.eval(M.case(name).rows)
    _compare(m, r, lg, dg, name + " thresholds +inf")


def test_every_row_reaches_the_last_level(capi, ctx):
    """thresholds -1e30: every queue is full, and in the detector every window is a positive (the positives' buffer is filled to its
    last slot)"""
    name = "levels-rbf"
    m, r = M.with_thresholds(name, -1e30)
    assert np.all(r.level == 144) and r.positive.all()
    h = _handle(capi, ctx, m, (name, "-1e30"))
    lg, dg = h.eval(M.case(name).rows)
    _compare(m, r, lg, dg, name + " thresholds -1e30")
    pyr, layer = _pyramid(capi, ctx)
    patches = M.window_patches(M.image(), 6, 6)
    c = M.types.SimpleNamespace(pw=6, ph=6, patches=patches, origins=M.window_origins(6, 6), space=M.FEATURE_GRAY, conv=(1.0 / 255.0, 0.0))
    rw = M.evaluate(m, M.convert(patches, *c.conv))
    assert rw.positive.all()
    dets = _detect(capi, ctx, pyr, layer, h, m, rw, c, name + " thresholds -1e30, detector")
    assert len(dets) == len(patches) == pyr.window_count(6, 6, 1, 1)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_few_rows(capi, ctx, n):
    """one lane, a wavefront less one, a wavefront and one, a workgroup and one"""
    name = "levels-rbf"
    m, r = M.model(name), M.reference(name)
    lg, dg = _rvm(capi, ctx, name).eval(M.case(name).rows[:n])
    _compare(m, r, lg, dg, "%s n=%d" % (name, n), rows=slice(0, n))


# ---- NaN and infinities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.names("nonfinite-"))
def test_nonfinite_rows(capi, ctx, name):
    """std::min(x, s) keeps a NaN of x (HistogramIntersectionKernel.hpp:88-92); with fminf the NaN disappeared on the device and the window
    went on through the cascade, where the reference leaves at level 0 with a NaN distance"""
    c, m, r = M.case(name), M.model(name), M.reference(name)
    lg, dg = _rvm(capi, ctx, name).eval(c.rows)
    assert np.array_equal(lg, r.level), (name, np.nonzero(lg != r.level)[0][:5])
    assert np.array_equal(dg, r.dist, equal_nan=True), name


# ---- the length limit -------------------------------------------------------------------------------------------------------------------
def test_length_limit(capi, ctx):
    """k_rvm_deep keeps a window's vector in LDS (1024 floats); k_rvm_pass has no such limit.  33 * 32 elements run with 16 levels and are
    refused, before anything is queued, with 17"""
    name = "limit-rbf"
    c = M.case(name)
    assert c.rows.shape[1] == 33 * 32 > M.MAX_PATCH ** 2
    _, m, r, h = _eval_case(capi, ctx, name, 16)
    h17 = _rvm(capi, ctx, name, 17)
    with pytest.raises(capi.FdError) as e:
        h17.eval(c.rows)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "1024" in str(e.value), e.value
    lg, dg = h.eval(c.rows)
    _compare(m, r, lg, dg, name + " after the refusal")


def test_models_leave_the_device():
    """not a check: the module's cached handles give their device memory back"""
    for h in _RVMS.values():
        h.close()
    _RVMS.clear()
    if "p" in _PYR:
        _PYR["p"].close()
    _PYR.clear()
