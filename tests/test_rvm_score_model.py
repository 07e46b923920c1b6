"""The numpy model of the RVM cascade (tests/rvm_score_model.py) on every case tests/test_gpu_rvm_score.py runs, without a GPU: the
calibration leaves what each case is there for (an exit at every level, positives and negatives at the last one, enough rows past the
grid-stride limits, every row sure), and the CPU oracle, an independent restatement of the same specification, gives the model's levels
on every row, its distance bits for the kernels without a libm call and distances inside the derived bound for RBF."""
import numpy as np
import pytest

import rvm_score_model as M

CUS = 256
CASES = M.names("levels-") + M.names("wrap-") + M.names("u8-") + ["bench-shape", "limit-rbf"]


def _runs():
    out = []
    for name in CASES:
        nus = M.LEVELS_NUM_USED if name.startswith("levels-") else (16, 17) if name == "limit-rbf" else (None,)
        out += [(name, nu) for nu in nus]
    return out


def _id(v):
    return "all" if v is None else str(v)


@pytest.mark.parametrize("name,nu", _runs(), ids=_id)
def test_calibration_conditions(name, nu):
    c, m, r = M.case(name, CUS), M.model(name, nu, CUS), M.reference(name, nu, CUS)
    used = M.num_used(m)
    assert used == (max(c.num_useds) if nu is None else nu)
    assert np.all(np.isfinite(r.dist))
    unsure = np.nonzero(~r.sure)[0]
    print("%s num_used=%d: smallest margin %.3g, largest bound %.3g, %d positives, %d rows at the last level" %
          (name, used, r.margin.min() if used > 1 else np.inf, r.bound.max(), r.positive.sum(), (r.level == used - 1).sum()))
    assert len(unsure) == 0, (name, used, unsure[:5], r.margin[unsure[:5]], r.bound[unsure[:5]])
    exits = np.bincount(r.level, minlength=used)
    assert len(exits) == used and np.all(exits >= 1), (name, used, np.nonzero(exits == 0)[0])
    last = r.level == used - 1
    assert r.positive.sum() >= 1 and (last & ~r.positive).sum() >= 1, (name, used)
    if m["kernel"] == M.RBF:
        assert np.all(r.bound > 0) and r.bound.max() < 1e-10
    else:
        assert not r.bound.any()
    if name.startswith("levels-") and used > M.DEEP_FROM:
        assert r.reached[M.DEEP_FROM] > 1000          # the deep kernel sees thousands of windows, and an exit on every lane
        if used > M.DEEP_FROM + 64:
            assert r.reached[M.DEEP_FROM + 64] >= 64  # ... and its second block more than a workgroup's worth
    if name.startswith("wrap-"):
        assert len(c.rows) > M.pass_rows_to_wrap(CUS) and r.reached[M.DEEP_FROM] > M.deep_rows_to_wrap(CUS)


@pytest.mark.parametrize("name,nu", _runs(), ids=_id)
def test_oracle_agrees_with_the_model(oracle, name, nu):
    c, m, r = M.case(name, CUS), M.model(name, nu, CUS), M.reference(name, nu, CUS)
    ro = oracle.Rvm(m)
    lo, do = ro.eval(c.rows)
    ro.close()
    assert np.array_equal(lo, r.level), (name, nu, np.nonzero(lo != r.level)[0][:5])
    if m["kernel"] == M.RBF:
        err = np.abs(do - r.dist)
        w = int(np.argmax(err / r.bound))
        print("%s num_used=%s: max |oracle - model| / bound = %.3g (row %d)" % (name, nu, err[w] / r.bound[w], w))
        assert np.all(err <= r.bound), (name, nu, w, err[w], r.bound[w])
    else:
        assert do.tobytes() == r.dist.tobytes(), (name, nu, np.nonzero(do != r.dist)[0][:5])


def test_evaluate_is_the_cached_path():
    """the cases' shared tables and the plain entry point are one model"""
    for name in ("levels-rbf", "u8-5x5-hik", "u8-6x6-poly"):
        c = M.case(name)
        for nu in (c.num_useds[0], c.num_useds[-1]):
            m, r = M.model(name, nu), M.reference(name, nu)
            e = M.evaluate(m, c.rows[:500])
            assert np.array_equal(e.level, r.level[:500]) and e.dist.tobytes() == r.dist[:500].tobytes()
            assert np.array_equal(e.bound, r.bound[:500]) and np.array_equal(e.sure, r.sure[:500])
            assert np.array_equal(M.calibrate(m, c.rows, c.pass_rate), m["thresholds"])


def test_model_against_a_scalar_restatement():
    """kernel_values() and distances() on a few rows of every kernel against python loops over numpy scalars"""
    for name in ("u8-5x5-rbf", "u8-5x5-hik", "u8-5x5-linear", "u8-5x5-poly"):
        c, m = M.case(name), M.model(name)
        K = M.kernel_values(m, c.rows[:3], 4)
        D = M.distances(m, K)
        co = np.asarray(m["coeff"], np.float32)
        for r in range(3):
            d = None
            for k in range(4):
                x, s = c.rows[r], m["sv"][k]
                if m["kernel"] == M.RBF:
                    acc = np.float32(0)
                    for a, b in zip(x, s):
                        diff = np.float32(a - b)
                        acc = np.float32(acc + np.float32(diff * diff))
                    kv = np.exp(-np.float64(m["p0"]) * np.float64(acc))
                elif m["kernel"] == M.HIK:
                    acc = np.float32(0)
                    for a, b in zip(x, s):
                        acc = np.float32(acc + min(a, b))
                    kv = np.float64(acc)
                else:
                    kv = np.float64(0)
                    for a, b in zip(x, s):
                        kv = kv + np.float64(a) * np.float64(b)
                    if m["kernel"] == M.POLY:
                        base = np.float64(m["p0"]) * kv + np.float64(m["p1"])
                        assert m["p2"] == 3
                        # degree 3 by square-and-multiply: ret = 1 * base, tmp = base^2, ret = base * base^2
                        kv = (np.float64(1.0) * base) * (base * base)
                assert kv == K[r, k], (name, r, k)
                term = np.float64(co[k * (k + 1) // 2 + k]) * kv
                d = -np.float64(np.float32(m["bias"])) + term if k == 0 else d + term
                assert d == D[r, k], (name, r, k)


def test_bound_is_the_derived_one():
    c, m = M.case("levels-rbf"), M.model("levels-rbf")
    K = M.kernel_values(m, c.rows[:5], 3)
    B = M.bounds(m, K)
    cd = np.abs(M.diag(m))
    A2 = abs(np.float64(np.float32(0.1))) + cd[0] * K[:, 0] + cd[1] * K[:, 1] + cd[2] * K[:, 2]
    assert np.allclose(B[:, 2], 7 * 2.0 ** -52 * A2, rtol=1e-15)
    assert [M.u8_load_path(pw * ph) for pw, ph in M.U8_PATCHES] == ["dword", "chunk16", "chunk16", "chunk16", "dword", "scalar", "scalar", "chunk16"]
    assert M.pass_rows_to_wrap(256) + 77 == 524365 and M.deep_rows_to_wrap(256) == 8192


def test_fp32_chain_is_inside_the_summation_bound_of_the_fp64_specification():
    """the model's fp32 sum of squared differences, its exp and the running sum against a pure-fp64 evaluation of levels-rbf: inside the
    sequential-summation bound gamma_(dim+2) carried through exp and the sum (derived in the model's docstring)"""
    c, m = M.case("levels-rbf"), M.model("levels-rbf")
    gap, allowed = M.spec_gap(m, c.rows[:1500])
    w = np.unravel_index(np.argmax(gap / allowed), gap.shape)
    print("levels-rbf: max |fp32 chain - fp64| / bound = %.3g at row %d level %d (gap %.3g)" % (gap[w] / allowed[w], w[0], w[1], gap[w]))
    assert gap.max() > 0 and np.all(gap <= allowed)
    assert allowed.max() < 1e-3   # the bound says something: far below the distances' spread


def _device_shaped(m, D, mutant=None):
    """(level, dist) by the cascade cut the way csrc/rvm.hip cuts it: levels below DEEP_FROM one after the other, then blocks of 64 levels
    at once with the FIRST leaving level of a block taken.  mutant: a subtly wrong k_rvm_deep -- 'last_lane' takes the last leaving
    level of a block, 'no_handover' starts every block after the first from the distance the queue handed in (d_15) and not from the
    previous block's last distance, 'stale_lane' returns the distance of the block's last valid level and not of the leaving one"""
    nu = M.num_used(m)
    thr = np.asarray(m["thresholds"], np.float32).astype(np.float64)
    n = len(D)
    level, dist, alive = np.full(n, -1, np.int32), np.zeros(n), np.ones(n, bool)
    for k in range(min(M.DEEP_FROM, nu)):
        leaves = alive & ~((D[:, k] >= thr[k]) & (k + 1 < nu))
        level[leaves], dist[leaves] = k, D[leaves, k]
        alive &= ~leaves
    for kb in range(M.DEEP_FROM, nu, 64):
        ks = np.arange(kb, min(kb + 64, nu))
        Db = D[:, ks]
        if mutant == "no_handover" and kb > M.DEEP_FROM:
            Db = Db - (D[:, kb - 1] - D[:, M.DEEP_FROM - 1])[:, None]
        lv = ~((Db >= thr[None, ks]) & (ks + 1 < nu)[None, :])
        e = (len(ks) - 1 - lv[:, ::-1].argmax(1)) if mutant == "last_lane" else lv.argmax(1)
        out = alive & lv.any(1)
        level[out] = kb + e[out]
        dist[out] = Db[out, -1] if mutant == "stale_lane" else Db[out, e[out]]
        alive &= ~out
    assert not alive.any()
    return level, dist


@pytest.mark.parametrize("name", M.names("levels-"))
def test_levels_cases_notice_a_subtly_wrong_deep_kernel(name):
    """against the numpy model only: the blocked evaluation is the model, and each of three wrong block kernels changes a level or a
    distance of the case at the num_used values that put exits inside the first block, at its end, and in the second block"""
    for nu in (17, 79, 80, 81, 145):
        m, r = M.model(name, nu), M.reference(name, nu)
        D = M._tables(name)[1]
        level, dist = _device_shaped(m, D)
        assert np.array_equal(level, r.level) and dist.tobytes() == r.dist.tobytes()
        for mutant in ("last_lane", "stale_lane", "no_handover"):
            lm, dm = _device_shaped(m, D, mutant)
            differs = not np.array_equal(lm, r.level) or dm.tobytes() != r.dist.tobytes()
            # one valid lane in the only block: first == last lane; one block only: no hand-over
            same_by_construction = (nu == 17 and mutant != "no_handover") or (mutant == "no_handover" and nu <= M.DEEP_FROM + 64)
            assert differs != same_by_construction, (name, nu, mutant)


@pytest.mark.parametrize("name", M.names("nonfinite-"))
def test_nonfinite_rows(oracle, name):
    """one NaN, +inf or -inf per row, at the first, a middle and the last element: model and oracle give the same level and distance.
    A NaN makes every kernel value NaN, and the window leaves at level 0"""
    c, m, r = M.case(name), M.model(name), M.reference(name)
    assert M.num_used(m) == M.NONFINITE_NUM_USED and len(c.rows) == M.NONFINITE_ROWS
    assert np.all((~np.isfinite(c.rows)).sum(1) == 1)
    nan_rows = np.isnan(c.rows).any(1)
    assert nan_rows.sum() >= 21 and np.all(r.level[nan_rows] == 0) and np.all(np.isnan(r.dist[nan_rows]))
    ro = oracle.Rvm(m)
    lo, do = ro.eval(c.rows)
    ro.close()
    assert np.array_equal(lo, r.level)
    assert np.array_equal(do, r.dist, equal_nan=True)


def test_bench_shape_features(synth):
    """the hq64 rows of bench-shape are HistEq64Filter's by the oracle and by the vectorised numpy version alike"""
    c = M.case("bench-shape")
    assert np.array_equal(synth.histeq64_np(c.gray.reshape(-1, 20, 20)).reshape(len(c.gray), -1), c.patches)
    assert len(c.rows) == len(c.origins) == (M.IMAGE_W - 20) * (M.IMAGE_H - 20) and len(c.base["sv"]) == 100
    assert np.array_equal(c.gray[-1].reshape(20, 20), M.image()[M.IMAGE_H - 21:M.IMAGE_H - 1, M.IMAGE_W - 21:M.IMAGE_W - 1])
