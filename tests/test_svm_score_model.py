"""The float64 model of SVM scoring (tests/svm_score_model.py) on every case tests/test_gpu_svm_score.py runs, without a GPU:
the CPU oracle stays inside the bounds the kernels are held to (so the reference alone does not use them up), the launchers' limits
restated in the model are what the issue's cases assume, and four subtly wrong kernels, built into the model, break the u8 bound."""
import numpy as np
import pytest

import svm_score_model as M

CASES = M.NAMES + [M.SVS_PERSISTENT]


@pytest.mark.parametrize("name", CASES)
def test_oracle_is_inside_the_bounds_of_the_gpu_test(oracle, name):
    c = M.case(name)
    d, b = M.reference(name)
    do = oracle.Svm(c.m).distance(c.rows)
    ob = M.oracle_bound(c.m, c.rows, c.path)
    err = np.abs(do - d)
    worst = int(np.argmax(err / ob))
    print("%s: max |oracle - model| / bound = %.3g (row %d of %d)" % (name, err[worst] / ob[worst], worst, len(d)))
    assert np.all(np.isfinite(d)) and np.all(b > 0)
    assert np.all(err <= ob), (name, worst, err[worst], ob[worst])


def test_bounds_are_the_table_of_the_issue():
    c = M.case("u8lanes-poly3-d400-s130")
    s = M.scale(c.m, c.rows)
    assert np.array_equal(M.bound(c.m, c.rows, "u8"), (130 + 8 + 6) * 2.0 ** -53 * s)
    c = M.case("f32-poly3-d4099-s3")
    s = M.scale(c.m, c.rows)
    assert np.allclose(M.bound(c.m, c.rows, "generic"), ((65 + 8 + 6) + (3 + 8 + 6)) * 2.0 ** -53 * s, rtol=1e-15)
    c = M.case("f32-hik-d65-s5")
    assert np.array_equal(M.bound(c.m, c.rows, "generic"), (2 + 9) * 2.0 ** -24 * M.scale(c.m, c.rows))
    c = M.case("f32-rbf-d400-s200")
    assert np.array_equal(M.bound(c.m, c.rows, "generic"), np.full(7, (7 + 9) * 2.0 ** -24 * M.coeff_sum(c.m)))
    c = M.case("rbfmfma-d324-s257-n130")
    assert np.array_equal(M.bound(c.m, c.rows, "mfma"), np.full(130, 1e-5 * M.coeff_sum(c.m)))
    # scale: |c| K(|x|, |s|) + |bias|; for non-negative rows and a positive p0, p1 that is the sum of the terms' magnitudes
    c = M.case("f32-poly3-signed-d65-s5")
    x, sv, co = c.rows.astype(np.float64), c.m["sv"].astype(np.float64), c.m["coeff"].astype(np.float64)
    want = (np.abs(co)[None, :] * (0.3 * (np.abs(x) @ np.abs(sv).T) + 0.7) ** 3).sum(1) + 0.25
    assert np.allclose(M.scale(c.m, c.rows), want, rtol=1e-13)


def test_model_against_a_scalar_restatement():
    """distance() on one small case of every kernel and dtype against python loops in exact rational / float arithmetic"""
    from fractions import Fraction
    for name in ("u8mfma-d33-s96-n33", "u8lanes-hik-d17-s65", "u8lanes-linear-d15-s63", "u8lanes-poly2-d17-s65", "f32-linear-signed-d65-s5",
                 "f32-poly3-signed-d65-s5", "f32-hik-d65-s5", "f32-rbf-d65-s5"):
        c = M.case(name)
        d, _ = M.reference(name)
        m = c.m
        for r in (0, len(c.rows) - 1):
            x = [Fraction(float(v)) for v in c.rows[r]]
            total = -Fraction(float(m["bias"]))
            for s, co in zip(m["sv"], m["coeff"]):
                sv = [Fraction(float(v)) for v in s]
                if m["kernel"] == M.RBF:
                    kv = Fraction(float(np.exp(np.longdouble(-m["p0"]) * np.longdouble(float(sum((a - b) ** 2 for a, b in zip(x, sv)))))))
                elif m["kernel"] == M.HIK:
                    kv = sum(min(a, b) for a, b in zip(x, sv))
                else:
                    kv = sum(a * b for a, b in zip(x, sv))
                    if m["kernel"] == M.POLY:
                        kv = (Fraction(m["p0"]) * kv + Fraction(m["p1"])) ** int(m["p2"])
                total += Fraction(float(co)) * kv
            assert abs(float(total) - d[r]) <= 4 * 2.0 ** -53 * M.scale(m, c.rows[r:r + 1])[0], (name, r)


def test_launcher_limits_of_the_model():
    # the issue's cases: 48 k-steps at 1536, the pb that used to be refused, the LDS boundary of the accepted range
    assert M.u8_mfma_lds_bytes(1536, M.u8_mfma_max_nsv(1536)) <= M.LDS_LIMIT < M.u8_mfma_lds_bytes(1536, M.u8_mfma_max_nsv(1536) + 1)
    assert M.u8_mfma_max_nsv(1536) % 32 == 0
    assert M.u8_mfma_available(M.case("u8bound-accepted").m) and not M.u8_mfma_available(M.case("u8bound-refused").m)
    assert not M.u8_mfma_available(M.case("u8lanes-rbf-d1600-s130").m)
    dim, _, n = M.U8_LONG
    assert not M.u8_lanes_fits(dim, 8) and M.u8_lanes_production_pb(dim, n) == 4
    assert [M.u8_lanes_production_pb(48, n) for n in M.U8_THRESHOLD_N] == [2, 4, 4, 8]
    assert M.F32_GENERIC_MAX_DIM == 16384 and M.U8_LANES_MAX_DIM == 32768
    assert M.u8_lanes_fits(M.U8_LANES_MAX_DIM, 2) and not M.u8_lanes_fits(M.U8_LANES_MAX_DIM + 1, 2)
    assert M.rbf_mfma_lds_bytes(600) <= 160 * 1024 < M.rbf_mfma_lds_bytes(M.RBF_MFMA_REFUSED_DIM)
    n = M.svs_persistent_n(256)
    assert n == 16454 and n % 32 != 0
    # 128 workgroups per 256-SV group walk 515 tiles of 32 rows: four or five each, so both buffers of the double buffer end a walk
    tiles, grid = (n + 31) // 32, 256 // 2
    assert sorted({len(range(b, tiles, grid)) for b in range(grid)}) == [4, 5]


MUTANT_ROWS = 40   # a mutant has to show on the first rows or the last one; the large cases need not be scored whole


def _mutant_rows(c):
    return c.rows if len(c.rows) <= MUTANT_ROWS else np.concatenate([c.rows[:MUTANT_ROWS - 1], c.rows[-1:]])


@pytest.mark.parametrize("mutant", M.MUTANTS)
@pytest.mark.parametrize("name", M.U8_NAMES)
def test_u8_bound_rejects_a_subtly_wrong_kernel(name, mutant):
    """Against the numpy model only: a kernel that drops the last byte of ONE support vector, stages a row's pad bytes as the value 0,
    reads the coefficients one index off, or skips the last support vector leaves the u8 bound on at least one row of every u8 case.
    Staging pad bytes as 0 is a different kernel only where the vector is shifted by 128 (the i8 MFMA kernel: 0 becomes -128 against the
    table's absent = 0) AND has pad bytes (dim % 32 != 0); min, the dot product and the unshifted SSD of k_svm_u8_lanes ignore zeros, and
    there the mutant must be the identity."""
    c = M.case(name)
    x = _mutant_rows(c)
    d, b = M.distance(c.m, x), M.bound(c.m, x, "u8")
    dm = M.distance(c.m, x, mutant=mutant)
    if mutant == "pad_as_zero" and not (M.u8_mfma_available(c.m) and c.dim % 32):
        assert np.array_equal(dm, d)
        return
    assert np.any(np.abs(dm - d) > b), (name, mutant, np.max(np.abs(dm - d) / b))
