"""Every kernel body of csrc/svm.hip, by name (fd_debug_svm_launch), against the float64 model of tests/svm_score_model.py at the sizes
where the bodies take another path: padding units, staging branches, prefetch rounds, tails, thresholds between variants, LDS limits.
The bounds are the model's (derived for the u8 and k_svm_generic paths, the project's 1e-5 sum|c| contract for f32 RBF on the matrix
pipe); the CPU oracle is the secondary check, with its own error added.  Next to the bounds: the production launchers give the bits of
the variant they are documented to choose, and variants that promise identical sums give identical bits."""
import os

import numpy as np
import pytest

import svm_score_model as M

pytestmark = pytest.mark.gpu

_SVMS, _ORACLE = {}, {}


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _svm(capi, ctx, name, num_cus=256):
    """the case's model on the device, created once"""
    if (name, num_cus) not in _SVMS:
        _SVMS[name, num_cus] = capi.Svm(ctx, M.case(name, num_cus).m)
    return _SVMS[name, num_cus]


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _written(capi, a):
    return a.view(np.uint64) != np.uint64(capi.SVM_SENTINEL_BITS)


def _check(oracle, name, got, rows=None, num_cus=256, what=""):
    """got against the model (the bound) and against the oracle (the bound + the oracle's own); rows: which of the case's rows got holds"""
    c = M.case(name, num_cus)
    d, b = M.reference(name, num_cus)
    if (name, num_cus) not in _ORACLE:
        _ORACLE[name, num_cus] = (oracle.Svm(c.m).distance(c.rows), M.oracle_bound(c.m, c.rows, c.path))
    do, ob = _ORACLE[name, num_cus]
    rows = slice(None) if rows is None else rows
    d, b, do, ob = d[rows], b[rows], do[rows], ob[rows]
    assert got.shape == d.shape and np.all(np.isfinite(got)), (name, what)
    err = np.abs(got - d)
    w = int(np.argmax(err / b))
    rel = err.max() / M.coeff_sum(c.m)
    print("%s %s: max |kernel - model| = %.3g of the bound (row %d of %d), %.3g sum|c|" % (name, what, err[w] / b[w], w, len(d), rel))
    assert np.all(err <= b), (name, what, w, err[w], b[w])
    assert np.all(np.abs(got - do) <= b + ob), (name, what)
    return rel


def _refused(capi, fn):
    with pytest.raises(capi.FdError) as e:
        fn()
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT, e.value
    return e.value


# ---- u8 RBF on the i8 matrix pipe ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.names("u8mfma-d") + M.names("u8mfma-idx"))
def test_u8_rbf_mfma_both_widths(capi, ctx, oracle, name):
    """byte-wise and word staging (dim % 4, a stride that is no multiple of 4), 1 .. 48 k-steps (three prefetch rounds of the 16-wavefront
    body), 1 .. 3 support-vector tiles, partial workgroups, saturated rows and support vectors, a slot list with repeats"""
    c, s = M.case(name), _svm(capi, ctx, name)
    o8 = capi.svm_launch(ctx, s, c.store, capi.SVM_U8_MFMA_8, idx=c.idx)
    o16 = capi.svm_launch(ctx, s, c.store, capi.SVM_U8_MFMA_16, idx=c.idx)
    prod = capi.svm_launch(ctx, s, c.store, capi.SVM_PRODUCTION, idx=c.idx)
    _check(oracle, name, o8, what="<8>")
    assert _same(o8, o16) and _same(o8, prod)
    if c.idx is None:
        assert _same(o8, s.distance(c.rows))
        assert _same(o8, capi.svm_u8_both(ctx, s, c.rows)[1])


@pytest.mark.parametrize("dcount", M.DCOUNTS)
def test_u8_rbf_mfma_device_count(capi, ctx, oracle, dcount):
    name = "u8mfma-count"
    c, s = M.case(name), _svm(capi, ctx, name)
    n, k = len(c.rows), min(dcount, len(c.rows))
    full = capi.svm_launch(ctx, s, c.store, capi.SVM_U8_MFMA_8)
    for variant in (capi.SVM_U8_MFMA_8, capi.SVM_U8_MFMA_16, capi.SVM_PRODUCTION):   # production with a count: <16> up to 2048 vectors
        out = capi.svm_launch(ctx, s, c.store, variant, dcount=dcount)
        assert np.array_equal(_written(capi, out), np.arange(n) < k), (variant, dcount)
        assert _same(out[:k], full[:k])
    _check(oracle, name, full)
    _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, capi.SVM_U8_LANES_2, dcount=dcount))   # that body reads no count


def test_u8_rbf_mfma_lds_boundary(capi, ctx, oracle):
    """dim = 1536: the largest support-vector count fd_svm_u8_mfma_available accepts runs on the matrix pipe, one more runs RBF in
    k_svm_u8_lanes; both inside the u8 bound"""
    a, r = "u8bound-accepted", "u8bound-refused"
    assert len(M.case(r).m["sv"]) == len(M.case(a).m["sv"]) + 1 == M.u8_mfma_max_nsv(1536) + 1
    ca, sa = M.case(a), _svm(capi, ctx, a)
    o8 = capi.svm_launch(ctx, sa, ca.store, capi.SVM_U8_MFMA_8)
    _check(oracle, a, o8, what="<8>")
    assert _same(o8, capi.svm_launch(ctx, sa, ca.store, capi.SVM_U8_MFMA_16))
    assert _same(o8, capi.svm_launch(ctx, sa, ca.store, capi.SVM_PRODUCTION))
    _check(oracle, a, capi.svm_launch(ctx, sa, ca.store, capi.SVM_U8_LANES_2), what="lanes")
    cr, sr = M.case(r), _svm(capi, ctx, r)
    for variant in (capi.SVM_U8_MFMA_8, capi.SVM_U8_MFMA_16):
        _refused(capi, lambda: capi.svm_launch(ctx, sr, cr.store, variant))
    _refused(capi, lambda: capi.svm_u8_both(ctx, sr, cr.rows))
    _refused(capi, lambda: capi.svm_launch(ctx, sr, cr.store, capi.SVM_PRODUCTION, dcount=5))
    lanes = capi.svm_launch(ctx, sr, cr.store, capi.SVM_U8_LANES_2)
    _check(oracle, r, lanes, what="lanes")
    assert _same(lanes, capi.svm_launch(ctx, sr, cr.store, capi.SVM_PRODUCTION))


# ---- u8, one lane per support vector -------------------------------------------------------------------------------------------------------
LANES = {2: "SVM_U8_LANES_2", 4: "SVM_U8_LANES_4", 8: "SVM_U8_LANES_8"}


@pytest.mark.parametrize("name", M.names("u8lanes-"))
def test_u8_lanes_every_width(capi, ctx, oracle, name):
    """HIK, linear, polynomial and (dim > 1536) RBF; one 16-byte group .. 100, 1 .. 3 passes of 64 support vectors per wavefront quarter;
    full, partial and single-vector workgroups of 2, 4 and 8"""
    c, s = M.case(name), _svm(capi, ctx, name)
    all_rows = {pb: capi.svm_launch(ctx, s, c.store, getattr(capi, v)) for pb, v in LANES.items()}
    _check(oracle, name, all_rows[2], what="pb=2")
    assert _same(all_rows[2], all_rows[4]) and _same(all_rows[2], all_rows[8])   # the arithmetic per vector does not depend on pb
    assert _same(all_rows[2], capi.svm_launch(ctx, s, c.store, capi.SVM_PRODUCTION)) and _same(all_rows[2], s.distance(c.rows))
    for pb, v in LANES.items():
        for n in sorted({1, pb - 1, pb, pb + 1}):
            assert _same(capi.svm_launch(ctx, s, c.store, getattr(capi, v), n=n), all_rows[2][:n]), (pb, n)
    idx = np.array([36, 0, 36, 5, 1], np.uint32)
    assert _same(capi.svm_launch(ctx, s, c.store, capi.SVM_U8_LANES_4, idx=idx), all_rows[2][idx])


@pytest.mark.parametrize("name", M.names("u8thresholds-"))
def test_u8_lanes_production_thresholds(capi, ctx, oracle, name):
    """the launcher takes 4 vectors per workgroup from 8192 and 8 from 16384 vectors: either side of both"""
    c, s = M.case(name), _svm(capi, ctx, name)
    for n in M.U8_THRESHOLD_N:
        pb = M.u8_lanes_production_pb(c.dim, n)
        prod = capi.svm_launch(ctx, s, c.store, capi.SVM_PRODUCTION, n=n)
        assert _same(prod, capi.svm_launch(ctx, s, c.store, getattr(capi, LANES[pb]), n=n)), (n, pb)
        _check(oracle, name, prod, rows=slice(0, n), what="n=%d pb=%d" % (n, pb))


def test_u8_lanes_long_vectors_get_fewer_per_workgroup(capi, ctx, oracle):
    """16384 vectors of 8200 bytes: eight per workgroup do not fit the LDS, four do.  The launcher used to refuse ("feature vector too
    long") what it scores 100 at a time."""
    name = "u8long-hik"
    c, s = M.case(name), _svm(capi, ctx, name)
    assert not M.u8_lanes_fits(c.dim, 8) and M.u8_lanes_production_pb(c.dim, len(c.rows)) == 4
    whole = s.distance(c.rows)
    _check(oracle, name, whole)
    chunks = np.concatenate([s.distance(c.rows[i:i + 100]) for i in range(0, len(c.rows), 100)])
    assert _same(whole, chunks)
    _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, capi.SVM_U8_LANES_8, n=16))
    assert _same(whole[:16], capi.svm_launch(ctx, s, c.store, capi.SVM_U8_LANES_4, n=16))


def test_u8_lanes_lds_boundary(capi, ctx, oracle):
    """two u8 vectors that fill the 64 KiB of dynamic LDS exactly are scored (the kernel's static arrays come on top: the launch limit
    is on the dynamic part, the CU has 160 KiB); the next length gets the library's invalid-argument"""
    name = "u8longest-hik"
    c, s = M.case(name), _svm(capi, ctx, name)
    assert c.dim == M.U8_LANES_MAX_DIM
    out = s.distance(c.rows)
    _check(oracle, name, out)
    assert _same(out, capi.svm_launch(ctx, s, c.store, capi.SVM_U8_LANES_2))
    m = dict(c.m, sv=np.zeros((2, c.dim + 1), np.uint8))
    s1 = capi.Svm(ctx, m)
    x = np.zeros((2, c.dim + 1), np.uint8)
    _refused(capi, lambda: s1.distance(x))
    _refused(capi, lambda: capi.svm_launch(ctx, s1, x, capi.SVM_U8_LANES_2))
    s1.close()


# ---- f32, k_svm_generic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.names("f32-"))
def test_generic_f32(capi, ctx, oracle, name):
    """all four kernels; 1 .. 65 elements per lane pass, 1 .. 50 support vectors per wavefront (fewer support vectors than wavefronts
    included); non-negative rows, signed ones for the kernels that take them"""
    c, s = M.case(name), _svm(capi, ctx, name)
    out = capi.svm_launch(ctx, s, c.store, capi.SVM_GENERIC)
    _check(oracle, name, out)
    assert _same(out, capi.svm_launch(ctx, s, c.store, capi.SVM_PRODUCTION)) and _same(out, s.distance(c.rows))
    assert _same(out[:1], capi.svm_launch(ctx, s, c.store, capi.SVM_GENERIC, n=1))
    idx = np.array([6, 0, 6, 3], np.uint32)
    assert _same(out[idx], capi.svm_launch(ctx, s, c.store, capi.SVM_GENERIC, idx=idx))
    wide = np.zeros((len(c.rows), c.dim + 3), np.float32)   # a row stride larger than the vector
    wide[:, :c.dim] = c.rows
    assert _same(out, capi.svm_launch(ctx, s, wide, capi.SVM_GENERIC))
    _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, capi.SVM_U8_LANES_2))
    _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, capi.SVM_U8_MFMA_8))


@pytest.mark.parametrize("name", M.names("f32count-"))
def test_generic_f32_device_count(capi, ctx, oracle, name):
    c, s = M.case(name), _svm(capi, ctx, name)
    n = len(c.rows)
    full = capi.svm_launch(ctx, s, c.store, capi.SVM_GENERIC)
    _check(oracle, name, full)
    for dcount in M.DCOUNTS:
        k = min(dcount, n)
        for variant in (capi.SVM_GENERIC, capi.SVM_PRODUCTION):
            out = capi.svm_launch(ctx, s, c.store, variant, dcount=dcount)
            assert np.array_equal(_written(capi, out), np.arange(n) < k), (variant, dcount)
            assert _same(out[:k], full[:k])


@pytest.mark.parametrize("name", M.names("f32longest-"))
def test_generic_f32_lds_boundary(capi, ctx, oracle, name):
    """a vector that fills the 64 KiB of dynamic LDS exactly is scored (red[4] comes on top: the launch limit is on the dynamic part);
    one element more gets the library's invalid-argument from every launcher"""
    c, s = M.case(name), _svm(capi, ctx, name)
    assert c.dim == M.F32_GENERIC_MAX_DIM
    out = s.distance(c.rows)
    _check(oracle, name, out)
    assert _same(out, capi.svm_launch(ctx, s, c.store, capi.SVM_GENERIC))
    m = dict(c.m, sv=np.zeros((2, c.dim + 1), np.float32))
    s1 = capi.Svm(ctx, m)
    x = np.zeros((2, c.dim + 1), np.float32)
    _refused(capi, lambda: s1.distance(x))
    for variant, dcount in ((capi.SVM_GENERIC, -1), (capi.SVM_PRODUCTION, -1), (capi.SVM_PRODUCTION, 1)):
        _refused(capi, lambda: capi.svm_launch(ctx, s1, x, variant, dcount=dcount))
    s1.close()


# ---- f32 RBF on the f32 matrix pipe ------------------------------------------------------------------------------------------------------------
def _svs_is_production():
    return os.environ.get("FD_SVM_KERNEL", "2").strip() == "2"   # the launcher's own switch


@pytest.mark.parametrize("name", M.names("rbfmfma-d"))
def test_rbf_mfma_a_resident(capi, ctx, oracle, name):
    """Q = KP / 8 below the prefetch ring's depth, tails of 1, 2 and 3 groups, the largest Q the 160 KiB budget takes; 1 .. 2 groups of
    256 support vectors with 1 .. 257 real ones; partial, full and several workgroups of 64 rows"""
    c, s = M.case(name), _svm(capi, ctx, name)
    out = capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA)
    _check(oracle, name, out)
    prod = capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA_PRODUCTION)
    if (c.dim + 7) // 8 * 8 in (328, 336):   # HOG-324: the launcher's choice is the support-vector-stationary body
        svs = capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA_SVS)
        _check(oracle, name, svs, what="svs")
        assert _same(prod, svs if _svs_is_production() else out)
    else:
        assert _same(prod, out)
        _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA_SVS))
    _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA, dcount=1))
    _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA, idx=np.zeros(1, np.uint32)))
    # the same model through k_svm_generic: its own, tighter bound against the same model
    g = capi.svm_launch(ctx, s, c.store, capi.SVM_GENERIC)
    assert np.all(np.abs(g - M.reference(name)[0]) <= M.bound(c.m, c.rows, "generic"))


def test_rbf_mfma_refuses_what_the_lds_does_not_hold(capi, ctx):
    name = "rbfmfma-refused-d%d" % M.RBF_MFMA_REFUSED_DIM
    c, s = M.case(name), _svm(capi, ctx, name)
    for variant in (capi.SVM_RBF_MFMA, capi.SVM_RBF_MFMA_PRODUCTION, capi.SVM_RBF_MFMA_SVS):
        _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, variant))
    g = capi.svm_launch(ctx, s, c.store, capi.SVM_GENERIC)
    assert np.all(np.abs(g - M.reference(name)[0]) <= M.bound(c.m, c.rows, "generic"))
    lin = capi.Svm(ctx, dict(c.m, kernel=M.LINEAR))   # no tables: not an RBF model
    _refused(capi, lambda: capi.svm_launch(ctx, lin, c.store, capi.SVM_RBF_MFMA))
    lin.close()
    _refused(capi, lambda: capi.svm_launch(ctx, s, c.store, 10))


@pytest.mark.parametrize("name", M.names("rbfsvs-d"))
def test_rbf_mfma_sv_stationary(capi, ctx, oracle, name):
    """both instantiations (padded lengths 328 and 336) at their shortest, HOG and longest vectors; one and two groups of 256 support
    vectors; 1, 33, 65 rows (one tile, two, three with the last one partial)"""
    c, s = M.case(name), _svm(capi, ctx, name)
    out = capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA_SVS)
    _check(oracle, name, out, what="svs")
    prod = capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA_PRODUCTION)
    a_res = capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA)
    _check(oracle, name, a_res, what="A-resident")
    assert _same(prod, out if _svs_is_production() else a_res)


def test_rbf_mfma_sv_stationary_persistent_loop(capi, ctx, oracle, num_cus):
    """more tiles than workgroups: with 257 support vectors the grid is num_cus / 2 workgroups per group of 256, and
    64 (num_cus / 2) 2 + 70 rows are four full rounds of 32-row tiles and three more tiles, the last one partial: workgroups walk four
    or five tiles, so the walk ends in either buffer of the double buffer"""
    name = M.SVS_PERSISTENT
    c, s = M.case(name, num_cus), _svm(capi, ctx, name, num_cus)
    n = len(c.rows)
    assert n == M.svs_persistent_n(num_cus) and n % 32
    tiles, grid = (n + 31) // 32, max(1, num_cus // 2)
    assert {len(range(b, tiles, grid)) for b in range(min(grid, tiles))} == {4, 5}
    out = capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA_SVS)
    _check(oracle, name, out, num_cus=num_cus, what="svs")
    if _svs_is_production():
        assert _same(out, capi.svm_launch(ctx, s, c.store, capi.SVM_RBF_MFMA_PRODUCTION))


def test_models_leave_the_device():
    """not a check: the module's cached models give their device memory back"""
    for s in _SVMS.values():
        s.close()
    _SVMS.clear()
    _ORACLE.clear()
