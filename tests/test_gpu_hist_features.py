"""k_hist_features and k_hog_tile (csrc/hog.hip) against the float64 model of tests/hist_model.py at the sizes where the kernels take another
path: more than 64 cells, blocks and output elements per wavefront, a second window per workgroup, the lane layouts of k_hog_tile from
one cell to 64, the padded fragment-major rows of the MFMA SVM, contents that drive the normalisers to their ends, the host table caches
and the limits of the launchers.  The bound is the model's (derived, tests/hist_model.py); the CPU oracle is the secondary check: bit for
bit where the library keeps the reference's order, inside the bound on each side elsewhere."""
import ctypes as C

import numpy as np
import pytest

import hist_model as M
import svm_score_model as S

pytestmark = pytest.mark.gpu

TWO_LAYERS = dict(octave_layers=2, min_scale=0.7, max_scale=1.0)


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _hist_params(capi, c, sx=1, sy=1):
    return capi.hist_params(kind=c.kind, pw=c.pw, ph=c.ph, sx=sx, sy=sy, bins=c.bins, cell=c.cell, block=c.block, levels=c.levels,
                            interpolate=c.interpolate, signed_and_unsigned=c.sau, concatenate=c.concatenate, normalization=c.normalization,
                            cell_h=c.cell_h, block_h=c.block_h)


def _hog_params(capi, c, sx, sy):
    return capi.hog_params(pw=c.pw, ph=c.ph, sx=sx, sy=sy, bins=c.bins, cell=c.cell, block=c.block, signed_and_unsigned=c.sau)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _inside(kernel, what, got, f, b):
    assert got.shape == f.shape and got.dtype == np.float32 and np.all(np.isfinite(got)), what
    ratio, i = M.worst(np.abs(got.astype(np.float64) - f), b)
    print("%s %s: max |kernel - model| = %.3g of the bound (element %d of %d)" % (kernel, what, ratio, i, f.size))
    assert ratio <= 1, (what, i, got.flat[i], f.flat[i], b.flat[i])
    assert not got[f == 0].any(), what


def _refused(capi, fn):
    with pytest.raises(capi.FdError) as e:
        fn()
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT, e.value


def _raw_patch_batch(capi, ctx, patches, hp, F=1):
    """fd_hist_patch_batch itself (capi.hist_patch_batch answers an invalid parameter set before the library sees it)"""
    p = np.ascontiguousarray(patches, np.uint8)
    out = np.zeros((len(p), F), np.float32)
    return capi.lib().fd_hist_patch_batch(ctx.h, p.ctypes.data_as(C.c_void_p), len(p), p.shape[3] if p.ndim == 4 else 1, C.byref(hp),
                                          out.ctypes.data_as(C.c_void_p))


# ---- k_hist_features through fd_hist_patch_batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in M.NAMES if n != M.LDS_REFUSED])
def test_patch_batch_inside_the_bound(capi, ctx, oracle, num_cus, name):
    c = M.case(name, num_cus)
    f, b = M.reference(name, num_cus)
    got = capi.hist_patch_batch(ctx, c.patches, _hist_params(capi, c))
    _inside("k_hist_features", name, got, f, b)
    if c.content in M.ZERO_CONTENT:
        assert not got.any()
    if c.oracle_patches is not None:
        fo = M.oracle_features(oracle, c, c.oracle_patches)
        if M.exact(c):
            assert _same(got, fo), (name, np.abs(got - fo).max())
        else:
            assert np.all(np.abs(got.astype(np.float64) - fo) <= 2 * b), name
    if getattr(c, "grid", 0):   # every workgroup took a second window; the first and the second of a workgroup, alone, give the same bits
        assert len(c.patches) == num_cus * 32 + 3
        again = capi.hist_patch_batch(ctx, c.patches[[0, c.grid, c.grid + 2]], _hist_params(capi, c))
        assert _same(again, got[[0, c.grid, c.grid + 2]])


# ---- the pyramid routes ---------------------------------------------------------------------------------------------------------------------------
def _pyramid(capi, ctx, image, kw, **layer_filter):
    p = capi.Pyramid(ctx, **kw)
    p.set_layer_filter(**layer_filter)
    p.update(image)
    return p


def _cut(pyr, pw, ph, sx, sy):
    wins = pyr.windows(pw, ph, sx, sy)
    return wins, M.cut_windows([pyr.layer(i) for i in range(len(pyr.layers()))], wins, pw, ph)


@pytest.mark.parametrize("case", range(len(M.EXTRACT_HIST)))
def test_extract_hist_is_patch_batch_on_the_cut_windows(capi, ctx, case):
    lf, kw = M.EXTRACT_HIST[case]
    pyr = _pyramid(capi, ctx, M.gray_image(*M.EXTRACT_HIST_IMAGE), TWO_LAYERS, **lf)
    wins, patches = _cut(pyr, 20, 20, 2, 3)
    assert len(set(wins[:, 0])) == 2 and len(wins) > 64
    c = M.patch_case(ch=patches.shape[3] if patches.ndim == 4 else 1, **kw)
    flat = patches.reshape(len(patches), 400, -1)
    if lf["kind"] == 1:   # windows wholly in the flat / checkerboard regions (all weights 0) and in the step edges, on the device's layers
        zero, saturated = M.content_windows(M.features(c, patches), flat[..., :2], c.bins)
        assert len(zero) >= 2 and len(saturated) >= 1
    else:
        assert (flat[..., 0] == flat[:, :1, 0]).all(1).any()
    got = capi.extract_hist(ctx, pyr, _hist_params(capi, c, 2, 3))
    assert _same(got, capi.hist_patch_batch(ctx, patches, _hist_params(capi, c)))
    _inside("k_hist_features", "extract_hist %d" % case, got, M.features(c, patches), M.bound(c, patches))
    pyr.close()


def _tile_pyramid(capi, ctx, geo, launch):
    _, _, _, _, bins, sau, _ = M.TILE_GEOMETRIES[geo]
    w, h, kw, sx, sy, _ = M.TILE_LAUNCHES[launch]
    return _pyramid(capi, ctx, M.gray_image(launch, w, h), kw, kind=1, bins=bins, signed_gradients=sau), sx, sy


@pytest.mark.parametrize("launch", list(M.TILE_LAUNCHES))
@pytest.mark.parametrize("geo", list(M.TILE_GEOMETRIES))
def test_extract_hog_inside_the_bound(capi, ctx, geo, launch):
    c = M.tile_case(geo)
    pyr, sx, sy = _tile_pyramid(capi, ctx, geo, launch)
    wins, patches = _cut(pyr, c.pw, c.ph, sx, sy)
    assert len(wins) > 0
    got = capi.extract_hog(ctx, pyr, _hog_params(capi, c, sx, sy))
    f = M.features(c, patches)
    _inside("k_hog_tile<false>", "%s %s" % (geo, launch), got, f, M.bound(c, patches))
    if launch == "two-layers":   # all-zero windows (normaliser 1 / sqrt(eps)) and windows at the step response are among them
        zero, saturated = M.content_windows(f, patches, c.bins)
        assert len(zero) >= 2 and len(saturated) >= 1 and not got[zero].any() and got[saturated].any(1).all()
    assert _same(got, capi.extract_hist(ctx, pyr, _hist_params(capi, c, sx, sy)))   # both claim the reference's order
    pyr.close()


def test_extract_hog_second_item_per_workgroup(capi, ctx, num_cus):
    geo, w, h, kw, sx, sy = M.TILE_PERSISTENT
    c = M.tile_case(geo)
    pyr = _pyramid(capi, ctx, M.gray_image("persistent", w, h), kw, kind=1, bins=c.bins)
    wins, patches = _cut(pyr, c.pw, c.ph, sx, sy)
    assert len(wins) > num_cus * 16 * 4          # C = 49: one item per window, four per workgroup
    got = capi.extract_hog(ctx, pyr, _hog_params(capi, c, sx, sy))
    f = M.features(c, patches)
    _inside("k_hog_tile<false>", "%s persistent" % geo, got, f, M.bound(c, patches))
    zero, saturated = M.content_windows(f, patches, c.bins)
    assert len(zero) >= 2 and len(saturated) >= 1 and not got[zero].any()
    assert _same(got, capi.extract_hist(ctx, pyr, _hist_params(capi, c, sx, sy)))
    pyr.close()


@pytest.mark.parametrize("launch", list(M.TILE_LAUNCHES))
@pytest.mark.parametrize("geo", list(M.TILE_GEOMETRIES))
def test_detect_hog_svm_fragment_path(capi, ctx, monkeypatch, geo, launch):
    """k_hog_tile<true>: the fragment-major rows with their padding and |x|^2 are what the MFMA SVM scores; none of these geometries is
    the fused one"""
    monkeypatch.delenv("FD_HOG_FUSED", raising=False)
    c = M.tile_case(geo)
    g = M.geometry(c)
    pyr, sx, sy = _tile_pyramid(capi, ctx, geo, launch)
    hp = _hog_params(capi, c, sx, sy)
    wins = pyr.windows(c.pw, c.ph, sx, sy)
    feats = capi.extract_hog(ctx, pyr, hp)
    m, kv = M.svm_for(geo + launch, feats)
    svm = capi.Svm(ctx, m)
    if not M.rbf_mfma_fits(g.F):   # the SVM's tile does not fit the LDS: refused, and the features still come
        _refused(capi, lambda: capi.detect_hog_svm(ctx, pyr, svm, hp))
        assert _same(feats, capi.extract_hog(ctx, pyr, hp))
        svm.close(); pyr.close()
        return
    assert ((kv >= 0.05) & (kv <= 0.95)).mean() >= 0.5
    if launch == "two-layers":   # all-zero fragment rows with |x|^2 = 0 are scored too
        assert (~feats.any(1)).sum() >= 2
    _, d = capi.detect_hog_svm(ctx, pyr, svm, hp)
    ref, b = S.distance(m, feats), S.bound(m, feats, "mfma")
    err = np.abs(d - ref)
    print("k_hog_tile<true> %s %s: max |distance - model| = %.3g of the bound, %d windows" % (geo, launch, (err / b).max(), len(d)))
    assert d.shape == ref.shape and np.all(err <= b)
    thr = float(np.float32(np.median(d)))
    svm2 = capi.Svm(ctx, dict(m, threshold=thr))
    dets, d2 = capi.detect_hog_svm(ctx, pyr, svm2, hp)
    assert _same(d, d2)
    pos = np.nonzero(d2 >= thr)[0]
    assert 0 < len(pos) < len(d2) or len(d2) == 1
    assert [(int(t["layer"]), int(t["lx"]), int(t["ly"])) for t in dets] == [tuple(int(v) for v in wins[i][:3]) for i in pos]
    svm.close(); svm2.close(); pyr.close()


def test_detect_hog_svm_second_item_per_workgroup(capi, ctx, monkeypatch, num_cus):
    """k_hog_tile<true> with C = 49 and one block (F = 441, KP = 448: |x|^2 from 64 partial sums per window) on more than
    num_cus * 16 * 4 windows: a wavefront takes a second (tile, pass) item"""
    monkeypatch.delenv("FD_HOG_FUSED", raising=False)
    _, w, h, kw, sx, sy = M.TILE_PERSISTENT
    geo = M.TILE_PERSISTENT_FRAG
    c = M.tile_case(geo)
    pyr = _pyramid(capi, ctx, M.gray_image("persistent", w, h), kw, kind=1, bins=c.bins)
    hp = _hog_params(capi, c, sx, sy)
    wins, patches = _cut(pyr, c.pw, c.ph, sx, sy)
    assert len(wins) > num_cus * 16 * 4 and len(wins) % 32 != 0
    feats = capi.extract_hog(ctx, pyr, hp)
    _inside("k_hog_tile<false>", "%s persistent" % geo, feats, M.features(c, patches), M.bound(c, patches))
    m, kv = M.svm_for(geo + "persistent", feats)
    assert ((kv >= 0.05) & (kv <= 0.95)).mean() >= 0.5 and (~feats.any(1)).sum() >= 2
    svm = capi.Svm(ctx, m)
    _, d = capi.detect_hog_svm(ctx, pyr, svm, hp)
    ref, b = S.distance(m, feats), S.bound(m, feats, "mfma")
    err = np.abs(d - ref)
    print("k_hog_tile<true> %s persistent: max |distance - model| = %.3g of the bound, %d windows" % (geo, (err / b).max(), len(d)))
    assert d.shape == ref.shape and np.all(err <= b)
    thr = float(np.float32(np.median(d)))
    svm2 = capi.Svm(ctx, dict(m, threshold=thr))
    dets, d2 = capi.detect_hog_svm(ctx, pyr, svm2, hp)
    pos = np.nonzero(d2 >= thr)[0]
    assert _same(d, d2) and 0 < len(pos) < len(d2)
    assert [(int(t["layer"]), int(t["lx"]), int(t["ly"])) for t in dets] == [tuple(int(v) for v in wins[i][:3]) for i in pos]
    svm.close(); svm2.close(); pyr.close()


# ---- the host tables of both kernels are cached per context ---------------------------------------------------------------------------------
def test_table_caches_a_b_a(capi, ctx):
    a, b = M.case("hog-23x17-c5-b2-interp"), M.case("hog-23x17-c5-b2")   # the same patch size, interpolating and not
    c3 = M.case("spatial-b1-norm2")
    runs = [capi.hist_patch_batch(ctx, c.patches, _hist_params(capi, c)) for c in (a, b, a, c3, a, b)]
    assert _same(runs[0], runs[2]) and _same(runs[0], runs[4]) and _same(runs[1], runs[5]) and not _same(runs[0], runs[1])
    pyr, sx, sy = _tile_pyramid(capi, ctx, "20x20-c6-b2-9", "two-layers")
    ga, gb = M.tile_case("20x20-c6-b2-9"), M.tile_case("20x20-c4-b1-9")
    runs = [capi.extract_hog(ctx, pyr, _hog_params(capi, t, sx, sy)) for t in (ga, gb, ga, gb)]
    assert _same(runs[0], runs[2]) and _same(runs[1], runs[3]) and runs[0].shape != runs[1].shape
    pyr.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(capi, ctx):
    good = M.tile_case("20x20-c6-b2-9")
    pyr, sx, sy = _tile_pyramid(capi, ctx, "20x20-c6-b2-9", "two-layers")
    first = capi.extract_hog(ctx, pyr, _hog_params(capi, good, sx, sy))
    hog_refused = dict(
        side33=dict(pw=33, ph=20), cells65=dict(pw=26, ph=10, cell=2, block=2), blocks65=dict(pw=26, ph=10, cell=2, block=1),
        hist1025=dict(cell=4, block=1, bins=41), bins65=dict(cell=20, block=1, bins=65), odd_sau=dict(bins=9, signed_and_unsigned=True))
    assert 13 * 5 == 65 and 12 * 4 < 64 and 25 * 41 == 1025
    for what, kw in hog_refused.items():
        _refused(capi, lambda: capi.extract_hog(ctx, pyr, capi.hog_params(**dict(dict(sx=sx, sy=sy), **kw))))
        assert capi.lib().fd_hog_feature_length(C.byref(capi.hog_params(**kw))) == -1, what
        assert _same(first, capi.extract_hog(ctx, pyr, _hog_params(capi, good, sx, sy))), what
    pyr.close()
    c = M.case("hog-23x17-c5-b2")
    hp = _hist_params(capi, c)
    before = capi.hist_patch_batch(ctx, c.patches, hp)
    side65 = np.zeros((2, 20, 65, 2), np.uint8)
    odd = M.patch_case(M.HOG, bins=9, sau=True, block=2)
    for what, patches, bad in (("side 65", side65, capi.hist_params(kind=M.HOG, pw=65, ph=20, bins=9, cell=5, block=1)),
                               ("odd bins", np.zeros((2, 20, 20, 2), np.uint8), _hist_params(capi, odd))):
        assert _raw_patch_batch(capi, ctx, patches, bad) == capi.FD_ERR_INVALID_ARGUMENT, what
        assert _same(before, capi.hist_patch_batch(ctx, c.patches, hp)), what
    # the LDS limit: the vector of 169 * 234 floats with its patch and tables is above 160 KiB, 169 * 233 is below and inside the bound
    acc, ref = M.case(M.LDS_ACCEPTED), M.case(M.LDS_REFUSED)
    assert M.lds_bytes(acc) <= M.LDS_BUDGET < M.lds_bytes(ref)
    got = capi.hist_patch_batch(ctx, acc.patches, _hist_params(capi, acc))
    _refused(capi, lambda: capi.hist_patch_batch(ctx, ref.patches, _hist_params(capi, ref)))
    assert _same(got, capi.hist_patch_batch(ctx, acc.patches, _hist_params(capi, acc)))
    _inside("k_hist_features", M.LDS_ACCEPTED, got, *M.reference(M.LDS_ACCEPTED))
    assert _same(before, capi.hist_patch_batch(ctx, c.patches, hp))
