"""GPU parity tests: the HIP path through the C ABI against the CPU oracle on identical seeded inputs.
Bit-exact for integer/byte/index work (pyramid layers, window enumeration, HistEq64, WVM level and
fp32 filter output, HOG features, detections); stated tolerances for the fp paths that reorder sums."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FF = dict(inc=float(np.float32(0.92)), min_scale=float(np.float32(0.05)), max_scale=float(np.float32(0.16)))  # FaceFrontal.cfg


def _pyr_pair(oracle, capi, ctx, frame, **kw):
    po = oracle.Pyramid(**kw)
    po.update(frame)
    pg = capi.Pyramid(ctx, **kw)
    pg.update(frame)
    return po, pg


def _same_geometry(g, o):
    for f in ("cx", "cy", "w", "h", "layer", "lx", "ly"):
        assert np.array_equal(g[f], o[f]), f


def test_native_library_loaded(capi, ctx):
    assert b"gfx950" in capi.lib().fd_version()
    maps = open("/proc/self/maps").read()
    assert "libfd_hip.so" in maps


@pytest.mark.parametrize("size,kw", [((640, 480), FF), ((640, 480), dict(octave_layers=5, min_scale=1 / 16, max_scale=1.0)),
                                      ((321, 243), dict(octave_layers=3, min_scale=0.1, max_scale=0.8)),
                                      ((1283, 721), dict(octave_layers=4, min_scale=0.05, max_scale=0.6)),   # width % 4 != 0: dwords over the right edge
                                      ((97, 131), dict(octave_layers=6, min_scale=0.2, max_scale=1.0)),
                                      ((1920, 1080), dict(inc=float(np.float32(0.9)), min_scale=float(np.float32(0.09)),
                                                          max_scale=float(np.float32(0.25))))])
def test_pyramid_layers_bit_exact(oracle, capi, ctx, synth, size, kw):
    frame = synth.make_frame(size[0], size[1], seed=size[0])
    po, pg = _pyr_pair(oracle, capi, ctx, frame, **kw)
    assert pg.octave_layers == po.octave_layers and pg.inc == po.inc
    lo, lg = po.layers(), pg.layers()
    assert lo == lg
    for i in range(len(lo)):
        assert np.array_equal(pg.layer(i), po.layer(i)), "layer %d" % i
    # gray input must give the same pyramid as its BGR source converted by the oracle
    gray = oracle.bgr2gray(frame)
    pg.update(gray)
    assert np.array_equal(pg.layer(len(lg) - 1), po.layer(len(lo) - 1))
    pg.close()


@pytest.mark.parametrize("size", [(13, 9), (7, 5), (9, 2), (3, 37), (130, 3), (2, 2), (257, 5)])
def test_pyramid_of_tiny_frames_bit_exact(oracle, capi, ctx, synth, size):
    """Layers of one to three pixels across: the pyrDown kernels' closed-form BORDER_REFLECT_101 (two pixels out on either side, so a
    1- or 2-pixel layer is reflected more than once by the reference) and the clamped, unpredicated tile fetch at both edges at once."""
    frame = synth.make_frame(size[0], size[1], seed=7 + size[0] * size[1])
    for kw in (dict(octave_layers=1, min_scale=0.03, max_scale=1.0), dict(octave_layers=3, min_scale=0.06, max_scale=1.0)):
        po, pg = _pyr_pair(oracle, capi, ctx, frame, **kw)
        lo, lg = po.layers(), pg.layers()
        assert lo == lg and len(lo) >= 2
        for i in range(len(lo)):
            assert np.array_equal(pg.layer(i), po.layer(i)), (kw, "layer %d of %s" % (i, lo))
        pg.close()


@pytest.mark.parametrize("roi", [None, (100, 80, 300, 200), (-20, -10, 200, 100), (500, 400, 400, 400)])
def test_window_enumeration(oracle, capi, ctx, frame640, roi):
    po, pg = _pyr_pair(oracle, capi, ctx, frame640, **FF)
    for (pw, ph, sx, sy) in ((20, 20, 1, 1), (20, 20, 2, 2), (32, 16, 3, 1)):
        assert np.array_equal(pg.windows(pw, ph, sx, sy, roi), po.windows(pw, ph, sx, sy, roi))
    pg.close()


def test_layer_filters_bit_exact(oracle, capi, ctx, frame640):
    kw = dict(octave_layers=3, min_scale=0.2, max_scale=1.0)
    for filt in (dict(kind=1, bins=9), dict(kind=1, bins=8, signed_gradients=True), dict(kind=1, bins=9, interpolate=True),
                 dict(kind=1, bins=9, grad_kernel=3), dict(kind=1, bins=9, grad_kernel=5), dict(kind=1, bins=12, grad_kernel=7, signed_gradients=True),
                 dict(kind=1, bins=9, grad_kernel=-1, interpolate=True), dict(kind=1, bins=9, grad_kernel=3, blur_kernel=3),
                 dict(kind=1, bins=9, grad_kernel=1, blur_kernel=4), dict(kind=2, lbp_type=0), dict(kind=2, lbp_type=1), dict(kind=2, lbp_type=2),
                 dict(kind=2, lbp_type=3)):
        po = oracle.Pyramid(**kw)
        po.set_layer_filter(**filt)
        po.update(frame640)
        pg = capi.Pyramid(ctx, **kw)
        pg.set_layer_filter(**filt)
        pg.update(frame640)
        assert pg.layers() == po.layers()
        for i in range(len(po.layers())):
            assert np.array_equal(pg.layer(i), po.layer(i)), (filt, i)
        pg.close()


def test_histeq64_bit_exact_including_half_ties(oracle, ctx):
    rng = np.random.default_rng(3)
    patches = rng.integers(0, 256, (512, 20, 20), dtype=np.uint8)
    # exact .5 ties: cumulative counts of 40, 120, 200, ... pixels (255/400 * k = m + 0.5)
    t = np.zeros((20, 20), np.uint8).ravel()
    t[:40] = 8; t[40:120] = 100; t[120:200] = 160; t[200:] = 250
    patches[0] = t.reshape(20, 20)
    patches[1] = 255
    patches[2] = 0
    out = ctx.histeq64(patches)
    for i in range(len(patches)):
        assert np.array_equal(out[i], oracle.histeq64(patches[i])), i
    for (w, h) in ((32, 16), (16, 24), (24, 24), (32, 24)):
        p = rng.integers(0, 256, (64, h, w), dtype=np.uint8)
        o = ctx.histeq64(p)
        for i in range(len(p)):
            assert np.array_equal(o[i], oracle.histeq64(p[i])), (w, h, i)


def test_greyworld_bit_exact(oracle, ctx, frame640):
    assert np.array_equal(ctx.greyworld(frame640), oracle.greyworld(frame640))


def test_wvm_all_windows_bit_exact(oracle, capi, ctx, frame640, small_models):
    """Every window's (last level, fp32 filter output) must equal the CPU cascade exactly."""
    wvm, _ = small_models
    po, pg = _pyr_pair(oracle, capi, ctx, frame640, **FF)
    wo = oracle.Wvm(wvm)
    wg = capi.Wvm(ctx, wvm)
    for step in (1, 2):
        pos_o, lv_o, fo_o = oracle.sliding_wvm(po, wo, step, step)
        pos_g, lv_g, fo_g = capi.detect_wvm(ctx, pg, wg, step, step, want_all=True)
        assert len(lv_g) == len(lv_o) == (16185 if step == 1 else 4161)
        assert np.array_equal(lv_g, lv_o)
        assert np.array_equal(fo_g, fo_o)
        assert len(pos_g) == len(pos_o)
        _same_geometry(pos_g, pos_o)
        assert np.array_equal(pos_g["score"], pos_o["fout"])
        assert np.array_equal(pos_g["probability"], pos_o["prob"])
    wg.close(); pg.close()


@pytest.mark.parametrize("num_used", [17, 23, 29])
def test_wvm_with_a_used_filter_count_between_level_groups(oracle, capi, ctx, frame640, small_models, num_used):
    """numUsedFilters (WvmClassifier.cpp:151-158) that is not a multiple of numFiltersPerLevel: the classes of stage B have different
    numbers of generations; every window's (last level, fp32 output) and the positives against the CPU cascade, production and exact path."""
    wvm = dict(small_models[0])
    wvm["num_used"] = num_used
    po, pg = _pyr_pair(oracle, capi, ctx, frame640, **FF)
    wo = oracle.Wvm(wvm)
    wg = capi.Wvm(ctx, wvm)
    pos_o, lv_o, fo_o = oracle.sliding_wvm(po, wo, 1, 1)
    pos_g, lv_g, fo_g = capi.detect_wvm(ctx, pg, wg, 1, 1, want_all=True)
    assert np.array_equal(lv_g, lv_o) and np.array_equal(fo_g, fo_o)
    assert int((lv_o == num_used - 1).sum()) > 100   # windows do run to the last used level (whether they are positives is the threshold's matter)
    pos_p, _, _ = capi.detect_wvm(ctx, pg, wg, 1, 1, want_all=False)   # dense pre-filter + stage B
    assert len(pos_p) == len(pos_o) == len(pos_g)
    if len(pos_o):
        _same_geometry(pos_p, pos_o)
        assert np.array_equal(pos_p["score"], pos_o["fout"])
    wg.close(); pg.close()


def test_wvm_full_size_model_and_other_patch_shapes(oracle, capi, ctx, synth, frame640):
    gray = oracle.bgr2gray(frame640)
    rng = np.random.default_rng(8)
    cfgs = dict(synth.DETECTOR_CFGS)
    cfgs["odd19x21"] = (0.9, 0.5, 0.7, 19, 21, 9, 4)   # run-time-sized kernel instance, odd height
    cfgs["tiny7x5"] = (0.9, 0.5, 0.7, 7, 5, 3, 4)
    cfgs["nper40"] = (0.9, 0.5, 0.7, 20, 20, 40, 1)   # numPer > 32: one-window stage A kernel with compile-time geometry
    # 16 grey values x up to 8 rects x 14 classes: > 1280 rects per generation (stage B stages them piecewise) and the 16-value kernel
    cfgs["manyrects"] = (0.9, 0.5, 0.7, 20, 20, 14, 1)
    cfgs["manyrects24"] = (0.9, 0.5, 0.7, 24, 24, 9, 1)
    extra = dict(manyrects=dict(cntval=16, rect_range=(6, 8)), manyrects24=dict(cntval=12, rect_range=(1, 8)))
    for (name, n_levels) in (("FaceFrontal", 20), ("LeftEyeCenter", 3), ("NoseTip", 2), ("LeftEarCenter", 2), ("LeftLipCorner", 2),
                             ("odd19x21", 4), ("tiny7x5", 8), ("nper40", 2), ("manyrects", 3), ("manyrects24", 9)):
        inc, mn, mx, pw, ph, nper, _ = cfgs[name]
        calib = synth.random_patches(gray[::2, ::2].copy(), pw, ph, 3000, rng)
        wvm = synth.make_wvm(31, fw=pw, fh=ph, n_per=nper, n_levels=n_levels, calib_patches=calib, min_survivors=48, **extra.get(name, {}))
        kw = dict(inc=float(np.float32(inc)), min_scale=float(np.float32(mn)), max_scale=float(np.float32(mx)))
        small = frame640[:240, :320] if name != "FaceFrontal" else frame640
        po, pg = _pyr_pair(oracle, capi, ctx, small, **kw)
        wo, wg = oracle.Wvm(wvm), capi.Wvm(ctx, wvm)
        step = 1 if name == "FaceFrontal" else 3
        pos_o, lv_o, fo_o = oracle.sliding_wvm(po, wo, step, step)
        pos_g, lv_g, fo_g = capi.detect_wvm(ctx, pg, wg, step, step, want_all=True)
        assert len(lv_o) > 0
        assert np.array_equal(lv_g, lv_o), name
        assert np.array_equal(fo_g, fo_o), name
        _same_geometry(pos_g, pos_o)
        wg.close(); pg.close()


def test_wvm_eval_batch_per_patch_api(oracle, capi, ctx, small_models):
    """fd_wvm_eval_batch backs the per-Mat classify()/getProbability() of the reference interface"""
    wvm, _ = small_models
    rng = np.random.default_rng(17)
    patches = np.stack([oracle.histeq64(rng.integers(0, 256, (20, 20), dtype=np.uint8)) for _ in range(300)])
    wo, wg = oracle.Wvm(wvm), capi.Wvm(ctx, wvm)
    lv, sc = capi.wvm_eval(ctx, wg, patches)
    for i in range(len(patches)):
        l, f = wo.eval(patches[i])
        assert (l, np.float32(f)) == (lv[i], sc[i]), i
    wg.close()


@pytest.mark.parametrize("kernel,dtype", [(2, 0), (3, 0), (0, 0), (1, 0), (2, 1), (3, 1), (0, 1), (1, 1)])
def test_svm_distance_batch(oracle, capi, ctx, kernel, dtype):
    rng = np.random.default_rng(kernel * 2 + dtype)
    nsv, dim, n = 200, 400, 64
    if dtype == 0:
        sv = rng.integers(0, 256, (nsv, dim), dtype=np.uint8)
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        p0 = {2: 0.04 / 65025.0, 1: 1.0 / 65025.0}.get(kernel, 0.0)
    else:
        sv = rng.random((nsv, dim)).astype(np.float32) * 0.2
        x = rng.random((n, dim)).astype(np.float32) * 0.2
        p0 = {2: 0.5, 1: 0.3}.get(kernel, 0.0)
    m = dict(kernel=kernel, p0=p0, p1=0.7, p2=3, dtype=dtype, sv=sv, coeff=rng.normal(0, 1, nsv).astype(np.float32),
             bias=np.float32(0.25), threshold=0.0)
    do = oracle.Svm(m).distance(x)
    sg = capi.Svm(ctx, m)
    dg = sg.distance(x)
    # integer kernels are exact per term; only the order of the fp64 sum over support vectors differs.
    # f32 RBF/HIK reorder an fp32 sum inside each kernel value -> 1e-4 relative to the term scale.
    scale = np.abs(m["coeff"]).sum() * (np.abs(do).max() / max(np.abs(m["coeff"]).sum(), 1e-30) if kernel in (0, 1, 3) else 1.0)
    tol = 1e-12 if (dtype == 0) else 1e-5
    assert np.all(np.abs(dg - do) <= 1e-4 * np.abs(do) + tol * max(scale, 1.0)), (np.abs(dg - do).max(), scale)
    if dtype == 0 and kernel in (2, 3):
        assert np.allclose(dg, do, rtol=1e-12, atol=1e-12 * scale)
    sg.close()


def test_five_stage_cascade_identical_detections(oracle, capi, ctx, frame640, small_models):
    wvm, svm = small_models
    po, pg = _pyr_pair(oracle, capi, ctx, frame640, **FF)
    wo, so = oracle.Wvm(wvm), oracle.Svm(svm)
    wg, sg = capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)
    for roi in (None, (120, 60, 360, 300)):
        do, sto = oracle.five_stage(po, wo, so, 5.0, 0.0, 1, 1, roi)
        dg, stg = capi.detect_five_stage(ctx, pg, wg, sg, 5.0, 0.0, 1, 1, roi)
        assert np.array_equal(stg, sto), (stg, sto)
        assert sto[0] > 10 and sto[2] > 0, "test model produces no detections: %s" % sto
        _same_geometry(dg, do)
        assert np.array_equal(dg["probability"], do["prob"])
        assert np.allclose(dg["score"], do["fout"], rtol=1e-6, atol=1e-6)
    # relative OE distance and ratio
    do, sto = oracle.five_stage(po, wo, so, 0.5, 0.7, 2, 2, None)
    dg, stg = capi.detect_five_stage(ctx, pg, wg, sg, 0.5, 0.7, 2, 2, None)
    assert np.array_equal(stg, sto)
    _same_geometry(dg, do)
    wg.close(); sg.close(); pg.close()


def test_golden_cascade_fixture(capi, ctx):
    """Committed oracle vectors (tests/golden): the GPU path must reproduce them on the GPU box,
    where neither the reference nor (necessarily) the oracle build is available."""
    g = np.load(os.path.join(G, "orc_cascade_160x120.npz"))
    wvm = {k[5:]: g[k] for k in g.files if k.startswith("wvm__")}
    svm = {k[5:]: g[k] for k in g.files if k.startswith("svm__")}
    svm["dtype"] = int(svm["dtype"]); svm["kernel"] = int(svm["kernel"])
    pg = capi.Pyramid(ctx, octave_layers=4, min_scale=0.4, max_scale=1.0)
    pg.update(g["frame"])
    sizes = np.array([[l["index"], l["w"], l["h"]] for l in pg.layers()], np.int32)
    assert np.array_equal(sizes, g["layer_sizes"])
    assert np.array_equal(pg.layer(len(sizes) - 1), g["last_layer"])
    wg, sg = capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)
    pos, lv, fo = capi.detect_wvm(ctx, pg, wg, 1, 1, want_all=True)
    assert np.array_equal(lv, g["wvm_level"])
    assert np.array_equal(fo, g["wvm_fout"])
    dets, stages = capi.detect_five_stage(ctx, pg, wg, sg)
    assert np.array_equal(stages, g["stages"])
    for f in ("cx", "cy", "w", "h", "layer", "lx", "ly"):
        assert np.array_equal(dets[f], g["five"][f])
    pg2 = capi.Pyramid(ctx, octave_layers=3, min_scale=0.3, max_scale=1.0)
    pg2.set_layer_filter(1, bins=9)
    pg2.update(g["frame"])
    feats = capi.extract_hog(ctx, pg2, capi.hog_params())
    assert len(feats) == int(g["hog_n"])
    assert np.array_equal(feats[:64], g["hog_feat_head"])
    wg.close(); sg.close(); pg.close(); pg2.close()


@pytest.mark.parametrize("hp", [dict(), dict(signed_and_unsigned=True, bins=8), dict(cell=4, block=1), dict(pw=32, ph=16, cell=8, block=2),
                                dict(sx=1, sy=3, cell=10, block=1)])
def test_hog_features_bit_exact(oracle, capi, ctx, frame640, hp):
    kw = dict(octave_layers=2, min_scale=0.25, max_scale=0.6)
    p = dict(pw=20, ph=20, sx=2, sy=2, bins=9, cell=5, block=2, signed_and_unsigned=False)
    p.update(hp)
    po = oracle.Pyramid(**kw)
    po.set_layer_filter(1, bins=p["bins"], signed_gradients=p["signed_and_unsigned"])
    po.update(frame640)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_layer_filter(1, bins=p["bins"], signed_gradients=p["signed_and_unsigned"])
    pg.update(frame640)
    _, _, fo = oracle.sliding_hog_svm(po, None, p["pw"], p["ph"], p["sx"], p["sy"], p["bins"], p["cell"], p["block"], False,
                                      p["signed_and_unsigned"], want_feats=10 ** 9)
    fg = capi.extract_hog(ctx, pg, capi.hog_params(**p))
    assert fg.shape == fo.shape and len(fo) > 1000
    assert np.array_equal(fg, fo)
    pg.close()


def _oracle_hist_features(oracle, po, hp, fn):
    """fn(bin-image patch) for every window of the oracle pyramid, in extraction order"""
    layers = [po.layer(i) for i in range(len(po.layers()))]
    feats = []
    for lp, lx, ly, *_ in po.windows(hp.patch_w, hp.patch_h, hp.step_x, hp.step_y):
        feats.append(fn(np.ascontiguousarray(layers[lp][ly:ly + hp.patch_h, lx:lx + hp.patch_w])))
    return np.stack(feats)


HIST_CASES = [
    # (layer filter kwargs, hist params, oracle function name, oracle kwargs, exact?)
    (dict(kind=1, bins=9), dict(kind=0, bins=9, cell=5, block=2, interpolate=True), "hog_filter",
     dict(bins=9, cell=5, block=2, interpolate=True), True),
    (dict(kind=1, bins=8, signed_gradients=True, interpolate=True), dict(kind=0, bins=8, cell=5, block=2, interpolate=True, signed_and_unsigned=True),
     "hog_filter", dict(bins=8, cell=5, block=2, interpolate=True, signed_and_unsigned=True), True),
    (dict(kind=1, bins=9), dict(kind=0, bins=9, cell=4, block=3), "hog_filter", dict(bins=9, cell=4, block=3), True),
    (dict(kind=2, lbp_type=1), dict(kind=1, bins=59, cell=5, block=1, normalization=2), "spatial_histogram",
     dict(bins=59, cell=5, block=1, normalization=2), False),
    (dict(kind=2, lbp_type=0), dict(kind=1, bins=256, cell=10, block=1, interpolate=True, normalization=1), "spatial_histogram",
     dict(bins=256, cell=10, block=1, interpolate=True, normalization=1), False),
    (dict(kind=2, lbp_type=2), dict(kind=1, bins=16, cell=5, block=2, concatenate=True, normalization=4), "spatial_histogram",
     dict(bins=16, cell=5, block=2, concatenate=True, normalization=4), True),
    (dict(kind=1, bins=9), dict(kind=1, bins=9, cell=5, block=2, concatenate=False, normalization=3, interpolate=True), "spatial_histogram",
     dict(bins=9, cell=5, block=2, concatenate=False, normalization=3, interpolate=True), True),
    (dict(kind=1, bins=9), dict(kind=1, bins=9, cell=5, block=1, normalization=0), "spatial_histogram",
     dict(bins=9, cell=5, block=1, normalization=0), True),
    (dict(kind=1, bins=8, signed_gradients=True), dict(kind=2, bins=8, levels=3, signed_and_unsigned=True), "pyramid_hog",
     dict(bins=8, levels=3, signed_and_unsigned=True), True),
    (dict(kind=1, bins=9, interpolate=True), dict(kind=2, bins=9, levels=2, interpolate=True), "pyramid_hog",
     dict(bins=9, levels=2, interpolate=True), True),
    (dict(kind=2, lbp_type=1), dict(kind=3, bins=59, levels=3, normalization=1), "spatial_pyramid_histogram",
     dict(bins=59, levels=3, normalization=1), True),
    (dict(kind=1, bins=9), dict(kind=3, bins=9, levels=2, interpolate=True, normalization=2), "spatial_pyramid_histogram",
     dict(bins=9, levels=2, interpolate=True, normalization=2), True),
    # non-square cells and blocks (cellWidth 5, cellHeight 4, blockWidth 2, blockHeight 3)
    (dict(kind=1, bins=9), dict(kind=0, bins=9, cell=5, cell_h=4, block=2, block_h=3), "hog_filter",
     dict(bins=9, cell=5, cell_h=4, block=2, block_h=3), True),
    (dict(kind=2, lbp_type=3), dict(kind=1, bins=16, cell=4, cell_h=10, block=3, block_h=1, concatenate=True, normalization=1, interpolate=True),
     "spatial_histogram", dict(bins=16, cell=4, cell_h=10, block=3, block_h=1, concatenate=True, normalization=1, interpolate=True), True),
]


@pytest.mark.parametrize("case", range(len(HIST_CASES)))
def test_histogram_filters_match_oracle(oracle, capi, ctx, frame640, case):
    """HogFilter (interpolating), SpatialHistogramFilter, PyramidHogFilter, SpatialPyramidHistogramFilter on every
    window.  Bit-exact where the reference order is reproduced; the whole-vector normalisation of the block-1x1
    SpatialHistogramFilter reduces in fp64 across lanes and is compared at 1e-6 relative."""
    lf, hpk, fname, okw, exact = HIST_CASES[case]
    kw = dict(octave_layers=2, min_scale=0.2, max_scale=0.4)
    small = np.ascontiguousarray(frame640[:240, :320])
    po = oracle.Pyramid(**kw)
    po.set_layer_filter(**lf)
    po.update(small)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_layer_filter(**lf)
    pg.update(small)
    hp = capi.hist_params(pw=20, ph=20, sx=3, sy=3, **hpk)
    fo = _oracle_hist_features(oracle, po, hp, lambda patch: getattr(oracle, fname)(patch, **okw))
    fg = capi.extract_hist(ctx, pg, hp)
    assert fg.shape == fo.shape and len(fo) > 300
    if exact:
        assert np.array_equal(fg, fo)
    else:
        assert np.allclose(fg, fo, rtol=1e-6, atol=1e-9)
    pg.close(); po.close()


def test_lbp_hik_svm_detector(oracle, capi, ctx, synth, frame640):
    """LBP(uniform) layers + SpatialHistogramFilter + histogram-intersection SVM (the LBP chain of
    BenchmarkRunner.cpp:185-201): distances within 1e-4 relative, positives identical away from the threshold."""
    kw = dict(octave_layers=2, min_scale=0.2, max_scale=0.4)
    small = np.ascontiguousarray(frame640[:240, :320])
    po = oracle.Pyramid(**kw)
    po.set_layer_filter(kind=2, lbp_type=1)
    po.update(small)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_layer_filter(kind=2, lbp_type=1)
    pg.update(small)
    hp = capi.hist_params(kind=1, pw=20, ph=20, sx=3, sy=3, bins=59, cell=5, block=1, normalization=1)
    fo = _oracle_hist_features(oracle, po, hp, lambda patch: oracle.spatial_histogram(patch, bins=59, cell=5, block=1, normalization=1))
    rng = np.random.default_rng(5)
    nsv = 96
    sv = fo[rng.choice(len(fo), nsv, replace=False)].copy()
    coeff = rng.normal(0, 1, nsv).astype(np.float32)
    m = dict(kernel=3, dtype=1, sv=sv, coeff=coeff, bias=np.float32(0.0), p0=0.0, p1=0.0, p2=0.0, threshold=0.0, logistic_a=0.0,
             logistic_b=-1.0)
    so = oracle.Svm(m)
    do = so.distance(fo)
    m["threshold"] = float(np.float32(np.quantile(do, 0.97)))
    sg = capi.Svm(ctx, m)
    dets, dg = capi.detect_hist_svm(ctx, pg, sg, hp)
    scale = np.abs(coeff).sum() * fo.sum(1).max()
    assert np.max(np.abs(dg - do)) <= 1e-4 * scale
    margin = 1e-4 * scale
    sure = np.abs(do - float(m["threshold"])) > margin
    pos_o = do >= float(m["threshold"])
    wins = po.windows(20, 20, 3, 3)
    got = {(int(d["layer"]), int(d["lx"]), int(d["ly"])) for d in dets}
    for i in np.nonzero(sure)[0]:
        key = (int(wins[i][0]), int(wins[i][1]), int(wins[i][2]))
        assert (key in got) == bool(pos_o[i])
    sg.close(); pg.close(); po.close()


def test_whi_chain_and_histeq(oracle, capi, ctx, frame640):
    """WhiteningFilter -> HistogramEqualizationFilter -> ConversionFilter -> UnitNormFilter per patch and per
    pyramid window.  The kernel evaluates the oracle's DFT sums in the same order (whitened + equalised u8 image
    bit-identical); the L2 norm is reduced across lanes, hence 1e-6 relative on the final floats."""
    gray = oracle.bgr2gray(frame640)
    rng = np.random.default_rng(4)
    for (h, w) in ((20, 20), (24, 24), (16, 32), (15, 21)):
        patches = np.stack([gray[y:y + h, x:x + w] for y, x in zip(rng.integers(0, 400, 40), rng.integers(0, 560, 40))])
        patches[0] = 77   # constant patch: equalizeHist early-out
        eq_g = capi.equalize_hist_batch(ctx, patches)
        eq_o = np.stack([oracle.equalize_hist(p_) for p_ in patches])
        assert np.array_equal(eq_g, eq_o)
        for alpha, cutoff in ((1.0, 0.390625), (0.5, 0.0)):
            wg = capi.whi_batch(ctx, patches, alpha, cutoff)
            wo = np.stack([oracle.whi(p_, alpha, cutoff) for p_ in patches])
            assert np.allclose(wg, wo, rtol=1e-6, atol=1e-9)
    kw = dict(octave_layers=2, min_scale=0.2, max_scale=0.4)
    small = np.ascontiguousarray(frame640[:240, :320])
    po = oracle.Pyramid(**kw); po.update(small)
    pg = capi.Pyramid(ctx, **kw); pg.update(small)
    wp = capi.whi_params(20, 20, 3, 3)
    layers = [po.layer(i) for i in range(len(po.layers()))]
    fo = np.stack([oracle.whi(np.ascontiguousarray(layers[lp][ly:ly + 20, lx:lx + 20])).ravel() for lp, lx, ly, *_ in po.windows(20, 20, 3, 3)])
    fg = capi.extract_whi(ctx, pg, wp)
    assert fg.shape == fo.shape and len(fo) > 300
    assert np.allclose(fg, fo, rtol=1e-6, atol=1e-9)
    # whi + RBF SVM detector (ffpDetectApp.cpp featurespace "whi", classifier "psvm")
    nsv = 64
    sv = fo[rng.choice(len(fo), nsv, replace=False)].copy()
    coeff = rng.normal(0, 1, nsv).astype(np.float32)
    m = dict(kernel=2, dtype=1, sv=sv, coeff=coeff, bias=np.float32(0.1), p0=2.0, p1=0.0, p2=0.0, threshold=0.0, logistic_a=0.0, logistic_b=-1.0)
    so = oracle.Svm(m)
    do = so.distance(fo)
    m["threshold"] = float(np.float32(np.quantile(do, 0.95)))
    sg = capi.Svm(ctx, m)
    dets, dg = capi.detect_whi_svm(ctx, pg, sg, wp)
    scale = np.abs(coeff).sum()
    assert np.max(np.abs(dg - do)) <= 1e-4 * scale
    sure = np.abs(do - m["threshold"]) > 1e-4 * scale
    wins = po.windows(20, 20, 3, 3)
    got = {(int(d["layer"]), int(d["lx"]), int(d["ly"])) for d in dets}
    for i in np.nonzero(sure)[0]:
        assert ((int(wins[i][0]), int(wins[i][1]), int(wins[i][2])) in got) == bool(do[i] >= m["threshold"])
    sg.close(); pg.close(); po.close()


@pytest.mark.parametrize("kernel", [2, 1, 3, 0])
def test_rvm_eval_batch_matches_oracle(oracle, capi, ctx, synth, kernel):
    """fd_rvm_eval_batch (per-Mat API of RvmClassifier): last level identical, fp64 distance to the last bits
    (the device exp may differ from libm by an ulp of fp64)."""
    rng = np.random.default_rng(31 + kernel)
    feats = (rng.integers(0, 256, (3000, 20 * 20)).astype(np.float32)) * np.float32(1.0 / 255.0)
    feats += (rng.random(feats.shape) * 0.01).astype(np.float32)
    m = synth.make_rvm(7 + kernel, feats[:1500], 20, 20, n_filters=40, kernel=kernel)
    ro, rg = oracle.Rvm(m), capi.Rvm(ctx, m)
    lo, do = ro.eval(feats)
    lg, dg = rg.eval(feats)
    assert np.array_equal(lg, lo)
    assert np.allclose(dg, do, rtol=1e-12, atol=1e-300)
    assert (lo == 39).sum() > 0 and (lo < 3).sum() > len(feats) // 3
    m2 = dict(m, num_used=5)
    lo2, _ = oracle.Rvm(m2).eval(feats)
    r2 = capi.Rvm(ctx, m2)
    lg2, _ = r2.eval(feats)
    assert np.array_equal(lg2, lo2) and lo2.max() == 4
    rg.close(); r2.close(); ro.close()


@pytest.mark.parametrize("space,scale,shift,pw,ph", [(1, 1.0, 0.0, 20, 20), (0, 1.0 / 255.0, 0.0, 24, 24), (2, 0.5, -3.0, 16, 24), (1, 1.0, 0.0, 19, 21)])
def test_rvm_sliding_window_detector(oracle, capi, ctx, synth, frame640, space, scale, shift, pw, ph):
    """SlidingWindowDetector + ProbabilisticRvmClassifier ("prvm") on the gray / hq64 / histeq feature spaces followed by
    ConversionFilter(CV_32F, scale, shift): every window's last level identical, distances to 1e-12, same detections."""
    kw = dict(octave_layers=2, min_scale=0.2, max_scale=0.4)
    small = np.ascontiguousarray(frame640[:240, :320])
    po = oracle.Pyramid(**kw); po.update(small)
    pg = capi.Pyramid(ctx, **kw); pg.update(small)
    layers = [po.layer(i) for i in range(len(po.layers()))]
    wins = po.windows(pw, ph, 2, 2)
    pat = np.stack([np.ascontiguousarray(layers[lp][ly:ly + ph, lx:lx + pw]) for lp, lx, ly, *_ in wins])
    if space == 1:
        pat = np.stack([oracle.histeq64(p_) for p_ in pat])
    elif space == 2:
        pat = np.stack([oracle.equalize_hist(p_) for p_ in pat])
    feats = pat.reshape(len(pat), -1).astype(np.float32) * np.float32(scale) + np.float32(shift)
    m = synth.make_rvm(3, feats[::3], pw, ph, n_filters=30, kernel=2)
    ro, rg = oracle.Rvm(m), capi.Rvm(ctx, m)
    lo, do = ro.eval(feats)
    dets, lg, dg = capi.detect_rvm(ctx, pg, rg, feature_space=space, conv_scale=scale, conv_shift=shift, sx=2, sy=2)
    assert len(lg) == len(lo) > 1000
    assert np.array_equal(lg, lo)
    assert np.allclose(dg, do, rtol=1e-12, atol=1e-300)
    pos = np.nonzero((lo == 29) & (do >= m["thresholds"][29]))[0]
    assert len(dets) == len(pos) > 0
    for dt, i in zip(dets, pos):
        assert (int(dt["layer"]), int(dt["lx"]), int(dt["ly"]), int(dt["cx"]), int(dt["cy"]), int(dt["w"]), int(dt["h"])) == tuple(int(v) for v in wins[i])
        assert abs(dt["probability"] - ro.probability(do[i])) <= 1e-12
    rg.close(); pg.close(); po.close(); ro.close()


def test_five_stage_batch_equals_single_calls(oracle, capi, ctx, synth, frame640, small_models):
    """fd_detect_five_stage_batch (all WVM stages queued first, host stages overlapped) returns exactly what the
    individual fd_detect_five_stage calls return; two detectors share a pyramid."""
    wvm, svm = small_models
    gray = oracle.bgr2gray(frame640)
    rng = np.random.default_rng(5)
    calib = synth.random_patches(gray[::2, ::2].copy(), 24, 24, 3000, rng)
    wvm2 = synth.make_wvm(77, fw=24, fh=24, n_per=10, n_levels=3, calib_patches=calib, min_survivors=48)
    eq = synth.histeq64_np(synth.random_patches(gray[::2, ::2].copy(), 24, 24, 400, rng))
    svm2 = synth.make_svm_u8(78, eq, nsv=256, calib=eq[256:])
    pA = capi.Pyramid(ctx, **FF); pA.update(frame640)
    pB = capi.Pyramid(ctx, inc=0.9, min_scale=0.3, max_scale=0.5); pB.update(frame640)
    dets = [(pA, capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)), (pB, capi.Wvm(ctx, wvm2), capi.Svm(ctx, svm2)), (pB, capi.Wvm(ctx, wvm), capi.Svm(ctx, svm))]
    single = [capi.detect_five_stage(ctx, p_, w_, s_) for p_, w_, s_ in dets]
    batch = capi.detect_five_stage_batch(ctx, dets)
    assert sum(len(d) for d, _ in single) > 0
    for (d1, st1), (d2, st2) in zip(single, batch):
        assert np.array_equal(st1, st2)
        assert d1.tobytes() == d2.tobytes()
    for p_, w_, s_ in dets:
        w_.close(); s_.close()
    pA.close(); pB.close()


def test_condensation_wvm_svm_model(oracle, capi, ctx, frame640, small_models):
    """condensation::WvmSvmModel::evaluate (particle-filter measurement model): samples -> single-patch windows
    (DirectPyramidFeatureExtractor::extract(x, y, w, h)) -> WVM for all, SVM for the 8 most probable positives."""
    wvm, svm = small_models
    po, pg = _pyr_pair(oracle, capi, ctx, frame640, **FF)
    wo, so = oracle.Wvm(wvm), oracle.Svm(svm)
    wg, sg = capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)
    rng = np.random.default_rng(12)
    n = 3000
    size = rng.integers(90, 460, n)                       # FaceFrontal layers cover patch widths of about 125..400 px
    samples = np.stack([rng.integers(-20, 660, n), rng.integers(-20, 500, n), size, size], 1).astype(np.int32)
    # dense cluster around WVM positives so that more than 8 samples survive the cascade
    pos, _, _ = oracle.sliding_wvm(po, wo, 1, 1)
    assert len(pos) > 8
    extra = np.array([[d["cx"], d["cy"], d["w"], d["h"]] for d in pos[:40]], np.int32)
    samples = np.concatenate([samples, extra, extra[:5]])
    to, wo_ = oracle.wvm_svm_evaluate(po, wo, so, samples)
    tg, wg_ = capi.wvm_svm_evaluate(ctx, pg, wg, sg, samples)
    assert np.array_equal(tg, to)
    assert np.allclose(wg_, wo_, rtol=1e-12, atol=0)
    valid = np.array([oracle.extract_single(po, 20, 20, *s_) is not None for s_ in samples])
    assert 100 < valid.sum() < len(samples) and np.all(wo_[~valid] == 0) and np.all(wo_[valid] > 0)
    assert 1 <= to.sum() <= 8
    # empty / all-invalid inputs
    t0, w0 = capi.wvm_svm_evaluate(ctx, pg, wg, sg, np.zeros((0, 4), np.int32))
    assert len(t0) == 0
    t1, w1 = capi.wvm_svm_evaluate(ctx, pg, wg, sg, np.array([[5, 5, 3000, 3000], [100, 100, 0, 0]], np.int32))
    assert not t1.any() and np.all(w1 == 0)
    wg.close(); sg.close(); pg.close()


def test_full_size_properties_config2_and_config3(oracle, capi, ctx, synth):
    """BASELINE full sizes, where the oracle is too slow to score every window: size-independent properties.
    Config 2 (640x480, 278,142 windows): window count, positives == {distance >= threshold} in extraction order, probability =
    logistic(distance), a second run is identical, and a strided sample of windows is checked against the oracle features + SVM.
    Config 3 shape (1080p): per-detector window counts add up to SURVEY App. D's 32,113,402; the FaceFrontal five-stage result is
    reproducible, stage counts are non-increasing, all boxes lie in the frame and the batch entry point agrees."""
    frame = synth.make_frame(640, 480, seed=31)
    kw = dict(octave_layers=5, min_scale=1 / 16, max_scale=1.0)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_layer_filter(1, bins=9)
    pg.update(synth.make_frame(640, 480, seed=32))
    hp = capi.hog_params(20, 20, 2, 2, 9, 5, 2, False)
    feats2 = capi.extract_hog(ctx, pg, hp)
    assert len(feats2) == 278142
    m = synth.make_svm_f32(6, feats2, nsv=1024, gamma=0.5, positive_fraction=0.01)
    sg = capi.Svm(ctx, m)
    pg.update(frame)
    dets, dist = capi.detect_hog_svm(ctx, pg, sg, hp)
    assert len(dist) == 278142
    pos = np.nonzero(dist >= float(np.float32(m["threshold"])))[0]
    assert len(dets) == len(pos) > 100
    wins = pg.windows(20, 20, 2, 2)
    assert np.array_equal(np.stack([dets["layer"], dets["lx"], dets["ly"]], 1), wins[pos][:, :3])
    so = oracle.Svm(m)
    assert np.allclose(dets["probability"], [so.probability(d) for d in dist[pos]], rtol=1e-12)
    dets2, dist2 = capi.detect_hog_svm(ctx, pg, sg, hp)
    assert np.array_equal(dist2, dist) and dets2.tobytes() == dets.tobytes()
    # strided sample against the oracle (features bit-exact, distances 1e-4 of the natural scale)
    po = oracle.Pyramid(**kw)
    po.set_layer_filter(1, bins=9)
    po.update(frame)
    layers = [po.layer(i) for i in range(len(po.layers()))]
    fg = capi.extract_hog(ctx, pg, hp)
    idx = np.arange(0, 278142, 997)
    fo = np.stack([oracle.hog_filter(np.ascontiguousarray(layers[wins[i][0]][wins[i][2]:wins[i][2] + 20, wins[i][1]:wins[i][1] + 20]), 9, 5, 2) for i in idx])
    assert np.array_equal(fg[idx], fo)
    do = so.distance(fo)
    assert np.max(np.abs(dist[idx] - do)) <= 1e-4 * np.abs(m["coeff"]).sum()
    sg.close(); pg.close(); po.close()

    # config 3 shape
    total = 0
    pyrs = {}
    for name, (inc, mn, mx, pw, ph, nper, nlev) in synth.DETECTOR_CFGS.items():
        key = (inc, mn, mx)
        if key not in pyrs:
            pyrs[key] = capi.Pyramid(ctx, inc=float(np.float32(inc)), min_scale=float(np.float32(mn)), max_scale=float(np.float32(mx)))
            pyrs[key].update(np.zeros((1080, 1920), np.uint8))
        total += pyrs[key].window_count(pw, ph, 1, 1)
    assert total == 32113402
    for p_ in pyrs.values():
        p_.close()
    gray = oracle.bgr2gray(synth.make_frame(640, 480, seed=20260927))
    calib = synth.random_patches(gray[::4, ::4].copy(), 20, 20, 8000, np.random.default_rng(1))
    wvm_m = synth.make_wvm(7, calib_patches=calib)
    eq = synth.histeq64_np(synth.random_patches(gray[::4, ::4].copy(), 20, 20, 1400, np.random.default_rng(2)))
    svm_m = synth.make_svm_u8(3, eq, nsv=1024, calib=eq[1024:])
    big = synth.make_frame(1920, 1080, seed=20260927)
    pA, pB = capi.Pyramid(ctx, **FF), capi.Pyramid(ctx, **FF)
    pA.update(big); pB.update(big)
    assert pA.window_count(20, 20, 1, 1) == 190616
    wA, wB, sv_ = capi.Wvm(ctx, wvm_m), capi.Wvm(ctx, wvm_m), capi.Svm(ctx, svm_m)
    d1, st1 = capi.detect_five_stage(ctx, pA, wA, sv_)
    d2, st2 = capi.detect_five_stage(ctx, pA, wA, sv_)
    assert d1.tobytes() == d2.tobytes() and np.array_equal(st1, st2)
    assert st1[0] >= st1[1] >= st1[2] >= st1[3] == len(d1) > 0
    assert np.all(d1["cx"] >= 0) and np.all(d1["cx"] < 1920) and np.all(d1["cy"] >= 0) and np.all(d1["cy"] < 1080)
    assert np.all(np.diff(d1["probability"]) <= 0)          # sorted by probability (FiveStageSlidingWindowDetector.cpp:316)
    (b1, bs1), (b2, bs2) = capi.detect_five_stage_batch(ctx, [(pA, wA, sv_), (pB, wB, sv_)])
    assert b1.tobytes() == d1.tobytes() and b2.tobytes() == d1.tobytes() and np.array_equal(bs1, st1) and np.array_equal(bs2, st1)
    # the WVM stage on a strided sample of the 190,616 windows against the oracle
    posw, lv, fo_ = capi.detect_wvm(ctx, pA, wA, 1, 1, want_all=True)
    po = oracle.Pyramid(**FF); po.update(big)
    wo = oracle.Wvm(wvm_m)
    layers = [po.layer(i) for i in range(len(po.layers()))]
    wins = po.windows(20, 20, 1, 1)
    for i in list(range(0, 190616, 1499)) + [int(d["level"]) * 0 + k for k, d in enumerate(posw[:0])]:
        lp, lx, ly = wins[i][:3]
        l_, f_ = wo.eval(oracle.histeq64(np.ascontiguousarray(layers[lp][ly:ly + 20, lx:lx + 20])))
        assert (l_, np.float32(f_)) == (lv[i], fo_[i]), i
    wA.close(); wB.close(); sv_.close(); pA.close(); pB.close(); po.close()


@pytest.mark.parametrize("cell,ub,ib,ic", [(8, 9, False, True), (8, 9, True, True), (4, 9, False, False), (6, 6, True, False), (5, 18, False, True)])
def test_fhog_filter_bit_exact(oracle, capi, ctx, frame640, cell, ub, ib, ic):
    """filtering::FhogFilter on gray (CV_8UC1) and BGR (CV_8UC3) images and on pyramid layers: descriptors bit-identical to the
    oracle (lane == cell walks its pixels in the reference's scan order; the gradient LUT is built with the host libm on both sides)."""
    gray = oracle.bgr2gray(frame640)
    for img in (gray, np.ascontiguousarray(gray[:97, :131]), np.ascontiguousarray(gray[:cell, :cell * 3]), np.ascontiguousarray(gray[:5, :300]),
                frame640, np.ascontiguousarray(frame640[:97, :131]), np.ascontiguousarray(frame640[:cell, :cell * 3])):
        fo = oracle.fhog(img, cell, ub, ib, ic, 0.2)
        fg = capi.fhog(ctx, gray=img, cell_size=cell, unsigned_bins=ub, interpolate_bins=ib, interpolate_cells=ic, alpha=0.2)
        assert fg.shape == fo.shape
        assert np.array_equal(fg, fo)
    kw = dict(octave_layers=3, min_scale=0.2, max_scale=1.0)
    po = oracle.Pyramid(**kw); po.update(frame640)
    pg = capi.Pyramid(ctx, **kw); pg.update(frame640)
    for li in (0, len(po.layers()) - 1):
        fo = oracle.fhog(po.layer(li), cell, ub, ib, ic, 0.35)
        fg = capi.fhog(ctx, pyramid=pg, layer=li, cell_size=cell, unsigned_bins=ub, interpolate_bins=ib, interpolate_cells=ic, alpha=0.35)
        assert fo.size > 0 and np.array_equal(fg, fo)
    pg.close(); po.close()


@pytest.mark.parametrize("cfg", [dict(size=(320, 240), win=(6, 6), cell=8, octl=5, ib=False, ic=True, minw=0, ws=1.0, hs=1.0, ch=3, nms=(0.3, 0)),
                                 dict(size=(400, 300), win=(5, 7), cell=6, octl=3, ib=True, ic=True, minw=80, ws=0.8, hs=1.1, ch=1, nms=(0.5, 2)),
                                 dict(size=(251, 333), win=(8, 4), cell=4, octl=4, ib=False, ic=False, minw=0, ws=1.0, hs=1.0, ch=3, nms=(0.4, 1))])
def test_aggregated_features_detector(oracle, capi, ctx, synth, cfg):
    """detection::AggregatedFeaturesDetector (GrayscaleFilter + FhogFilter feature pyramid, linear SVM as ConvolutionFilter, score
    threshold, window bounds, rescaleWindow, IoU NMS): candidates (scores included) and final detections identical to the oracle."""
    W, H = cfg["size"]
    frame = synth.make_frame(W, H, seed=77)
    img = frame if cfg["ch"] == 3 else oracle.bgr2gray(frame)
    ww, wh = cfg["win"]
    rng = np.random.default_rng(5)
    weights = rng.normal(0, 0.05, (wh, ww, 31)).astype(np.float32)
    # threshold: a high quantile of the scores of the full-resolution layer, so that a few hundred windows are positive
    sc0, _ = oracle.aggregated_candidates(img, weights, 0.1, -1e30, cell_size=cfg["cell"], interpolate_bins=cfg["ib"], interpolate_cells=cfg["ic"],
                                          octave_layers=cfg["octl"], min_window_width=cfg["minw"])
    thr = float(np.float32(np.quantile(sc0, 0.9)))
    kw = dict(cell_size=cfg["cell"], interpolate_bins=cfg["ib"], interpolate_cells=cfg["ic"], octave_layers=cfg["octl"], min_window_width=cfg["minw"],
              width_scale=cfg["ws"], height_scale=cfg["hs"])
    so, bo = oracle.aggregated_candidates(img, weights, 0.1, thr, **kw)
    det = capi.Aggregated(ctx, weights, 0.1, thr, nms_overlap=cfg["nms"][0], nms_type=cfg["nms"][1], **kw)
    fin, cand = det.detect(img)
    assert len(cand) == len(so) > 5
    assert np.array_equal(cand["score"], so)
    assert np.array_equal(np.stack([cand["x"], cand["y"], cand["w"], cand["h"]], 1), bo)
    fs, fb = oracle.nms_iou(so, bo, cfg["nms"][0], cfg["nms"][1])
    assert len(fin) == len(fs) > 0
    assert np.array_equal(fin["score"], fs) and np.array_equal(np.stack([fin["x"], fin["y"], fin["w"], fin["h"]], 1), fb)
    fin2, _ = det.detect(img)   # second frame of the same size reuses the pyramid
    assert fin2.tobytes() == fin.tobytes()
    det.close()


def test_aggregated_features_detector_image_size_changes(oracle, capi, ctx, synth):
    """an exact FHOG handle fed images of different sizes: first, second, first again.  Every call rebuilds the pyramid and the
    layer geometry (the code an approximated handle shares) and must give the oracle's candidates (scores and boxes) and final
    detections; the third call's bytes equal the first's; no layer is approximated.  A handle's threshold is fixed when it is
    created, so the sequence runs on two handles, one per image's threshold (the float32 0.9-quantile of that image's scores at all
    positions): each image is checked at its own threshold, where the oracle alone gives 46 of 453 and 18 of 172 positions as
    candidates and 18 and 7 detections, and at the other image's."""
    images = [synth.make_frame(176, 144, seed=77), synth.make_frame(131, 97, seed=77)]
    weights = np.random.default_rng(5).normal(0, 0.05, (4, 4, 31)).astype(np.float32)
    kw = dict(cell_size=8, octave_layers=2, min_window_width=0)
    thresholds = [float(np.float32(np.quantile(oracle.aggregated_candidates(img, weights, 0.1, -1e30, **kw)[0], 0.9))) for img in images]
    for own, thr in enumerate(thresholds):
        det = capi.Aggregated(ctx, weights, 0.1, thr, nms_overlap=0.3, nms_type=0, **kw)
        first = None
        for which in (0, 1, 0):
            so, bo = oracle.aggregated_candidates(images[which], weights, 0.1, thr, **kw)
            fs, fb = oracle.nms_iou(so, bo, 0.3, 0)
            fin, cand = det.detect(images[which])
            assert len(cand) == len(so) and (which != own or len(so) > 5)
            assert np.array_equal(cand["score"], so)
            assert np.array_equal(np.stack([cand["x"], cand["y"], cand["w"], cand["h"]], 1), bo)
            assert len(fin) == len(fs) and (which != own or len(fs) > 0)
            assert np.array_equal(fin["score"], fs) and np.array_equal(np.stack([fin["x"], fin["y"], fin["w"], fin["h"]], 1), fb)
            layers = det.layers()
            assert len(layers) >= 2 and not layers["approximated"].any()
            if first is None:
                first = (fin.tobytes(), cand.tobytes())
        assert (fin.tobytes(), cand.tobytes()) == first
        det.close()


def test_hog_rbf_svm_detector_config2(oracle, capi, ctx, synth):
    """BASELINE config 2 shape on a reduced frame: HOG-324 + RBF SVM (MFMA path).  Scores within
    1e-4 relative (of the natural scale sum|coeff_i| K_i), positives identical away from the threshold."""
    frame = synth.make_frame(320, 240, seed=11)
    frame2 = synth.make_frame(320, 240, seed=12)
    kw = dict(octave_layers=5, min_scale=1 / 16, max_scale=1.0)
    po = oracle.Pyramid(**kw)
    po.set_layer_filter(1, bins=9)
    po.update(frame2)
    _, _, feats2 = oracle.sliding_hog_svm(po, None, 20, 20, 2, 2, 9, 5, 2, want_feats=10 ** 9)
    m = synth.make_svm_f32(5, feats2, nsv=300, gamma=0.5, positive_fraction=0.02)   # 300: exercises SV padding to 512
    po.update(frame)
    so = oracle.Svm(m)
    dets_o, dist_o, _ = oracle.sliding_hog_svm(po, so, 20, 20, 2, 2, 9, 5, 2)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_layer_filter(1, bins=9)
    pg.update(frame)
    sg = capi.Svm(ctx, m)
    dets_g, dist_g = capi.detect_hog_svm(ctx, pg, sg, capi.hog_params())
    assert len(dist_g) == len(dist_o) and len(dist_o) % 64 != 0
    err = np.abs(dist_g - dist_o)
    scale = np.abs(m["coeff"]).sum()
    assert err.max() <= 1e-4 * max(1.0, np.abs(dist_o).max()), err.max()
    assert err.max() <= 1e-5 * scale
    safe = np.abs(dist_o - m["threshold"]) > 1e-4
    pos_o = np.nonzero((dist_o >= m["threshold"]))[0]
    pos_g = np.nonzero((dist_g >= m["threshold"]))[0]
    assert np.array_equal(pos_o[safe[pos_o]], pos_g[safe[pos_g]])
    assert len(pos_o) > 0
    if np.array_equal(pos_o, pos_g):
        _same_geometry(dets_g, dets_o)
        assert np.allclose(dets_g["probability"], dets_o["prob"], rtol=1e-4)
    sg.close(); pg.close()


def _fused_case(capi, ctx, synth, size, nsv):
    """a frame of that size in a gradient-bin pyramid and an RBF SVM of nsv support vectors on config 2's HOG shape:
    (frame, pyramid arguments, pyramid, model, model on the device)"""
    W, H = size
    frame = synth.make_frame(W, H, seed=31)
    kw = dict(octave_layers=5, min_scale=1 / 16, max_scale=1.0)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_layer_filter(1, bins=9)
    pg.update(synth.make_frame(W, H, seed=32))
    feats2 = capi.extract_hog(ctx, pg, capi.hog_params())
    if len(feats2) < nsv:   # tiny frames (a handful of windows, fewer than one tile of 32): support vectors from a larger frame's vectors
        pb = capi.Pyramid(ctx, **kw)
        pb.set_layer_filter(1, bins=9)
        pb.update(synth.make_frame(320, 240, seed=33))
        feats2 = capi.extract_hog(ctx, pb, capi.hog_params())
        pb.close()
    m = synth.make_svm_f32(7, feats2[:: max(1, len(feats2) // 4000)], nsv=nsv, gamma=0.5, positive_fraction=0.05)
    pg.update(frame)
    return frame, kw, pg, m, capi.Svm(ctx, m)


@pytest.mark.parametrize("size,nsv", [((160, 120), 100), ((320, 240), 300), ((333, 251), 1024), ((640, 480), 64), ((45, 37), 33), ((97, 22), 256)])
def test_hog_svm_fused_kernel_equals_the_two_kernel_path(oracle, capi, ctx, synth, size, nsv, monkeypatch):
    """config 2's shape runs as ONE kernel (hog_svm_fused.hpp: HOG vectors produced in the registers of the MFMA operand, support
    vectors streamed).  Against the two-kernel path (k_hog_tile -> features in HBM -> k_svm_rbf_mfma_svs, FD_HOG_FUSED=0) the HOG
    values are the same bits; |x|^2 (fp32) and the fp64 sum over support vectors are added in another order: distances within 2e-7 of sum|coeff|,
    the same positives away from the threshold.  The sizes cover a launch without a full round (the tail split over 2..32
    support-vector parts), full rounds + a tail, window counts that are not multiples of 32, and 2 / 16 / 32 support-vector tiles."""
    frame, kw, pg, m, sg = _fused_case(capi, ctx, synth, size, nsv)
    monkeypatch.setenv("FD_HOG_FUSED", "0")
    dets_2, dist_2 = capi.detect_hog_svm(ctx, pg, sg, capi.hog_params())
    monkeypatch.setenv("FD_HOG_FUSED", "1")
    dets_f, dist_f = capi.detect_hog_svm(ctx, pg, sg, capi.hog_params())
    dets_f2, dist_f2 = capi.detect_hog_svm(ctx, pg, sg, capi.hog_params())
    assert np.array_equal(dist_f, dist_f2) and np.array_equal(dets_f, dets_f2)        # deterministic
    assert len(dist_f) == len(dist_2) > 0
    scale = np.abs(m["coeff"]).sum()
    assert np.abs(dist_f - dist_2).max() <= 2e-7 * scale, np.abs(dist_f - dist_2).max()   # |x|^2 is an fp32 sum in another order
    safe = np.abs(dist_2 - m["threshold"]) > 1e-6 * scale
    pos_2, pos_f = np.nonzero(dist_2 >= m["threshold"])[0], np.nonzero(dist_f >= m["threshold"])[0]
    assert np.array_equal(pos_2[safe[pos_2]], pos_f[safe[pos_f]])
    # ... and against the oracle on a strided sample of the windows (the full-size comparison is test_gpu_fullsize's)
    po = oracle.Pyramid(**kw)
    po.set_layer_filter(1, bins=9)
    po.update(frame)
    if len(dist_f) <= 70000:
        _, dist_o, _ = oracle.sliding_hog_svm(po, oracle.Svm(m), 20, 20, 2, 2, 9, 5, 2)
        assert np.abs(dist_f - dist_o).max() <= 1e-5 * scale
    sg.close(); pg.close()


def test_every_window_of_every_scan_family_lands_where_the_oracle_enumerates_it(oracle, capi, ctx, synth, monkeypatch):
    """The numbering rule the window-scan families share (windows layer by layer in extraction order, a layer without windows
    shares its successor's first index, a tile's tail repeats the last window), for EVERY window: with thresholds no window can
    miss, the detections of the HOG (fused and two-kernel), histogram, whi and RVM detectors are the oracle's window list, row by
    row.  96 x 72 at two layers per octave: layers 96x72, 68x51, 48x36, 34x26, 24x18 hold 988 / 384 / 112 / 21 / 0 windows of
    20 x 20 at step 2 -- a trailing empty layer, and 32-window tiles that straddle every layer boundary (988 % 32 = 28); the RVM
    with a roi sees 50 / 4 / 0 / 0 / 0."""
    frame = synth.make_frame(96, 72, seed=11)
    kw = dict(octave_layers=2, min_scale=0.25, max_scale=1.0)
    po, pg = _pyr_pair(oracle, capi, ctx, frame, **kw)
    assert [(L["w"], L["h"]) for L in po.layers()] == [(96, 72), (68, 51), (48, 36), (34, 26), (24, 18)]
    wins = po.windows(20, 20, 2, 2)
    assert np.bincount(wins[:, 0], minlength=5).tolist() == [988, 384, 112, 21, 0]
    pb = capi.Pyramid(ctx, **kw)   # the gradient-bin pyramid of the HOG and histogram runs
    pb.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9)
    pb.update(frame)

    def rows(dets):   # the oracle's columns
        return np.stack([dets[f] for f in ("layer", "lx", "ly", "cx", "cy", "w", "h")], 1).astype(np.int32)

    def same(dets, expect):
        assert len(dets) == len(expect)
        assert np.array_equal(rows(dets), expect)

    rng = np.random.default_rng(17)

    def svm_all_positive(dim):   # an RBF distance is bounded by sum|coeff| + |bias|: -1e30 lies below every one
        return capi.Svm(ctx, dict(kernel=2, dtype=1, sv=rng.random((64, dim)).astype(np.float32), coeff=rng.normal(0, 1, 64).astype(np.float32),
                                  bias=np.float32(0.1), p0=0.5, p1=0.0, p2=0.0, threshold=-1e30, logistic_a=0.0, logistic_b=-1.0))

    s324, s400 = svm_all_positive(324), svm_all_positive(400)
    same(capi.detect_hog_svm(ctx, pb, s324, capi.hog_params())[0], wins)            # the fused 20/5/2/9 shape
    monkeypatch.setenv("FD_HOG_FUSED", "0")
    same(capi.detect_hog_svm(ctx, pb, s324, capi.hog_params())[0], wins)            # k_hog_tile + the selection kernel
    monkeypatch.delenv("FD_HOG_FUSED")
    same(capi.detect_hist_svm(ctx, pb, s324, capi.hist_params(kind=0, block=2))[0], wins)
    same(capi.detect_whi_svm(ctx, pg, s400, capi.whi_params())[0], wins)
    m = synth.make_rvm(3, rng.integers(0, 256, (64, 400)).astype(np.float32), 20, 20, n_filters=20)   # 20 levels: the passes and the deep kernel
    m["thresholds"][:] = -1e30
    rg = capi.Rvm(ctx, m)
    same(capi.detect_rvm(ctx, pg, rg, sx=2, sy=2)[0], wins)
    roi = (30, 20, 40, 30)
    wroi = po.windows(20, 20, 2, 2, roi)
    assert np.bincount(wroi[:, 0], minlength=5).tolist() == [50, 4, 0, 0, 0]
    same(capi.detect_rvm(ctx, pg, rg, sx=2, sy=2, roi=roi)[0], wroi)
    rg.close(); s324.close(); s400.close(); pb.close(); pg.close(); po.close()


@pytest.mark.parametrize("size,nsv", [((45, 37), 33), ((97, 22), 256)])
def test_hsf_subs_is_gone(capi, ctx, synth, size, nsv, monkeypatch):
    """k_hog_svm_fused has one body.  FD_HSF_SUBS used to pick one of three per call, unvalidated: 0 returned garbage, 2 a variant no
    test ran, anything else the default body with the LDS sized for another.  Whatever it is set to, distances and detections are
    now the bytes of a run without it."""
    monkeypatch.delenv("FD_HOG_FUSED", raising=False)
    monkeypatch.delenv("FD_HSF_SUBS", raising=False)
    _, _, pg, _, sg = _fused_case(capi, ctx, synth, size, nsv)
    dets, dist = capi.detect_hog_svm(ctx, pg, sg, capi.hog_params())
    assert len(dist) > 0
    for value in ("0", "2", "7"):
        monkeypatch.setenv("FD_HSF_SUBS", value)
        dets_v, dist_v = capi.detect_hog_svm(ctx, pg, sg, capi.hog_params())
        assert dist_v.tobytes() == dist.tobytes() and dets_v.tobytes() == dets.tobytes(), value
    sg.close(); pg.close()


def test_selected_positives_are_exactly_the_windows_at_or_above_the_threshold(oracle, capi, ctx, synth, monkeypatch):
    """k_select_positives (the two-kernel HOG path, the histogram and the whi detectors) appends a wavefront's positives with one
    atomic: every lane of a wavefront has to reach the ballot, with the windows behind the last one voting no.  The 96 x 72 frame of
    the scan-family test has 1505 windows: 23 full wavefronts and one of 33 lanes.  Thresholds come from a run's own distances -- the
    largest float below or at the minimum, the median rounded to float, the smallest float above the maximum -- and the decision is
    re-derived from the distances the same run returned, so there is no tolerance: the detections are the oracle's window rows at
    nonzero(distance >= threshold), every window once, none twice, all of them / half of them / none (an empty ballot in every
    wavefront).  "Half": the 753 distances from the median up, or 752 when the float threshold lies just above the median; the
    models' gamma is 1 / (median squared distance between feature vectors), so neighbouring distances are many float steps apart."""
    frame = synth.make_frame(96, 72, seed=11)
    kw = dict(octave_layers=2, min_scale=0.25, max_scale=1.0)
    po, pg = _pyr_pair(oracle, capi, ctx, frame, **kw)
    wins = po.windows(20, 20, 2, 2)
    n = len(wins)
    assert n == 1505 and n % 64 == 33
    pb = capi.Pyramid(ctx, **kw)
    pb.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9)
    pb.update(frame)
    monkeypatch.setenv("FD_HOG_FUSED", "0")
    hist = capi.hist_params(kind=0, block=2)
    families = [(capi.extract_hog(ctx, pb, capi.hog_params()), lambda s: capi.detect_hog_svm(ctx, pb, s, capi.hog_params(), want_all=True)),
                (capi.extract_hist(ctx, pb, hist), lambda s: capi.detect_hist_svm(ctx, pb, s, hist, want_all=True)),
                (capi.extract_whi(ctx, pg, capi.whi_params()), lambda s: capi.detect_whi_svm(ctx, pg, s, capi.whi_params(), want_all=True))]
    for which, (feats, detect) in enumerate(families):
        assert len(feats) == n
        sub = feats[::16].astype(np.float64)
        d2 = (sub ** 2).sum(1)[:, None] + (sub ** 2).sum(1)[None, :] - 2 * sub @ sub.T
        m = synth.make_svm_f32(41 + which, feats, nsv=64, gamma=1.0 / np.median(d2[d2 > 0]))

        def run(threshold):
            s = capi.Svm(ctx, dict(m, threshold=threshold))
            dets, dist = detect(s)
            s.close()
            rows = np.stack([dets[f] for f in ("layer", "lx", "ly", "cx", "cy", "w", "h")], 1).astype(np.int32)
            return rows, dist

        _, dist0 = run(np.float32(-1e30))
        lo, mid, hi = np.float32(dist0.min()), np.float32(np.median(dist0)), np.float32(dist0.max())
        lo = lo if lo <= dist0.min() else np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf)) if hi <= dist0.max() else hi
        for thr, counts in ((lo, (n,)), (mid, (n // 2, n // 2 + 1)), (hi, (0,))):
            rows, dist = run(thr)
            pos = np.nonzero(dist >= np.float64(thr))[0]
            assert len(pos) in counts, (which, thr, len(pos))
            assert np.array_equal(rows, wins[pos]), (which, thr)
    pb.close(); pg.close(); po.close()


def test_sdm_descriptors_bit_exact(oracle, capi, ctx, synth):
    gray = synth.make_frame(256, 256, seed=21, channels=1)
    rng = np.random.default_rng(1)
    px = rng.uniform(40, 216, 40).astype(np.float32)
    py = rng.uniform(40, 216, 40).astype(np.float32)
    # points whose window crosses the left/top border use the zero-extended image (where the quirk allows)
    px[:4] = [3.2, 8.5, 5.5, 200.4]
    py[:4] = [100.0, 120.5, 60.5, 150.0]
    for wsh in (12, 15, 21, 33):
        do = oracle.sdm_descriptors(gray, px, py, wsh)
        assert do is not None
        dg = capi.sdm_descriptors(ctx, gray, px, py, wsh)
        assert dg.shape == do.shape == (40, 279)
        assert np.array_equal(dg, do), wsh
    do = oracle.sdm_descriptors(gray, px[4:], py[4:], 0, variant=0, num_cells=3, cell_size=8, num_bins=4)
    dg = capi.sdm_descriptors(ctx, gray, px[4:], py[4:], 0, variant=0, num_cells=3, cell_size=8, num_bins=4)
    assert np.array_equal(dg, do)


@pytest.mark.parametrize("geometry", [(4, 10, 9, 1), (6, 8, 5, 0), (2, 20, 9, 1), (5, 6, 16, 0), (1, 4, 9, 1), (3, 16, 9, 1)])
def test_sdm_descriptors_of_every_working_image_shape(oracle, capi, ctx, synth, geometry):
    """The extractor's own geometry (non-adaptive: VlHogDescriptorExtractor(numCells, cellSize, numBins), DescriptorExtractor.hpp:128-215)
    on the shapes the adaptive 30x30 image never reaches: working images of 40 and 48 pixels (64-bit orientation masks, magnitudes in
    their own LDS block, the generic resize-free path), cells of 20 pixels, 16 orientations, one cell -- the
    voting by (orientation, cell column) lanes with sliding cell-row accumulators has to give hog.c's sums on all of them."""
    nc, cs, nb, variant = geometry
    gray = synth.make_frame(256, 256, seed=23, channels=1)
    rng = np.random.default_rng(5)
    half = nc * (cs // 2)
    px = rng.uniform(half + 2, 253 - half, 24).astype(np.float32)
    py = rng.uniform(half + 2, 253 - half, 24).astype(np.float32)
    do = oracle.sdm_descriptors(gray, px, py, 0, variant=variant, num_cells=nc, cell_size=cs, num_bins=nb)
    assert do is not None
    dg = capi.sdm_descriptors(ctx, gray, px, py, 0, variant=variant, num_cells=nc, cell_size=cs, num_bins=nb)
    assert dg.shape == do.shape and np.array_equal(dg, do), geometry


def test_sdm_fit_batch(oracle, capi, ctx, synth):
    """68 landmarks, 4 cascade steps (BASELINE config 4 shape, reduced batch).  Landmarks within 1e-4 relative."""
    model = synth.make_sdm(9, L=68, S=4)
    B = 6
    imgs = np.stack([synth.make_frame(256, 256, seed=100 + i, channels=1) for i in range(B)])
    boxes = np.array([[48, 48, 160, 160]] * B, np.int32)
    boxes[1] = [40, 56, 150, 170]
    sg = capi.Sdm(ctx, model)
    shapes, status = sg.fit(imgs, boxes)
    for i in range(B):
        st, ref = oracle.sdm_fit(imgs[i], model, boxes[i])
        assert st == 0 and status[i] == 0
        assert np.allclose(shapes[i], ref, rtol=1e-4, atol=1e-4), np.abs(shapes[i] - ref).max()
    # R = 0 returns the rigidly aligned mean (SURVEY.md App. C invariant)
    zero = dict(model)
    zero["R"] = [np.zeros_like(r) for r in model["R"]]
    s0, _ = capi.Sdm(ctx, zero).fit(imgs[:1], boxes[:1])
    _, r0 = oracle.sdm_fit(imgs[0], zero, boxes[0])
    assert np.array_equal(s0[0], r0)
    # fd_sdm_fit_batch_begin / _end: four batches of different content queued by one host thread, collected out of order -- the same
    # shapes as the blocking calls (each ticket owns its scratch set; consecutive tickets run on alternating streams)
    batches = [(imgs[k:k + 3], boxes[k:k + 3]) for k in (0, 3, 1, 2)]
    ref = [sg.fit(*b) for b in batches]
    tickets = [sg.fit_begin(*b) for b in batches]
    for k in (2, 0, 3, 1):
        sh, st = sg.fit_end(tickets[k])
        assert np.array_equal(sh, ref[k][0]) and np.array_equal(st, ref[k][1]), k
    sg.close()


def test_sdm_real_regressors(oracle, capi, ctx, synth):
    """VERDICT r04 task 2: the reference's real trained regressors (SDM_Model_HOG_Zhenhua_11012014.txt re-packed by
    tests/golden/make_sdm_real.py; coefficients ~5e-2, landmarks move 5-15 px per step) through fd_sdm_fit_batch, all 5 steps, on the
    32 seeded crops of the fixture.  Tolerance: 1e-4 relative per landmark coordinate (north_star).  Descriptors of every step at the
    oracle's landmark positions are bit-identical to the reference's own hog.c (the committed ref_desc arrays)."""
    import importlib.util
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_sdm_real", os.path.join(G, "make_sdm_real.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = np.load(os.path.join(G, "sdm_real_11012014.npz"))
    model = mod.unpack_model(g)
    L, S, B = model["L"], model["S"], int(g["nfaces"])
    imgs = np.stack([synth.make_frame(256, 256, seed=int(g["frame_seed0"]) + i, channels=1) for i in range(B)])
    boxes = np.tile(g["face_box"].astype(np.int32), (B, 1))
    sg = capi.Sdm(ctx, model)
    shapes, status = sg.fit(imgs, boxes)
    assert not status.any()
    ref = g["oracle_shapes"][:, S]
    err = np.abs(shapes - ref) / np.maximum(np.abs(ref), 1.0)
    assert err.max() <= 1e-4, (err.max(), np.argwhere(err > 1e-4)[:5])
    # every intermediate step as well (prefix models): a cvRound(landmark) that flipped at step s would show here first
    for s in range(1, S):
        sub = dict(model, S=s, R=model["R"][:s], desc_params=model["desc_params"][:3 * s])
        sh, st = capi.Sdm(ctx, sub).fit(imgs, boxes)
        ref_s = g["oracle_shapes"][:, s]
        e = np.abs(sh - ref_s) / np.maximum(np.abs(ref_s), 1.0)
        assert not st.any() and e.max() <= 1e-4, (s, e.max())
    # live oracle on two faces (the committed shapes are its output in the build container)
    for f in (3, 29):
        st, r = oracle.sdm_fit(imgs[f], model, boxes[f])
        assert st == 0 and np.array_equal(r, ref[f])
    # descriptors of every step: HIP kernel == the reference's hog.c
    for f in (0, 17):
        for s in range(S):
            nc, cp, nb = [int(v) for v in model["desc_params"][3 * s:3 * s + 3]]
            shp = g["oracle_shapes"][f, s]
            d = capi.sdm_descriptors(ctx, imgs[f], shp[:L].copy(), shp[L:].copy(), 0, variant=1, num_cells=nc, cell_size=cp, num_bins=nb)
            assert np.array_equal(d, g["ref_desc_f%d_s%d" % (f, s)]), (f, s)
    sg.close()
    # a model whose rows do not fit its descriptor parameters is refused (the reference's gemm would assert)
    bad = dict(model, desc_params=np.array([3, 3, 4] * S, np.int32))
    with pytest.raises(capi.FdError):
        capi.Sdm(ctx, bad)


def test_pyramid_updated_again_and_again_is_bit_exact(oracle, capi, ctx, synth):
    """One pyramid object updated twelve times -- host images and device-resident images at changing addresses, a change of the frame size
    and back, a gray pyramid and one with gradient-bin layers: every update gives the oracle's layers bit for bit (nothing of an earlier
    update survives in the arena or the tables).  (Written for round 5's hipGraph replay of the update, which was measured and dropped.)"""
    import torch
    for kw, filt in ((dict(inc=float(np.float32(0.92)), min_scale=float(np.float32(0.05)), max_scale=float(np.float32(0.16))), False),
                     (dict(octave_layers=3, min_scale=0.25, max_scale=1.0), True)):
        pg, po = capi.Pyramid(ctx, **kw), oracle.Pyramid(**kw)
        if filt:
            pg.set_layer_filter(kind=1, bins=9)
            po.set_layer_filter(kind=1, bins=9)
        sizes = [(640, 480)] * 5 + [(320, 240)] * 4 + [(640, 480)] * 3
        keep = []
        for i, (W, H) in enumerate(sizes):
            fr = synth.make_frame(W, H, seed=900 + i)
            if i % 2 == 0:
                pg.update(fr)                                   # host image: staged in the pyramid's input buffer
            else:
                t = torch.from_numpy(fr).cuda()                 # device image at a new address every time
                keep.append(t)
                pg.update_device(t.data_ptr(), W, H, 3)
            po.update(fr)
            lg, lo = pg.layers(), po.layers()
            assert len(lg) == len(lo) > 0
            for k in range(len(lo)):
                assert np.array_equal(pg.layer(k), po.layer(k)), (filt, i, k)   # (the filtered layer when the pyramid has a layer filter)
        pg.close()


def test_errors_are_reported_not_swallowed(capi, ctx):
    with pytest.raises(capi.FdError) as e:
        capi.Pyramid(ctx, octave_layers=0, min_scale=0.1, max_scale=1.0)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError):
        capi.Pyramid(ctx, octave_layers=3, min_scale=0.1, max_scale=1.5)
    p = capi.Pyramid(ctx, octave_layers=3, min_scale=0.5, max_scale=1.0)
    with pytest.raises(capi.FdError):
        p.window_count(20, 20, 0, 1)  # stepX has to be greater than zero
    p.update(np.zeros((8, 8), np.uint8))
    assert p.window_count(20, 20, 1, 1) == 0  # image smaller than the patch: no windows, no error
    p.close()


def test_error_paths_of_the_later_entry_points(capi, ctx, synth):
    """invalid arguments of the FHOG / aggregated / NMS / RVM / histogram entry points come back as status codes + messages"""
    gray = np.zeros((40, 40), np.uint8)
    with pytest.raises(capi.FdError) as e:
        capi.fhog(ctx, gray=np.zeros((40, 40, 2), np.uint8))   # neither CV_8UC1 nor CV_8UC3
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "CV_8UC" in str(e.value)
    with pytest.raises(capi.FdError):
        capi.fhog(ctx, gray=gray, cell_size=0)
    with pytest.raises(capi.FdError):
        capi.fhog(ctx, gray=gray, unsigned_bins=0)
    with pytest.raises(capi.FdError):
        capi.fhog(ctx, gray=gray, unsigned_bins=19)    # more than 36 signed bins: backend limit, reported
    with pytest.raises(capi.FdError):
        capi.fhog(ctx, gray=gray, alpha=0.0)
    assert capi.fhog(ctx, gray=np.zeros((5, 40), np.uint8)).shape == (0, 5, 31)   # image lower than a cell: empty descriptor map
    wts = np.zeros((4, 4, 31), np.float32)
    with pytest.raises(capi.FdError):
        capi.Aggregated(ctx, wts, 0.0, 0.0, octave_layers=0)
    det = capi.Aggregated(ctx, wts, 0.0, 0.0, cell_size=8)
    with pytest.raises(capi.FdError):
        det.detect(np.zeros((33, 33, 3), np.uint8))   # one pyramid layer only: the score pyramid cannot estimate its lambdas
    det.close()
    boxes = np.zeros(3, capi.BOX_DTYPE)
    boxes["w"] = boxes["h"] = 10
    with pytest.raises(capi.FdError):
        capi.nms_iou(boxes, 1.5)   # overlap threshold above 1: no cluster ever forms, the reference would spin
    pg = capi.Pyramid(ctx, octave_layers=2, min_scale=0.5, max_scale=1.0)
    pg.set_layer_filter(1, bins=9)
    pg.update(synth.make_frame(96, 80, seed=1))
    with pytest.raises((capi.FdError, ValueError)):
        capi.extract_hist(ctx, pg, capi.hist_params(kind=0, pw=20, ph=20, bins=9, cell=5, block=9))   # block larger than the cell grid
    pg.close()


def test_golden_next_rows_fixture(capi, ctx):
    """Committed oracle vectors of the SURVEY 8(f) rows (tests/golden/orc_next_rows_128x96.npz): FHOG on gray / BGR images and the
    aggregated detector bit-exact, RVM levels exact and distances to 1e-12, whitening chain to 1e-6, equalizeHist exact."""
    g = np.load(os.path.join(G, "orc_next_rows_128x96.npz"))
    frame = g["frame"]
    pg = capi.Pyramid(ctx, octave_layers=2, min_scale=0.4, max_scale=0.8)
    pg.update(frame)
    gray = g["gray"]
    assert np.array_equal(capi.fhog(ctx, gray=gray), g["fhog_gray"])
    assert np.array_equal(capi.fhog(ctx, gray=frame), g["fhog_bgr"])
    assert np.array_equal(capi.fhog(ctx, gray=gray, cell_size=4, unsigned_bins=6, interpolate_bins=True, interpolate_cells=False), g["fhog_gray_c4_b6_ib"])
    det = capi.Aggregated(ctx, g["agg_weights"], 0.05, float(g["agg_threshold"]), cell_size=8, octave_layers=4, nms_overlap=0.3, nms_type=0)
    fin, cand = det.detect(frame)
    assert np.array_equal(cand["score"], g["agg_cand_scores"])
    assert np.array_equal(np.stack([cand["x"], cand["y"], cand["w"], cand["h"]], 1), g["agg_cand_boxes"])
    assert np.array_equal(fin["score"], g["agg_final_scores"])
    assert np.array_equal(np.stack([fin["x"], fin["y"], fin["w"], fin["h"]], 1), g["agg_final_boxes"])
    det.close()
    m = {k[5:]: g[k] for k in g.files if k.startswith("rvm__")}
    for k in ("kernel", "filter_w", "filter_h", "num_used"):
        m[k] = int(m[k])
    for k in ("p0", "p1", "p2", "logistic_a", "logistic_b", "bias"):
        m[k] = float(m[k])
    rg = capi.Rvm(ctx, m)
    dets, lg, dg = capi.detect_rvm(ctx, pg, rg, feature_space=1, conv_scale=1.0, conv_shift=0.0, sx=2, sy=2)
    assert np.array_equal(lg, g["rvm_level"])
    assert np.allclose(dg, g["rvm_dist"], rtol=1e-12, atol=1e-12 * float(np.abs(g["rvm_dist"]).max()))
    rg.close()
    assert np.array_equal(capi.equalize_hist_batch(ctx, g["whi_patches"]), g["eqhist_out"])
    assert np.allclose(capi.whi_batch(ctx, g["whi_patches"], 1.0, 0.390625), g["whi_out"], rtol=1e-6, atol=1e-9)
    pg.close()


def test_five_stage_batch_in_two_halves_with_two_frames_in_flight(oracle, capi, ctx, synth, frame640, small_models):
    """fd_five_stage_batch_begin / _end: the cascades of a second frame (its own pyramid and handles) are queued before the
    first frame's host stages run; both frames return exactly the oracle's detections."""
    wvm, svm = small_models
    frames = [frame640, synth.make_frame(640, 480, seed=424242)]
    sets, exp = [], []
    for f in frames:
        po = oracle.Pyramid(**FF); po.update(f)
        exp.append(oracle.five_stage(po, oracle.Wvm(wvm), oracle.Svm(svm), 5.0, 0.0, 1, 1, None))
        sets.append((capi.Pyramid(ctx, **FF), capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)))
        po.close()
    import torch
    dfr = [torch.from_numpy(f).cuda() for f in frames]
    b0 = capi.FiveStageBatch(ctx, [sets[0]], device_frames=[(dfr[0].data_ptr(), 640, 480, 3)])
    b1 = capi.FiveStageBatch(ctx, [sets[1]], device_frames=[(dfr[1].data_ptr(), 640, 480, 3)])
    for b, (do, sto) in ((b0, exp[0]), (b1, exp[1])):
        (dg, stg), = b.end()
        assert np.array_equal(stg, sto)
        _same_geometry(dg, do)
        assert np.array_equal(dg["probability"], do["prob"])
    with pytest.raises(capi.FdError):
        capi.FiveStageBatch(ctx, [sets[0], sets[0]])   # two jobs sharing a WVM handle
    for p_, w_, s_ in sets:
        w_.close(); s_.close(); p_.close()


def test_wvm_model_validation(capi, ctx, synth):
    """fd_wvm_create rejects models whose offset tables are not ascending or point past the stated array lengths (a truncated or
    corrupt model file must not turn into out-of-bounds reads)."""
    m = synth.make_wvm(5, n_per=4, n_levels=5)
    capi.Wvm(ctx, m).close()
    bad = dict(m); bad["val_off"] = m["val_off"].copy(); bad["val_off"][3] = bad["val_off"][2]
    with pytest.raises(capi.FdError) as e:
        capi.Wvm(ctx, bad)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    bad = dict(m); bad["rec_off"] = m["rec_off"].copy(); bad["rec_off"][-1] += 7    # past the rects array
    with pytest.raises(capi.FdError):
        capi.Wvm(ctx, bad)
    bad = dict(m); bad["val"] = m["val"][:-3]                                       # truncated grey values
    with pytest.raises(capi.FdError):
        capi.Wvm(ctx, bad)
