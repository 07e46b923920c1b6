"""FPDW channel features on the device (fd_fpdw_image, fd_fpdw_cells_image, capi.Aggregated(features="fpdw")) against the CPU model
of tests/fpdw_model.py.

What comes out of the look-up table -- which bin channel(s) of a pixel are non-zero -- is identical.  The values are compared
with the model's float64 results by the bounds of fpdw_model: relative 2 N 2^-24 for the bin and magnitude channels (N float32
roundings on the kernel's longest summation path, 76 at cell = radius = 8: 9.1e-6, below the 2e-5 the reference's own running
sums drift), absolute for L*u*v*.  Every test prints its largest error in units of its bound."""

import numpy as np
import pytest

import aggregated_approx_model as approx
import fpdw_model as model

pytestmark = pytest.mark.gpu

SIZES = [(37, 29), (64, 48), (131, 67)]
CELL_RADIUS = [(4, 4), (5, 5), (8, 8), (4, 0)]
CONTENTS = ["frame", "flat", "saturated", "ramp"]


def _content(synth, kind, w, h):
    if kind == "frame":
        return synth.make_frame(w, h, seed=w + h)
    if kind == "flat":
        return np.full((h, w, 3), 128, np.uint8)
    if kind == "saturated":   # one channel saturated, a black quarter
        img = synth.make_frame(w, h, seed=w + h + 1).copy()
        img[:, :, 2] = 255
        img[:h // 2, :w // 2] = 0
        return img
    # diagonal ramps: central differences of 4 in both directions, gradient codes (129, 129) above and (125, 129) below: exact
    # 45 and 135 degree ties
    y, x = np.mgrid[0:h, 0:w]
    top = np.clip(2 * (x + y), 0, 255)
    bottom = np.clip(2 * (y - x) + 200, 0, 255)
    ramp = np.where(y < h // 2, top, bottom).astype(np.uint8)
    return np.stack([ramp, ramp, ramp], 2)


@pytest.mark.parametrize("cell,radius", CELL_RADIUS, ids=["c%d-r%d" % cr for cr in CELL_RADIUS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_standalone_parity(oracle, capi, ctx, synth, size, cell, radius):
    w, h = size
    worst_px, worst_cell = 0.0, 0.0
    for kind in CONTENTS:
        img = _content(synth, kind, w, h)
        for fast in (True, False):
            for interp in (False, True):
                p = model.params(cell, radius, fast, interp)
                exact, _ = model.features_image(oracle, img, p)
                kw = dict(cell_size=cell, fast_gradient=fast, interpolate_bins=interp, normalization_radius=radius)
                got = capi.fpdw_image(ctx, img, **kw)
                what = "%s fast=%d interp=%d" % (kind, fast, interp)
                assert got.shape == exact.shape == (h, w, model.CHANNELS)
                # the bin channel(s) a pixel votes for come from the look-up table: identical
                assert np.array_equal(got[:, :, :model.BINS] != 0, exact[:, :, :model.BINS] != 0), what
                ok, ratio = model.within(got, exact, *model.pixel_bounds(p))
                worst_px = max(worst_px, ratio)
                assert ok, "%s: per-pixel error %.3f of the bound" % (what, ratio)
                if kind == "flat":
                    assert not got[:, :, :model.BINS + 1].any()
                cells = capi.fpdw_cells_image(ctx, img, **kw)
                exact_cells = model.aggregate(exact, cell)
                assert cells.shape == exact_cells.shape == (h // cell, w // cell, model.CHANNELS)
                assert np.array_equal(cells[:, :, :model.BINS] != 0, exact_cells[:, :, :model.BINS] != 0), what
                ok, ratio = model.within(cells, exact_cells, *model.cell_bounds(p))
                worst_cell = max(worst_cell, ratio)
                assert ok, "%s: cell error %.3f of the bound" % (what, ratio)
    print("largest error / bound: per pixel %.3f, cells %.3f (rtol %.2e)" % (worst_px, worst_cell, model.rtol(cell, radius)))


def test_images_below_the_filter_limits(capi, ctx, synth):
    img = synth.make_frame(40, 8, seed=1)
    with pytest.raises(capi.FdError) as e:   # the normaliser: rows <= radius
        capi.fpdw_image(ctx, img, cell_size=8, normalization_radius=8)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    assert "TriangularConvolutionFilter: image must have at least 9 rows, but had only 8" in str(e.value)
    img = synth.make_frame(17, 30, seed=1)
    with pytest.raises(capi.FdError) as e:   # cols < 2 radius + 2
        capi.fpdw_image(ctx, img, cell_size=8, normalization_radius=8)
    assert "TriangularConvolutionFilter: image must have at least 18 columns, but had only 17" in str(e.value)
    img = synth.make_frame(15, 30, seed=1)
    assert capi.fpdw_image(ctx, img, cell_size=8, normalization_radius=0).shape == (30, 15, 10)   # no normaliser, no limit
    with pytest.raises(capi.FdError) as e:   # the aggregation filter: radius cell - 1
        capi.fpdw_cells_image(ctx, img, cell_size=8, normalization_radius=0)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    assert "TriangularConvolutionFilter: image must have at least 16 columns, but had only 15" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        capi.fpdw_cells_image(ctx, img, cell_size=0)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "cellSize must be bigger than zero" in str(e.value)
    with pytest.raises(capi.FdError) as e:
        capi.fpdw_image(ctx, img, cell_size=4, normalization_constant=0.0)
    assert "normalizationConstant must be bigger than zero" in str(e.value)


# ---- the detector ----------------------------------------------------------------------------------------------------------------
CONFIGS = [
    dict(n=2, size=(320, 240), window_w=4, window_h=5, cell=4, min_window_width=0, seed=16),
    dict(n=3, size=(333, 217), window_w=4, window_h=5, cell=4, min_window_width=0, seed=29),
    dict(n=4, size=(640, 480), window_w=8, window_h=8, cell=8, min_window_width=0, seed=1),
]
IDS = ["n%d-%dx%d-c%d" % (c["n"], c["size"][0], c["size"][1], c["cell"]) for c in CONFIGS]
FIXED_LAMBDAS = np.concatenate([np.linspace(0.05, 0.3, 6), [0.11, 0.0, 0.02, -0.03]])


def _image(synth, cfg, seed=77):
    return synth.make_frame(cfg["size"][0], cfg["size"][1], seed=seed)


def _weights(cfg):
    return np.random.default_rng(cfg["seed"]).normal(0, 0.05, (cfg["window_h"], cfg["window_w"], model.CHANNELS)).astype(np.float32)


def _detector(capi, ctx, cfg, bias, thr, approximate, lambdas=None, **kw):
    return capi.Aggregated(ctx, _weights(cfg), bias, thr, cell_size=cfg["cell"], octave_layers=cfg["n"], min_window_width=cfg["min_window_width"],
                           approximate=approximate, lambdas=lambdas, features="fpdw", **kw)


_MODEL = {}


def _model_layers(oracle, synth, ci, approximate, lambdas_key):
    """(layers, feature maps, lambdas) of CONFIGS[ci], computed once; lambdas_key: None (exact / estimated) or "fixed\""""
    key = (ci, approximate, lambdas_key)
    if key not in _MODEL:
        cfg = CONFIGS[ci]
        lam = FIXED_LAMBDAS if lambdas_key == "fixed" else None
        _MODEL[key] = model.feature_layers(oracle, _image(synth, cfg), cfg, model.params(cfg["cell"]), approximate, lam)
    return _MODEL[key]


def _same_layers(got, want):
    assert len(got) == len(want)
    for g, m in zip(got, want):
        assert (int(g["index"]), int(g["approximated"]), int(g["parent"]), int(g["rows"]), int(g["cols"])) == \
               (m["index"], m["approximated"], m["parent"], m["rows"], m["cols"])
        assert (float(g["scale"]), float(g["scale_x"]), float(g["scale_y"])) == (m["scale"], m["scale_x"], m["scale_y"])


def _boxes(a):
    return np.stack([a["x"], a["y"], a["w"], a["h"]], 1)


def _check_layers(det, layers, feats, p):
    worst = 0.0
    for i, (L, f) in enumerate(zip(layers, feats)):
        got = det.feature_layer(i)
        assert got.shape == f.shape and f.size > 0
        ok, ratio = model.within(got, f, *model.cell_bounds(p, bool(L["approximated"])))
        worst = max(worst, ratio)
        assert ok, "layer %d (index %d, approximated %d): error %.3f of the bound" % (i, L["index"], L["approximated"], ratio)
    return worst


@pytest.mark.parametrize("approximate", [False, True], ids=["exact", "approximated"])
@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=IDS)
def test_feature_layers(oracle, capi, ctx, synth, ci, approximate):
    cfg = CONFIGS[ci]
    img = _image(synth, cfg)
    layers, feats, _ = _model_layers(oracle, synth, ci, approximate, "fixed" if approximate else None)
    if approximate:
        assert any(L["approximated"] for L in layers)
        _same_layers(layers, approx.plan(cfg["window_w"], cfg["window_h"], cfg["cell"], cfg["n"], 0, *cfg["size"], estimate=False))
    det = _detector(capi, ctx, cfg, 0.1, 1e30, approximate, FIXED_LAMBDAS if approximate else None)
    det.detect(img)
    _same_layers(det.layers(), layers)
    if approximate:
        assert np.array_equal(det.lambdas(), FIXED_LAMBDAS)
    worst = _check_layers(det, layers, feats, model.params(cfg["cell"]))
    print("largest error / bound over %d layers: %.3f (rtol %.2e)" % (len(layers), worst, model.rtol(cfg["cell"], cfg["cell"])))
    det.close()


@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=IDS)
def test_estimated_lambdas(oracle, capi, ctx, synth, ci):
    cfg = CONFIGS[ci]
    _, _, lam_model = _model_layers(oracle, synth, ci, True, None)
    det = _detector(capi, ctx, cfg, 0.1, 1e30, True)
    det.detect(_image(synth, cfg))
    lam = det.lambdas().copy()
    det.close()
    # a channel mean of non-negative cells errs by rtol relative (L*u*v*: by less), the ratio of two by 2 rtol, -log(ratio) / log(2) by 2 rtol / ln 2
    bound = 2 * model.rtol(cfg["cell"], cfg["cell"]) / np.log(2)
    err = float(np.abs(lam - lam_model).max())
    print("max |lambda - model| = %.3e (bound %.3e)" % (err, bound))
    assert lam.shape == (model.CHANNELS,) and np.all(np.isfinite(lam_model))
    assert err <= bound


@pytest.mark.parametrize("ci", range(len(CONFIGS)), ids=IDS)
def test_candidates_and_detections(oracle, capi, ctx, synth, ci):
    cfg = CONFIGS[ci]
    img = _image(synth, cfg)
    p = model.params(cfg["cell"])
    layers, feats, _ = _model_layers(oracle, synth, ci, True, "fixed")
    weights, bias, ws, hs, nms = _weights(cfg), 0.1, 0.8, 1.1, (0.4, 0)
    thr, scores, bounds = model.gap_threshold(layers, feats, weights, bias, p)
    sc, bx, where = approx.candidates(layers, scores, thr, cfg, ws, hs)
    bd = np.concatenate([b[s > np.float32(thr)] for s, b in zip(scores, bounds)])
    assert len(sc) >= 2 and {layers[i]["approximated"] for i in where.tolist()} == {0, 1}   # CONFIGS' seeds are chosen for this
    det = _detector(capi, ctx, cfg, bias, thr, True, FIXED_LAMBDAS, width_scale=ws, height_scale=hs, nms_overlap=nms[0], nms_type=nms[1])
    fin, cand = det.detect(img)
    assert len(cand) == len(sc)
    assert np.array_equal(_boxes(cand), bx)   # every candidate, in order
    err = np.abs(cand["score"].astype(np.float64) - sc.astype(np.float64))
    print("%d candidates, largest score error / bound: %.3f" % (len(sc), float((err / bd).max())))
    assert np.all(err <= bd)
    fs, fb = oracle.nms_iou(sc.astype(np.float32), bx, nms[0], nms[1])
    assert len(fin) == len(fs) > 0 and np.array_equal(_boxes(fin), fb)
    det.close()


def test_handle_behaviour(oracle, capi, ctx, synth):
    cfg = CONFIGS[0]
    img = _image(synth, cfg)
    p = model.params(cfg["cell"])
    layers, feats, _ = _model_layers(oracle, synth, 0, True, "fixed")
    thr, _, _ = model.gap_threshold(layers, feats, _weights(cfg), 0.1, p)
    det = _detector(capi, ctx, cfg, 0.1, thr, True, FIXED_LAMBDAS)
    fin1, cand1 = det.detect(img)
    last1 = det.feature_layer(len(layers) - 1)
    fin2, cand2 = det.detect(img)   # same size: buffers reused, same bytes
    assert len(cand1) > 0 and fin2.tobytes() == fin1.tobytes() and cand2.tobytes() == cand1.tobytes()
    assert det.feature_layer(len(layers) - 1).tobytes() == last1.tobytes()
    # another size: everything is rebuilt
    cfg_b = dict(cfg, size=(200, 150))
    img_b = _image(synth, cfg_b)
    det.detect(img_b)
    layers_b, feats_b, _ = model.feature_layers(oracle, img_b, cfg_b, p, True, FIXED_LAMBDAS)
    _same_layers(det.layers(), layers_b)
    _check_layers(det, layers_b, feats_b, p)
    # and back
    fin3, cand3 = det.detect(img)
    assert fin3.tobytes() == fin1.tobytes() and cand3.tobytes() == cand1.tobytes()
    # a frame that lives in HBM gives the same answer
    import torch
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    fin4, cand4 = det.detect_device(dev.data_ptr(), cfg["size"][0], cfg["size"][1], 3, candidates=True)
    assert fin4.tobytes() == fin1.tobytes() and cand4.tobytes() == cand1.tobytes()
    det.close()


def test_fhog_and_fpdw_handles_side_by_side(oracle, capi, ctx, synth):
    cfg = CONFIGS[0]
    img = _image(synth, cfg)
    layers, feats, _ = _model_layers(oracle, synth, 0, False, None)
    fpdw = _detector(capi, ctx, cfg, 0.1, 1e30, False)
    w_fhog = np.random.default_rng(5).normal(0, 0.05, (cfg["window_h"], cfg["window_w"], 31)).astype(np.float32)
    fhog = capi.Aggregated(ctx, w_fhog, 0.1, 1e30, cell_size=cfg["cell"], octave_layers=cfg["n"])
    want_fhog = None
    for _ in range(2):
        fhog.detect(img)
        f0 = fhog.feature_layer(0)
        assert f0.shape[2] == 31
        want_fhog = f0 if want_fhog is None else want_fhog
        assert f0.tobytes() == want_fhog.tobytes()
        fpdw.detect(img)
        with pytest.raises(capi.FdError):
            fhog.feature_layer(0)   # its feature layers were overwritten by the other handle's detect
        _check_layers(fpdw, layers, feats, model.params(cfg["cell"]))
    fhog.detect(img)
    with pytest.raises(capi.FdError):
        fpdw.feature_layer(0)
    fhog.close()
    fpdw.close()


def test_errors(oracle, capi, ctx, synth):
    cfg = CONFIGS[0]
    img = _image(synth, cfg)
    det = _detector(capi, ctx, cfg, 0.1, 0.0, False)
    for bad in (oracle.bgr2gray(img), np.zeros((240, 320, 4), np.uint8)):
        with pytest.raises(capi.FdError) as e:
            det.detect(bad)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "the gradient image type must be CV_8UC3" in str(e.value)
    det.detect(img)   # the handle stays usable
    det.close()
    with pytest.raises(capi.FdError) as e:
        _detector(capi, ctx, cfg, 0.1, 0.0, True, np.zeros(31))
    assert e.value.code == capi.FD_ERR_RUNTIME and "the number of lambdas does not match the number of channels" in str(e.value)
    with pytest.raises(ValueError):
        _detector(capi, ctx, cfg, 0.1, 0.0, False, FIXED_LAMBDAS)
    with pytest.raises(capi.FdError) as e:
        _detector(capi, ctx, cfg, 0.1, 0.0, False, normalization_radius=-1)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError) as e:   # one cell with this normaliser does not fit a workgroup's tile
        _detector(capi, ctx, cfg, 0.1, 0.0, False, normalization_radius=200)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    # a layer below the aggregation filter's limits: with a window of one cell the smallest layer of a 75 x 70 image is 7 x 7
    # pixels, and the 8-tap filter of cell size 4 asks for 8 columns (no normaliser, so that this filter is the one that objects)
    tiny = capi.Aggregated(ctx, np.zeros((1, 1, 10), np.float32), 0.0, 0.0, cell_size=4, octave_layers=2, features="fpdw", normalization_radius=0)
    with pytest.raises(capi.FdError) as e:
        tiny.detect(synth.make_frame(75, 70, seed=3))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    assert "TriangularConvolutionFilter: image must have at least 8 columns, but had only 7" in str(e.value)
    tiny.detect(synth.make_frame(120, 100, seed=3))   # smallest layer 8 x 7: within the limits
    tiny.close()
    small = synth.make_frame(17, 21, seed=3)   # one layer only: the score pyramid of an exact handle needs two
    det = _detector(capi, ctx, cfg, 0.1, 0.0, False)
    with pytest.raises(capi.FdError) as e:
        det.detect(small)
    assert e.value.code == capi.FD_ERR_RUNTIME and "at least two pyramid layers" in str(e.value)
    det.close()
