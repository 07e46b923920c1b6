"""AggregatedFeaturesDetector on an approximated feature pyramid (capi.Aggregated(approximate=True)) against the CPU model of
tests/aggregated_approx_model.py: feature layers bit-identical with explicit lambdas, estimated lambdas within 1e-9 (a double sum
of <= 4e4 non-negative floats errs by < 5e-12 relative, < 2e-11 through log(ratio) / log(2)), and with the returned lambdas fed
into the model feature layers, candidates and final detections bit-identical."""
import numpy as np
import pytest

import aggregated_approx_model as model

pytestmark = pytest.mark.gpu

CONFIGS = [
    dict(n=8, size=(640, 480), window_w=8, window_h=8, cell=8, min_window_width=0, ch=3),
    dict(n=2, size=(640, 480), window_w=10, window_h=12, cell=4, min_window_width=0, ch=1),      # smallest layer dropped
    dict(n=3, size=(333, 517), window_w=8, window_h=8, cell=4, min_window_width=0, ch=3),
    dict(n=4, size=(1280, 720), window_w=10, window_h=12, cell=8, min_window_width=120, ch=1),   # maxScale < 1
    dict(n=8, size=(1920, 1080), window_w=8, window_h=8, cell=8, min_window_width=0, ch=3),
    dict(n=3, size=(1280, 720), window_w=8, window_h=8, cell=8, min_window_width=96, ch=1),      # maxScale < 1, layer dropped
    dict(n=4, size=(640, 480), window_w=8, window_h=8, cell=8, min_window_width=0, ch=3, bins=12),   # 40 channels: k_fhog_score_wide
]
IDS = ["n%d-%dx%d-c%d-%s%s" % (c["n"], c["size"][0], c["size"][1], c["cell"], "bgr" if c["ch"] == 3 else "gray",
                              "-b%d" % c["bins"] if "bins" in c else "") for c in CONFIGS]
D = 31


def _channels(cfg):
    return 3 * cfg.get("bins", 9) + 4


def _fixed_lambdas(cfg):
    B = cfg.get("bins", 9)
    return np.concatenate([np.linspace(0.05, 0.35, 2 * B), np.linspace(-0.1, 0.2, B), [0.11, 0.13, 0.17, 0.19]])


FIXED_LAMBDAS = _fixed_lambdas({})


def _image(synth, oracle, cfg, seed=77):
    frame = synth.make_frame(cfg["size"][0], cfg["size"][1], seed=seed)
    return frame if cfg["ch"] == 3 else oracle.bgr2gray(frame)


def _cfg(cfg):
    return dict(cfg, unsigned_bins=cfg.get("bins", 9))


def _weights(cfg, seed=5):
    return np.random.default_rng(seed).normal(0, 0.05, (cfg["window_h"], cfg["window_w"], _channels(cfg))).astype(np.float32)


def _detector(capi, ctx, cfg, weights, bias, thr, lambdas=None, approximate=True, **kw):
    return capi.Aggregated(ctx, weights, bias, thr, cell_size=cfg["cell"], unsigned_bins=cfg.get("bins", 9), octave_layers=cfg["n"],
                           min_window_width=cfg["min_window_width"], approximate=approximate, lambdas=lambdas, **kw)


def _plan(cfg):
    return model.plan(cfg["window_w"], cfg["window_h"], cfg["cell"], cfg["n"], cfg["min_window_width"], *cfg["size"])


def _same_layers(got, want):
    assert len(got) == len(want)
    for g, m in zip(got, want):
        assert (int(g["index"]), int(g["approximated"]), int(g["parent"]), int(g["rows"]), int(g["cols"])) == \
               (m["index"], m["approximated"], m["parent"], m["rows"], m["cols"])
        assert (float(g["scale"]), float(g["scale_x"]), float(g["scale_y"])) == (m["scale"], m["scale_x"], m["scale_y"])


def _boxes(a):
    return np.stack([a["x"], a["y"], a["w"], a["h"]], 1)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_feature_layers_with_explicit_lambdas(oracle, capi, ctx, synth, cfg):
    img = _image(synth, oracle, cfg)
    layers = _plan(cfg)
    assert any(L["approximated"] for L in layers)
    for lambdas in (np.zeros(_channels(cfg)), _fixed_lambdas(cfg)):
        det = _detector(capi, ctx, cfg, _weights(cfg), 0.1, 1e30, lambdas=lambdas)
        det.detect(img)
        _same_layers(det.layers(), layers)
        assert np.array_equal(det.lambdas(), lambdas)
        feats, _ = model.feature_layers(oracle, img, layers, _cfg(cfg), lambdas)
        for i, f in enumerate(feats):
            got = det.feature_layer(i)
            assert got.shape == f.shape and f.size > 0
            assert got.tobytes() == f.tobytes(), "layer %d (index %d, approximated %d)" % (i, layers[i]["index"], layers[i]["approximated"])
        det.close()


def _threshold(layers, scores):
    """a quantile of the model's scores that leaves > 5 candidates, at least one on an exact and one on an approximated layer"""
    flat = np.concatenate([s.ravel() for s in scores])
    best = {0: -np.inf, 1: -np.inf}
    for L, s in zip(layers, scores):
        if s.size:
            best[L["approximated"]] = max(best[L["approximated"]], float(s.max()))
    for q in (0.999, 0.995, 0.99, 0.95, 0.9, 0.5):
        thr = float(np.float32(np.quantile(flat, q)))
        if thr < min(best.values()) and int((flat > np.float32(thr)).sum()) > 5:
            return thr
    raise AssertionError("no quantile leaves candidates on both kinds of layers")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_estimated_lambdas_candidates_and_detections(oracle, capi, ctx, synth, cfg):
    img = _image(synth, oracle, cfg)
    layers = _plan(cfg)
    weights = _weights(cfg)
    bias, ws, hs, nms = 0.1, 0.8, 1.1, (0.4, 2)
    # pass 1: lambdas only
    det = _detector(capi, ctx, cfg, weights, bias, 1e30)
    fin, cand = det.detect(img)
    assert len(fin) == 0 and len(cand) == 0
    lam = det.lambdas().copy()
    _, lam_model = model.feature_layers(oracle, img, layers, _cfg(cfg))
    print("max |lambda - model| = %.3e" % float(np.abs(lam - lam_model).max()))
    assert lam.shape == (_channels(cfg),) and np.all(np.isfinite(lam_model))
    assert float(np.abs(lam - lam_model).max()) <= 1e-9
    det.close()
    # pass 2: the returned lambdas into the model; everything downstream bit-identical
    feats, _ = model.feature_layers(oracle, img, layers, _cfg(cfg), lam)
    scores = model.all_scores(layers, feats, weights, bias)
    thr = _threshold(layers, scores)
    sc, bx, where = model.candidates(layers, scores, thr, _cfg(cfg), ws, hs)
    kinds = {layers[i]["approximated"] for i in where.tolist()}
    assert len(sc) > 5 and kinds == {0, 1}
    det = _detector(capi, ctx, cfg, weights, bias, thr, width_scale=ws, height_scale=hs, nms_overlap=nms[0], nms_type=nms[1])
    fin, cand = det.detect(img)
    assert np.array_equal(det.lambdas(), lam)   # same image, same sums
    for i, f in enumerate(feats):
        assert det.feature_layer(i).tobytes() == f.tobytes(), "layer %d" % i
    assert len(cand) == len(sc)
    assert np.array_equal(cand["score"], sc)
    assert np.array_equal(_boxes(cand), bx)
    fs, fb = oracle.nms_iou(sc, bx, nms[0], nms[1])
    assert len(fin) == len(fs) > 0
    assert np.array_equal(fin["score"], fs) and np.array_equal(_boxes(fin), fb)
    det.close()


@pytest.mark.parametrize("ch", [1, 3])
def test_one_layer_per_octave_equals_the_oracle_detector(oracle, capi, ctx, synth, ch):
    """n = 1: no approximated layers, so the frozen oracle's exact detector is an independent reference"""
    cfg = dict(n=1, size=(640, 480), window_w=8, window_h=8, cell=8, min_window_width=0, ch=ch)
    img = _image(synth, oracle, cfg)
    weights = _weights(cfg)
    sc0, _ = oracle.aggregated_candidates(img, weights, 0.1, -1e30, cell_size=8, octave_layers=1)
    thr = float(np.float32(np.quantile(sc0, 0.98)))
    so, bo = oracle.aggregated_candidates(img, weights, 0.1, thr, cell_size=8, octave_layers=1)
    det = _detector(capi, ctx, cfg, weights, 0.1, thr)
    fin, cand = det.detect(img)
    assert not det.layers()["approximated"].any()
    assert len(cand) == len(so) > 5
    assert np.array_equal(cand["score"], so) and np.array_equal(_boxes(cand), bo)
    fs, fb = oracle.nms_iou(so, bo, 0.3, 0)
    assert np.array_equal(fin["score"], fs) and np.array_equal(_boxes(fin), fb)
    det.close()


def test_handle_and_buffer_reuse(oracle, capi, ctx, synth):
    cfg = CONFIGS[0]
    weights = _weights(cfg)
    img = _image(synth, oracle, cfg)
    layers = _plan(cfg)
    feats, lam_model = model.feature_layers(oracle, img, layers, _cfg(cfg))
    scores = model.all_scores(layers, feats, weights, 0.1)
    thr = _threshold(layers, scores)
    det = _detector(capi, ctx, cfg, weights, 0.1, thr)
    fin1, cand1 = det.detect(img)
    lam1 = det.lambdas().copy()
    last1 = det.feature_layer(len(layers) - 1)
    fin2, cand2 = det.detect(img)   # same size: buffers reused, same bytes
    assert fin2.tobytes() == fin1.tobytes() and cand2.tobytes() == cand1.tobytes() and len(cand1) > 5
    assert np.array_equal(det.lambdas(), lam1) and det.feature_layer(len(layers) - 1).tobytes() == last1.tobytes()
    # another image of the same size: lambdas are estimated again
    img_b = _image(synth, oracle, cfg, seed=78)
    det.detect(img_b)
    lam_b = det.lambdas().copy()
    _, lam_b_model = model.feature_layers(oracle, img_b, layers, _cfg(cfg))
    assert not np.array_equal(lam_b, lam1) and float(np.abs(lam_b - lam_b_model).max()) <= 1e-9
    # another size: everything is rebuilt
    cfg_c = dict(cfg, size=(400, 300))
    img_c = _image(synth, oracle, cfg_c)
    det.detect(img_c)
    layers_c = _plan(cfg_c)
    _same_layers(det.layers(), layers_c)
    feats_c, _ = model.feature_layers(oracle, img_c, layers_c, _cfg(cfg_c), det.lambdas())
    for i, f in enumerate(feats_c):
        assert det.feature_layer(i).tobytes() == f.tobytes()
    # and back
    fin3, cand3 = det.detect(img)
    assert fin3.tobytes() == fin1.tobytes() and cand3.tobytes() == cand1.tobytes()
    det.close()


def test_exact_and_approximated_handles_side_by_side(oracle, capi, ctx, synth):
    cfg = dict(n=4, size=(640, 480), window_w=8, window_h=8, cell=8, min_window_width=0, ch=3)
    img = _image(synth, oracle, cfg)
    weights = _weights(cfg)
    sc0, _ = oracle.aggregated_candidates(img, weights, 0.1, -1e30, cell_size=8, octave_layers=4)
    thr = float(np.float32(np.quantile(sc0, 0.99)))
    so, bo = oracle.aggregated_candidates(img, weights, 0.1, thr, cell_size=8, octave_layers=4)
    exact = _detector(capi, ctx, cfg, weights, 0.1, thr, approximate=False)
    approx = _detector(capi, ctx, cfg, weights, 0.1, thr, lambdas=FIXED_LAMBDAS)
    layers = _plan(cfg)
    feats, _ = model.feature_layers(oracle, img, layers, _cfg(cfg), FIXED_LAMBDAS)
    sa, ba, _ = model.candidates(layers, model.all_scores(layers, feats, weights, 0.1), thr, _cfg(cfg))
    assert len(so) > 5 and len(sa) > 5 and not (len(sa) == len(so) and np.array_equal(sa, so))
    for _ in range(3):
        _, ce = exact.detect(img)
        assert np.array_equal(ce["score"], so) and np.array_equal(_boxes(ce), bo)
        assert not exact.layers()["approximated"].any()
        _, ca = approx.detect(img)
        assert np.array_equal(ca["score"], sa) and np.array_equal(_boxes(ca), ba)
        with pytest.raises(capi.FdError):
            exact.feature_layer(0)   # its feature layers were overwritten by the other handle's detect
        assert approx.feature_layer(1).tobytes() == feats[1].tobytes()
    exact.close()
    approx.close()


def test_errors(oracle, capi, ctx, synth):
    cfg = CONFIGS[0]
    with pytest.raises(capi.FdError) as e:
        _detector(capi, ctx, cfg, _weights(cfg), 0.1, 0.0, lambdas=np.zeros(30))
    assert e.value.code == capi.FD_ERR_RUNTIME and "the number of lambdas does not match the number of channels" in str(e.value)
    small = synth.make_frame(100, 100, seed=3)   # one octave only
    det = _detector(capi, ctx, cfg, _weights(cfg), 0.1, 0.0)
    with pytest.raises(capi.FdError) as e:
        det.detect(small)
    assert e.value.code == capi.FD_ERR_RUNTIME and "at least two pyramid layers are needed to estimate the lambdas" in str(e.value)
    det.detect(_image(synth, oracle, cfg))   # the handle stays usable
    det.close()
    # given lambdas need no second octave (ImagePyramid.cpp:209-213): the single exact layer and its approximations
    det = _detector(capi, ctx, cfg, _weights(cfg), 0.1, 1e30, lambdas=FIXED_LAMBDAS)
    det.detect(small)
    layers = model.plan(cfg["window_w"], cfg["window_h"], cfg["cell"], cfg["n"], 0, 100, 100, estimate=False)
    assert sum(1 for L in layers if not L["approximated"]) == 1 and len(layers) > 1
    _same_layers(det.layers(), layers)
    feats, _ = model.feature_layers(oracle, small, layers, _cfg(cfg), FIXED_LAMBDAS)
    for i, f in enumerate(feats):
        assert det.feature_layer(i).tobytes() == f.tobytes()
    det.close()
    with pytest.raises(ValueError):
        _detector(capi, ctx, cfg, _weights(cfg), 0.1, 0.0, lambdas=np.zeros(D), approximate=False)
