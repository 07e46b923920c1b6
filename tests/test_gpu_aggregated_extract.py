"""AggregatedFeaturesExtractor::update / extract(Rect) on the device (fd_aggregated_update, fd_aggregated_extract and its kernel
k_agg_gather, fd_aggregated_set_svm) against tests/detector_training_model.py on the handle's own feature layers: a 160 x 120
image, an FHOG handle (cell 8, window 4 x 4, two layers per octave) and an approximated FPDW handle (window 3 x 5)."""
import numpy as np
import pytest

import detector_training_model as T

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, CELL = 160, 120, 8
SENTINEL = np.float32(-12345.5)
HANDLES = {
    "fhog": dict(window_w=4, window_h=4, n=2, d=31, kw=dict()),
    "fpdw-approx": dict(window_w=3, window_h=5, n=3, d=10, kw=dict(approximate=True, features="fpdw")),
}


def _weights(cfg, seed=5):
    return np.random.default_rng(seed).normal(0, 0.05, (cfg["window_h"], cfg["window_w"], cfg["d"])).astype(np.float32)


def _handle(capi, ctx, cfg, weights=None, bias=0.1, thr=1e30):
    return capi.Aggregated(ctx, _weights(cfg) if weights is None else weights, bias, thr, cell_size=CELL, octave_layers=cfg["n"], **cfg["kw"])


@pytest.fixture(scope="module")
def image(synth):
    return synth.make_frame(WIDTH, HEIGHT, seed=77)


def _box_at(cfg, L, cell_x, cell_y):
    """a box of the layer's window size whose centre lies in the middle of cell (cell_x, cell_y) of layer L"""
    sx, sy = float(L["scale_x"]), float(L["scale_y"])
    w, h = T.cround(cfg["window_w"] * CELL / sx), T.cround(cfg["window_h"] * CELL / sy)
    cx, cy = (cell_x + 0.5) * CELL / sx, (cell_y + 0.5) * CELL / sy
    return (int(round(cx - 0.5 * w)), int(round(cy - 0.5 * h)), w, h)


def _boxes(cfg, layers):
    """every branch of extract: per layer the first and the last window position and the four windows that leave it by one
    cell; widths whose layer lies below and above the pyramid; a width of 0; duplicates"""
    ww, wh = cfg["window_w"], cfg["window_h"]
    boxes = []
    for L in layers:
        cols, rows = int(L["cols"]), int(L["rows"])
        if cols < ww or rows < wh:
            continue
        cx0, cy0, cx1, cy1 = ww // 2, wh // 2, cols - ww + ww // 2, rows - wh + wh // 2
        boxes += [_box_at(cfg, L, cx0, cy0), _box_at(cfg, L, cx1, cy1), _box_at(cfg, L, cx0, cy1), _box_at(cfg, L, cx1, cy0)]
        boxes += [_box_at(cfg, L, cx0 - 1, cy0), _box_at(cfg, L, cx1 + 1, cy0), _box_at(cfg, L, cx0, cy0 - 1), _box_at(cfg, L, cx0, cy1 + 1)]
    boxes += [(40, 30, ww * CELL // 4, wh * CELL // 4), (0, 0, 8 * WIDTH, 8 * HEIGHT), (10, 10, 0, 10)]
    boxes += [(16, 8, ww * CELL, wh * CELL), (16, 8, ww * CELL, wh * CELL), boxes[0], boxes[4]]
    return boxes


def _check(det, cfg, boxes):
    layers = det.layers()
    feats = [det.feature_layer(i) for i in range(len(layers))]
    d = cfg["window_w"] * cfg["window_h"] * cfg["d"]
    out = np.full((len(boxes), d), SENTINEL, np.float32)
    got, bounds, valid = det.extract(boxes, out=out)
    assert got is out
    geo = dict(window_w=cfg["window_w"], window_h=cfg["window_h"], cell=CELL, octave_layers=cfg["n"])
    n_valid = 0
    for k, box in enumerate(boxes):
        want = T.extract(box, layers, feats, **geo)
        assert bool(valid[k]) == (want is not None), (k, box)
        if want is None:
            assert (got[k] == SENTINEL).all(), (k, box)   # untouched
            continue
        n_valid += 1
        assert got[k].tobytes() == np.ascontiguousarray(want[0]).tobytes(), (k, box)
        assert (int(bounds[k]["x"]), int(bounds[k]["y"]), int(bounds[k]["w"]), int(bounds[k]["h"])) == want[1], (k, box)
        assert bounds[k]["score"] == 0
    return n_valid, layers


@pytest.mark.parametrize("name", list(HANDLES))
def test_extract_equals_slicing_the_feature_layers(capi, ctx, image, name):
    cfg = HANDLES[name]
    det = _handle(capi, ctx, cfg)
    det.update(image)
    layers = det.layers()
    assert len(layers) >= 3 and (name == "fhog" or any(int(L["approximated"]) for L in layers))
    boxes = _boxes(cfg, layers)
    n_valid, _ = _check(det, cfg, boxes)
    # what the list is for: per usable layer four inside and four outside, the model and the construction agree on which
    geo = dict(window_w=cfg["window_w"], window_h=cfg["window_h"], cell=CELL, octave_layers=cfg["n"])
    usable = [i for i, L in enumerate(layers) if int(L["cols"]) >= cfg["window_w"] and int(L["rows"]) >= cfg["window_h"]]
    assert len(usable) >= 3
    for u, i in enumerate(usable):
        res = [T.resolve(b, layers, **geo) for b in boxes[8 * u:8 * u + 8]]
        L = layers[i]
        assert res[0] == (i, 0, 0) and res[1] == (i, int(L["cols"]) - cfg["window_w"], int(L["rows"]) - cfg["window_h"]), (i, res)
        assert res[2] is not None and res[3] is not None and res[4:] == [None] * 4, (i, res)
    tail = [T.resolve(b, layers, **geo) for b in boxes[8 * len(usable):]]
    assert tail[:3] == [None] * 3 and tail[3] is not None and tail[3] == tail[4] and tail[5] == (usable[0], 0, 0) and tail[6] is None
    assert n_valid == 4 * len(usable) + 3
    # n = 1, and n = 257: more than one block of the gather kernel, every row a different one of the list
    assert _check(det, cfg, [boxes[1]])[0] == 1
    assert _check(det, cfg, [boxes[4]])[0] == 0
    many = [boxes[k % len(boxes)] for k in range(257)]
    assert _check(det, cfg, many)[0] > 100
    assert det.extract(np.zeros((0, 4), np.int32))[0].shape == (0, cfg["window_w"] * cfg["window_h"] * cfg["d"])
    det.close()


def test_features_in_device_memory(capi, ctx, image):
    """features_on_device: the rows land in the caller's device matrix at their index, invalid rows untouched"""
    import ctypes as C
    import torch
    cfg = HANDLES["fhog"]
    det = _handle(capi, ctx, cfg)
    det.update(image)
    boxes = _boxes(cfg, det.layers())
    want, _, want_valid = det.extract(boxes, out=np.full((len(boxes), 4 * 4 * 31), SENTINEL, np.float32))
    dev = torch.full((len(boxes), 4 * 4 * 31), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b = np.ascontiguousarray(boxes, np.int32)
    valid, bounds = np.zeros(len(boxes), np.uint8), np.zeros(len(boxes), capi.BOX_DTYPE)
    ctx.check(capi.lib().fd_aggregated_extract(ctx.h, det.h, len(boxes), capi._ptr(b), C.c_void_p(dev.data_ptr()), 1, capi._ptr(bounds), capi._ptr(valid)))
    assert np.array_equal(valid.astype(bool), want_valid) and 0 < want_valid.sum() < len(boxes)
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    det.close()


def test_update_gives_the_layers_of_detect(capi, ctx, image):
    """detect = update + scores: the same candidates and detections with and without an update in between, and the same
    feature layers"""
    cfg = HANDLES["fhog"]
    w = _weights(cfg)
    a, b = _handle(capi, ctx, cfg, w, 0.0, 0.0), _handle(capi, ctx, cfg, w, 0.0, 0.0)
    a.update(image)
    fa = [a.feature_layer(i) for i in range(len(a.layers()))]
    da, ca = a.detect(image)
    db, cb = b.detect(image)
    assert len(ca) > 0 and ca.tobytes() == cb.tobytes() and da.tobytes() == db.tobytes()
    assert a.layers().tobytes() == b.layers().tobytes()
    for i, f in enumerate(fa):
        assert f.tobytes() == b.feature_layer(i).tobytes()
    a.close()
    b.close()


def test_extract_needs_the_contexts_current_features(capi, ctx, image):
    cfg = HANDLES["fhog"]
    a, b = _handle(capi, ctx, cfg), _handle(capi, ctx, cfg)
    with pytest.raises(capi.FdError) as e:
        a.extract([(16, 8, 32, 32)])   # before any update
    assert e.value.code == capi.FD_ERR_RUNTIME
    a.update(image)
    assert a.extract([(16, 8, 32, 32)])[2].all()
    b.detect(image)
    with pytest.raises(capi.FdError) as e:
        a.extract([(16, 8, 32, 32)])
    assert e.value.code == capi.FD_ERR_RUNTIME and "gone" in str(e.value)
    assert b.extract([(16, 8, 32, 32)])[2].all()   # detect leaves its handle's layers current
    a.update(image)
    assert a.extract([(16, 8, 32, 32)])[2].all()
    a.close()
    b.close()


def test_null_pointers(capi, ctx, image):
    import ctypes as C
    lib = capi.lib()
    cfg = HANDLES["fhog"]
    a = _handle(capi, ctx, cfg)
    a.update(image)
    boxes = np.array([[16, 8, 32, 32]], np.int32)
    feats, valid = np.zeros((1, 4 * 4 * 31), np.float32), np.zeros(1, np.uint8)
    P = capi._ptr
    calls = [lambda: lib.fd_aggregated_extract(ctx.h, None, 1, P(boxes), P(feats), 0, None, P(valid)),
             lambda: lib.fd_aggregated_extract(ctx.h, a.h, 1, None, P(feats), 0, None, P(valid)),
             lambda: lib.fd_aggregated_extract(ctx.h, a.h, 1, P(boxes), None, 0, None, P(valid)),
             lambda: lib.fd_aggregated_extract(ctx.h, a.h, 1, P(boxes), P(feats), 0, None, None),
             lambda: lib.fd_aggregated_extract(ctx.h, a.h, -1, P(boxes), P(feats), 0, None, P(valid)),
             lambda: lib.fd_aggregated_update(ctx.h, a.h, None, WIDTH, HEIGHT, 3, 0),
             lambda: lib.fd_aggregated_update(ctx.h, None, P(image), WIDTH, HEIGHT, 3, 0),
             lambda: lib.fd_aggregated_set_svm(ctx.h, a.h, None, 0.0, 0.0),
             lambda: lib.fd_aggregated_set_svm(ctx.h, None, P(feats), 0.0, 0.0)]
    for i, call in enumerate(calls):
        assert call() == capi.FD_ERR_INVALID_ARGUMENT, i
    assert lib.fd_aggregated_extract(ctx.h, a.h, 1, P(boxes), P(feats), 0, None, P(valid)) == capi.FD_OK and valid[0] == 1   # bounds are optional
    a.close()


@pytest.mark.parametrize("name", list(HANDLES))
def test_set_svm_equals_a_fresh_handle(capi, ctx, image, name):
    cfg = HANDLES[name]
    w1, w2 = _weights(cfg, 5), _weights(cfg, 6)
    a = _handle(capi, ctx, cfg, w1, 0.1, 0.0)
    d1, c1 = a.detect(image)
    a.set_svm(w2, -0.05, 0.02)
    d2, c2 = a.detect(image)
    b = _handle(capi, ctx, cfg, w2, -0.05, 0.02)
    db, cb = b.detect(image)
    assert len(cb) > 0 and c2.tobytes() == cb.tobytes() and d2.tobytes() == db.tobytes() and c2.tobytes() != c1.tobytes()
    with pytest.raises(ValueError):
        a.set_svm(w2[:-1], 0.0, 0.0)
    a.close()
    b.close()
