"""CPU model of the aggregated-features detector on an approximated feature pyramid (createApproximateDetector with
GrayscaleFilter + FhogFilter; ImagePyramid::createApproximated), shared by the test_*aggregated_approx* files.

Built only from the frozen oracle's pieces -- Pyramid(octave_layers=1), fhog, orc_resize_linear_f32 per channel, nms_iou -- plus
numpy float32 for the factor multiply and the score accumulation in k_fhog_score's documented order.  Every scale is evaluated
with math.pow / repeated *= 0.5 in the reference's expression order: whether the smallest layer exists depends on the double
rounding of exactly these expressions."""
import ctypes as C
import math

import numpy as np


def limits(window_w, window_h, cell, n, min_window_width, width, height):
    """(minScale, maxScale) of AggregatedFeaturesExtractor (AggregatedFeaturesExtractor.cpp:30-31,47-77)"""
    patch_w, patch_h = window_w * cell, window_h * cell
    inc = math.pow(0.5, 1.0 / n)
    max_scale = 1.0
    if min_window_width > patch_w:
        m = patch_w / min_window_width
        max_scale = math.pow(inc, math.ceil(math.log(m) / math.log(inc)))
    aspect, image_aspect = patch_h / patch_w, height / width
    max_width = int(height / aspect) if aspect > image_aspect else width
    m = patch_w / max_width
    min_scale = math.pow(inc, int(math.log(m) / math.log(inc)))
    return min_scale, max_scale


def source_layers(min_scale, max_scale, width, height):
    """kept layers (index, scale, w, h) of ImagePyramid(1, min, max) (ImagePyramid.cpp:170-198)"""
    out = []
    scale = 1.0
    w, h = width, height
    if min_scale <= scale <= max_scale:
        out.append((0, scale, w, h))
    scale *= 0.5
    j = 1
    while scale >= min_scale and w > 1:
        w, h = (w + 1) // 2, (h + 1) // 2
        if scale <= max_scale:
            out.append((j, scale, w, h))
        j += 1
        scale *= 0.5
    return out


def plan(window_w, window_h, cell, n, min_window_width, width, height, estimate=True):
    """layer list of createLayers(const ImagePyramid&) (ImagePyramid.cpp:200-235); None when the lambdas are to be estimated and fewer
    than two exact layers remain"""
    min_scale, max_scale = limits(window_w, window_h, cell, n, min_window_width, width, height)
    src = source_layers(min_scale, max_scale, width, height)
    if estimate and len(src) < 2:
        return None
    inc = math.pow(0.5, 1.0 / n)
    layers = []
    for j, scale, w, h in src:
        exact = dict(index=j * n, approximated=0, parent=-1, rows=h // cell, cols=w // cell, scale=scale, scale_x=w / width,
                     scale_y=h / height, s=1.0)
        parent = len(layers)
        layers.append(exact)
        for i in range(1, n):
            s = math.pow(inc, i)
            overall = exact["scale"] * s
            if min_scale <= overall <= max_scale:
                layers.append(dict(index=exact["index"] + i, approximated=1, parent=parent, rows=round(exact["rows"] * s),
                                   cols=round(exact["cols"] * s), scale=overall, scale_x=exact["scale_x"] * s,
                                   scale_y=exact["scale_y"] * s, s=s))   # round(): half to even, like cvRound
    return layers


def resize_channels(oracle, feat, rows, cols):
    """cv::resize(INTER_LINEAR) of every channel of a (R, C, D) float32 map on its own"""
    f = oracle.lib().orc_resize_linear_f32
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    f.restype = None
    R, Cc, D = feat.shape
    out = np.empty((rows, cols, D), np.float32)
    for c in range(D):
        src = np.ascontiguousarray(feat[:, :, c])
        dst = np.empty((rows, cols), np.float32)
        f(src.ctypes.data_as(C.c_void_p), Cc, R, dst.ctypes.data_as(C.c_void_p), cols, rows)
        out[:, :, c] = dst
    return out


def estimate_lambdas(exact_feats, exact_scales):
    """ImagePyramid::estimateLambdas (ImagePyramid.cpp:237-275): layers [1], [2] of more than two, else [0], [1]"""
    a = 1 if len(exact_feats) > 2 else 0
    means = [f.astype(np.float64).sum(axis=(0, 1)) / (f.shape[0] * f.shape[1]) for f in exact_feats[a:a + 2]]
    ratio = exact_scales[a] / exact_scales[a + 1]
    return np.array([-math.log(m1 / m2) / math.log(ratio) for m1, m2 in zip(means[0], means[1])], np.float64)


def feature_layers(oracle, image, layers, cfg, lambdas=None):
    """(feature maps in layer order, lambdas used); cfg: window_w, window_h, cell, n, min_window_width, unsigned_bins"""
    h, w = image.shape[:2]
    min_scale, max_scale = limits(cfg["window_w"], cfg["window_h"], cfg["cell"], cfg["n"], cfg["min_window_width"], w, h)
    pyr = oracle.Pyramid(octave_layers=1, min_scale=min_scale, max_scale=max_scale)
    pyr.update(image)
    exact_pos = [i for i, L in enumerate(layers) if not L["approximated"]]
    assert len(pyr.layers()) == len(exact_pos)
    feats = [None] * len(layers)
    for k, i in enumerate(exact_pos):
        assert pyr.layers()[k]["scale"] == layers[i]["scale"]
        feats[i] = oracle.fhog(pyr.layer(k), cell_size=cfg["cell"], unsigned_bins=cfg["unsigned_bins"])
        assert feats[i].shape[:2] == (layers[i]["rows"], layers[i]["cols"])
    pyr.close()
    if lambdas is None:
        lambdas = estimate_lambdas([feats[i] for i in exact_pos], [layers[i]["scale"] for i in exact_pos])
    lambdas = np.asarray(lambdas, np.float64)
    for i, L in enumerate(layers):
        if L["approximated"]:
            factor = np.array([np.float32(math.pow(L["s"], -lam)) for lam in lambdas], np.float32)
            feats[i] = resize_channels(oracle, feats[L["parent"]], L["rows"], L["cols"]) * factor[None, None, :]
    return feats, lambdas


def score_map(feat, weights, bias):
    """k_fhog_score's order: per channel the kernel window row-major in float32, then the channels in order onto -bias"""
    wh, ww, D = weights.shape
    vh, vw = feat.shape[0] - wh + 1, feat.shape[1] - ww + 1
    if vh <= 0 or vw <= 0:
        return np.empty((0, 0), np.float32)
    acc = np.zeros((vh, vw, D), np.float32)
    for ky in range(wh):
        for kx in range(ww):
            acc = acc + weights[ky, kx][None, None, :] * feat[ky:ky + vh, kx:kx + vw, :]
    score = np.full((vh, vw), -np.float32(bias), np.float32)
    for c in range(D):
        score = score + acc[:, :, c]
    return score


def _cround(v):   # std::round on non-negative values
    return int(math.floor(v + 0.5))


def candidates(layers, scores, threshold, cfg, width_scale=1.0, height_scale=1.0):
    """getPositiveWindows (AggregatedFeaturesDetector.cpp:87-112): (score[n], xywh[n, 4], layer position[n])"""
    cs = cfg["cell"]
    sc, boxes, where = [], [], []
    for i, (L, S) in enumerate(zip(layers, scores)):
        ys, xs = np.nonzero(S > np.float32(threshold))
        for y, x in zip(ys.tolist(), xs.tolist()):
            bx, by = _cround((x * cs) / L["scale_x"]), _cround((y * cs) / L["scale_y"])
            bw, bh = _cround((cfg["window_w"] * cs) / L["scale_x"]), _cround((cfg["window_h"] * cs) / L["scale_y"])
            cx, cy = bx + bw // 2, by + bh // 2
            rw, rh = int(np.float32(width_scale) * np.float32(bw)), int(np.float32(height_scale) * np.float32(bh))
            sc.append(S[y, x])
            boxes.append((cx - rw // 2, cy - rh // 2, rw, rh))
            where.append(i)
    return np.array(sc, np.float32), np.array(boxes, np.int32).reshape(-1, 4), np.array(where, np.int32)


def all_scores(layers, feats, weights, bias):
    return [score_map(f, weights, bias) for f in feats]
