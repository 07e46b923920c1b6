"""CPU model of the FPDW channel features (ChainedFilter(FpdwFeaturesFilter, AggregationFilter(cell, true, false))) and of the
aggregated-features detector built on them, shared by the test_*fpdw* files.

The BGR pyramid is the frozen oracle's Pyramid run on each colour plane (cv::resize and cv::pyrDown treat the channels of a
CV_8UC3 image independently), bgr2gray is the oracle's.  The gradient codes are integers and the look-up table is float32
arithmetic restated operation by operation (its orientation is (float)atan2((double)gY, (double)gX)), so codes,
bins, weights and magnitudes are exact.  Everything behind them -- the triangular normaliser, the division, L*u*v*, the
aggregation -- is float64 in closed form: the exact value the float32 kernel is compared with by tolerance.  plan, resize_channels,
estimate_lambdas, score_map, candidates come from aggregated_approx_model."""
import math

import numpy as np

import aggregated_approx_model as approx

CHANNELS = 10
BINS = 6
U = 2.0 ** -24   # unit roundoff of float32


# ---- tolerances ---------------------------------------------------------------------------------------------------------------
def rounding_count(cell, radius):
    """float32 roundings on the longest path of k_fpdw's summation scheme to a bin / magnitude cell value: the separable
    normaliser (one fmaf per tap: 2 (2r + 1)), its scale, + k, the division, the bin weight (1 - w2, the product), the separable
    aggregation (one fmaf per tap, 2 * 2 cell at most) and its scale; rounded up to the issue's 2 (2r + 1) + 4 cell + 10"""
    return (2 * (2 * radius + 1) if radius > 0 else 0) + 4 * cell + 10


def rtol(cell, radius):
    """relative bound of the bin and magnitude channels (all addends are non-negative): 2 N u"""
    return 2 * rounding_count(cell, radius) * U


# L*u*v* per pixel, absolute, after the / 354.  With u = 2^-24: the gamma table entry, the float matrix coefficient, the product and
# two sums give X, Y, Z 5 u relative; L = 116 cbrt(Y) - 16 <= 100 errs by <= 116 (5/3 + 2 + 1) u + 100 u < 650 u absolute;
# the denominator 8 u, u' = 4 X / d <= 0.63 errs by 14 u relative, u' - u_n by < 10 u absolute; 13 L (u' - u_n): 1300 * 10 u from
# u', 13 * 0.45 * 650 u from L, 2 * 220 u from the products: < 17300 u; + 134 and / 354: 17300 u / 354 + 3 u.  v likewise.
ATOL_LUV = 17300 * U / 354 + 3 * U   # 3.1e-6


# ---- look-up table and gradient codes (exact) ----------------------------------------------------------------------------------
def gradient_lut(interpolate):
    """FpdwFeaturesFilter::createGradientLut: dict of 65536-entry arrays, index gx | gy << 8"""
    f32 = np.float32
    code = np.arange(65536)
    gX = (f32(1) * (code & 255).astype(f32) - f32(127)) / f32(255)
    gY = (f32(1) * (code >> 8).astype(f32) - f32(127)) / f32(255)
    magnitude = np.sqrt(gX * gX + gY * gY)
    PI, TWO_PI = f32(math.pi), f32(2 * math.pi)
    o = np.array([math.atan2(float(y), float(x)) for x, y in zip(gX, gY)], np.float64).astype(f32)
    o = np.where(o < 0, o + TWO_PI, o).astype(f32)
    o = np.where(o >= PI, o - PI, o).astype(f32)
    value2bin = f32(BINS) / PI
    if interpolate:
        b = o * value2bin
        bin1 = b.astype(np.int32)   # truncation
        bin2 = np.where(bin1 + 1 == BINS, 0, bin1 + 1).astype(np.int32)
        w2 = b - bin1.astype(f32)
        w1 = f32(1) - w2
    else:
        bin1 = (o * value2bin + f32(0.5)).astype(np.int32)
        bin1 = np.where(bin1 == BINS, 0, bin1).astype(np.int32)
        bin2 = np.zeros(65536, np.int32)
        w1, w2 = np.ones(65536, f32), np.zeros(65536, f32)
    assert magnitude.dtype == f32 and w1.dtype == f32 and w2.dtype == f32
    return dict(bin1=bin1, bin2=bin2, w1=w1, w2=w2, magnitude=magnitude)


_LUTS = {}


def lut(interpolate):
    if interpolate not in _LUTS:
        _LUTS[interpolate] = gradient_lut(interpolate)
    return _LUTS[interpolate]


def gradient_codes(plane):
    """GradientFilter(1) on a CV_8UC1 plane, BORDER_REPLICATE: gx | gy << 8"""
    p = np.pad(plane.astype(np.int64), 1, mode="edge")
    dx = p[1:-1, 2:] - p[1:-1, :-2]
    dy = p[2:, 1:-1] - p[:-2, 1:-1]
    gx = np.clip(np.rint(dx * 0.5 + 127), 0, 255).astype(np.int64)   # rint: half to even, like cvRound
    gy = np.clip(np.rint(dy * 0.5 + 127), 0, 255).astype(np.int64)
    return gx | (gy << 8)


def image_codes(oracle, bgr, fast_gradient):
    if fast_gradient:
        return gradient_codes(oracle.bgr2gray(bgr))
    mag = lut(False)["magnitude"]
    best = gradient_codes(bgr[:, :, 0])
    for ch in (1, 2):   # a later channel wins only with a strictly larger magnitude
        c = gradient_codes(bgr[:, :, ch])
        best = np.where(mag[best] < mag[c], c, best)
    return best


# ---- triangular filters in closed form (float64) -------------------------------------------------------------------------------
def _tap_matrix(n, samples, offsets, weights):
    """(len(samples), n) matrix of a 1-D filter sampled at `samples` with replicated border"""
    A = np.zeros((len(samples), n), np.float64)
    for j, s in enumerate(samples):
        for o, w in zip(offsets, weights):
            A[j, min(max(s + o, 0), n - 1)] += w
    return A


def check_triangular_limits(rows, cols, radius):
    """TriangularConvolutionFilter::applyTo's argument checks (TriangularConvolutionFilter.cpp:74-79)"""
    if rows <= radius:
        raise ValueError("TriangularConvolutionFilter: image must have at least %d rows, but had only %d" % (radius + 1, rows))
    if cols < 2 * radius + 2:
        raise ValueError("TriangularConvolutionFilter: image must have at least %d columns, but had only %d" % (2 * radius + 2, cols))


def triangular_smooth(img, radius):
    """TriangularConvolutionFilter(2 radius + 1, 1, 1, 0) on a (h, w) map"""
    h, w = img.shape
    check_triangular_limits(h, w, radius)
    off = list(range(-radius, radius + 1))
    wts = [radius + 1 - abs(t) for t in off]
    Ay, Ax = _tap_matrix(h, range(h), off, wts), _tap_matrix(w, range(w), off, wts)
    return (Ay @ img @ Ax.T) / float((radius + 1) ** 4)


def aggregate(desc, cell):
    """AggregationFilter(cell, true, false) on a (h, w, D) map: (h / cell, w / cell, D)"""
    h, w, _ = desc.shape
    check_triangular_limits(h, w, cell - 1)
    if cell % 2:
        off = list(range(-(cell - 1), cell))
        wts = [cell - abs(t) for t in off]
        norm = cell * cell / float(cell ** 4)
    else:
        off = list(range(-cell, cell))
        wts = [2 * t + 1 for t in range(cell)] + [2 * t + 1 for t in range(cell - 1, -1, -1)]
        norm = cell * cell / (4.0 * cell ** 4)
    Ay = _tap_matrix(h, [cell // 2 + j * cell for j in range(h // cell)], off, wts)
    Ax = _tap_matrix(w, [cell // 2 + j * cell for j in range(w // cell)], off, wts)
    rows = np.tensordot(Ay, desc, (1, 0))                                # (r, x, d)
    return np.tensordot(Ax, rows, (1, 1)).transpose(1, 0, 2) * norm      # (c, r, d) -> (r, c, d)


# ---- L*u*v* (OpenCV's documented CV_BGR2Luv on floats c / 255, float64) -----------------------------------------------------
def gamma_table():
    c = np.arange(256) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def normalized_luv(bgr):
    g = gamma_table()
    B, G, R = g[bgr[:, :, 0]], g[bgr[:, :, 1]], g[bgr[:, :, 2]]
    X = 0.412453 * R + 0.357580 * G + 0.180423 * B
    Y = 0.212671 * R + 0.715160 * G + 0.072169 * B
    Z = 0.019334 * R + 0.119193 * G + 0.950227 * B
    L = np.where(Y > 0.008856, 116.0 * np.cbrt(Y) - 16.0, 903.3 * Y)
    d = np.maximum(X + 15 * Y + 3 * Z, float(np.finfo(np.float32).eps))
    u = 13 * L * (4 * X / d - 0.19793943)
    v = 13 * L * (9 * Y / d - 0.46831096)
    return np.stack([L / 354, (u + 134) / 354, (v + 140) / 354], 2)


# ---- the filters ---------------------------------------------------------------------------------------------------------------
def params(cell, radius=None, fast_gradient=True, interpolate=False, constant=0.01):
    return dict(cell=cell, radius=cell if radius is None else radius, fast_gradient=fast_gradient, interpolate=interpolate,
                constant=float(np.float32(constant)))   # the C ABI carries the constant as a float


def features_image(oracle, bgr, p):
    """FpdwFeaturesFilter::applyTo: ((h, w, 10) float64, per-pixel (bin1, bin2) of the vote)"""
    T = lut(p["interpolate"])
    code = image_codes(oracle, bgr, p["fast_gradient"])
    M = T["magnitude"][code].astype(np.float64)
    Mn = M / (triangular_smooth(M, p["radius"]) + p["constant"]) if p["radius"] > 0 else M
    h, w = code.shape
    out = np.zeros((h, w, CHANNELS), np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    b1, b2 = T["bin1"][code], T["bin2"][code]
    if p["interpolate"]:
        out[yy, xx, b2] = T["w2"][code].astype(np.float64) * Mn
    out[yy, xx, b1] = T["w1"][code].astype(np.float64) * Mn
    out[:, :, BINS] = Mn
    out[:, :, BINS + 1:] = normalized_luv(bgr)
    return out, (b1, b2)


def features_cells(oracle, bgr, p):
    """the whole chain: (h / cell, w / cell, 10) float64"""
    desc, _ = features_image(oracle, bgr, p)
    return aggregate(desc, p["cell"])


def cell_bounds(p, approximated=False):
    """(rtol array, atol array) per channel of a cell map: bins and magnitude relative; L*u*v* cells are sums of cell^2 pixel
    values (alpha = cell^2) through the same aggregation roundings.  Approximated layers: the bilinear resize's two roundings more."""
    c = p["cell"]
    extra = 2 if approximated else 0
    r = np.full(CHANNELS, rtol(c, p["radius"]) + 2 * extra * U)
    a = np.zeros(CHANNELS)
    r[BINS + 1:] = 2 * (4 * c + 2 + extra) * U
    a[BINS + 1:] = ATOL_LUV * c * c
    return r, a


def pixel_bounds(p):
    r = np.full(CHANNELS, 2 * ((2 * (2 * p["radius"] + 1) if p["radius"] > 0 else 0) + 6) * U)
    a = np.zeros(CHANNELS)
    r[BINS + 1:] = 0
    a[BINS + 1:] = ATOL_LUV
    return r, a


def within(got, exact, r, a):
    """(ok, largest error in units of the bound)"""
    bound = r[None, None, :] * np.abs(exact) + a[None, None, :]
    err = np.abs(got.astype(np.float64) - exact)
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    return bool(np.all(err <= bound)), float(ratio.max())


# ---- BGR pyramid and feature layers --------------------------------------------------------------------------------------------
def bgr_layers(oracle, bgr, octave_layers, min_scale, max_scale):
    """[(info, (h, w, 3) uint8)] of ImagePyramid(octave_layers, min, max) on a CV_8UC3 image without image filter"""
    planes = []
    infos = None
    for ch in range(3):
        pyr = oracle.Pyramid(octave_layers=octave_layers, min_scale=min_scale, max_scale=max_scale)
        pyr.update(np.ascontiguousarray(bgr[:, :, ch]))
        infos = pyr.layers()
        planes.append([pyr.layer(k) for k in range(len(infos))])
        pyr.close()
    return [(infos[k], np.stack([planes[0][k], planes[1][k], planes[2][k]], 2)) for k in range(len(infos))]


def feature_layers(oracle, bgr, cfg, p, approximate, lambdas=None):
    """(layers, float64 feature maps in layer order, lambdas used or None); cfg: window_w, window_h, cell, n, min_window_width.
    Exact handles: every layer of the n-layers-per-octave pyramid.  Approximated: approx.plan's list; the approximated layers are the
    per-channel cv::resize of the float32 rounding of the octave's exact layer, times (float)pow(s, -lambda)."""
    h, w = bgr.shape[:2]
    min_scale, max_scale = approx.limits(cfg["window_w"], cfg["window_h"], cfg["cell"], cfg["n"], cfg["min_window_width"], w, h)
    if not approximate:
        layers, feats = [], []
        for info, img in bgr_layers(oracle, bgr, cfg["n"], min_scale, max_scale):
            f = features_cells(oracle, img, p)
            layers.append(dict(index=info["index"], approximated=0, parent=-1, rows=f.shape[0], cols=f.shape[1], scale=info["scale"],
                               scale_x=info["w"] / w, scale_y=info["h"] / h, s=1.0))
            feats.append(f)
        return layers, feats, None
    layers = approx.plan(cfg["window_w"], cfg["window_h"], cfg["cell"], cfg["n"], cfg["min_window_width"], w, h, estimate=lambdas is None)
    src = bgr_layers(oracle, bgr, 1, min_scale, max_scale)
    exact_pos = [i for i, L in enumerate(layers) if not L["approximated"]]
    assert len(src) == len(exact_pos)
    feats = [None] * len(layers)
    for (info, img), i in zip(src, exact_pos):
        assert info["scale"] == layers[i]["scale"]
        feats[i] = features_cells(oracle, img, p)
        assert feats[i].shape[:2] == (layers[i]["rows"], layers[i]["cols"])
    if lambdas is None:
        lambdas = approx.estimate_lambdas([feats[i] for i in exact_pos], [layers[i]["scale"] for i in exact_pos])
    lambdas = np.asarray(lambdas, np.float64)
    for i, L in enumerate(layers):
        if L["approximated"]:
            factor = np.array([math.pow(L["s"], -lam) for lam in lambdas], np.float64)
            parent = feats[L["parent"]].astype(np.float32)
            feats[i] = approx.resize_channels(oracle, parent, L["rows"], L["cols"]).astype(np.float64) * factor[None, None, :]
    return layers, feats, lambdas


def gap_threshold(layers, feats, weights, bias, p):
    """(threshold, model scores, score bound per layer): the midpoint of the largest gap between consecutive sorted scores among the
    model's top 200, which must be more than twice the score bound rtol sum |w f| + atol sum |w| of the windows next to it"""
    scores = [approx.score_map(f, weights, bias) for f in feats]
    bounds = []
    for L, f in zip(layers, feats):
        r, a = cell_bounds(p, bool(L["approximated"]))
        bounds.append(approx.score_map(np.abs(f) * r[None, None, :] + a[None, None, :], np.abs(weights), 0.0))
    flat = np.concatenate([s.ravel() for s in scores])
    bflat = np.concatenate([b.ravel() for b in bounds])
    order = np.argsort(-flat)[:200]
    top = flat[order]
    k = int(np.argmax(top[:-1] - top[1:]))
    gap = float(top[k] - top[k + 1])
    assert gap > 2 * float(bflat[order].max()), "the largest gap (%.3e) does not clear the score bound (%.3e)" % (gap, float(bflat[order].max()))
    return float(np.float32(0.5 * (top[k] + top[k + 1]))), scores, bounds
