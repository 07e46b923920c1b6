"""numpy restatement of imageprocessing::CompleteExtendedHogFilter (CompleteExtendedHogFilter.cpp:19-303), written from the cited
lines: float32 step by step where the reference computes in float, float64 where it computes in double, the reference's loop order
for every accumulation.  OpenCV is absent, so the reference's own filter cannot be compiled; the device code is compared against
this restatement bit for bit.

Readings made (the same k_fhog_desc made for FhogAggregationFilter): `1.f / sqrt(float)` is fp32 (1.f / sqrtf), std::min(alpha, x) on
floats, `0.5 * (h1 + h2 + h3 + h4)` and `0.2357 * t` are a float sum times a double literal, rounded to float on assignment."""
import math

import numpy as np

F = np.float32
EPS = F(1e-4)   # CompleteExtendedHogFilter.cpp:17

_atan2 = np.frompyfunc(math.atan2, 2, 1)   # libm, like the reference (numpy's own arctan2 may be a vectorised approximation)


def check_params(bin_count, signed, unsigned, cell_size=1):
    if cell_size < 1 or bin_count < 1:
        raise ValueError("cell size and bin count must be positive")
    if not signed and not unsigned:   # :23-24
        raise ValueError("signedGradients or unsignedGradients has to be true")
    if signed and unsigned and bin_count % 2 != 0:   # :25-26
        raise ValueError("the bin count has to be even")


def channels(bin_count, signed, unsigned):
    return bin_count + (bin_count // 2 if signed and unsigned else 0) + 4   # :65


def size(width, height, cell_size, bin_count, signed, unsigned):
    check_params(bin_count, signed, unsigned, cell_size)
    return height // cell_size, width // cell_size, channels(bin_count, signed, unsigned)   # :63-65


def gradient_lut(bin_count, signed, interpolate_bins):
    """the constructor's table (:31-58): index1, index2 (int32), weight1, weight2 (float32), each (512, 512) indexed [x, y]"""
    code = np.arange(512, dtype=np.float64) - 256
    g = code / (2. * 255.)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    direction = _atan2(gy, gx).astype(np.float64)
    magnitude = np.sqrt(gx * gx + gy * gy)
    if signed:
        direction = direction + math.pi
        bin_index = direction * float(bin_count) / (2 * math.pi)
    else:
        direction = np.where(direction < 0, direction + math.pi, direction)
        bin_index = direction * float(bin_count) / math.pi
    fl = np.floor(bin_index)
    if interpolate_bins:
        i1 = fl.astype(np.int64) % bin_count
        i2 = np.ceil(bin_index).astype(np.int64) % bin_count
        w2 = (magnitude * (bin_index - fl)).astype(F)
        w1 = (magnitude - w2.astype(np.float64)).astype(F)
    else:
        rounded = fl + ((bin_index - fl) >= 0.5)   # round(): halves away from zero, bin_index >= 0
        i1 = rounded.astype(np.int64) % bin_count
        i2 = i1
        w1 = magnitude.astype(F)
        w2 = np.zeros_like(w1)
    return i1.astype(np.int32), i2.astype(np.int32), w1, w2


def cell_lut(size_px, count, cell_size, interpolate_cells):
    """createLut (:72-103): index1, index2, weight1, weight2 per pixel row / column"""
    i1, i2 = np.zeros(size_px, np.int64), np.zeros(size_px, np.int64)
    w1, w2 = np.zeros(size_px, F), np.zeros(size_px, F)
    for m in range(size_px):
        if interpolate_cells:
            real = (float(m) + 0.5) / float(cell_size) - 0.5
            a = int(math.floor(real))
            b = a + 1
            v2 = F(real - a)
            v1 = F(F(1) - v2)
            if a < 0:
                a, v1 = b, F(0)
            elif b >= count:
                b, v2 = a, F(0)
            i1[m], i2[m], w1[m], w2[m] = a, b, v1, v2
        else:
            i1[m], i2[m], w1[m], w2[m] = m // cell_size, -1, F(1), F(0)
    return i1, i2, w1, w2


_LUTS = {}


def _lut(bin_count, signed, interpolate_bins):
    key = (bin_count, bool(signed), bool(interpolate_bins))
    if key not in _LUTS:
        _LUTS[key] = gradient_lut(*key)
    return _LUTS[key]


def initial_histograms(image, cell_size, bin_count, signed, interpolate_bins, interpolate_cells):
    """buildInitialHistograms (:105-161): (rows, cols, bin_count) float32, accumulated in the reference's raster scan"""
    image = np.asarray(image, np.uint8)
    rows, cols = image.shape[0] // cell_size, image.shape[1] // cell_size
    height, width = rows * cell_size, cols * cell_size
    li1, li2, lw1, lw2 = _lut(bin_count, signed, interpolate_bins)
    ri1, ri2, rw1, rw2 = cell_lut(image.shape[0], rows, cell_size, interpolate_cells)
    ci1, ci2, cw1, cw2 = cell_lut(image.shape[1], cols, cell_size, interpolate_cells)
    img = image.astype(np.int64)
    hist = np.zeros((rows, cols, bin_count), F)
    for y in range(height):
        for x in range(width):
            dx = img[y, min(width - 1, x + 1)] - img[y, max(0, x - 1)] + 256      # :126
            dy = img[min(height - 1, y + 1), x] - img[max(0, y - 1), x] + 256    # :127
            b1, b2, w1, w2 = li1[dx, dy], li2[dx, dy], lw1[dx, dy], lw2[dx, dy]
            if interpolate_cells:
                for (r, rw) in ((ri1[y], rw1[y]), (ri2[y], rw2[y])):
                    for (c, cw) in ((ci1[x], cw1[x]), (ci2[x], cw2[x])):
                        hist[r, c, b1] = hist[r, c, b1] + F(F(w1 * rw) * cw)
                        if interpolate_bins:
                            hist[r, c, b2] = hist[r, c, b2] + F(F(w2 * rw) * cw)
            else:
                r, c = ri1[y], ci1[x]
                hist[r, c, b1] = hist[r, c, b1] + w1
                if interpolate_bins:
                    hist[r, c, b2] = hist[r, c, b2] + w2
    return hist


def descriptors(hist, bin_count, signed, unsigned, alpha):
    """buildDescriptors (:163-303) from the (rows, cols, bin_count) histograms"""
    rows, cols = hist.shape[:2]
    half = bin_count // 2
    alpha = F(alpha)
    energies = np.zeros((rows, cols), F)
    for r in range(rows):
        for c in range(cols):
            e = F(0)
            if signed:   # :168-180
                for b in range(half):
                    u = F(hist[r, c, b] + hist[r, c, b + half])
                    e = F(e + F(u * u))
            else:        # :181-190
                for b in range(bin_count):
                    e = F(e + F(hist[r, c, b] * hist[r, c, b]))
            energies[r, c] = e
    both = signed and unsigned
    out = np.zeros((rows, cols, channels(bin_count, signed, unsigned)), F)

    def norm(a, b, c, d):
        return F(F(1) / np.sqrt(F(F(F(F(a + b) + c) + d) + EPS)))

    def half_sum(h):   # 0.5 * (h1 + h2 + h3 + h4): float sum, double product, rounded to float
        return F(0.5 * float(F(F(F(h[0] + h[1]) + h[2]) + h[3])))

    for r in range(rows):
        for c in range(cols):
            r0, r2 = max(0, r - 1), min(r + 1, rows - 1)
            c0, c2 = max(0, c - 1), min(c + 1, cols - 1)
            E = energies
            n = [norm(E[r0, c0], E[r0, c], E[r, c0], E[r, c]), norm(E[r0, c], E[r0, c2], E[r, c], E[r, c2]),
                 norm(E[r, c0], E[r, c], E[r2, c0], E[r2, c]), norm(E[r, c], E[r, c2], E[r2, c], E[r2, c2])]
            d = hist[r, c]
            if both:     # :218-226
                for b in range(half):
                    s = F(d[b] + d[b + half])
                    out[r, c, bin_count + b] = half_sum([min(alpha, F(s * k)) for k in n])
            t = [F(0)] * 4
            for b in range(bin_count):   # :234-244 / :283-293
                h = [min(alpha, F(d[b] * k)) for k in n]
                out[r, c, b] = half_sum(h)
                t = [F(t[k] + h[k]) for k in range(4)]
            base = bin_count + (half if both else 0)
            for k in range(4):           # :247-250 / :296-299
                out[r, c, base + k] = F(0.2357 * float(t[k]))
    return out


def cehog(image, cell_size, bin_count, signed, unsigned, interpolate_bins, interpolate_cells, alpha):
    """applyTo (:62-70)"""
    check_params(bin_count, signed, unsigned, cell_size)
    hist = initial_histograms(image, cell_size, bin_count, signed, interpolate_bins, interpolate_cells)
    return descriptors(hist, bin_count, signed, unsigned, alpha)


# ---- the tracker: ExtendedHogBasedMeasurementModel's pyramids, samples, peak and maxima ---------------------------------------------

def cv_round(v):
    """cvRound: half to even"""
    return int(np.rint(v))


def std_round(v):
    """std::round: halves away from zero"""
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def pyramid_limits(cell_cols, cell_size, min_width, max_width, octave_layers):
    """ExtendedHogFeatureExtractor::createPyramid (ExtendedHogFeatureExtractor.cpp:32-41) with the constructor's arguments (:76-84):
    (min scale, max scale)"""
    width = (cell_cols + 2) * cell_size
    min_w = (cell_cols + 2) * min_width // cell_cols
    max_w = (cell_cols + 2) * max_width // cell_cols
    inc = math.pow(0.5, 1. / octave_layers)
    min_sf, max_sf = width / max_w, width / min_w
    max_index = cv_round(math.log(min_sf) / math.log(inc))
    min_index = cv_round(math.log(max_sf) / math.log(inc))
    return math.pow(inc, max_index), math.pow(inc, min_index)


def plan_layers(width, height, cell_cols, cell_size, min_width, max_width, octave_layers):
    """ImagePyramid::createLayers(const Mat&) (ImagePyramid.cpp:170-198) for that pyramid: [(index, w, h, rows, cols, scale)] in index order"""
    min_s, max_s = pyramid_limits(cell_cols, cell_size, min_width, max_width, octave_layers)
    inc = math.pow(0.5, 1. / octave_layers)
    out = []
    for i in range(octave_layers):
        s = math.pow(inc, i)
        w, h = cv_round(width * s), cv_round(height * s)
        if max_s >= s >= min_s:
            out.append((i, w, h, h // cell_size, w // cell_size, s))
        s *= 0.5
        j = 1
        while s >= min_s and w > 1:
            w, h = (w + 1) // 2, (h + 1) // 2
            if s <= max_s:
                out.append((i + j * octave_layers, w, h, h // cell_size, w // cell_size, s))
            j += 1
            s *= 0.5
    return sorted(out)


def heat_layer(features, weights, bias):
    """ConvolutionFilter::applyTo (ConvolutionFilter.cpp:27-43): per channel the correlation with that channel of the kernel, anchor at
    the kernel centre, zero border, float32 sums over the kernel in row-major order; the channel results added in channel order onto
    (float)delta, delta = -bias"""
    rows, cols, D = features.shape
    kh, kw = weights.shape[:2]
    ay, ax = kh // 2, kw // 2
    sacc = np.zeros((rows, cols, D), F)
    for ky in range(kh):
        for kx in range(kw):
            oy, ox = ky - ay, kx - ax   # tap reads F[y + oy, x + ox]
            y0, y1 = max(0, -oy), min(rows, rows - oy)
            x0, x1 = max(0, -ox), min(cols, cols - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            prod = (weights[ky, kx][None, None, :] * features[y0 + oy:y1 + oy, x0 + ox:x1 + ox]).astype(F)
            sacc[y0:y1, x0:x1] = sacc[y0:y1, x0:x1] + prod
    heat = np.full((rows, cols), F(-F(bias)), F)
    for c in range(D):
        heat = heat + sacc[:, :, c]
    return heat


def ordered_dot(window, weights, bias):
    """the same arithmetic on one window of cells: per channel the row-major sum, then the channels onto delta"""
    kh, kw, D = weights.shape
    s = F(-F(bias))
    for c in range(D):
        acc = F(0)
        for ky in range(kh):
            for kx in range(kw):
                acc = F(acc + F(weights[ky, kx, c] * window[ky, kx, c]))
        s = F(s + acc)
    return s


def sample_window(x, y, width, height, layers, cell_cols, cell_rows, cell_size, octave_layers):
    """CellBasedPyramidFeatureExtractor::getLayer / getScaled (.cpp:58-69) + DirectPyramidFeatureExtractor::extract (.cpp:67-73,133-143):
    (layer position, bx, by) in cells, or None"""
    if width <= 0 or height <= 0 or not layers:
        return None
    inc = math.pow(0.5, 1. / octave_layers)
    power = math.log((cell_cols * cell_size) / float(width)) / math.log(inc)
    real = std_round(power) - layers[0][0]
    if real < 0 or real >= len(layers):
        return None
    _, _, _, rows, cols, scale = layers[real]
    bx = cv_round((x - int_div(width, 2)) * scale / cell_size)
    by = cv_round((y - int_div(height, 2)) * scale / cell_size)
    if bx < 0 or by < 0 or bx + cell_cols > cols or by + cell_rows > rows:
        return None
    return real, bx, by


def int_div(a, b):
    """C++ int division (truncation)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def patch_window(x, y, width, height, layers, cell_cols, cell_rows, cell_size, octave_layers):
    """ExtendedHogFeatureExtractor::extract (.cpp:95-107): (layer position, bx, by) in the layer's pixels, or None"""
    if width <= 0 or height <= 0 or not layers:
        return None
    width = std_round((cell_cols + 2) / cell_cols * width)
    height = std_round((cell_rows + 2) / cell_rows * height)
    pw, ph = (cell_cols + 2) * cell_size, (cell_rows + 2) * cell_size
    inc = math.pow(0.5, 1. / octave_layers)
    real = std_round(math.log(pw / float(width)) / math.log(inc)) - layers[0][0]
    if real < 0 or real >= len(layers):
        return None
    _, w, h, _, _, scale = layers[real]
    bx, by = cv_round((x - int_div(width, 2)) * scale), cv_round((y - int_div(height, 2)) * scale)
    if bx < -cell_size or bx + pw > w + cell_size or by < -cell_size or by + ph > h + cell_size:
        return None
    return real, bx, by


def mirrored_patch(gray, bx, by, pw, ph):
    """createIndexLut / createPatchData (.cpp:112-115,132-143)"""
    def lut(size, start, n):
        idx = np.arange(start, start + n)
        idx = np.where(idx < 0, -idx - 1, idx)
        return np.where(idx >= size, 2 * size - idx - 1, idx)
    return np.ascontiguousarray(gray[np.ix_(lut(gray.shape[0], by, ph), lut(gray.shape[1], bx, pw))])


def offered_positions(rows, cols, cell_rows, cell_cols):
    """the loop bounds of getHeatPeak / createGoodNegativeExamples (:441-443): (row range, column range), the last full position excluded"""
    return (range(cell_rows // 2, rows + cell_rows // 2 - cell_rows), range(cell_cols // 2, cols + cell_cols // 2 - cell_cols))


def heat_peak(heats, layers, cell_cols, cell_rows, cell_size):
    """getHeatPeak (:434-456): (found, score, (x, y, w, h)); strict > in layer / row / column order"""
    best, bounds, found = None, (0, 0, 0, 0), False
    for heat, (_, _, _, rows, cols, scale) in zip(heats, layers):
        rr, cr = offered_positions(rows, cols, cell_rows, cell_cols)
        for r in rr:
            for c in cr:
                s = heat[r, c]
                if (best is None and s > -np.inf) or (best is not None and s > best):
                    best, found = s, True
                    bounds = (cv_round((c - cell_cols // 2) * cell_size / scale), cv_round((r - cell_rows // 2) * cell_size / scale),
                              cv_round(cell_cols * cell_size / scale), cv_round(cell_rows * cell_size / scale))
    return found, best, bounds


def heat_maxima(heats, layers, cell_cols, cell_rows, cell_size, threshold):
    """the scan of createGoodNegativeExamples (:621-652): [(score, x, y, w, h)] in scan order"""
    out = []
    thr = F(threshold)
    for heat, (_, _, _, rows, cols, scale) in zip(heats, layers):
        rr, cr = offered_positions(rows, cols, cell_rows, cell_cols)
        for r in rr:
            for c in cr:
                s = heat[r, c]
                if s > thr and all(s >= heat[r + dr, c + dc] for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0)):
                    out.append((s, cv_round((c - cell_cols // 2) * cell_size / scale), cv_round((r - cell_rows // 2) * cell_size / scale),
                                cv_round(cell_cols * cell_size / scale), cv_round(cell_rows * cell_size / scale)))
    return out


# ---- the measurement model's host rules ---------------------------------------------------------------------------------------------

def cell_grid(width, height, cell_count):
    """the cell-grid rule of ExtendedHogBasedMeasurementModel::initialize (ExtendedHogBasedMeasurementModel.cpp:221-228): (columns, rows)"""
    aspect = float(height) / float(width)
    if aspect < 1:
        rows = cv_round(math.sqrt(aspect * cell_count))
        cols = cv_round(rows / aspect)
    else:
        cols = cv_round(math.sqrt(cell_count / aspect))
        rows = cv_round(aspect * cols)
    return cols, rows


def max_width(image_w, image_h, target_w, target_h):
    """:234-241"""
    aspect = float(target_h) / float(target_w)
    return int(image_h / aspect) if aspect > float(image_h) / float(image_w) else image_w


def ehog_feature_length(patch_w, patch_h, bins, cell_w, cell_h, signed_and_unsigned, alpha=0.2, channels=2):
    """ExtendedHogFilter: the constructor's checks (ExtendedHogFilter.cpp:24-31,42-51) and the grid of applyTo (:55-56); -1 where invalid"""
    cell_h = cell_h or cell_w
    if channels not in (1, 2, 4) or bins <= 0 or cell_w <= 0 or cell_h <= 0 or not alpha > 0 or (signed_and_unsigned and bins % 2):
        return -1
    if patch_w < 1 or patch_h < 1:
        return -1
    rows, cols = cv_round(patch_h / float(cell_h)), cv_round(patch_w / float(cell_w))
    if rows < 1 or cols < 1:
        return -1
    return rows * cols * (bins + (bins // 2 if signed_and_unsigned else 0) + 4)


def overlap(a, b):
    """computeOverlap (:694-698) of rectangles (x, y, w, h)"""
    x0, y0 = max(a[0], b[0]), max(a[1], b[1])
    x1, y1 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    inter = float((x1 - x0) * (y1 - y0)) if x1 > x0 and y1 > y0 else 0.0
    return inter / (float(a[2] * a[3]) + float(b[2] * b[3]) - inter)


def good_negative_boxes(maxima, target_bounds, positive_overlap=0.5, negative_overlap=0.5):
    """createGoodNegativeExamples behind the scan (:646,653-667): overlap filter, ascending sort, greedy suppression from the best"""
    cand = [(m[0], tuple(int(v) for v in m[1:])) for m in maxima if overlap(target_bounds, m[1:]) < positive_overlap]
    cand.sort(key=lambda c: c[0])
    out = []
    while cand:
        box = cand.pop()[1]
        out.append(box)
        cand = [c for c in cand if not overlap(box, c[1]) > negative_overlap]
    return out
