"""CPU model of the integral-image feature family, written from the reference: IntegralImageFilter.cpp:18-21 (cv::integral, CV_32S),
DirectImageFeatureExtractor.cpp:42-52 (sample windows), HaarFeatureFilter.cpp:41-158, IntegralGradientFilter.cpp:23-85,
GradientSumFilter.cpp:22-60 and UnitNormFilter(NORM_L2).  Plain numpy; it never calls the library under test.

Every float step of the reference is a float32 step here (np.float32 scalars, or float32 arrays whose element-wise operations round
once per operation like the C expressions do), cvRound is np.rint on the value promoted to float64, integer sums wrap to int32.
Each extraction also returns the validity of every sample: the patch exists (it lies inside the (H + 1) x (W + 1) integral image)
and every read of the filter lies inside the integral image."""
import numpy as np

F = np.float32
TYPE_2RECTANGLE, TYPE_3RECTANGLE, TYPE_4RECTANGLE, TYPE_CENTER_SURROUND, TYPES_ALL = 1, 2, 4, 8, 15


def cv_round(v):
    """cvRound: the value as a double, rounded half to even"""
    return int(np.rint(np.float64(v)))


def bgr2gray(bgr):
    """cv::cvtColor(BGR2GRAY) on 8-bit images (GrayscaleFilter.cpp:18-24)"""
    a = np.asarray(bgr, np.uint8).astype(np.int64)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def integral(gray):
    """cv::integral with sdepth CV_32S, one pixel at a time: I[y + 1][x + 1] = I[y][x + 1] + (sum of row y up to x)"""
    g = np.asarray(gray, np.uint8)
    h, w = g.shape
    out = np.zeros((h + 1, w + 1), np.int64)
    for y in range(h):
        run = 0
        row = g[y].tolist()
        above = out[y]
        cur = out[y + 1]
        for x in range(w):
            run += row[x]
            cur[x + 1] = above[x + 1] + run
    assert out.max() <= 2 ** 31 - 1
    return out.astype(np.int32)


def integral_fast(gray):
    """the same by two cumulative sums (tests/test_integral_host.py checks the two against each other)"""
    g = np.asarray(gray, np.uint8).astype(np.int64)
    out = np.zeros((g.shape[0] + 1, g.shape[1] + 1), np.int64)
    out[1:, 1:] = g.cumsum(0).cumsum(1)
    return out.astype(np.int32)


# ---- sample windows ---------------------------------------------------------------------------------------------------------------
def patch_origin(sample, iw, ih):
    """(x0, y0, exists) of DirectImageFeatureExtractor::extract on an iw x ih integral image; C integer division truncates"""
    x, y, w, h = (int(v) for v in sample)
    x0 = x - int(w / 2)
    y0 = y - int(h / 2)
    exists = w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= iw and y0 + h <= ih
    return x0, y0, exists


# ---- HaarFeatureFilter ------------------------------------------------------------------------------------------------------------
def haar_grid(count):
    step = F(1) / F(count + 1)
    return np.array([F(i + 1) * step for i in range(count)], np.float32)


def haar_features(sizes=(0.2, 0.4), xs=None, ys=None, types=TYPES_ALL):
    """buildFeatures (HaarFeatureFilter.cpp:53-136): list of (rects [(x, y, w, h)], weights, factor, area), all np.float32"""
    xs = haar_grid(5) if xs is None else xs
    ys = xs if ys is None else ys
    feats = []
    for size in sizes:
        size = F(size)
        for y in ys:
            for x in xs:
                x, y = F(x), F(y)
                bx, by, bw, bh = x - size / F(2), y - size / F(2), size, size
                if bx < F(0) or bx + bw > F(1) or by < F(0) or by + bh > F(1):
                    continue
                area = bw * bh
                if types & TYPE_2RECTANGLE:
                    feats.append(([(bx, by, F(0.5) * bw, bh), (bx + F(0.5) * bw, by, F(0.5) * bw, bh)], [F(1), F(-1)], F(255) * F(1) / F(2), area))
                    feats.append(([(bx, by, bw, F(0.5) * bh), (bx, by + F(0.5) * bh, bw, F(0.5) * bh)], [F(1), F(-1)], F(255) * F(1) / F(2), area))
                if types & TYPE_3RECTANGLE:
                    feats.append(([(bx, by, bw / F(3), bh), (bx + bw / F(3), by, bw / F(3), bh), (bx + F(2) * bw / F(3), by, bw / F(3), bh)],
                                  [F(1), F(-2), F(1)], F(255) * F(2) / F(3), area))
                    feats.append(([(bx, by, bw, bh / F(3)), (bx, by + bh / F(3), bw, bh / F(3)), (bx, by + F(2) * bh / F(3), bw, bh / F(3))],
                                  [F(1), F(-2), F(1)], F(255) * F(2) / F(3), area))
                if types & TYPE_4RECTANGLE:
                    feats.append(([(bx, by, bw / F(2), bh / F(2)), (bx + bw / F(2), by + bh / F(2), bw / F(2), bh / F(2)),
                                   (bx + bw / F(2), by, bw / F(2), bh / F(2)), (bx, by + bh / F(2), bw / F(2), bh / F(2))],
                                  [F(1), F(1), F(-1), F(-1)], F(255) * F(1) / F(2), area))
                if types & TYPE_CENTER_SURROUND:
                    feats.append(([(bx, by, bw, bh), (bx + bw / F(4), by + bh / F(4), bw / F(2), bh / F(2))], [F(1), F(-4)],
                                  F(255) * F(3) / F(4), area))
    for rects, weights, factor, area in feats:
        assert all(type(v) is np.float32 for r in rects for v in r) and type(factor) is np.float32 and type(area) is np.float32
    return feats


def haar_table(feats):
    """the feature list as arrays: rects [n, 4, 4] (unused rectangles zero, weight zero), weights [n, 4], counts, factor, area"""
    n = len(feats)
    rects = np.zeros((n, 4, 4), np.float32)
    weights = np.zeros((n, 4), np.float32)
    counts = np.zeros(n, np.int32)
    factor = np.zeros(n, np.float32)
    area = np.zeros(n, np.float32)
    for i, (r, w, f, a) in enumerate(feats):
        counts[i] = len(r)
        rects[i, :len(r)] = np.array(r, np.float32)
        weights[i, :len(w)] = np.array(w, np.float32)
        factor[i], area[i] = f, a
    return rects, weights, counts, factor, area


def _wrap32(a):
    return ((np.asarray(a, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31)


def haar_extract(integral_image, feats, samples):
    """HaarFeatureFilter::applyTo (:138-158) per sample -> (features f32 [n, F], valid bool [n]).  Vectorised over the features of a
    sample: every array operation below is one float32 (or integer) operation per element, in the reference's order."""
    I = np.asarray(integral_image, np.int64)
    ih, iw = I.shape
    rects, weights, counts, factor, area = haar_table(feats)
    used = np.arange(4)[None, :] < counts[:, None]
    out = np.zeros((len(samples), len(feats)), np.float32)
    valid = np.zeros(len(samples), bool)
    for s, sample in enumerate(samples):
        x0, y0, exists = patch_origin(sample, iw, ih)
        if not exists or not len(feats):
            valid[s] = exists
            continue
        cols, rows = F(int(sample[2])), F(int(sample[3]))
        x1 = np.rint((rects[:, :, 0] * cols).astype(np.float64)).astype(np.int64)
        x2 = np.rint(((rects[:, :, 0] + rects[:, :, 2]) * cols).astype(np.float64)).astype(np.int64)
        y1 = np.rint((rects[:, :, 1] * rows).astype(np.float64)).astype(np.int64)
        y2 = np.rint(((rects[:, :, 1] + rects[:, :, 3]) * rows).astype(np.float64)).astype(np.int64)
        # every read of a used rectangle inside the integral image; an edge at 1.0 reads column `cols` / row `rows` of the patch
        inside = (x0 + x1 >= 0) & (x0 + x2 < iw) & (y0 + y1 >= 0) & (y0 + y2 < ih) & (x0 + x2 >= 0) & (x0 + x1 < iw) & (y0 + y2 >= 0) & (y0 + y1 < ih)
        if not inside[used].all():
            continue
        valid[s] = True
        x1, x2, y1, y2 = (np.where(used, v, 0) for v in (x1, x2, y1, y2))
        area_sum = _wrap32(I[y0 + y1, x0 + x1] + I[y0 + y2, x0 + x2] - I[y0 + y1, x0 + x2] - I[y0 + y2, x0 + x1])
        value = np.zeros(len(feats), np.float32)
        for j in range(4):
            term = weights[:, j] * area_sum[:, j].astype(np.float32)
            value = np.where(used[:, j], value + term, value)
        out[s] = value / (factor * area * cols * rows)
    assert out.dtype == np.float32
    return out, valid


# ---- IntegralGradientFilter -------------------------------------------------------------------------------------------------------
def _trunc_div(a, d):
    return np.sign(a) * (np.abs(a) // d)


def gradient_patches(integral_image, rows, cols, samples):
    """IntegralGradientFilter(rows, cols)::applyTo (IntegralGradientFilter.cpp:23-85) per sample -> (u8 [n, rows, cols, 2], valid)"""
    I = np.asarray(integral_image, np.int64)
    ih, iw = I.shape
    out = np.zeros((len(samples), rows, cols, 2), np.uint8)
    valid = np.zeros(len(samples), bool)
    for s, sample in enumerate(samples):
        x0, y0, exists = patch_origin(sample, iw, ih)
        if not exists:
            continue
        width, height = int(sample[2]) - 1, int(sample[3]) - 1
        rx = max(1, cv_round(np.float64(width - 1) / np.float64(cols + 2)))
        ry = max(1, cv_round(np.float64(height - 1) / np.float64(rows + 2)))
        sx = np.float64(width - 3 * rx) / np.float64(cols - 1)
        sy = np.float64(height - 3 * ry) / np.float64(rows - 1)
        half = ry * rx
        r = y0 + np.rint(np.float64(ry) + np.arange(rows, dtype=np.float64) * sy).astype(np.int64)
        c = x0 + np.rint(np.float64(rx) + np.arange(cols, dtype=np.float64) * sx).astype(np.int64)
        oy = [-ry, 0, ry, 2 * ry]
        ox = [-rx, 0, rx, 2 * rx]
        if min(r.min() + oy[0], c.min() + ox[0]) < 0 or r.max() + oy[3] >= ih or c.max() + ox[3] >= iw:
            continue
        valid[s] = True
        R, Cc = r[:, None], c[None, :]

        def p(iy, ix):
            return I[R + oy[iy], Cc + ox[ix]]
        p1, p2 = p(0, 1), p(0, 2)
        p3, p4, p5, p6 = p(1, 0), p(1, 1), p(1, 2), p(1, 3)
        p7, p8, p9, p10 = p(2, 0), p(2, 1), p(2, 2), p(2, 3)
        p11, p12 = p(3, 1), p(3, 2)
        top = p1 - p2 - p4 + p5
        bottom = p8 - p9 - p11 + p12
        left = p3 - p4 - p7 + p8
        right = p5 - p6 - p9 + p10
        dx = _trunc_div(_wrap32(right - left), 2 * half)
        dy = _trunc_div(_wrap32(bottom - top), 2 * half)
        out[s, :, :, 0] = ((dx + 127) & 255).astype(np.uint8)
        out[s, :, :, 1] = ((dy + 127) & 255).astype(np.uint8)
    return out, valid


# ---- GradientSumFilter ------------------------------------------------------------------------------------------------------------
def gradient_sums(grad, cell_rows, cell_cols):
    """GradientSumFilter(cell_rows, cell_cols)::applyTo (GradientSumFilter.cpp:22-60) on [n, rows, cols, 2] u8 -> f32 [n, cells * 4];
    the four float32 sums of a cell are accumulated in j (rows) then i (columns) order"""
    g = np.asarray(grad, np.uint8)
    n, rows, cols = g.shape[:3]
    if rows % cell_rows != 0:
        raise ValueError("GradientSumFilter: image row count (%d) is not divisible by cell count (%d)" % (rows, cell_rows))
    if cols % cell_cols != 0:
        raise ValueError("GradientSumFilter: image column count (%d) is not divisible by cell count (%d)" % (cols, cell_cols))
    ch, cw = rows // cell_rows, cols // cell_cols
    normalizer = F(1) / F(127)
    d = normalizer * (g.astype(np.int32) - 127).astype(np.float32)          # [n, rows, cols, 2]
    d = d.reshape(n, cell_rows, ch, cell_cols, cw, 2)
    acc = np.zeros((n, cell_rows, cell_cols, 4), np.float32)
    for j in range(ch):
        for i in range(cw):
            v = d[:, :, j, :, i, :]
            acc[..., 0] = acc[..., 0] + v[..., 0]
            acc[..., 1] = acc[..., 1] + v[..., 1]
            acc[..., 2] = acc[..., 2] + np.abs(v[..., 0])
            acc[..., 3] = acc[..., 3] + np.abs(v[..., 1])
    assert acc.dtype == np.float32
    return acc.reshape(n, cell_rows * cell_cols * 4)


def unit_norm_l2(vectors):
    """UnitNormFilter(NORM_L2) in float64: v / (|v| + 1e-4f)"""
    v = np.asarray(vectors, np.float32).astype(np.float64)
    norm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    return v / (norm + np.float64(np.float32(1e-4)))


def surf_extract(integral_image, gradient_count, cell_count, samples):
    """createSurfExtractor's patch filters -> (unnormalised f32 sums, float64 normalised descriptor, valid)"""
    grad, valid = gradient_patches(integral_image, gradient_count, gradient_count, samples)
    sums = gradient_sums(grad, cell_count, cell_count)
    sums[~valid] = 0
    return sums, unit_norm_l2(sums), valid


def ulp_distance(got, want64):
    """|got - want| in units of the float32 spacing at want (float64 reference)"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    spacing = np.spacing(np.maximum(np.abs(want32), np.float32(2.0 ** -126))).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64)) / spacing


# ---- the sample generator of the device tests ------------------------------------------------------------------------------------------
def make_samples(width, height, seed=7, n_random=560):
    """About 600 samples {x, y, w, h} on a width x height frame (integral image (height + 1) x (width + 1)): random windows with
    widths and heights 3..121 (w != h, odd values), windows flush with each border of the integral image, windows one pixel outside
    each border, the full image, and duplicates."""
    rng = np.random.default_rng(seed)
    iw, ih = width + 1, height + 1
    out = []

    def centred(x0, y0, w, h):   # the sample whose patch origin is (x0, y0)
        out.append((x0 + w // 2, y0 + h // 2, w, h))
    for _ in range(n_random):
        w, h = int(rng.integers(3, 122)), int(rng.integers(3, 122))
        if w == h:
            h = h + 1 if h < 121 else h - 1
        centred(int(rng.integers(0, iw - w + 1)), int(rng.integers(0, ih - h + 1)), w, h)
    for w, h in [(3, 5), (4, 4), (7, 3), (20, 31), (33, 20), (121, 77), (64, 121), (21, 21)]:
        centred(0, 17, w, h)                 # flush left
        centred(13, 0, w, h)                 # flush top
        centred(iw - w, 9, w, h)             # flush right: the patch holds the last column of the integral image
        centred(11, ih - h, w, h)            # flush bottom
        centred(iw - w, ih - h, w, h)        # corner
        centred(-1, 17, w, h)                # one pixel outside each border
        centred(13, -1, w, h)
        centred(iw - w + 1, 9, w, h)
        centred(11, ih - h + 1, w, h)
        centred(iw - w - 1, ih - h - 1, w, h)   # one short of flush: an edge at 1.0 still reads inside the integral image
    centred(0, 0, iw, ih)                    # the whole integral image
    centred(0, 0, width, height)             # the whole frame
    out.extend(out[5:25])                    # duplicates
    out.append((50, 50, 0, 10))              # degenerate sizes: no patch
    out.append((50, 50, 10, -3))
    return np.array(out, np.int32)
