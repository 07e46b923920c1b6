"""CPU model of the integral HOG family ("ihog" / "iehog", AdaptiveTracking.cpp:189-213):
IntegralFeatureExtractor(DirectImageFeatureExtractor[Grayscale, IntegralImage | IntegralGradientFilter, GradientBinningFilter,
<histogram filter>]), optionally inside a PatchResizingFeatureExtractor.  It chains tests/integral_model.gradient_patches, the
oracle's GradientBinningFilter and histogram filters (HogFilter, SpatialHistogramFilter, PyramidHogFilter,
SpatialPyramidHistogramFilter), and for ExtendedHogFilter the oracle's cell histograms with tests/ehog_model.descriptors.  It never
calls the library under test.  The two wrapper extractors are integer maps of a sample, written from IntegralFeatureExtractor.hpp:
36-47 and PatchResizingFeatureExtractor.hpp:41-52."""
import numpy as np

import ehog_model
import integral_model

HIST_HOG, HIST_SPATIAL, HIST_PYRAMID_HOG, HIST_SPATIAL_PYRAMID = 0, 1, 2, 3


def cv_round(v):
    return int(np.rint(np.float64(v)))


# ---- the wrapper extractors: what the inner extractor's extract(x, y, width, height) receives ------------------------------------------
def integral_extractor_map(sample):
    """IntegralFeatureExtractor::extract: (x + (width odd), y + (height odd), width + 1, height + 1)"""
    x, y, w, h = (int(v) for v in sample)
    return (x + (0 if w % 2 == 0 else 1), y + (0 if h % 2 == 0 else 1), w + 1, h + 1)


def patch_resizing_map(sample, factor, x_offset=0.0, y_offset=0.0):
    """PatchResizingFeatureExtractor::extract: cvRound of double expressions"""
    x, y, w, h = (int(v) for v in sample)
    return (cv_round(x + np.float64(x_offset) * w), cv_round(y + np.float64(y_offset) * h), cv_round(np.float64(factor) * w),
            cv_round(np.float64(factor) * h))


def map_samples(samples, scale=1.0, integral=True):
    """the samples of the tracker -> the samples of the innermost DirectImageFeatureExtractor, outer wrapper first:
    PatchResizingFeatureExtractor(scale) when scale != 1, then IntegralFeatureExtractor.  The tracking apps read `scale` as a float
    (AdaptiveTracking.cpp:141) and hand it to the double parameter of the wrapper: 1.1 arrives as 1.10000002384, so a width of 15
    becomes cvRound(16.5000004) = 17 where the double 1.1 would give the even 16"""
    factor = np.float64(np.float32(scale))
    out = []
    for s in np.asarray(samples).reshape(-1, 4):
        s = tuple(int(v) for v in s)
        if scale != 1.0:
            s = patch_resizing_map(s, factor)
        if integral:
            s = integral_extractor_map(s)
        out.append(s)
    return np.array(out, np.int32).reshape(-1, 4)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def cell_grid(rows, cols, cell, cell_h=0):
    return cv_round(rows / float(cell_h or cell)), cv_round(cols / float(cell))


def hist_feature_length(grid, kind, bins, cell=0, block=1, levels=0, signed_and_unsigned=False, concatenate=False, cell_h=0, block_h=0):
    """floats per sample of the four histogram filters on a rows x cols patch; -1 where the filter refuses the patch"""
    rows, cols = grid
    if kind in (HIST_HOG, HIST_SPATIAL):
        if cell <= 0 or block <= 0:
            return -1
        r, c = cell_grid(rows, cols, cell, cell_h)
        bh = block_h or block
        br, bc = r - bh + 1, c - block + 1
        if r < 1 or c < 1 or br < 1 or bc < 1:
            return -1
        if kind == HIST_HOG:
            if signed_and_unsigned and bins % 2:
                return -1
            return br * bc * block * bh * (bins + (bins // 2 if signed_and_unsigned else 0))
        if block == 1 and bh == 1:
            return r * c * bins
        return br * bc * (block * bh * bins if concatenate else bins)
    if levels < 1 or levels > 5:
        return -1
    count = sum(4 ** l for l in range(levels))
    if kind == HIST_PYRAMID_HOG:
        if signed_and_unsigned and bins % 2:
            return -1
        return count * (bins + (bins // 2 if signed_and_unsigned else 0))
    return count * bins


def feature_length(case):
    """floats per sample of a case (the dictionaries of CASES below); -1 where it is refused"""
    rows, cols = case["grid"]
    bins = case["bins"]
    if not (2 <= rows <= 64 and 2 <= cols <= 64) or not 1 <= bins <= 255:
        return -1
    if case.get("patch", (cols, rows)) != (cols, rows) or case.get("filter_bins", bins) != bins:
        return -1
    if case["filter"] == "ehog":
        return ehog_model.ehog_feature_length(cols, rows, bins, case["cell"], case.get("cell_h", 0), case.get("sau", False), case.get("alpha", 0.2),
                                              4 if case.get("interpolate_bins") else 2)
    return hist_feature_length((rows, cols), case["filter"], bins, case.get("cell", 0), case.get("block", 1), case.get("levels", 0),
                               case.get("sau", False), case.get("concatenate", False))


def features(oracle, integral_image, case, samples):
    """the feature rows of `samples` (what the innermost extractor receives) -> (f32 [n, F], valid bool [n]); invalid rows are zero"""
    rows, cols = case["grid"]
    bins = case["bins"]
    grad, valid = integral_model.gradient_patches(integral_image, rows, cols, samples)
    F = feature_length(case)
    assert F > 0
    out = np.zeros((len(samples), F), np.float32)
    for i in np.nonzero(valid)[0]:
        binimg = oracle.gradient_binning(np.ascontiguousarray(grad[i]), bins, bool(case.get("signed")), bool(case.get("interpolate_bins")))
        f, ip, sau = case["filter"], bool(case.get("interpolate")), bool(case.get("sau"))
        if f == HIST_HOG:
            v = oracle.hog_filter(binimg, bins, case["cell"], case.get("block", 1), interpolate=ip, signed_and_unsigned=sau)
        elif f == HIST_SPATIAL:
            v = oracle.spatial_histogram(binimg, bins, case["cell"], case.get("block", 1), interpolate=ip, concatenate=bool(case.get("concatenate")),
                                         normalization=case.get("normalization", 0))
        elif f == HIST_PYRAMID_HOG:
            v = oracle.pyramid_hog(binimg, bins, case["levels"], interpolate=ip, signed_and_unsigned=sau)
        elif f == HIST_SPATIAL_PYRAMID:
            v = oracle.spatial_pyramid_histogram(binimg, bins, case["levels"], interpolate=ip, normalization=case.get("normalization", 0))
        else:   # ExtendedHogFilter: HistogramFilter::createCellHistograms, then the descriptors
            r, c = cell_grid(rows, cols, case["cell"], case.get("cell_h", 0))
            cells = np.asarray(oracle.spatial_histogram(binimg, bins, case["cell"], 1, interpolate=ip, normalization=0, cell_h=case.get("cell_h", 0)),
                               np.float32).reshape(r, c, bins)
            v = ehog_model.descriptors(cells, bins, sau, True, case.get("alpha", 0.2))
        out[i] = np.asarray(v, np.float32).ravel()
    return out, valid


def make_frame(width, height, seed):
    """uniform noise over a smooth ramp, gray: the gradient directions vary, so every bin is hit"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    ramp = 30.0 + 110.0 * xx / max(width - 1, 1) + 60.0 * yy / max(height - 1, 1)
    return np.clip(np.rint(ramp + rng.uniform(-45, 45, (height, width))), 0, 255).astype(np.uint8)


# ---- the cases of the device tests: the smallest shapes at which the kernel can go wrong ------------------------------------------------
def _crossed(name, base, sau_bins):
    """binning interpolation x cell interpolation x signedAndUnsigned (which needs an even bin count and signed gradients)"""
    out = {}
    for ib in (False, True):
        for ic in (False, True):
            for sau in (False, True):
                c = dict(base, interpolate_bins=ib, interpolate=ic, sau=sau)
                if sau:
                    c.update(bins=sau_bins, signed=True)
                out["%s-%s-%s-%s" % (name, "bins4" if ib else "bins2", "icell" if ic else "plain", "sau" if sau else "single")] = c
    return out


DEFAULT = dict(grid=(30, 30), bins=9, signed=False, interpolate_bins=True, filter=HIST_SPATIAL, cell=6, block=1, interpolate=False, normalization=1)
CASES = {"default": DEFAULT}   # the reference's default ihog configuration
CASES.update(_crossed("hog30", dict(grid=(30, 30), bins=9, filter=HIST_HOG, cell=5, block=2), 8))
CASES.update({
    "spatial7x5-blocks": dict(grid=(7, 5), bins=9, interpolate_bins=True, filter=HIST_SPATIAL, cell=2, block=2, interpolate=True, concatenate=True,
                              normalization=2),
    "hog7x5": dict(grid=(7, 5), bins=9, signed=True, filter=HIST_HOG, cell=2, block=1),
    "hog2x2": dict(grid=(2, 2), bins=4, signed=True, interpolate_bins=True, filter=HIST_HOG, cell=1, block=1, sau=True),
    "spatial2x2": dict(grid=(2, 2), bins=9, filter=HIST_SPATIAL, cell=1, block=1, interpolate=True, normalization=3),
    "spatial64": dict(grid=(64, 64), bins=9, interpolate_bins=True, filter=HIST_SPATIAL, cell=4, block=1, interpolate=True, normalization=1),
    "hog64": dict(grid=(64, 64), bins=9, filter=HIST_HOG, cell=4, block=1),
    "phog32-3": dict(grid=(32, 32), bins=8, signed=True, interpolate_bins=True, filter=HIST_PYRAMID_HOG, levels=3, sau=True),
    "phog32-2": dict(grid=(32, 32), bins=9, filter=HIST_PYRAMID_HOG, levels=2, interpolate=True),
    "spyramid32-2": dict(grid=(32, 32), bins=9, interpolate_bins=True, filter=HIST_SPATIAL_PYRAMID, levels=2, normalization=3),
    "spyramid32-3": dict(grid=(32, 32), bins=9, filter=HIST_SPATIAL_PYRAMID, levels=3, interpolate=True, normalization=1),
    "ehog20x12": dict(grid=(20, 12), bins=9, interpolate_bins=True, filter="ehog", cell=4, interpolate=True, alpha=0.2),
})
CASES.update(_crossed("ehog30", dict(grid=(30, 30), bins=9, filter="ehog", cell=6, alpha=0.2), 18))
EHOG_MODEL_CASE = "ehog30-bins4-icell-sau"
