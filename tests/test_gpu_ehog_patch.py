"""ExtendedHogFilter as a patch filter (fd_ehog_patch_batch): the cell histograms are the oracle's SpatialHistogramFilter with 1 x 1
blocks and no normalisation (HistogramFilter::createCellHistograms), the descriptors on top of them are tests/ehog_model.py's --
bit for bit.  And once the composition GradientFilter -> GradientBinningFilter -> ExtendedHogFilter of createEHogExtractor."""
import numpy as np
import pytest

import ehog_model as model

pytestmark = pytest.mark.gpu

N = 7


def _bin_patches(oracle, synth, pw, ph, channels, bins, seed):
    """bin-image patches with `channels` bytes per pixel: LBP-like codes (1), gradient bins + weights (2), interpolated (4)"""
    rng = np.random.default_rng(seed)
    if channels == 1:
        return rng.integers(0, bins, (N, ph, pw), dtype=np.uint8)
    gray = oracle.bgr2gray(synth.make_frame(160, 120, seed=seed))
    out = []
    for k in range(N):
        x, y = int(rng.integers(0, 160 - pw)), int(rng.integers(0, 120 - ph))
        grad = oracle.gradient_filter(np.ascontiguousarray(gray[y:y + ph, x:x + pw]), 1, 0)
        out.append(oracle.gradient_binning(grad, bins, signed_gradients=True, interpolate=channels == 4))
    return np.stack(out)


def _want(oracle, patches, bins, cell, interpolate, sau, alpha):
    out = []
    for p in patches:
        ph, pw = p.shape[:2]
        rows, cols = model.cv_round(ph / cell), model.cv_round(pw / cell)
        cells = np.asarray(oracle.spatial_histogram(np.ascontiguousarray(p), bins, cell, 1, interpolate=interpolate, normalization=0), np.float32)
        hist = cells.reshape(rows, cols, bins)
        out.append(model.descriptors(hist, bins, sau, True, alpha).reshape(rows * cols, -1))
    return np.stack(out)


@pytest.mark.parametrize("sau", [False, True], ids=["single", "signed+unsigned"])
@pytest.mark.parametrize("interpolate", [False, True], ids=["plain", "interpolated"])
@pytest.mark.parametrize("channels", [1, 2, 4])
@pytest.mark.parametrize("size", [(20, 20), (21, 19)], ids=["20x20", "21x19"])
def test_patch_batch(oracle, capi, ctx, synth, size, channels, interpolate, sau):
    """21 x 19 at cell 5 is a 4 x 4 grid of uneven cells after cvRound"""
    pw, ph = size
    bins, alpha = 18, 0.2 if sau else 0.48
    patches = _bin_patches(oracle, synth, pw, ph, channels, bins, seed=pw + channels)
    ep = capi.ehog_patch_params(pw, ph, bins=bins, cell_w=5, interpolate=interpolate, signed_and_unsigned=sau, alpha=alpha)
    got = capi.ehog_patch_batch(ctx, patches, ep)
    want = _want(oracle, patches, bins, 5, interpolate, sau, alpha)
    assert got.shape == want.shape == (N, 16, bins + (bins // 2 if sau else 0) + 4)
    assert capi.ehog_feature_length(ep, channels) == 16 * got.shape[2]
    assert got.tobytes() == want.tobytes(), "%d values differ" % int((got != want).sum())
    assert got.any()


def test_composition_of_the_ehog_feature_type(oracle, capi, ctx, synth):
    """createEHogExtractor (BenchmarkRunner.cpp): GradientFilter(1) -> GradientBinningFilter(bins, signed, interpolate) ->
    ExtendedHogFilter, all three on the device, against the oracle's first two stages, its cell histograms and the model"""
    gray = oracle.bgr2gray(synth.make_frame(160, 120, seed=9))
    rng = np.random.default_rng(9)
    pw = ph = 20
    patches = np.stack([np.ascontiguousarray(gray[y:y + ph, x:x + pw]) for x, y in zip(rng.integers(0, 140, N), rng.integers(0, 100, N))])
    grad = capi.gradient_image(ctx, patches.reshape(N * ph, pw), 1).reshape(N, ph, pw, 2)
    # the gradient filter works on the stack as one image: only rows inside a patch are compared against the per-patch oracle
    bins_img = capi.gradient_binning_image(ctx, grad.reshape(N * ph, pw, 2), 18, signed_gradients=True, interpolate=True).reshape(N, ph, pw, 4)
    ep = capi.ehog_patch_params(pw, ph, bins=18, cell_w=5, interpolate=True, signed_and_unsigned=True, alpha=0.2)
    got = capi.ehog_patch_batch(ctx, bins_img, ep)
    want_bins = np.stack([oracle.gradient_binning(g, 18, signed_gradients=True, interpolate=True) for g in grad])
    assert np.array_equal(bins_img, want_bins)
    want = _want(oracle, want_bins, 18, 5, True, True, 0.2)
    assert got.tobytes() == want.tobytes()
    # inner rows of every patch carry the same gradients as the oracle's per-patch GradientFilter
    per_patch = np.stack([oracle.gradient_filter(p, 1, 0) for p in patches])
    assert np.array_equal(grad[:, 1:-1], per_patch[:, 1:-1])


def test_invalid_calls(capi, ctx):
    ok = dict(bins=18, cell_w=5)
    assert capi.ehog_feature_length(capi.ehog_patch_params(20, 20, **ok), 2) == 16 * 22
    assert capi.ehog_feature_length(capi.ehog_patch_params(20, 20, signed_and_unsigned=True, **ok), 4) == 16 * 31
    assert capi.ehog_feature_length(capi.ehog_patch_params(20, 20, bins=9, cell_w=5, cell_h=10), 2) == 2 * 4 * 13
    bad = [capi.ehog_patch_params(2, 20, **ok),                                   # cvRound(2 / 5) = 0 columns
           capi.ehog_patch_params(20, 2, **ok),                                   # 0 rows
           capi.ehog_patch_params(20, 20, bins=0, cell_w=5), capi.ehog_patch_params(20, 20, bins=18, cell_w=0),
           capi.ehog_patch_params(20, 20, bins=9, cell_w=5, signed_and_unsigned=True), capi.ehog_patch_params(20, 20, alpha=0.0, **ok)]
    for ep in bad:
        assert capi.ehog_feature_length(ep, 2) == -1
        with pytest.raises(capi.FdError) as e:
            ctx.check(capi.lib().fd_ehog_patch_batch(ctx.h, np.zeros(4096, np.uint8).ctypes.data, 1, 2, ep, np.zeros(4096, np.float32).ctypes.data))
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    assert capi.ehog_feature_length(capi.ehog_patch_params(20, 20, **ok), 3) == -1
