"""CompleteExtendedHogFilter on the device (fd_cehog_image, fd_pyramid_cehog_layer) against tests/ehog_model.py, bit for bit: every
accumulation order is the reference's, and the device's fp32 add / multiply / divide / sqrt are correctly rounded."""
import numpy as np
import pytest

import ehog_model as model

pytestmark = pytest.mark.gpu

# (bin_count, signed, unsigned, alpha)
MODES = [(9, False, True, 0.48), (18, True, False, 0.2), (18, True, True, 0.2)]
MODE_IDS = ["unsigned9", "signed18", "both18"]
INTERP = [(False, False), (False, True), (True, False), (True, True)]
INTERP_IDS = ["plain", "cells", "bins", "bins+cells"]


def _image(w, h, seed):
    """smooth structure plus noise: gradients of every direction, magnitudes from 0 to large"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(x / 3.1 + seed) * np.cos(y / 4.3) + 20 * rng.standard_normal((h, w))
    return np.clip(np.rint(base), 0, 255).astype(np.uint8)


def _params(capi, cell, mode, interp):
    bins, signed, unsigned, alpha = mode
    return capi.cehog_params(cell_size=cell, bin_count=bins, signed_gradients=signed, unsigned_gradients=unsigned, interpolate_bins=interp[0],
                             interpolate_cells=interp[1], alpha=alpha)


def _model(img, cell, mode, interp):
    bins, signed, unsigned, alpha = mode
    return model.cehog(img, cell, bins, signed, unsigned, interp[0], interp[1], alpha)


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%d of %d values differ, first at %s: %r != %r" % (len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("interp", INTERP, ids=INTERP_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cell", [4, 5])
@pytest.mark.parametrize("size", [(37, 29), (40, 30)], ids=["37x29", "40x30"])
def test_image_equals_the_model(capi, ctx, size, cell, mode, interp):
    img = _image(size[0], size[1], seed=cell * 10 + len(MODES) * INTERP.index(interp) + MODES.index(mode))
    _same(capi.cehog_image(ctx, _params(capi, cell, mode, interp), gray=img), _model(img, cell, mode, interp))


def test_gradients_clamp_at_the_covered_area(capi, ctx):
    """37 x 29 at cell 5 covers 35 x 25: the pixels beyond must not be read, so changing them changes nothing (FhogFilter would read them)"""
    img = _image(37, 29, seed=3)
    fp = _params(capi, 5, MODES[2], (False, True))
    a = capi.cehog_image(ctx, fp, gray=img)
    img2 = img.copy()
    img2[25:, :] = 255 - img2[25:, :]
    img2[:, 35:] = 255 - img2[:, 35:]
    _same(capi.cehog_image(ctx, fp, gray=img2), a)
    _same(a, capi.cehog_image(ctx, fp, gray=np.ascontiguousarray(img[:25, :35])))


@pytest.mark.parametrize("interp", INTERP, ids=INTERP_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("size", [(23, 5), (7, 6), (5, 23)], ids=["one-cell-row", "one-cell", "one-cell-column"])
def test_degenerate_grids(capi, ctx, size, mode, interp):
    """every neighbour clamp of the normalisers (and, with one cell, of the cell interpolation) coincides"""
    img = _image(size[0], size[1], seed=11)
    _same(capi.cehog_image(ctx, _params(capi, 5, mode, interp), gray=img), _model(img, 5, mode, interp))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_flat_image(capi, ctx, mode):
    """no gradient anywhere: the energies are 0, eps alone normalises, every feature is 0"""
    img = np.full((30, 40), 77, np.uint8)
    got = capi.cehog_image(ctx, _params(capi, 5, mode, (True, True)), gray=img)
    _same(got, _model(img, 5, mode, (True, True)))
    assert not got.any()


@pytest.mark.parametrize("interp", [(False, False), (True, True)], ids=["plain", "bins+cells"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_full_range_noise(capi, ctx, mode, interp):
    """gradients up to +-255 in both directions: the far corners of the look-up table, truncation at alpha on most bins"""
    rng = np.random.default_rng(99)
    img = rng.integers(0, 256, (29, 37), dtype=np.uint8)
    img[rng.random(img.shape) < 0.3] = 0
    img[rng.random(img.shape) < 0.3] = 255
    _same(capi.cehog_image(ctx, _params(capi, 4, mode, interp), gray=img), _model(img, 4, mode, interp))


def test_more_than_one_block_and_wide_descriptor(capi, ctx):
    """96 x 80 at cell 4 is 480 cells (eight 64-cell blocks); 36 signed + 18 unsigned bins is the widest descriptor (58 channels)"""
    img = _image(96, 80, seed=5)
    mode = (36, True, True, 0.2)
    got = capi.cehog_image(ctx, _params(capi, 4, mode, (True, True)), gray=img)
    assert got.shape == (20, 24, 58)
    _same(got, _model(img, 4, mode, (True, True)))


def test_image_smaller_than_a_cell(capi, ctx):
    for (w, h) in [(4, 9), (9, 4), (3, 3)]:
        with pytest.raises(capi.FdError) as e:
            capi.cehog_image(ctx, _params(capi, 5, MODES[2], (False, True)), gray=np.zeros((h, w), np.uint8))
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError) as e:   # more bins than the backend's histograms hold
        capi.cehog_image(ctx, capi.cehog_params(cell_size=5, bin_count=38), gray=np.zeros((20, 20), np.uint8))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_fhog_is_untouched_between_cehog_calls(capi, ctx):
    """the two filters share kernels and scratch but not look-up tables: FHOG before and after a CEHOG call is the same"""
    img = _image(40, 30, seed=8)
    before = capi.fhog(ctx, gray=img, cell_size=5, interpolate_bins=True)
    capi.cehog_image(ctx, _params(capi, 5, MODES[2], (True, True)), gray=img)
    _same(capi.fhog(ctx, gray=img, cell_size=5, interpolate_bins=True), before)


def test_pyramid_layer(capi, ctx, synth):
    """fd_pyramid_cehog_layer equals the filter on the downloaded gray layer (first layer: 24 x 20 cells; last: not a multiple of 4)"""
    pyr = capi.Pyramid(ctx, octave_layers=2, min_scale=0.4, max_scale=1.0)
    pyr.update(synth.make_frame(96, 80, seed=12))
    layers = pyr.layers()
    assert len(layers) >= 3
    mode, interp = MODES[2], (False, True)
    for li in (0, len(layers) - 1):
        got = capi.cehog_image(ctx, _params(capi, 4, mode, interp), pyramid=pyr, layer=li)
        _same(got, _model(pyr.layer(li), 4, mode, interp))
