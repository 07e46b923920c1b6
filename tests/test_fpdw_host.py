"""FPDW channel features, the parts that need no device: the gradient look-up table (bit for bit against tests/fpdw_model.py on all
65,536 codes), fd_fpdw_size, and the new host headers."""
import os
import subprocess

import numpy as np
import pytest

import fpdw_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("interpolate", [False, True], ids=["nearest", "interpolated"])
def test_gradient_lut_equals_the_model(capi, interpolate):
    got = capi.fpdw_gradient_lut(interpolate_bins=interpolate)
    want = model.gradient_lut(interpolate)
    for name in ("bin1", "bin2", "w1", "w2", "magnitude"):
        assert got[name].dtype == want[name].dtype and got[name].shape == (65536,)
        assert got[name].tobytes() == want[name].tobytes(), name
    assert int(got["bin1"].max()) < model.BINS and int(got["bin2"].max()) < model.BINS and int(got["bin1"].min()) >= 0
    if interpolate:
        assert np.all(got["bin1"] != got["bin2"])
    # 45 and 135 degrees lie on bin boundaries (1.5 and 4.5 bins): code (127 + d, 127 + d) and (127 - d, 127 + d)
    d = np.arange(1, 128)
    diag, anti = (127 + d) | ((127 + d) << 8), (127 - d) | ((127 + d) << 8)
    assert set(got["bin1"][diag].tolist()) <= {1, 2} and set(got["bin1"][anti].tolist()) <= {4, 5}
    # the zero gradient
    zero = 127 | (127 << 8)
    assert got["magnitude"][zero] == 0 and got["bin1"][zero] == 0


def test_size(capi):
    for (w, h, c) in [(37, 29, 4), (64, 48, 5), (131, 67, 8), (640, 480, 8), (3, 3, 4)]:
        assert capi.fpdw_size(w, h, cell_size=c) == (h // c, w // c, model.CHANNELS)
    for c in (0, -3):
        with pytest.raises(capi.FdError) as e:
            capi.fpdw_size(64, 48, cell_size=c)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_model_triangular_filters_are_normalised():
    """a constant image stays constant under the normaliser and becomes cell^2 times itself under the aggregation (alpha = cell^2)"""
    flat = np.full((23, 31), 0.37)
    assert np.allclose(model.triangular_smooth(flat, 5), 0.37, rtol=1e-14)
    for cell in (4, 5, 8):
        out = model.aggregate(np.full((29, 37, 2), 0.37), cell)
        assert out.shape == (29 // cell, 37 // cell, 2) and np.allclose(out, 0.37 * cell * cell, rtol=1e-14)
    with pytest.raises(ValueError, match="at least 6 rows"):
        model.triangular_smooth(np.zeros((5, 40)), 5)
    with pytest.raises(ValueError, match="at least 12 columns"):
        model.triangular_smooth(np.zeros((9, 11)), 5)


def test_bounds_are_below_the_reference_drift():
    """the bounds the device tests use, from the kernel's rounding count, stay below what the reference's own running sums drift by"""
    for c, r in [(4, 4), (5, 5), (8, 8), (4, 0)]:
        assert model.rtol(c, r) <= 2e-5
    assert model.rounding_count(8, 8) == 76 and model.ATOL_LUV <= 1e-5


def test_host_headers_compile():
    """the new host headers are self-contained (syntax only)"""
    inc = os.path.join(ROOT, "featuredetection_amd", "host", "include")
    for hdr in ("imageprocessing/filtering/FpdwFeaturesFilter.hpp", "imageprocessing/filtering/AggregationFilter.hpp"):
        src = '#include "%s"\nint main() { return 0; }\n' % hdr
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                       input=src.encode(), check=True)
