"""Integral-image features, the parts that need no device: HaarFeatureFilter's feature table and grid (bit for bit against
tests/integral_model.py), the model's integral image, and the argument errors that are reported before anything touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import integral_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAAR_CASES = {
    "default": dict(sizes=(0.2, 0.4), grid=(5, 5), types=15),
    "edge-at-one": dict(sizes=(0.5, 1.0), xs=(0.5,), types=15),
    "grid3x7-types-2-8": dict(sizes=(0.2, 0.4), grid=(3, 7), types=2 | 8),
    "type1": dict(sizes=(0.3,), grid=(4, 4), types=1),
    "type2": dict(sizes=(0.25,), grid=(4, 4), types=2),
    "type4": dict(sizes=(0.35,), grid=(4, 4), types=4),
    "type8": dict(sizes=(0.45,), grid=(4, 4), types=8),
}


def model_features(case):
    if "xs" in case:
        xs = ys = np.array(case["xs"], np.float32)
    else:
        xs, ys = model.haar_grid(case["grid"][0]), model.haar_grid(case["grid"][1])
    return model.haar_features(case["sizes"], xs, ys, case["types"])


def capi_params(capi, case):
    if "xs" in case:
        return capi.haar_params(sizes=case["sizes"], xs=case["xs"], types=case["types"])
    return capi.haar_params(sizes=case["sizes"], grid=case["grid"], types=case["types"])


@pytest.mark.parametrize("name", sorted(HAAR_CASES))
def test_haar_features_equal_the_model(capi, name):
    case = HAAR_CASES[name]
    got = capi.haar_features(capi_params(capi, case))
    rects, weights, counts, factor, area = model.haar_table(model_features(case))
    assert len(got) == len(counts) == capi.haar_feature_count(capi_params(capi, case)) and len(got) > 0
    assert np.array_equal(got["num_rects"], counts)
    for field, want in (("rects", rects), ("weights", weights), ("factor", factor), ("area", area)):
        assert got[field].dtype == np.float32 and got[field].tobytes() == want.tobytes(), field


def test_default_feature_table_counts(capi):
    """34 base positions (25 at size 0.2, 9 at size 0.4: x = 1/6 and x = 5/6 fall out), six features each with all types"""
    feats = model_features(HAAR_CASES["default"])
    assert len(feats) == 204
    for types, per in ((1, 2), (2, 2), (4, 1), (8, 1)):
        assert len(model_features(dict(HAAR_CASES["default"], types=types))) == 34 * per
    assert len(model.haar_features((0.2,), types=8)) == 25 and len(model.haar_features((0.4,), types=8)) == 9
    edges = [float(v) for rects, _, _, _ in feats for (x, y, w, h) in rects for v in (x + w, y + h)]
    assert abs(max(edges) - 0.9333) < 1e-4
    got = capi.haar_features(capi.haar_params())
    assert len(got) == 204 and set(got["num_rects"].tolist()) == {2, 3, 4}
    # the edge-at-one table has a rectangle edge of exactly 1.0
    rects = capi.haar_features(capi_params(capi, HAAR_CASES["edge-at-one"]))["rects"]
    assert float((rects[:, :, 0] + rects[:, :, 2]).max()) == 1.0 and float((rects[:, :, 1] + rects[:, :, 3]).max()) == 1.0


def test_haar_grid(capi):
    for count in range(1, 9):
        got = capi.haar_grid(count)
        assert got.dtype == np.float32 and got.tobytes() == model.haar_grid(count).tobytes()
    assert len(capi.haar_grid(0)) == 0
    with pytest.raises(capi.FdError):
        capi.haar_grid(-1)


def test_invalid_haar_parameters(capi):
    lib = capi.lib()
    assert lib.fd_haar_feature_count(None) == -1
    assert lib.fd_haar_feature_count(C.byref(capi.haar_params(types=16).c)) == -1
    assert lib.fd_haar_feature_count(C.byref(capi.haar_params(types=-1).c)) == -1
    assert lib.fd_haar_feature_count(C.byref(capi.haar_params(sizes=(1.5,), xs=(0.5,)).c)) == 0   # every position falls out
    assert lib.fd_haar_feature_count(C.byref(capi.haar_params(sizes=(float("nan"),)).c)) == -1
    hp = capi.haar_params()
    cnt = C.c_int()
    out = np.zeros(10, capi.HAAR_FEATURE_DTYPE)
    assert lib.fd_haar_features(C.byref(hp.c), out.ctypes.data_as(C.c_void_p), 10, C.byref(cnt)) == capi.FD_ERR_CAPACITY and cnt.value == 204
    assert lib.fd_haar_features(None, None, 0, C.byref(cnt)) == capi.FD_ERR_INVALID_ARGUMENT
    assert lib.fd_haar_features(C.byref(hp.c), None, 0, None) == capi.FD_ERR_INVALID_ARGUMENT


def test_model_integral_image():
    rng = np.random.default_rng(3)
    for h, w in [(1, 1), (1, 9), (9, 1), (23, 31)]:
        g = rng.integers(0, 256, (h, w)).astype(np.uint8)
        I = model.integral(g)
        pad = np.zeros((h + 1, w + 1), np.int64)
        pad[1:, 1:] = np.cumsum(np.cumsum(g.astype(np.int64), axis=0), axis=1)
        assert I.dtype == np.int32 and np.array_equal(I, pad) and np.array_equal(model.integral_fast(g), pad)
    full = model.integral_fast(np.full((40, 50), 255, np.uint8))
    assert full[-1, -1] == 255 * 40 * 50 and not full[0].any() and not full[:, 0].any()


def test_model_sample_rules():
    """the window rule of DirectImageFeatureExtractor::extract and the generator's coverage"""
    s = model.make_samples(160, 120)
    assert 550 <= len(s) <= 700
    geo = [model.patch_origin(v, 161, 121) for v in s]
    exists = np.array([g[2] for g in geo])
    assert exists.sum() > 500 and (~exists).sum() >= 30
    ok = s[exists]
    x0 = np.array([g[0] for g in geo])[exists]
    y0 = np.array([g[1] for g in geo])[exists]
    assert (x0 == 0).any() and (y0 == 0).any() and (x0 + ok[:, 2] == 161).any() and (y0 + ok[:, 3] == 121).any()
    assert ok[:, 2].min() == 3 and ok[:, 2].max() == 161 and (ok[:, 2] % 2 == 1).any() and (ok[:, 2] != ok[:, 3]).any()
    assert len({tuple(v) for v in s.tolist()}) < len(s)   # duplicates
    assert model.patch_origin((5, 5, -3, 4), 161, 121)[2] is False


def test_null_arguments_without_a_device(capi):
    """NULL handles and contexts are FD_ERR_INVALID_ARGUMENT, and nothing is dereferenced"""
    lib = capi.lib()
    bad = capi.FD_ERR_INVALID_ARGUMENT
    h = C.c_void_p()
    assert lib.fd_integral_create(None, C.byref(h)) == bad and not h
    assert lib.fd_integral_update(None, None, 10, 10, 1, 0) == bad
    assert lib.fd_integral_download(None, None) == bad
    w, hh = C.c_int(), C.c_int()
    assert lib.fd_integral_size(None, C.byref(w), C.byref(hh)) == bad
    one = np.zeros(4, np.uint8)
    assert lib.fd_integral_image(None, one.ctypes.data_as(C.c_void_p), 2, 2, one.ctypes.data_as(C.c_void_p)) == bad
    assert lib.fd_integral_gradient_patches(None, None, 4, 4, 0, None, None, None) == bad
    assert lib.fd_gradient_sum_batch(None, None, 0, 12, 12, 4, 4, None) == bad
    assert lib.fd_integral_extract_surf(None, None, 12, 4, 0, None, None, None) == bad
    assert lib.fd_integral_extract_haar(None, None, None, 0, None, None, None) == bad
    assert lib.fd_integral_svm_evaluate_samples(None, None, 0, None, None, 0, None, None, None) == bad
    lib.fd_integral_destroy(None)


def test_argument_rules_without_a_device(capi):
    """rows < 2, cell divisibility, the overflow bound and the LDS bound of the fused SURF kernel, through the host-only functions
    that the device entry points themselves decide by (a NULL context would hide which rule answered)"""
    lib = capi.lib()
    # the overflow bound: 255 * width * height > 2^31 - 1
    assert 255 * 2896 * 2896 <= 2 ** 31 - 1 < 255 * 2897 * 2907
    for w, h in [(1, 1), (160, 120), (1920, 1080), (2896, 2896), (2907, 2896), (8421504, 1), (1, 8421504), (2904, 2899)]:
        assert 255 * w * h <= 2 ** 31 - 1
        assert lib.fd_integral_image_length(w, h) == (w + 1) * (h + 1), (w, h)
    for w, h in [(4000, 3000), (2897, 2907), (2907, 2897), (8421505, 1), (1, 8421505), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1), (65536, 65536)]:
        assert 255 * w * h > 2 ** 31 - 1
        assert lib.fd_integral_image_length(w, h) == -1, (w, h)
    for w, h in [(0, 5), (5, 0), (-1, 5), (-(2 ** 31), -(2 ** 31))]:
        assert lib.fd_integral_image_length(w, h) == -1
    # IntegralGradientFilter: rows, cols >= 2
    assert lib.fd_integral_gradient_length(2, 2) == 8 and lib.fd_integral_gradient_length(8, 12) == 192
    assert lib.fd_integral_gradient_length(16384, 16384) == 2 ** 29
    for rows, cols in [(1, 4), (4, 1), (0, 0), (-3, 4), (16385, 2), (2, 2 ** 31 - 1)]:
        assert lib.fd_integral_gradient_length(rows, cols) == -1, (rows, cols)
    # GradientSumFilter: the two divisibility errors
    assert lib.fd_gradient_sum_length(12, 12, 4, 4) == 64 and lib.fd_gradient_sum_length(8, 12, 2, 3) == 24
    assert lib.fd_gradient_sum_length(12, 12, 12, 12) == 576 and lib.fd_gradient_sum_length(16384, 16384, 16384, 16384) == 2 ** 30
    for args in [(12, 12, 5, 4), (12, 12, 4, 5), (12, 12, 0, 4), (12, 12, 4, 0), (0, 12, 1, 1), (12, 12, -4, 4), (32768, 2, 2, 2), (12, 12, 24, 12)]:
        assert lib.fd_gradient_sum_length(*args) == -1, args
    with pytest.raises(ValueError, match="not divisible"):
        model.gradient_sums(np.zeros((1, 12, 12, 2), np.uint8), 5, 4)
    # the fused SURF kernel: 2 <= G <= 64, G % C == 0, and four wavefronts of [2 G G bytes padded to 16 | 16 C C bytes] in 160 KB of LDS
    def fits(g, c):
        return 4 * ((2 * g * g + 15) // 16 * 16 + 16 * c * c) <= 160 * 1024
    for g in range(-1, 70):
        for c in range(-1, 70):
            ok = 2 <= g <= 64 and c >= 1 and g % c == 0 and fits(g, c)
            assert lib.fd_surf_feature_length(g, c) == (4 * c * c if ok else -1), (g, c)
    assert capi.surf_feature_length(12, 4) == 64 and capi.surf_feature_length(64, 32) == 4096 and capi.surf_feature_length(47, 47) == 8836
    for g, c in [(48, 48), (56, 56), (64, 64), (12, 5), (1, 1), (65, 5)]:
        with pytest.raises(capi.FdError):
            capi.surf_feature_length(g, c)


def test_host_headers_compile():
    """the new host headers are self-contained (syntax only)"""
    inc = os.path.join(ROOT, "featuredetection_amd", "host", "include")
    for hdr in ("imageprocessing/IntegralImageFilter.hpp", "imageprocessing/HaarFeatureFilter.hpp", "imageprocessing/IntegralGradientFilter.hpp",
                "imageprocessing/GradientSumFilter.hpp", "imageprocessing/DirectImageFeatureExtractor.hpp", "condensation/SingleClassifierModel.hpp"):
        src = '#include "%s"\nint main() { return 0; }\n' % hdr
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", inc, "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                       input=src.encode(), check=True)
