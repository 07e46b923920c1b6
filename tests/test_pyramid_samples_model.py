"""Sampled pyramid features, the parts that need no device: the new symbols, the sample -> window rule of fd_sample_windows against
tests/pyramid_samples_model.py, the limits and the argument rules that are decided without a context, the integer magnitude rule
of imageprocessing::GradientMagnitudeFilter, and the model's MT19937."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pyramid_samples_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = 2.0 ** (-1.0 / 3.0)
NEW_SYMBOLS = ("fd_sample_windows", "fd_pyramid_sample_windows", "fd_hist_samples_limits", "fd_hist_extract_samples", "fd_ehog_extract_samples",
               "fd_hist_svm_evaluate_samples", "fd_hist_svm_evaluate_samples_distance", "fd_gradient_magnitude_image")


def six_layers():
    """scales 0.7937^k of a 120 x 96 image and the layer sizes those scales give"""
    return [dict(index=k, scale=0.7937 ** k, w=model.cv_round(120 * 0.7937 ** k), h=model.cv_round(96 * 0.7937 ** k)) for k in range(6)]


def test_symbols_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi._SIGS and getattr(lib, name).argtypes is not None, name
    assert re.search(r"FD_LAYER_GRADMAG_LBP = 3\b", header) and capi.FD_LAYER_GRADMAG_LBP == 3
    assert re.search(r"FD_HIST_SAMPLES_MAX = 1 << 20\b", header) and capi.FD_HIST_SAMPLES_MAX == 1 << 20
    assert (capi.FD_SAMPLES_HIST, capi.FD_SAMPLES_EHOG) == (0, 1)
    for name in ("sample_windows", "hist_extract_samples", "ehog_extract_samples", "hist_svm_evaluate_samples", "gradient_magnitude_image"):
        assert callable(getattr(capi, name)), name
    assert callable(capi.Pyramid.sample_windows)


def test_header_compiles_as_c99():
    src = '#include "fd_hip.h"\nint main(void) { return FD_LAYER_GRADMAG_LBP + FD_SAMPLES_EHOG + (FD_HIST_SAMPLES_MAX > 0); }\n'
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=src.encode(), check=True)


@pytest.mark.parametrize("pw,ph", [(16, 16), (12, 20)])
def test_sample_windows_equal_the_model(capi, pw, ph):
    layers = six_layers()
    s = model.make_samples(layers, INC, pw, ph)
    want = model.sample_windows(layers, INC, pw, ph, s)
    # the categories, on the model alone
    assert 50 <= len(s) <= 90
    ok = want[:, 3] == 1
    assert 2 * ok.sum() >= len(s)
    assert set(want[ok, 0].tolist()) == set(range(6))                      # every layer hit
    lw = np.array([layers[l]["w"] for l in want[ok, 0]])
    lh = np.array([layers[l]["h"] for l in want[ok, 0]])
    assert (want[ok, 1] == 0).any() and (want[ok, 2] == 0).any()           # flush with each border
    assert (want[ok, 1] + pw == lw).any() and (want[ok, 2] + ph == lh).any()

    def raw(v):   # the window the rule computes before its bounds check
        x, y, width, height = v
        L = layers[model.lround(np.log(pw / width) / np.log(INC))]
        return model.cv_round((x - model.c_div2(width)) * L["scale"]), model.cv_round((y - model.c_div2(height)) * L["scale"]), L
    past = {"left": False, "top": False, "right": False, "bottom": False}
    for v, w in zip(s.tolist(), want.tolist()):
        if w[3] or v[2] <= 0:
            continue
        idx = model.lround(np.log(pw / v[2]) / np.log(INC))
        if not 0 <= idx < 6:
            continue
        bx, by, L = raw(v)
        past["left"] |= bx == -1
        past["top"] |= by == -1
        past["right"] |= bx + pw == L["w"] + 1
        past["bottom"] |= by + ph == L["h"] + 1
    assert all(past.values()), past                                        # one pixel past each border
    assert (s[:, 2] <= 0).sum() >= 2 and not want[s[:, 2] <= 0, 3].any()   # width <= 0
    idx = np.array([model.lround(np.log(pw / v) / np.log(INC)) if v > 0 else 0 for v in s[:, 2].tolist()])
    assert (idx < 0).any() and (idx > 5).any()                             # before the first and behind the last kept layer
    assert (s[ok, 2] % 2 == 1).any() and (s[ok, 2] % 2 == 0).any() and (s[:, 3] % 2 == 1).any()
    assert (s[:, 0] - s[:, 2] // 2 < 0).any()                              # negative x - width / 2
    assert len({tuple(v) for v in s.tolist()}) < len(s)                    # identical samples
    got = capi.sample_windows(layers, INC, pw, ph, s)
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_rounding_rules_of_the_model():
    assert [model.lround(v) for v in (0.5, 1.5, -0.5, -1.5, 2.4, -2.6)] == [1, 2, -1, -2, 2, -3]
    assert [model.cv_round(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 2.6)] == [0, 2, 2, 0, -2, 3]
    assert [model.c_div2(v) for v in (7, -7, 8, -8, 1, -1)] == [3, -3, 4, -4, 0, 0]


def test_limits_and_argument_rules_without_a_device(capi):
    lib = capi.lib()
    bad = capi.FD_ERR_INVALID_ARGUMENT
    n = C.c_int()
    assert lib.fd_hist_samples_limits(C.byref(n)) == capi.FD_OK and n.value == 1 << 20 == capi.hist_samples_limits()
    assert lib.fd_hist_samples_limits(None) == bad
    layers = six_layers()
    s = np.array([[60, 48, 16, 16]], np.int32)
    assert capi.sample_windows(layers, INC, 16, 16, s)[0, 3] == 1
    assert len(capi.sample_windows(layers, INC, 16, 16, np.zeros((0, 4), np.int32))) == 0
    assert not capi.sample_windows([], INC, 16, 16, s)[0, 3]               # no kept layer: no window
    for kw in (dict(inc=1.0), dict(inc=0.0), dict(inc=float("nan")), dict(pw=0), dict(ph=0)):
        a = dict(inc=INC, pw=16, ph=16)
        a.update(kw)
        with pytest.raises(capi.FdError):
            capi.sample_windows(layers, a["inc"], a["pw"], a["ph"], s)
    gap = [dict(l) for l in layers]
    gap[3]["index"] = 7                                                    # the kept layers have consecutive indices
    with pytest.raises(capi.FdError):
        capi.sample_windows(gap, INC, 16, 16, s)
    out = np.zeros(4, np.int32)
    assert lib.fd_sample_windows(0, None, None, None, None, INC, 16, 16, 1, None, out.ctypes.data_as(C.c_void_p)) == bad
    assert lib.fd_sample_windows(0, None, None, None, None, INC, 16, 16, -1, None, None) == bad
    # NULL handles and contexts: FD_ERR_INVALID_ARGUMENT, nothing is dereferenced
    assert lib.fd_pyramid_sample_windows(None, 16, 16, 0, None, None) == bad
    assert lib.fd_hist_extract_samples(None, None, None, 0, None, None, None) == bad
    assert lib.fd_ehog_extract_samples(None, None, None, 0, None, None, None) == bad
    assert lib.fd_hist_svm_evaluate_samples(None, None, 0, None, None, 0, None, None, None) == bad
    assert lib.fd_hist_svm_evaluate_samples_distance(None, None, 0, None, None, 0, None, None, None, None) == bad
    one = np.zeros(4, np.uint8)
    assert lib.fd_gradient_magnitude_image(None, one.ctypes.data_as(C.c_void_p), 1, 1, one.ctypes.data_as(C.c_void_p)) == bad
    with pytest.raises(capi.FdError):
        capi.gradient_magnitude_image(None, np.zeros((3, 3), np.uint8))   # not a two-channel image


def test_extreme_samples_have_no_window(capi):
    """coordinates and widths at the ends of int32 neither overflow nor find a window"""
    layers = six_layers()
    big = 2 ** 31 - 1
    s = np.array([[big, big, 16, 16], [-big - 1, -big - 1, 16, 16], [60, 48, big, big], [60, 48, 1, 1], [big, 0, 21, -big - 1]], np.int32)
    assert not capi.sample_windows(layers, INC, 16, 16, s)[:, 3].any()
    assert not model.sample_windows(layers, INC, 16, 16, s)[:, 3].any()


def test_magnitude_rule_over_all_codes():
    """the integer rule equals the rounded float64 square root for all 65536 (gx, gy) codes, because no tie exists"""
    s = np.arange(2 * 128 * 128 + 1, dtype=np.int64)
    r = model.magnitude_table()
    assert (r * r - r < s)[1:].all() and (s <= r * r + r).all() and r[0] == 0 and r.max() == 181
    # a tie would need s = (k + 1/2)^2 = k^2 + k + 1/4: never an integer
    k = np.arange(0, 200, dtype=np.int64)
    assert not np.isin(4 * s, (2 * k + 1) ** 2).any()
    gx, gy = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    grad = np.stack([gx, gy], axis=-1).astype(np.uint8)
    want = np.rint(np.sqrt(((gx - 127.0) ** 2 + (gy - 127.0) ** 2).astype(np.float64)))
    got = model.gradient_magnitude(grad)
    assert got.dtype == np.uint8 and np.array_equal(got, np.minimum(want, 255).astype(np.uint8))
    assert got[127, 127] == 0 and got[255, 255] == 181 and got[0, 0] == 180 and got[127, 255] == 128


def test_mt19937_against_the_standard():
    """the first outputs of seed 5489 and the 10000th (the value the C++ standard names for mt19937)"""
    g = model.MT19937(5489)
    first = [g.next() for _ in range(5)]
    assert first == [3499211612, 581869302, 3890346734, 3586334585, 545404204]
    for _ in range(10000 - 6):
        g.next()
    assert g.next() == 4123659995
    g = model.MT19937(5489)
    assert g.below(10) == (3499211612 * 10) >> 32 and g.below(1) == 0
    assert all(0 <= model.MT19937(s).below(7) < 7 for s in range(20))
    with pytest.raises(ValueError):
        g.below(0)


def test_selection_model_counts():
    """adapt's selection: 1 or 5 positives, 6 / 18 / 26 negatives around the target, the frame counter"""
    for around, count in ((0, 0), (1, 6), (2, 18), (3, 26)):
        sel = model.Selection(negatives_around_target=around, additional_negatives=0, test_negatives=3, start_frame_count=2)
        every = lambda x, y, w, h: True
        assert sel.adapt(96, 80, [], (48, 40, 20), every, None) is None and sel.frame_count == 1
        pos, neg, test = sel.adapt(96, 80, [], (48, 40, 20), every, None)
        assert len(pos) == 5 and len(neg) == count and len(test) == 3
        assert pos[1] == (47, 40, 20) and all(s[2] in (20, 10, 40) for s in neg)
    sel = model.Selection(positive_offset_factor=0, additional_negatives=4, test_negatives=0, start_frame_count=1)
    parts = [(10, 10, 20, 0.3), (12, 70, 20, 0.9), (48, 40, 20, 1.0), (80, 10, 8, 0.1), (85, 70, 20, 0.5), (5, 40, 20, 0.7)]
    pos, neg, test = sel.adapt(96, 80, parts, (48, 40, 20), lambda x, y, w, h: True, None)
    assert pos == [(48, 40, 20)] and test == []
    assert neg == [(10, 10, 20), (85, 70, 20), (5, 40, 20), (12, 70, 20)]   # the four heaviest outside the bounds, ascending weight
