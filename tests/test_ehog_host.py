"""Extended HOG, the parts that need no device: the gradient look-up table (bit for bit against tests/ehog_model.py on
all 512 x 512 codes, every sign mode x bin interpolation), fd_cehog_size, fd_ehog_feature_length and fd_ehog_tracker_plan_layers against the
model including degenerate sizes, the cell-grid rule of initialize, PatchResizingFeatureExtractor on a stub, the host classes' argument
exceptions, and the header compiled as C."""
import math
import os
import subprocess

import numpy as np
import pytest

import ehog_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (bin_count, signed, unsigned): the three sign modes of the filter
MODES = [(9, False, True), (18, True, False), (18, True, True)]
MODE_IDS = ["unsigned9", "signed18", "both18"]


@pytest.mark.parametrize("interpolate", [False, True], ids=["nearest", "interpolated"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gradient_lut_equals_the_model(capi, mode, interpolate):
    bins, signed, unsigned = mode
    fp = capi.cehog_params(cell_size=5, bin_count=bins, signed_gradients=signed, unsigned_gradients=unsigned, interpolate_bins=interpolate)
    got = capi.cehog_gradient_lut(fp)
    want = model.gradient_lut(bins, signed, interpolate)
    for name, g, w in zip(("index1", "index2", "weight1", "weight2"), got, want):
        assert g.dtype == w.dtype and g.shape == (512, 512), name
        assert g.tobytes() == w.tobytes(), name
    i1, i2, w1, w2 = got
    assert 0 <= int(i1.min()) and int(i1.max()) < bins and 0 <= int(i2.min()) and int(i2.max()) < bins
    assert w1[256, 256] == 0 and w2[256, 256] == 0   # the zero gradient
    if not interpolate:
        assert np.array_equal(i1, i2) and not w2.any()
    # a gradient along +x (dx > 0, dy = 0): direction 0, which the signed table moves to pi = half the circle
    assert i1[300, 256] == (bins // 2 if signed else 0)


def test_lut_index_order(capi):
    """index dx * 512 + dy, not the transposed order FhogFilter uses: a pure y gradient sits in row 256"""
    fp = capi.cehog_params(bin_count=18, signed_gradients=True, unsigned_gradients=False)
    i1, _, w1, _ = capi.cehog_gradient_lut(fp)
    assert w1[256, 356] == np.float32(100 / 510.0) and w1[356, 256] == np.float32(100 / 510.0)
    assert i1[356, 256] == 9      # atan2(0, +) + pi = pi            -> 18 * pi / 2 pi = 9
    assert i1[256, 356] == 14     # atan2(+, 0) + pi = 3 pi / 2      -> 13.5, rounds away from zero
    assert i1[256, 156] == 5      # atan2(-, 0) + pi = pi / 2        -> 4.5, rounds away from zero


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_size(capi, mode):
    bins, signed, unsigned = mode
    for (w, h, c) in [(37, 29, 4), (40, 30, 5), (640, 480, 8), (5, 5, 5), (4, 9, 5), (9, 4, 5), (0, 0, 3)]:
        fp = capi.cehog_params(cell_size=c, bin_count=bins, signed_gradients=signed, unsigned_gradients=unsigned)
        assert capi.cehog_size(fp, w, h) == model.size(w, h, c, bins, signed, unsigned)
    assert capi.cehog_size(capi.cehog_params(cell_size=5, bin_count=bins, signed_gradients=signed, unsigned_gradients=unsigned), 4, 9)[1] == 0


@pytest.mark.parametrize("kw", [dict(cell_size=0), dict(cell_size=-2), dict(bin_count=0), dict(signed_gradients=False, unsigned_gradients=False),
                                dict(bin_count=9, signed_gradients=True, unsigned_gradients=True)],
                         ids=["cell0", "cell-2", "bins0", "no-gradients", "both-odd"])
def test_invalid_parameters(capi, kw):
    fp = capi.cehog_params(**kw)
    for call in (lambda: capi.cehog_size(fp, 64, 48), lambda: capi.cehog_gradient_lut(fp)):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        model.check_params(fp.bin_count, fp.signed_gradients, fp.unsigned_gradients, fp.cell_size)


def test_header_compiles_as_c():
    src = '#include "fd_hip.h"\nint main(void) { fd_cehog_params p; p.cell_size = 5; return p.cell_size - 5; }\n'
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=src.encode(), check=True)


def _tracker_prm(capi, cols, rows, cell, olc, min_w, max_w, bins=18, signed=True, unsigned=True):
    fp = capi.cehog_params(cell_size=cell, bin_count=bins, signed_gradients=signed, unsigned_gradients=unsigned)
    return capi.ehog_tracker_params(fp, cols, rows, olc, min_w, max_w)


@pytest.mark.parametrize("case", [(96, 80, 3, 4, 4, 2, 12, 60), (96, 80, 4, 3, 4, 2, 16, 60), (640, 480, 5, 7, 5, 5, 25, 342), (1920, 1080, 5, 7, 5, 5, 25, 771),
                                  (77, 90, 3, 4, 4, 2, 12, 60), (320, 240, 7, 5, 5, 3, 35, 320), (40, 30, 3, 4, 4, 2, 12, 60), (11, 9, 3, 4, 4, 2, 12, 60),
                                  (96, 80, 3, 4, 4, 2, 5, 60)],
                         ids=lambda c: "%dx%d-%dx%d" % c[:4])
def test_plan_layers_equals_the_model(capi, case):
    """createPyramid's integer divisions, cvRound on the layer indices and pow-derived limits, then ImagePyramid's own layer rule"""
    w, h, cols, rows, cell, olc, min_w, max_w = case
    want = model.plan_layers(w, h, cols, cell, min_w, max_w, olc)
    assert len(want) >= 2
    got = capi.ehog_tracker_plan_layers(_tracker_prm(capi, cols, rows, cell, olc, min_w, max_w), w, h)
    assert [(g["index"], g["width"], g["height"], g["rows"], g["cols"], g["scale"]) for g in got] == want
    assert all(a["index"] < b["index"] for a, b in zip(got[:-1], got[1:]))


def test_plan_layers_limits(capi):
    mn, mx = model.pyramid_limits(5, 5, 25, 342, 5)
    assert mx == 1.0 and 0 < mn < 0.1
    # (cols + 2) * minWidth / cols is an integer division: 7 * 26 / 5 = 36, not 36.4
    assert model.pyramid_limits(5, 5, 26, 342, 5)[1] == math.pow(math.pow(0.5, 1. / 5), model.cv_round(math.log(35 / 36) / math.log(math.pow(0.5, 1. / 5))))
    # one layer only: the feature pyramid needs two
    with pytest.raises(capi.FdError) as e:
        capi.ehog_tracker_plan_layers(_tracker_prm(capi, 3, 4, 4, 2, 12, 12), 96, 80)
    assert e.value.code == capi.FD_ERR_RUNTIME
    assert len(model.plan_layers(96, 80, 3, 4, 12, 12, 2)) == 1
    for bad in [(0, 4, 4, 2, 12, 60), (3, 0, 4, 2, 12, 60), (3, 4, 0, 2, 12, 60), (3, 4, 4, 0, 12, 60), (3, 4, 4, 2, 0, 60), (3, 4, 4, 2, 30, 20)]:
        with pytest.raises(capi.FdError) as e:
            capi.ehog_tracker_plan_layers(_tracker_prm(capi, *bad), 96, 80)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    for (w, h) in [(0, 80), (96, 0), (-1, -1)]:
        with pytest.raises(capi.FdError) as e:
            capi.ehog_tracker_plan_layers(_tracker_prm(capi, 3, 4, 4, 2, 12, 60), w, h)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT


def test_patch_lds_bytes(capi):
    """patch bytes + histograms + energies + inner descriptors, each rounded up to 16: about 6 KB at the tracker's defaults"""
    def want(cols, rows, cell, bins, D):
        up = lambda v: (v + 15) & ~15
        pr, pc = rows + 2, cols + 2
        return up(up(up(up(pr * pc * cell * cell) + pr * pc * bins * 4) + pr * pc * 4) + rows * cols * D * 4)
    assert capi.ehog_tracker_patch_lds_bytes(_tracker_prm(capi, 5, 7, 5, 5, 25, 300, bins=9, signed=False)) == want(5, 7, 5, 9, 13) < 6144
    assert capi.ehog_tracker_patch_lds_bytes(_tracker_prm(capi, 5, 7, 5, 5, 25, 300)) == want(5, 7, 5, 18, 31)
    assert capi.ehog_tracker_patch_lds_bytes(_tracker_prm(capi, 30, 30, 4, 2, 120, 200)) > 65536
    assert capi.ehog_tracker_patch_lds_bytes(_tracker_prm(capi, 0, 7, 5, 5, 25, 300)) == -1


HOST_PROGRAM = r'''
#include "imageprocessing/CompleteExtendedHogFilter.hpp"
#include "imageprocessing/ExtendedHogFilter.hpp"
#include "imageprocessing/PatchResizingFeatureExtractor.hpp"
#include <cstdio>
#include <functional>
#include <stdexcept>
using namespace imageprocessing;

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static bool invalid(const std::function<void()>& f) {
    try { f(); } catch (const std::invalid_argument&) { return true; } catch (...) { return false; }
    return false;
}

// records what it is asked for and answers with a patch of that position and size
struct Stub : public FeatureExtractor {
    using FeatureExtractor::update;
    mutable int x = 0, y = 0, w = 0, h = 0;
    bool none = false;
    int updates = 0;
    void update(std::shared_ptr<VersionedImage>) override { ++updates; }
    std::shared_ptr<Patch> extract(int px, int py, int pw, int ph) const override {
        x = px; y = py; w = pw; h = ph;
        if (none) return std::shared_ptr<Patch>();
        return std::make_shared<Patch>(px, py, pw, ph, cv::Mat());
    }
};

int main() {
    // CompleteExtendedHogFilter.cpp:23-26
    expect(invalid([] { CompleteExtendedHogFilter f(8, 18, false, false); }), "neither gradient kind");
    expect(invalid([] { CompleteExtendedHogFilter f(8, 9, true, true); }), "both kinds, odd bin count");
    expect(!invalid([] { CompleteExtendedHogFilter f(5, 9, false, true, false, true, 0.48f); }), "the tracker's unsigned filter");
    CompleteExtendedHogFilter both;
    expect(both.getCellSize() == 8 && both.getDescriptorSize() == 31, "defaults: cell 8, 18 + 9 + 4 channels");
    expect(CompleteExtendedHogFilter(5, 9, false, true).getDescriptorSize() == 13, "unsigned only: 9 + 4 channels");
    expect(invalid([&] { cv::Mat bgr(10, 10, CV_8UC3); both.applyTo(bgr); }), "CV_8UC1 only");
    // ExtendedHogFilter.cpp:24-31,42-51
    expect(invalid([] { ExtendedHogFilter f(0, 5, false, false); }), "binCount 0");
    expect(invalid([] { ExtendedHogFilter f(9, 0, false, false); }), "cellSize 0");
    expect(invalid([] { ExtendedHogFilter f(9, 5, 0, false, false); }), "cellHeight 0");
    expect(invalid([] { ExtendedHogFilter f(9, 5, false, true); }), "signedAndUnsigned with an odd bin count");
    expect(invalid([] { ExtendedHogFilter f(9, 5, false, false, 0.f); }), "alpha 0");
    ExtendedHogFilter e(18, 5, 6, true, true);
    expect(e.getCellWidth() == 5 && e.getCellHeight() == 6, "cell width and height");
    expect(invalid([&] { cv::Mat f32(10, 10, CV_32FC1); e.applyTo(f32); }), "CV_8U bin images only");
    // PatchResizingFeatureExtractor.hpp:41-52: cvRound (half to even) on every step
    auto stub = std::make_shared<Stub>();
    PatchResizingFeatureExtractor r(stub, 1.5, 0.25, -0.1);
    std::shared_ptr<Patch> p = r.extract(100, 80, 21, 31);
    expect(stub->x == 98 && stub->y == 88 && stub->w == 32 && stub->h == 46, "request: cvRound(100 - 2.1), cvRound(80 + 7.75), cvRound(31.5), cvRound(46.5)");
    expect(p && p->getWidth() == 21 && p->getHeight() == 31, "patch size: cvRound(32 / 1.5), cvRound(46 / 1.5)");
    expect(p && p->getX() == 100 && p->getY() == 80, "patch position: cvRound(98 + 2.1), cvRound(88 - 7.75)");
    PatchResizingFeatureExtractor half(stub, 0.5);
    p = half.extract(10, 10, 5, 7);
    expect(stub->w == 2 && stub->h == 4, "cvRound(2.5) = 2, cvRound(3.5) = 4");
    expect(p && p->getWidth() == 4 && p->getHeight() == 8 && p->getX() == 10 && p->getY() == 10, "half-size patch reported at twice its size");
    stub->none = true;
    expect(!r.extract(100, 80, 21, 31), "no patch stays no patch");
    r.update(cv::Mat(4, 4, CV_8UC1));
    expect(stub->updates == 1, "update is forwarded");
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
'''


def test_host_classes(tmp_path):
    """argument exceptions of the two filters and PatchResizingFeatureExtractor's arithmetic on a stub extractor: no device involved"""
    src = tmp_path / "ehog_host.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "ehog_host"
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr



GRID_PROGRAM = r'''
#include "condensation/ExtendedHogBasedMeasurementModel.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    for (int i = 1; i + 2 < argc; i += 3) {
        size_t cols = 0, rows = 0;
        condensation::ExtendedHogBasedMeasurementModel::computeCellGrid(std::atoi(argv[i]), std::atoi(argv[i + 1]), (size_t)std::atoi(argv[i + 2]), cols, rows);
        std::printf("%zu %zu\n", cols, rows);
    }
    // the model refuses classifiers whose kernel is not linear (ExtendedHogBasedMeasurementModel.cpp:74-75)
    try {
        condensation::ExtendedHogBasedMeasurementModel m(std::make_shared<classification::ProbabilisticSvmClassifier>(std::make_shared<classification::RbfKernel>(0.5)));
        std::printf("accepted\n");
    } catch (const std::invalid_argument&) { std::printf("refused\n"); }
    condensation::ExtendedHogBasedMeasurementModel ok(std::make_shared<classification::ProbabilisticSvmClassifier>(std::make_shared<classification::LinearKernel>()));
    std::printf("%d %d\n", ok.isUsable() ? 1 : 0, ok.getFusedEvaluationCount());
    condensation::Sample::setAspectRatio(5, 7);
    std::printf("%d\n", condensation::Sample(10, 10, 30).getHeight());
    return 0;
}
'''

GRID_CASES = [(30, 42, 35), (42, 30, 35), (50, 50, 35), (20, 60, 35), (60, 20, 35), (31, 47, 35), (100, 130, 48), (64, 48, 12), (10, 100, 35), (33, 33, 1),
              (25, 35, 2), (7, 9, 35)]


def test_cell_grid_rule_of_initialize(tmp_path):
    """ExtendedHogBasedMeasurementModel::computeCellGrid (the rule of initialize, :221-228) against the model; no device involved"""
    src = tmp_path / "grid.cpp"
    src.write_text(GRID_PROGRAM)
    exe = tmp_path / "grid"
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe)] + [str(v) for c in GRID_CASES for v in c], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    got = [tuple(int(v) for v in l.split()) for l in lines[:len(GRID_CASES)]]
    assert got == [model.cell_grid(*c) for c in GRID_CASES]
    assert got[0] == (5, 7) and got[1] == (7, 5) and got[2] == (6, 6)
    assert lines[len(GRID_CASES):len(GRID_CASES) + 3] == ["refused", "0 0", "42"]
    assert model.max_width(160, 120, 30, 42) == 85 and model.max_width(160, 120, 42, 30) == 160


@pytest.mark.parametrize("sau", [False, True])
def test_ehog_feature_length_equals_the_model(capi, sau):
    for (pw, ph) in [(20, 20), (21, 19), (5, 5), (2, 20), (20, 2), (3, 3), (2, 2), (64, 64), (12, 13), (0, 10), (10, 0), (-4, 8)]:
        for (bins, cw, ch) in [(18, 5, 0), (9, 5, 0), (18, 5, 10), (18, 4, 6), (0, 5, 0), (18, 0, 0), (8, 7, 3)]:
            for channels in (1, 2, 3, 4):
                ep = capi.ehog_patch_params(pw, ph, bins=bins, cell_w=cw, cell_h=ch, signed_and_unsigned=sau, alpha=0.2)
                assert capi.ehog_feature_length(ep, channels) == model.ehog_feature_length(pw, ph, bins, cw, ch, sau, 0.2, channels), (pw, ph, bins, cw, ch, channels)
    assert capi.ehog_feature_length(capi.ehog_patch_params(20, 20, bins=18, cell_w=5, alpha=0.0), 2) == -1
    assert model.ehog_feature_length(2, 20, 18, 5, 0, False) == -1 and model.ehog_feature_length(21, 19, 18, 5, 0, True) == 16 * 31
