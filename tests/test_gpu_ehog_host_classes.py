"""The host classes imageprocessing::CompleteExtendedHogFilter and ExtendedHogFilter (applyTo on one Mat) against the C ABI calls they
wrap: a small program built on the host layer reads raw images and writes the descriptors."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "imageprocessing/CompleteExtendedHogFilter.hpp"
#include "imageprocessing/ExtendedHogFilter.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace imageprocessing;

static cv::Mat readImage(const char* path, int rows, int cols, int type) {
    cv::Mat m(rows, cols, type);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(m.data, 1, (size_t)rows * cols * m.channels(), f) != (size_t)rows * cols * m.channels()) std::exit(2);
    std::fclose(f);
    return m;
}
static void writeFloats(const char* path, const cv::Mat& m) {
    FILE* f = std::fopen(path, "wb");
    for (int r = 0; r < m.rows; ++r) std::fwrite(m.ptr<float>(r), sizeof(float), (size_t)m.cols, f);
    std::fclose(f);
    std::printf("%d %d\n", m.rows, m.cols);
}

int main(int argc, char** argv) {
    // gray 37 x 29 -> the tracker's unsigned filter and the default one
    cv::Mat gray = readImage(argv[1], 29, 37, CV_8UC1);
    writeFloats(argv[3], CompleteExtendedHogFilter(5, 9, false, true, false, true, 0.48f).applyTo(gray));
    writeFloats(argv[4], CompleteExtendedHogFilter(4, 18, true, true, true, true, 0.2f).applyTo(gray));
    // interpolated gradient bin image 21 x 19 (CV_8UC4) -> ExtendedHogFilter
    cv::Mat bins = readImage(argv[2], 19, 21, CV_8UC4);
    writeFloats(argv[5], ExtendedHogFilter(18, 5, true, true, 0.2f).applyTo(bins));
    return 0;
}
'''


def test_filters_per_mat(capi, ctx, oracle, synth, tmp_path):
    gray = np.ascontiguousarray(oracle.bgr2gray(synth.make_frame(160, 120, seed=4))[40:69, 50:87])
    assert gray.shape == (29, 37)
    patch = np.ascontiguousarray(oracle.bgr2gray(synth.make_frame(160, 120, seed=4))[10:29, 5:26])
    bins = oracle.gradient_binning(oracle.gradient_filter(patch, 1, 0), 18, signed_gradients=True, interpolate=True)
    assert bins.shape == (19, 21, 4)
    gray.tofile(tmp_path / "gray.bin")
    bins.tofile(tmp_path / "bins.bin")
    src = tmp_path / "prog.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "prog"
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    outs = [str(tmp_path / n) for n in ("a.f32", "b.f32", "c.f32")]
    run = subprocess.run([str(exe), str(tmp_path / "gray.bin"), str(tmp_path / "bins.bin")] + outs, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split() == ["5", str(7 * 13), "7", str(9 * 31), "4", str(4 * 31)]
    a = capi.cehog_image(ctx, capi.cehog_params(5, 9, False, True, False, True, 0.48), gray=gray)
    b = capi.cehog_image(ctx, capi.cehog_params(4, 18, True, True, True, True, 0.2), gray=gray)
    c = capi.ehog_patch_batch(ctx, bins[None], capi.ehog_patch_params(21, 19, bins=18, cell_w=5, interpolate=True, signed_and_unsigned=True, alpha=0.2))
    for path, want in zip(outs, (a, b, c)):
        got = np.fromfile(path, np.float32)
        assert got.size == want.size and got.tobytes() == want.tobytes(), path
        assert got.any()


EXTRACTOR_PROGRAM = r'''
#include "imageprocessing/CellBasedPyramidFeatureExtractor.hpp"
#include "imageprocessing/ExtendedHogFeatureExtractor.hpp"
#include <cstdio>
#include <cstdlib>
using namespace imageprocessing;

int main(int argc, char** argv) {
    cv::Mat gray(80, 96, CV_8UC1);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(gray.data, 1, 96 * 80, f) != 96 * 80) return 2;
    std::fclose(f);
    auto filter = std::make_shared<CompleteExtendedHogFilter>(4, 18, true, true, false, true, 0.2f);
    auto patches = std::make_shared<ExtendedHogFeatureExtractor>(filter, 3, 4, 12, 60, 2);
    CellBasedPyramidFeatureExtractor cells(patches);
    cells.update(gray);   // forwards to the shared handle
    FILE* out = std::fopen(argv[2], "wb");
    for (int i = 3; i + 3 < argc; i += 4) {
        const int x = std::atoi(argv[i]), y = std::atoi(argv[i + 1]), w = std::atoi(argv[i + 2]), h = std::atoi(argv[i + 3]);
        std::shared_ptr<Patch> p[2] = {patches->extract(x, y, w, h), cells.extract(x, y, w, h)};
        for (int k = 0; k < 2; ++k) {
            if (!p[k]) { std::printf("none\n"); continue; }
            std::printf("%d %d %d %d %d %d\n", p[k]->getX(), p[k]->getY(), p[k]->getWidth(), p[k]->getHeight(), p[k]->getData().rows, p[k]->getData().cols);
            for (int r = 0; r < p[k]->getData().rows; ++r) std::fwrite(p[k]->getData().ptr<float>(r), sizeof(float), (size_t)p[k]->getData().cols, out);
        }
    }
    std::fclose(out);
    bool refused = false;
    try { ExtendedHogFeatureExtractor bad(filter, 0, 4, 12, 60, 2); } catch (const std::invalid_argument&) { refused = true; }
    std::printf("%s\n", refused ? "refused" : "accepted");
    return 0;
}
'''


def test_extractors(capi, ctx, oracle, synth, tmp_path):
    """ExtendedHogFeatureExtractor::extract and CellBasedPyramidFeatureExtractor::extract on one shared handle: the data equal
    fd_ehog_tracker_extract_patches / _extract_cells, the patch geometry is the reference's (ExtendedHogFeatureExtractor.cpp:125-129,
    DirectPyramidFeatureExtractor.cpp:137-142 with CellBasedPyramidFeatureExtractor's getOriginal)"""
    import ehog_model as model
    gray = np.ascontiguousarray(oracle.bgr2gray(synth.make_frame(96, 80, seed=31)))
    gray.tofile(tmp_path / "gray.bin")
    samples = [(40, 40, 12, 16), (47, 39, 25, 33), (8, 10, 12, 16), (2, 40, 12, 16), (40, 40, 400, 400), (60, 50, 37, 49)]
    src = tmp_path / "prog.cpp"
    src.write_text(EXTRACTOR_PROGRAM)
    exe = tmp_path / "prog"
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe), str(tmp_path / "gray.bin"), str(tmp_path / "out.f32")] + [str(v) for s in samples for v in s],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "refused" and len(lines) == 2 * len(samples) + 1
    cols, rows, cell, olc, D = 3, 4, 4, 2, 31
    fp = capi.cehog_params(4, 18, True, True, False, True, 0.2)
    t = capi.EhogTracker(ctx, capi.ehog_tracker_params(fp, cols, rows, olc, 12, 60))
    t.update(gray)
    pvalid, pfeat = t.extract_patches(samples)
    cvalid, cfeat = t.extract_cells(samples)
    layers = model.plan_layers(96, 80, cols, cell, 12, 60, olc)
    data = np.fromfile(tmp_path / "out.f32", np.float32)
    at = 0
    for i, s in enumerate(samples):
        for k, (valid, feat) in enumerate(((pvalid, pfeat), (cvalid, cfeat))):
            line = lines[2 * i + k]
            assert (line != "none") == bool(valid[i]), (i, k, line)
            if line == "none":
                continue
            got = [int(v) for v in line.split()]
            assert got[4:] == [rows, cols * D]
            assert data[at:at + rows * cols * D].tobytes() == feat[i].tobytes(), (i, k)
            at += rows * cols * D
            if k == 0:   # ExtendedHogFeatureExtractor.cpp:96-104,125-129
                li, bx, by = model.patch_window(*s, layers, cols, rows, cell, olc)
                scale = layers[li][5]
                ow, oh = model.cv_round(cols * cell / scale), model.cv_round(rows * cell / scale)
                want = [model.cv_round((bx + cell) / scale) + ow // 2, model.cv_round((by + cell) / scale) + oh // 2, ow, oh]
            else:        # DirectPyramidFeatureExtractor.cpp:137-142 in cells
                li, bx, by = model.sample_window(*s, layers, cols, rows, cell, olc)
                scale = layers[li][5]
                ow, oh = model.cv_round(cols * cell / scale), model.cv_round(rows * cell / scale)
                want = [model.cv_round(bx * cell / scale) + ow // 2, model.cv_round(by * cell / scale) + oh // 2, ow, oh]
            assert got[:4] == want, (i, k)
    assert at == data.size and pvalid.sum() >= 4 and cvalid.sum() >= 3 and not pvalid[4]
    t.close()
