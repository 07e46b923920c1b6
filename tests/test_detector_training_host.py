"""The host-only pieces of detector training (host/include/detectortraining/): a small program on the host headers prints what
Annotations, DetectorTrainer::adjustSize, the mirroring, createRandomBounds with a fixed seed, the overlap test, cv::flip and
LabeledImage::adjustSizes give, and the documented exceptions that need no device; the output is compared with
tests/detector_training_model.py.  No device is involved."""
import os
import subprocess

import numpy as np
import pytest

import detector_training_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "detectortraining/DetectorTrainer.hpp"
#include "imageprocessing/filtering/FhogFilter.hpp"
using imageio::RectLandmark;

static void print(const char* what, const std::vector<cv::Rect>& boxes) {
    std::printf("%s", what);
    for (const cv::Rect& b : boxes) std::printf(" %d,%d,%d,%d", b.x, b.y, b.width, b.height);
    std::printf("\n");
}
static void print(const RectLandmark& l) {
    std::printf("landmark %s %a %a %a %a\n", l.getName().c_str(), (double)l.getX(), (double)l.getY(), (double)l.getWidth(), (double)l.getHeight());
}
static DetectorTrainer trainer(int ww, int wh, int cell, float ws, float hs, unsigned seed, double overlap = 0.3) {
    DetectorTrainer t(false, "", seed);
    FeatureParams fp;
    fp.windowSizeInCells = cv::Size(ww, wh);
    fp.cellSizeInPixels = cell;
    fp.octaveLayerCount = 2;
    fp.widthScaleFactor = ws;
    fp.heightScaleFactor = hs;
    t.setFeatures(fp, std::make_shared<imageprocessing::filtering::FhogFilter>(cell), std::make_shared<imageprocessing::GrayscaleFilter>());
    TrainingParams tp;
    tp.overlapThreshold = overlap;
    t.setTrainingParameters(tp);
    return t;
}

int main() {
    std::vector<RectLandmark> lms = {RectLandmark("face", 50, 40, 20, 30), RectLandmark("ignore-blur", 100.5f, 60.5f, 11, 10),
                                     RectLandmark("ignored", cv::Rect(3, 4, 5, 6)), RectLandmark("tiny", 10, 10, 4, 4), RectLandmark("wide", 30, 30, 40, 4),
                                     RectLandmark("half", 2.5f, -2.5f, 0, 0)};
    for (int pass = 0; pass < 2; ++pass) {
        Annotations a(lms, pass ? cv::Size(8, 8) : cv::Size());
        print("nonnegatives", a.nonNegatives);
        print("positives", a.positives);
        print("fuzzies", a.fuzzies);
    }
    const double aspects[4][3] = {{4, 4, 1}, {3, 6, 1}, {4, 3, 1}, {4, 3, 0}};
    for (int k = 0; k < 4; ++k) {
        DetectorTrainer t = trainer((int)aspects[k][0], (int)aspects[k][1], 8, aspects[k][2] ? 1.0f : 1.2f, aspects[k][2] ? 1.0f : 1.1f, 1);
        for (const RectLandmark& l : lms) print(t.adjustSize(l));
    }
    {
        LabeledImage li(cv::Mat(4, 4, CV_8UC1), lms);
        li.adjustSizes(4.0 / 3.0);
        for (const RectLandmark& l : li.landmarks) print(l);
    }
    for (float x : {0.f, 127.f, 40.25f, 63.5f}) print(DetectorTrainer::flipHorizontally(RectLandmark("m", x, 7, 3, 4), 128));
    {
        cv::Mat gray(2, 6, CV_8UC1), bgr(1, 4, CV_8UC3);
        for (int i = 0; i < 12; ++i) { gray.data[i] = (unsigned char)i; bgr.data[i] = (unsigned char)i; }
        cv::Mat roi(gray, cv::Rect(1, 0, 4, 2));   // not continuous
        for (const cv::Mat& m : {DetectorTrainer::flipHorizontally(gray), DetectorTrainer::flipHorizontally(bgr), DetectorTrainer::flipHorizontally(roi)}) {
            std::printf("flip %d %d %d :", m.rows, m.cols, m.channels());
            for (int r = 0; r < m.rows; ++r)
                for (int c = 0; c < m.cols * m.channels(); ++c) std::printf(" %d", (int)m.ptr<unsigned char>(r)[c]);
            std::printf("\n");
        }
    }
    const int shapes[3][4] = {{4, 4, 128, 96}, {3, 5, 128, 96}, {4, 4, 32, 40}};
    for (int k = 0; k < 3; ++k)
        for (unsigned seed : {7u, 7u, 8u}) {
            DetectorTrainer t = trainer(shapes[k][0], shapes[k][1], 8, 1, 1, seed);
            std::vector<cv::Rect> boxes;
            for (int i = 0; i < 200; ++i) boxes.push_back(t.createRandomBounds(cv::Size(shapes[k][2], shapes[k][3])));
            print("random", boxes);
        }
    {
        DetectorTrainer t = trainer(4, 4, 8, 1, 1, 1, 0.25);
        std::printf("overlap %a %a %a %d %d %d\n", DetectorTrainer::computeOverlap(cv::Rect(0, 0, 10, 10), cv::Rect(5, 0, 10, 10)),
                    DetectorTrainer::computeOverlap(cv::Rect(0, 0, 10, 10), cv::Rect(10, 0, 10, 10)),
                    DetectorTrainer::computeOverlap(cv::Rect(0, 0, 4, 4), cv::Rect(0, 0, 4, 16)),
                    t.isOverlapping(cv::Rect(0, 0, 4, 4), {cv::Rect(0, 0, 4, 16)}) ? 1 : 0,
                    t.isOverlapping(cv::Rect(0, 0, 4, 4), {cv::Rect(100, 100, 5, 5), cv::Rect(0, 0, 4, 15)}) ? 1 : 0,
                    t.isOverlapping(cv::Rect(0, 0, 4, 4), {}) ? 1 : 0);
    }
    // the exceptions that are thrown before the device is needed
    try {
        DetectorTrainer t = trainer(4, 4, 8, 1, 1, 1);
        TrainingParams tp;
        tp.probabilistic = true;
        t.setTrainingParameters(tp);
        t.train({});
        std::printf("probabilistic: no exception\n");
    } catch (const std::invalid_argument& e) {
        std::printf("probabilistic: invalid_argument %s\n", e.what());
    }
    try {
        DetectorTrainer t = trainer(4, 4, 8, 1, 1, 1);
        t.createRandomBounds(cv::Size(31, 96));
        std::printf("small image: no exception\n");
    } catch (const std::runtime_error& e) {
        std::printf("small image: runtime_error %s\n", e.what());
    }
    try {   // 16385 examples of one float: refused by the classifier before anything is sent to the device
        auto svm = libsvm::LibSvmClassifier::createBinarySvm(std::make_shared<classification::LinearKernel>(), 1.0);
        std::vector<cv::Mat> positives(1, cv::Mat::zeros(1, 1, CV_32FC1)), negatives(16384, cv::Mat::zeros(1, 1, CV_32FC1));
        svm->retrain(positives, negatives);
        std::printf("too many: no exception\n");
    } catch (const std::runtime_error& e) {
        std::printf("too many: runtime_error %s\n", e.what());
    }
    {   // the store of the hard negatives under an untrained classifier: the examples in their order, up to the capacity
        auto svm = libsvm::LibSvmClassifier::createBinarySvm(std::make_shared<classification::LinearKernel>(), 1.0);
        HardNegativeExampleManagement store(svm, 3);
        std::vector<cv::Mat> examples;
        for (int i = 0; i < 5; ++i) {
            examples.push_back(cv::Mat::zeros(1, 1, CV_32FC1));
            examples.back().at<float>(0, 0) = (float)(10 + i);
        }
        store.add(examples);
        std::printf("store %zu :", store.size());
        for (auto it = store.iterator(); it->hasNext();) std::printf(" %d", (int)it->next().at<float>(0, 0));
        std::printf("\n");
    }
    return 0;
}
'''

LMS = [T.landmark("face", 50, 40, 20, 30), T.landmark("ignore-blur", 100.5, 60.5, 11, 10), T.landmark_from_rect("ignored", 3, 4, 5, 6),
       T.landmark("tiny", 10, 10, 4, 4), T.landmark("wide", 30, 30, 40, 4), T.landmark("half", 2.5, -2.5, 0, 0)]


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    d = tmp_path_factory.mktemp("detector_training")
    src, exe = d / "pieces.cpp", d / "pieces"
    src.write_text(PROGRAM)
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(pkg, "host", "include"), "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return run.stdout.splitlines()


def _take(lines, key):
    return [ln[len(key) + 1:] for ln in lines if ln.split(" ", 1)[0] == key]


def _boxes(text):
    return [tuple(int(v) for v in b.split(",")) for b in text.split()]


def _landmark(text):
    name, x, y, w, h = text.split()
    return (name,) + tuple(np.float32(float.fromhex(v)) for v in (x, y, w, h))


def test_annotations(output):
    non, pos, fuz = _take(output, "nonnegatives"), _take(output, "positives"), _take(output, "fuzzies")
    for k, min_size in enumerate([(0, 0), (8, 8)]):
        want = T.annotations(LMS, min_size)
        assert _boxes(non[k]) == want["non_negatives"] and _boxes(pos[k]) == want["positives"] and _boxes(fuz[k]) == want["fuzzies"]
    assert _boxes(fuz[0]) == [(95, 56, 11, 10), (3, 4, 5, 6)]


def test_adjust_size_and_mirroring(output):
    got = [_landmark(t) for t in _take(output, "landmark")]
    want = []
    for ww, wh, ws, hs in [(4, 4, 1.0, 1.0), (3, 6, 1.0, 1.0), (4, 3, 1.0, 1.0), (4, 3, 1.2, 1.1)]:
        want += [T.adjust_size(lm, ws, hs, float(ww) / float(wh)) for lm in LMS]
    want += [T.adjust_size(lm, 1.0, 1.0, 4.0 / 3.0) for lm in LMS]   # LabeledImage::adjustSizes
    want += [T.flip_landmark(T.landmark("m", x, 7, 3, 4), 128) for x in (0, 127, 40.25, 63.5)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0] and [np.float32(v).tobytes() for v in g[1:]] == [np.float32(v).tobytes() for v in w[1:]], (g, w)
    assert got[-4][1] == 127 and got[-3][1] == 0


def test_flip(output):
    flips = _take(output, "flip")
    gray, bgr = np.arange(12, dtype=np.uint8).reshape(2, 6), np.arange(12, dtype=np.uint8).reshape(1, 4, 3)
    want = [gray, bgr, gray[:, 1:5]]
    for text, img in zip(flips, want):
        head, values = text.split(":")
        rows, cols, ch = (int(v) for v in head.split())
        assert (rows, cols, ch) == (img.shape[0], img.shape[1], 1 if img.ndim == 2 else img.shape[2])
        assert [int(v) for v in values.split()] == T.flip_image(img).reshape(-1).tolist()


def test_random_bounds_with_a_fixed_seed(output):
    runs = [_boxes(t) for t in _take(output, "random")]
    assert len(runs) == 9
    for k, (ww, wh, iw, ih) in enumerate([(4, 4, 128, 96), (3, 5, 128, 96), (4, 4, 32, 40)]):
        a, b, c = runs[3 * k:3 * k + 3]
        assert a == b and len(a) == 200                     # the seed decides
        assert all(T.is_random_bounds(box, iw, ih, ww, wh, 8) for box in a + c)
        lo, hi, _ = T.random_bounds_limits(iw, ih, ww, wh, 8)
        if lo < hi:
            assert a != c
            widths = {box[2] for box in a}
            assert min(widths) < lo + (hi - lo) // 4 and max(widths) > hi - (hi - lo) // 4 and len({box[:2] for box in a}) > 50
        else:
            assert {box[2:] for box in a} == {(32, 32)} and {box[0] for box in a} == {0} and {box[1] for box in a} == set(range(9))


def test_overlap(output):
    o = _take(output, "overlap")[0].split()
    assert [float.fromhex(v) for v in o[:3]] == [T.overlap((0, 0, 10, 10), (5, 0, 10, 10)), 0.0, 0.25]
    assert [int(v) for v in o[3:]] == [0, 1, 0]   # == the threshold keeps, > rejects


def test_documented_exceptions(output):
    text = "\n".join(output)
    assert "probabilistic: invalid_argument" in text and "probabilistic output" in text
    assert "small image: runtime_error" in text
    line = [ln for ln in output if ln.startswith("too many:")][0]
    assert "runtime_error" in line and "16385" in line and "16384" in line and "maxNegatives" in line
    assert "store 3 : 10 11 12" in text
