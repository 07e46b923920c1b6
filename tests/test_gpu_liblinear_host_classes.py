"""liblinear::LibLinearClassifier of the host layer, trained on the device: a small program retrains twice, with and without the
bias term, on unlimited positives, age-based negatives of capacity 4 and three static negatives with scale 0.5, and prints what
it holds.  Python predicts the rows and their order (positives, negatives, static negatives) and compares with
capi.liblinear_train on them: equal floats.  classification::TrainableProbabilisticSvmClassifier on top computes its logistic
pair as with any other trainable SVM."""
import math
import os
import subprocess

import numpy as np
import pytest

import liblinear_cases as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HIGH, LOW = 39, 0.95, 0.05

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include "classification/AgeBasedExampleManagement.hpp"
#include "classification/TrainableProbabilisticSvmClassifier.hpp"
#include "liblinear/LibLinearClassifier.hpp"
using namespace classification;
using liblinear::LibLinearClassifier;

static std::vector<cv::Mat> take(std::ifstream& f, int n, int d) {
    std::vector<cv::Mat> out;
    for (int i = 0; i < n; ++i) {
        cv::Mat m(1, d, CV_32FC1);
        f.read((char*)m.data, sizeof(float) * d);
        out.push_back(m);
    }
    return out;
}

static void report(const char* what, bool result, LibLinearClassifier& svm, TrainableProbabilisticSvmClassifier& tp, const std::vector<cv::Mat>& probes) {
    const fd_liblinear_params& p = svm.getLastTrainingParameters();
    const fd_liblinear_info& info = svm.getLastTrainingInfo();
    std::printf("%s result %d usable %d\n", what, result ? 1 : 0, tp.isUsable() ? 1 : 0);
    std::printf("params %.17g %.17g %.17g %.17g %d\n", p.C, p.weight_pos, p.weight_neg, p.eps, p.bias);
    std::printf("info %d %d %d %d %d\n", info.iterations, info.cg_steps, info.converged, svm.getLastPositiveCount(), svm.getLastNegativeCount());
    const auto& sv = svm.getSvm()->getSupportVectors();
    std::printf("svm %zu %zu %.9g %.9g\nw", sv.size(), svm.getSvm()->getCoefficients().size(),
                svm.getSvm()->getCoefficients().empty() ? 0.f : svm.getSvm()->getCoefficients()[0], svm.getSvm()->getBias());
    if (!sv.empty()) for (int k = 0; k < sv[0].cols; ++k) std::printf(" %.9g", sv[0].at<float>(0, k));
    std::printf("\nlogistic %.17g %.17g\ndistances", tp.getProbabilisticSvm()->getLogisticA(), tp.getProbabilisticSvm()->getLogisticB());
    for (const cv::Mat& m : probes) std::printf(" %.17g", svm.getSvm()->computeHyperplaneDistance(m));
    std::printf("\n");
}

int main(int argc, char** argv) {
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[5];
    f.read((char*)hdr, sizeof(hdr));
    const int d = hdr[0];
    auto p1 = take(f, hdr[1], d), n1 = take(f, hdr[2], d), p2 = take(f, hdr[3], d), n2 = take(f, hdr[4], d);
    std::vector<cv::Mat> all;
    for (auto* v : {&p1, &n1, &p2, &n2}) all.insert(all.end(), v->begin(), v->end());
    for (int bias = 0; bias < 2; ++bias) {
        auto svm = std::make_shared<LibLinearClassifier>(2.0, bias != 0);
        svm->setNegativeExampleManagement(std::unique_ptr<ExampleManagement>(new AgeBasedExampleManagement(4)));
        svm->loadStaticNegatives(argv[2], 3, 0.5);
        TrainableProbabilisticSvmClassifier tp(svm, 2, 3, ''' + repr(HIGH) + ", " + repr(LOW) + r''');
        std::printf("start%d usable %d static %zu\n", bias, tp.isUsable() ? 1 : 0, svm->getStaticNegatives().size());
        report(bias ? "first1" : "first0", tp.retrain(p1, n1), *svm, tp, all);
        report(bias ? "nothing1" : "nothing0", tp.retrain(std::vector<cv::Mat>(), std::vector<cv::Mat>()), *svm, tp, all);
        report(bias ? "second1" : "second0", tp.retrain(p2, n2), *svm, tp, all);
        tp.reset();
        std::printf("reset%d usable %d sv %zu bias %.9g\n", bias, tp.isUsable() ? 1 : 0, svm->getSvm()->getSupportVectors().size(), svm->getSvm()->getBias());
    }
    try {
        std::vector<cv::Mat> bytes{cv::Mat::zeros(1, d, CV_8UC1)};
        LibLinearClassifier().retrain(bytes, n1);
        std::printf("throws depth no\n");
    } catch (const std::invalid_argument&) {
        std::printf("throws depth invalid_argument\n");
    }
    return 0;
}
'''


def _ring(store, capacity, new, pos):
    for e in new:
        if len(store) < capacity:
            store.append(e)
        else:
            store[pos] = e
            pos = (pos + 1) % len(store)
    return pos


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("liblinear_host_classes")
    x = L.make_x(77, 5, 9, D)
    p1, p2, n1, n2 = x[:2], x[2:5], x[5:8], x[8:14]   # 2 + 3 positives, 3 + 6 negatives
    static = L.make_x(78, 1, 4, D)[1:]                 # four lines, three are read
    data, negatives = d / "examples.bin", d / "negatives.txt"
    with open(data, "wb") as f:
        f.write(np.array([D, len(p1), len(n1), len(p2), len(n2)], np.int32).tobytes())
        for a in (p1, n1, p2, n2):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    negatives.write_text("".join(",".join("%.9g" % (2 * v) for v in row) + "\n" for row in static))
    src, exe = d / "classes.cpp", d / "classes"
    src.write_text(PROGRAM)
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(pkg, "host", "include"), "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    r = subprocess.run([str(exe), str(data), str(negatives)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # what the program holds of the file: (float)(0.5 * value) of the nine-digit text of 2 x
    held = np.array([[np.float32(0.5 * float("%.9g" % (2 * v))) for v in row] for row in static[:3]], np.float32)
    return r.stdout.splitlines(), (p1, n1, p2, n2), held


def _block(lines, what):
    k = next(i for i, l in enumerate(lines) if l.startswith(what + " result"))
    head = lines[k].split()
    out = dict(result=int(head[2]), usable=int(head[4]))
    out["params"] = [float(v) for v in lines[k + 1].split()[1:]]
    out["info"] = [int(v) for v in lines[k + 2].split()[1:]]
    t = lines[k + 3].split()[1:]
    out["nsv"], out["ncoef"], out["coef"], out["bias"] = int(t[0]), int(t[1]), float(t[2]), float(t[3])
    out["w"] = np.array([float(v) for v in lines[k + 4].split()[1:]], np.float32)
    t = lines[k + 5].split()
    out["logistic"] = (float(t[1]), float(t[2]))
    out["distances"] = [float(v) for v in lines[k + 6].split()[1:]]
    return out


def _logistic(mean_pos, mean_neg, high=HIGH, low=LOW):
    b = (math.log((1 - low) / low) - math.log((1 - high) / high)) / (mean_neg - mean_pos)
    return math.log((1 - high) / high) - b * mean_pos, b


def _mean(values):
    s = 0.0
    for v in values:
        s += v
    return s / len(values)


def _check(capi, ctx, got, bias, pos, neg, held, pos_ring, neg_ring, allx):
    x = np.concatenate([pos, neg, held])
    assert got["result"] == 1 and got["usable"] == 1
    assert got["params"] == [2.0, 1.0, 1.0, 0.01, float(bias)]
    w, b, _, _, info = capi.liblinear_train(ctx, x, len(pos), C=2.0, bias=bool(bias))
    assert got["info"] == [info["iterations"], info["cg_steps"], info["converged"], len(pos), len(neg) + len(held)]
    assert (got["nsv"], got["ncoef"], got["coef"]) == (1, 1, 1.0)
    assert np.float32(got["bias"]).tobytes() == np.float32(b).tobytes() and (b != 0) == bool(bias)
    assert got["w"].tobytes() == w.tobytes()
    for k, dist in enumerate(got["distances"]):   # the classifier object scores with what it was given
        assert abs(dist - (float(allx[k].astype(np.float64) @ w.astype(np.float64)) - b)) <= 1e-4
    a, bb = _logistic(_mean([got["distances"][i] for i in pos_ring]), _mean([got["distances"][i] for i in neg_ring]))
    assert got["logistic"] == (a, bb)


@pytest.mark.parametrize("bias", [0, 1])
def test_retrain_twice(capi, ctx, run, bias):
    lines, (p1, n1, p2, n2), held = run
    assert "start%d usable 0 static 3" % bias in lines
    allx = np.concatenate([p1, n1, p2, n2])
    ip1, in1 = list(range(0, 2)), list(range(2, 5))
    ip2, in2 = list(range(5, 8)), list(range(8, 14))
    pos_ring, neg_ring = [], []
    pp = _ring(pos_ring, 2, ip1, 0)
    pn = _ring(neg_ring, 3, in1, 0)
    first = _block(lines, "first%d" % bias)
    _check(capi, ctx, first, bias, allx[ip1], allx[in1], held, pos_ring, neg_ring, allx)
    nothing = _block(lines, "nothing%d" % bias)   # nothing new: no training, the model stays
    assert nothing["result"] == 1 and nothing["w"].tobytes() == first["w"].tobytes() and nothing["info"] == first["info"]
    negs = []
    p = _ring(negs, 4, in1, 0)
    p = _ring(negs, 4, in2, p)
    assert negs == [in2[5], in2[2], in2[3], in2[4]]
    _ring(pos_ring, 2, ip2, pp)
    _ring(neg_ring, 3, in2, pn)
    second = _block(lines, "second%d" % bias)
    _check(capi, ctx, second, bias, allx[ip1 + ip2], allx[negs], held, pos_ring, neg_ring, allx)
    assert second["w"].tobytes() != first["w"].tobytes()


def test_reset_and_depth(run):
    lines = run[0]
    assert "reset0 usable 0 sv 0 bias 0" in lines and "reset1 usable 0 sv 0 bias 0" in lines
    assert "throws depth invalid_argument" in lines
