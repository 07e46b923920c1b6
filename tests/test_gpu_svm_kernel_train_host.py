"""libsvm::LibSvmClassifier::createBinaryKernelSvm of the host layer (not in the reference: createBinarySvm keeps refusing the
kernels it does not train), trained on the device: a small program retrains an RBF classifier twice and resets it; support vectors,
coefficients and bias are compared with capi.kernel_svm_train on the examples that the Python restatement of the stores predicts
(unlimited positives, age-based negatives of capacity 4), the class weights with compensateImbalance's rule."""
import os
import subprocess

import numpy as np
import pytest

import svm_kernel_train_model as K
import svm_train_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, GAMMA = 39, 0.5
KERNEL = (K.RBF, GAMMA, 0.0, 0.0)

PROGRAM = r'''
#include <cstdio>
#include <fstream>
#include "classification/AgeBasedExampleManagement.hpp"
#include "classification/TrainableProbabilisticSvmClassifier.hpp"
#include "classification/HistogramIntersectionKernel.hpp"
#include "classification/RbfKernel.hpp"
#include "libsvm/LibSvmClassifier.hpp"
using namespace classification;
using libsvm::LibSvmClassifier;

static std::vector<cv::Mat> take(std::ifstream& f, int n, int d) {
    std::vector<cv::Mat> out;
    for (int i = 0; i < n; ++i) {
        cv::Mat m(1, d, CV_32FC1);
        f.read((char*)m.data, sizeof(float) * d);
        out.push_back(m);
    }
    return out;
}

static void report(const char* what, bool result, LibSvmClassifier& svm, TrainableProbabilisticSvmClassifier& tp, const std::vector<cv::Mat>& probes) {
    const fd_svm_train_params& p = svm.getLastTrainingParameters();
    const fd_svm_train_info& info = svm.getLastTrainingInfo();
    std::printf("%s result %d usable %d\n", what, result ? 1 : 0, tp.isUsable() ? 1 : 0);
    std::printf("params %.17g %.17g %.17g %.17g\n", p.C, p.weight_pos, p.weight_neg, p.eps);
    std::printf("info %d %d %d %d %.17g\n", info.iterations, info.converged, info.n_sv, info.n_bounded, info.rho);
    const auto& sv = svm.getSvm()->getSupportVectors();
    const auto& coef = svm.getSvm()->getCoefficients();
    std::printf("svm %zu %zu %.9g %d %d\ncoefficients", sv.size(), coef.size(), svm.getSvm()->getBias(), svm.getLastPositiveCount(),
                svm.getLastNegativeCount());
    for (float c : coef) std::printf(" %.9g", c);
    std::printf("\n");
    for (const cv::Mat& m : sv) {
        std::printf("sv %d %d", m.rows, m.cols);
        for (int k = 0; k < m.cols; ++k) std::printf(" %.9g", m.at<float>(0, k));
        std::printf("\n");
    }
    std::printf("distances");
    for (const cv::Mat& m : probes) std::printf(" %.17g", svm.getSvm()->computeHyperplaneDistance(m));
    std::printf("\n");
}

template <class F> static void expectInvalid(const char* what, F f) {
    try {
        f();
        std::printf("throws %s no\n", what);
    } catch (const std::invalid_argument&) {
        std::printf("throws %s invalid_argument\n", what);
    }
}

int main(int argc, char** argv) {
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[5];
    f.read((char*)hdr, sizeof(hdr));
    const int d = hdr[0];
    auto p1 = take(f, hdr[1], d), n1 = take(f, hdr[2], d), p2 = take(f, hdr[3], d), n2 = take(f, hdr[4], d);
    std::vector<cv::Mat> all;
    for (auto* v : {&p1, &n1, &p2, &n2}) all.insert(all.end(), v->begin(), v->end());
    auto svm = LibSvmClassifier::createBinaryKernelSvm(std::make_shared<RbfKernel>(''' + repr(GAMMA) + r'''), 1.0, true);
    svm->setNegativeExampleManagement(std::unique_ptr<ExampleManagement>(new AgeBasedExampleManagement(4)));
    TrainableProbabilisticSvmClassifier tp(svm, 2, 3);
    std::printf("start usable %d kernelform %d\n", tp.isUsable() ? 1 : 0, svm->trainsSupportVectors() ? 1 : 0);
    report("first", tp.retrain(p1, n1), *svm, tp, all);
    report("nothing", tp.retrain(std::vector<cv::Mat>(), std::vector<cv::Mat>()), *svm, tp, all);
    report("second", tp.retrain(p2, n2), *svm, tp, all);
    std::printf("logistic %d\n", tp.getProbabilisticSvm()->getLogisticB() < 0 ? 1 : 0);
    tp.reset();
    std::printf("reset usable %d sv %zu\n", tp.isUsable() ? 1 : 0, svm->getSvm()->getSupportVectors().size());
    auto waiting = LibSvmClassifier::createBinaryKernelSvm(std::make_shared<HistogramIntersectionKernel>());
    waiting->setNegativeExampleManagement(std::unique_ptr<ExampleManagement>(new AgeBasedExampleManagement(10, 9)));
    std::printf("waiting %d\n", waiting->retrain(p1, n1) ? 1 : 0);
    // on an SvmClassifier of the caller's
    auto given = std::make_shared<SvmClassifier>(std::make_shared<HistogramIntersectionKernel>());
    auto onGiven = LibSvmClassifier::createBinaryKernelSvm(given);
    const bool givenUsable = onGiven->retrain(p1, n1);
    std::printf("given %d sv %zu\n", givenUsable ? 1 : 0, given->getSupportVectors().size());
    expectInvalid("rbf", [] { LibSvmClassifier::createBinarySvm(std::make_shared<RbfKernel>(0.5)); });
    expectInvalid("oneclass", [] { LibSvmClassifier::createOneClassSvm(std::make_shared<RbfKernel>(0.5)); });
    expectInvalid("depth", [&] {
        std::vector<cv::Mat> bytes{cv::Mat::zeros(1, d, CV_8UC1)};
        LibSvmClassifier::createBinaryKernelSvm(std::make_shared<RbfKernel>(0.5))->retrain(bytes, n1);
    });
    expectInvalid("gamma", [&] { LibSvmClassifier::createBinaryKernelSvm(std::make_shared<RbfKernel>(-1.0))->retrain(p1, n1); });
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
    d = tmp_path_factory.mktemp("svm_kernel_train_host")
    x = M.ehog_like(5, 9, D, seed=77)
    p1, p2, n1, n2 = x[:2], x[2:5], x[5:8], x[8:14]   # 2 + 3 positives, 3 + 6 negatives
    data = d / "examples.bin"
    with open(data, "wb") as f:
        f.write(np.array([D, len(p1), len(n1), len(p2), len(n2)], np.int32).tobytes())
        for a in (p1, n1, p2, n2):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    src, exe = d / "classes.cpp", d / "classes"
    src.write_text(PROGRAM)
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(pkg, "host", "include"), "-I",
                    os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines(), (p1, n1, p2, n2)


def _block(lines, what):
    k = next(i for i, l in enumerate(lines) if l.startswith(what + " result"))
    head = lines[k].split()
    out = dict(result=int(head[2]), usable=int(head[4]))
    out["params"] = [float(v) for v in lines[k + 1].split()[1:]]
    t = lines[k + 2].split()[1:]
    out["info"] = [int(v) for v in t[:4]] + [float(t[4])]
    t = lines[k + 3].split()[1:]
    out["nsv"], out["ncoef"], out["bias"], out["counts"] = int(t[0]), int(t[1]), float(t[2]), (int(t[3]), int(t[4]))
    out["coef"] = np.array([float(v) for v in lines[k + 4].split()[1:]], np.float32)
    out["sv"] = np.array([[float(v) for v in lines[k + 5 + q].split()[3:]] for q in range(out["nsv"])], np.float32)
    out["shapes"] = [tuple(int(v) for v in lines[k + 5 + q].split()[1:3]) for q in range(out["nsv"])]
    out["distances"] = [float(v) for v in lines[k + 5 + out["nsv"]].split()[1:]]
    return out


def _check(capi, ctx, got, pos, neg, allx):
    x = np.concatenate([pos, neg])
    wp, wn = len(neg) / len(pos), len(pos) / len(neg)
    assert got["result"] == 1 and got["usable"] == 1 and got["counts"] == (len(pos), len(neg))
    assert got["params"] == [1.0, wp, wn, 1e-4]   # compensateImbalance: negatives / positives and positives / negatives
    sv_index, coef, sv, bias, alpha, info = capi.kernel_svm_train(ctx, x, len(pos), KERNEL, C=1.0, weight_pos=wp, weight_neg=wn, eps=1e-4)
    assert got["info"] == [info["iterations"], info["converged"], info["n_sv"], info["n_bounded"], info["rho"]]
    assert got["nsv"] == got["ncoef"] == info["n_sv"] >= 2 and np.float32(got["bias"]) == np.float32(bias)
    assert got["coef"].tobytes() == coef.tobytes() and got["sv"].tobytes() == sv.tobytes() == x[sv_index].tobytes()
    assert got["shapes"] == [(1, D)] * info["n_sv"]   # the stored example Mats themselves
    # the classifier object scores with what it was given, at the tolerance of the scorer's closure test
    want = coef.astype(np.float64) @ K.kernel64_between(sv, allx, KERNEL) - info["rho"]
    tol = 1e-4 * max(1.0, float(np.abs(coef.astype(np.float64)).sum()))   # max |K| = 1
    assert np.abs(np.array(got["distances"]) - want).max() <= tol


def test_retrain_twice(capi, ctx, run):
    lines, (p1, n1, p2, n2) = run
    assert lines[0] == "start usable 0 kernelform 1"
    allx = np.concatenate([p1, n1, p2, n2])
    ip1, in1 = list(range(0, 2)), list(range(2, 5))
    ip2, in2 = list(range(5, 8)), list(range(8, 14))
    first = _block(lines, "first")
    _check(capi, ctx, first, allx[ip1], allx[in1], allx)
    # nothing new: no training, the model stays
    nothing = _block(lines, "nothing")
    assert nothing["result"] == 1 and nothing["sv"].tobytes() == first["sv"].tobytes() and nothing["info"] == first["info"]
    # second: the stored examples are reused; the age-based negatives (capacity 4) keep n1 + n2[0], then n2[1:] overwrite the oldest
    negs = []
    p = _ring(negs, 4, in1, 0)
    p = _ring(negs, 4, in2, p)
    assert negs == [in2[5], in2[2], in2[3], in2[4]]
    second = _block(lines, "second")
    _check(capi, ctx, second, allx[ip1 + ip2], allx[negs], allx)
    assert second["sv"].tobytes() != first["sv"].tobytes()
    assert "logistic 1" in lines   # TrainableProbabilisticSvmClassifier on top: positives score above negatives


def test_reset_other_kernels_and_exceptions(run):
    lines, _ = run
    assert "reset usable 0 sv 0" in lines and "waiting 0" in lines
    given = next(l for l in lines if l.startswith("given")).split()
    assert given[1] == "1" and int(given[3]) >= 2
    for what in ("rbf", "oneclass", "depth", "gamma"):
        assert "throws %s invalid_argument" % what in lines
