"""The host layer's two shared decisions, without a device: fdhost::with_capacity (fdcompat/runtime.hpp) over a fake call that records
its invocations, and the route functions of detection/detection_all.hpp on objects that are only constructed.  The expected routes are
the branch order of SlidingWindowDetector::detectWindows and FiveStageSlidingWindowDetector::run as they stood before the functions
existed, written out row by row."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "detection/detection_all.hpp"
#include <cstdio>
#include <cstring>
#include <functional>
using namespace imageprocessing;
using namespace classification;
using namespace detection;
using std::make_shared;
using std::shared_ptr;
static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }

// ---- with_capacity: a call that "has" `have` items and answers `status` when they do not fit (or always, with `always`)
struct Fake {
    int have = 0, status = FD_ERR_CAPACITY;
    bool always = false;
    std::vector<int> capacities;   // one entry per invocation
    int operator()(int* out, int cap, int* count) {
        capacities.push_back(cap);
        *count = have;
        for (int i = 0; i < have && i < cap; ++i) out[i] = 100 + i;
        return always || have > cap ? status : FD_OK;
    }
};
static bool throws(const std::function<void()>& f) {
    try { f(); } catch (const std::exception&) { return true; }
    return false;
}
static void capacity_cases() {
    {   // a result that fits: one call
        Fake f; f.have = 3;
        std::vector<int> v = fdhost::with_capacity<int>(4, std::ref(f));
        expect(f.capacities == std::vector<int>{4} && v == std::vector<int>({100, 101, 102}), "fits: one call, trimmed to the count");
    }
    {   // FD_ERR_CAPACITY reporting n: exactly two calls, the second with capacity n, n items
        Fake f; f.have = 9;
        std::vector<int> v = fdhost::with_capacity<int>(4, std::ref(f));
        expect(f.capacities == std::vector<int>({4, 9}), "too small: two calls, the second with the reported count");
        expect(v.size() == 9 && v.front() == 100 && v.back() == 108, "too small: all items");
    }
    {   // a count of 0: empty
        Fake f;
        expect(fdhost::with_capacity<int>(4, std::ref(f)).empty() && f.capacities.size() == 1, "count 0: empty, one call");
    }
    {   // FD_ERR_CAPACITY twice: an error after two calls, never a loop
        Fake f; f.have = 9; f.always = true;
        expect(throws([&] { fdhost::with_capacity<int>(4, std::ref(f)); }), "capacity error twice throws");
        expect(f.capacities == std::vector<int>({4, 9}), "capacity error twice: two calls");
    }
    {   // FD_ERR_DEVICE_CAPACITY: thrown without a second call
        Fake f; f.have = 9; f.always = true; f.status = FD_ERR_DEVICE_CAPACITY;
        expect(throws([&] { fdhost::with_capacity<int>(4, std::ref(f)); }), "device capacity throws");
        expect(f.capacities == std::vector<int>{4}, "device capacity: one call");
    }
    {   // the 64-bit count of the sliding-window scans
        int64_t seen = 0;
        auto v = fdhost::with_capacity<char>((int64_t)1 << 16, [&](char*, int64_t cap, int64_t* count) { seen = cap; *count = 2; return (int)FD_OK; });
        expect(seen == 65536 && v.size() == 2, "int64_t counts");
    }
}

// ---- routes
static shared_ptr<ImagePyramid> pyramid() { return ImagePyramid::createApproximated(3, 0.2, 0.8, std::vector<double>()); }   // holds no native pyramid
static shared_ptr<DirectPyramidFeatureExtractor> direct(std::initializer_list<shared_ptr<ImageFilter>> filters) {
    auto e = make_shared<DirectPyramidFeatureExtractor>(pyramid(), 20, 20);
    for (auto& f : filters) e->addPatchFilter(f);
    return e;
}
static shared_ptr<ProbabilisticSvmClassifier> svm(shared_ptr<Kernel> kernel, int depth, int length) {
    auto p = make_shared<ProbabilisticSvmClassifier>(kernel);
    if (length > 0) p->getSvm()->setSvmParameters({cv::Mat(1, length, depth)}, {1.f}, 0.0);
    return p;
}
// FDRVM1 model file with one filter of w x h
static shared_ptr<RvmClassifier> rvm(const std::string& path, int w, int h) {
    FILE* f = std::fopen(path.c_str(), "wb");
    const int32_t hdr[5] = {FD_KERNEL_RBF, w, h, 1, 1};
    const double prm[3] = {0.5, 0, 0};
    const float bias = 0.f, coeff = 1.f, threshold = 0.f;
    std::vector<float> sv((size_t)w * h, 0.25f);
    std::fwrite("FDRVM1\0\0", 1, 8, f); std::fwrite(hdr, 4, 5, f); std::fwrite(prm, 8, 3, f); std::fwrite(&bias, 4, 1, f);
    std::fwrite(sv.data(), 4, sv.size(), f); std::fwrite(&coeff, 4, 1, f); std::fwrite(&threshold, 4, 1, f);
    std::fclose(f);
    return RvmClassifier::loadFromFile(path);
}

int main(int argc, char** argv) {
    capacity_cases();
    const std::string dir = argv[1];
    auto rbf = make_shared<RbfKernel>(0.5);
    auto linear = make_shared<LinearKernel>();
    auto pwvm = make_shared<ProbabilisticWvmClassifier>(make_shared<WvmClassifier>());
    auto rvmA = rvm(dir + "/a.fdrvm", 4, 5), rvmB = rvm(dir + "/b.fdrvm", 4, 5), rvmC = rvm(dir + "/c.fdrvm", 5, 5);
    auto prvmA = make_shared<ProbabilisticRvmClassifier>(rvmA), prvmA2 = make_shared<ProbabilisticRvmClassifier>(rvmA);
    auto prvmB = make_shared<ProbabilisticRvmClassifier>(rvmB), prvmC = make_shared<ProbabilisticRvmClassifier>(rvmC);
    auto f32rbf = svm(rbf, CV_32F, 20), f32linear = svm(linear, CV_32F, 20), u8rbf = svm(rbf, CV_8U, 20), f32other = svm(rbf, CV_32F, 21),
         noVectors = svm(rbf, CV_32F, 0);

    auto plain = direct({});
    auto histeq = direct({make_shared<HistEq64Filter>()});
    auto hog = direct({make_shared<HogFilter>(9, 5, 2)});
    auto hogInterpolating = direct({make_shared<HogFilter>(9, 5, 2, true)});
    auto gray32 = direct({make_shared<ConversionFilter>(CV_32F, 1.0 / 255.0, 0.0)});
    auto hq32 = direct({make_shared<HistEq64Filter>(), make_shared<ConversionFilter>(CV_32F, 1.0 / 255.0, 0.0)});
    auto whi = make_shared<FilteringPyramidFeatureExtractor>(plain);
    whi->addPatchFilter(make_shared<WhiteningFilter>());
    whi->addPatchFilter(make_shared<HistogramEqualizationFilter>());
    whi->addPatchFilter(make_shared<ConversionFilter>(CV_32F, 1.0 / 127.5, -1.0));
    whi->addPatchFilter(make_shared<UnitNormFilter>(cv::NORM_L2));
    auto lbp = make_shared<FilteringPyramidFeatureExtractor>(plain);
    lbp->addPatchFilter(make_shared<LbpFilter>(LbpFilter::Type::LBP8));

    // (a) the resolver
    expect(resolveFusedExtractor(hog) == hog, "a DirectPyramidFeatureExtractor resolves to itself");
    expect(resolveFusedExtractor(whi) && resolveFusedExtractor(whi) == whi->getFusedExtractor() && resolveFusedExtractor(whi)->getWhiChain(), "a fused filtering extractor resolves to its fused extractor");
    expect(!resolveFusedExtractor(lbp), "an LBP patch filter is not fused");
    expect(!resolveFusedExtractor(nullptr), "no extractor");
    // the f32 predicate
    expect(hasF32SupportVectors(f32rbf.get()) && !hasF32SupportVectors(u8rbf.get()) && !hasF32SupportVectors(noVectors.get()) && !hasF32SupportVectors(nullptr), "f32 vectors");

    // (b) the first-stage route, in the order of precedence
    auto scan = [](const shared_ptr<PyramidFeatureExtractor>& e, const shared_ptr<ProbabilisticClassifier>& c) { return fusedScanRoute(resolveFusedExtractor(e).get(), c.get()); };
    expect(scan(histeq, pwvm) == FusedScan::Wvm, "1: WVM on HistEq64");
    expect(scan(hq32, pwvm) == FusedScan::Wvm, "1: WVM on HistEq64 + conversion");
    expect(scan(plain, pwvm) == FusedScan::Generic, "6: WVM without HistEq64");
    expect(scan(hog, f32rbf) == FusedScan::HogSvm, "2: HOG + f32 RBF SVM");
    expect(scan(hog, f32linear) == FusedScan::HistSvm, "5: HOG with a linear kernel");
    expect(scan(hog, u8rbf) == FusedScan::Generic, "6: HOG with u8 vectors");
    expect(scan(hog, noVectors) == FusedScan::Generic, "6: HOG, an SVM without vectors");
    expect(scan(hogInterpolating, f32rbf) == FusedScan::HistSvm, "5: an interpolating HogFilter is a histogram filter only");
    expect(scan(gray32, prvmA) == FusedScan::Rvm, "3: RVM on gray + conversion");
    expect(scan(hq32, prvmA) == FusedScan::Rvm, "3: RVM on HistEq64 + conversion");
    expect(scan(plain, prvmA) == FusedScan::Generic, "6: RVM without conversion");
    expect(scan(whi, prvmA) == FusedScan::Generic, "6: RVM on the whi chain");
    expect(scan(hog, prvmA) == FusedScan::Generic, "6: RVM on a histogram filter");
    expect(scan(whi, f32rbf) == FusedScan::WhiSvm, "4: a filtering extractor around the whi chain");
    expect(scan(whi, f32linear) == FusedScan::WhiSvm, "4: whi chain, any kernel");
    expect(scan(whi, u8rbf) == FusedScan::Generic, "6: whi chain with u8 vectors");
    expect(scan(lbp, f32rbf) == FusedScan::Generic, "6: a filtering extractor around an LBP filter");
    expect(scan(plain, f32rbf) == FusedScan::Generic, "6: an f32 SVM on unfiltered patches");
    expect(scan(gray32, f32rbf) == FusedScan::Generic, "6: an f32 SVM on a converted u8 feature space");
    expect(scan(histeq, f32rbf) == FusedScan::Generic, "6: an f32 SVM on HistEq64 patches");
    expect(fusedScanRoute(nullptr, pwvm.get()) == FusedScan::Generic, "6: a null fused extractor");

    // (c) the five-stage route
    auto five = [](const shared_ptr<PyramidFeatureExtractor>& e, const shared_ptr<ProbabilisticClassifier>& first, const shared_ptr<ProbabilisticClassifier>& second) {
        return fiveStageRoute(resolveFusedExtractor(e).get(), first.get(), second.get());
    };
    expect(five(histeq, pwvm, u8rbf) == FiveStageRoute::WvmSvm, "WVM + u8 SVM");
    expect(five(histeq, pwvm, noVectors) == FiveStageRoute::WvmSvm, "WVM + an SVM without support vectors");
    expect(five(histeq, pwvm, f32rbf) == FiveStageRoute::Composition, "WVM + f32 SVM");
    expect(five(histeq, pwvm, prvmA) == FiveStageRoute::Composition, "WVM + RVM");
    expect(five(plain, pwvm, u8rbf) == FiveStageRoute::Composition, "WVM without HistEq64");
    expect(five(lbp, pwvm, u8rbf) == FiveStageRoute::Composition, "WVM, no fused extractor");
    expect(five(gray32, prvmA, f32rbf) == FiveStageRoute::RvmSecond, "RVM + f32 SVM of the filter size");
    expect(five(gray32, prvmA, f32linear) == FiveStageRoute::RvmSecond, "RVM + f32 SVM, any kernel");
    expect(five(gray32, prvmA, f32other) == FiveStageRoute::Composition, "RVM + f32 SVM of another length");
    expect(five(gray32, prvmA, u8rbf) == FiveStageRoute::Composition, "RVM + u8 SVM");
    expect(five(gray32, prvmA, noVectors) == FiveStageRoute::Composition, "RVM + an SVM without support vectors");
    expect(five(gray32, prvmA, prvmB) == FiveStageRoute::RvmSecond, "RVM + another RVM of equal filter size");
    expect(five(gray32, prvmA, prvmA2) == FiveStageRoute::Composition, "RVM + the same RvmClassifier");
    expect(five(gray32, prvmA, prvmA) == FiveStageRoute::Composition, "RVM + itself");
    expect(five(gray32, prvmA, prvmC) == FiveStageRoute::Composition, "RVM + an RVM of another filter size");
    expect(five(gray32, prvmA, pwvm) == FiveStageRoute::Composition, "RVM + WVM");
    expect(five(plain, prvmA, f32rbf) == FiveStageRoute::Composition, "RVM without conversion");
    expect(five(hog, f32rbf, f32rbf) == FiveStageRoute::Composition, "an SVM first stage");
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
'''


def test_capacity_retry_and_routes(tmp_path):
    src = tmp_path / "host_routes.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "host_routes"
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
