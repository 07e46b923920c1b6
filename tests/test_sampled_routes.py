"""The host layer's answer to "which batched device call serves this extractor's samples?", without a device: sampledChainOf
(imageprocessing/imageprocessing_all.hpp) and sampledRoute (condensation/condensation_all.hpp) on objects that are only constructed.
The expected rows are the branch order of SingleClassifierModel::evaluate, DirectPyramidFeatureExtractor::extract(samples),
PositionDependentMeasurementModel::hasWindow / extractAll, patch_channels and rvm_classify_samples as they stood before the descriptor
existed, written out row by row.

A histogram or extended-HOG chain resolves only on a pyramid with a layer filter, and such a pyramid owns a native pyramid from its
constructor on: those two resolution rows run in the test marked gpu (the same program with the argument "device").  Their routes and
derived facts are checked without a device on descriptors filled in by hand.

ExtendedHogFilter refuses an odd bin count with signed-and-unsigned gradients, so the channel rows are 9 bins unsigned (9 + 4 = 13 floats
per cell) and 18 bins signed-and-unsigned (18 + 9 + 4 = 31)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "condensation/condensation_all.hpp"
#include <cstdio>
#include <cstring>
using namespace imageprocessing;
using namespace classification;
using namespace condensation;
using std::make_shared;
using std::shared_ptr;
using Kind = SampledChain::Kind;
static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }

static shared_ptr<ImagePyramid> grayPyramid() { return ImagePyramid::createApproximated(3, 0.2, 0.8, std::vector<double>()); }   // holds no native pyramid
static shared_ptr<DirectPyramidFeatureExtractor> direct(shared_ptr<ImagePyramid> pyramid, int w, int h, std::initializer_list<shared_ptr<ImageFilter>> filters) {
    auto e = make_shared<DirectPyramidFeatureExtractor>(pyramid, w, h);
    for (auto& f : filters) e->addPatchFilter(f);
    return e;
}
static shared_ptr<DirectImageFeatureExtractor> image(std::initializer_list<shared_ptr<ImageFilter>> filters) {   // never updated: no integral image
    auto e = make_shared<DirectImageFeatureExtractor>();
    e->addImageFilter(make_shared<GrayscaleFilter>());
    e->addImageFilter(make_shared<IntegralImageFilter>());
    for (auto& f : filters) e->addPatchFilter(f);
    return e;
}
static shared_ptr<ProbabilisticSvmClassifier> svm(int depth, int length) {
    auto p = make_shared<ProbabilisticSvmClassifier>(make_shared<RbfKernel>(0.5));
    p->getSvm()->setSvmParameters({cv::Mat(1, length, depth)}, {1.f}, 0.0);
    return p;
}
struct NeverTrained : public TrainableSvmClassifier {
    using TrainableSvmClassifier::TrainableSvmClassifier;
    bool retrain(const std::vector<cv::Mat>&, const std::vector<cv::Mat>&) override { return false; }
    void reset() override {}
};
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
static SampledRoute route(const SampledChain& chain, const shared_ptr<ProbabilisticClassifier>& c) { return sampledRoute(chain, sampledClassifierOf(c.get())); }

int main(int argc, char** argv) {
    const std::string dir = argv[1];
    const bool device = argc > 2 && std::strcmp(argv[2], "device") == 0;
    auto f32 = svm(CV_32F, 20), u8 = svm(CV_8U, 20);
    auto neverTrained = make_shared<NeverTrained>(make_shared<RbfKernel>(0.5));
    neverTrained->getSvm()->setSvmParameters({cv::Mat(1, 20, CV_32F)}, {1.f}, 0.0);
    shared_ptr<ProbabilisticClassifier> trainableF32 = make_shared<FixedTrainableProbabilisticSvmClassifier>(neverTrained, 1.0, 0.0);
    shared_ptr<ProbabilisticClassifier> prvm = make_shared<ProbabilisticRvmClassifier>(rvm(dir + "/a.fdrvm", 4, 5));
    shared_ptr<ProbabilisticClassifier> pwvm = make_shared<ProbabilisticWvmClassifier>(make_shared<WvmClassifier>());

    if (device) {   // the two chains that need a bin-image pyramid
        auto binPyramid = [](int bins, bool signedGradients) {
            auto p = make_shared<ImagePyramid>((size_t)3, 0.2, 0.8);
            p->addLayerFilter(make_shared<GradientFilter>(1));
            p->addLayerFilter(make_shared<GradientBinningFilter>(bins, signedGradients, false));
            return p;
        };
        auto hog = direct(binPyramid(9, false), 20, 20, {make_shared<HogFilter>(9, 5, 2)});
        const SampledChain h = sampledChainOf(hog.get());
        expect(h.kind == Kind::Hist && h.onPyramid() && h.pyramid == hog.get() && !h.image && h.ready(), "one HogFilter on bin-image layers: Hist");
        expect(h.hist.patch_w == 20 && h.hist.patch_h == 20 && h.hist.bins == 9, "Hist: the parameters of getSampledChain");
        expect(h.matRows() == 1 && h.cellChannels() == 1, "Hist: 1 x F, single-channel cells");
        expect(route(h, f32) == SampledRoute::Svm && route(h, u8) == SampledRoute::Loop && route(h, prvm) == SampledRoute::Loop, "Hist routes");
        auto ehog = direct(binPyramid(18, true), 20, 20, {make_shared<ExtendedHogFilter>(18, 5, false, true)});
        const SampledChain e = sampledChainOf(ehog.get());
        expect(e.kind == Kind::Ehog && e.onPyramid() && e.pyramid == ehog.get(), "one ExtendedHogFilter on gradient-bin layers: Ehog");
        expect(e.ehog.patch_w == 20 && e.ehog.patch_h == 20 && e.ehog.bins == 18 && e.ehog.cell_w == 5 && e.ehog.cell_h == 5 && e.ehog.signed_and_unsigned, "Ehog: the parameters");
        expect(e.matRows() == 4 && e.cellChannels() == 31, "Ehog: four cell rows of 18 + 9 + 4 floats per cell");
        auto ehog9 = direct(binPyramid(9, false), 20, 20, {make_shared<ExtendedHogFilter>(9, 5, false, false)});
        expect(sampledChainOf(ehog9.get()).kind == Kind::Ehog && sampledChainOf(ehog9.get()).cellChannels() == 13, "Ehog, 9 unsigned bins: 9 + 4 floats per cell");
        expect(route(e, f32) == SampledRoute::Svm && route(e, trainableF32) == SampledRoute::Svm && route(e, prvm) == SampledRoute::Loop, "Ehog routes");
        auto wrappedHog = make_shared<PatchResizingFeatureExtractor>(hog, 1.5);
        expect(sampledChainOf(wrappedHog.get()).kind == Kind::None, "a histogram chain behind a PatchResizingFeatureExtractor: None");
        std::printf("%d failures\n", failures);
        return failures ? 1 : 0;
    }

    // ---- pyramid extractors on a gray pyramid
    auto ehogFilter = make_shared<ExtendedHogFilter>(18, 5, false, true), ehogUnsigned = make_shared<ExtendedHogFilter>(9, 5, false, false);
    auto ehogOnGray = direct(grayPyramid(), 20, 20, {ehogFilter});
    auto gray32 = direct(grayPyramid(), 20, 24, {make_shared<ConversionFilter>(CV_32F, 1.0 / 255.0, 0.0)});
    auto hq32 = direct(grayPyramid(), 20, 20, {make_shared<HistEq64Filter>(), make_shared<ConversionFilter>(CV_32F, 1.0 / 255.0, 0.0)});
    auto whi = direct(grayPyramid(), 20, 20, {make_shared<WhiteningFilter>(), make_shared<HistogramEqualizationFilter>(),
                                              make_shared<ConversionFilter>(CV_32F, 1.0 / 127.5, -1.0), make_shared<UnitNormFilter>(cv::NORM_L2)});
    auto hq = direct(grayPyramid(), 20, 20, {make_shared<HistEq64Filter>()});
    auto hogOnGray = direct(grayPyramid(), 20, 20, {make_shared<HogFilter>(9, 5, 2)});
    {
        const SampledChain c = sampledChainOf(ehogOnGray.get());
        expect(c.kind == Kind::None && !c.onPyramid() && !c.ready() && !c.extractable(), "an ExtendedHogFilter on a gray pyramid: None");
        expect(c.pyramid == ehogOnGray.get() && c.cellChannels() == 31, "... whose cells still have 18 + 9 + 4 channels (patch_channels asks the filter)");
        expect(sampledChainOf(direct(grayPyramid(), 20, 20, {ehogUnsigned}).get()).cellChannels() == 13, "unsigned only: 9 + 4 channels");
        expect(sampledChainOf(make_shared<PatchResizingFeatureExtractor>(ehogOnGray, 1.5).get()).cellChannels() == 31, "the channels of an ehog extractor behind a wrapper");
        expect(sampledChainOf(hogOnGray.get()).kind == Kind::None, "a HogFilter on a gray pyramid: None");
    }
    {
        const SampledChain c = sampledChainOf(gray32.get());
        expect(c.kind == Kind::Patch && c.patch.feature_space == FD_FEATURE_GRAY && c.patch.patch_w == 20 && c.patch.patch_h == 24, "[ConversionFilter(CV_32F)]: Patch / GRAY");
        expect(c.patch.conv_scale == (float)(1.0 / 255.0) && c.patch.conv_shift == 0.f, "Patch: the conversion in float");
        expect(c.onPyramid() && c.ready() && c.extractable() && c.pyramid == gray32.get() && !c.wrappers.wrapped(), "Patch: on the pyramid, itself");
        expect(c.matRows() == 24 && c.cellChannels() == 1 && c.featureLength(1) == 480, "a gray patch keeps its shape: 24 rows, 480 floats");
        expect(route(c, prvm) == SampledRoute::PatchRvm, "Patch + ProbabilisticRvmClassifier: PatchRvm");
        expect(route(c, trainableF32) == SampledRoute::Svm, "Patch + f32 SVM behind a TrainableProbabilisticSvmClassifier: Svm");
        expect(route(c, f32) == SampledRoute::Svm && route(c, u8) == SampledRoute::Loop && route(c, pwvm) == SampledRoute::Loop, "Patch + f32 SVM, u8 SVM, WVM");
    }
    expect(sampledChainOf(hq32.get()).kind == Kind::Patch && sampledChainOf(hq32.get()).patch.feature_space == FD_FEATURE_HQ64, "[HistEq64Filter, ConversionFilter]: Patch / HQ64");
    {
        const SampledChain c = sampledChainOf(whi.get());
        expect(c.kind == Kind::Patch && c.patch.feature_space == FD_FEATURE_WHI, "the four-filter whi chain: Patch / WHI");
        expect(route(c, prvm) == SampledRoute::PatchRvm && route(c, f32) == SampledRoute::Svm, "whi routes");
    }
    expect(sampledChainOf(hq.get()).kind == Kind::None, "[HistEq64Filter] alone: None");
    for (const shared_ptr<DirectPyramidFeatureExtractor>& e : {gray32, hq32, whi}) {
        auto wrapped = make_shared<PatchResizingFeatureExtractor>(e, 1.5);
        const SampledChain c = sampledChainOf(wrapped.get());
        expect(c.kind == Kind::None && c.pyramid == e.get() && c.wrappers.wrapped(), "a pyramid chain behind a PatchResizingFeatureExtractor: None");
        expect(route(c, f32) == SampledRoute::Loop && route(c, prvm) == SampledRoute::Loop, "None + anything: Loop");
    }
    expect(sampledChainOf(nullptr).kind == Kind::None, "no extractor: None");

    // ---- image extractors, bare and behind one and two wrappers
    auto haar = image({make_shared<HaarFeatureFilter>()});
    auto surf = image({make_shared<IntegralGradientFilter>(8), make_shared<GradientSumFilter>(4), make_shared<UnitNormFilter>(cv::NORM_L2)});
    auto ihog = image({make_shared<IntegralGradientFilter>(10, 10), make_shared<GradientBinningFilter>(9, false, false), make_shared<HogFilter>(9, 5, 2)});
    auto iehog = image({make_shared<IntegralGradientFilter>(10, 10), make_shared<GradientBinningFilter>(18, true, false), ehogFilter});
    auto surfL1 = image({make_shared<IntegralGradientFilter>(8), make_shared<GradientSumFilter>(4), make_shared<UnitNormFilter>(cv::NORM_L1)});
    struct Row { shared_ptr<DirectImageFeatureExtractor> e; Kind kind; const char* what; };
    for (const Row& r : {Row{haar, Kind::Haar, "haar"}, Row{surf, Kind::Surf, "surf"}, Row{ihog, Kind::IntegralHog, "ihog"}, Row{iehog, Kind::IntegralHog, "iehog"}}) {
        auto one = make_shared<IntegralFeatureExtractor>(r.e);
        auto two = make_shared<PatchResizingFeatureExtractor>(one, 2.0, 0.25, 0.0);
        for (const FeatureExtractor* outer : {(const FeatureExtractor*)r.e.get(), (const FeatureExtractor*)one.get(), (const FeatureExtractor*)two.get()}) {
            const SampledChain c = sampledChainOf(outer);
            expect(c.kind == r.kind && c.image == r.e.get() && !c.pyramid && !c.onPyramid(), r.what);
            expect(!c.ready() && !c.extractable(), "no integral image yet: not ready (the callers keep their loops)");
            expect(route(c, f32) == SampledRoute::Svm && route(c, u8) == SampledRoute::Loop && route(c, prvm) == SampledRoute::Loop, "the pure route does not ask for a device");
            expect(c.wrappers.wrapped() == (outer != r.e.get()), "wrapped");
        }
        // outer to inner: PatchResizing (10, 20, 7, 9) -> (10, cvRound(22.25) = 22, 14, 18), then Integral: even sizes, (10, 22, 15, 19);
        // inner to outer would be (11, 21, 8, 10) -> (11, cvRound(23.5) = 24, 16, 20)
        int32_t s[4] = {10, 20, 7, 9};
        sampledChainOf(two.get()).wrappers.map(s);
        expect(s[0] == 10 && s[1] == 22 && s[2] == 15 && s[3] == 19, "map() applies the wrappers outer to inner");
    }
    expect(sampledChainOf(haar.get()).haar == haar->getHaarChain() && sampledChainOf(surf.get()).haar == nullptr, "Haar keeps its filter");
    expect(sampledChainOf(surf.get()).surf.gradient_count == 8 && sampledChainOf(surf.get()).surf.cell_count == 4, "Surf: gradient and cell count");
    expect(sampledChainOf(surfL1.get()).kind == Kind::None, "gradient + sum + L1 norm: None");
    {
        const SampledChain h = sampledChainOf(ihog.get()), e = sampledChainOf(iehog.get());
        expect(h.ihog.kind == FD_SAMPLES_HIST && h.ihog.grad_rows == 10 && h.ihog.bins == 9 && h.matRows() == 1 && h.cellChannels() == 1, "ihog: the histogram sub-kind, 1 x F");
        expect(e.ihog.kind == FD_SAMPLES_EHOG && e.matRows() == 2 && e.cellChannels() == 31, "iehog: the extended-HOG sub-kind, two cell rows of 31 channels");
        expect(sampledChainOf(make_shared<IntegralFeatureExtractor>(iehog).get()).cellChannels() == 31, "iehog behind a wrapper: 31 channels");
    }

    // ---- descriptors filled in by hand: the routes and derived facts of the kinds that resolve on bin-image layers only
    {
        SampledChain h(nullptr);
        h.kind = Kind::Hist;
        expect(route(h, f32) == SampledRoute::Svm, "Hist + f32 SVM: Svm");
        expect(route(h, u8) == SampledRoute::Loop, "Hist + u8 SVM: Loop");
        expect(route(h, prvm) == SampledRoute::Loop, "Hist + ProbabilisticRvmClassifier: Loop");
        expect(route(h, trainableF32) == SampledRoute::Svm, "Hist + trainable f32 SVM: Svm");
        expect(h.matRows() == 1 && h.cellChannels() == 1 && h.onPyramid(), "Hist: 1 x F");
        SampledChain e(nullptr);
        e.kind = Kind::Ehog;
        e.ehog = fd_ehog_patch_params{20, 23, 9, 5, 5, 0, 1, 0.2f};
        expect(e.matRows() == 5, "Ehog: cvRound(23 / 5) cell rows");
        e.ehog.patch_h = 22;
        expect(e.matRows() == 4, "Ehog: cvRound(22 / 5) cell rows");
        expect(route(e, f32) == SampledRoute::Svm && route(e, prvm) == SampledRoute::Loop && route(e, u8) == SampledRoute::Loop, "Ehog routes");
        SampledChain none(nullptr);
        expect(route(none, f32) == SampledRoute::Loop && route(none, prvm) == SampledRoute::Loop && route(none, trainableF32) == SampledRoute::Loop, "None + anything: Loop");
        expect(none.matRows() == 1 && none.cellChannels() == 1 && !none.ready(), "None: nothing to ask");
    }
    // the classifier, resolved once
    expect(sampledClassifierOf(f32.get()).svm == f32.get() && !sampledClassifierOf(f32.get()).rvm, "an f32 ProbabilisticSvmClassifier");
    expect(!sampledClassifierOf(u8.get()).svm, "u8 vectors: no SVM route");
    expect(sampledClassifierOf(trainableF32.get()).svm == std::static_pointer_cast<TrainableProbabilisticSvmClassifier>(trainableF32)->getProbabilisticSvm().get(), "the SVM behind a trainable classifier");
    expect(sampledClassifierOf(prvm.get()).rvm == prvm.get() && !sampledClassifierOf(prvm.get()).svm, "a ProbabilisticRvmClassifier");
    expect(!sampledClassifierOf(pwvm.get()).svm && !sampledClassifierOf(pwvm.get()).rvm && !sampledClassifierOf(nullptr).svm, "neither");
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
'''


def _run(tmp_path, *args):
    src = tmp_path / "sampled_routes.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "sampled_routes"
    pkg = os.path.join(ROOT, "featuredetection_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(pkg, "host", "include"), "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", pkg, "-lfd_host", "-lfd_hip", "-Wl,-rpath," + pkg], check=True)
    run = subprocess.run([str(exe), str(tmp_path), *args], capture_output=True, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr


def test_sampled_chains_and_routes(tmp_path):
    _run(tmp_path)


@pytest.mark.gpu
def test_sampled_chains_on_bin_image_pyramids(tmp_path):
    _run(tmp_path, "device")
