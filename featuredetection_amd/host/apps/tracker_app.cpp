// tracker_app -- the frame loop of the reference's adaptiveTrackingApp / headTrackingApp / trackingBenchmarkApp (TrackingBenchmark.cpp:489-510,553):
// a condensation::AdaptiveCondensationTracker on ResamplingSampler(LowVarianceSampling, SimpleTransitionModel or OpticalFlowTransitionModel)
// or GridSampler, an
// ExtendedHogBasedMeasurementModel and FilteringStateExtractor(WeightedMeanStateExtractor).
//   usage: tracker_app [--counts] [--adaptation] [--dump] <config.cfg> <x> <y> <width> <height> <frame0.ppm|pgm> [<frame1> ...]
// config (boost info format), the `tracking` block of algorithm.cfg:
//   tracking {
//     transition simple { positionDeviation 10  sizeDeviation 0.1 }
//     transition opticalFlow { positionDeviation 10  sizeDeviation 0.08  fallback simple { positionDeviation 12.8  sizeDeviation 0.1 } }
//                                                                              (headTrackingApp/default.cfg:16-27; in place of the line above)
//     adaptive { resampling { particleCount 800  randomRate 0.35  minSize 40  maxSize 200 } }
//     tracker partiallyAdaptive: `measurement wvmSvm { .. }` as the static model and `adaptive selfLearning { .. }` (tracking_setup.hpp) as the
//                        adaptive one; no initialisation, every frame is printed
//     grid { minSize 20 maxSize 80 sizeScale 1.2 stepSize 0.1 }                (optional: a GridSampler in place of the resampling sampler)
//     initialCount 800   seed 1                                                (seed: the samplers' generators get seed, seed + 1, seed + 2;
//                                                                               seed + 1 is the simple model's, also as the fallback; the flow model's seed + 3)
//     measurement ehog { cellSize 5 cellCount 35 signedAndUnsigned 0 interpolateBins 0 interpolateCells 1 octaveLayerCount 5
//                        rejectionThreshold -1.5 useSlidingWindow 1 conservativeReInit 0 negativeExampleCount 10 initialNegativeExampleCount 50
//                        randomExampleCount 50 negativeScoreThreshold -1.0 positiveOverlapThreshold 0.5 negativeOverlapThreshold 0.5
//                        adaptation position adaptationThreshold 0.75 exclusionThreshold 0.0
//                        classifier { training { c 1  compensateImbalance 0  negativeCapacity 100 }  logisticA 0.00556  logisticB -2.95  threshold 0 } }
//                        (training { type libLinear  c 1  bias 0  negativeCapacity 100 }: a liblinear::LibLinearClassifier; type libSvm is the default)
//     measurement positionDependent { feature grayscale|h|whi|hog|ehog|lbp|glbp { ... }  filter none  startFrameCount 1 ...  classifier { training { ... } } }
//                        (filter before|after { classifierFile .. feature .. { ... } }: an RVM in front of / behind the adaptive classifier)
//                        (in place of `measurement ehog`: a condensation::PositionDependentMeasurementModel, keys in tracking_setup.hpp; the
//                         AdaptiveCondensationTracker initialises its model once, so startFrameCount must be 1 for it to start; its generator gets seed + 4)
//     measurement wvmSvm { firstClassifier { classifierFile <FDWVM1 file> }  secondClassifier { classifierFile <SVM text file> threshold 0 }
//                          patch { width 20 height 20 minWidth 80 maxWidth 480 octaveLayerCount 5 } }
//                        (in place of `measurement ehog`: the reference's face tracker, FaceTracking.cpp:73-129 -- a CondensationTracker on
//                         condensation::WvmSvmModel; the classifier nodes are those of ffp_detect_app.  The sampler's minSize / maxSize default to
//                         the patch's minWidth / maxWidth.  This tracker has no initialisation: the box is not read, frame 0 is processed like
//                         every other frame and reported as "init <found> [x y w h]", and `adapted` is always 0)
//     validator rvm { classifierFile <FDRVM1 file> feature grayscale|h|whi { ... } sizes "0.9 1 1.1" displacements "-0.1 0 0.1" }
//                        (optional: a ClassificationBasedStateValidator on the tracker; keys in tracking_setup.hpp)
//   }
// the box is the target's bounding box (top left corner) in frame 0.  Prints "init <0|1> [x y w h]", then per further frame
//   "frame <f> found <0|1> <x> <y> <w> <h> adapted <0|1> route <generic|device> ms <wall time of process()>"
// With `transition opticalFlow` every frame line is followed by "flow <0|1> tracked <0|1> valid <n> correct <m> motion <x> <y> <ratio>": whether
// the flow (1) or the fallback (0) predicted the frame, whether points were tracked at all, the pairs tracked both ways, those of them
// that count as correct, and the median flow (%.9g).  With --dump the draws of the transition model follow it: "z <zx> <zy> <zsize>" per
// resampled sample on a flow frame (the normal draws), "d ..." as below on a fallback frame.
// With --dump every frame is followed by "draws u <0|1> <u> copies <n> fresh <m>", one "d <dx> <dy> <factor>" per copy, one "f <x> <y>
// <size>" per random sample, "samples <n>" and one "s <x> <y> <size> <vx> <vy> <vsize> <weight> <score> <target> <clusterId>" per sample
// (%.17g / %.9g: the values round-trip), so that tests/condensation_model.py can replay the run.
// With --counts (before --dump) a last line "evaluations fused <n> loop <m>" reports, for `measurement positionDependent` on a
// SingleClassifierModel, how many batched evaluations scored their samples in device calls and how many in the per-sample loop; for
// `measurement wvmSvm` the batched evaluations (frame 0 included) and the calls of the single-sample evaluate.
// With --adaptation (behind --counts, before --dump; `measurement ehog` and `positionDependent`) every frame line is followed by
// "adaptation <0|1> materialized <0|1>": whether the model adapted, and whether process() left the generation as Sample objects (always
// on the generic route; on the device route only where a validator or the model's adapt had to read them -- the line is printed before
// --dump asks for the samples).  For an adapted frame of `measurement positionDependent` the record of the adaptation follows:
// "positives <n>", "negatives <n>" and "testNegatives <n>", each followed by its samples as "ap|an|at <x> <y> <size>".
//   tracker_app --selftest <seed> <frames> <count> <randomRate>
// runs the samplers, the transition model and the extractors without a device: a CondensationTracker on a stub measurement model that
// weighs a sample by its distance to a moving point, on 64 x 48 frames; it dumps every frame as above, and the GridSampler's samples.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include "condensation/AdaptiveCondensationTracker.hpp"
#include "condensation/CondensationTracker.hpp"
#include "condensation/OpticalFlowTransitionModel.hpp"
#include "liblinear/LibLinearClassifier.hpp"
#include "libsvm/LibSvmClassifier.hpp"
#include "fdcompat/ptree.hpp"
#include "tracking_setup.hpp"

using namespace imageprocessing;
using namespace classification;
using namespace condensation;
using boost::property_tree::ptree;
using std::make_shared;
using std::shared_ptr;
using std::string;

static cv::Mat read_pnm(const string& path) {
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f.is_open()) throw std::runtime_error("cannot open image " + path);
    string magic;
    int w, h, maxv;
    f >> magic >> w >> h >> maxv;
    f.get();
    if ((magic != "P5" && magic != "P6") || maxv != 255) throw std::runtime_error("only binary PGM/PPM with maxval 255 are supported");
    const int ch = magic == "P6" ? 3 : 1;
    cv::Mat img(h, w, CV_MAKETYPE(CV_8U, ch));
    f.read((char*)img.data, (size_t)w * h * ch);
    if (ch == 3)
        for (size_t i = 0; i < (size_t)w * h; ++i) std::swap(img.data[3 * i], img.data[3 * i + 2]);
    return img;
}

// a subclass that changes nothing: the device route restates the class itself and must leave any subclass to the generic route
struct SubclassedFlowModel : public OpticalFlowTransitionModel {
    using OpticalFlowTransitionModel::OpticalFlowTransitionModel;
};

// the optical-flow transition model of a sampler, if it has one
static shared_ptr<OpticalFlowTransitionModel> flow_model(const shared_ptr<Sampler>& sampler) {
    auto resampling = std::dynamic_pointer_cast<ResamplingSampler>(sampler);
    return resampling ? std::dynamic_pointer_cast<OpticalFlowTransitionModel>(resampling->getTransitionModel()) : nullptr;
}

static void print_flow(const OpticalFlowTransitionModel& flow) {
    const fd_flow_motion& m = flow.getLastMotion();
    std::printf("flow %d tracked %d valid %d correct %d motion %.9g %.9g %.9g\n", flow.usedFlow() ? 1 : 0, flow.getPoints().empty() ? 0 : 1, m.n_valid, m.n_correct,
                m.median_x, m.median_y, m.median_ratio);
}

static void dump(const shared_ptr<Sampler>& sampler, const std::vector<shared_ptr<Sample>>& samples) {
    if (auto resampling = std::dynamic_pointer_cast<ResamplingSampler>(sampler)) {
        const ResamplingSampler::Draws& d = resampling->getLastDraws();
        if (auto flow = flow_model(sampler)) {   // the sampler does not know this model's draws: the copies are what is not fresh
            auto simple = std::dynamic_pointer_cast<SimpleTransitionModel>(flow->getFallback());
            const std::vector<double> none;
            const std::vector<double>& t = flow->usedFlow() ? flow->getLastDraws() : (simple ? simple->getLastDiffusion() : none);
            std::printf("draws u %d %.17g copies %zu fresh %zu\n", d.hasU ? 1 : 0, d.u, samples.size() - d.fresh.size() / 3, d.fresh.size() / 3);
            for (size_t i = 0; i + 2 < t.size(); i += 3) std::printf("%s %.17g %.17g %.17g\n", flow->usedFlow() ? "z" : "d", t[i], t[i + 1], t[i + 2]);
        } else {
            std::printf("draws u %d %.17g copies %zu fresh %zu\n", d.hasU ? 1 : 0, d.u, d.diffusion.size() / 3, d.fresh.size() / 3);
            for (size_t i = 0; i + 2 < d.diffusion.size(); i += 3) std::printf("d %.17g %.17g %.17g\n", d.diffusion[i], d.diffusion[i + 1], d.diffusion[i + 2]);
        }
        for (size_t i = 0; i + 2 < d.fresh.size(); i += 3) std::printf("f %d %d %d\n", d.fresh[i], d.fresh[i + 1], d.fresh[i + 2]);
    }
    std::printf("samples %zu\n", samples.size());
    for (const auto& s : samples)
        std::printf("s %d %d %d %d %d %.9g %.17g %.17g %d %d\n", s->getX(), s->getY(), s->getSize(), s->getVx(), s->getVy(), s->getVSize(), s->getWeight(),
                    s->getScore(), s->isTarget() ? 1 : 0, s->getClusterId());
}

// weight = 1 / (1 + squared distance to a point that moves with the frames), target when closer than 12 pixels; no device involved
struct StubModel : public MeasurementModel {
    using MeasurementModel::evaluate;
    int frame = 0;
    void update(shared_ptr<VersionedImage>) override { ++frame; }
    void evaluate(Sample& sample) const override {
        const double dx = sample.getX() - (20 + 2 * frame), dy = sample.getY() - (16 + frame);
        const double d2 = dx * dx + dy * dy;
        sample.setScore(-d2);
        sample.setWeight(sample.getWeight() * (1.0 / (1.0 + d2)));
        sample.setTarget(d2 < 144);
    }
};

static void print_frame(int f, const boost::optional<cv::Rect>& found, bool adapted, ParticleFrameLoop::Route route, double ms) {
    const cv::Rect r = found ? *found : cv::Rect();
    std::printf("frame %d found %d %d %d %d %d adapted %d route %s ms %.3f\n", f, found ? 1 : 0, r.x, r.y, r.width, r.height, adapted ? 1 : 0,
                route == ParticleFrameLoop::Route::DEVICE ? "device" : "generic", ms);
}

// --adaptation: what the frame's adapt did, and for PositionDependentMeasurementModel the samples it chose
static void print_adaptation(bool adapted, bool materialized, const PositionDependentMeasurementModel* dependent) {
    std::printf("adaptation %d materialized %d\n", adapted ? 1 : 0, materialized ? 1 : 0);
    if (!adapted || !dependent) return;
    const PositionDependentMeasurementModel::AdaptationRecord& r = dependent->getLastAdaptation();
    auto list = [](const char* name, const char* tag, const std::vector<cv::Rect>& rects) {
        std::printf("%s %zu\n", name, rects.size());
        for (const cv::Rect& s : rects) std::printf("%s %d %d %d\n", tag, s.x, s.y, s.width);
    };
    list("positives", "ap", r.positives);
    list("negatives", "an", r.negatives);
    list("testNegatives", "at", r.testNegatives);
}

// `measurement wvmSvm`: the face tracker's graph (FaceTracking.cpp:73-129) over the frames argv[first ..]
static int track_wvm_svm(const ptree& pt, const shared_ptr<TransitionModel>& transitionModel, unsigned seed, bool counting, bool dumping, int first, int argc,
                         char** argv) {
    const tracking_setup::WvmSvmSetup setup = tracking_setup::createWvmSvm(pt.get_child("measurement"));
    auto sampler = make_shared<ResamplingSampler>(pt.get("adaptive.resampling.particleCount", 800), pt.get("adaptive.resampling.randomRate", 0.35),
                                                  make_shared<LowVarianceSampling>(seed), transitionModel, pt.get("adaptive.resampling.minSize", setup.minWidth),
                                                  pt.get("adaptive.resampling.maxSize", setup.maxWidth), seed + 2);
    CondensationTracker tracker(sampler, setup.model, make_shared<FilteringStateExtractor>(make_shared<WeightedMeanStateExtractor>()));
    for (int f = first; f < argc; ++f) {
        const cv::Mat frame = read_pnm(argv[f]);
        if (f == first) sampler->init(frame);
        const auto t0 = std::chrono::steady_clock::now();
        boost::optional<cv::Rect> found = tracker.process(frame);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (f == first) {
            if (found) std::printf("init 1 %d %d %d %d\n", found->x, found->y, found->width, found->height);
            else std::printf("init 0\n");
            continue;
        }
        print_frame(f - first, found, false, tracker.getLastRoute(), ms);
        if (auto flow = flow_model(tracker.getSampler())) print_flow(*flow);
        if (dumping) dump(tracker.getSampler(), tracker.getSamples());
    }
    if (counting) std::printf("evaluations fused %d loop %d\n", setup.model->getFusedEvaluationCount(), setup.model->getLoopEvaluationCount());
    return 0;
}

// `tracker partiallyAdaptive`: the graph of the reference's partiallyAdaptiveTrackingApp -- WvmSvmModel until the self-learning model,
// bootstrapped from its samples, is usable -- over the frames argv[first ..].  The frame line gains `model <static|adaptive>`; with
// --adaptation the chosen examples follow as `sp|sn <index> <x> <y> <size> <valid>`
static int track_partially_adaptive(const ptree& pt, const shared_ptr<TransitionModel>& transitionModel, unsigned seed, bool adaptation, bool dumping, int first,
                                    int argc, char** argv) {
    if (pt.get("measurement", string("")) != "wvmSvm") throw std::invalid_argument("tracker_app: `tracker partiallyAdaptive` needs `measurement wvmSvm` as its static model");
    if (pt.get("adaptive", string("")) != "selfLearning")
        throw std::invalid_argument("tracker_app: `tracker partiallyAdaptive` needs `adaptive selfLearning { .. }` as its adaptive model");
    if (std::dynamic_pointer_cast<OpticalFlowTransitionModel>(transitionModel))
        throw std::invalid_argument("tracker_app: `transition opticalFlow` is not built under `tracker partiallyAdaptive`");
    const tracking_setup::WvmSvmSetup setup = tracking_setup::createWvmSvm(pt.get_child("measurement"));
    shared_ptr<SelfLearningMeasurementModel> adaptive = tracking_setup::createSelfLearning(pt.get_child("adaptive"));
    auto sampler = make_shared<ResamplingSampler>(pt.get("adaptive.resampling.particleCount", 800), pt.get("adaptive.resampling.randomRate", 0.35),
                                                  make_shared<LowVarianceSampling>(seed), transitionModel, pt.get("adaptive.resampling.minSize", setup.minWidth),
                                                  pt.get("adaptive.resampling.maxSize", setup.maxWidth), seed + 2);
    PartiallyAdaptiveCondensationTracker tracker(sampler, setup.model, adaptive, make_shared<FilteringStateExtractor>(make_shared<WeightedMeanStateExtractor>()));
    for (int f = first; f < argc; ++f) {
        const cv::Mat frame = read_pnm(argv[f]);
        if (f == first) sampler->init(frame);
        const bool wasUsable = adaptive->isUsable();
        const auto t0 = std::chrono::steady_clock::now();
        boost::optional<cv::Rect> found = tracker.process(frame);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const bool materialized = tracker.samplesMaterialized();   // before anything below asks for the samples
        const cv::Rect r = found ? *found : cv::Rect();
        std::printf("frame %d found %d %d %d %d %d adapted %d route %s model %s ms %.3f\n", f - first, found ? 1 : 0, r.x, r.y, r.width, r.height,
                    adaptive->isUsable() ? 1 : 0, tracker.getLastRoute() == ParticleFrameLoop::Route::DEVICE ? "device" : "generic",
                    tracker.hasUsedAdaptiveModel() ? "adaptive" : "static", ms);
        if (adaptation) {
            std::printf("adaptation %d materialized %d usable %d positives %zu negatives %zu\n", wasUsable ? 1 : 0, materialized ? 1 : 0, adaptive->isUsable() ? 1 : 0,
                        adaptive->getLastPositives().size(), adaptive->getLastNegatives().size());
            for (const fd_particles_example& e : adaptive->getLastPositives()) std::printf("sp %d %d %d %d %d\n", e.index, e.x, e.y, e.size, e.valid);
            for (const fd_particles_example& e : adaptive->getLastNegatives()) std::printf("sn %d %d %d %d %d\n", e.index, e.x, e.y, e.size, e.valid);
        }
        if (dumping) dump(tracker.getSampler(), tracker.getSamples());
    }
    return 0;
}

static int selftest(int argc, char** argv) {
    if (argc < 6) return 2;
    const unsigned seed = (unsigned)std::atoi(argv[2]);
    const int frames = std::atoi(argv[3]), count = std::atoi(argv[4]);
    const double randomRate = std::atof(argv[5]);
    cv::Mat image(48, 64, CV_8UC1);
    std::memset(image.data, 0, 48 * 64);
    Sample::setAspectRatio(1.0);
    auto sampler = make_shared<ResamplingSampler>(count, randomRate, make_shared<LowVarianceSampling>(seed), make_shared<SimpleTransitionModel>(3.0, 0.1, seed + 1),
                                                  8, 80, seed + 2);
    sampler->init(image);
    CondensationTracker tracker(sampler, make_shared<StubModel>(), make_shared<FilteringStateExtractor>(make_shared<WeightedMeanStateExtractor>()));
    MaxWeightStateExtractor maxWeight;
    for (int f = 0; f < frames; ++f) {
        boost::optional<cv::Rect> box = tracker.process(image);
        shared_ptr<Sample> s = tracker.getState();
        if (s) std::printf("frame %d found 1 %d %d %d %d %d %.9g route generic\n", f, s->getX(), s->getY(), s->getSize(), s->getVx(), s->getVy(), s->getVSize());
        else std::printf("frame %d found 0 route generic\n", f);
        shared_ptr<Sample> m = maxWeight.extract(tracker.getSamples());
        if (m) std::printf("max 1 %d %d %d\n", m->getX(), m->getY(), m->getSize());
        else std::printf("max 0\n");
        dump(sampler, tracker.getSamples());
        if (box && s && (box->width != s->getWidth() || box->x != s->getX() - s->getWidth() / 2)) return 1;
    }
    GridSampler grid(10, 40, 1.5f, 0.25f);
    std::vector<shared_ptr<Sample>> none, cells;
    grid.sample(none, cells, image, shared_ptr<Sample>());
    std::printf("grid %zu\n", cells.size());
    for (const auto& s : cells) std::printf("g %d %d %d\n", s->getX(), s->getY(), s->getSize());
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc > 1 && string(argv[1]) == "--selftest") return selftest(argc, argv);
        const bool counting = argc > 1 && string(argv[1]) == "--counts";
        const int afterCounts = counting ? 2 : 1;
        const bool adaptation = argc > afterCounts && string(argv[afterCounts]) == "--adaptation";
        const int afterAdaptation = afterCounts + (adaptation ? 1 : 0);
        const bool dumping = argc > afterAdaptation && string(argv[afterAdaptation]) == "--dump";
        const int a = afterAdaptation + (dumping ? 1 : 0);
        if (argc < a + 6) {
            std::fprintf(stderr, "usage: %s [--counts] [--adaptation] [--dump] <config.cfg> <x> <y> <width> <height> <frame0> [<frame1> ...]\n", argv[0]);
            return 2;
        }
        ptree all;
        boost::property_tree::read_info(string(argv[a]), all);
        const ptree& pt = all.get_child("tracking");
        const unsigned seed = (unsigned)pt.get("seed", 1);
        const string transition = pt.get("transition", string("simple"));
        shared_ptr<TransitionModel> transitionModel;
        if (transition == "simple") {
            transitionModel = make_shared<SimpleTransitionModel>(pt.get("transition.positionDeviation", 10.0), pt.get("transition.sizeDeviation", 0.1), seed + 1);
        } else if (transition == "opticalFlow") {   // HeadTracking.cpp:545-550
            if (pt.get("transition.fallback", string("simple")) != "simple") throw std::invalid_argument("tracker_app: only `fallback simple` is supported");
            auto fallback = make_shared<SimpleTransitionModel>(pt.get("transition.fallback.positionDeviation", 12.8), pt.get("transition.fallback.sizeDeviation", 0.1), seed + 1);
            // gridSize (default 10) and subclass (default 0: the class itself) are not the reference's keys: they let a test build the
            // configurations that must keep the generic route under FD_COND_DEVICE=1
            const int grid = pt.get("transition.gridSize", 10);
            const double positionDeviation = pt.get("transition.positionDeviation", 10.0), sizeDeviation = pt.get("transition.sizeDeviation", 0.08);
            if (pt.get("transition.subclass", 0) != 0)
                transitionModel = make_shared<SubclassedFlowModel>(fallback, positionDeviation, sizeDeviation, cv::Size(grid, grid), true, cv::Size(15, 15), 2, seed + 3);
            else
                transitionModel = make_shared<OpticalFlowTransitionModel>(fallback, positionDeviation, sizeDeviation, cv::Size(grid, grid), true, cv::Size(15, 15), 2,
                                                                          seed + 3);
        } else {
            throw std::invalid_argument("tracker_app: invalid transition model type: " + transition);
        }
        const string trackerType = pt.get("tracker", string("adaptive"));
        if (trackerType == "partiallyAdaptive") return track_partially_adaptive(pt, transitionModel, seed, adaptation, dumping, a + 5, argc, argv);
        if (trackerType != "adaptive") throw std::invalid_argument("tracker_app: invalid tracker type: " + trackerType + " (adaptive and partiallyAdaptive are supported)");
        const string measurement = pt.get("measurement", string("ehog"));
        if (measurement != "ehog" && measurement != "positionDependent" && measurement != "wvmSvm")
            throw std::invalid_argument("tracker_app: invalid measurement model type: " + measurement + " (ehog, positionDependent and wvmSvm are supported)");
        if (measurement == "wvmSvm") return track_wvm_svm(pt, transitionModel, seed, counting, dumping, a + 5, argc, argv);
        shared_ptr<Sampler> sampler;
        if (pt.count("grid"))
            sampler = make_shared<GridSampler>(pt.get("grid.minSize", 20), pt.get("grid.maxSize", 80), (float)pt.get("grid.sizeScale", 1.2), (float)pt.get("grid.stepSize", 0.1));
        else
            sampler = make_shared<ResamplingSampler>(pt.get("adaptive.resampling.particleCount", 800), pt.get("adaptive.resampling.randomRate", 0.35),
                                                     make_shared<LowVarianceSampling>(seed), transitionModel,
                                                     pt.get("adaptive.resampling.minSize", 40), pt.get("adaptive.resampling.maxSize", 200), seed + 2);
        const ptree& mt = pt.get_child("measurement");
        const ptree& ct = mt.get_child("classifier");
        shared_ptr<AdaptiveMeasurementModel> adaptiveModel;
        shared_ptr<ExtendedHogBasedMeasurementModel> model;
        if (measurement == "positionDependent") {
            adaptiveModel = tracking_setup::createPositionDependent(mt, seed + 4).model;
        } else if (ct.count("training")) {
            shared_ptr<TrainableSvmClassifier> svm = tracking_setup::createTrainableSvm(ct);
            model = make_shared<ExtendedHogBasedMeasurementModel>(
                make_shared<FixedTrainableProbabilisticSvmClassifier>(svm, ct.get("logisticA", 0.00556), ct.get("logisticB", -2.95)));
        } else {
            model = make_shared<ExtendedHogBasedMeasurementModel>(ProbabilisticSvmClassifier::load(ct));
        }
        if (model) {
            adaptiveModel = model;
            model->setHogParams(mt.get("cellSize", 5), mt.get("cellCount", 35), mt.get("signedAndUnsigned", 0) != 0, mt.get("interpolateBins", 0) != 0,
                                mt.get("interpolateCells", 1) != 0, mt.get("octaveLayerCount", 5));
            model->setRejectionThreshold(mt.get("rejectionThreshold", -1.5));
            model->setUseSlidingWindow(mt.get("useSlidingWindow", 1) != 0, mt.get("conservativeReInit", 0) != 0);
            model->setNegativeExampleParams(mt.get("negativeExampleCount", 10), mt.get("initialNegativeExampleCount", 50), mt.get("randomExampleCount", 50),
                                            (float)mt.get("negativeScoreThreshold", -1.0));
            model->setOverlapThresholds(mt.get("positiveOverlapThreshold", 0.5), mt.get("negativeOverlapThreshold", 0.5));
            const string adaptation = mt.get("adaptation", string("position"));
            model->setAdaptation(adaptation == "none" ? ExtendedHogBasedMeasurementModel::Adaptation::NONE
                                 : adaptation == "trajectory" ? ExtendedHogBasedMeasurementModel::Adaptation::TRAJECTORY
                                                              : ExtendedHogBasedMeasurementModel::Adaptation::POSITION,
                                 mt.get("adaptationThreshold", 0.75), mt.get("exclusionThreshold", 0.0));
        }
        AdaptiveCondensationTracker tracker(sampler, adaptiveModel, make_shared<FilteringStateExtractor>(make_shared<WeightedMeanStateExtractor>()),
                                            pt.get("initialCount", 800));
        if (auto validator = tracking_setup::createValidator(pt)) tracker.addValidator(validator);
        const cv::Rect box(std::atoi(argv[a + 1]), std::atoi(argv[a + 2]), std::atoi(argv[a + 3]), std::atoi(argv[a + 4]));
        boost::optional<cv::Rect> start = tracker.initialize(read_pnm(argv[a + 5]), box);
        if (!start) {
            std::printf("init 0\n");
            return 1;
        }
        std::printf("init 1 %d %d %d %d\n", start->x, start->y, start->width, start->height);
        for (int f = a + 6; f < argc; ++f) {
            const cv::Mat frame = read_pnm(argv[f]);
            const auto t0 = std::chrono::steady_clock::now();
            boost::optional<cv::Rect> found = tracker.process(frame);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            const bool materialized = tracker.samplesMaterialized();   // before anything below asks for the samples
            print_frame(f - a - 5, found, tracker.hasAdapted(), tracker.getLastRoute(), ms);
            if (adaptation) print_adaptation(tracker.hasAdapted(), materialized, std::dynamic_pointer_cast<PositionDependentMeasurementModel>(adaptiveModel).get());
            if (auto flow = flow_model(tracker.getSampler())) print_flow(*flow);
            if (dumping) dump(tracker.getSampler(), tracker.getSamples());
        }
        if (counting) {
            auto dependent = std::dynamic_pointer_cast<PositionDependentMeasurementModel>(adaptiveModel);
            auto single = dependent ? std::dynamic_pointer_cast<SingleClassifierModel>(dependent->getMeasurementModel()) : nullptr;
            if (single) std::printf("evaluations fused %d loop %d\n", single->getFusedEvaluationCount(), single->getLoopEvaluationCount());
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "tracker_app: %s\n", e.what());
        return 1;
    }
}
