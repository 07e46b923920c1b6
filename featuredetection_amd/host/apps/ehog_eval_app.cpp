// ehog_eval_app -- the measurement step of the reference's trackers with a condensation::ExtendedHogBasedMeasurementModel
// (headTrackingApp, adaptiveTrackingApp, trackingBenchmarkApp): initialises the model on a target, then scores a list of samples on one
// frame and reports the heat peak and the good negative examples.
//   usage: ehog_eval_app <config.cfg> <image.ppm|pgm> <samples.txt>
// config (boost info format):
//   target { x <cx> y <cy> width <w> height <h> }     the target the model is initialised on: its aspect ratio fixes the cell grid
//   classifier { classifierFile <SVM text file: LinearKernel, one support vector of rows * cols * channels values> [threshold t] [logisticA a logisticB b] }
//   hog { cellSize 5  cellCount 35  signedAndUnsigned 0  interpolateBins 0  interpolateCells 1  octaveLayerCount 5 }         (optional)
//   rejectionThreshold -1.5   useSlidingWindow 1   conservativeReInit 0   negativeScoreThreshold -1.0                      (optional)
//   positiveOverlapThreshold 0.5   negativeOverlapThreshold 0.5   adaptationThreshold 0.75                                  (optional)
//   targetLost 0|1                                    1: adapt(image, samples) is called before the evaluation (the target was lost)
// Training mode: when the classifier block has a `training` child
//   classifier { training { c 1  compensateImbalance 0  negativeCapacity 100 } [logisticA a logisticB b] }
// the model is built on a libsvm::LibSvmClassifier (LinearKernel; unlimited positives, age-based negatives of that capacity) behind a
// FixedTrainableProbabilisticSvmClassifier, further frames may follow the samples file
//   usage: ehog_eval_app <config.cfg> <frame0> <samples.txt> [<frame1> ...]
// and the app runs initialize on frame 0, then per further frame update, evaluate (a copy of the samples) and adapt(image, samples,
// target) with the configured target; `adaptation none|position|trajectory` and `exclusionThreshold` are read too.  Per frame it prints
// "frame <f> usable <0|1> adapted <0|1>", per retraining "train pos <n> neg <m>" followed by one "p <x> <y> <w> <h>" per positive sample
// (centre form) and one "n <x> <y> <w> <h>" per negative's bounds, then "info <iterations> <converged> <n_sv> <n_bounded> <rho>" and
// "w <all weights>" of the classifier; the single-frame output below follows for the last frame.
// samples.txt: one "x y size" per line (width = size, height = cvRound(rows / cols * size)).
// Prints  "grid <cols> <rows>", per sample "<target 0|1> <score> <weight> <x> <y> <size> <clusterId>" (position and size after the
// evaluation: a re-initialisation moves the samples), "peak <score> <x> <y> <w> <h>", "negatives <n>" and one "<x> <y> <w> <h>" per
// example; on stderr the number of fused device calls the batched evaluation made.
#include <cstdio>
#include <fstream>
#include <iostream>
#include "condensation/ExtendedHogBasedMeasurementModel.hpp"
#include "libsvm/LibSvmClassifier.hpp"
#include "fdcompat/ptree.hpp"

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

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <config.cfg> <image.ppm|pgm> <samples.txt>\n", argv[0]);
        return 2;
    }
    try {
        ptree pt;
        boost::property_tree::read_info(string(argv[1]), pt);
        const bool training = pt.get_child("classifier").count("training") > 0;
        shared_ptr<libsvm::LibSvmClassifier> trainedSvm;
        std::unique_ptr<ExtendedHogBasedMeasurementModel> modelPtr;
        if (training) {
            const ptree& tr = pt.get_child("classifier.training");
            trainedSvm = libsvm::LibSvmClassifier::createBinarySvm(make_shared<LinearKernel>(), tr.get("c", 1.0), tr.get("compensateImbalance", 0) != 0);
            trainedSvm->setNegativeExampleManagement(std::unique_ptr<ExampleManagement>(new AgeBasedExampleManagement(tr.get("negativeCapacity", 100))));
            modelPtr.reset(new ExtendedHogBasedMeasurementModel(make_shared<FixedTrainableProbabilisticSvmClassifier>(
                trainedSvm, pt.get("classifier.logisticA", 0.00556), pt.get("classifier.logisticB", -2.95))));
        } else {
            modelPtr.reset(new ExtendedHogBasedMeasurementModel(ProbabilisticSvmClassifier::load(pt.get_child("classifier"))));
        }
        ExtendedHogBasedMeasurementModel& model = *modelPtr;
        model.setHogParams(pt.get("hog.cellSize", 5), pt.get("hog.cellCount", 35), pt.get("hog.signedAndUnsigned", 0) != 0,
                           pt.get("hog.interpolateBins", 0) != 0, pt.get("hog.interpolateCells", 1) != 0, pt.get("hog.octaveLayerCount", 5));
        model.setRejectionThreshold(pt.get("rejectionThreshold", -1.5));
        model.setUseSlidingWindow(pt.get("useSlidingWindow", 1) != 0, pt.get("conservativeReInit", 0) != 0);
        model.setNegativeExampleParams(10, 50, 50, (float)pt.get("negativeScoreThreshold", -1.0));
        model.setOverlapThresholds(pt.get("positiveOverlapThreshold", 0.5), pt.get("negativeOverlapThreshold", 0.5));
        const string adaptation = pt.get("adaptation", string("position"));
        model.setAdaptation(adaptation == "none" ? ExtendedHogBasedMeasurementModel::Adaptation::NONE
                            : adaptation == "trajectory" ? ExtendedHogBasedMeasurementModel::Adaptation::TRAJECTORY
                                                         : ExtendedHogBasedMeasurementModel::Adaptation::POSITION,
                            pt.get("adaptationThreshold", 0.75), pt.get("exclusionThreshold", 0.0));
        auto image = make_shared<VersionedImage>(read_pnm(argv[2]));
        // the target: a sample whose height follows from the aspect ratio, as the trackers create it from the initial bounding box
        const int tw = pt.get<int>("target.width"), th = pt.get<int>("target.height");
        Sample::setAspectRatio(tw, th);
        Sample target(pt.get<int>("target.x"), pt.get<int>("target.y"), tw);
        if (!model.initialize(image, target)) throw std::runtime_error("the target has no patch in the image");
        std::printf("grid %zu %zu\n", model.getCellColumnCount(), model.getCellRowCount());
        std::vector<shared_ptr<Sample>> samples;
        std::ifstream sf(argv[3]);
        if (!sf.is_open()) throw std::runtime_error(string("cannot open samples ") + argv[3]);
        int x, y, size;
        while (sf >> x >> y >> size) samples.push_back(make_shared<Sample>(x, y, size));
        if (training) {
            size_t logged = 0;
            auto report = [&](int frame, bool adapted) {
                std::printf("frame %d usable %d adapted %d\n", frame, model.isUsable() ? 1 : 0, adapted ? 1 : 0);
                const auto& log = model.getTrainingLog();
                for (; logged < log.size(); ++logged) {
                    std::printf("train pos %zu neg %zu\n", log[logged].positives.size(), log[logged].negatives.size());
                    for (const cv::Rect& r : log[logged].positives) std::printf("p %d %d %d %d\n", r.x, r.y, r.width, r.height);
                    for (const cv::Rect& r : log[logged].negatives) std::printf("n %d %d %d %d\n", r.x, r.y, r.width, r.height);
                }
                const fd_svm_train_info& info = trainedSvm->getLastTrainingInfo();
                std::printf("info %d %d %d %d %.17g\nw", info.iterations, info.converged, info.n_sv, info.n_bounded, info.rho);
                const auto& sv = trainedSvm->getSvm()->getSupportVectors();
                if (!sv.empty())
                    for (size_t k = 0; k < sv[0].total(); ++k) std::printf(" %.9g", sv[0].ptr<float>(0)[k]);
                std::printf("\n");
            };
            report(0, true);
            for (int f = 4; f < argc; ++f) {
                image = make_shared<VersionedImage>(read_pnm(argv[f]));
                model.update(image);
                std::vector<shared_ptr<Sample>> copy;
                for (const auto& s : samples) copy.push_back(make_shared<Sample>(s->getX(), s->getY(), s->getSize()));
                model.evaluate(image, copy);
                report(f - 3, model.adapt(image, copy, target));
            }
        }
        if (pt.get("targetLost", 0) != 0) model.adapt(image, samples);
        model.evaluate(image, samples);
        std::fprintf(stderr, "%zu samples: %d fused device call(s)\n", samples.size(), model.getFusedEvaluationCount());
        for (const auto& s : samples)
            std::printf("%d %.9g %.17g %d %d %d %d\n", s->isTarget() ? 1 : 0, s->getScore(), s->getWeight(), s->getX(), s->getY(), s->getSize(), s->getClusterId());
        if (pt.get("useSlidingWindow", 1) != 0) {
            std::pair<double, cv::Rect> peak = model.getHeatPeak();
            std::printf("peak %.9g %d %d %d %d\n", peak.first, peak.second.x, peak.second.y, peak.second.width, peak.second.height);
            std::vector<cv::Rect> bounds;
            std::vector<cv::Mat> negatives = model.createGoodNegativeExamples(target.getBounds(), &bounds);
            std::printf("negatives %zu\n", negatives.size());
            for (const cv::Rect& b : bounds) std::printf("%d %d %d %d\n", b.x, b.y, b.width, b.height);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
