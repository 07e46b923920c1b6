// position_dependent_eval_app -- condensation::PositionDependentMeasurementModel frame by frame on given targets and particles, so that a
// test can follow every choice it makes.
//   usage: position_dependent_eval_app <config.cfg> <script.txt>
// config (boost info format): tracking { seed 1  measurement positionDependent { ... } }, the keys of tracking_setup.hpp.  Two more keys
// are read beside them: `wrapped 1` puts the feature extractor behind a PatchResizingFeatureExtractor(extractor, 1.0) for the model and its
// SingleClassifierModel (the per-sample routes), `printVectors 1` prints the positive vectors of every retraining.
// script (plain text), per frame:
//   frame <image.pgm|ppm> <targetX> <targetY> <targetSize> <particleCount>      (targetSize 0: no target in this frame)
//   <x> <y> <size>                                                              (particleCount lines)
// Per frame the app evaluates the particles (when the model is usable), adapts the model and prints
//   frame <f> usable_before <0|1> evaluated <0|1> fused <n> loop <n>
//   e <target 0|1> <weight %.17g>                                               (per particle, after evaluate; the weight is 1 before the model is usable)
//   adapt <return value 0|1> usable <0|1> retrained <0|1>
//   positives <n> / negatives <n> / tests <n>, each followed by n lines "s <x> <y> <size>"   (when a retraining was reached)
//   vectors <positive vectors> <negative vectors>
//   pv <rows> <cols> <values %.9g ...>                                         (with `printVectors 1`: every positive vector passed to retrain, row-major)
//   svm <supportVectors> <dimension> bias <%.9g> threshold <%.9g> logistic <%.17g> <%.17g>, then per support vector
//   "sv <coefficient %.9g> <values %.9g ...>"                                   (the classifier after this frame; nothing while it has no vectors)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
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

static void print_samples(const char* name, const std::vector<cv::Rect>& samples) {
    std::printf("%s %zu\n", name, samples.size());
    for (const cv::Rect& s : samples) std::printf("s %d %d %d\n", s.x, s.y, s.width);
}

int main(int argc, char** argv) {
    try {
        if (argc != 3) {
            std::fprintf(stderr, "usage: %s <config.cfg> <script.txt>\n", argv[0]);
            return 2;
        }
        ptree all;
        boost::property_tree::read_info(string(argv[1]), all);
        const ptree& pt = all.get_child("tracking");
        if (pt.get("measurement", string()) != "positionDependent") throw std::invalid_argument("the config needs a `measurement positionDependent` block");
        const ptree& mt = pt.get_child("measurement");
        tracking_setup::PositionDependentSetup setup = tracking_setup::createPositionDependent(mt, (unsigned)pt.get("seed", 1));
        shared_ptr<PositionDependentMeasurementModel> model = setup.model;
        if (mt.get("wrapped", 0) != 0) {   // the same model on a wrapped extractor: per-sample extraction, SingleClassifierModel keeps its loop
            auto wrapped = make_shared<PatchResizingFeatureExtractor>(setup.featureExtractor, 1.0);
            model = make_shared<PositionDependentMeasurementModel>(make_shared<SingleClassifierModel>(wrapped, setup.classifier), wrapped,
                                                                   setup.classifier, (unsigned)pt.get("seed", 1));
            model->setFrameCounts(mt.get("startFrameCount", 3u), mt.get("stopFrameCount", 0u));
            model->setThresholds(mt.get("targetThreshold", 0.7f), mt.get("confidenceThreshold", 0.95f));
            model->setOffsetFactors(mt.get("positiveOffsetFactor", 0.05f), mt.get("negativeOffsetFactor", 0.5f));
            model->setSamplingProperties(mt.get("sampleNegativesAroundTarget", 0u), mt.get("sampleAdditionalNegatives", 10u), mt.get("sampleTestNegatives", 10u),
                                         tracking_setup::flag(mt, "exploitSymmetry"));
        }
        const bool printVectors = mt.get("printVectors", 0) != 0;
        auto single = std::dynamic_pointer_cast<SingleClassifierModel>(model->getMeasurementModel());
        std::ifstream script(argv[2]);
        if (!script.is_open()) throw std::runtime_error(string("cannot open ") + argv[2]);
        auto image = make_shared<VersionedImage>();
        string word, path;
        int frame = 0;
        while (script >> word) {
            if (word != "frame") throw std::runtime_error("script: expected `frame`, got " + word);
            int tx, ty, ts, count;
            if (!(script >> path >> tx >> ty >> ts >> count) || count < 0) throw std::runtime_error("script: bad frame line");
            std::vector<shared_ptr<Sample>> particles;
            for (int i = 0; i < count; ++i) {
                int x, y, size;
                if (!(script >> x >> y >> size)) throw std::runtime_error("script: bad particle line");
                particles.push_back(make_shared<Sample>(x, y, size));
            }
            image->setData(read_pnm(path));
            const bool usableBefore = model->isUsable();
            if (usableBefore) model->evaluate(image, particles);
            std::printf("frame %d usable_before %d evaluated %d fused %d loop %d\n", frame, usableBefore ? 1 : 0, usableBefore ? 1 : 0,
                        single ? single->getFusedEvaluationCount() : -1, single ? single->getLoopEvaluationCount() : -1);
            for (const auto& p : particles) std::printf("e %d %.17g\n", p->isTarget() ? 1 : 0, p->getWeight());
            const size_t logged = model->getAdaptationCount();
            bool adapted;
            if (ts > 0) adapted = model->adapt(image, particles, Sample(tx, ty, ts));
            else adapted = model->adapt(image, particles);
            const bool retrained = model->getAdaptationCount() > logged;
            std::printf("adapt %d usable %d retrained %d\n", adapted ? 1 : 0, model->isUsable() ? 1 : 0, retrained ? 1 : 0);
            if (retrained) {
                const PositionDependentMeasurementModel::AdaptationRecord& r = model->getLastAdaptation();
                print_samples("positives", r.positives);
                print_samples("negatives", r.negatives);
                print_samples("tests", r.testNegatives);
                std::printf("vectors %zu %zu\n", r.positiveVectors.size(), r.negativeVectors.size());
                if (printVectors)
                    for (const cv::Mat& v : r.positiveVectors) {
                        std::printf("pv %d %d", v.rows, v.cols);
                        for (int y = 0; y < v.rows; ++y)
                            for (int x = 0; x < v.cols; ++x) std::printf(" %.9g", (double)v.ptr<float>(y)[x]);
                        std::printf("\n");
                    }
            }
            const auto psvm = setup.classifier->getProbabilisticSvm();
            const auto& svs = psvm->getSvm()->getSupportVectors();
            if (!svs.empty()) {
                const size_t d = (size_t)svs[0].rows * svs[0].cols * svs[0].channels();
                std::printf("svm %zu %zu bias %.9g threshold %.9g logistic %.17g %.17g\n", svs.size(), d, (double)psvm->getSvm()->getBias(),
                            (double)psvm->getSvm()->getThreshold(), psvm->getLogisticA(), psvm->getLogisticB());
                for (size_t i = 0; i < svs.size(); ++i) {
                    std::printf("sv %.9g", (double)psvm->getSvm()->getCoefficients()[i]);
                    const float* v = svs[i].ptr<float>(0);
                    for (size_t k = 0; k < d; ++k) std::printf(" %.9g", (double)v[k]);
                    std::printf("\n");
                }
            }
            ++frame;
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "position_dependent_eval_app: %s\n", e.what());
        return 1;
    }
}
