// detector_training_app -- trains the linear SVM of an AggregatedFeaturesDetector from annotated images (the TRAIN task of the
// reference's DetectorTrainingApp) and writes it in the text format of SvmClassifier::store, which
// aggregated_detect_app reads.
//
//   detector_training_app train <images.lst> <features.cfg> <training.cfg> <out.svm> [--seed N] [--trace file]
//
// images.lst: one line per image, "image.pgm|ppm" followed by its boxes as "name x y width height" (top-left corner, pixels); a
//             name that starts with "ignore" marks a region that is neither positive nor negative
// features.cfg (INFO format, the keys of DetectorTrainingApp.cpp:236-258):
//   type fhog[N] | fpdw   windowWidthInCells ..  windowHeightInCells ..  cellSizeInPixels ..  octaveLayerCount ..
//   widthScaleFactor ..  heightScaleFactor ..
// training.cfg (:260-273):
//   mirrorTrainingData ..  maxNegatives ..  randomNegativesPerImage ..  maxHardNegativesPerImage ..  bootstrappingRounds ..
//   negativeScoreThreshold ..  overlapThreshold ..  C ..  compensateImbalance ..  probabilistic ..
// type fhog: image filter GrayscaleFilter, layer filter FhogFilter(cell, N, false, true, 0.2); type fpdw: no image filter, layer filter
// ChainedFilter(FpdwFeaturesFilter(true, false, cell, 0.01), AggregationFilter(cell, true, false)), BGR images only
// (DetectorTrainingApp.cpp:78-113).  --seed: the seed of the random negatives (default 5489).  --trace: the record of
// DetectorTrainer::setTrace.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include "detectortraining/DetectorTrainer.hpp"
#include "imageprocessing/filtering/AggregationFilter.hpp"
#include "imageprocessing/filtering/FhogFilter.hpp"
#include "imageprocessing/filtering/FpdwFeaturesFilter.hpp"
#include "fdcompat/ptree.hpp"

using namespace imageprocessing;
using boost::property_tree::ptree;
using imageprocessing::filtering::AggregationFilter;
using imageprocessing::filtering::FhogFilter;
using imageprocessing::filtering::FpdwFeaturesFilter;
using std::make_shared;
using std::shared_ptr;
using std::string;
using std::vector;

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
    if (ch == 3)  // PPM is RGB, the reference works on BGR
        for (size_t i = 0; i < (size_t)w * h; ++i) std::swap(img.data[3 * i], img.data[3 * i + 2]);
    return img;
}

// "true" / "false" / "1" / "0" (the INFO parser hands out strings)
static bool flag(const ptree& node, const string& key) {
    const string v = node.get<string>(key);
    if (v == "true" || v == "1") return true;
    if (v == "false" || v == "0") return false;
    throw std::invalid_argument("expected true/false for " + key + ", but was '" + v + "'");
}

static vector<LabeledImage> read_images(const string& path) {
    std::ifstream list(path.c_str());
    if (!list.is_open()) throw std::runtime_error("cannot open image list " + path);
    vector<LabeledImage> images;
    string line;
    while (std::getline(list, line)) {
        std::istringstream in(line);
        string file, name;
        if (!(in >> file)) continue;
        vector<imageio::RectLandmark> landmarks;
        while (in >> name) {
            int x, y, w, h;
            if (!(in >> x >> y >> w >> h)) throw std::invalid_argument("image list: expected 'name x y width height' after " + file);
            landmarks.emplace_back(name, cv::Rect(x, y, w, h));
        }
        images.emplace_back(read_pnm(file), landmarks);
    }
    return images;
}

int main(int argc, char** argv) {
    if (argc < 6 || string(argv[1]) != "train") {
        std::fprintf(stderr, "call: %s train images.lst features.cfg training.cfg out.svm [--seed N] [--trace file]\n", argv[0]);
        return 2;
    }
    try {
        unsigned int seed = 5489u;
        string tracePath;
        for (int a = 6; a < argc; ++a) {
            const string arg = argv[a];
            if (arg == "--seed" && a + 1 < argc) seed = (unsigned int)std::strtoul(argv[++a], nullptr, 10);
            else if (arg == "--trace" && a + 1 < argc) tracePath = argv[++a];
            else throw std::invalid_argument("unknown argument " + arg);
        }
        ptree fcfg, tcfg;
        boost::property_tree::read_info(string(argv[3]), fcfg);
        boost::property_tree::read_info(string(argv[4]), tcfg);
        FeatureParams fp;
        fp.windowSizeInCells = cv::Size(fcfg.get<int>("windowWidthInCells"), fcfg.get<int>("windowHeightInCells"));
        fp.cellSizeInPixels = fcfg.get<int>("cellSizeInPixels");
        fp.octaveLayerCount = fcfg.get<int>("octaveLayerCount");
        fp.widthScaleFactor = fcfg.get<float>("widthScaleFactor");
        fp.heightScaleFactor = fcfg.get<float>("heightScaleFactor");
        TrainingParams tp;
        tp.mirrorTrainingData = flag(tcfg, "mirrorTrainingData");
        tp.maxNegatives = tcfg.get<int>("maxNegatives");
        tp.randomNegativesPerImage = tcfg.get<int>("randomNegativesPerImage");
        tp.maxHardNegativesPerImage = tcfg.get<int>("maxHardNegativesPerImage");
        tp.bootstrappingRounds = tcfg.get<int>("bootstrappingRounds");
        tp.negativeScoreThreshold = tcfg.get<float>("negativeScoreThreshold");
        tp.overlapThreshold = tcfg.get<double>("overlapThreshold");
        tp.C = tcfg.get<double>("C");
        tp.compensateImbalance = flag(tcfg, "compensateImbalance");
        tp.probabilistic = flag(tcfg, "probabilistic");

        const string type = fcfg.get<string>("type");
        shared_ptr<ImageFilter> imageFilter, layerFilter;
        if (type.compare(0, 4, "fhog") == 0) {
            const int bins = type.size() > 4 ? std::stoi(type.substr(4)) : 9;
            imageFilter = make_shared<GrayscaleFilter>();
            layerFilter = make_shared<FhogFilter>(fp.cellSizeInPixels, bins, false, true, 0.2f);
        } else if (type == "fpdw") {
            auto chain = make_shared<ChainedFilter>();
            chain->add(make_shared<FpdwFeaturesFilter>(true, false, fp.cellSizeInPixels, 0.01));
            chain->add(make_shared<AggregationFilter>(fp.cellSizeInPixels, true, false));
            layerFilter = chain;
        } else {
            throw std::invalid_argument("expected fhog/fpdw, but was '" + type + "'");
        }

        const vector<LabeledImage> images = read_images(argv[2]);
        std::ofstream traceFile;
        DetectorTrainer trainer(true, "", seed);
        if (!tracePath.empty()) {
            traceFile.open(tracePath.c_str());
            if (!traceFile.is_open()) throw std::runtime_error("cannot write trace " + tracePath);
            trainer.setTrace(&traceFile);
        }
        trainer.setTrainingParameters(tp);
        trainer.setFeatures(fp, layerFilter, imageFilter);
        trainer.train(images);
        trainer.storeClassifier(argv[5]);
    } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "invalid argument: %s\n", e.what());
        return 1;
    } catch (const std::logic_error& e) {
        std::fprintf(stderr, "logic error: %s\n", e.what());
        return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "runtime error: %s\n", e.what());
        return 1;
    }
    return 0;
}
