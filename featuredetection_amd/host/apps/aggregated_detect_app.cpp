// aggregated_detect_app -- example of an AggregatedFeaturesDetector application on this backend.  It reads the feature and
// detection keys of the reference's DetectorTrainingApp configs and, as the key `approximatePyramid` says, builds the detector either
// on exact feature layers (the filter constructor) or on an approximated feature pyramid (ImagePyramid::createApproximated ->
// AggregatedFeaturesExtractor -> the extractor constructor), through the host layer's classes.
//
//   aggregated_detect_app <config.cfg> <svm file> <image.pgm|ppm>...
//
// config (INFO format):
//   features  { type fhog[N] | fpdw  windowWidthInCells .. windowHeightInCells .. cellSizeInPixels .. widthScaleFactor .. heightScaleFactor ..
//               lambdas "l0 l1 ..." (optional, this app: the lambdas of the approximated pyramid; absent = estimated per image) }
//   detection { minWindowWidthInPixels .. minWindowHeightInPixels .. octaveLayerCount .. approximatePyramid true|false
//               nmsOverlapThreshold ..  threshold .. (optional, this app: the SVM's threshold, default 0) }
// type fpdw: no image filter, layer filter ChainedFilter(FpdwFeaturesFilter(true, false, cell, 0.01), AggregationFilter(cell, true, false))
// (DetectorTrainingApp.cpp:99-113), ten lambdas, BGR images only.
// The SVM is read from the text format of SvmClassifier::store.  Output: one line per detection, "<image index> x y width height score".
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include "detection/detection_all.hpp"
#include "imageprocessing/extraction/AggregatedFeaturesExtractor.hpp"
#include "imageprocessing/filtering/AggregationFilter.hpp"
#include "imageprocessing/filtering/FhogFilter.hpp"
#include "imageprocessing/filtering/FpdwFeaturesFilter.hpp"
#include "fdcompat/ptree.hpp"

using namespace detection;
using namespace imageprocessing;
using classification::SvmClassifier;
using boost::property_tree::ptree;
using imageprocessing::extraction::AggregatedFeaturesExtractor;
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

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "call: %s config svm image...\n", argv[0]);
        return 2;
    }
    try {
        ptree config;
        boost::property_tree::read_info(string(argv[1]), config);
        const ptree& fcfg = config.get_child("features");
        const ptree& dcfg = config.get_child("detection");
        // features: FHOG cells, fhog or fhog<unsigned bin count>, or FPDW channel features
        const string type = fcfg.get<string>("type");
        const bool fpdw = type == "fpdw";
        if (!fpdw && type.compare(0, 4, "fhog") != 0) throw std::invalid_argument("features.type: expected fhog[N] or fpdw, but was '" + type + "'");
        const int bins = !fpdw && type.size() > 4 ? std::stoi(type.substr(4)) : 9;
        const int cell = fcfg.get<int>("cellSizeInPixels");
        const cv::Size window(fcfg.get<int>("windowWidthInCells"), fcfg.get<int>("windowHeightInCells"));
        const float widthScale = 1.0f / fcfg.get<float>("widthScaleFactor"), heightScale = 1.0f / fcfg.get<float>("heightScaleFactor");
        vector<double> lambdas;
        {
            std::istringstream in(fcfg.get<string>("lambdas", ""));
            for (double v; in >> v;) lambdas.push_back(v);
        }
        // detection
        const int octaveLayers = dcfg.get<int>("octaveLayerCount");
        const int minWidth = dcfg.get<int>("minWindowWidthInPixels");
        (void)dcfg.get<int>("minWindowHeightInPixels");   // required like in the reference's configs; the width decides
        const bool approximate = flag(dcfg, "approximatePyramid");

        std::ifstream svmFile(argv[2]);
        if (!svmFile.is_open()) throw std::runtime_error(string("cannot open SVM file ") + argv[2]);
        shared_ptr<SvmClassifier> svm = SvmClassifier::load(svmFile);
        svm->setThreshold(dcfg.get<float>("threshold", 0.0f));

        auto gray = make_shared<GrayscaleFilter>();
        shared_ptr<ImageFilter> layerFilter;
        if (fpdw) {
            auto chain = make_shared<ChainedFilter>();
            chain->add(make_shared<FpdwFeaturesFilter>(true, false, cell, 0.01));
            chain->add(make_shared<AggregationFilter>(cell, true, false));
            layerFilter = chain;
        } else {
            layerFilter = make_shared<FhogFilter>(cell, bins, false, true, 0.2f);
        }
        auto nms = make_shared<NonMaximumSuppression>(dcfg.get<double>("nmsOverlapThreshold"), NonMaximumSuppression::MaximumType::MAX_SCORE);
        shared_ptr<AggregatedFeaturesDetector> detector;
        if (approximate) {
            auto pyramid = ImagePyramid::createApproximated(octaveLayers, 0.5, 1.0, lambdas);
            if (!fpdw) pyramid->addImageFilter(gray);
            pyramid->addLayerFilter(layerFilter);
            detector = make_shared<AggregatedFeaturesDetector>(make_shared<AggregatedFeaturesExtractor>(pyramid, window, cell, true, minWidth), svm, nms,
                                                               widthScale, heightScale);
        } else {
            if (!lambdas.empty()) throw std::invalid_argument("features.lambdas belong to approximatePyramid true");
            if (fpdw) detector = make_shared<AggregatedFeaturesDetector>(layerFilter, cell, window, octaveLayers, svm, nms, widthScale, heightScale, minWidth);
            else detector = make_shared<AggregatedFeaturesDetector>(gray, layerFilter, cell, window, octaveLayers, svm, nms, widthScale, heightScale, minWidth);
        }
        for (int a = 3; a < argc; ++a) {
            const cv::Mat image = read_pnm(argv[a]);
            for (const auto& d : detector->detectWithScores(image))
                std::printf("%d %d %d %d %d %.9g\n", a - 3, d.first.x, d.first.y, d.first.width, d.first.height, (double)d.second);
        }
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
