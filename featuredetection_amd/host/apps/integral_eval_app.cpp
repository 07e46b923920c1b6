// integral_eval_app -- the measurement step of the reference's particle-filter trackers with a condensation::SingleClassifierModel over
// an integral-image feature extractor, as benchmarkApp wires it (BenchmarkRunner.cpp:202-233 createHaarExtractor, :278-286
// createSurfExtractor): scores a list of samples on one frame.
//   usage: integral_eval_app <config.cfg> <image.ppm|pgm> <samples.txt>
// config (boost info format, keys of benchmarkApp):
//   feature haar { sizes "0.2 0.4"  gridRows 5  gridCols 5  types "2rect 3rect 4rect center-surround" }     (types: also "all")
//   feature surf { gradientCount 12  cellCount 4 }
//   feature ihog { gradientCount 30  bins 9  signed false  interpolate true  scale 1.1                      (keys of the tracking apps,
//                  histogram spatial { cellSize 6 blockSize 1 interpolate false normalization l2norm } }     AdaptiveTracking.cpp:189-213:
//   feature iehog { gradientCount 30  bins 18  signed true  interpolate false  scale 1.1                    behind an IntegralFeatureExtractor,
//                   histogram { cellSize 6 interpolate 0 signedAndUnsigned 1 alpha 0.2 } }                  and a PatchResizingFeatureExtractor
//                                                                                                           when scale != 1)
//   classifier { classifierFile <SVM text file>  [threshold t] [logisticA a logisticB b] }
//   aspectRatio r                                                                                           (optional, default 1)
// samples.txt: one "x y size" per line (width = size, height = cvRound(aspectRatio * size)).  Prints "<target 0|1> <weight>" per sample, and on
// stderr whether the samples were scored by one fused device call or by the per-sample loop.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include "condensation/condensation_all.hpp"
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

static shared_ptr<FeatureExtractor> createHaarExtractor(const ptree& config) {   // BenchmarkRunner.cpp:202-233
    std::vector<float> sizes;
    float size;
    std::istringstream sizesStream(config.get<string>("sizes"));
    while (sizesStream >> size) sizes.push_back(size);
    const float gridRows = config.get<float>("gridRows");
    const float gridCols = config.get<float>("gridCols");
    int types = 0;
    string type;
    std::istringstream typesStream(config.get<string>("types"));
    while (typesStream >> type) {
        if (type == "2rect") types |= HaarFeatureFilter::TYPE_2RECTANGLE;
        else if (type == "3rect") types |= HaarFeatureFilter::TYPE_3RECTANGLE;
        else if (type == "4rect") types |= HaarFeatureFilter::TYPE_4RECTANGLE;
        else if (type == "center-surround") types |= HaarFeatureFilter::TYPE_CENTER_SURROUND;
        else if (type == "all") types |= HaarFeatureFilter::TYPES_ALL;
    }
    auto featureExtractor = make_shared<DirectImageFeatureExtractor>();
    featureExtractor->addImageFilter(make_shared<GrayscaleFilter>());
    featureExtractor->addImageFilter(make_shared<IntegralImageFilter>());
    // as the reference passes them: gridRows is the constructor's xCount, gridCols its yCount
    featureExtractor->addPatchFilter(make_shared<HaarFeatureFilter>(sizes, (unsigned int)gridRows, (unsigned int)gridCols, types));
    return featureExtractor;
}

static shared_ptr<FeatureExtractor> createSurfExtractor(const ptree& config) {   // BenchmarkRunner.cpp:278-286
    auto featureExtractor = make_shared<DirectImageFeatureExtractor>();
    featureExtractor->addImageFilter(make_shared<GrayscaleFilter>());
    featureExtractor->addImageFilter(make_shared<IntegralImageFilter>());
    featureExtractor->addPatchFilter(make_shared<IntegralGradientFilter>(config.get<int>("gradientCount")));
    featureExtractor->addPatchFilter(make_shared<GradientSumFilter>(config.get<int>("cellCount")));
    featureExtractor->addPatchFilter(make_shared<UnitNormFilter>(cv::NORM_L2));
    return featureExtractor;
}

static shared_ptr<FeatureExtractor> createFeatureExtractor(const ptree& config) {   // BenchmarkRunner.cpp:288-313
    const string kind = config.get_value<string>();
    if (kind == "haar") return createHaarExtractor(config);
    if (kind == "surf") return createSurfExtractor(config);
    if (kind == "ihog" || kind == "iehog") return tracking_setup::createFeatureExtractor(config);
    throw std::invalid_argument("invalid feature type: " + kind + " (integral_eval_app knows haar, surf, ihog and iehog)");
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <config.cfg> <image.ppm|pgm> <samples.txt>\n", argv[0]);
        return 2;
    }
    try {
        ptree pt;
        boost::property_tree::read_info(string(argv[1]), pt);
        auto featureExtractor = createFeatureExtractor(pt.get_child("feature"));
        auto classifier = ProbabilisticSvmClassifier::load(pt.get_child("classifier"));
        Sample::setAspectRatio(pt.get("aspectRatio", 1.0));
        SingleClassifierModel model(featureExtractor, classifier);
        std::vector<shared_ptr<Sample>> samples;
        std::ifstream sf(argv[3]);
        if (!sf.is_open()) throw std::runtime_error(string("cannot open samples ") + argv[3]);
        int x, y, size;
        while (sf >> x >> y >> size) samples.push_back(make_shared<Sample>(x, y, size));
        auto image = make_shared<VersionedImage>(read_pnm(argv[2]));
        model.evaluate(image, samples);
        std::fprintf(stderr, "%zu samples: %s\n", samples.size(), model.getFusedEvaluationCount() == 1 ? "one fused device call" : "per-sample loop");
        for (const auto& s : samples) std::printf("%d %.17g\n", s->isTarget() ? 1 : 0, s->getWeight());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
