// tracking_setup.hpp -- what tracker_app, position_dependent_eval_app and filtering_eval_app share: the pyramid feature types of the
// reference's createFeatureExtractor (HeadTracking.cpp:117-167,199-330: grayscale, h, whi, hog, ehog, lbp, glbp on a `pyramid direct`
// block), the trainable classifier of a `classifier` block, condensation::PositionDependentMeasurementModel from a `measurement
// positionDependent` block with its optional RVM filter (HeadTracking.cpp:503-533), and the RVM validator (HeadTracking.cpp:568-577).
//   measurement positionDependent {
//     feature grayscale|h|whi { pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }   scale 1 }
//                        (grayscale: ConversionFilter(CV_32F, 1/255); h: HistogramEqualizationFilter, ConversionFilter(CV_32F, 1/127.5, -1);
//                         whi: WhiteningFilter, HistogramEqualizationFilter, that ConversionFilter, UnitNormFilter(NORM_L2))
//     feature hog|ehog|lbp|glbp { pyramid direct { patch { width 16 height 16 minWidth 16 maxWidth 64 } interval 3 }   scale 1
//        gradientKernel 1 blurKernel 0 bins 9 signed 0 interpolate 0     (hog, ehog; glbp: gradientKernel, blurKernel)
//        type lbp8|lbp8uniform|lbp4|lbp4rotated                           (lbp, glbp)
//        histogram spatial { cellSize 4 blockSize 2 interpolate 0 signedAndUnsigned 0 concatenate 0 normalization l2hys }
//        histogram pyramid { levels 2 interpolate 0 signedAndUnsigned 0 normalization l2norm }
//        (ehog: histogram { cellSize 4 interpolate 0 signedAndUnsigned 0 alpha 0.2 }) }
//     filter before|after { classifierFile <FDRVM1 file>  [numFiltersToUse n]  feature grayscale|h|whi { ... } }
//                        (condensation::FilteringClassifierModel with an RvmClassifier on features of its own: before = RESET_WEIGHT,
//                         after = KEEP_WEIGHT; in place of `filter none`)
//     filter none   startFrameCount 3  stopFrameCount 0  targetThreshold 0.7  confidenceThreshold 0.95  positiveOffsetFactor 0.05
//     negativeOffsetFactor 0.5  sampleNegativesAroundTarget 0  sampleAdditionalNegatives 10  sampleTestNegatives 10  exploitSymmetry 0
//     classifier { training { type libSvm|libLinear c 1 ... }  logisticA 0.00556  logisticB -2.95  threshold 0 }
//     subclass 0         (1, with `filter none`: a subclass of the model that overrides nothing, for the tests of the device route)
//   }
//   validator rvm { classifierFile <FDRVM1 file>  [numFiltersToUse n]  feature grayscale|h|whi { ... }  sizes "0.9 1 1.1"  displacements "-0.1 0 0.1" }
//                        (beside `measurement`, in the `tracking` block: a condensation::ClassificationBasedStateValidator on the adaptive tracker)
//     feature haar { sizes "0.2 0.4" gridRows 5 gridCols 5 types "2rect 3rect 4rect center-surround"   scale 1 }
//     feature ihog { gradientCount 30 bins 9 signed false interpolate true  histogram spatial|pyramid { ... }   scale 1.1 }
//     feature iehog { gradientCount 30 bins 18 signed true interpolate false  histogram { cellSize 6 interpolate 0 signedAndUnsigned 1 alpha 0.2 }  scale 1 }
//     feature surf { gradientCount 12 cellCount 4   scale 1 }
//                        (the integral feature types of AdaptiveTracking.cpp:152-221: a DirectImageFeatureExtractor on the integral image,
//                         behind an IntegralFeatureExtractor except for haar, behind a PatchResizingFeatureExtractor when scale != 1)
//   measurement wvmSvm { firstClassifier { classifierFile .. } secondClassifier { classifierFile .. threshold .. }
//                        patch { width 20 height 20 minWidth 80 maxWidth 480 octaveLayerCount 5 } }
//                        (condensation::WvmSvmModel on DirectPyramidFeatureExtractor + GrayscaleFilter + HistEq64Filter: FaceTracking.cpp:75-84)
// Not built, each an invalid_argument that names it: the feature type histeq (u8 vectors: this host layer's RvmClassifier and the
// trainers take CV_32F) and `pyramid derived`.  A bare `filter before` / `filter after` without its block is refused with what the
// block needs.
#pragma once
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <sstream>
#include <vector>
#include "condensation/AdaptiveCondensationTracker.hpp"
#include "condensation/ClassificationBasedStateValidator.hpp"
#include "condensation/FilteringClassifierModel.hpp"
#include "condensation/PositionDependentMeasurementModel.hpp"
#include "imageprocessing/GradientMagnitudeFilter.hpp"
#include "liblinear/LibLinearClassifier.hpp"
#include "libsvm/LibSvmClassifier.hpp"
#include "fdcompat/ptree.hpp"

namespace tracking_setup {

using boost::property_tree::ptree;
using namespace imageprocessing;
using namespace classification;

// a boolean key: 0 / 1, or true / false as the reference's configuration files write them (boost's get<bool> reads both)
inline bool flag(const ptree& config, const std::string& key, bool dflt = false) {
    const std::string word = config.get<std::string>(key, std::string());
    if (word == "true") return true;
    if (word == "false") return false;
    return config.get<int>(key, dflt ? 1 : 0) != 0;
}

// DirectPyramidFeatureExtractor(width, height, minWidth, maxWidth, octaveLayerCount) with a GrayscaleFilter (DirectPyramidFeatureExtractor.cpp:27-36)
inline std::shared_ptr<DirectPyramidFeatureExtractor> createPyramidExtractor(int width, int height, int minWidth, int maxWidth, int interval);
// createPyramidExtractor, `direct` (DirectPyramidFeatureExtractor.cpp:41-43)
inline std::shared_ptr<DirectPyramidFeatureExtractor> createPyramidExtractor(const ptree& config) {
    if (config.get_value<std::string>() == "derived")
        throw std::invalid_argument("tracking: `pyramid derived` (a pyramid on the layers of another extractor's pyramid) is not built; use `pyramid direct`");
    if (config.get_value<std::string>() != "direct")
        throw std::invalid_argument("tracking: pyramid type `" + config.get_value<std::string>() + "` is not built (only `pyramid direct`)");
    return createPyramidExtractor(config.get<int>("patch.width"), config.get<int>("patch.height"), config.get<int>("patch.minWidth"), config.get<int>("patch.maxWidth"),
                                  config.get<int>("interval"));
}
inline std::shared_ptr<DirectPyramidFeatureExtractor> createPyramidExtractor(int width, int height, int minWidth, int maxWidth, int interval) {
    const double inc = std::pow(0.5, 1. / interval);
    double minScale = static_cast<double>(width) / maxWidth, maxScale = static_cast<double>(width) / minWidth;
    const int maxLayerIndex = cv::cvRound(std::log(minScale) / std::log(inc)), minLayerIndex = cv::cvRound(std::log(maxScale) / std::log(inc));
    maxScale = std::pow(inc, minLayerIndex);
    minScale = std::pow(inc, maxLayerIndex);
    auto extractor = std::make_shared<DirectPyramidFeatureExtractor>(std::make_shared<ImagePyramid>(static_cast<size_t>(interval), minScale, maxScale), width, height);
    extractor->addImageFilter(std::make_shared<GrayscaleFilter>());
    return extractor;
}

inline std::shared_ptr<HistogramFilter> createHistogramFilter(unsigned int bins, const ptree& config) {
    const std::string name = config.get<std::string>("normalization");
    HistogramFilter::Normalization normalization;
    if (name == "none") normalization = HistogramFilter::Normalization::NONE;
    else if (name == "l2norm") normalization = HistogramFilter::Normalization::L2NORM;
    else if (name == "l2hys") normalization = HistogramFilter::Normalization::L2HYS;
    else if (name == "l1norm") normalization = HistogramFilter::Normalization::L1NORM;
    else if (name == "l1sqrt") normalization = HistogramFilter::Normalization::L1SQRT;
    else throw std::invalid_argument("tracking: invalid normalization method: " + name);
    if (config.get_value<std::string>() == "spatial")
        return std::make_shared<SpatialHistogramFilter>((int)bins, config.get<int>("cellSize"), config.get<int>("blockSize"), flag(config, "interpolate"),
                                                        flag(config, "concatenate"), normalization);
    if (config.get_value<std::string>() == "pyramid")
        return std::make_shared<SpatialPyramidHistogramFilter>((int)bins, config.get<int>("levels"), flag(config, "interpolate"), normalization);
    throw std::invalid_argument("tracking: invalid histogram type: " + config.get_value<std::string>());
}

inline std::shared_ptr<HistogramFilter> createHogFilter(int bins, const ptree& config) {
    if (config.get_value<std::string>() == "spatial") {
        if (config.get<int>("blockSize") == 1 && !flag(config, "signedAndUnsigned")) return createHistogramFilter(bins, config);
        return std::make_shared<HogFilter>(bins, config.get<int>("cellSize"), config.get<int>("blockSize"), flag(config, "interpolate"), flag(config, "signedAndUnsigned"));
    }
    if (config.get_value<std::string>() == "pyramid")
        return std::make_shared<PyramidHogFilter>(bins, config.get<int>("levels"), flag(config, "interpolate"), flag(config, "signedAndUnsigned"));
    throw std::invalid_argument("tracking: invalid histogram type: " + config.get_value<std::string>());
}

inline std::shared_ptr<LbpFilter> createLbpFilter(const std::string& lbpType) {
    if (lbpType == "lbp8") return std::make_shared<LbpFilter>(LbpFilter::Type::LBP8);
    if (lbpType == "lbp8uniform") return std::make_shared<LbpFilter>(LbpFilter::Type::LBP8_UNIFORM);
    if (lbpType == "lbp4") return std::make_shared<LbpFilter>(LbpFilter::Type::LBP4);
    if (lbpType == "lbp4rotated") return std::make_shared<LbpFilter>(LbpFilter::Type::LBP4_ROTATED);
    throw std::invalid_argument("tracking: invalid LBP type: " + lbpType);
}

// wrapFeatureExtractor (AdaptiveTracking.cpp:263-267)
inline std::shared_ptr<FeatureExtractor> wrapFeatureExtractor(std::shared_ptr<FeatureExtractor> extractor, float scaleFactor) {
    if (scaleFactor == 1.0) return extractor;
    return std::make_shared<PatchResizingFeatureExtractor>(extractor, scaleFactor);
}

// "0.2 0.4" -> {0.2f, 0.4f}
inline std::vector<float> readFloats(const std::string& text) {
    std::vector<float> values;
    std::istringstream in(text);
    float value;
    while (in >> value) values.push_back(value);
    return values;
}

// the integral feature types (AdaptiveTracking.cpp:152-221): a DirectImageFeatureExtractor on [GrayscaleFilter, IntegralImageFilter];
// ihog, iehog and surf sit behind an IntegralFeatureExtractor, haar does not
inline std::shared_ptr<FeatureExtractor> createIntegralExtractor(const std::string& type, const ptree& config) {
    auto extractor = std::make_shared<DirectImageFeatureExtractor>();
    extractor->addImageFilter(std::make_shared<GrayscaleFilter>());
    extractor->addImageFilter(std::make_shared<IntegralImageFilter>());
    if (type == "haar") {
        int types = 0;
        std::string name;
        std::istringstream typesStream(config.get<std::string>("types"));
        while (typesStream >> name) {
            if (name == "2rect") types |= HaarFeatureFilter::TYPE_2RECTANGLE;
            else if (name == "3rect") types |= HaarFeatureFilter::TYPE_3RECTANGLE;
            else if (name == "4rect") types |= HaarFeatureFilter::TYPE_4RECTANGLE;
            else if (name == "center-surround") types |= HaarFeatureFilter::TYPE_CENTER_SURROUND;
            else if (name == "all") types |= HaarFeatureFilter::TYPES_ALL;
        }
        // as the reference passes them: gridRows is the constructor's xCount, gridCols its yCount
        extractor->addPatchFilter(std::make_shared<HaarFeatureFilter>(readFloats(config.get<std::string>("sizes")), (unsigned int)config.get<float>("gridRows"),
                                                                      (unsigned int)config.get<float>("gridCols"), types));
        return extractor;
    }
    extractor->addPatchFilter(std::make_shared<IntegralGradientFilter>(config.get<int>("gradientCount")));
    if (type == "surf") {
        extractor->addPatchFilter(std::make_shared<GradientSumFilter>(config.get<int>("cellCount")));
        extractor->addPatchFilter(std::make_shared<UnitNormFilter>(cv::NORM_L2));
    } else {
        extractor->addPatchFilter(std::make_shared<GradientBinningFilter>(config.get<int>("bins"), flag(config, "signed"), flag(config, "interpolate")));
        if (type == "ihog")
            extractor->addPatchFilter(createHogFilter(config.get<int>("bins"), config.get_child("histogram")));
        else
            extractor->addPatchFilter(std::make_shared<ExtendedHogFilter>(config.get<int>("bins"), config.get<int>("histogram.cellSize"), flag(config, "histogram.interpolate"),
                                                                          flag(config, "histogram.signedAndUnsigned"), config.get<float>("histogram.alpha")));
    }
    return std::make_shared<IntegralFeatureExtractor>(extractor);
}

inline std::shared_ptr<FeatureExtractor> createFeatureExtractor(const ptree& config) {
    const std::string type = config.get_value<std::string>();
    const float scaleFactor = config.get<float>("scale", 1.f);
    std::shared_ptr<DirectPyramidFeatureExtractor> extractor;
    if (type == "hog" || type == "ehog") {
        extractor = createPyramidExtractor(config.get_child("pyramid"));
        extractor->addLayerFilter(std::make_shared<GradientFilter>(config.get<int>("gradientKernel"), config.get<int>("blurKernel")));
        extractor->addLayerFilter(std::make_shared<GradientBinningFilter>(config.get<int>("bins"), flag(config, "signed"), flag(config, "interpolate")));
        if (type == "hog")
            extractor->addPatchFilter(createHogFilter(config.get<int>("bins"), config.get_child("histogram")));
        else
            extractor->addPatchFilter(std::make_shared<ExtendedHogFilter>(config.get<int>("bins"), config.get<int>("histogram.cellSize"), flag(config, "histogram.interpolate"),
                                                                          flag(config, "histogram.signedAndUnsigned"), config.get<float>("histogram.alpha")));
    } else if (type == "lbp" || type == "glbp") {
        extractor = createPyramidExtractor(config.get_child("pyramid"));
        std::shared_ptr<LbpFilter> lbpFilter = createLbpFilter(config.get<std::string>("type"));
        if (type == "glbp") {
            extractor->addLayerFilter(std::make_shared<GradientFilter>(config.get<int>("gradientKernel"), config.get<int>("blurKernel")));
            extractor->addLayerFilter(std::make_shared<GradientMagnitudeFilter>());
        }
        extractor->addLayerFilter(lbpFilter);
        extractor->addPatchFilter(createHistogramFilter(lbpFilter->getBinCount(), config.get_child("histogram")));
    } else if (type == "grayscale" || type == "h" || type == "whi") {   // HeadTracking.cpp:144-167
        extractor = createPyramidExtractor(config.get_child("pyramid"));
        if (type == "whi") extractor->addPatchFilter(std::make_shared<WhiteningFilter>());
        if (type != "grayscale") extractor->addPatchFilter(std::make_shared<HistogramEqualizationFilter>());
        extractor->addPatchFilter(type == "grayscale" ? std::make_shared<ConversionFilter>(CV_32F, 1.0 / 255.0)
                                                      : std::make_shared<ConversionFilter>(CV_32F, 1.0 / 127.5, -1.0));
        if (type == "whi") extractor->addPatchFilter(std::make_shared<UnitNormFilter>(cv::NORM_L2));
    } else if (type == "histeq") {
        throw std::invalid_argument("tracking: the feature type `histeq` is not built (its vectors are u8; the RvmClassifier and the trainers of this "
                                    "host layer take CV_32F vectors: use `h`)");
    } else if (type == "haar" || type == "ihog" || type == "iehog" || type == "surf") {
        return wrapFeatureExtractor(createIntegralExtractor(type, config), scaleFactor);
    } else {
        throw std::invalid_argument("tracking: invalid feature type: " + type);
    }
    return wrapFeatureExtractor(extractor, scaleFactor);
}

// the trainable SVM of a `classifier { training { ... } }` block
inline std::shared_ptr<TrainableSvmClassifier> createTrainableSvm(const ptree& ct) {
    const ptree& tr = ct.get_child("training");
    const std::string trainingType = tr.get("type", std::string("libSvm"));
    std::shared_ptr<TrainableSvmClassifier> svm;
    std::unique_ptr<ExampleManagement> negatives(new AgeBasedExampleManagement(tr.get("negativeCapacity", 100)));
    if (trainingType == "libLinear") {
        auto linear = std::make_shared<liblinear::LibLinearClassifier>(tr.get("c", 1.0), tr.get("bias", 0) != 0);
        linear->setNegativeExampleManagement(std::move(negatives));
        svm = linear;
    } else if (trainingType == "libSvm") {
        auto dual = libsvm::LibSvmClassifier::createBinarySvm(std::make_shared<LinearKernel>(), tr.get("c", 1.0), tr.get("compensateImbalance", 0) != 0);
        dual->setNegativeExampleManagement(std::move(negatives));
        svm = dual;
    } else {
        throw std::invalid_argument("tracker_app: invalid training type: " + trainingType);
    }
    svm->getSvm()->setThreshold(ct.get("threshold", 0.0f));   // as ProbabilisticSvmClassifier::load reads it
    return svm;
}

// the RvmClassifier of a `filter` or `validator` block: classifierFile, optional numFiltersToUse
inline std::shared_ptr<RvmClassifier> createRvm(const ptree& config) {
    std::shared_ptr<RvmClassifier> rvm = RvmClassifier::load(config);
    if (int count = config.get("numFiltersToUse", 0)) rvm->setNumFiltersToUse((unsigned int)count);
    return rvm;
}

// "0.9 1 1.1" -> {0.9, 1, 1.1}
inline std::vector<double> readValues(const std::string& text) {
    std::vector<double> values;
    std::istringstream in(text);
    double value;
    while (in >> value) values.push_back(value);
    if (values.empty() || !in.eof()) throw std::invalid_argument("tracking: invalid list of values: `" + text + "`");
    return values;
}

// `validator rvm { ... }` of the tracking block (HeadTracking.cpp:568-577); null for `validator none` or no such key
inline std::shared_ptr<condensation::ClassificationBasedStateValidator> createValidator(const ptree& pt) {
    const std::string type = pt.get("validator", std::string("none"));
    if (type == "none") return nullptr;
    if (type != "rvm") throw std::invalid_argument("tracking: invalid validator type: " + type);
    const ptree& vt = pt.get_child("validator");
    if (!vt.count("classifierFile") || !vt.count("feature"))
        throw std::invalid_argument("tracking: `validator rvm` (condensation::ClassificationBasedStateValidator) needs a block: validator rvm { classifierFile "
                                    "<FDRVM1 file> [numFiltersToUse n] feature grayscale|h|whi { pyramid direct { .. } } sizes \"0.9 1 1.1\" displacements \"-0.1 0 0.1\" }");
    return std::make_shared<condensation::ClassificationBasedStateValidator>(createFeatureExtractor(vt.get_child("feature")), createRvm(vt),
                                                                             readValues(vt.get("sizes", std::string("1"))),
                                                                             readValues(vt.get("displacements", std::string("0"))));
}

struct PositionDependentSetup {
    std::shared_ptr<FeatureExtractor> featureExtractor;
    std::shared_ptr<TrainableProbabilisticSvmClassifier> classifier;
    std::shared_ptr<condensation::PositionDependentMeasurementModel> model;
    std::shared_ptr<FeatureExtractor> filterExtractor;                       // with `filter before|after`
    std::shared_ptr<RvmClassifier> filter;
    std::shared_ptr<condensation::FilteringClassifierModel> filteringModel;
};
// the filtering behaviour of a `filter` key: false for `none`
inline bool filterBehavior(const ptree& mt, condensation::FilteringClassifierModel::Behavior& behavior) {
    const std::string filter = mt.get("filter", std::string("none"));
    if (filter == "none") return false;
    if (filter != "before" && filter != "after") throw std::invalid_argument("tracking: invalid filter type: " + filter);
    const ptree& ft = mt.get_child("filter");
    if (!ft.count("classifierFile") || !ft.count("feature"))
        throw std::invalid_argument("tracking: `filter " + filter + "` (condensation::FilteringClassifierModel) needs a block: filter " + filter +
                                    " { classifierFile <FDRVM1 file> [numFiltersToUse n] feature grayscale|h|whi { pyramid direct { .. } } }");
    behavior = filter == "before" ? condensation::FilteringClassifierModel::Behavior::RESET_WEIGHT : condensation::FilteringClassifierModel::Behavior::KEEP_WEIGHT;
    return true;
}
// a subclass that changes nothing (`subclass 1`, not one of the reference's keys): the device route restates the class itself and must
// leave any subclass to the generic route
struct SubclassedPositionDependentModel : public condensation::PositionDependentMeasurementModel {
    using condensation::PositionDependentMeasurementModel::PositionDependentMeasurementModel;
};
inline PositionDependentSetup createPositionDependent(const ptree& mt, unsigned int seed) {
    PositionDependentSetup s;
    condensation::FilteringClassifierModel::Behavior behavior;
    const bool filtering = filterBehavior(mt, behavior);
    s.featureExtractor = createFeatureExtractor(mt.get_child("feature"));
    const ptree& ct = mt.get_child("classifier");
    s.classifier = std::make_shared<FixedTrainableProbabilisticSvmClassifier>(createTrainableSvm(ct), ct.get("logisticA", 0.00556), ct.get("logisticB", -2.95));
    if (filtering) {   // HeadTracking.cpp:507-518
        s.filterExtractor = createFeatureExtractor(mt.get_child("filter.feature"));
        s.filter = createRvm(mt.get_child("filter"));
        s.filteringModel = std::make_shared<condensation::FilteringClassifierModel>(s.filterExtractor, s.filter, s.featureExtractor, s.classifier, behavior);
        s.model = std::make_shared<condensation::PositionDependentMeasurementModel>(s.filteringModel, s.featureExtractor, s.classifier, seed);
    } else if (mt.get("subclass", 0) != 0) {
        s.model = std::make_shared<SubclassedPositionDependentModel>(s.featureExtractor, s.classifier, seed);
    } else {
        s.model = std::make_shared<condensation::PositionDependentMeasurementModel>(s.featureExtractor, s.classifier, seed);
    }
    s.model->setFrameCounts(mt.get("startFrameCount", 3u), mt.get("stopFrameCount", 0u));
    s.model->setThresholds(mt.get("targetThreshold", 0.7f), mt.get("confidenceThreshold", 0.95f));
    s.model->setOffsetFactors(mt.get("positiveOffsetFactor", 0.05f), mt.get("negativeOffsetFactor", 0.5f));
    s.model->setSamplingProperties(mt.get("sampleNegativesAroundTarget", 0u), mt.get("sampleAdditionalNegatives", 10u), mt.get("sampleTestNegatives", 10u),
                                   flag(mt, "exploitSymmetry"));
    return s;
}

// `measurement wvmSvm { firstClassifier { .. } secondClassifier { .. } patch { width 20 height 20 minWidth 80 maxWidth 480 octaveLayerCount 5 } }`:
// the measurement model of the reference's face tracker (FaceTracking.cpp:75-84), the classifier nodes as ffp_detect_app and
// condensation_eval_app load them, the patch defaults those of FaceTracking.cpp:75
struct WvmSvmSetup {
    std::shared_ptr<DirectPyramidFeatureExtractor> featureExtractor;
    std::shared_ptr<condensation::WvmSvmModel> model;
    int minWidth, maxWidth;
};
inline WvmSvmSetup createWvmSvm(const ptree& mt) {
    if (!mt.count("firstClassifier") || !mt.count("secondClassifier"))
        throw std::invalid_argument("tracking: `measurement wvmSvm` (condensation::WvmSvmModel) needs a block: measurement wvmSvm { firstClassifier { classifierFile "
                                    "<FDWVM1 file> } secondClassifier { classifierFile <SVM text file> [threshold t] } [patch { width 20 height 20 minWidth 80 "
                                    "maxWidth 480 octaveLayerCount 5 }] }");
    WvmSvmSetup s;
    s.minWidth = mt.get("patch.minWidth", 80);
    s.maxWidth = mt.get("patch.maxWidth", 480);
    s.featureExtractor = createPyramidExtractor(mt.get("patch.width", 20), mt.get("patch.height", 20), s.minWidth, s.maxWidth, mt.get("patch.octaveLayerCount", 5));
    s.featureExtractor->addPatchFilter(std::make_shared<HistEq64Filter>());
    s.model = std::make_shared<condensation::WvmSvmModel>(s.featureExtractor, ProbabilisticWvmClassifier::load(mt.get_child("firstClassifier")),
                                                          ProbabilisticSvmClassifier::load(mt.get_child("secondClassifier")));
    return s;
}

// `adaptive selfLearning { positiveThreshold 0.85 negativeThreshold 0.05 feature <type> { .. } classifier { kernel rbf { gamma g } | poly {
// alpha a constant c degree d }  training { c 1 compensateImbalance 0 examples fixedsize positiveExamples 10 negativeExamples 50
// minPositiveExamples 3 }  probabilistic fixed { logisticA a logisticB b } | default { positiveExamples 10 negativeExamples 50 } } }`: the
// adaptive model of the reference's partiallyAdaptiveTrackingApp, as far as the classes behind its keys exist here.  `fixedsize` is an
// AgeBasedExampleManagement of that capacity (minPositiveExamples is its required size); `subclass 1` (not one of the reference's keys)
// builds a subclass that changes nothing, which must keep the generic route
struct SubclassedSelfLearningModel : public condensation::SelfLearningMeasurementModel {
    using condensation::SelfLearningMeasurementModel::SelfLearningMeasurementModel;
};
inline std::shared_ptr<condensation::SelfLearningMeasurementModel> createSelfLearning(const ptree& at) {
    if (!at.count("feature") || !at.count("classifier"))
        throw std::invalid_argument("tracking: `adaptive selfLearning` (condensation::SelfLearningMeasurementModel) needs a block: adaptive selfLearning { "
                                    "positiveThreshold p negativeThreshold n feature <type> { .. } classifier { kernel rbf { gamma g } training { c 1 } "
                                    "probabilistic fixed { logisticA a logisticB b } } }");
    const ptree& ct = at.get_child("classifier");
    if (flag(ct, "withWvm")) throw std::invalid_argument("tracking: `withWvm true` (TrainableProbabilisticTwoStageClassifier) is not built");
    if (ct.count("training") && ct.get_child("training").count("staticNegatives"))
        throw std::invalid_argument("tracking: `staticNegatives` is not built (LibSvmClassifier::loadStaticNegatives)");
    const std::string kernelType = ct.get("kernel", std::string("rbf"));
    std::shared_ptr<Kernel> kernel;
    if (kernelType == "rbf") kernel = std::make_shared<RbfKernel>(ct.get("kernel.gamma", 0.002));
    else if (kernelType == "poly") kernel = std::make_shared<PolynomialKernel>(ct.get("kernel.alpha", 0.05), ct.get("kernel.constant", 0.0), ct.get("kernel.degree", 2));
    else throw std::invalid_argument("tracking: invalid kernel type: " + kernelType + " (rbf and poly are supported)");
    const std::string examples = ct.get("training.examples", std::string("fixedsize"));
    if (examples == "framebased") throw std::invalid_argument("tracking: `examples framebased` (FrameBasedExampleManagement) is not built: use `fixedsize`");
    if (examples != "fixedsize") throw std::invalid_argument("tracking: invalid example management: " + examples);
    auto svm = libsvm::LibSvmClassifier::createBinaryKernelSvm(kernel, ct.get("training.c", 1.0), ct.get("training.compensateImbalance", 0) != 0);
    svm->setPositiveExampleManagement(std::unique_ptr<ExampleManagement>(
        new AgeBasedExampleManagement(ct.get("training.positiveExamples", 10), ct.get("training.minPositiveExamples", 3))));
    svm->setNegativeExampleManagement(std::unique_ptr<ExampleManagement>(new AgeBasedExampleManagement(ct.get("training.negativeExamples", 50))));
    svm->getSvm()->setThreshold(ct.get("threshold", 0.0f));
    const std::string probabilistic = ct.get("probabilistic", std::string("fixed"));
    std::shared_ptr<TrainableProbabilisticSvmClassifier> classifier;
    if (probabilistic == "fixed")
        classifier = std::make_shared<FixedTrainableProbabilisticSvmClassifier>(svm, ct.get("probabilistic.logisticA", 0.00556), ct.get("probabilistic.logisticB", -2.95));
    else if (probabilistic == "default")
        classifier = std::make_shared<TrainableProbabilisticSvmClassifier>(svm, ct.get("probabilistic.positiveExamples", 10), ct.get("probabilistic.negativeExamples", 50));
    else
        throw std::invalid_argument("tracking: invalid probabilistic type: " + probabilistic + " (default and fixed are supported)");
    std::shared_ptr<FeatureExtractor> extractor = createFeatureExtractor(at.get_child("feature"));
    const double positiveThreshold = at.get("positiveThreshold", 0.85), negativeThreshold = at.get("negativeThreshold", 0.05);
    if (at.get("subclass", 0) != 0) return std::make_shared<SubclassedSelfLearningModel>(extractor, classifier, positiveThreshold, negativeThreshold);
    return std::make_shared<condensation::SelfLearningMeasurementModel>(extractor, classifier, positiveThreshold, negativeThreshold);
}

}  // namespace tracking_setup
