// DetectorTrainer.hpp / DetectorTrainer.cpp of the reference's DetectorTrainingApp (:99-160 / :41-301): trains the linear SVM of an
// AggregatedFeaturesDetector from annotated images -- positive windows, random negatives, a C-SVC, then rounds of hard-negative
// bootstrapping with the detector under training.  Features and the SVM run on the device
// (extraction::AggregatedFeaturesExtractor, libsvm::LibSvmClassifier).  Deviations from the reference:
//   * a seeded std::mt19937 (constructor argument) replaces std::random_device;
//   * addRandomNegativeExamples gives up with std::runtime_error after maxRejectedDrawsPerNegative rejected draws per wanted
//     negative (the reference loops forever on an image its annotations cover);
//   * TrainingParams::probabilistic throws std::invalid_argument (LibSvmClassifier has no sigmoid fit on this backend);
//   * more than 16384 examples at a training throw std::runtime_error naming TrainingParams::maxNegatives.
// Not in the reference: setTrace(stream) records what a replay needs (detector_training_app --trace).
#pragma once
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <ostream>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>
#include "detectortraining/Annotations.hpp"
#include "detectortraining/LabeledImage.hpp"
#include "classification/ConfidenceBasedExampleManagement.hpp"
#include "classification/LinearKernel.hpp"
#include "classification/SvmClassifier.hpp"
#include "detection/AggregatedFeaturesDetector.hpp"
#include "detection/NonMaximumSuppression.hpp"
#include "imageprocessing/extraction/AggregatedFeaturesExtractor.hpp"
#include "libsvm/LibSvmClassifier.hpp"

struct FeatureParams {
    cv::Size windowSizeInCells;       // detection window size in cells
    int cellSizeInPixels = 8;
    int octaveLayerCount = 5;         // image pyramid layers per octave
    float widthScaleFactor = 1.0f;    // applied to the annotated width before training
    float heightScaleFactor = 1.0f;
    cv::Size windowSizeInPixels() const { return cv::Size(windowSizeInCells.width * cellSizeInPixels, windowSizeInCells.height * cellSizeInPixels); }
    double windowAspectRatio() const { return static_cast<double>(windowSizeInCells.width) / static_cast<double>(windowSizeInCells.height); }
    float widthScaleFactorInv() const { return 1.0f / widthScaleFactor; }
    float heightScaleFactorInv() const { return 1.0f / heightScaleFactor; }
};

struct TrainingParams {
    bool mirrorTrainingData = true;
    int maxNegatives = 0;                  // 0: not constrained
    int randomNegativesPerImage = 20;
    int maxHardNegativesPerImage = 100;    // per image and bootstrapping round
    int bootstrappingRounds = 3;
    float negativeScoreThreshold = -1.0f;  // SVM score threshold for retrieving strong negatives
    double overlapThreshold = 0.3;         // maximum overlap between a negative and a non-negative annotation
    double C = 1;
    bool compensateImbalance = false;
    bool probabilistic = false;            // not available on this backend
    int maxRejectedDrawsPerNegative = 1000;   // not in the reference: bound of addRandomNegativeExamples
};

// keeps the negatives the classifier is least sure about (ConfidenceBasedExampleManagement, negatives, nothing kept unconditionally).
// Before the first training the reference's untrained SVM scores every example 0, and which of the equally confident examples its
// sort keeps is the sort's choice; here the untrained classifier takes new examples in their order until the store is full.
class HardNegativeExampleManagement : public classification::ConfidenceBasedExampleManagement {
public:
    HardNegativeExampleManagement(const std::shared_ptr<classification::BinaryClassifier>& classifier, size_t capacity)
        : classification::ConfidenceBasedExampleManagement(classifier, false, capacity),
          trainable(std::dynamic_pointer_cast<classification::TrainableClassifier>(classifier)) {
        setFirstExamplesToKeep(0);
    }
    void add(const std::vector<cv::Mat>& newExamples) override {
        std::shared_ptr<classification::TrainableClassifier> t = trainable.lock();
        if (t && !t->isUsable()) {
            for (size_t i = 0; i < newExamples.size() && examples.size() < capacity; ++i) examples.push_back(newExamples[i]);
            return;
        }
        classification::ConfidenceBasedExampleManagement::add(newExamples);
    }
private:
    std::weak_ptr<classification::TrainableClassifier> trainable;
};

class DetectorTrainer {
public:
    explicit DetectorTrainer(bool printProgressInformation = false, std::string printPrefix = "", unsigned int seed = 5489u)
        : printProgressInformation(printProgressInformation), printPrefix(printPrefix), aspectRatio(1), aspectRatioInv(1), generator(seed) {}

    void setTrainingParameters(TrainingParams params) { trainingParams = params; }

    void setFeatures(FeatureParams params, const std::shared_ptr<imageprocessing::ImageFilter>& filter,
                     const std::shared_ptr<imageprocessing::ImageFilter>& imageFilter = std::shared_ptr<imageprocessing::ImageFilter>()) {
        featureParams = params;
        aspectRatio = params.windowAspectRatio();
        aspectRatioInv = 1.0 / aspectRatio;
        this->imageFilter = imageFilter;
        this->filter = filter;
        featureExtractor.reset();   // created by train(): the device is not touched before
    }

    void train(std::vector<LabeledImage> images) {
        using imageprocessing::extraction::AggregatedFeaturesExtractor;
        if (!filter) throw std::runtime_error("DetectorTrainer: setFeatures has to be called before train");
        createEmptyClassifier();
        if (!featureExtractor) {
            if (!imageFilter)
                featureExtractor = std::make_shared<AggregatedFeaturesExtractor>(filter, featureParams.windowSizeInCells, featureParams.cellSizeInPixels,
                                                                                 featureParams.octaveLayerCount);
            else
                featureExtractor = std::make_shared<AggregatedFeaturesExtractor>(imageFilter, filter, featureParams.windowSizeInCells,
                                                                                 featureParams.cellSizeInPixels, featureParams.octaveLayerCount);
        }
        collectTrainingExamples(images, true, -1);
        trainClassifier(true);
        for (int round = 0; round < trainingParams.bootstrappingRounds; ++round) {
            collectTrainingExamples(images, false, round);
            trainClassifier(false);
        }
    }

    void storeClassifier(const std::string& filename) const {
        std::ofstream stream(filename);
        if (!stream.is_open()) throw std::runtime_error("DetectorTrainer: cannot write " + filename);
        classifier->getSvm()->store(stream);
        stream.close();
    }

    cv::Mat getWeightVector() const { return classifier->getSvm()->getSupportVectors().front(); }

    std::shared_ptr<detection::AggregatedFeaturesDetector> getDetector(std::shared_ptr<detection::NonMaximumSuppression> nms) const {
        return getDetector(nms, featureParams.octaveLayerCount);
    }
    std::shared_ptr<detection::AggregatedFeaturesDetector> getDetector(std::shared_ptr<detection::NonMaximumSuppression> nms, int octaveLayerCount,
                                                                       float threshold = 0) const {
        using detection::AggregatedFeaturesDetector;
        if (!classifier || !classifier->isUsable()) throw std::runtime_error("DetectorTrainer: must train a classifier first");
        classifier->getSvm()->setThreshold(threshold);
        std::shared_ptr<AggregatedFeaturesDetector> detector;
        if (!imageFilter)
            detector = std::make_shared<AggregatedFeaturesDetector>(filter, featureParams.cellSizeInPixels, featureParams.windowSizeInCells, octaveLayerCount,
                                                                    classifier->getSvm(), nms, featureParams.widthScaleFactorInv(),
                                                                    featureParams.heightScaleFactorInv());
        else
            detector = std::make_shared<AggregatedFeaturesDetector>(imageFilter, filter, featureParams.cellSizeInPixels, featureParams.windowSizeInCells,
                                                                    octaveLayerCount, classifier->getSvm(), nms, featureParams.widthScaleFactorInv(),
                                                                    featureParams.heightScaleFactorInv());
        classifier->getSvm()->setThreshold(0);
        return detector;
    }

    // not in the reference.  The trace, one record per line (floats in C99 hexadecimal):
    //   image <index> <mirrored> <round>            round -1: the initial collection
    //   positive x y w h  <1 bx by bw bh | 0>        an annotated box and the bounds of its patch
    //   random x y w h  <accepted>  <1 bx by bw bh | 0>   every draw, in draw order
    //   hard x y w h  <accepted>  <1 bx by bw bh | 0>     every detection that was looked at, in the detector's order
    //   training <initial> n_pos n_neg new_pos new_neg iterations rho
    //   weights bias w0 w1 ...
    void setTrace(std::ostream* stream) { trace = stream; }
    std::shared_ptr<libsvm::LibSvmClassifier> getClassifier() const { return classifier; }
    std::shared_ptr<imageprocessing::extraction::AggregatedFeaturesExtractor> getFeatureExtractor() const { return featureExtractor; }

    // the pieces of train(), public for the host tests
    imageio::RectLandmark adjustSize(const imageio::RectLandmark& landmark) const {
        float width = featureParams.widthScaleFactor * landmark.getWidth();
        float height = featureParams.heightScaleFactor * landmark.getHeight();
        if (width < aspectRatio * height) width = aspectRatio * height;
        else if (width > aspectRatio * height) height = width * aspectRatioInv;
        return imageio::RectLandmark(landmark.getName(), landmark.getX(), landmark.getY(), width, height);
    }
    static cv::Mat flipHorizontally(const cv::Mat& image) {
        cv::Mat flipped;
        cv::flip(image, flipped, 1);
        return flipped;
    }
    static imageio::RectLandmark flipHorizontally(const imageio::RectLandmark& landmark, int imageWidth) {
        const float mirroredX = imageWidth - landmark.getX() - 1;
        return imageio::RectLandmark(landmark.getName(), mirroredX, landmark.getY(), landmark.getWidth(), landmark.getHeight());
    }
    cv::Rect createRandomBounds(cv::Size imageSize) {
        typedef std::uniform_int_distribution<int> uniform_int;
        const int minWidth = featureParams.windowSizeInPixels().width;
        const int maxWidth = std::min(imageSize.width, static_cast<int>(imageSize.height * aspectRatio));
        if (maxWidth < minWidth) throw std::runtime_error("DetectorTrainer: the image is smaller than the detection window");
        const int width = uniform_int{minWidth, maxWidth}(generator);
        const int height = static_cast<int>(std::round(width * aspectRatioInv));
        const int x = uniform_int{0, imageSize.width - width}(generator);
        const int y = uniform_int{0, imageSize.height - height}(generator);
        return cv::Rect(x, y, width, height);
    }
    bool isOverlapping(cv::Rect boxToTest, const std::vector<cv::Rect>& otherBoxes) const {
        for (const cv::Rect& otherBox : otherBoxes)
            if (computeOverlap(boxToTest, otherBox) > trainingParams.overlapThreshold) return true;
        return false;
    }
    static double computeOverlap(cv::Rect a, cv::Rect b) {
        const double intersectionArea = (a & b).area();
        const double unionArea = a.area() + b.area() - intersectionArea;
        return intersectionArea / unionArea;
    }

private:
    void createEmptyClassifier() {
        classifier = libsvm::LibSvmClassifier::createBinarySvm(std::make_shared<classification::LinearKernel>(), trainingParams.C,
                                                               trainingParams.compensateImbalance, trainingParams.probabilistic);
        if (trainingParams.maxNegatives > 0)
            classifier->setNegativeExampleManagement(std::unique_ptr<classification::ExampleManagement>(
                new HardNegativeExampleManagement(classifier, trainingParams.maxNegatives)));
    }

    void collectTrainingExamples(const std::vector<LabeledImage>& images, bool initial, int round) {
        if (printProgressInformation)
            std::cout << printPrefix << (initial ? "collecting initial training examples" : "collecting additional hard negative training examples")
                      << std::endl;
        for (size_t index = 0; index < images.size(); ++index) {
            const LabeledImage& labeledImage = images[index];
            std::vector<imageio::RectLandmark> landmarks;
            landmarks.reserve(labeledImage.landmarks.size());
            for (const imageio::RectLandmark& landmark : labeledImage.landmarks) landmarks.push_back(adjustSize(landmark));
            if (trace) *trace << "image " << index << " 0 " << round << "\n";
            addTrainingExamples(labeledImage.image, Annotations(landmarks), initial);
            if (trainingParams.mirrorTrainingData) {
                std::vector<imageio::RectLandmark> mirrored;
                mirrored.reserve(landmarks.size());
                for (const imageio::RectLandmark& landmark : landmarks) mirrored.push_back(flipHorizontally(landmark, labeledImage.image.cols));
                if (trace) *trace << "image " << index << " 1 " << round << "\n";
                addTrainingExamples(flipHorizontally(labeledImage.image), Annotations(mirrored), initial);
            }
        }
    }

    void addTrainingExamples(const cv::Mat& image, const Annotations& annotations, bool initial) {
        imageSize = cv::Size(image.cols, image.rows);
        featureExtractor->update(image);
        if (initial) {
            addPositiveExamples(annotations.positives);
            addRandomNegativeExamples(annotations.nonNegatives);
        } else {
            addHardNegativeExamples(annotations.nonNegatives);
        }
    }

    void tracePatch(const char* kind, cv::Rect box, int accepted, const std::shared_ptr<imageprocessing::Patch>& patch) {
        if (!trace) return;
        *trace << kind << " " << box.x << " " << box.y << " " << box.width << " " << box.height;
        if (accepted >= 0) *trace << " " << accepted;
        if (patch) {
            const cv::Rect b = patch->getBounds();
            *trace << " 1 " << b.x << " " << b.y << " " << b.width << " " << b.height << "\n";
        } else {
            *trace << " 0\n";
        }
    }

    void addPositiveExamples(const std::vector<cv::Rect>& positiveBoxes) {
        const std::vector<std::shared_ptr<imageprocessing::Patch>> patches = featureExtractor->extract(positiveBoxes);   // one launch per image
        for (size_t k = 0; k < patches.size(); ++k) {
            if (patches[k]) positiveTrainingExamples.push_back(patches[k]->getData());
            tracePatch("positive", positiveBoxes[k], -1, patches[k]);
        }
    }

    void addRandomNegativeExamples(const std::vector<cv::Rect>& nonNegativeBoxes) {
        int addedCount = 0;
        long rejected = 0;
        const long maxRejected = (long)trainingParams.maxRejectedDrawsPerNegative * std::max(trainingParams.randomNegativesPerImage, 1);
        while (addedCount < trainingParams.randomNegativesPerImage) {
            if (addNegativeIfNotOverlapping("random", createRandomBounds(imageSize), nonNegativeBoxes)) ++addedCount;
            else if (++rejected > maxRejected)
                throw std::runtime_error("DetectorTrainer: no random negative found in " + std::to_string(rejected) +
                                         " draws (do the annotations cover the image?)");
        }
    }

    // the first maxHardNegativesPerImage windows, in the detector's candidate order (NonMaximumSuppression(1.0) returns its input as
    // it is), that pass the overlap test after re-extraction
    void addHardNegativeExamples(const std::vector<cv::Rect>& nonNegativeBoxes) {
        const auto detections = featureExtractor->detectWindows(*classifier->getSvm(), trainingParams.negativeScoreThreshold);
        auto detection = detections.begin();
        int addedCount = 0;
        while (detection != detections.end() && addedCount < trainingParams.maxHardNegativesPerImage) {
            if (addNegativeIfNotOverlapping("hard", detection->first, nonNegativeBoxes)) ++addedCount;
            ++detection;
        }
    }

    bool addNegativeIfNotOverlapping(const char* kind, cv::Rect candidate, const std::vector<cv::Rect>& nonNegativeBoxes) {
        const std::shared_ptr<imageprocessing::Patch> patch = featureExtractor->extract(candidate);
        const bool accepted = patch && !isOverlapping(patch->getBounds(), nonNegativeBoxes);
        tracePatch(kind, candidate, accepted ? 1 : 0, patch);
        if (!accepted) return false;
        negativeTrainingExamples.push_back(patch->getData());
        return true;
    }

    void trainClassifier(bool initial) {
        if (printProgressInformation) {
            if (initial)
                std::cout << printPrefix << "training classifier (with " << positiveTrainingExamples.size() << " positives and "
                          << negativeTrainingExamples.size() << " negatives)" << std::endl;
            else
                std::cout << printPrefix << "re-training classifier (found " << negativeTrainingExamples.size() << " potential new negatives)" << std::endl;
        }
        const bool trains = !positiveTrainingExamples.empty() || !negativeTrainingExamples.empty();
        if (!classifier->retrain(positiveTrainingExamples, negativeTrainingExamples))
            throw std::runtime_error("DetectorTrainer: SVM is not usable after training");
        if (classifier->getSvm()->getSupportVectors().size() != 1)   // should never happen because of the linear kernel
            throw std::runtime_error("DetectorTrainer: the amount of support vectors has to be one (w)");
        if (trace && trains) {
            char buf[64];
            const fd_svm_train_info& info = classifier->getLastTrainingInfo();
            std::snprintf(buf, sizeof(buf), "%a", info.rho);
            *trace << "training " << (initial ? 1 : 0) << " " << classifier->getLastPositiveCount() << " " << classifier->getLastNegativeCount() << " "
                   << positiveTrainingExamples.size() << " " << negativeTrainingExamples.size() << " " << info.iterations << " " << buf << "\n";
            const cv::Mat w = getWeightVector();
            std::snprintf(buf, sizeof(buf), "%a", (double)classifier->getSvm()->getBias());
            *trace << "weights " << buf;
            const float* values = w.ptr<float>(0);
            for (size_t k = 0; k < w.total() * w.channels(); ++k) {
                std::snprintf(buf, sizeof(buf), "%a", (double)values[k]);
                *trace << " " << buf;
            }
            *trace << "\n";
        }
        positiveTrainingExamples.clear();
        negativeTrainingExamples.clear();
    }

    bool printProgressInformation;
    std::string printPrefix;
    FeatureParams featureParams;
    TrainingParams trainingParams;
    double aspectRatio, aspectRatioInv;
    std::shared_ptr<imageprocessing::ImageFilter> imageFilter, filter;
    std::shared_ptr<imageprocessing::extraction::AggregatedFeaturesExtractor> featureExtractor;
    std::shared_ptr<libsvm::LibSvmClassifier> classifier;
    std::mt19937 generator;
    cv::Size imageSize;
    std::vector<cv::Mat> positiveTrainingExamples, negativeTrainingExamples;
    std::ostream* trace = nullptr;
};
