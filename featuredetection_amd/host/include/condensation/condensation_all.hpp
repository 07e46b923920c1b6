// condensation/*.hpp of the reference (the measurement-model side of the particle filter) on top of the C ABI.
// the tracking-side caller of the WVM -> SVM path.
#pragma once
#include <memory>
#include <random>
#include <vector>
#include "classification/classification_all.hpp"
#include "imageprocessing/imageprocessing_all.hpp"

namespace condensation {

// Sample.hpp:30-330 (position, size, velocity, weight, target flag; the fields the measurement model touches)
class Sample {
public:
    Sample() : x(0), y(0), size(0), vx(0), vy(0), vsize(1), weight(1), target(false), clusterId(getNextClusterId()) {}
    Sample(int x, int y, int size) : x(x), y(y), size(size), vx(0), vy(0), vsize(1), weight(1), target(false), clusterId(getNextClusterId()) {}
    Sample(int x, int y, int size, int vx, int vy, float vsize)
        : x(x), y(y), size(size), vx(vx), vy(vy), vsize(vsize), weight(1), target(false), clusterId(getNextClusterId()) {}
    cv::Rect getBounds() const { return cv::Rect(x - getWidth() / 2, y - getHeight() / 2, getWidth(), getHeight()); }
    int getX() const { return x; }
    void setX(int v) { x = v; }
    int getY() const { return y; }
    void setY(int v) { y = v; }
    int getSize() const { return size; }
    void setSize(int v) { size = v; }
    int getWidth() const { return size; }
    int getHeight() const { return cv::cvRound(Sample::aspectRatio * size); }
    int getVx() const { return vx; }
    void setVx(int v) { vx = v; }
    int getVy() const { return vy; }
    void setVy(int v) { vy = v; }
    float getVSize() const { return vsize; }
    void setVSize(float v) { vsize = v; }
    double getScore() const { return score; }
    void setScore(double s) { score = s; }
    int getClusterId() const { return clusterId; }
    void setClusterId(int id) { clusterId = id; }
    void resetAncestor() {}   // ancestors belong to the adaptation half (Sample.hpp:256-258), which is not kept here
    double getWeight() const { return weight; }
    void setWeight(double w) { weight = w; }
    bool isTarget() const { return target; }
    void setTarget(bool t) { target = t; }
    static void setAspectRatio(double ratio) { Sample::aspectRatio = ratio; }
    static void setAspectRatio(int width, int height) { setAspectRatio(static_cast<double>(height) / static_cast<double>(width)); }   // Sample.hpp:317-319
    static double getAspectRatio() { return Sample::aspectRatio; }
    static int getNextClusterId() { return nextClusterId++; }
    static double aspectRatio;   // Sample.cpp:12
    static int nextClusterId;    // Sample.cpp:13
private:
    int x, y, size, vx, vy;
    float vsize;
    double weight;
    bool target;
    double score = 0;
    int clusterId;
};

// MeasurementModel.hpp:25-56
class MeasurementModel {
public:
    virtual ~MeasurementModel() {}
    virtual void update(std::shared_ptr<imageprocessing::VersionedImage> image) = 0;
    virtual void evaluate(Sample& sample) const = 0;
    virtual void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) {
        update(image);
        for (std::shared_ptr<Sample> sample : samples) evaluate(*sample);
    }
};

// WvmSvmModel.hpp / WvmSvmModel.cpp:36-118.  With a DirectPyramidFeatureExtractor + HistEq64Filter all samples are
// scored in one call of fd_wvm_svm_evaluate_samples.
class WvmSvmModel : public MeasurementModel {
public:
    WvmSvmModel(std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor, std::shared_ptr<classification::ProbabilisticWvmClassifier> wvm,
                std::shared_ptr<classification::ProbabilisticSvmClassifier> svm);
    void update(std::shared_ptr<imageprocessing::VersionedImage> image) override;
    void evaluate(Sample& sample) const override;
    void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) override;
private:
    std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor;
    std::shared_ptr<classification::ProbabilisticWvmClassifier> wvm;
    std::shared_ptr<classification::ProbabilisticSvmClassifier> svm;
};

// SingleClassifierModel.hpp:30-69 / SingleClassifierModel.cpp:22-63: one feature extractor, one probabilistic classifier.  The
// batched evaluate(image, samples) scores all samples with one fd_integral_svm_evaluate_samples when the extractor is a
// DirectImageFeatureExtractor with the chain of createHaarExtractor or createSurfExtractor (BenchmarkRunner.cpp:202-233,278-286) and
// the classifier a ProbabilisticSvmClassifier on f32 vectors; any other combination runs the per-sample loop.  (The reference's
// result cache per patch is not kept: the results are the same.)  getFusedEvaluationCount / getLoopEvaluationCount (not in the
// reference) tell which of the two ran: the results do not.
class SingleClassifierModel : public MeasurementModel {
public:
    SingleClassifierModel(std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor, std::shared_ptr<classification::ProbabilisticClassifier> classifier);
    void update(std::shared_ptr<imageprocessing::VersionedImage> image) override;
    void evaluate(Sample& sample) const override;
    void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) override;
    // calls of evaluate(image, samples) that scored their samples with one fd_integral_svm_evaluate_samples / with the per-sample loop
    int getFusedEvaluationCount() const { return fusedEvaluations; }
    int getLoopEvaluationCount() const { return loopEvaluations; }
private:
    std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor;
    std::shared_ptr<classification::ProbabilisticClassifier> classifier;
    int fusedEvaluations = 0, loopEvaluations = 0;
};

// ExtendedHogBasedMeasurementModel.hpp / .cpp:60-742, the evaluation half, on one fd_ehog_tracker: update, evaluate(image, samples) with
// the re-initialisation branches and targetLost, evaluate(Sample&), isValid, getHeatPeak, createGoodNegativeExamples, the setters and
// the cell-grid rule of initialize.  With the constructor that takes a ProbabilisticSvmClassifier initialize / adapt do not retrain (the one
// deviation); they take the weight vector and the bias from the classifier, which must hold a LinearKernel and one support
// vector of cellRowCount * cellColumnCount * channels values.  With the reference's constructor (a TrainableProbabilisticSvmClassifier)
// initialize is :321-384 and adapt :386-419 with adaptation NONE, POSITION and TRAJECTORY; CORRECTED_TRAJECTORY throws std::runtime_error.  The batched evaluate scores all samples with one fd_ehog_tracker_evaluate_samples
// (sliding window) or one fd_ehog_tracker_extract_patches (no sliding window); getFusedEvaluationCount (not in the reference) counts them.
class ExtendedHogBasedMeasurementModel : public MeasurementModel {
public:
    enum class Adaptation { NONE, POSITION, TRAJECTORY, CORRECTED_TRAJECTORY };
    explicit ExtendedHogBasedMeasurementModel(std::shared_ptr<classification::ProbabilisticSvmClassifier> classifier);
    // the reference's constructor (:60-75): initialize / adapt create training examples and retrain the classifier (see below)
    explicit ExtendedHogBasedMeasurementModel(std::shared_ptr<classification::TrainableProbabilisticSvmClassifier> trainable);
    ~ExtendedHogBasedMeasurementModel();
    ExtendedHogBasedMeasurementModel(const ExtendedHogBasedMeasurementModel&) = delete;
    ExtendedHogBasedMeasurementModel& operator=(const ExtendedHogBasedMeasurementModel&) = delete;
    void update(std::shared_ptr<imageprocessing::VersionedImage> image) override;
    void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) override;
    void evaluate(Sample& sample) const override;
    bool isValid(const Sample& target, const std::vector<std::shared_ptr<Sample>>& samples, std::shared_ptr<imageprocessing::VersionedImage> image);
    bool isUsable() const { return usable; }
    bool initialize(std::shared_ptr<imageprocessing::VersionedImage> image, Sample& target);
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples, const Sample& target);
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples);
    void reset();
    std::pair<double, cv::Rect> getHeatPeak() const;
    // the examples (cellRowCount x cellColumnCount * channels CV_32F each) and, optionally, their bounds in the order they were chosen
    std::vector<cv::Mat> createGoodNegativeExamples(cv::Rect targetBounds, std::vector<cv::Rect>* bounds = nullptr) const;
    // :671-692: windows of random width and position that overlap the target by less than positiveOverlapThreshold, drawn from the
    // model's std::mt19937 (default seed); extracted like the model's negatives (cells with the sliding window, patches without)
    std::vector<cv::Mat> createRandomNegativeExamples(size_t count, const cv::Mat& image, cv::Rect targetBounds, std::vector<cv::Rect>* bounds = nullptr) const;
    // not in the reference: what every retraining of initialize / adapt was given, in order -- the positive samples {x, y, width,
    // height} (centre form, extracted as patches) and the bounds of the negative examples -- so that a caller can follow it
    struct TrainingRecord {
        std::vector<cv::Rect> positives, negatives;
    };
    const std::vector<TrainingRecord>& getTrainingLog() const { return trainingLog; }
    void setHogParams(size_t cellSize, size_t cellCount, bool signedAndUnsigned, bool interpolateBins, bool interpolateCells, int octaveLayerCount);
    void setRejectionThreshold(double rejectionThreshold) { this->rejectionThreshold = rejectionThreshold; }
    void setUseSlidingWindow(bool useSlidingWindow, bool conservativeReInit) { this->useSlidingWindow = useSlidingWindow; this->conservativeReInit = conservativeReInit; }
    void setNegativeExampleParams(size_t negativeExampleCount, size_t initialNegativeExampleCount, size_t randomExampleCount, float negativeScoreThreshold);
    void setOverlapThresholds(double positiveOverlapThreshold, double negativeOverlapThreshold);
    void setAdaptation(Adaptation adaptation, double adaptationThreshold, double exclusionThreshold);
    // the cell-grid rule of initialize (:221-228): columns and rows for a target of width x height and about cellCount cells
    static void computeCellGrid(int width, int height, size_t cellCount, size_t& cellColumnCount, size_t& cellRowCount);
    size_t getCellColumnCount() const { return cellColumnCount; }
    size_t getCellRowCount() const { return cellRowCount; }
    bool isTargetLost() const { return targetLost; }
    int getFusedEvaluationCount() const { return fusedEvaluations; }
    fd_ehog_tracker* native() const { return tracker; }
private:
    void takeClassifierWeights();
    void setTrainingTarget(fd_ehog_tracker* target);
    bool retrain(const std::vector<cv::Mat>& positives, const std::vector<cv::Mat>& negatives, const std::vector<cv::Rect>& positiveSamples,
                 const std::vector<cv::Rect>& negativeBounds);
    std::vector<cv::Mat> createPositiveTrainingExamples(const Sample& target, std::vector<cv::Rect>& samplesUsed);
    std::vector<cv::Mat> createNegativeTrainingExamples(const cv::Mat& image, cv::Rect targetBounds, std::vector<cv::Rect>& bounds) const;
    cv::Rect createRandomBounds(const cv::Mat& image) const;
    bool extractPositive(const Sample& target, cv::Mat& features, double* score) const;
    void evaluateAll(std::vector<std::shared_ptr<Sample>>& samples, double* bestScore);
    void scored(Sample& sample, bool valid, double score) const;
    double computeOverlap(cv::Rect a, cv::Rect b) const;
    size_t cellSize, cellCount;
    bool signedAndUnsigned, interpolateBins, interpolateCells;
    int octaveLayerCount;
    double rejectionThreshold;
    bool useSlidingWindow, conservativeReInit;
    size_t negativeExampleCount, initialNegativeExampleCount, randomExampleCount;
    float negativeScoreThreshold;
    double positiveOverlapThreshold, negativeOverlapThreshold;
    Adaptation adaptation;
    double adaptationThreshold, exclusionThreshold;
    std::shared_ptr<classification::ProbabilisticSvmClassifier> classifier;
    std::shared_ptr<classification::TrainableProbabilisticSvmClassifier> trainable;   // null with the first constructor
    std::vector<cv::Mat> trajectoryFeatures;
    std::vector<cv::Rect> trajectorySamples;
    std::vector<TrainingRecord> trainingLog;
    bool trainsOnHandle = false;   // the trainable's SVM is a LibSvmClassifier that trains on `tracker` (fd_ehog_tracker_train_svm)
    fd_ehog_tracker* tracker = nullptr;
    size_t cellRowCount = 0, cellColumnCount = 0, minWidth = 0, maxWidth = 0;
    bool initialized = false, usable = false, targetLost = false;
    mutable std::mt19937 generator;
    mutable std::normal_distribution<> normalDistribution;
    cv::Mat initialFeatures;
    int fusedEvaluations = 0;
};

}  // namespace condensation
