// condensation/*.hpp of the reference (the measurement-model side of the particle filter) on top of the C ABI.
// the tracking-side caller of the WVM -> SVM path.
#pragma once
#include <memory>
#include <optional>
#include <random>
#include <vector>
#include "classification/classification_all.hpp"
#include "imageprocessing/imageprocessing_all.hpp"

namespace boost { using std::optional; }   // the trackers return boost::optional<cv::Rect>; std::optional reads the same

namespace condensation {

// Sample.hpp:30-330 (position, size, velocity, weight, target flag; the fields the measurement model touches)
class Sample {
public:
    Sample() : x(0), y(0), size(0), vx(0), vy(0), vsize(1), weight(1), target(false), clusterId(getNextClusterId()) {}
    Sample(int x, int y, int size) : x(x), y(y), size(size), vx(0), vy(0), vsize(1), weight(1), target(false), clusterId(getNextClusterId()) {}
    Sample(int x, int y, int size, int vx, int vy, float vsize)
        : x(x), y(y), size(size), vx(vx), vy(vy), vsize(vsize), weight(1), target(false), clusterId(getNextClusterId()) {}
    // a descendant (Sample.hpp:64-66): the parent's values and cluster, score 0, no target flag
    explicit Sample(std::shared_ptr<Sample> other, double weight = 1)
        : x(other->x), y(other->y), size(other->size), vx(other->vx), vy(other->vy), vsize(other->vsize), weight(weight), target(false),
          clusterId(other->clusterId), ancestor(other) {}
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
    const std::shared_ptr<Sample> getAncestor() const { return ancestor; }
    void setAncestor(std::shared_ptr<Sample> a) { ancestor = a; }
    void resetAncestor() { ancestor.reset(); }
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
    std::shared_ptr<Sample> ancestor;
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

// AdaptiveMeasurementModel.hpp:25-83
class AdaptiveMeasurementModel : public MeasurementModel {
public:
    using MeasurementModel::evaluate;
    virtual ~AdaptiveMeasurementModel() {}
    virtual bool isUsable() const = 0;
    virtual bool initialize(std::shared_ptr<imageprocessing::VersionedImage> image, Sample& target) = 0;
    virtual bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples, const Sample& target) = 0;
    virtual bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples) = 0;
    virtual void reset() = 0;
};

// StateValidator.hpp:24-40
class StateValidator {
public:
    virtual ~StateValidator() {}
    virtual bool isValid(const Sample& target, const std::vector<std::shared_ptr<Sample>>& samples, std::shared_ptr<imageprocessing::VersionedImage> image) = 0;
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
    // Not in the reference.  Whether the model has a resident evaluation right now: the extractor is a
    // DirectPyramidFeatureExtractor with a HistEq64Filter on a gray pyramid (what evaluate(image, samples) needs), also behind at most
    // FD_SAMPLE_MAPS_MAX PatchResizingFeatureExtractors, its pyramid holds an image, has at most 64 layers and a width -> layer table that
    // fits FD_SAMPLE_TABLE_MAX.  About what the extractor holds now, as SingleClassifierModel::residentPlan
    bool residentPossible() const;
    // evaluate(image, samples) for a generation that lives in `particles`: update, fd_particles_evaluate_wvm_svm, fd_particles_weigh_wvm_svm,
    // nothing copied back.  logic_error where residentPossible() does not hold after the update
    void evaluateResident(std::shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles);
    // calls of evaluate(image, samples) / evaluateResident, each one set of device calls for all samples, and calls of evaluate(sample)
    int getFusedEvaluationCount() const { return fusedEvaluations; }
    int getLoopEvaluationCount() const { return loopEvaluations; }
private:
    std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor;
    std::shared_ptr<classification::ProbabilisticWvmClassifier> wvm;
    std::shared_ptr<classification::ProbabilisticSvmClassifier> svm;
    int fusedEvaluations = 0;
    mutable int loopEvaluations = 0;
};

// Not in the reference: how the models below score the samples of an extractor with a sampled chain (imageprocessing::SampledChain,
// resolved by sampledChainOf) in one device call.  sampledClassifierOf resolves the classifier once: svm is the
// ProbabilisticSvmClassifier (also the one behind a TrainableProbabilisticSvmClassifier) when it works on f32 vectors, rvm the
// ProbabilisticRvmClassifier.  sampledRoute asks no device: Svm for any chain with such an SVM (SampledChain::svmEvaluate), PatchRvm for a
// gray-patch chain with an RVM (fd_patch_rvm_evaluate_samples), Loop for everything else.
struct SampledClassifier {
    const classification::ProbabilisticSvmClassifier* svm;
    classification::ProbabilisticRvmClassifier* rvm;
};
enum class SampledRoute { Loop, Svm, PatchRvm };
SampledClassifier sampledClassifierOf(classification::ProbabilisticClassifier* classifier);
SampledRoute sampledRoute(const imageprocessing::SampledChain& chain, const SampledClassifier& classifier);

// SingleClassifierModel.hpp:30-69 / SingleClassifierModel.cpp:22-63: one feature extractor, one probabilistic classifier.  The
// batched evaluate(image, samples) scores all samples in one device call where sampledRoute finds one for the extractor's chain and the
// classifier and the chain is ready (an integral image exists); any other combination runs the per-sample loop.  With an RVM the
// verdict and the probability are the classifier's own getProbability(level, distance).  (The reference's result cache per patch is
// not kept: the results are the same.)  getFusedEvaluationCount / getLoopEvaluationCount (not in the reference) tell which of the two
// ran: the results do not.
class SingleClassifierModel : public MeasurementModel {
public:
    SingleClassifierModel(std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor, std::shared_ptr<classification::ProbabilisticClassifier> classifier);
    void update(std::shared_ptr<imageprocessing::VersionedImage> image) override;
    void evaluate(Sample& sample) const override;
    void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) override;
    // calls of evaluate(image, samples) that scored their samples with one fd_integral_svm_evaluate_samples / with the per-sample loop
    int getFusedEvaluationCount() const { return fusedEvaluations; }
    int getLoopEvaluationCount() const { return loopEvaluations; }
    std::shared_ptr<imageprocessing::FeatureExtractor> getFeatureExtractor() const { return featureExtractor; }
    std::shared_ptr<classification::ProbabilisticClassifier> getClassifier() const { return classifier; }
    // evaluate(image, samples) for a generation that lives in `particles`: update, then one
    // fd_particles_evaluate_integral or fd_particles_evaluate_pyramid and one fd_particles_weigh_classifier, nothing copied back.  It
    // resolves its own plan after the update; logic_error where that plan is None
    void evaluateResident(std::shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles);
    // Which resident evaluation the model has right now, resolved once.  The classifier is a (Trainable)ProbabilisticSvmClassifier on f32
    // vectors and the extractor resolves to a chain with at most FD_SAMPLE_MAPS_MAX wrappers that is ready.  Integral: a Haar, SURF or
    // integral HOG chain.  Pyramid: a DirectPyramidFeatureExtractor with a histogram, extended HOG or gray-patch chain behind
    // PatchResizingFeatureExtractors only, on a pyramid that holds an image and whose width -> layer table fits FD_SAMPLE_TABLE_MAX.
    // The answer is about what the extractor holds now: update(image) can change it (the first image of a pyramid, another layer count)
    struct ResidentPlan {
        enum class Family { None, Integral, Pyramid } family;
        imageprocessing::SampledChain chain;   // resolved with mapsApplied
        SampledClassifier scorer;
        const std::vector<fd_sample_map>& maps() const { return chain.wrappers.sampleMaps(); }
    };
    ResidentPlan residentPlan() const;
private:
    std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor;
    std::shared_ptr<classification::ProbabilisticClassifier> classifier;
    int fusedEvaluations = 0, loopEvaluations = 0;
};

// FilteringClassifierModel.hpp / FilteringClassifierModel.cpp:27-103: a binary classifier on features of its own in front of (RESET_WEIGHT)
// or behind (KEEP_WEIGHT) a measurement model.  RESET_WEIGHT: a sample that does not pass the filter (no patch included) gets target
// false and weight 0 and never reaches the model.  KEEP_WEIGHT: the model evaluates every sample; a sample it marked as target loses the
// flag when it does not pass the filter, and keeps its weight.  The batched evaluate asks the filter once for all samples it concerns
// (fd_patch_rvm_evaluate_samples) when the filter is an RvmClassifier or a ProbabilisticRvmClassifier and the chain of the filter's
// extractor a gray-patch one, and hands the model the passing samples in one batched evaluate (RESET_WEIGHT; KEEP_WEIGHT: all samples
// first); anything else asks per sample.  Targets and weights do not depend on the route.  (The reference's result cache per patch is
// not kept: the results are the same.)  getFusedFilterCount / getLoopFilterCount (not in the reference) count the batched evaluate
// calls by the route their filter took.
class FilteringClassifierModel : public MeasurementModel {
public:
    enum class Behavior { RESET_WEIGHT, KEEP_WEIGHT };
    FilteringClassifierModel(std::shared_ptr<imageprocessing::FeatureExtractor> filterFeatureExtractor, std::shared_ptr<classification::BinaryClassifier> filter,
                             std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor, std::shared_ptr<classification::ProbabilisticClassifier> classifier,
                             Behavior behavior);
    FilteringClassifierModel(std::shared_ptr<imageprocessing::FeatureExtractor> filterFeatureExtractor, std::shared_ptr<classification::BinaryClassifier> filter,
                             std::shared_ptr<MeasurementModel> measurementModel, Behavior behavior);
    void update(std::shared_ptr<imageprocessing::VersionedImage> image) override;
    void evaluate(Sample& sample) const override;
    void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) override;
    int getFusedFilterCount() const { return fusedFilters; }
    int getLoopFilterCount() const { return loopFilters; }
    std::shared_ptr<MeasurementModel> getMeasurementModel() const { return measurementModel; }
private:
    bool passesFilter(const Sample& sample) const;
    // the filter's verdict for every sample of the list: one device call when the route allows it (true), else per sample (false)
    bool passFilter(const std::vector<std::shared_ptr<Sample>>& samples, std::vector<char>& passes) const;
    Behavior behavior;
    std::shared_ptr<MeasurementModel> measurementModel;
    std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor;
    std::shared_ptr<classification::BinaryClassifier> filter;
    int fusedFilters = 0, loopFilters = 0;
};

// ClassificationBasedStateValidator.hpp / .cpp:28-45: the state is valid when the classifier accepts one window of a small grid around
// it -- for every size factor size = round(factor * target size), for every x displacement x = target x + round(displacement * size),
// for every y displacement likewise (std::round: half-way cases away from zero), in that order.  With an RvmClassifier (or a
// ProbabilisticRvmClassifier) on an extractor with a gray-patch chain the whole grid is one fd_patch_rvm_evaluate_samples and the verdict
// is any(target); otherwise the windows are asked one by one up to the first accepted.
// getLastCandidates (not in the reference) returns the grid of the last call as Rect(x, y, size, size): centre and size, not bounds.
class ClassificationBasedStateValidator : public StateValidator {
public:
    ClassificationBasedStateValidator(std::shared_ptr<imageprocessing::FeatureExtractor> extractor, std::shared_ptr<classification::BinaryClassifier> classifier,
                                      std::vector<double> sizes = {1}, std::vector<double> displacements = {0});
    bool isValid(const Sample& target, const std::vector<std::shared_ptr<Sample>>& samples, std::shared_ptr<imageprocessing::VersionedImage> image) override;
    const std::vector<cv::Rect>& getLastCandidates() const { return lastCandidates; }
    int getFusedValidationCount() const { return fusedValidations; }
    int getLoopValidationCount() const { return loopValidations; }
private:
    std::shared_ptr<imageprocessing::FeatureExtractor> extractor;
    std::shared_ptr<classification::BinaryClassifier> classifier;
    std::vector<double> sizes, displacements;
    std::vector<cv::Rect> lastCandidates;
    int fusedValidations = 0, loopValidations = 0;
};

// PositionDependentMeasurementModel.hpp / .cpp:28-274: a measurement model that learns its classifier from the target position --
// the frame counters, the target-threshold gate, 1 or 5 positives, 6 / 18 / 26 negatives around the target, the weight-ordered
// additional negatives taken from the particles, random negatives and random test negatives, the confidence-filtered retrain
// against the unfiltered one, exploitSymmetry (cv::flip(.., 1) of the patch data).
// Not the reference's: a std::mt19937(seed) constructor argument replaces the default-constructed boost::mt19937, and
// distribution(generator, n) is (uint64(engine()) * n) >> 32 -- one 32-bit draw per call, the result in [0, n); n <= 0 throws
// invalid_argument (undefined in the reference).  With an extractor whose chain is extractable (SampledChain: the pyramid kinds, and
// integral HOG once an integral image exists) every sample set of one adapt (positives, negatives, test negatives) is extracted in
// one device call (SampledChain::extract), whether a random sample has a window is decided on the host by the rule of the kernels
// (SampledChain::hasWindow), and with a (Trainable)ProbabilisticSvm classifier the confidence predicates score all vectors of a set
// in one call.  exploitSymmetry mirrors patch data as cv::flip(.., 1) mirrors the reference's Mat: an ExtendedHogFilter descriptor is
// rows x cols cells of bins (+ bins / 2) + 4 channels there and rows x cols * channels CV_32FC1 here, so for a
// DirectPyramidFeatureExtractor on an ehog chain (also behind a PatchResizingFeatureExtractor) the cells of a row change places and
// every cell keeps its channel order; all other patch data is flipped element by element, which is the reference's result for
// single-channel data (an ExtendedHogFilter reached through any other extractor type is not recognised).
// getLastAdaptation / getAdaptationCount (not in the reference) tell what the last adapt that reached a retraining chose.
class PositionDependentMeasurementModel : public AdaptiveMeasurementModel {
public:
    PositionDependentMeasurementModel(std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor,
                                      std::shared_ptr<classification::TrainableProbabilisticClassifier> classifier,
                                      unsigned int seed = std::mt19937::default_seed);
    PositionDependentMeasurementModel(std::shared_ptr<MeasurementModel> measurementModel, std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor,
                                      std::shared_ptr<classification::TrainableProbabilisticClassifier> classifier,
                                      unsigned int seed = std::mt19937::default_seed);
    void update(std::shared_ptr<imageprocessing::VersionedImage> image) override;
    void evaluate(Sample& sample) const override;
    void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) override;
    bool isUsable() const override { return usable; }
    void reset() override;
    bool initialize(std::shared_ptr<imageprocessing::VersionedImage> image, Sample& target) override;
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples, const Sample& target) override;
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples) override;
    void setFrameCounts(unsigned int startFrameCount = 3, unsigned int stopFrameCount = 0) {
        this->startFrameCount = startFrameCount;
        this->stopFrameCount = stopFrameCount;
    }
    void setThresholds(float targetThreshold = 0.7f, float confidenceThreshold = 0.95f) {
        this->targetThreshold = targetThreshold;
        this->confidenceThreshold = confidenceThreshold;
    }
    void setOffsetFactors(float positiveOffsetFactor = 0.05f, float negativeOffsetFactor = 0.5f) {
        this->positiveOffsetFactor = positiveOffsetFactor;
        this->negativeOffsetFactor = negativeOffsetFactor;
    }
    void setSamplingProperties(unsigned int sampleNegativesAroundTarget = 0, unsigned int sampleAdditionalNegatives = 10,
                               unsigned int sampleTestNegatives = 10, bool exploitSymmetry = false) {
        this->sampleNegativesAroundTarget = sampleNegativesAroundTarget;
        this->sampleAdditionalNegatives = sampleAdditionalNegatives;
        this->sampleTestNegatives = sampleTestNegatives;
        this->exploitSymmetry = exploitSymmetry;
    }
    // not in the reference: the samples {x, y, size} the last adapt that reached a retraining chose and the vectors it passed on (the
    // Mats share their buffers with the classifier's examples); one record is kept, getAdaptationCount counts the retrainings
    struct AdaptationRecord {
        std::vector<cv::Rect> positives, negatives, testNegatives;   // Rect(x, y, size, size): centre and size, not bounds
        std::vector<cv::Mat> positiveVectors, negativeVectors;
    };
    const AdaptationRecord& getLastAdaptation() const { return lastAdaptation; }
    size_t getAdaptationCount() const { return adaptationCount; }
    std::shared_ptr<MeasurementModel> getMeasurementModel() const { return measurementModel; }
    // not in the reference: adapt(image, samples, target) in its two parts, for a generation that lives on the device.
    // The samples are read for one thing, the sampleAdditionalNegatives samples with the largest weights outside the box around the
    // target (:172-192): chooseAdditionalNegatives makes that choice on the host, fd_particles_state_negatives on the device.
    // adaptResident is adapt with the choice already made (`chosen` in the list's order, at most sampleAdditionalNegatives samples);
    // adapt itself is adaptResident(image, target, chooseAdditionalNegatives(samples, target)), so both routes draw the same random
    // samples and pass the same examples on in the same order.
    std::vector<Sample> chooseAdditionalNegatives(const std::vector<std::shared_ptr<Sample>>& samples, const Sample& target) const;
    bool adaptResident(std::shared_ptr<imageprocessing::VersionedImage> image, const Sample& target, const std::vector<Sample>& chosen);
    // what fd_particles_state_negatives needs for this model's choice: {sampleAdditionalNegatives, negativeOffsetFactor, 1 - factor,
    // 1 / (1 - factor)}, the floats as adapt forms them.  False where the device is not asked: sampleAdditionalNegatives is 0 (nothing is
    // read from the samples) or above FD_PARTICLES_NEGATIVES_MAX, or a bound is not finite.
    bool residentNegatives(fd_particles_negatives_params& params) const;
private:
    // the box around the target: {xLow, xHigh, yLow, yHigh, sizeLow, sizeHigh} (fd_particles_negatives_bounds)
    struct NegativeBounds {
        int32_t v[6];
        bool outside(const Sample& s) const {
            return s.getX() <= v[0] || s.getX() >= v[1] || s.getY() <= v[2] || s.getY() >= v[3] || s.getSize() <= v[4] || s.getSize() >= v[5];
        }
    };
    NegativeBounds negativeBounds(const Sample& target) const;
    int draw(int n);   // distribution(generator, n)
    Sample createRandomSample(const cv::Mat& image);
    bool hasWindow(int x, int y, int width, int height) const;
    // the patch data of every sample that has a patch; square: extracted with (size, size) as the random samples are
    std::vector<cv::Mat> extractAll(const std::vector<Sample>& samples, bool square) const;
    std::vector<double> probabilities(const std::vector<cv::Mat>& vectors) const;
    std::vector<cv::Mat> getFeatureVectors(const std::vector<Sample>& samples, int predicate /* 0 all, 1 positives, 2 negatives */) const;
    std::mt19937 generator;
    std::shared_ptr<MeasurementModel> measurementModel;
    std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor;
    std::shared_ptr<classification::TrainableProbabilisticClassifier> classifier;
    bool usable;
    unsigned int frameCount, startFrameCount, stopFrameCount;
    float targetThreshold, confidenceThreshold, positiveOffsetFactor, negativeOffsetFactor;
    unsigned int sampleNegativesAroundTarget, sampleAdditionalNegatives, sampleTestNegatives;
    bool exploitSymmetry;
    AdaptationRecord lastAdaptation;
    size_t adaptationCount = 0;
};

// ExtendedHogBasedMeasurementModel.hpp / .cpp:60-742, the evaluation half, on one fd_ehog_tracker: update, evaluate(image, samples) with
// the re-initialisation branches and targetLost, evaluate(Sample&), isValid, getHeatPeak, createGoodNegativeExamples, the setters and
// the cell-grid rule of initialize.  With the constructor that takes a ProbabilisticSvmClassifier initialize / adapt do not retrain (the one
// deviation); they take the weight vector and the bias from the classifier, which must hold a LinearKernel and one support
// vector of cellRowCount * cellColumnCount * channels values.  With the reference's constructor (a TrainableProbabilisticSvmClassifier)
// initialize is :321-384 and adapt :386-419 with adaptation NONE, POSITION and TRAJECTORY; CORRECTED_TRAJECTORY throws std::runtime_error.  The batched evaluate scores all samples with one fd_ehog_tracker_evaluate_samples
// (sliding window) or one fd_ehog_tracker_extract_patches (no sliding window); getFusedEvaluationCount (not in the reference) counts them.
class ExtendedHogBasedMeasurementModel : public AdaptiveMeasurementModel, public StateValidator {
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
    bool isValid(const Sample& target, const std::vector<std::shared_ptr<Sample>>& samples, std::shared_ptr<imageprocessing::VersionedImage> image) override;
    bool isUsable() const override { return usable; }
    bool initialize(std::shared_ptr<imageprocessing::VersionedImage> image, Sample& target) override;
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples, const Sample& target) override;
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples) override;
    void reset() override;
    // not in the reference: evaluate(image, samples) for a particle set that lives on the device (fd_particles, bound to native()) -- the
    // same branches, re-initialisation draws and weights; the samples never visit the host unless a re-initialisation rewrites them.
    // Fills info with the extracted state (FilteringStateExtractor(WeightedMeanStateExtractor)); throws when a weight is not finite.
    void evaluateResident(std::shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles, fd_particles_info& info);
    Adaptation getAdaptation() const { return adaptation; }
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

// Sampler.hpp:24-48
// SelfLearningMeasurementModel.hpp / .cpp:26-133: a classifier that is retrained on the frame's own most and least confident samples,
// at most 10 per side.  evaluate is SingleClassifierModel's (target and weight, .cpp:53-74).  adapt picks the examples by the library's
// rule (fd_particles_examples_select, the comparisons k_particles_examples runs): while the model is usable only samples
// with a patch are examples, before that every sample is a candidate and the extraction decides; a side with more than 10 candidates
// keeps the best 10 in sorted order, equal weights to the lower index (the reference's std::sort is unstable).  The feature vectors go to
// retrain as 1 x n rows.  Thresholds with negativeThreshold > positiveThreshold are refused (std::invalid_argument).
class SelfLearningMeasurementModel : public AdaptiveMeasurementModel {
public:
    SelfLearningMeasurementModel(std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor,
                                 std::shared_ptr<classification::TrainableProbabilisticClassifier> classifier, double positiveThreshold = 0.85,
                                 double negativeThreshold = 0.05);
    void update(std::shared_ptr<imageprocessing::VersionedImage> image) override { model.update(image); }
    void evaluate(Sample& sample) const override { model.evaluate(sample); }
    void evaluate(std::shared_ptr<imageprocessing::VersionedImage> image, std::vector<std::shared_ptr<Sample>>& samples) override { model.evaluate(image, samples); }
    bool isUsable() const override { return usable; }
    bool initialize(std::shared_ptr<imageprocessing::VersionedImage>, Sample&) override { return false; }
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples, const Sample&) override {
        return adapt(image, samples);
    }
    bool adapt(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<std::shared_ptr<Sample>>& samples) override;
    void reset() override;
    // Not in the reference.  The resident evaluation is SingleClassifierModel's; readExamples updates the extractor with
    // the image and reads the state of the generation in `particles` through fd_particles_state_examples_*, with require_window =
    // isUsable(): the examples and their rows stay in the model until adaptResident, which ends in the retrain call adapt ends in.
    SingleClassifierModel::ResidentPlan residentPlan() const;   // while not usable: the extraction alone, no scoring classifier needed
    void evaluateResident(std::shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles) { model.evaluateResident(image, particles); }
    void readExamples(std::shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles, fd_particles_info& info);
    bool adaptResident(std::shared_ptr<imageprocessing::VersionedImage> image, const std::vector<fd_particles_example>& positives,
                       const std::vector<fd_particles_example>& negatives, const std::vector<float>& rows);
    bool adaptResident(std::shared_ptr<imageprocessing::VersionedImage> image) { return adaptResident(image, lastPositives, lastNegatives, lastRows); }
    // the examples of the last adaptation, in list order (valid: the sample had a patch and went to retrain)
    const std::vector<fd_particles_example>& getLastPositives() const { return lastPositives; }
    const std::vector<fd_particles_example>& getLastNegatives() const { return lastNegatives; }
private:
    fd_particles_examples_params examplesParams() const;
    SingleClassifierModel model;
    std::shared_ptr<imageprocessing::FeatureExtractor> featureExtractor;
    std::shared_ptr<classification::TrainableProbabilisticClassifier> classifier;
    double positiveThreshold, negativeThreshold;
    bool usable = false;
    std::vector<fd_particles_example> lastPositives, lastNegatives;
    std::vector<float> lastRows;
    int lastRowLength = 0;
};

class Sampler {
public:
    virtual ~Sampler() {}
    virtual void init(const cv::Mat& image) = 0;
    virtual void sample(const std::vector<std::shared_ptr<Sample>>& samples, std::vector<std::shared_ptr<Sample>>& newSamples, const cv::Mat& image,
                        const std::shared_ptr<Sample> target) = 0;
};

// ResamplingAlgorithm.hpp:22-38
class ResamplingAlgorithm {
public:
    virtual ~ResamplingAlgorithm() {}
    virtual void resample(const std::vector<std::shared_ptr<Sample>>& samples, size_t count, std::vector<std::shared_ptr<Sample>>& newSamples) = 0;
};

// LowVarianceSampling.hpp / .cpp:17-46.  The reference seeds a boost::mt19937 with time(0); here a std::mt19937 with `seed` and a
// std::uniform_real_distribution<> on [0, 1): one draw per resample call that has samples and a positive step.  Where rounding leaves
// the last pointers above the total weight the walk stops at the last sample (the reference increments its iterator past the end).
class LowVarianceSampling : public ResamplingAlgorithm {
public:
    explicit LowVarianceSampling(unsigned int seed = std::mt19937::default_seed);
    void resample(const std::vector<std::shared_ptr<Sample>>& samples, size_t count, std::vector<std::shared_ptr<Sample>>& newSamples) override;
    double computeWeightSum(const std::vector<std::shared_ptr<Sample>>& samples);
    // the next uniform number, as resample takes it; the last one is kept for replaying a run
    double draw() { lastDraw = distribution(generator); drew = true; return lastDraw; }
    bool hasLastDraw() const { return drew; }
    double getLastDraw() const { return lastDraw; }
    void forgetLastDraw() { drew = false; }
private:
    std::mt19937 generator;
    std::uniform_real_distribution<> distribution;
    double lastDraw = 0;
    bool drew = false;
};

// TransitionModel.hpp:24-49
class TransitionModel {
public:
    virtual ~TransitionModel() {}
    virtual void init(const cv::Mat& image) = 0;
    virtual void predict(std::vector<std::shared_ptr<Sample>>& samples, const cv::Mat& image, const std::shared_ptr<Sample> target) = 0;
};

// SimpleTransitionModel.hpp / .cpp:19-44.  std::mt19937(seed) + std::normal_distribution<>: three draws per sample, in the order x
// velocity, y velocity, size factor.
class SimpleTransitionModel : public TransitionModel {
public:
    explicit SimpleTransitionModel(double positionDeviation, double sizeDeviation, unsigned int seed = std::mt19937::default_seed);
    void init(const cv::Mat& image) override;
    void predict(std::vector<std::shared_ptr<Sample>>& samples, const cv::Mat& image, const std::shared_ptr<Sample> target) override;
    double getPositionDeviation() const { return positionDeviation; }
    void setPositionDeviation(double deviation) { positionDeviation = deviation; }
    double getSizeDeviation() const { return sizeDeviation; }
    void setSizeDeviation(double deviation) { sizeDeviation = deviation; }
    // the three draws of one sample as predict applies them: {positionDeviation * z, positionDeviation * z, pow(2, sizeDeviation * z)}
    void drawDiffusion(double out[3]);
    // predict for one sample with its draws (the arithmetic of k_particles_sample)
    static void apply(Sample& sample, const double diffusion[3]);
    const std::vector<double>& getLastDiffusion() const { return lastDiffusion; }   // the draws of the last predict, 3 per sample
    // the draws of a predict over `samples` samples without the samples: they become the last diffusion
    const std::vector<double>& drawBlock(size_t samples);
    // what the next draw depends on -- the distribution caches its second value, so it is part of the state -- and the last diffusion:
    // a device frame that drew a block it did not use puts the snapshot back
    struct DrawState {
        std::mt19937 generator;
        std::normal_distribution<> distribution;
        std::vector<double> lastDiffusion;
    };
    DrawState drawState() const { return DrawState{generator, distribution, lastDiffusion}; }
    void restoreDrawState(const DrawState& state) { generator = state.generator; distribution = state.distribution; lastDiffusion = state.lastDiffusion; }
private:
    std::vector<double> lastDiffusion;
    double positionDeviation, sizeDeviation;
    std::mt19937 generator;
    std::normal_distribution<> distribution;
};

// OpticalFlowTransitionModel.hpp / .cpp:27-191 on one fd_flow: the pyramids of the previous and the current frame
// live on the device, predict is fd_flow_update, fd_flow_track_fb (forward, then backward from the forward results) and
// fd_flow_median, then the motion of every sample on the host.  The fallback predicts exactly where the reference's does: no previous
// frame, no target, fewer than points / 2 pairs tracked both ways, fewer than points / 2 of them with a squared forward-backward
// distance of at most 0.5; the frame becomes the previous one before either of the late fallbacks, as in the reference.
// Not the reference's: std::mt19937(seed) + std::normal_distribution<> in place of boost::mt19937(time(0)) -- three draws per sample in
// the order x, y, size; pairs of equal forward-backward distance are ordered by point index (the reference's std::sort on the
// distance alone leaves them to the implementation); with fewer than two correct pairs (a grid of fewer than four points) the
// fallback predicts, where the reference indexes an empty vector; the flow handle is rebuilt when the frame size changes; drawFlow
// is left out (fdcompat has no drawing).  usedFlow / getLastMotion / getLastDraws tell what the last predict did.
class OpticalFlowTransitionModel : public TransitionModel {
public:
    explicit OpticalFlowTransitionModel(std::shared_ptr<TransitionModel> fallback, double positionDeviation, double sizeDeviation,
                                        cv::Size gridSize = cv::Size(10, 10), bool circle = true, cv::Size windowSize = cv::Size(15, 15), int maxLevel = 2,
                                        unsigned int seed = std::mt19937::default_seed);
    ~OpticalFlowTransitionModel();
    OpticalFlowTransitionModel(const OpticalFlowTransitionModel&) = delete;
    OpticalFlowTransitionModel& operator=(const OpticalFlowTransitionModel&) = delete;
    void init(const cv::Mat& image) override;
    void predict(std::vector<std::shared_ptr<Sample>>& samples, const cv::Mat& image, const std::shared_ptr<Sample> target) override;
    double getPositionDeviation() const { return positionDeviation; }
    void setPositionDeviation(double deviation) { positionDeviation = deviation; }
    double getSizeDeviation() const { return sizeDeviation; }
    void setSizeDeviation(double deviation) { sizeDeviation = deviation; }
    std::shared_ptr<TransitionModel> getFallback() const { return fallback; }
    const std::vector<cv::Point2f>& getTemplatePoints() const { return templatePoints; }
    const std::vector<cv::Point2f>& getPoints() const { return points; }                 // of the last predict; empty when it did not track
    // after a resident predict the tracks are still on the device: these three fetch them on demand (fd_flow_get_tracks)
    const std::vector<cv::Point2f>& getForwardPoints() const { fetchTracks(); return forwardPoints; }
    const std::vector<cv::Point2f>& getBackwardPoints() const { fetchTracks(); return backwardPoints; }
    // the point indices of the correct flows, ordered by forward-backward distance (squaredDistances[0 .. correctFlowCount) of the reference)
    const std::vector<int>& getCorrectFlowIndices() const { fetchTracks(); return correctFlowIndices; }
    bool usedFlow() const { return flowUsed; }                                           // the last predict moved the samples by the flow
    const fd_flow_motion& getLastMotion() const { return lastMotion; }                   // of the last predict; all zero when it did not track (order is not set)
    const std::vector<double>& getLastDraws() const { return lastDraws; }                // the normal draws of the last flow prediction, 3 per sample
    // predict for one sample with its three normal draws
    static void apply(Sample& sample, float medianX, float medianY, float medianRatio, double positionDeviation, double sizeDeviation, const double z[3]);
    // predict for a generation that lives on the device, in three steps.  residentPossible: the fallback is exactly a
    // SimpleTransitionModel and the grid has at most FD_FLOW_RESIDENT_MAX_POINTS points.  beginResident: the frame becomes the current
    // one; true when the points of `target` were queued for tracking (fd_flow_track_fb_resident), false where predict would hand over
    // to the fallback before tracking (no previous pyramid, no target).  drawResident: the normal draws of `samples` samples, as
    // fd_particles_sample_flow takes them, behind a snapshot of the generator and the distribution.  endResident: what the device's
    // motion says happened; a motion that is not ok puts the snapshot back, as if the draws had not been taken.
    bool residentPossible() const;
    bool beginResident(const cv::Mat& image, const std::shared_ptr<Sample> target);
    const std::vector<double>& drawResident(size_t samples);
    void endResident(const fd_flow_motion_info& motion);
    fd_flow* native() const { return flow; }
protected:
    // the frame becomes the current one (fd_flow_update); tracks `points` forward and the results backward (fd_flow_track_fb)
    virtual void updatePyramid(const cv::Mat& image);
    virtual void trackPoints(const std::vector<cv::Point2f>& points, std::vector<cv::Point2f>& forwardPoints, std::vector<cv::Point2f>& backwardPoints,
                             std::vector<cv::uchar>& forwardStatus, std::vector<cv::uchar>& backwardStatus);
private:
    std::shared_ptr<TransitionModel> fallback;
    std::vector<cv::Point2f> templatePoints;
    cv::Size gridSize, windowSize;
    int maxLevel;
    fd_flow* flow = nullptr;
    int flowWidth = 0, flowHeight = 0;
    bool hasPrevious = false;
    void fetchTracks() const;
    std::vector<cv::Point2f> points;
    mutable std::vector<cv::Point2f> forwardPoints, backwardPoints;
    mutable std::vector<cv::uchar> forwardStatus, backwardStatus;
    mutable std::vector<int> correctFlowIndices;
    mutable bool tracksOnDevice = false;   // a resident predict tracked `points`: the four arrays and the indices are fetched on demand
    std::vector<double> residentDiffusion;
    std::mt19937 generatorBefore;
    std::normal_distribution<> distributionBefore;
    fd_flow_motion lastMotion{};
    bool flowUsed = false;
    std::vector<double> lastDraws;
    double positionDeviation, sizeDeviation;
    std::mt19937 generator;
    std::normal_distribution<> distribution;
};

// ResamplingSampler.hpp / .cpp:24-71.  std::mt19937(seed): per random sample one std::uniform_real_distribution<> draw (the size), then
// std::uniform_int_distribution<int>(0, cols - size) and (0, rows - size).
class ResamplingSampler : public Sampler {
public:
    ResamplingSampler(unsigned int count, double randomRate, std::shared_ptr<ResamplingAlgorithm> resamplingAlgorithm,
                      std::shared_ptr<TransitionModel> transitionModel, int minSize, int maxSize, unsigned int seed = std::mt19937::default_seed);
    void init(const cv::Mat& image) override;
    void sample(const std::vector<std::shared_ptr<Sample>>& samples, std::vector<std::shared_ptr<Sample>>& newSamples, const cv::Mat& image,
                const std::shared_ptr<Sample> target) override;
    int getCount() { return count; }
    void setCount(unsigned int count) { this->count = count; }
    double getRandomRate() { return randomRate; }
    void setRandomRate(double randomRate) { this->randomRate = std::max(0.0, std::min(1.0, randomRate)); }
    std::shared_ptr<ResamplingAlgorithm> getResamplingAlgorithm() const { return resamplingAlgorithm; }
    std::shared_ptr<TransitionModel> getTransitionModel() const { return transitionModel; }
    // the values of one random sample {x, y, size} for an image of cols x rows (sampleValues, .cpp:61-71)
    void drawValues(int cols, int rows, int32_t out[3]);
    // not in the reference: what the last frame drew, in the order it was drawn (u, then three numbers per copy, then the values of the
    // random samples), for replaying a run
    struct Draws {
        bool hasU = false;
        double u = 0;
        std::vector<double> diffusion;   // 3 per copy
        std::vector<int32_t> fresh;      // 3 per random sample
    };
    const Draws& getLastDraws() const { return lastDraws; }
    // the draws of one frame without the Sample objects, in sample()'s order: for an old generation of oldCount samples whose weights
    // add up (in index order) to oldWeightSum.  Needs LowVarianceSampling; the diffusion is drawn from `simple`, by default the
    // sampler's own SimpleTransitionModel (an OpticalFlowTransitionModel's fallback is the caller's to pass).
    const Draws& drawFrame(size_t oldCount, double oldWeightSum, int cols, int rows, SimpleTransitionModel* simple = nullptr);
private:
    Draws lastDraws;
    void sampleValues(Sample& sample, const cv::Mat& image);
    unsigned int count;
    double randomRate;
    std::shared_ptr<ResamplingAlgorithm> resamplingAlgorithm;
    std::shared_ptr<TransitionModel> transitionModel;
    int minSize, maxSize;
    std::mt19937 generator;
    std::uniform_real_distribution<> realDistribution;
};

// GridSampler.hpp / .cpp:23-53
class GridSampler : public Sampler {
public:
    GridSampler(int minSize, int maxSize, float sizeScale, float stepSize);
    void init(const cv::Mat& image) override;
    void sample(const std::vector<std::shared_ptr<Sample>>& samples, std::vector<std::shared_ptr<Sample>>& newSamples, const cv::Mat& image,
                const std::shared_ptr<Sample> target) override;
private:
    int minSize, maxSize;
    float sizeScale, stepSize;
};

// StateExtractor.hpp:22-38
class StateExtractor {
public:
    virtual ~StateExtractor() {}
    virtual std::shared_ptr<Sample> extract(const std::vector<std::shared_ptr<Sample>>& samples) = 0;
};

// FilteringStateExtractor.hpp / .cpp:16-25: the samples with the target flag go to the wrapped extractor
class FilteringStateExtractor : public StateExtractor {
public:
    explicit FilteringStateExtractor(std::shared_ptr<StateExtractor> extractor);
    std::shared_ptr<Sample> extract(const std::vector<std::shared_ptr<Sample>>& samples) override;
    std::shared_ptr<StateExtractor> getExtractor() const { return extractor; }
private:
    std::shared_ptr<StateExtractor> extractor;
};

// WeightedMeanStateExtractor.hpp / .cpp:21-62.  The reference picks the largest cluster with max_element over an unordered_map, so
// equally large clusters are decided by the hash order; here the one whose first member has the lowest sample index wins.
class WeightedMeanStateExtractor : public StateExtractor {
public:
    WeightedMeanStateExtractor();
    std::shared_ptr<Sample> extract(const std::vector<std::shared_ptr<Sample>>& samples) override;
};

// MaxWeightStateExtractor.hpp / .cpp:16-30
class MaxWeightStateExtractor : public StateExtractor {
public:
    MaxWeightStateExtractor();
    std::shared_ptr<Sample> extract(const std::vector<std::shared_ptr<Sample>>& samples) override;
};

// The two trackers share the frame loop: sample -> evaluate -> extract (CondensationTracker.cpp:35-47), and for the adaptive one
// validators and adapt (AdaptiveCondensationTracker.cpp:67-95).  Not in the reference: the device route.  With
// FD_COND_DEVICE=1 a frame runs on a particle set that stays on the device (fd_particles) when its sampler is a ResamplingSampler on
// LowVarianceSampling, its extractor FilteringStateExtractor(WeightedMeanStateExtractor), and model and transition model are one of
//  - ExtendedHogBasedMeasurementModel with adaptation NONE or POSITION, under SimpleTransitionModel;
//  - SingleClassifierModel (also the one inside a PositionDependentMeasurementModel) with a ProbabilisticSvmClassifier on f32 vectors on
//    a Haar, SURF or integral HOG extractor, under SimpleTransitionModel or an OpticalFlowTransitionModel with a SimpleTransitionModel
//    fallback and a grid of at most 1024 points;
//  - the same SingleClassifierModel on a DirectPyramidFeatureExtractor with a histogram, extended HOG or gray-patch chain (also behind
//    PatchResizingFeatureExtractors), under SimpleTransitionModel only;
//  - WvmSvmModel where WvmSvmModel::residentPossible holds, under SimpleTransitionModel only.
// These classes exactly: a subclass of any of them may override what the route restates and therefore keeps the generic route.  The
// host draws the same random numbers in the same order and reads one fd_particles_info back.  getSamples() then builds the Sample
// objects on demand; they carry no ancestors.  Every other configuration takes the generic route over vector<shared_ptr<Sample>>.
// A model that is exactly PositionDependentMeasurementModel gets the samples its adapt reads chosen on the device in that one read-back
// (PositionDependentMeasurementModel::residentNegatives), so its frames do not build the Sample objects at all; a validator that is
// exactly ClassificationBasedStateValidator (it ignores its samples) does not make them either.
class ParticleFrameLoop {
public:
    enum class Route { NONE, GENERIC, DEVICE };
    Route getLastRoute() const { return lastRoute; }
    // the current generation exists as Sample objects: always on the generic route; on the device route once something has asked for
    // them (getSamples(), a validator or a model that reads samples)
    bool samplesMaterialized() const { return materialized; }
protected:
    // the last frame left its samples on the device and neither the model's isValid nor its adapt reads them
    bool samplesUnread() const { return lastRoute == Route::DEVICE && lastKind == ResidentKind::Ehog; }
    // the last frame left its samples on the device and brought back, with the state, what PositionDependentMeasurementModel::adapt reads
    // of them (fd_particles_state_negatives): chosenNegatives() is the argument of adaptResident
    bool negativesChosen() const { return lastRoute == Route::DEVICE && residentChose; }
    const std::vector<Sample>& chosenNegatives() const { return residentChosen; }
    // the generation lives on the device alone (a validator that does not read its samples argument need not get it)
    bool samplesOnDeviceOnly() const { return resident && !materialized; }
    // PartiallyAdaptiveCondensationTracker: the model whose examples a device frame reads with its state (readExamples) in place of the
    // plain state; the frame takes the device route only while this model has a resident plan.  examplesRead(): the last frame did so
    std::shared_ptr<SelfLearningMeasurementModel> examplesModel;
    bool examplesRead() const { return lastRoute == Route::DEVICE && residentExamples; }
    ParticleFrameLoop(std::shared_ptr<Sampler> sampler, std::shared_ptr<MeasurementModel> measurementModel, std::shared_ptr<StateExtractor> extractor);
    ~ParticleFrameLoop();
    ParticleFrameLoop(const ParticleFrameLoop&) = delete;
    ParticleFrameLoop& operator=(const ParticleFrameLoop&) = delete;
    void step(const cv::Mat& imageData);   // one frame up to the extracted state
    const std::vector<std::shared_ptr<Sample>>& currentSamples() const;
    void replaceSamples(const std::vector<std::shared_ptr<Sample>>& newSamples);
    mutable std::vector<std::shared_ptr<Sample>> samples;
    std::vector<std::shared_ptr<Sample>> oldSamples;
    std::shared_ptr<Sample> state;
    std::shared_ptr<imageprocessing::VersionedImage> image;
    std::shared_ptr<Sampler> sampler;
    std::shared_ptr<MeasurementModel> measurementModel;
    std::shared_ptr<StateExtractor> extractor;
private:
    // which resident frame the configuration has, decided before the model's update(image): Ehog is ExtendedHogBasedMeasurementModel on a
    // set bound to its tracker; Integral and Pyramid are the two families of SingleClassifierModel::residentPlan, WvmSvm is WvmSvmModel,
    // all three on an unbound set
    enum class ResidentKind { None, Ehog, Integral, Pyramid, WvmSvm };
    ResidentKind residentKind() const;
    void deviceStep();
    void bindParticles(fd_ehog_tracker* tracker);
    void releaseParticles();
    void uploadGeneration();
    fd_particles* particles = nullptr;
    fd_ehog_tracker* particlesOn = nullptr;   // the tracker handle `particles` is bound to; NULL: an unbound set
    bool resident = false;                    // the current generation lives in `particles`
    mutable bool materialized = true;         // `samples` holds it as well
    int residentCount = 0;
    double residentWeightSum = 0;
    bool residentExamples = false;            // the last device frame read its state through SelfLearningMeasurementModel::readExamples
    bool residentChose = false;               // the last device frame read its state through fd_particles_state_negatives
    std::vector<Sample> residentChosen;       // what it chose, in the list order of adapt
    Route lastRoute = Route::NONE;
    ResidentKind lastKind = ResidentKind::None;
};

// CondensationTracker.hpp / .cpp:25-47
class CondensationTracker : public ParticleFrameLoop {
public:
    CondensationTracker(std::shared_ptr<Sampler> sampler, std::shared_ptr<MeasurementModel> measurementModel, std::shared_ptr<StateExtractor> extractor);
    boost::optional<cv::Rect> process(const cv::Mat& image);
    std::shared_ptr<Sample> getState() { return state; }
    const std::vector<std::shared_ptr<Sample>>& getSamples() const { return currentSamples(); }
    std::shared_ptr<Sampler> getSampler() { return sampler; }
    void setSampler(std::shared_ptr<Sampler> sampler) { this->sampler = sampler; }
};

// AdaptiveCondensationTracker.hpp / .cpp:29-119
class AdaptiveCondensationTracker : public ParticleFrameLoop {
public:
    AdaptiveCondensationTracker(std::shared_ptr<Sampler> sampler, std::shared_ptr<AdaptiveMeasurementModel> measurementModel,
                                std::shared_ptr<StateExtractor> extractor, int initialCount);
    boost::optional<cv::Rect> initialize(const cv::Mat& image, const cv::Rect& position);
    boost::optional<cv::Rect> process(const cv::Mat& image);
    void reset();
    bool hasAdapted();
    std::shared_ptr<Sample> getState();
    const std::vector<std::shared_ptr<Sample>>& getSamples() const;
    std::shared_ptr<Sampler> getSampler();
    void setSampler(std::shared_ptr<Sampler> sampler);
    void addValidator(std::shared_ptr<StateValidator> validator);
private:
    int initialCount;
    bool adapted;
    std::shared_ptr<AdaptiveMeasurementModel> adaptiveModel;
    std::vector<std::shared_ptr<StateValidator>> validators;
};

// PartiallyAdaptiveCondensationTracker.hpp / .cpp:26-71: a static model until the adaptive one, bootstrapped from the static model's most
// and least confident samples, is usable.  On ParticleFrameLoop: under FD_COND_DEVICE=1 a frame takes the device route when the initial
// model is exactly WvmSvmModel with residentPossible, the adaptive model exactly SelfLearningMeasurementModel with a resident plan, and
// sampler, SimpleTransitionModel and state extractor are the ones the route requires; no Sample objects are built then unless
// getSamples() asks for them.
class PartiallyAdaptiveCondensationTracker : public ParticleFrameLoop {
public:
    PartiallyAdaptiveCondensationTracker(std::shared_ptr<Sampler> sampler, std::shared_ptr<MeasurementModel> initialMeasurementModel,
                                         std::shared_ptr<AdaptiveMeasurementModel> measurementModel, std::shared_ptr<StateExtractor> extractor);
    boost::optional<cv::Rect> process(const cv::Mat& image);
    std::shared_ptr<Sample> getState() { return state; }
    const std::vector<std::shared_ptr<Sample>>& getSamples() const { return currentSamples(); }
    std::shared_ptr<Sampler> getSampler() { return sampler; }
    void setSampler(std::shared_ptr<Sampler> sampler) { this->sampler = sampler; }
    bool isUsingAdaptiveModel() { return useAdaptiveModel; }
    bool hasUsedAdaptiveModel() { return usedAdaptiveModel; }
    void setUseAdaptiveModel(bool useAdaptive);
private:
    bool useAdaptiveModel = true, usedAdaptiveModel = false;
    std::shared_ptr<MeasurementModel> initialModel;
    std::shared_ptr<AdaptiveMeasurementModel> adaptiveModel;
};

}  // namespace condensation
