// LandmarkBasedSupervisedDescentTraining.hpp / .cpp of the reference on top of fd_sdm_train (include/fd_hip.h).
// The data preparation of train() (.cpp:211-291) runs on the host in the reference's float / double arithmetic; the cascade loop
// (.cpp:297-365) is fd_sdm_train.  How the cv::MatExpr lines evaluate (OpenCV folds "a * s + t" chains into one convertTo whose
// two coefficients are doubles rounded to float, applied as x * alpha + beta in float):
//   alignMean            x * (float)(s * w) + (float)((0.5 + t) * w + box.x)                      (.cpp:391-392)
//   rescaleModel         x * (float)(1 / s.mu) + (float)(-t.mu / s.mu)                            (.cpp:190-191)
//   unit-sum-sq-norm     x + (float)(-centroid), then x * (float)(1 / sqrtf(sum of float squares))  (.cpp:54-68)
//   calculateMean        cv::reduce(AVG): float column sums in image order, times (float)(1 / rows)
//   cv::mean             double sum / n;  cv::meanStdDev: population, sqrt(max(sum(x^2) / n - mean^2, 0)) in double
// Deviations: one seeded std::mt19937 for the whole training (constructor argument; the reference seeds a fresh engine from
// random_device per sample) with the draw order fixed as scale, tx, ty (the reference passes tx, ty as two arguments of one call:
// unspecified order); nothing is drawn into the training images (.cpp:263-264,273); train() honours setRegularisation once it has
// been called -- until then it is what the reference compiles to: Automatic, factor 0.5, affine component regularised (.hpp:187);
// regulariseWithEigenvalueThreshold throws.  A trained model is for SdmLandmarkModelFitting(model, adaptive = false).
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <numeric>
#include <random>
#include <stdexcept>
#include "superviseddescent/superviseddescent_all.hpp"

namespace superviseddescent {

enum class RegularizationType { Manual, Automatic, EigenvalueThreshold };

class LandmarkBasedSupervisedDescentTraining {
public:
    struct GaussParameter { float mu = 0.0f; float sigma = 1.0f; };
    struct AlignmentStatistics { GaussParameter tx, ty, sx, sy; };
    struct Regularisation { float factor = 0.5f; bool regulariseAffineComponent = false; bool regulariseWithEigenvalueThreshold = false; };
    enum class AlignGroundtruth { NONE, NORMALIZED_FACEBOX };
    enum class MeanNormalization { NONE, UNIT_SUM_SQUARED_NORMS };
    // what train() did, for callers that want to look (sdm_train_app --trace)
    struct Trace {
        std::vector<float> mean, normalisedMean, rescaledMean;
        AlignmentStatistics first, second;
        std::vector<float> draws;          // scale, tx, ty per sample, in draw order
        std::vector<float> startShapes;    // rows x 2L, the caller's order (image-major)
        std::vector<float> finalShapes;    // rows x 2L after the last step, the caller's order
        std::vector<fd_sdm_train_step_info> steps;   // S + 1
    };

    explicit LandmarkBasedSupervisedDescentTraining(unsigned int seed = 5489u) : engine(seed) {}
    void setNumSamplesPerImage(int n) { numSamplesPerImage = n; }
    void setNumCascadeSteps(int n) { numCascadeSteps = n; }
    void setRegularisation(Regularisation r) { regularisation = r; regularisationSet = true; }
    void setAlignGroundtruth(AlignGroundtruth a) { alignGroundtruth = a; }
    void setMeanNormalization(MeanNormalization m) { meanNormalization = m; }
    void setPrepareOnly(bool on) { prepareOnly = on; }   // train() stops after the preparation: no device call, an empty model
    const Trace& getTrace() const { return trace; }

    static cv::Mat transformLandmarksNormalized(cv::Mat landmarks, cv::Rect box);
    static cv::Mat meanNormalizationUnitSumSquaredNorms(cv::Mat modelMean);
    static cv::Mat calculateMean(cv::Mat landmarks, AlignGroundtruth alignGroundtruth, MeanNormalization meanNormalization,
                                 std::vector<cv::Rect> faceboxes = std::vector<cv::Rect>());
    static AlignmentStatistics calculateAlignmentStatistics(std::vector<cv::Rect> trainingFaceboxes, cv::Mat groundtruthLandmarks, cv::Mat initialShapeEstimateX0);
    static cv::Mat rescaleModel(cv::Mat modelMean, const AlignmentStatistics& alignmentStatistics);
    SdmLandmarkModel train(std::vector<cv::Mat> trainingImages, std::vector<cv::Mat> trainingGroundtruthLandmarks, std::vector<cv::Rect> trainingFaceboxes,
                           std::vector<std::string> modelLandmarks, std::vector<std::string> descriptorTypes,
                           std::vector<std::shared_ptr<DescriptorExtractor>> descriptorExtractors);

private:
    int numSamplesPerImage = 10, numCascadeSteps = 5;
    Regularisation regularisation;
    bool regularisationSet = false, prepareOnly = false;
    AlignGroundtruth alignGroundtruth = AlignGroundtruth::NONE;
    MeanNormalization meanNormalization = MeanNormalization::UNIT_SUM_SQUARED_NORMS;
    std::mt19937 engine;
    Trace trace;
};

// ---- free functions (.cpp:383-414, 439-518, 559-578)
inline cv::Mat alignMean(cv::Mat mean, cv::Rect faceBox, float scalingX = 1.0f, float scalingY = 1.0f, float translationX = 0.0f, float translationY = 0.0f) {
    cv::Mat out = mean.clone();
    const int L = mean.cols / 2;
    const float ax = (float)((double)scalingX * faceBox.width), bx = (float)((0.5 + (double)translationX) * faceBox.width + faceBox.x);
    const float ay = (float)((double)scalingY * faceBox.height), by = (float)((0.5 + (double)translationY) * faceBox.height + faceBox.y);
    for (int i = 0; i < L; ++i) {
        out.at<float>(0, i) = mean.at<float>(0, i) * ax + bx;
        out.at<float>(0, i + L) = mean.at<float>(0, i + L) * ay + by;
    }
    return out;
}
namespace detail {
inline double meanOf(const cv::Mat& row, int c0, int c1) {
    double s = 0.0;
    for (int c = c0; c < c1; ++c) s += (double)row.at<float>(0, c);
    return s / (c1 - c0);
}
inline void minMaxOf(const cv::Mat& row, int c0, int c1, double& mn, double& mx) {
    mn = mx = (double)row.at<float>(0, c0);
    for (int c = c0; c < c1; ++c) { const double v = row.at<float>(0, c); mn = std::min(mn, v); mx = std::max(mx, v); }
}
inline cv::Mat rowOf(const cv::Mat& m, int r) {
    cv::Mat out(1, m.cols, CV_32FC1);
    for (int c = 0; c < m.cols; ++c) out.at<float>(0, c) = m.at<float>(r, c);
    return out;
}
}  // namespace detail
// both take 1 x n rows
inline float calculateMeanTranslation(cv::Mat groundtruth, cv::Mat estimate) {
    return (float)(detail::meanOf(estimate, 0, estimate.cols) - detail::meanOf(groundtruth, 0, groundtruth.cols));
}
inline float calculateScaleRatio(cv::Mat groundtruth, cv::Mat estimate) {
    double gmin, gmax, emin, emax;
    detail::minMaxOf(groundtruth, 0, groundtruth.cols, gmin, gmax);
    detail::minMaxOf(estimate, 0, estimate.cols, emin, emax);
    return (float)((emax - emin) / (gmax - gmin));
}
// draws scale, tx, ty from the engine, in this order; drawn (optional) receives the three values
inline cv::Mat getPerturbedShape(cv::Mat modelMean, LandmarkBasedSupervisedDescentTraining::AlignmentStatistics st, cv::Rect detectedFace, std::mt19937& engine,
                                 float* drawn = nullptr) {
    std::normal_distribution<float> rndN_t_x(st.tx.mu, st.tx.sigma), rndN_t_y(st.ty.mu, st.ty.sigma);
    LandmarkBasedSupervisedDescentTraining::GaussParameter sv;
    sv.mu = (float)((st.sx.mu + st.sy.mu) / 2.0);
    sv.sigma = (float)((st.sx.sigma + st.sy.sigma) / 2.0);
    std::normal_distribution<float> rndN_scale(sv.mu, sv.sigma);
    const float s = rndN_scale(engine), tx = rndN_t_x(engine), ty = rndN_t_y(engine);
    if (drawn) { drawn[0] = s; drawn[1] = tx; drawn[2] = ty; }
    return alignMean(modelMean, detectedFace, s, s, tx, ty);
}
// linearRegression (.cpp:439-518; defaults of the header, .hpp:187) through fd_sdm_linear_regression: A is M x D, b is M x N, returns D x N
inline cv::Mat linearRegression(cv::Mat A, cv::Mat b, RegularizationType regularizationType = RegularizationType::Automatic, float lambda = 0.5f,
                                bool regularizeAffineComponent = true) {
    if (regularizationType == RegularizationType::EigenvalueThreshold)
        throw std::runtime_error("linearRegression: EigenvalueThreshold regularisation needs Eigen's FullPivLU::maxPivot() * threshold() and is not built");
    if (A.type() != CV_32FC1 || b.type() != CV_32FC1 || A.rows != b.rows) throw std::invalid_argument("linearRegression: A and b must be CV_32FC1 with equal rows");
    std::vector<float> a((size_t)A.rows * A.cols), bb((size_t)b.rows * b.cols);
    for (int r = 0; r < A.rows; ++r) for (int c = 0; c < A.cols; ++c) a[(size_t)r * A.cols + c] = A.at<float>(r, c);
    for (int r = 0; r < b.rows; ++r) for (int c = 0; c < b.cols; ++c) bb[(size_t)r * b.cols + c] = b.at<float>(r, c);
    cv::Mat x(A.cols, b.cols, CV_32FC1);
    fdhost::check(fd_sdm_linear_regression(fdhost::context(), a.data(), bb.data(), A.rows, A.cols, b.cols,
                                           regularizationType == RegularizationType::Automatic ? FD_SDM_REG_AUTOMATIC : FD_SDM_REG_MANUAL, (double)lambda,
                                           regularizeAffineComponent ? 1 : 0, x.ptr<float>(0), nullptr, nullptr, nullptr));
    return x;
}

// ---- the class
inline cv::Mat LandmarkBasedSupervisedDescentTraining::transformLandmarksNormalized(cv::Mat landmarks, cv::Rect box) {   // .cpp:34-46
    cv::Mat t(landmarks.rows, landmarks.cols, landmarks.type());
    const int L = landmarks.cols / 2;
    for (int i = 0; i < L; ++i) {
        t.at<float>(i) = ((landmarks.at<float>(i) - box.x) / static_cast<float>(box.width)) - 0.5f;
        t.at<float>(i + L) = ((landmarks.at<float>(i + L) - box.y) / static_cast<float>(box.height)) - 0.5f;
    }
    return t;
}
inline cv::Mat LandmarkBasedSupervisedDescentTraining::meanNormalizationUnitSumSquaredNorms(cv::Mat modelMean) {   // .cpp:48-70
    const int L = modelMean.cols / 2;
    const float ncx = (float)(-detail::meanOf(modelMean, 0, L)), ncy = (float)(-detail::meanOf(modelMean, L, 2 * L));
    for (int i = 0; i < L; ++i) { modelMean.at<float>(0, i) = modelMean.at<float>(0, i) + ncx; modelMean.at<float>(0, i + L) = modelMean.at<float>(0, i + L) + ncy; }
    float total = 0.0f;
    for (int p = 0; p < L; ++p) {
        const float x = modelMean.at<float>(0, p), y = modelMean.at<float>(0, p + L);
        total += (x * x + y * y);
    }
    const float inv = (float)(1.0 / (double)std::sqrt(total));
    for (int i = 0; i < 2 * L; ++i) modelMean.at<float>(0, i) = modelMean.at<float>(0, i) * inv;
    return modelMean;
}
inline cv::Mat LandmarkBasedSupervisedDescentTraining::calculateMean(cv::Mat landmarks, AlignGroundtruth align, MeanNormalization norm, std::vector<cv::Rect> faceboxes) {
    if (landmarks.empty()) throw std::runtime_error("No landmarks provided to calculate the mean.");
    cv::Mat lm = landmarks.clone();
    if (align == AlignGroundtruth::NORMALIZED_FACEBOX) {   // "untested" in the reference
        if ((int)faceboxes.size() != lm.rows)
            throw std::runtime_error("'AlignGroundtruth' is set to NORMALIZED_FACEBOX but faceboxes.size() != landmarks.size(). Please provide a face-box for each set of landmarks.");
        for (int r = 0; r < lm.rows; ++r) {
            cv::Mat t = transformLandmarksNormalized(detail::rowOf(lm, r), faceboxes[r]);
            for (int c = 0; c < lm.cols; ++c) lm.at<float>(r, c) = t.at<float>(0, c);
        }
    }
    cv::Mat mean(1, lm.cols, CV_32FC1);
    const float inv = (float)(1.0 / lm.rows);
    for (int c = 0; c < lm.cols; ++c) {
        float s = 0.0f;
        for (int r = 0; r < lm.rows; ++r) s += lm.at<float>(r, c);
        mean.at<float>(0, c) = s * inv;
    }
    if (norm == MeanNormalization::UNIT_SUM_SQUARED_NORMS) mean = meanNormalizationUnitSumSquaredNorms(mean);
    return mean;
}
inline LandmarkBasedSupervisedDescentTraining::AlignmentStatistics LandmarkBasedSupervisedDescentTraining::calculateAlignmentStatistics(
    std::vector<cv::Rect> boxes, cv::Mat gt, cv::Mat x0) {   // .cpp:130-184
    const int n = gt.rows, L = gt.cols / 2;
    std::vector<float> d[4];
    for (int i = 0; i < n; ++i) {
        auto part = [&](const cv::Mat& m, int c0) { cv::Mat p(1, L, CV_32FC1); for (int c = 0; c < L; ++c) p.at<float>(0, c) = m.at<float>(i, c0 + c); return p; };
        cv::Mat gx = part(gt, 0), gy = part(gt, L), ex = part(x0, 0), ey = part(x0, L);
        d[0].push_back(calculateMeanTranslation(gx, ex) / boxes[i].width);
        d[1].push_back(calculateMeanTranslation(gy, ey) / boxes[i].height);
        d[2].push_back(calculateScaleRatio(gx, ex));
        d[3].push_back(calculateScaleRatio(gy, ey));
    }
    auto stat = [&](const std::vector<float>& v) {
        double s = 0.0, sq = 0.0;
        for (float x : v) { s += (double)x; sq += (double)x * (double)x; }
        const double mean = s / v.size(), var = std::max(sq / v.size() - mean * mean, 0.0);
        GaussParameter g;
        g.mu = (float)mean;
        g.sigma = (float)std::sqrt(var);
        return g;
    };
    AlignmentStatistics a;
    a.tx = stat(d[0]); a.ty = stat(d[1]); a.sx = stat(d[2]); a.sy = stat(d[3]);
    return a;
}
inline cv::Mat LandmarkBasedSupervisedDescentTraining::rescaleModel(cv::Mat modelMean, const AlignmentStatistics& st) {   // .cpp:186-193
    const int L = modelMean.cols / 2;
    const float ax = (float)(1.0 / (double)st.sx.mu), bx = (float)(-(double)st.tx.mu / (double)st.sx.mu);
    const float ay = (float)(1.0 / (double)st.sy.mu), by = (float)(-(double)st.ty.mu / (double)st.sy.mu);
    for (int i = 0; i < L; ++i) {
        modelMean.at<float>(0, i) = modelMean.at<float>(0, i) * ax + bx;
        modelMean.at<float>(0, i + L) = modelMean.at<float>(0, i + L) * ay + by;
    }
    return modelMean;
}
inline SdmLandmarkModel LandmarkBasedSupervisedDescentTraining::train(std::vector<cv::Mat> images, std::vector<cv::Mat> landmarks, std::vector<cv::Rect> boxes,
                                                                      std::vector<std::string> modelLandmarks, std::vector<std::string> descriptorTypes,
                                                                      std::vector<std::shared_ptr<DescriptorExtractor>> extractors) {
    const int n = (int)images.size(), L = (int)modelLandmarks.size(), N = 2 * L, S = numCascadeSteps, K1 = numSamplesPerImage + 1;
    if (n == 0 || (int)landmarks.size() != n || (int)boxes.size() != n) throw std::invalid_argument("train: need one landmark row and one face box per image");
    if ((int)extractors.size() < S || (int)descriptorTypes.size() < S) throw std::invalid_argument("train: need one descriptor extractor per cascade step");
    // only what the device runs: VlHog extractors with explicit parameters, one type for all steps
    std::vector<int32_t> dp;
    int variant = -1;
    for (int s = 0; s < S; ++s) {
        auto e = std::dynamic_pointer_cast<VlHogDescriptorExtractor>(extractors[s]);
        if (!e || e->getNumCells() < 1) throw std::logic_error("LandmarkBasedSupervisedDescentTraining: only VlHogDescriptorExtractors with numCells, cellSize and numBins are available on this backend");
        const int v = e->getType() == VlHogDescriptorExtractor::VlHogType::Uoctti ? 1 : 0;
        if (variant >= 0 && v != variant) throw std::logic_error("LandmarkBasedSupervisedDescentTraining: the cascade steps must share one VlHog type");
        variant = v;
        dp.push_back(e->getNumCells()); dp.push_back(e->getCellSize()); dp.push_back(e->getNumBins());
    }
    if (regularisationSet && regularisation.regulariseWithEigenvalueThreshold)
        throw std::runtime_error("LandmarkBasedSupervisedDescentTraining: regulariseWithEigenvalueThreshold (EigenvalueThreshold regularisation) is not built");
    // ---- .cpp:211-291
    cv::Mat gt(n, N, CV_32FC1);
    for (int i = 0; i < n; ++i) for (int c = 0; c < N; ++c) gt.at<float>(i, c) = landmarks[i].at<float>(c);
    auto toVec = [&](const cv::Mat& row) { std::vector<float> v(N); for (int c = 0; c < N; ++c) v[c] = row.at<float>(0, c); return v; };
    trace = Trace();
    trace.mean = toVec(calculateMean(gt, alignGroundtruth, MeanNormalization::NONE, boxes));
    cv::Mat modelMean = calculateMean(gt, alignGroundtruth, meanNormalization, boxes);
    trace.normalisedMean = toVec(modelMean);
    auto alignAll = [&](const cv::Mat& mean) {
        cv::Mat x0(n, N, CV_32FC1);
        for (int i = 0; i < n; ++i) { cv::Mat a = alignMean(mean, boxes[i]); for (int c = 0; c < N; ++c) x0.at<float>(i, c) = a.at<float>(0, c); }
        return x0;
    };
    AlignmentStatistics st = calculateAlignmentStatistics(boxes, gt, alignAll(modelMean));
    trace.first = st;
    modelMean = rescaleModel(modelMean, st);
    trace.rescaledMean = toVec(modelMean);
    st = calculateAlignmentStatistics(boxes, gt, alignAll(modelMean));
    trace.second = st;
    const size_t M = (size_t)n * K1;
    std::vector<float> x0(M * N), gts(M * N);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < K1; ++k) {
            float drawn[3];
            cv::Mat s = k == 0 ? alignMean(modelMean, boxes[i]) : getPerturbedShape(modelMean, st, boxes[i], engine, drawn);
            if (k) trace.draws.insert(trace.draws.end(), drawn, drawn + 3);
            for (int c = 0; c < N; ++c) { x0[((size_t)i * K1 + k) * N + c] = s.at<float>(0, c); gts[((size_t)i * K1 + k) * N + c] = gt.at<float>(i, c); }
        }
    trace.startShapes = x0;
    if (prepareOnly) return SdmLandmarkModel(modelMean, modelLandmarks, {}, {}, {});
    // ---- size groups: images sorted by (width, height), stable; rows follow their images and come back in the caller's order
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return std::make_pair(images[a].cols, images[a].rows) < std::make_pair(images[b].cols, images[b].rows);
    });
    std::vector<std::vector<unsigned char>> stacks;
    std::vector<fd_sdm_train_group> groups;
    std::vector<float> gx0(M * N), ggt(M * N);
    for (int p = 0; p < n; ++p) {
        const int i = order[p];
        if (images[i].type() != CV_8UC1) throw std::invalid_argument("train: this backend expects CV_8UC1 (gray) training images");
        const int W = images[i].cols, H = images[i].rows;
        if (groups.empty() || groups.back().width != W || groups.back().height != H) {
            stacks.emplace_back();
            fd_sdm_train_group g = {nullptr, W, H, 0, 0};
            groups.push_back(g);
        }
        for (int y = 0; y < H; ++y) stacks.back().insert(stacks.back().end(), images[i].ptr<unsigned char>(y), images[i].ptr<unsigned char>(y) + W);
        ++groups.back().count;
        std::copy(x0.begin() + (size_t)i * K1 * N, x0.begin() + (size_t)(i + 1) * K1 * N, gx0.begin() + (size_t)p * K1 * N);
        std::copy(gts.begin() + (size_t)i * K1 * N, gts.begin() + (size_t)(i + 1) * K1 * N, ggt.begin() + (size_t)p * K1 * N);
    }
    for (size_t g = 0; g < groups.size(); ++g) groups[g].images = stacks[g].data();
    fd_sdm_train_params prm = {};
    prm.num_landmarks = L; prm.num_steps = S; prm.hog_variant = variant; prm.desc_params = dp.data();
    prm.regularisation = FD_SDM_REG_AUTOMATIC;
    prm.lambda = regularisationSet ? (double)regularisation.factor : 0.5;
    prm.regularise_affine = regularisationSet ? (regularisation.regulariseAffineComponent ? 1 : 0) : 1;
    std::vector<int32_t> dims(S);
    fdhost::check(fd_sdm_train_step_dims(&prm, dims.data()));
    std::vector<cv::Mat> regs;
    std::vector<float*> Rp;
    for (int s = 0; s < S; ++s) { regs.push_back(cv::Mat(dims[s], N, CV_32FC1)); Rp.push_back(regs.back().ptr<float>(0)); }
    std::vector<float> steps((size_t)(S + 1) * M * N);
    std::vector<int32_t> status(M);
    trace.steps.assign(S + 1, fd_sdm_train_step_info());
    fdhost::check(fd_sdm_train(fdhost::context(), &prm, groups.data(), (int)groups.size(), K1, gx0.data(), ggt.data(), Rp.data(), steps.data(), status.data(),
                               trace.steps.data()));
    trace.finalShapes.resize(M * N);
    for (int p = 0; p < n; ++p)
        std::copy(steps.begin() + ((size_t)S * M + (size_t)p * K1) * N, steps.begin() + ((size_t)S * M + (size_t)(p + 1) * K1) * N,
                  trace.finalShapes.begin() + (size_t)order[p] * K1 * N);
    descriptorTypes.resize(S);
    extractors.resize(S);
    return SdmLandmarkModel(modelMean, modelLandmarks, regs, extractors, descriptorTypes);
}

}  // namespace superviseddescent
