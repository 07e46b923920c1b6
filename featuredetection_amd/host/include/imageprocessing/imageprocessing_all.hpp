// imageprocessing/*.hpp of the reference, re-implemented on top of the C ABI (include/fd_hip.h).
// Class names, namespaces, constructor and method signatures follow the reference headers cited per
// class; the work is done by the HIP kernels behind fd_hip.h.  Filters that the GPU path fuses into a
// kernel (GradientFilter, GradientBinningFilter, HogFilter, LbpFilter as layer filter, HistEq64Filter as
// patch filter) are recognised by type when they are added to a pyramid / extractor; every filter also has
// its stand-alone ImageFilter::applyTo(const Mat&) form (one kernel launch per Mat: for composition and
// tests, not for the sliding-window hot loop).
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "fdcompat/cv.hpp"
#include "fdcompat/runtime.hpp"

namespace classification { class SvmClassifier; }

namespace imageprocessing {

// Version.hpp:18-46 -- (instance id, counter) pair used to avoid rebuilding pyramids
class Version {
public:
    Version() : instance(-1), counter(0) {}
    static Version fresh() { Version v; v.instance = nextInstance()++; return v; }
    bool operator==(const Version& o) const { return instance == o.instance && counter == o.counter; }
    bool operator!=(const Version& o) const { return !(*this == o); }
    Version& operator++() { ++counter; return *this; }
private:
    static int& nextInstance() { static int n = 0; return n; }
    int instance, counter;
};

// VersionedImage.hpp:19-67
class VersionedImage {
public:
    VersionedImage() : data(), version(Version::fresh()) {}
    explicit VersionedImage(const cv::Mat& d) : data(d), version(Version::fresh()) {}
    cv::Mat& getData() { return data; }
    const cv::Mat& getData() const { return data; }
    void setData(const cv::Mat& d) { data = d; ++version; }
    Version getVersion() const { return version; }
private:
    cv::Mat data;
    Version version;
};

// ImageFilter.hpp:18-57
class ImageFilter {
public:
    virtual ~ImageFilter() {}
    cv::Mat applyTo(const cv::Mat& image) const { cv::Mat filtered; return applyTo(image, filtered); }
    virtual cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const = 0;
    virtual void applyInPlace(cv::Mat& image) const { image = applyTo(image); }
};

// ChainedFilter.cpp:36-50
class ChainedFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    void add(std::shared_ptr<ImageFilter> filter) { filters.push_back(filter); }
    const std::vector<std::shared_ptr<ImageFilter>>& getFilters() const { return filters; }
    // the filters in turn.  Only the chain of exactly the two filters [filtering::FpdwFeaturesFilter, filtering::AggregationFilter] is
    // fused into one device call; inside any other chain AggregationFilter::applyTo is reached on its own and throws logic_error
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
private:
    std::vector<std::shared_ptr<ImageFilter>> filters;
};

// GrayscaleFilter.cpp:18-24 (image filter of the pyramid: fused into fd_pyramid_update)
class GrayscaleFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
};

// HistEq64Filter.cpp:32-125 (patch filter: fused into the WVM kernel; stand-alone via fd_histeq64_batch)
class HistEq64Filter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
};

// The "whi" patch filter chain of ffpDetectApp.cpp:449-454.  Added in this order to a (Filtering / Direct) pyramid feature
// extractor the four filters run as one fused kernel (fd_extract_whi / fd_detect_whi_svm); each also has its per-Mat form
// (fd_whitening_batch, fd_equalize_hist_batch, fd_convert_batch, fd_unit_norm_batch).
// WhiteningFilter.hpp:31 / WhiteningFilter.cpp:18-81
class WhiteningFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit WhiteningFilter(float alpha = 1, float cutoffFrequency = 0.390625f) : alpha(alpha), cutoffFrequency(cutoffFrequency) {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    float alpha, cutoffFrequency;
};
// HistogramEqualizationFilter.cpp (cv::equalizeHist)
class HistogramEqualizationFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
};
// ConversionFilter.hpp: convertTo(type, alpha, beta)
class ConversionFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit ConversionFilter(int type, double alpha = 1, double beta = 0) : type(type), alpha(alpha), beta(beta) {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int type;
    double alpha, beta;
};
// UnitNormFilter.hpp / UnitNormFilter.cpp (eps 1e-4)
class UnitNormFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit UnitNormFilter(int normType = cv::NORM_L2) : normType(normType) {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int normType;
};
// ZeroMeanUnitVarianceFilter.cpp:21-34 (ffpDetectApp.cpp:77 includes it; host only: cv::meanStdDev in double, then (x - mean) / deviation
// on the CV_32F copy, all zeros for a constant image)
class ZeroMeanUnitVarianceFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    ZeroMeanUnitVarianceFilter() {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
};
// ReshapingFilter.hpp: Mat::reshape(channels, rows) (ffpDetectApp.cpp:465-467 turns patches into row vectors); the fused
// kernels work on flat vectors, so inside a fused chain it is a no-op
class ReshapingFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit ReshapingFilter(int rows, int channels = 0) : rows(rows), channels(channels) {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int rows, channels;
};

// GreyWorldNormalizationFilter.cpp:20-71
class GreyWorldNormalizationFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
};

// GradientFilter.cpp:16-59 (fused as a layer filter; applyTo: CV_8UC1 -> CV_8UC2 via fd_gradient_image)
class GradientFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit GradientFilter(int kernelSize, int blurKernelSize = 0);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int kernelSize, blurKernelSize;
};

// GradientBinningFilter.cpp:18-93 (fused as a layer filter; applyTo: CV_8UC2 -> CV_8UC2 / CV_8UC4 via fd_gradient_binning_image)
class GradientBinningFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit GradientBinningFilter(unsigned int bins, bool signedGradients = false, bool interpolate = false);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    unsigned int getBinCount() const { return bins; }
    unsigned int bins;
    bool signedGradients, interpolate;
};

// GradientMagnitudeFilter.hpp:39-50 / GradientMagnitudeFilter.cpp:19-42: the magnitude of a two-channel gradient image.  On this
// backend CV_8UC2 only (the output of GradientFilter: saturate_cast<uchar>(sqrt(x^2 + y^2)) with x, y = value - 127, via
// fd_gradient_magnitude_image); other depths throw invalid_argument naming the depth.  As a layer filter it is fused: the chain
// GradientFilter, GradientMagnitudeFilter, LbpFilter (the "glbp" feature type) runs as FD_LAYER_GRADMAG_LBP
class GradientMagnitudeFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    GradientMagnitudeFilter() {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
};

// LbpFilter.hpp (fused as a layer filter; applyTo via fd_lbp_image)
class LbpFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    enum class Type { LBP8, LBP8_UNIFORM, LBP4, LBP4_ROTATED };
    explicit LbpFilter(Type type = Type::LBP8) : type(type) {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    unsigned int getBinCount() const;
    Type type;
};

// HistogramFilter.hpp:24-33 -- base of the histogram patch filters.  On this backend they run fused on the
// pyramid's bin-image layers (k_hog_tile / k_hist_features); applyTo(Mat) runs the same kernel on one bin-image
// patch (fd_hist_patch_batch) and returns the 1 x F CV_32F feature vector.
class HistogramFilter : public ImageFilter {
public:
    enum class Normalization { NONE, L2NORM, L2HYS, L1NORM, L1SQRT };
    explicit HistogramFilter(Normalization normalization) : normalization(normalization) {}
    Normalization normalization;
};

// HogFilter.hpp / HogFilter.cpp:16-57
class HogFilter : public HistogramFilter {
public:
    using ImageFilter::applyTo;
    explicit HogFilter(int binCount, int cellSize = 5, int blockSize = 2, bool interpolate = false, bool signedAndUnsigned = false);
    HogFilter(int binCount, int cellWidth, int cellHeight, int blockWidth, int blockHeight, bool interpolate = false,
              bool signedAndUnsigned = false);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int binCount, cellWidth, cellHeight, blockWidth, blockHeight;
    bool interpolate, signedAndUnsigned;
};

// ExtendedHogFilter.hpp:45-57 / ExtendedHogFilter.cpp:14-209 (fd_ehog_patch_batch on one patch): bin image -> rows x cols cells of
// binCount (+ binCount / 2 with signedAndUnsigned) + 4 floats, stored as rows x cols * channels CV_32F.  Per patch only (applyTo, a
// FilteringFeatureExtractor): it is not part of a fused pyramid chain.
class ExtendedHogFilter : public HistogramFilter {
public:
    using ImageFilter::applyTo;
    ExtendedHogFilter(int binCount, int cellSize, bool interpolate, bool signedAndUnsigned, float alpha = 0.2f);
    ExtendedHogFilter(int binCount, int cellWidth, int cellHeight, bool interpolate, bool signedAndUnsigned, float alpha = 0.2f);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int getCellWidth() { return cellWidth; }
    int getCellHeight() { return cellHeight; }
    int binCount, cellWidth, cellHeight;
    bool interpolate, signedAndUnsigned;
    float alpha;
};

// CompleteExtendedHogFilter.hpp:35-117 / CompleteExtendedHogFilter.cpp:19-303 (fd_cehog_image): CV_8UC1 -> rows x cols cells of
// binCount (+ binCount / 2 when both gradient kinds are set) + 4 floats, stored as rows x cols * channels CV_32F
class CompleteExtendedHogFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit CompleteExtendedHogFilter(size_t cellSize = 8, size_t binCount = 18, bool signedGradients = true, bool unsignedGradients = true,
                                       bool interpolateBins = false, bool interpolateCells = true, float alpha = 0.2f);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    size_t getCellSize() { return cellSize; }
    fd_cehog_params params() const;
    size_t getDescriptorSize() const { return binCount + (signedGradients && unsignedGradients ? binCount / 2 : 0) + 4; }
    size_t cellSize, binCount;
    bool signedGradients, unsignedGradients, interpolateBins, interpolateCells;
    float alpha;
};

// SpatialHistogramFilter.hpp:38-54 / SpatialHistogramFilter.cpp:16-54
class SpatialHistogramFilter : public HistogramFilter {
public:
    using ImageFilter::applyTo;
    SpatialHistogramFilter(int binCount, int cellSize, int blockSize, bool interpolate, bool concatenate = false,
                           Normalization normalization = Normalization::NONE);
    SpatialHistogramFilter(int binCount, int cellWidth, int cellHeight, int blockWidth, int blockHeight, bool interpolate,
                           bool concatenate = false, Normalization normalization = Normalization::NONE);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int binCount, cellWidth, cellHeight, blockWidth, blockHeight;
    bool interpolate, concatenate;
};

// PyramidHogFilter.hpp:35 / PyramidHogFilter.cpp:15-31
class PyramidHogFilter : public HistogramFilter {
public:
    using ImageFilter::applyTo;
    PyramidHogFilter(int binCount, int levelCount, bool interpolate = false, bool signedAndUnsigned = false);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int binCount, levelCount;
    bool interpolate, signedAndUnsigned;
};

// SpatialPyramidHistogramFilter.hpp:36 / SpatialPyramidHistogramFilter.cpp:21-35
class SpatialPyramidHistogramFilter : public HistogramFilter {
public:
    using ImageFilter::applyTo;
    SpatialPyramidHistogramFilter(int binCount, int levelCount, bool interpolate = false, Normalization normalization = Normalization::NONE);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int binCount, levelCount;
    bool interpolate;
};

// ImagePyramidLayer.hpp:34-163
class ImagePyramidLayer {
public:
    ImagePyramidLayer(int index, double scale, double scaleX, double scaleY, const cv::Mat& image)
        : index(index), scale(scale), scaleX(scaleX), scaleY(scaleY), image(image) {}
    int getScaled(int value) const { return cv::cvRound(value * scale); }
    int getOriginal(int value) const { return cv::cvRound(value / scale); }
    cv::Size getSize() const { return cv::Size(image.cols, image.rows); }
    int getIndex() const { return index; }
    double getScaleFactor() const { return scale; }
    const cv::Mat& getScaledImage() const { return image; }
private:
    int index;
    double scale, scaleX, scaleY;
    cv::Mat image;
};

// ImagePyramid.hpp / ImagePyramid.cpp:67-92,116-128,148-198,300-328 -- backed by fd_pyramid
class ImagePyramid {
public:
    ImagePyramid(size_t octaveLayerCount, double minScaleFactor, double maxScaleFactor = 1);
    ImagePyramid(double incrementalScaleFactor, double minScaleFactor, double maxScaleFactor = 1);
    // ImagePyramid.cpp:100-104: same layers as `pyramid`, restricted to scale factors within [min, max]; nothing is rebuilt,
    // the layers of the source (and its device arena) are shared (createLayers(const ImagePyramid&), :200-235, without the
    // approximated in-between layers of createApproximated)
    ImagePyramid(std::shared_ptr<ImagePyramid> pyramid, double minScaleFactor, double maxScaleFactor = 1);
    // ImagePyramid.cpp:51-63: a feature pyramid whose layers are computed on one layer per octave only and approximated (resized,
    // scaled by pow(s, -lambda) per channel) in between.  On this backend such a pyramid is the recipe of an
    // extraction::AggregatedFeaturesExtractor behind an AggregatedFeaturesDetector (image filter GrayscaleFilter, layer filter
    // filtering::FhogFilter); the device builds its layers inside fd_aggregated_detect.  Using it for anything else -- updating it
    // directly, extractors over its layers, other filters -- throws logic_error, and so does approximating an arbitrary source pyramid.
    static std::shared_ptr<ImagePyramid> createApproximated(int octaveLayerCount, double minScaleFactor, double maxScaleFactor,
                                                            std::vector<double> lambdas = {});
    static std::shared_ptr<ImagePyramid> createApproximated(std::shared_ptr<ImagePyramid> pyramid, int octaveLayerCount,
                                                            std::vector<double> lambdas = {});
    // empty: estimated per image.  An AggregatedFeaturesDetector reads the lambdas, the layer filter and the image filter when it is
    // constructed on the extractor: later changes to the pyramid do not reach a detector that already exists.
    void setLambdas(const std::vector<double>& lambdas) { this->lambdas = lambdas; }
    const std::vector<double>& getLambdas() const { return lambdas; }
    bool isApproximated() const { return approximated; }
    size_t getOctaveLayerCount() const { return ctorOctaveLayers; }
    std::shared_ptr<ImageFilter> getApproximatedLayerFilter() const { return approxLayerFilter; }
    bool hasGrayscaleImageFilter() const { return imageChain.size() == 1 && imageChain[0] == FD_IMAGE_GRAY; }
    bool hasNoImageFilter() const { return imageChain.empty(); }
    // the FD_LAYER_* kind the layer filter chain maps to
    int getLayerFilterKind() const {
        return gradient && binning ? FD_LAYER_GRADBIN : (gradient && magnitude && lbp ? FD_LAYER_GRADMAG_LBP : (lbp && !gradient ? FD_LAYER_LBP : FD_LAYER_NONE));
    }
    ~ImagePyramid();
    ImagePyramid(const ImagePyramid&) = delete;
    ImagePyramid& operator=(const ImagePyramid&) = delete;
    // chains: [GrayscaleFilter] or [GreyWorldNormalizationFilter, GrayscaleFilter]; anything else throws logic_error
    void addImageFilter(const std::shared_ptr<ImageFilter>& filter);
    // the chains [GradientFilter, GradientBinningFilter], [LbpFilter] and [GradientFilter, GradientMagnitudeFilter, LbpFilter]
    void addLayerFilter(const std::shared_ptr<ImageFilter>& filter);
    void update(const cv::Mat& image);
    void update(const std::shared_ptr<VersionedImage>& image);
    void setSource(const cv::Mat& image) { setSource(std::make_shared<VersionedImage>(image)); }
    void setSource(const std::shared_ptr<VersionedImage>& image);     // ImagePyramid.cpp:132-139
    void setSource(const std::shared_ptr<ImagePyramid>& pyramid);     // ImagePyramid.cpp:141-144
    void update();                                                     // ImagePyramid.cpp:146-168
    const std::vector<std::shared_ptr<ImagePyramidLayer>>& getLayers() const;  // downloads the layers on first use
    const std::shared_ptr<ImagePyramidLayer> getLayer(int index) const;
    double getMinScaleFactor() const { return minScaleFactor; }
    double getMaxScaleFactor() const { return maxScaleFactor; }
    double getIncrementalScaleFactor() const;
    cv::Size getImageSize() const { return imageSize; }
    std::vector<std::pair<int, double>> getLayerScales() const;
    std::vector<cv::Size> getLayerSizes() const;
    fd_pyramid* native() const { return sourcePyramid ? sourcePyramid->native() : (requireExact(), handle); }
    std::shared_ptr<ImagePyramid> getSourcePyramid() const { return sourcePyramid; }
    // a second native pyramid with this pyramid's parameters that holds `frames` equally sized frames at once (backend extension
    // behind FiveStageSlidingWindowDetector::detectFrames); NULL for pyramids on a source pyramid or with layer filters
    fd_pyramid* createFramesPyramid(int frames) const;
    // Layer sub-range / region of interest of the extraction or detection call that follows (fd_pyramid_select), intersected
    // with the scale range of a pyramid that views another one; reset when the guard goes out of scope.
    class Selection {
    public:
        // viewFirst / viewLast: layer index range of a pyramid built on another one (-1: the pyramid owns its layers)
        Selection(fd_pyramid* h, int first, int last, int step, const cv::Rect* roi, int viewFirst = -1, int viewLast = -1);
        ~Selection();
        Selection(Selection&& o) : handle(o.handle) { o.handle = nullptr; }
        Selection(const Selection&) = delete;
    private:
        fd_pyramid* handle;
    };
    Selection select(int firstLayer = -1, int lastLayer = -1, int stepLayer = 1, const cv::Rect* roi = nullptr) const;
    static long buildCount();   // pyramids actually (re)built so far: the VersionedImage mechanism at work (tests)
private:
    struct Approximated {};
    ImagePyramid(Approximated, size_t octaveLayerCount, double minScaleFactor, double maxScaleFactor, std::vector<double> lambdas);
    void requireExact() const;   // logic_error on an approximated pyramid
    void applyLayerFilterConfig();
    void viewRange(int& first, int& last) const;   // layer indices of the source inside [minScaleFactor, maxScaleFactor]
    fd_pyramid* handle;
    std::shared_ptr<ImagePyramid> sourcePyramid;
    std::shared_ptr<VersionedImage> sourceImage;
    double minScaleFactor, maxScaleFactor;
    size_t ctorOctaveLayers = 0;          // constructor arguments (one of the two forms)
    double ctorIncremental = 0;
    cv::Size imageSize;
    Version version;
    std::shared_ptr<GradientFilter> gradient;
    std::shared_ptr<GradientBinningFilter> binning;
    std::shared_ptr<LbpFilter> lbp;
    std::shared_ptr<GradientMagnitudeFilter> magnitude;
    std::vector<int> imageChain;          // addImageFilter: FD_IMAGE_GREYWORLD_GRAY for a GreyWorldNormalizationFilter, FD_IMAGE_GRAY for a GrayscaleFilter
    mutable std::vector<std::shared_ptr<ImagePyramidLayer>> layers;
    mutable bool layersValid;
    bool approximated = false;            // createApproximated: no native pyramid; lambdas and layer filter are recorded
    std::vector<double> lambdas;
    std::shared_ptr<ImageFilter> approxLayerFilter;
};

// Patch.hpp:28-243
class Patch {
public:
    Patch() : center(0, 0), size(0, 0), data() {}
    Patch(int x, int y, int width, int height, const cv::Mat& data) : center(x, y), size(width, height), data(data) {}
    Patch(const Patch& other) : center(other.center), size(other.size), data(other.data.clone()) {}
    bool operator==(const Patch& o) const {
        return center.x == o.center.x && center.y == o.center.y && size.width == o.size.width && size.height == o.size.height;
    }
    cv::Rect getBounds() const { return cv::Rect(center.x - size.width / 2, center.y - size.height / 2, size.width, size.height); }
    int getX() const { return center.x; }
    int getY() const { return center.y; }
    int getWidth() const { return size.width; }
    int getHeight() const { return size.height; }
    void setX(int x) { center.x = x; }
    void setY(int y) { center.y = y; }
    void setWidth(int width) { size.width = width; }
    void setHeight(int height) { size.height = height; }
    cv::Mat& getData() { return data; }
    const cv::Mat& getData() const { return data; }
private:
    cv::Point center;
    cv::Size size;
    cv::Mat data;
};

// FeatureExtractor.hpp:22-55
class FeatureExtractor {
public:
    virtual ~FeatureExtractor() {}
    void update(const cv::Mat& image) { update(std::make_shared<VersionedImage>(image)); }
    virtual void update(std::shared_ptr<VersionedImage> image) = 0;
    virtual std::shared_ptr<Patch> extract(int x, int y, int width, int height) const = 0;
};

// PyramidFeatureExtractor.hpp:21-119
class PyramidFeatureExtractor : public FeatureExtractor {
public:
    using FeatureExtractor::update;
    using FeatureExtractor::extract;
    virtual std::vector<std::shared_ptr<Patch>> extract(int stepX, int stepY, cv::Rect roi = cv::Rect(), int firstLayer = -1,
                                                        int lastLayer = -1, int stepLayer = 1) const = 0;
    virtual std::shared_ptr<Patch> extract(int layer, int x, int y) const = 0;
    virtual int getLayerIndex(int width, int height) const = 0;
    virtual double getMinScaleFactor() const = 0;
    virtual double getMaxScaleFactor() const = 0;
    virtual double getIncrementalScaleFactor() const = 0;
    virtual cv::Size getPatchSize() const = 0;
    virtual cv::Size getImageSize() const = 0;
    virtual std::vector<std::pair<int, double>> getLayerScales() const = 0;
    virtual std::vector<cv::Size> getLayerSizes() const = 0;
    virtual std::vector<cv::Size> getPatchSizes() const = 0;
};

// DirectPyramidFeatureExtractor.hpp / .cpp:27-229
class DirectPyramidFeatureExtractor : public PyramidFeatureExtractor {
public:
    using PyramidFeatureExtractor::update;
    using PyramidFeatureExtractor::extract;
    DirectPyramidFeatureExtractor(std::shared_ptr<ImagePyramid> pyramid, int width, int height);
    void addImageFilter(std::shared_ptr<ImageFilter> filter) { pyramid->addImageFilter(filter); }
    void addLayerFilter(std::shared_ptr<ImageFilter> filter) { pyramid->addLayerFilter(filter); }
    void addPatchFilter(std::shared_ptr<ImageFilter> filter);          // HistEq64Filter or one HistogramFilter
    void update(std::shared_ptr<VersionedImage> image) override { pyramid->update(image); }
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override;
    std::vector<std::shared_ptr<Patch>> extract(int stepX, int stepY, cv::Rect roi = cv::Rect(), int firstLayer = -1, int lastLayer = -1,
                                                int stepLayer = 1) const override;
    std::shared_ptr<Patch> extract(int layer, int x, int y) const override;
    // not in the reference: extract(x, y, width, height) for every sample {x - width / 2, y - height / 2, width, height} at once,
    // null for a sample without a window.  One device call (SampledChain::extract) when the extractor has a sampled chain (below: the
    // hog, lbp, glbp and ehog feature types, and the grayscale, h and whi feature types); the per-sample path otherwise.
    // The patch geometry is the one extractFromLayer computes.
    std::vector<std::shared_ptr<Patch>> extract(const std::vector<cv::Rect>& samples) const;
    // the parameters of that device call: kind FD_SAMPLES_HIST (hp) or FD_SAMPLES_EHOG (ep); false: no such chain
    bool getSampledChain(int& kind, fd_hist_params& hp, fd_ehog_patch_params& ep) const;
    // the gray-patch chains of the sampled calls (fd_patch_*_samples): on a gray pyramid without layer filters or source pyramid the patch
    // filters are exactly [ConversionFilter(CV_32F)], [HistEq64Filter, ConversionFilter(CV_32F)], [HistogramEqualizationFilter,
    // ConversionFilter(CV_32F)] or the complete whi chain; false: any other chain
    bool getSampledPatchChain(fd_patch_samples_params& pp) const;
    int getLayerIndex(int width, int height) const override;
    double getMinScaleFactor() const override { return pyramid->getMinScaleFactor(); }
    double getMaxScaleFactor() const override { return pyramid->getMaxScaleFactor(); }
    double getIncrementalScaleFactor() const override { return pyramid->getIncrementalScaleFactor(); }
    cv::Size getPatchSize() const override { return cv::Size(patchWidth, patchHeight); }
    cv::Size getImageSize() const override { return pyramid->getImageSize(); }
    std::vector<std::pair<int, double>> getLayerScales() const override { return pyramid->getLayerScales(); }
    std::vector<cv::Size> getLayerSizes() const override { return pyramid->getLayerSizes(); }
    std::vector<cv::Size> getPatchSizes() const override;
    std::shared_ptr<ImagePyramid> getPyramid() { return pyramid; }
    const std::shared_ptr<ImagePyramid> getPyramid() const { return pyramid; }
    int getPatchWidth() const { return patchWidth; }
    int getPatchHeight() const { return patchHeight; }
    // which fused GPU path the patch filter chain maps to
    bool hasHistEq64() const { return (bool)histeq; }
    std::shared_ptr<HogFilter> getHogFilter() const { return hog; }   // non-interpolating square HogFilter: k_hog_tile path
    std::shared_ptr<HistogramFilter> getHistogramFilter() const { return hist; }
    std::shared_ptr<ExtendedHogFilter> getExtendedHogFilter() const { return ehog; }   // the only patch filter of an ehog chain
    // complete whi chain (WhiteningFilter, HistogramEqualizationFilter, ConversionFilter(CV_32F, 1/127.5, -1), UnitNormFilter(L2))
    std::shared_ptr<WhiteningFilter> getWhiChain() const { return whiStage == 4 ? whitening : nullptr; }
    // u8 feature space (0 gray, 1 hq64 = HistEq64Filter, 2 histeq = HistogramEqualizationFilter) followed by a
    // ConversionFilter(CV_32F, scale, shift): the input of a ProbabilisticRvmClassifier (fd_detect_rvm)
    std::shared_ptr<ConversionFilter> getConversion() const { return whiStage == 0 ? conversion : nullptr; }
    int getU8FeatureSpace() const { return histeq ? 1 : (equalization ? 2 : 0); }
    bool hasPatchFilters() const { return histeq || hist || ehog || whitening || equalization || conversion || reshaping; }
private:
    std::shared_ptr<Patch> extractFromLayer(const ImagePyramidLayer& layer, cv::Rect bounds) const;
    std::shared_ptr<ImagePyramid> pyramid;
    int patchWidth, patchHeight;
    std::shared_ptr<HistEq64Filter> histeq;
    std::shared_ptr<HogFilter> hog;
    std::shared_ptr<HistogramFilter> hist;
    std::shared_ptr<ExtendedHogFilter> ehog;   // alone in the chain: per Mat, and fused for sampled windows (extract(samples))
    std::shared_ptr<WhiteningFilter> whitening;
    std::shared_ptr<HistogramEqualizationFilter> equalization;
    std::shared_ptr<ConversionFilter> conversion;
    std::shared_ptr<ReshapingFilter> reshaping;
    int whiStage = 0;   // number of whi chain filters added so far (in order)
    std::shared_ptr<ChainedFilter> chain = std::make_shared<ChainedFilter>();   // every patch filter in the order added: the per-Mat form of extract(x, y, w, h) / extract(layer, x, y)
};

// FilteringPyramidFeatureExtractor.hpp:20-90 -- applies additional patch filters to the patches of another pyramid feature
// extractor (ffpDetectApp.cpp:445).  When the underlying extractor is a DirectPyramidFeatureExtractor without patch filters of
// its own and the added chain is one the kernels fuse (hq64, histeq, whi, histogram filters, + ConversionFilter /
// ReshapingFilter), the detectors run the fused GPU path (getFusedExtractor()); otherwise every patch goes through the filters'
// per-Mat applyTo, exactly like the reference.
class FilteringPyramidFeatureExtractor : public PyramidFeatureExtractor {
public:
    using PyramidFeatureExtractor::update;
    using PyramidFeatureExtractor::extract;
    explicit FilteringPyramidFeatureExtractor(std::shared_ptr<PyramidFeatureExtractor> extractor);
    void addPatchFilter(std::shared_ptr<ImageFilter> filter);
    void update(std::shared_ptr<VersionedImage> image) override { extractor->update(image); }
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override;
    std::vector<std::shared_ptr<Patch>> extract(int stepX, int stepY, cv::Rect roi = cv::Rect(), int firstLayer = -1, int lastLayer = -1,
                                                int stepLayer = 1) const override;
    std::shared_ptr<Patch> extract(int layer, int x, int y) const override;
    int getLayerIndex(int width, int height) const override { return extractor->getLayerIndex(width, height); }
    double getMinScaleFactor() const override { return extractor->getMinScaleFactor(); }
    double getMaxScaleFactor() const override { return extractor->getMaxScaleFactor(); }
    double getIncrementalScaleFactor() const override { return extractor->getIncrementalScaleFactor(); }
    cv::Size getPatchSize() const override { return extractor->getPatchSize(); }
    cv::Size getImageSize() const override { return extractor->getImageSize(); }
    std::vector<std::pair<int, double>> getLayerScales() const override { return extractor->getLayerScales(); }
    std::vector<cv::Size> getLayerSizes() const override { return extractor->getLayerSizes(); }
    std::vector<cv::Size> getPatchSizes() const override { return extractor->getPatchSizes(); }
    std::shared_ptr<PyramidFeatureExtractor> getExtractor() const { return extractor; }
    // the equivalent DirectPyramidFeatureExtractor (same pyramid, same patch size, the whole chain as its patch filters) when the
    // chain maps to a fused kernel, else null
    std::shared_ptr<DirectPyramidFeatureExtractor> getFusedExtractor() const { return fused; }
private:
    std::shared_ptr<PyramidFeatureExtractor> extractor;
    std::shared_ptr<ChainedFilter> patchFilter;
    std::shared_ptr<DirectPyramidFeatureExtractor> fused;
};

// FilteringFeatureExtractor.hpp:20-62 (ffpDetectApp.cpp:74 includes it): any FeatureExtractor plus patch filters applied per Mat
class FilteringFeatureExtractor : public FeatureExtractor {
public:
    using FeatureExtractor::update;
    explicit FilteringFeatureExtractor(std::shared_ptr<FeatureExtractor> extractor) : extractor(extractor), patchFilter(std::make_shared<ChainedFilter>()) {}
    void addPatchFilter(std::shared_ptr<ImageFilter> filter) { patchFilter->add(filter); }
    void update(std::shared_ptr<VersionedImage> image) override { extractor->update(image); }
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override {
        std::shared_ptr<Patch> patch = extractor->extract(x, y, width, height);
        if (patch) patchFilter->applyInPlace(patch->getData());
        return patch;
    }
private:
    std::shared_ptr<FeatureExtractor> extractor;
    std::shared_ptr<ChainedFilter> patchFilter;
};

// ExtendedHogFeatureExtractor.hpp / ExtendedHogFeatureExtractor.cpp:32-143 in its stand-alone form (:76-84: a CompleteExtendedHogFilter on a
// gray pyramid of its own, createPyramid) on one fd_ehog_tracker.  extract() is ExtendedHogFeatureExtractor::extract (:95-130): the patch
// widened by (cells + 2) / cells, up to one cell outside the layer (mirrored), the inner cells returned (rows x cols * channels CV_32F).
class ExtendedHogFeatureExtractor : public FeatureExtractor {
public:
    using FeatureExtractor::update;
    ExtendedHogFeatureExtractor(std::shared_ptr<CompleteExtendedHogFilter> ehogFilter, int cols, int rows, int minWidth, int maxWidth,
                                int octaveLayerCount = 5);
    ~ExtendedHogFeatureExtractor();
    ExtendedHogFeatureExtractor(const ExtendedHogFeatureExtractor&) = delete;
    ExtendedHogFeatureExtractor& operator=(const ExtendedHogFeatureExtractor&) = delete;
    void update(std::shared_ptr<VersionedImage> image) override;
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override;
    int getPatchWidth() const { return patchWidth; }
    int getPatchHeight() const { return patchHeight; }
    int getCols() const { return cols; }
    int getRows() const { return rows; }
    int getCellSize() const { return cellSize; }
    int getChannels() const { return channels; }
    int getOctaveLayerCount() const { return octaveLayerCount; }
    fd_ehog_tracker* native() const { return tracker; }   // feature pyramid, heat pyramid and sample calls of the same frame
private:
    fd_ehog_tracker* tracker;
    int cols, rows, cellSize, channels, patchWidth, patchHeight, octaveLayerCount;
    double widthFactor, heightFactor;
};

// CellBasedPyramidFeatureExtractor.hpp / CellBasedPyramidFeatureExtractor.cpp:37-78 on the feature pyramid an ExtendedHogFeatureExtractor's
// handle builds (on this backend the pyramid with the CompleteExtendedHogFilter layer filter lives inside the handle, so the extractor is
// constructed from the ExtendedHogFeatureExtractor it shares the gray pyramid with, as the measurement model wires them, instead of
// from an ImagePyramid): extract() returns windows of cols x rows cells (DirectPyramidFeatureExtractor.cpp:67-73,133-143).
class CellBasedPyramidFeatureExtractor : public FeatureExtractor {
public:
    using FeatureExtractor::update;
    explicit CellBasedPyramidFeatureExtractor(std::shared_ptr<ExtendedHogFeatureExtractor> base);
    void update(std::shared_ptr<VersionedImage> image) override { base->update(image); }
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override;
private:
    std::shared_ptr<ExtendedHogFeatureExtractor> base;
};

// one sample map on one sample, through the library's fd_sample_maps_apply (no allocation: extract calls this per patch)
inline void applySampleMap(const fd_sample_map& map, int& x, int& y, int& width, int& height) {
    int32_t s[4] = {x, y, width, height};
    if (fd_sample_maps_apply(&map, 1, 1, s) != FD_OK) throw std::logic_error("applySampleMap: fd_sample_maps_apply refused the map");
    x = s[0]; y = s[1]; width = s[2]; height = s[3];
}

// PatchResizingFeatureExtractor.hpp:21-60 (the `scale` key of createFeatureExtractor): asks the underlying extractor for a patch of
// another size and position and reports the patch with the size and position that were asked for
class PatchResizingFeatureExtractor : public FeatureExtractor {
public:
    using FeatureExtractor::update;
    PatchResizingFeatureExtractor(std::shared_ptr<FeatureExtractor> extractor, double factor, double yOffset = 0, double xOffset = 0)
        : extractor(extractor), factor(factor), yOffset(yOffset), xOffset(xOffset) {}
    void update(std::shared_ptr<VersionedImage> image) override { extractor->update(image); }
    // what the underlying extractor is asked for, as data: the library holds the one copy of the expressions (fd_sample_maps_apply on
    // the host, k_particles_xywh on the device)
    fd_sample_map sampleMap() const { return fd_sample_map{FD_SAMPLE_MAP_RESIZE, factor, xOffset, yOffset}; }
    void mapSample(int& x, int& y, int& width, int& height) const { applySampleMap(sampleMap(), x, y, width, height); }
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override {
        mapSample(x, y, width, height);
        std::shared_ptr<Patch> patch = extractor->extract(x, y, width, height);
        if (patch) {
            patch->setWidth(cv::cvRound(patch->getWidth() / factor));
            patch->setHeight(cv::cvRound(patch->getHeight() / factor));
            patch->setX(cv::cvRound(patch->getX() - xOffset * patch->getWidth()));
            patch->setY(cv::cvRound(patch->getY() - yOffset * patch->getHeight()));
        }
        return patch;
    }
    std::shared_ptr<FeatureExtractor> getExtractor() const { return extractor; }
    double getFactor() const { return factor; }
    double getXOffset() const { return xOffset; }
    double getYOffset() const { return yOffset; }
private:
    std::shared_ptr<FeatureExtractor> extractor;
    double factor, yOffset, xOffset;
};

// IntegralFeatureExtractor.hpp:17-55: a feature extractor on an integral image is asked for a patch one pixel wider and higher (the
// integral image has one row and column more than the image), moved by one where the size is odd
class IntegralFeatureExtractor : public FeatureExtractor {
public:
    using FeatureExtractor::update;
    explicit IntegralFeatureExtractor(std::shared_ptr<FeatureExtractor> extractor) : extractor(extractor) {}
    void update(std::shared_ptr<VersionedImage> image) override { extractor->update(image); }
    // what the underlying extractor is asked for, as data (see PatchResizingFeatureExtractor::sampleMap)
    fd_sample_map sampleMap() const { return fd_sample_map{FD_SAMPLE_MAP_INTEGRAL, 0.0, 0.0, 0.0}; }
    void mapSample(int& x, int& y, int& width, int& height) const { applySampleMap(sampleMap(), x, y, width, height); }
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override {
        const int offsetX = width % 2 == 0 ? 0 : 1, offsetY = height % 2 == 0 ? 0 : 1;
        mapSample(x, y, width, height);
        std::shared_ptr<Patch> patch = extractor->extract(x, y, width, height);
        if (patch) {
            patch->setX(patch->getX() - offsetX);
            patch->setY(patch->getY() - offsetY);
            patch->setWidth(patch->getWidth() - 1);
            patch->setHeight(patch->getHeight() - 1);
        }
        return patch;
    }
    std::shared_ptr<FeatureExtractor> getExtractor() const { return extractor; }
private:
    std::shared_ptr<FeatureExtractor> extractor;
};

// Not in the reference: the chain of PatchResizingFeatureExtractor / IntegralFeatureExtractor wrappers around an extractor, walked
// once.  inner() is the extractor the wrappers end at; map() applies every wrapper's forward map to a sample {x, y, width, height},
// outer to inner, so that the batched device calls receive what the innermost extract(x, y, width, height) would.
class ExtractorWrappers {
public:
    explicit ExtractorWrappers(const FeatureExtractor* outer) : innermost(outer) {
        for (;;) {
            if (auto* resizing = dynamic_cast<const PatchResizingFeatureExtractor*>(innermost)) { maps.push_back(resizing->sampleMap()); innermost = resizing->getExtractor().get(); }
            else if (auto* integral = dynamic_cast<const IntegralFeatureExtractor*>(innermost)) { maps.push_back(integral->sampleMap()); innermost = integral->getExtractor().get(); }
            else break;
        }
    }
    const FeatureExtractor* inner() const { return innermost; }
    bool wrapped() const { return !maps.empty(); }
    // the chain as data, outer to inner, walked once by the constructor: what fd_sample_maps_apply and fd_particles_evaluate_integral take
    const std::vector<fd_sample_map>& sampleMaps() const { return maps; }
    // n samples {x, y, width, height} in place: one library call per FD_SAMPLE_MAPS_MAX wrappers (a longer chain maps the same, in pieces)
    void map(int32_t* xywh, size_t n = 1) const {
        for (size_t first = 0; first < maps.size(); first += FD_SAMPLE_MAPS_MAX)
            if (fd_sample_maps_apply(maps.data() + first, (int)std::min(maps.size() - first, (size_t)FD_SAMPLE_MAPS_MAX), (int)n, xywh) != FD_OK)
                throw std::logic_error("ExtractorWrappers: fd_sample_maps_apply refused the chain");
    }
    void map(int& x, int& y, int& width, int& height) const {
        int32_t s[4] = {x, y, width, height};
        map(s);
        x = s[0]; y = s[1]; width = s[2]; height = s[3];
    }
private:
    const FeatureExtractor* innermost;
    std::vector<fd_sample_map> maps;
};

// Not in the reference: which batched device call serves the samples {x, y, width, height} of an extractor, answered once
// (sampledChainOf) for every model that asks.  A DirectPyramidFeatureExtractor resolves when it is the extractor itself, not wrapped
// (getSampledChain: Hist, Ehog; getSampledPatchChain: Patch); a DirectImageFeatureExtractor resolves through its wrappers, in the
// precedence getHaarChain, getSurfChain, getIntegralHogChain.  Resolving asks no device; ready() does.
class HaarFeatureFilter;
class DirectImageFeatureExtractor;
struct SampledChain {
    enum class Kind { None, Hist, Ehog, Patch, Haar, Surf, IntegralHog };
    explicit SampledChain(const FeatureExtractor* extractor) : wrappers(extractor) {}
    Kind kind = Kind::None;
    fd_hist_params hist{};                     // Hist
    fd_ehog_patch_params ehog{};               // Ehog
    fd_patch_samples_params patch{};           // Patch
    std::shared_ptr<HaarFeatureFilter> haar;   // Haar: fd_haar_params points into the filter
    fd_surf_params surf{};                     // Surf
    fd_integral_hog_params ihog{};             // IntegralHog
    ExtractorWrappers wrappers;                // the wrappers it walked; their inner extractor is one of these two, or neither
    const DirectPyramidFeatureExtractor* pyramid = nullptr;
    const DirectImageFeatureExtractor* image = nullptr;
    bool onPyramid() const { return kind == Kind::Hist || kind == Kind::Ehog || kind == Kind::Patch; }
    bool ready() const;   // the device object of the calls exists: a pyramid kind always, an integral kind after the first update
    bool extractable() const { return onPyramid() || (kind == Kind::IntegralHog && ready()); }   // the kinds extract and hasWindow serve
    int featureLength(int channels) const;   // floats per sample on layers of `channels` channels; negative: invalid, or Haar / Surf
    int matRows() const;                     // of a sample's Mat: cell rows for an ExtendedHogFilter, the patch height for a gray patch, else 1
    // floats per cell where the reference's Mat carries them as channels: those of the inner extractor's ExtendedHogFilter (also behind
    // wrappers, or on layers the sampled calls do not serve), 1 for everything else
    int cellChannels() const;
    // How the library is told about the chain: the handle of its family (one of the two; an integral image is NULL before the first
    // update), the C kind (FD_SAMPLES_* on a pyramid, FD_INTEGRAL_* on an integral image) and the parameter block of that kind.  The
    // blocks live in the chain, which therefore outlives the call; fd_haar_params, which points into the filter, lives in the descriptor
    struct DeviceCall {
        bool onPyramid = false;
        fd_pyramid* pyramid = nullptr;
        fd_integral* integral = nullptr;
        int kind = 0;
        const void* params() const { return block ? block : &haar; }
        const void* block = nullptr;   // into the chain; NULL: haar
        fd_haar_params haar{};
    };
    DeviceCall deviceCall() const;
    // The device conversations, on samples as the outermost extractor receives them.  extract: the patch data of every sample in one
    // fd_hist_ / fd_ehog_ / fd_patch_extract_samples or fd_integral_extract_hog, each Mat as extract(x, y, width, height)->getData()
    // gives it, empty where that returns null.  svmEvaluate: one fd_hist_ / fd_patch_ / fd_integral_svm_evaluate_samples.  hasWindow:
    // whether extract(x, y, width, height) would return a patch, by the rule of the kernels on the host
    std::vector<cv::Mat> extract(const std::vector<int32_t>& xywh) const;
    void svmEvaluate(const fd_svm* svm, const std::vector<int32_t>& xywh, uint8_t* target, double* weight) const;
    bool hasWindow(int x, int y, int width, int height) const;
    std::vector<int32_t> mapped(const std::vector<int32_t>& xywh) const;   // the samples of an integral kind behind the wrappers' maps
};
// mapsApplied: the caller puts every sample through the wrappers' maps itself before the layer rule (the resident particle set, DESIGN.md
// 4.7), so a wrapped DirectPyramidFeatureExtractor resolves too; extract, svmEvaluate and hasWindow are not for such a chain
SampledChain sampledChainOf(const FeatureExtractor* extractor, bool mapsApplied = false);

// ---- the integral-image family: image filters GrayscaleFilter -> IntegralImageFilter of a DirectImageFeatureExtractor, patch filters
// that are a handful of rectangle sums (the "haar" and "surf" feature types of BenchmarkRunner.cpp:202-233,278-286)
// IntegralImageFilter.hpp / IntegralImageFilter.cpp:16-21 (cv::integral): CV_8UC1 -> CV_32SC1, one row and column larger
// (fd_integral_image).  type: -1 or CV_32S; any other depth throws invalid_argument.
class IntegralImageFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit IntegralImageFilter(int type = -1);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
private:
    int type;
};

// A patch filter that reads a window of an integral image.  applyTo(const Mat&) takes the matrix it is given for the whole integral
// image (fd_integral_set_image) -- reads past it, such as a Haar rectangle edge at 1.0, throw invalid_argument; a
// DirectImageFeatureExtractor calls applyToSample with its device-resident integral image instead, where a window's reads may
// leave the window as long as they stay inside the image (like the reference's ROI header on the parent's memory).
class IntegralPatchFilter : public ImageFilter {
public:
    // false: the sample has no patch, or one of the filter's reads lies outside the integral image
    virtual bool applyToSample(fd_integral* integral, int x, int y, int width, int height, cv::Mat& filtered) const = 0;
protected:
    cv::Mat applyToWhole(const cv::Mat& image, cv::Mat& filtered, const char* name) const;
};

// HaarFeatureFilter.hpp:22-115 / HaarFeatureFilter.cpp:18-158 (fd_integral_extract_haar on one sample)
class HaarFeatureFilter : public IntegralPatchFilter {
public:
    using ImageFilter::applyTo;
    static const int TYPE_2RECTANGLE = 1;
    static const int TYPE_3RECTANGLE = 2;
    static const int TYPE_4RECTANGLE = 4;
    static const int TYPE_CENTER_SURROUND = 8;
    static const int TYPES_ALL = TYPE_2RECTANGLE | TYPE_3RECTANGLE | TYPE_4RECTANGLE | TYPE_CENTER_SURROUND;
    HaarFeatureFilter();   // all types, sizes 0.2 and 0.4, 5 x 5 grid
    HaarFeatureFilter(std::vector<float> sizes, unsigned int count, int types = TYPES_ALL);
    HaarFeatureFilter(std::vector<float> sizes, unsigned int xCount, unsigned int yCount, int types = TYPES_ALL);
    HaarFeatureFilter(std::vector<float> sizes, std::vector<float> coords, int types = TYPES_ALL);
    HaarFeatureFilter(std::vector<float> sizes, std::vector<float> xs, std::vector<float> ys, int types = TYPES_ALL);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    bool applyToSample(fd_integral* integral, int x, int y, int width, int height, cv::Mat& filtered) const override;
    fd_haar_params params() const;   // points into this object
    int getFeatureCount() const { return featureCount; }
private:
    void buildFeatures(std::vector<float> sizes, unsigned int xCount, unsigned int yCount, int types);
    void buildFeatures(std::vector<float> sizes, std::vector<float> xs, std::vector<float> ys, int types);
    std::vector<float> sizes, xs, ys;
    int types = TYPES_ALL, featureCount = 0;
};

// IntegralGradientFilter.hpp / IntegralGradientFilter.cpp:19-85 (fd_integral_gradient_patches on one sample): CV_32SC1 -> CV_8UC2
class IntegralGradientFilter : public IntegralPatchFilter {
public:
    using ImageFilter::applyTo;
    IntegralGradientFilter(int rows, int cols) : rows(rows), cols(cols) {}
    explicit IntegralGradientFilter(int count) : rows(count), cols(count) {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    bool applyToSample(fd_integral* integral, int x, int y, int width, int height, cv::Mat& filtered) const override;
    int getRows() const { return rows; }
    int getCols() const { return cols; }
private:
    int rows, cols;
};

// GradientSumFilter.hpp / GradientSumFilter.cpp:18-60 (fd_gradient_sum_batch on one patch): CV_8UC2 -> 1 x rows * cols * 4 CV_32FC1
class GradientSumFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    GradientSumFilter(int rows, int cols) : rows(rows), cols(cols) {}
    explicit GradientSumFilter(int count) : rows(count), cols(count) {}
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int getRows() const { return rows; }
    int getCols() const { return cols; }
private:
    int rows, cols;
};

// DirectImageFeatureExtractor.hpp:25-77 / DirectImageFeatureExtractor.cpp:21-52: patches are windows of the filtered image itself (no
// pyramid).  With the image filters [GrayscaleFilter, IntegralImageFilter] (or [IntegralImageFilter] on gray images) the integral
// image is built and kept on the device (fd_integral_update); an IntegralPatchFilter as first patch filter then reads it there,
// and condensation::SingleClassifierModel scores all samples of a frame in one call for the chains of createHaarExtractor and
// createSurfExtractor.  Any other filter combination runs per Mat on the host copies, like the reference.  A sample whose patch
// exists but whose first filter would read outside the integral image has no patch.
class DirectImageFeatureExtractor : public FeatureExtractor {
public:
    using FeatureExtractor::update;
    DirectImageFeatureExtractor();
    ~DirectImageFeatureExtractor();
    DirectImageFeatureExtractor(const DirectImageFeatureExtractor&) = delete;
    DirectImageFeatureExtractor& operator=(const DirectImageFeatureExtractor&) = delete;
    void addImageFilter(std::shared_ptr<ImageFilter> filter);
    void addPatchFilter(std::shared_ptr<ImageFilter> filter) { patchFilter->add(filter); }
    void update(std::shared_ptr<VersionedImage> image) override;
    std::shared_ptr<Patch> extract(int x, int y, int width, int height) const override;
    // the device-resident integral image of the last update; null when the image filters are another chain
    fd_integral* native() const { return integralChain ? integral : nullptr; }
    // patch filters == [HaarFeatureFilter]
    std::shared_ptr<HaarFeatureFilter> getHaarChain() const;
    // patch filters == [IntegralGradientFilter(g), GradientSumFilter(c), UnitNormFilter(NORM_L2)], both square
    bool getSurfChain(int& gradientCount, int& cellCount) const;
    // patch filters == [IntegralGradientFilter, GradientBinningFilter, one of HogFilter | SpatialHistogramFilter | PyramidHogFilter |
    // SpatialPyramidHistogramFilter | ExtendedHogFilter] (the ihog / iehog feature types) with parameters fd_integral_extract_hog takes
    bool getIntegralHogChain(fd_integral_hog_params& hp) const;
    // the last patch filter where it is an ExtendedHogFilter (the iehog feature type); null otherwise
    std::shared_ptr<ExtendedHogFilter> getExtendedHogFilter() const {
        const auto& f = patchFilter->getFilters();
        return f.empty() ? nullptr : std::dynamic_pointer_cast<ExtendedHogFilter>(f.back());
    }
private:
    const cv::Mat& hostImage() const;
    Version version;
    mutable cv::Mat image;       // the filtered image (for a device-resident integral image: downloaded when first needed)
    mutable bool imageOnHost = true;
    std::shared_ptr<ChainedFilter> imageFilter, patchFilter;
    bool integralChain = false;
    fd_integral* integral = nullptr;
};

// filtering/FhogFilter.hpp:55-56 / FhogFilter.cpp:20-72 (the cell descriptors of the AggregatedFeaturesDetector family)
namespace filtering {
class FhogFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit FhogFilter(int cellSize = 8, int unsignedBinCount = 9, bool interpolateBins = false, bool interpolateCells = true, float alpha = 0.2f);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;   // CV_8UC1 -> rows x cols x (3B+4) CV_32F (stored as rows x cols*(3B+4))
    int cellSize, unsignedBinCount;
    bool interpolateBins, interpolateCells;
    float alpha;
};

// filtering/FpdwFeaturesFilter.hpp:44 / FpdwFeaturesFilter.cpp:21-205: ten channels per pixel of a CV_8UC3 image -- six unsigned
// gradient-orientation bins, the normalised gradient magnitude, L*u*v* (fd_fpdw_image)
class FpdwFeaturesFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    FpdwFeaturesFilter(bool fastGradient, bool interpolate, int normalizationRadius = 5, double normalizationConstant = 0.01);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;   // CV_8UC3 -> rows x cols x 10 CV_32F (stored as rows x cols*10)
    bool fastGradient, interpolate;
    int normalizationRadius;
    double normalizationConstant;
};

// filtering/AggregationFilter.hpp:38 / AggregationFilter.cpp:20-36.  On this backend: the triangular form without normalisation
// (cellSize, true, false), as the second filter of a ChainedFilter behind a FpdwFeaturesFilter (fd_fpdw_cells_image) or in the layer
// filter of an AggregatedFeaturesDetector; box aggregation, normalize = true and applyTo on its own throw logic_error.
class AggregationFilter : public ImageFilter {
public:
    using ImageFilter::applyTo;
    explicit AggregationFilter(int cellSize, bool interpolate = false, bool normalize = false);
    cv::Mat applyTo(const cv::Mat& image, cv::Mat& filtered) const override;
    int cellSize;
};
}  // namespace filtering

// extraction/AggregatedFeaturesExtractor.hpp:27-146 / AggregatedFeaturesExtractor.cpp:23-130.  The feature pyramid lives on the
// device in an fd_aggregated handle (include/fd_hip.h) the extractor creates with its first update.  Feature-pyramid form: the
// pyramid must be an approximated one (ImagePyramid::createApproximated) with a GrayscaleFilter image filter and a
// filtering::FhogFilter layer filter, or no image filter and the FPDW chain, and the minimum scale factor must be adjusted per
// image; such an extractor is also the argument of AggregatedFeaturesDetector's extractor constructor.  Filter forms (.cpp:34-46):
// an exact feature pyramid with octaveLayerCount layers per octave, for the layer filters this backend runs on the device --
// (GrayscaleFilter, filtering::FhogFilter), a filtering::FhogFilter alone (gray images only), or
// ChainedFilter(filtering::FpdwFeaturesFilter, filtering::AggregationFilter) alone; anything else is a logic_error.
namespace extraction {
class AggregatedFeaturesExtractor {
public:
    AggregatedFeaturesExtractor(std::shared_ptr<ImagePyramid> featurePyramid, cv::Size patchSizeInCells, int cellSizeInPixels,
                                bool adjustMinScaleFactor, int minPatchWidthInPixels = 0);
    AggregatedFeaturesExtractor(std::shared_ptr<ImageFilter> layerFilter, cv::Size patchSizeInCells, int cellSizeInPixels, int octaveLayerCount,
                                int minPatchWidthInPixels = 0);
    AggregatedFeaturesExtractor(std::shared_ptr<ImageFilter> imageFilter, std::shared_ptr<ImageFilter> layerFilter, cv::Size patchSizeInCells,
                                int cellSizeInPixels, int octaveLayerCount, int minPatchWidthInPixels = 0);
    ~AggregatedFeaturesExtractor();
    AggregatedFeaturesExtractor(const AggregatedFeaturesExtractor&) = delete;
    AggregatedFeaturesExtractor& operator=(const AggregatedFeaturesExtractor&) = delete;
    std::shared_ptr<ImagePyramid> getFeaturePyramid() { return featurePyramid; }   // null for the filter forms
    cv::Size getPatchSizeInCells() const { return patchSizeInCells; }
    int getCellSizeInPixels() const { return cellSizeInPixels; }
    int getMinPatchWidthInPixels() const { return minPatchWidthInPixels; }
    int getOctaveLayerCount() const { return octaveLayerCount; }
    int getChannelCount() const { return channels; }
    // the feature layers of the image (fd_aggregated_update)
    void update(const cv::Mat& image) { update(std::make_shared<VersionedImage>(image)); }
    void update(std::shared_ptr<VersionedImage> image);
    // the patch of a box in image pixels: data is a patchSizeInCells CV_32FC(channels) Mat, the bounds are those of the cells in
    // image pixels; null where the reference returns null (fd_aggregated_extract)
    std::shared_ptr<Patch> extract(int centerX, int centerY, int width, int height) const;
    std::shared_ptr<Patch> extract(cv::Rect bounds) const;
    // not in the reference: all boxes of an image in one launch; result k is extract(bounds[k])
    std::vector<std::shared_ptr<Patch>> extract(const std::vector<cv::Rect>& bounds) const;
    // not in the reference: the windows of the current image whose score under the SVM exceeds `threshold`, before any non-maximum
    // suppression, in layer / row / column order -- what AggregatedFeaturesDetector(extractor, svm, NonMaximumSuppression(1.0))
    // ::detect(image) returns.  Installs the model in the extractor's handle (fd_aggregated_set_svm); its feature layers stay valid.
    std::vector<std::pair<cv::Rect, float>> detectWindows(const classification::SvmClassifier& svm, float threshold);
    fd_aggregated* native() const { return handle; }
private:
    void init(const ImageFilter* imageFilter, const ImageFilter* layerFilter);
    std::shared_ptr<ImagePyramid> featurePyramid;
    cv::Size patchSizeInCells;
    int cellSizeInPixels, minPatchWidthInPixels, octaveLayerCount = 0, channels = 0;
    bool grayOnly = false, colorOnly = false;   // image types the filters accept
    fd_aggregated* handle = nullptr;
    cv::Mat image;                              // of the last update
};
}  // namespace extraction

}  // namespace imageprocessing
