// featuredetection_amd/host/src/fd_host.cpp -- implementation of the reference-shaped C++ classes
// (host/include/{imageprocessing,classification,detection,superviseddescent}) on top of the C ABI.
// Everything numerical is delegated to libfd_hip.so; this file is object plumbing only.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <sstream>
#include "detection/detection_all.hpp"
#include "superviseddescent/superviseddescent_all.hpp"

using cv::Mat;
using cv::uchar;
using std::make_shared;
using std::shared_ptr;
using std::string;
using std::vector;

namespace fdhost {
fd_ctx* context() {
    static fd_ctx* ctx = nullptr;
    if (!ctx) {
        const char* dev = std::getenv("FD_DEVICE");
        int rc = fd_ctx_create(dev ? std::atoi(dev) : 0, nullptr, &ctx);
        if (rc != FD_OK || !ctx) throw std::runtime_error("fd_ctx_create failed: no usable gfx950 device (this backend has no CPU fallback)");
    }
    return ctx;
}
}  // namespace fdhost
using fdhost::check;
using fdhost::context;
using fdhost::with_capacity;

static Mat contiguous(const Mat& m) { return m.isContinuous() ? m : m.clone(); }

// =================================================================================================
namespace imageprocessing {

Mat GrayscaleFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.channels() == 1) { image.copyTo(filtered); return filtered; }
    // a one-layer pyramid at scale 1 is exactly the grayscale image (resize to the same size is a copy)
    fd_pyramid* p = nullptr;
    check(fd_pyramid_create(context(), 1, 1.0, 1.0, &p));
    Mat src = contiguous(image);
    int rc = fd_pyramid_update(p, src.data, src.cols, src.rows, src.channels(), 0);
    if (rc == FD_OK) {
        filtered.create(src.rows, src.cols, CV_8UC1);
        rc = fd_pyramid_layer_download(p, 0, filtered.data);
    }
    fd_pyramid_destroy(p);
    check(rc);
    return filtered;
}

// the FPDW chain a ChainedFilter may hold: [filtering::FpdwFeaturesFilter, filtering::AggregationFilter] as fd_fpdw_params
static bool fpdw_chain(const ImageFilter* filter, fd_fpdw_params& fp) {
    auto chain = dynamic_cast<const ChainedFilter*>(filter);
    if (!chain || chain->getFilters().size() != 2) return false;
    auto fpdw = std::dynamic_pointer_cast<filtering::FpdwFeaturesFilter>(chain->getFilters()[0]);
    auto agg = std::dynamic_pointer_cast<filtering::AggregationFilter>(chain->getFilters()[1]);
    if (!fpdw || !agg) return false;
    fp = fd_fpdw_params{agg->cellSize, fpdw->fastGradient, fpdw->interpolate, fpdw->normalizationRadius, (float)fpdw->normalizationConstant};
    return true;
}

static Mat fpdw_apply(const Mat& image, const fd_fpdw_params& fp, bool cells, Mat& descriptors) {
    if (image.type() != CV_8UC3)
        throw std::invalid_argument("FpdwFeaturesFilter: the gradient image type must be CV_8UC3 or CV_32FC3, but was " + std::to_string(image.type()) +
                                    " (this backend: CV_8UC3)");
    Mat src = contiguous(image);
    const int rows = cells ? src.rows / fp.cell_size : src.rows, cols = cells ? src.cols / fp.cell_size : src.cols;
    descriptors.create(rows, cols * 10, CV_32FC1);   // the compat Mat has no CV_32FC(n) with n > 4: channels are interleaved in the row
    // an image below one cell has no cells to write, but the call is made all the same: it reports the filters' limits as the reference does
    float none = 0.f;
    float* out = rows > 0 && cols > 0 ? descriptors.ptr<float>(0) : &none;
    check((cells ? fd_fpdw_cells_image : fd_fpdw_image)(context(), src.ptr<uchar>(0), src.cols, src.rows, &fp, out));
    return descriptors;
}

Mat ChainedFilter::applyTo(const Mat& image, Mat& filtered) const {
    fd_fpdw_params fp;
    if (fpdw_chain(this, fp)) return fpdw_apply(image, fp, true, filtered);
    if (filters.empty()) { image.copyTo(filtered); return filtered; }
    filtered = image;
    for (const auto& f : filters) { Mat tmp; f->applyTo(filtered, tmp); filtered = tmp; }
    return filtered;
}

Mat HistEq64Filter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC1) throw std::invalid_argument("HistEq64Filter: the image must be of type CV_8UC1");
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, CV_8UC1);
    check(fd_histeq64_batch(context(), src.data, 1, src.cols, src.rows, dst.data));
    filtered = dst;
    return filtered;
}

Mat GreyWorldNormalizationFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC3) throw std::invalid_argument("GreyWorldNormalizationFilter: The image type must be CV_8UC3");
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, CV_8UC3);
    check(fd_greyworld(context(), src.data, src.cols, src.rows, dst.data, 0));
    filtered = dst;
    return filtered;
}

GradientFilter::GradientFilter(int kernelSize, int blurKernelSize) : kernelSize(kernelSize), blurKernelSize(blurKernelSize) {
    if (kernelSize != 1 && kernelSize != 3 && kernelSize != 5 && kernelSize != 7 && kernelSize != CV_SCHARR)
        throw std::invalid_argument("GradientFilter: the kernel size must be 1, 3, 5, 7 or CV_SCHARR");   // GradientFilter.cpp:16-19
}
// ---- stand-alone ImageFilter::applyTo(const Mat&) forms (ImageFilter.hpp:18-57): one kernel launch per Mat through the C ABI
Mat GradientFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC1) throw std::invalid_argument("GradientFilter: the image must be of type CV_8UC1");
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, CV_8UC2);
    check(fd_gradient_filter_image(context(), src.data, src.cols, src.rows, kernelSize, blurKernelSize > 0 ? blurKernelSize : 0, dst.data));
    filtered = dst;
    return filtered;
}
GradientBinningFilter::GradientBinningFilter(unsigned int bins, bool signedGradients, bool interpolate)
    : bins(bins), signedGradients(signedGradients), interpolate(interpolate) {}
Mat GradientBinningFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC2) throw std::invalid_argument("GradientBinningFilter: the image must be of type CV_8UC2");
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, interpolate ? CV_8UC4 : CV_8UC2);
    check(fd_gradient_binning_image(context(), src.data, src.cols, src.rows, (int)bins, signedGradients, interpolate, dst.data));
    filtered = dst;
    return filtered;
}
Mat GradientMagnitudeFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.channels() != 2) throw std::invalid_argument("GradientMagnitudeFilter: the image must have two channels");   // GradientMagnitudeFilter.cpp:20-21
    if (image.depth() != CV_8U) throw std::invalid_argument("GradientMagnitudeFilter: unsupported image depth " + std::to_string(image.depth()));
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, CV_8UC1);
    check(fd_gradient_magnitude_image(context(), src.data, src.cols, src.rows, dst.data));
    filtered = dst;
    return filtered;
}
Mat LbpFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC1) throw std::invalid_argument("LbpFilter: the image must be of type CV_8UC1");
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, CV_8UC1);
    check(fd_lbp_image(context(), src.data, src.cols, src.rows, (int)type, dst.data));
    filtered = dst;
    return filtered;
}
unsigned int LbpFilter::getBinCount() const {
    switch (type) {
        case Type::LBP8: return 256;
        case Type::LBP8_UNIFORM: return 59;
        default: return 16;
    }
}
Mat WhiteningFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.channels() > 1) throw std::invalid_argument("WhiteningFilter: the image must have exactly one channel");
    if (image.type() != CV_8UC1) throw std::invalid_argument("WhiteningFilter: CV_8UC1 images are supported on this backend");
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, CV_8UC1);
    check(fd_whitening_batch(context(), src.data, 1, src.cols, src.rows, alpha, cutoffFrequency, dst.data));
    filtered = dst;
    return filtered;
}
Mat ConversionFilter::applyTo(const Mat& image, Mat& filtered) const {
    const int sd = image.depth(), dd = type & 7;
    if ((sd != CV_8U && sd != CV_32F) || (dd != CV_8U && dd != CV_32F))
        throw std::invalid_argument("ConversionFilter: CV_8U and CV_32F are supported on this backend");
    Mat src = contiguous(image);
    Mat dst(src.rows, src.cols, CV_MAKETYPE(dd, src.channels()));
    check(fd_convert_batch(context(), src.data, sd == CV_32F ? FD_DTYPE_F32 : FD_DTYPE_U8, (int64_t)src.rows * src.cols * src.channels(), alpha, beta,
                           dst.data, dd == CV_32F ? FD_DTYPE_F32 : FD_DTYPE_U8));
    filtered = dst;
    return filtered;
}
Mat UnitNormFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.channels() > 1) throw std::invalid_argument("UnitNormFilter: The image must have exactly one channel.");
    Mat f32 = image.depth() == CV_32F ? contiguous(image) : ConversionFilter(CV_32F).applyTo(image);   // image.convertTo(filtered, CV_32F)
    Mat dst(f32.rows, f32.cols, CV_32FC1);
    check(fd_unit_norm_batch(context(), f32.ptr<float>(0), 1, f32.rows * f32.cols, normType, dst.ptr<float>(0)));
    filtered = dst;
    return filtered;
}
Mat ZeroMeanUnitVarianceFilter::applyTo(const Mat& image, Mat& filtered) const {   // ZeroMeanUnitVarianceFilter.cpp:21-34
    if (image.channels() > 1) throw std::invalid_argument("ZeroMeanUnitVarianceFilter: The image must have exactly one channel.");
    Mat f32 = image.depth() == CV_32F ? contiguous(image).clone() : ConversionFilter(CV_32F).applyTo(image);   // image.convertTo(filtered, CV_32F)
    const size_t n = (size_t)f32.rows * f32.cols;
    const float* x = f32.ptr<float>(0);
    double s = 0, sq = 0;   // cv::meanStdDev: sums in double, population deviation
    for (size_t i = 0; i < n; ++i) { s += x[i]; sq += (double)x[i] * x[i]; }
    const double mean = n ? s / (double)n : 0.0;
    const double dev = n ? std::sqrt(std::max(sq / (double)n - mean * mean, 0.0)) : 0.0;
    Mat dst(f32.rows, f32.cols, CV_32FC1);
    float* o = dst.ptr<float>(0);
    for (size_t i = 0; i < n; ++i) o[i] = dev == 0 ? 0.f : (float)(((double)x[i] - mean) / dev);
    filtered = dst;
    return filtered;
}
Mat ReshapingFilter::applyTo(const Mat& image, Mat& filtered) const {   // Mat::reshape(cn, rows) of a continuous matrix
    Mat src = contiguous(image).clone();
    const int cn = channels == 0 ? src.channels() : channels;
    const size_t total = (size_t)src.rows * src.cols * src.channels();
    const int r = rows == 0 ? src.rows : rows;
    if (r <= 0 || total % ((size_t)r * cn) != 0) throw std::invalid_argument("ReshapingFilter: the matrix cannot be reshaped to the requested number of rows");
    Mat dst(r, (int)(total / ((size_t)r * cn)), CV_MAKETYPE(src.depth(), cn));
    std::memcpy(dst.data, src.data, total * Mat::elemSizeOf(src.depth()));
    filtered = dst;
    return filtered;
}
Mat HistogramEqualizationFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC1) throw std::invalid_argument("HistogramEqualizationFilter: the image must be of type CV_8UC1");
    Mat src = image.isContinuous() ? image : image.clone();
    filtered.create(src.rows, src.cols, CV_8UC1);
    check(fd_equalize_hist_batch(context(), src.ptr<uchar>(0), 1, src.cols, src.rows, filtered.ptr<uchar>(0)));
    return filtered;
}
HogFilter::HogFilter(int binCount, int cellSize, int blockSize, bool interpolate, bool signedAndUnsigned)
    : HogFilter(binCount, cellSize, cellSize, blockSize, blockSize, interpolate, signedAndUnsigned) {}
HogFilter::HogFilter(int binCount, int cellWidth, int cellHeight, int blockWidth, int blockHeight, bool interpolate, bool signedAndUnsigned)
    : HistogramFilter(Normalization::L2NORM), binCount(binCount), cellWidth(cellWidth), cellHeight(cellHeight), blockWidth(blockWidth),
      blockHeight(blockHeight), interpolate(interpolate), signedAndUnsigned(signedAndUnsigned) {
    if (binCount <= 0) throw std::invalid_argument("HogFilter: binCount must be greater than zero");
    if (cellWidth <= 0) throw std::invalid_argument("HogFilter: cellWidth must be greater than zero");
    if (cellHeight <= 0) throw std::invalid_argument("HogFilter: cellHeight must be greater than zero");
    if (blockWidth <= 0) throw std::invalid_argument("HogFilter: blockWidth must be greater than zero");
    if (blockHeight <= 0) throw std::invalid_argument("HogFilter: blockHeight must be greater than zero");
    if (signedAndUnsigned && binCount % 2 != 0)
        throw std::invalid_argument("HogFilter: the bin size must be even for signed and unsigned gradients to be combined");
}
SpatialHistogramFilter::SpatialHistogramFilter(int binCount, int cellSize, int blockSize, bool interpolate, bool concatenate, Normalization normalization)
    : SpatialHistogramFilter(binCount, cellSize, cellSize, blockSize, blockSize, interpolate, concatenate, normalization) {}
SpatialHistogramFilter::SpatialHistogramFilter(int binCount, int cellWidth, int cellHeight, int blockWidth, int blockHeight, bool interpolate,
                                               bool concatenate, Normalization normalization)
    : HistogramFilter(normalization), binCount(binCount), cellWidth(cellWidth), cellHeight(cellHeight), blockWidth(blockWidth),
      blockHeight(blockHeight), interpolate(interpolate), concatenate(concatenate) {
    if (binCount <= 0) throw std::invalid_argument("SpatialHistogramFilter: binCount must be greater than zero");
    if (cellWidth <= 0) throw std::invalid_argument("SpatialHistogramFilter: cellWidth must be greater than zero");
    if (cellHeight <= 0) throw std::invalid_argument("SpatialHistogramFilter: cellHeight must be greater than zero");
    if (blockWidth <= 0) throw std::invalid_argument("SpatialHistogramFilter: blockWidth must be greater than zero");
    if (blockHeight <= 0) throw std::invalid_argument("SpatialHistogramFilter: blockHeight must be greater than zero");
}
static Mat hist_apply(const HistogramFilter& f, const Mat& image, Mat& filtered);
Mat SpatialHistogramFilter::applyTo(const Mat& image, Mat& filtered) const { return hist_apply(*this, image, filtered); }
PyramidHogFilter::PyramidHogFilter(int binCount, int levelCount, bool interpolate, bool signedAndUnsigned)
    : HistogramFilter(Normalization::L2NORM), binCount(binCount), levelCount(levelCount), interpolate(interpolate),
      signedAndUnsigned(signedAndUnsigned) {
    if (binCount <= 0) throw std::invalid_argument("PyramidHogFilter: binCount must be greater than zero");
    if (levelCount <= 0) throw std::invalid_argument("PyramidHogFilter: levelCount must be greater than zero");
    if (signedAndUnsigned && binCount % 2 != 0)
        throw std::invalid_argument("PyramidHogFilter: the bin size must be even for signed and unsigned gradients to be combined");
}
Mat PyramidHogFilter::applyTo(const Mat& image, Mat& filtered) const { return hist_apply(*this, image, filtered); }
SpatialPyramidHistogramFilter::SpatialPyramidHistogramFilter(int binCount, int levelCount, bool interpolate, Normalization normalization)
    : HistogramFilter(normalization), binCount(binCount), levelCount(levelCount), interpolate(interpolate) {
    if (binCount <= 0) throw std::invalid_argument("SpatialPyramidHistogramFilter: binCount must be greater than zero");
    if (levelCount <= 0) throw std::invalid_argument("SpatialPyramidHistogramFilter: levelCount must be greater than zero");
}
Mat SpatialPyramidHistogramFilter::applyTo(const Mat& image, Mat& filtered) const { return hist_apply(*this, image, filtered); }

// parameters of the fused histogram kernels for a patch filter
static fd_hist_params hist_params_of(const HistogramFilter& f, int pw, int ph, int stepX, int stepY) {
    fd_hist_params hp;
    std::memset(&hp, 0, sizeof(hp));
    hp.patch_w = pw; hp.patch_h = ph; hp.step_x = stepX; hp.step_y = stepY;
    hp.normalization = (int)f.normalization;
    if (auto h = dynamic_cast<const HogFilter*>(&f)) {
        hp.kind = FD_HIST_HOG; hp.bins = h->binCount; hp.cell_size = h->cellWidth; hp.cell_h = h->cellHeight;
        hp.block_size = h->blockWidth; hp.block_h = h->blockHeight; hp.interpolate = h->interpolate; hp.signed_and_unsigned = h->signedAndUnsigned;
    } else if (auto s = dynamic_cast<const SpatialHistogramFilter*>(&f)) {
        hp.kind = FD_HIST_SPATIAL; hp.bins = s->binCount; hp.cell_size = s->cellWidth; hp.cell_h = s->cellHeight;
        hp.block_size = s->blockWidth; hp.block_h = s->blockHeight; hp.interpolate = s->interpolate; hp.concatenate = s->concatenate;
    } else if (auto q = dynamic_cast<const PyramidHogFilter*>(&f)) {
        hp.kind = FD_HIST_PYRAMID_HOG; hp.bins = q->binCount; hp.levels = q->levelCount; hp.interpolate = q->interpolate;
        hp.signed_and_unsigned = q->signedAndUnsigned;
    } else if (auto y = dynamic_cast<const SpatialPyramidHistogramFilter*>(&f)) {
        hp.kind = FD_HIST_SPATIAL_PYRAMID; hp.bins = y->binCount; hp.levels = y->levelCount; hp.interpolate = y->interpolate;
    } else {
        throw std::logic_error("unsupported HistogramFilter subclass");
    }
    return hp;
}
// HistogramFilter::applyTo(const Mat&): the bin image of one patch (CV_8UC1 bins, CV_8UC2 bin + weight, CV_8UC4 two bins + weights)
// -> 1 x F CV_32F feature vector
static Mat hist_apply(const HistogramFilter& f, const Mat& image, Mat& filtered) {
    if (image.depth() != CV_8U || (image.channels() != 1 && image.channels() != 2 && image.channels() != 4))
        throw std::invalid_argument("HistogramFilter: The image must have one, two or four channels and be of depth CV_8U");
    Mat src = contiguous(image);
    fd_hist_params hp = hist_params_of(f, src.cols, src.rows, 1, 1);
    const int F = fd_hist_feature_length(&hp, src.channels());
    if (F < 0) throw std::invalid_argument("HistogramFilter: invalid parameters for this patch size");
    Mat dst(1, F, CV_32FC1);
    check(fd_hist_patch_batch(context(), src.data, 1, src.channels(), &hp, dst.ptr<float>(0)));
    filtered = dst;
    return filtered;
}
Mat HogFilter::applyTo(const Mat& image, Mat& filtered) const { return hist_apply(*this, image, filtered); }

// ---- ExtendedHogFilter (ExtendedHogFilter.cpp:14-61), CompleteExtendedHogFilter (CompleteExtendedHogFilter.cpp:19-70) -----------------
ExtendedHogFilter::ExtendedHogFilter(int binCount, int cellSize, bool interpolate, bool signedAndUnsigned, float alpha)
    : HistogramFilter(Normalization::L2HYS), binCount(binCount), cellWidth(cellSize), cellHeight(cellSize), interpolate(interpolate),
      signedAndUnsigned(signedAndUnsigned), alpha(alpha) {
    if (binCount <= 0) throw std::invalid_argument("ExtendedHogFilter: binCount must be greater than zero");
    if (cellSize <= 0) throw std::invalid_argument("ExtendedHogFilter: cellSize must be greater than zero");
    if (signedAndUnsigned && binCount % 2 != 0)
        throw std::invalid_argument("ExtendedHogFilter: the bin size must be even for signed and unsigned gradients to be combined");
    if (alpha <= 0) throw std::invalid_argument("ExtendedHogFilter: alpha must be greater than zero");
}
ExtendedHogFilter::ExtendedHogFilter(int binCount, int cellWidth, int cellHeight, bool interpolate, bool signedAndUnsigned, float alpha)
    : HistogramFilter(Normalization::L2HYS), binCount(binCount), cellWidth(cellWidth), cellHeight(cellHeight), interpolate(interpolate),
      signedAndUnsigned(signedAndUnsigned), alpha(alpha) {
    if (binCount <= 0) throw std::invalid_argument("ExtendedHogFilter: binCount must be greater than zero");
    if (cellWidth <= 0) throw std::invalid_argument("ExtendedHogFilter: cellWidth must be greater than zero");
    if (cellHeight <= 0) throw std::invalid_argument("ExtendedHogFilter: cellHeight must be greater than zero");
    if (signedAndUnsigned && binCount % 2 != 0)
        throw std::invalid_argument("ExtendedHogFilter: the bin size must be even for signed and unsigned gradients to be combined");
    if (alpha <= 0) throw std::invalid_argument("ExtendedHogFilter: alpha must be greater than zero");
}
Mat ExtendedHogFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.depth() != CV_8U || (image.channels() != 1 && image.channels() != 2 && image.channels() != 4))
        throw std::invalid_argument("HistogramFilter: The image must have one, two or four channels and be of depth CV_8U");
    Mat src = contiguous(image);
    fd_ehog_patch_params ep = {src.cols, src.rows, binCount, cellWidth, cellHeight, interpolate, signedAndUnsigned, alpha};
    const int F = fd_ehog_feature_length(&ep, src.channels());
    if (F < 0) throw std::invalid_argument("ExtendedHogFilter: the patch is smaller than one cell");
    const int rows = cv::cvRound(static_cast<double>(src.rows) / static_cast<double>(cellHeight));
    Mat dst(rows, F / rows, CV_32FC1);   // the compat Mat has no CV_32FC(n) with n > 4: channels are interleaved in the row
    check(fd_ehog_patch_batch(context(), src.data, 1, src.channels(), &ep, dst.ptr<float>(0)));
    filtered = dst;
    return filtered;
}

CompleteExtendedHogFilter::CompleteExtendedHogFilter(size_t cellSize, size_t binCount, bool signedGradients, bool unsignedGradients,
                                                     bool interpolateBins, bool interpolateCells, float alpha)
    : cellSize(cellSize), binCount(binCount), signedGradients(signedGradients), unsignedGradients(unsignedGradients),
      interpolateBins(interpolateBins), interpolateCells(interpolateCells), alpha(alpha) {
    if (!signedGradients && !unsignedGradients)
        throw std::invalid_argument("CompleteExtendedHogFilter: signedGradients or unsignedGradients has to be true");
    if (signedGradients && unsignedGradients && binCount % 2 != 0)
        throw std::invalid_argument("CompleteExtendedHogFilter: if both signed and unsigned gradients should be used, the bin count has to be even");
    if (cellSize < 1 || binCount < 1) throw std::invalid_argument("CompleteExtendedHogFilter: cellSize and binCount must be greater than zero");
}
fd_cehog_params CompleteExtendedHogFilter::params() const {
    return fd_cehog_params{(int32_t)cellSize, (int32_t)binCount, signedGradients, unsignedGradients, interpolateBins, interpolateCells, alpha};
}
Mat CompleteExtendedHogFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC1) throw std::invalid_argument("CompleteExtendedHogFilter: image must be of type CV_8UC1");
    Mat src = contiguous(image);
    const fd_cehog_params fp = params();
    const int rows = src.rows / (int)cellSize, cols = src.cols / (int)cellSize, D = (int)getDescriptorSize();
    filtered.create(rows, cols * D, CV_32FC1);   // channels interleaved in the row, as for FhogFilter
    if (rows > 0 && cols > 0) check(fd_cehog_image(context(), src.ptr<uchar>(0), src.cols, src.rows, &fp, filtered.ptr<float>(0)));
    return filtered;
}

// ---- ImagePyramid -------------------------------------------------------------------------------
static const char* const kImageFilterChains =
    "ImagePyramid: the image filter chains available on this backend are [GrayscaleFilter] and "
    "[GreyWorldNormalizationFilter, GrayscaleFilter]";
ImagePyramid::ImagePyramid(size_t octaveLayerCount, double minS, double maxS)
    : handle(nullptr), minScaleFactor(minS), maxScaleFactor(maxS), ctorOctaveLayers(octaveLayerCount), layersValid(false) {
    check(fd_pyramid_create(context(), (int)octaveLayerCount, minS, maxS, &handle));
}
ImagePyramid::ImagePyramid(double inc, double minS, double maxS)
    : handle(nullptr), minScaleFactor(minS), maxScaleFactor(maxS), ctorIncremental(inc), layersValid(false) {
    check(fd_pyramid_create_inc(context(), inc, minS, maxS, &handle));
}
fd_pyramid* ImagePyramid::createFramesPyramid(int frames) const {
    if (sourcePyramid || !handle || gradient || binning || lbp) return nullptr;
    if (!imageChain.empty() && imageChain.back() != FD_IMAGE_GRAY) throw std::logic_error(kImageFilterChains);
    fd_pyramid* p = nullptr;
    if (ctorOctaveLayers) check(fd_pyramid_create(context(), (int)ctorOctaveLayers, minScaleFactor, maxScaleFactor, &p));
    else check(fd_pyramid_create_inc(context(), ctorIncremental, minScaleFactor, maxScaleFactor, &p));
    int rc = fd_pyramid_set_frames(p, frames);
    if (rc == FD_OK) rc = fd_pyramid_set_image_filter(p, fd_pyramid_image_filter(handle));
    if (rc != FD_OK) { fd_pyramid_destroy(p); check(rc); }
    return p;
}
ImagePyramid::ImagePyramid(shared_ptr<ImagePyramid> pyramid, double minS, double maxS)
    : handle(nullptr), sourcePyramid(pyramid), minScaleFactor(minS), maxScaleFactor(maxS), layersValid(false) {
    if (!pyramid) throw std::invalid_argument("ImagePyramid: the source pyramid must not be null");
}
// ImagePyramid.cpp:51-63.  The approximated pyramid holds no native pyramid: it records what fd_aggregated_create_approximated needs.
ImagePyramid::ImagePyramid(Approximated, size_t octaveLayerCount, double minS, double maxS, vector<double> lambdas)
    : handle(nullptr), minScaleFactor(minS), maxScaleFactor(maxS), ctorOctaveLayers(octaveLayerCount), layersValid(false), approximated(true),
      lambdas(std::move(lambdas)) {
    if (octaveLayerCount == 0) throw std::invalid_argument("ImagePyramid: the number of layers per octave must be greater than zero");
    if (minS <= 0) throw std::invalid_argument("ImagePyramid: the minimum scale factor must be greater than zero");
    if (maxS > 1) throw std::invalid_argument("ImagePyramid: the maximum scale factor must not exceed one");
}
shared_ptr<ImagePyramid> ImagePyramid::createApproximated(int octaveLayerCount, double minS, double maxS, vector<double> lambdas) {
    return shared_ptr<ImagePyramid>(new ImagePyramid(Approximated{}, (size_t)std::max(octaveLayerCount, 0), minS, maxS, std::move(lambdas)));
}
shared_ptr<ImagePyramid> ImagePyramid::createApproximated(shared_ptr<ImagePyramid>, int, vector<double>) {
    throw std::logic_error("ImagePyramid: approximating the layers of an arbitrary source pyramid is not available on this backend "
                           "(createApproximated(octaveLayerCount, min, max, lambdas) is)");
}
void ImagePyramid::requireExact() const {
    if (approximated)
        throw std::logic_error("ImagePyramid: an approximated pyramid is available as the feature pyramid of an AggregatedFeaturesExtractor "
                               "behind an AggregatedFeaturesDetector only");
}
ImagePyramid::~ImagePyramid() { if (handle) fd_pyramid_destroy(handle); }
double ImagePyramid::getIncrementalScaleFactor() const {
    if (approximated) return std::pow(0.5, 1. / ctorOctaveLayers);
    return fd_pyramid_incremental_scale(native());
}
static long g_pyramidBuilds = 0;
long ImagePyramid::buildCount() { return g_pyramidBuilds; }

// The image-filter chain is recorded and mapped to the native pyramid's setting (fd_pyramid_set_image_filter); the filters
// themselves run inside the pyramid kernels.  A GrayscaleFilter behind a GrayscaleFilter copies (GrayscaleFilter.cpp:18-24) and is
// not recorded again.
void ImagePyramid::addImageFilter(const shared_ptr<ImageFilter>& filter) {
    const bool gray = std::dynamic_pointer_cast<GrayscaleFilter>(filter) != nullptr;
    const bool greyWorld = std::dynamic_pointer_cast<GreyWorldNormalizationFilter>(filter) != nullptr;
    const bool endsGray = !imageChain.empty() && imageChain.back() == FD_IMAGE_GRAY;
    if (!gray && !(greyWorld && imageChain.empty())) throw std::logic_error(kImageFilterChains);
    if (!(gray && endsGray)) imageChain.push_back(gray ? FD_IMAGE_GRAY : FD_IMAGE_GREYWORLD_GRAY);
    if (handle) check(fd_pyramid_set_image_filter(handle, imageChain.front()));
    version = Version();   // the next update builds the layers again
    if (sourcePyramid) sourcePyramid->addImageFilter(filter);   // ImagePyramid.cpp:108-110
}
void ImagePyramid::setSource(const shared_ptr<VersionedImage>& image) {
    requireExact();
    if (sourcePyramid && !handle)
        throw std::logic_error("ImagePyramid: a pyramid that was constructed on another pyramid has no layer parameters of its own to build from an image");
    sourcePyramid.reset();
    sourceImage = image;
}
void ImagePyramid::setSource(const shared_ptr<ImagePyramid>& pyramid) {
    if (!pyramid) throw std::invalid_argument("ImagePyramid: the source pyramid must not be null");
    requireExact();
    if (gradient || binning || lbp) throw std::logic_error("ImagePyramid: layer filters on top of a source pyramid are not available on this backend");
    sourceImage.reset();
    sourcePyramid = pyramid;
    version = Version();
    layersValid = false;
}
void ImagePyramid::update() {   // ImagePyramid.cpp:146-168
    requireExact();
    if (sourcePyramid) {
        if (version != sourcePyramid->version) { version = sourcePyramid->version; imageSize = sourcePyramid->imageSize; layersValid = false; }
    } else if (sourceImage) {
        update(sourceImage);
    }
}
// layer indices of the source pyramid whose scale factors lie inside [minScaleFactor, maxScaleFactor] (ImagePyramid.cpp:217-222)
void ImagePyramid::viewRange(int& first, int& last) const {
    first = -1; last = -1;
    if (!sourcePyramid) return;
    first = 1 << 30; last = -2;   // empty unless a layer qualifies
    for (const auto& sc : sourcePyramid->getLayerScales())
        if (sc.second >= minScaleFactor && sc.second <= maxScaleFactor) { first = std::min(first, sc.first); last = std::max(last, sc.first); }
}
ImagePyramid::Selection::Selection(fd_pyramid* h, int first, int last, int step, const cv::Rect* roi, int viewFirst, int viewLast) : handle(h) {
    int r[4] = {0, 0, 0, 0};
    if (roi) { r[0] = roi->x; r[1] = roi->y; r[2] = roi->width; r[3] = roi->height; }
    // an empty range (first > last) selects nothing: express it as an index range no layer has
    if (last != -1 && first > last) { first = 1 << 30; last = 1 << 30; }
    check(fd_pyramid_select(handle, first, last, step, roi ? r : nullptr));
    // the layer step of extract() walks getLayers() of THIS pyramid: a view starts counting at its own first layer
    check(fd_pyramid_select_view(handle, viewFirst, viewLast));
}
ImagePyramid::Selection::~Selection() {
    if (handle) { fd_pyramid_select(handle, -1, -1, 1, nullptr); fd_pyramid_select_view(handle, -1, -1); }
}
ImagePyramid::Selection ImagePyramid::select(int firstLayer, int lastLayer, int stepLayer, const cv::Rect* roi) const {
    if (stepLayer < 1) throw std::invalid_argument("DirectPyramidFeatureExtractor: stepLayer has to be greater than zero");
    int vf, vl;
    viewRange(vf, vl);
    if (sourcePyramid) {   // intersect with the view's scale range
        firstLayer = firstLayer < 0 ? vf : std::max(firstLayer, vf);
        lastLayer = lastLayer < 0 ? vl : std::min(lastLayer, vl);
        if (vl == -2) { firstLayer = 1; lastLayer = 0; }
    }
    const cv::Rect* r = (roi && (roi->x != 0 || roi->y != 0 || roi->width != 0 || roi->height != 0)) ? roi : nullptr;
    const bool view = sourcePyramid && vl != -2;
    return Selection(native(), firstLayer, lastLayer, stepLayer, r, view ? vf : -1, view ? vl : -1);
}
void ImagePyramid::addLayerFilter(const shared_ptr<ImageFilter>& filter) {
    if (approximated) {
        fd_fpdw_params fp;
        if (approxLayerFilter || (!std::dynamic_pointer_cast<filtering::FhogFilter>(filter) && !fpdw_chain(filter.get(), fp)))
            throw std::logic_error("ImagePyramid: the layer filter of an approximated pyramid is one filtering::FhogFilter or one "
                                   "ChainedFilter(filtering::FpdwFeaturesFilter, filtering::AggregationFilter) on this backend");
        approxLayerFilter = filter;
        return;
    }
    if (sourcePyramid) throw std::logic_error("ImagePyramid: layer filters on top of a source pyramid are not available on this backend");
    if (auto g = std::dynamic_pointer_cast<GradientFilter>(filter)) gradient = g;
    else if (auto b = std::dynamic_pointer_cast<GradientBinningFilter>(filter)) binning = b;
    else if (auto l = std::dynamic_pointer_cast<LbpFilter>(filter)) lbp = l;
    else if (auto m = std::dynamic_pointer_cast<GradientMagnitudeFilter>(filter)) {
        if (!gradient || binning || lbp) throw std::logic_error("ImagePyramid: GradientMagnitudeFilter is available in the chain GradientFilter, GradientMagnitudeFilter, LbpFilter");
        magnitude = m;
    }
    else throw std::logic_error("ImagePyramid: unsupported layer filter (GradientFilter, GradientBinningFilter, GradientMagnitudeFilter, LbpFilter are available)");
    applyLayerFilterConfig();
}
void ImagePyramid::applyLayerFilterConfig() {
    if (gradient && binning)
    {
        check(fd_pyramid_set_layer_filter(handle, FD_LAYER_GRADBIN, (int)binning->bins, binning->signedGradients, binning->interpolate,
                                          gradient->kernelSize, 0));
        check(fd_pyramid_set_gradient_blur(handle, gradient->blurKernelSize > 0 ? gradient->blurKernelSize : 0));
    }
    else if (gradient && magnitude && lbp)
    {
        check(fd_pyramid_set_layer_filter(handle, FD_LAYER_GRADMAG_LBP, 0, 0, 0, gradient->kernelSize, (int)lbp->type));
        check(fd_pyramid_set_gradient_blur(handle, gradient->blurKernelSize > 0 ? gradient->blurKernelSize : 0));
    }
    else if (lbp && !gradient)
        check(fd_pyramid_set_layer_filter(handle, FD_LAYER_LBP, 0, 0, 0, 1, (int)lbp->type));
    version = Version();
}
void ImagePyramid::update(const Mat& image) { update(make_shared<VersionedImage>(image)); }
void ImagePyramid::update(const shared_ptr<VersionedImage>& image) {
    requireExact();
    if (sourcePyramid) {   // ImagePyramid.cpp:121-124: the source pyramid is updated (once per image version), this one follows
        sourcePyramid->update(image);
        update();
        return;
    }
    if (magnitude ? (!gradient || !lbp || binning) : ((gradient != nullptr) != (binning != nullptr)))
        throw std::logic_error("ImagePyramid: GradientFilter and GradientBinningFilter have to be added together");
    // a GreyWorldNormalizationFilter alone would give three-channel layers
    if (!imageChain.empty() && imageChain.back() != FD_IMAGE_GRAY) throw std::logic_error(kImageFilterChains);
    sourceImage = image;
    if (version == image->getVersion()) return;   // ImagePyramid.cpp:150
    Mat src = contiguous(image->getData());
    check(fd_pyramid_update(handle, src.data, src.cols, src.rows, src.channels(), 0));
    ++g_pyramidBuilds;
    imageSize = cv::Size(src.cols, src.rows);
    version = image->getVersion();
    layersValid = false;
}
const vector<shared_ptr<ImagePyramidLayer>>& ImagePyramid::getLayers() const {
    requireExact();
    if (sourcePyramid) {
        if (!layersValid) {
            layers.clear();
            for (const auto& l : sourcePyramid->getLayers())
                if (l->getScaleFactor() >= minScaleFactor && l->getScaleFactor() <= maxScaleFactor) layers.push_back(l);
            layersValid = true;
        }
        return layers;
    }
    if (!layersValid) {
        layers.clear();
        const int n = fd_pyramid_layer_count(handle);
        for (int i = 0; i < n; ++i) {
            int index, w, h, ch;
            double scale;
            check(fd_pyramid_layer_info(handle, i, &index, &scale, &w, &h, &ch));
            Mat img(h, w, CV_MAKETYPE(CV_8U, ch));
            check(fd_pyramid_layer_download(handle, i, img.data));
            layers.push_back(make_shared<ImagePyramidLayer>(index, scale, (double)w / imageSize.width, (double)h / imageSize.height, img));
        }
        layersValid = true;
    }
    return layers;
}
const shared_ptr<ImagePyramidLayer> ImagePyramid::getLayer(int index) const {
    const auto& ls = getLayers();
    if (ls.empty()) return shared_ptr<ImagePyramidLayer>();
    int real = index - ls.front()->getIndex();
    if (real < 0 || real >= (int)ls.size()) return shared_ptr<ImagePyramidLayer>();
    return ls[real];
}
vector<std::pair<int, double>> ImagePyramid::getLayerScales() const {
    requireExact();
    vector<std::pair<int, double>> out;
    if (sourcePyramid) {
        for (const auto& sc : sourcePyramid->getLayerScales())
            if (sc.second >= minScaleFactor && sc.second <= maxScaleFactor) out.push_back(sc);
        return out;
    }
    for (int i = 0; i < fd_pyramid_layer_count(handle); ++i) {
        int index, w, h, ch; double scale;
        fd_pyramid_layer_info(handle, i, &index, &scale, &w, &h, &ch);
        out.emplace_back(index, scale);
    }
    return out;
}
vector<cv::Size> ImagePyramid::getLayerSizes() const {
    requireExact();
    vector<cv::Size> out;
    if (sourcePyramid) {
        auto scales = sourcePyramid->getLayerScales();
        auto sizes = sourcePyramid->getLayerSizes();
        for (size_t i = 0; i < scales.size(); ++i)
            if (scales[i].second >= minScaleFactor && scales[i].second <= maxScaleFactor) out.push_back(sizes[i]);
        return out;
    }
    for (int i = 0; i < fd_pyramid_layer_count(handle); ++i) {
        int index, w, h, ch; double scale;
        fd_pyramid_layer_info(handle, i, &index, &scale, &w, &h, &ch);
        out.push_back(cv::Size(w, h));
    }
    return out;
}

// ---- the integral-image family ---------------------------------------------------------------------------------------------------
IntegralImageFilter::IntegralImageFilter(int type) : type(type) {
    if (type != -1 && (type & 7) != CV_32S) throw std::invalid_argument("IntegralImageFilter: this backend computes CV_32S integral images only (type -1 or CV_32S)");
}
Mat IntegralImageFilter::applyTo(const Mat& image, Mat& filtered) const {   // cv::integral(image, filtered, CV_32S)
    if (image.type() != CV_8UC1) throw std::invalid_argument("IntegralImageFilter: the image must be of type CV_8UC1");
    Mat src = contiguous(image);
    Mat dst(src.rows + 1, src.cols + 1, CV_32SC1);
    check(fd_integral_image(context(), src.data, src.cols, src.rows, dst.ptr<int32_t>(0)));
    filtered = dst;
    return filtered;
}

namespace {
struct IntegralHandle {   // owns a fd_integral for the duration of one stand-alone applyTo
    fd_integral* g = nullptr;
    IntegralHandle() { check(fd_integral_create(context(), &g)); }
    ~IntegralHandle() { fd_integral_destroy(g); }
};
}  // namespace

Mat IntegralPatchFilter::applyToWhole(const Mat& image, Mat& filtered, const char* name) const {
    if (image.type() != CV_32SC1) throw std::invalid_argument(string(name) + ": the image must be of type CV_32SC1");
    Mat src = contiguous(image);
    IntegralHandle h;
    check(fd_integral_set_image(h.g, src.ptr<int32_t>(0), src.cols, src.rows));
    if (!applyToSample(h.g, src.cols / 2, src.rows / 2, src.cols, src.rows, filtered))
        throw std::invalid_argument(string(name) + ": the filter reads outside of the given matrix (a window of a larger integral image goes through DirectImageFeatureExtractor)");
    return filtered;
}

HaarFeatureFilter::HaarFeatureFilter() {
    vector<float> s;
    s.push_back(0.2f);
    s.push_back(0.4f);
    buildFeatures(s, 5, 5, TYPES_ALL);
}
HaarFeatureFilter::HaarFeatureFilter(vector<float> sizes, unsigned int count, int types) { buildFeatures(sizes, count, count, types); }
HaarFeatureFilter::HaarFeatureFilter(vector<float> sizes, unsigned int xCount, unsigned int yCount, int types) { buildFeatures(sizes, xCount, yCount, types); }
HaarFeatureFilter::HaarFeatureFilter(vector<float> sizes, vector<float> coords, int types) { buildFeatures(sizes, coords, coords, types); }
HaarFeatureFilter::HaarFeatureFilter(vector<float> sizes, vector<float> xs, vector<float> ys, int types) { buildFeatures(sizes, xs, ys, types); }
void HaarFeatureFilter::buildFeatures(vector<float> sizes, unsigned int xCount, unsigned int yCount, int types) {   // HaarFeatureFilter.cpp:41-51
    vector<float> gx(xCount), gy(yCount);
    if (fd_haar_grid((int)xCount, gx.data()) != FD_OK || fd_haar_grid((int)yCount, gy.data()) != FD_OK) throw std::invalid_argument("HaarFeatureFilter: invalid grid size");
    buildFeatures(sizes, gx, gy, types);
}
void HaarFeatureFilter::buildFeatures(vector<float> sizes_, vector<float> xs_, vector<float> ys_, int types_) {
    sizes = sizes_; xs = xs_; ys = ys_; types = types_;
    const fd_haar_params hp = params();
    featureCount = fd_haar_feature_count(&hp);
    if (featureCount < 0) throw std::invalid_argument("HaarFeatureFilter: invalid parameters (types outside 1|2|4|8, or a rectangle edge outside [0, 1])");
}
fd_haar_params HaarFeatureFilter::params() const {
    fd_haar_params hp;
    hp.sizes = sizes.data(); hp.num_sizes = (int32_t)sizes.size();
    hp.xs = xs.data(); hp.num_xs = (int32_t)xs.size();
    hp.ys = ys.data(); hp.num_ys = (int32_t)ys.size();
    hp.types = types;
    return hp;
}
Mat HaarFeatureFilter::applyTo(const Mat& image, Mat& filtered) const { return applyToWhole(image, filtered, "HaarFeatureFilter"); }
bool HaarFeatureFilter::applyToSample(fd_integral* integral, int x, int y, int width, int height, Mat& filtered) const {
    const int32_t xywh[4] = {x, y, width, height};
    const fd_haar_params hp = params();
    Mat dst(1, featureCount, CV_32FC1);
    uint8_t valid = 0;
    check(fd_integral_extract_haar(context(), integral, &hp, 1, xywh, dst.ptr<float>(0), &valid));
    filtered = dst;
    return valid != 0;
}

Mat IntegralGradientFilter::applyTo(const Mat& image, Mat& filtered) const { return applyToWhole(image, filtered, "IntegralGradientFilter"); }
bool IntegralGradientFilter::applyToSample(fd_integral* integral, int x, int y, int width, int height, Mat& filtered) const {
    const int32_t xywh[4] = {x, y, width, height};
    Mat dst(std::max(rows, 1), std::max(cols, 1), CV_8UC2);
    uint8_t valid = 0;
    check(fd_integral_gradient_patches(context(), integral, rows, cols, 1, xywh, dst.data, &valid));
    filtered = dst;
    return valid != 0;
}

Mat GradientSumFilter::applyTo(const Mat& image, Mat& filtered) const {
    if (image.type() != CV_8UC2) throw std::invalid_argument("GradientSumFilter: the image must be of type CV_8UC2");
    Mat src = contiguous(image);
    Mat dst(1, std::max(rows, 1) * std::max(cols, 1) * 4, CV_32FC1);
    check(fd_gradient_sum_batch(context(), src.data, 1, src.rows, src.cols, rows, cols, dst.ptr<float>(0)));
    filtered = dst;
    return filtered;
}

DirectImageFeatureExtractor::DirectImageFeatureExtractor() : version(), image(), imageFilter(make_shared<ChainedFilter>()), patchFilter(make_shared<ChainedFilter>()) {}
DirectImageFeatureExtractor::~DirectImageFeatureExtractor() { if (integral) fd_integral_destroy(integral); }
void DirectImageFeatureExtractor::addImageFilter(shared_ptr<ImageFilter> filter) {
    imageFilter->add(filter);
    const auto& f = imageFilter->getFilters();
    integralChain = (f.size() == 1 && dynamic_cast<IntegralImageFilter*>(f[0].get())) ||
                    (f.size() == 2 && dynamic_cast<GrayscaleFilter*>(f[0].get()) && dynamic_cast<IntegralImageFilter*>(f[1].get()));
    version = Version();   // the filtered image belongs to the previous chain
}
void DirectImageFeatureExtractor::update(shared_ptr<VersionedImage> img) {   // DirectImageFeatureExtractor.cpp:35-40
    if (version == img->getVersion()) return;
    const Mat& data = img->getData();
    const bool gray = imageFilter->getFilters().size() == 2;
    if (integralChain && data.depth() == CV_8U && (data.channels() == 1 || (gray && data.channels() == 3))) {
        if (!integral) check(fd_integral_create(context(), &integral));
        Mat src = contiguous(data);
        check(fd_integral_update(integral, src.data, src.cols, src.rows, src.channels(), 0));
        image = Mat();
        imageOnHost = false;
    } else {
        if (integralChain) throw std::invalid_argument("IntegralImageFilter: the image must be of type CV_8UC1");
        imageFilter->applyTo(data, image);
        imageOnHost = true;
    }
    version = img->getVersion();
}
const Mat& DirectImageFeatureExtractor::hostImage() const {
    if (!imageOnHost) {
        int w = 0, h = 0;
        check(fd_integral_size(integral, &w, &h));
        Mat dst(h, w, CV_32SC1);
        check(fd_integral_download(integral, dst.ptr<int32_t>(0)));
        image = dst;
        imageOnHost = true;
    }
    return image;
}
shared_ptr<Patch> DirectImageFeatureExtractor::extract(int x, int y, int width, int height) const {   // DirectImageFeatureExtractor.cpp:42-52
    int cols = image.cols, rows = image.rows;
    if (native()) check(fd_integral_size(integral, &cols, &rows));
    const int patchBeginX = x - width / 2, patchBeginY = y - height / 2;
    const int patchEndX = patchBeginX + width, patchEndY = patchBeginY + height;
    if (width < 1 || height < 1 || patchBeginX < 0 || patchEndX > cols || patchBeginY < 0 || patchEndY > rows) return shared_ptr<Patch>();
    const auto& filters = patchFilter->getFilters();
    const IntegralPatchFilter* first = native() && !filters.empty() ? dynamic_cast<const IntegralPatchFilter*>(filters[0].get()) : nullptr;
    if (first) {
        Mat data;
        if (!first->applyToSample(integral, x, y, width, height, data)) return shared_ptr<Patch>();
        for (size_t i = 1; i < filters.size(); ++i) { Mat tmp; filters[i]->applyTo(data, tmp); data = tmp; }
        return make_shared<Patch>(x, y, width, height, data);
    }
    const Mat data(hostImage(), cv::Rect(patchBeginX, patchBeginY, width, height));
    return make_shared<Patch>(x, y, width, height, patchFilter->applyTo(data));
}
shared_ptr<HaarFeatureFilter> DirectImageFeatureExtractor::getHaarChain() const {
    const auto& f = patchFilter->getFilters();
    return f.size() == 1 ? std::dynamic_pointer_cast<HaarFeatureFilter>(f[0]) : nullptr;
}
bool DirectImageFeatureExtractor::getSurfChain(int& gradientCount, int& cellCount) const {
    const auto& f = patchFilter->getFilters();
    if (f.size() != 3) return false;
    const auto* g = dynamic_cast<const IntegralGradientFilter*>(f[0].get());
    const auto* s = dynamic_cast<const GradientSumFilter*>(f[1].get());
    const auto* u = dynamic_cast<const UnitNormFilter*>(f[2].get());
    if (!g || !s || !u || u->normType != cv::NORM_L2 || g->getRows() != g->getCols() || s->getRows() != s->getCols()) return false;
    gradientCount = g->getRows();
    cellCount = s->getRows();
    return true;
}
bool DirectImageFeatureExtractor::getIntegralHogChain(fd_integral_hog_params& hp) const {
    const auto& f = patchFilter->getFilters();
    if (f.size() != 3) return false;
    const auto* g = dynamic_cast<const IntegralGradientFilter*>(f[0].get());
    const auto* b = dynamic_cast<const GradientBinningFilter*>(f[1].get());
    const auto* h = dynamic_cast<const HistogramFilter*>(f[2].get());
    if (!g || !b || !h) return false;
    std::memset(&hp, 0, sizeof(hp));
    hp.grad_rows = g->getRows(); hp.grad_cols = g->getCols();
    hp.bins = (int32_t)b->bins; hp.signed_gradients = b->signedGradients; hp.interpolate_bins = b->interpolate;
    if (auto* e = dynamic_cast<const ExtendedHogFilter*>(h)) {
        hp.kind = FD_SAMPLES_EHOG;
        hp.ehog = fd_ehog_patch_params{hp.grad_cols, hp.grad_rows, e->binCount, e->cellWidth, e->cellHeight, e->interpolate, e->signedAndUnsigned, e->alpha};
    } else {
        hp.kind = FD_SAMPLES_HIST;
        hp.hist = hist_params_of(*h, hp.grad_cols, hp.grad_rows, 1, 1);
    }
    return fd_integral_hog_feature_length(&hp) > 0;   // anything the fused call refuses stays on the per-Mat composition
}

namespace filtering {
FhogFilter::FhogFilter(int cellSize, int unsignedBinCount, bool interpolateBins, bool interpolateCells, float alpha)
    : cellSize(cellSize), unsignedBinCount(unsignedBinCount), interpolateBins(interpolateBins), interpolateCells(interpolateCells), alpha(alpha) {
    if (unsignedBinCount < 1) throw std::invalid_argument("FhogFilter: unsignedBinCount must be bigger than zero, but was: " + std::to_string(unsignedBinCount));
    if (alpha <= 0) throw std::invalid_argument("FhogAggregationFilter: alpha must be bigger than zero, but was: " + std::to_string(alpha));
}
Mat FhogFilter::applyTo(const Mat& image, Mat& descriptors) const {
    if (image.type() != CV_8UC1 && image.type() != CV_8UC3)
        throw std::invalid_argument("FhogFilter: the image type must be CV_8UC1 or CV_8UC3, but was " + std::to_string(image.type()));
    Mat src = image.isContinuous() ? image : image.clone();
    fd_fhog_params fp = {cellSize, unsignedBinCount, interpolateBins, interpolateCells, alpha};
    const int rows = src.rows / cellSize, cols = src.cols / cellSize, D = 3 * unsignedBinCount + 4;
    descriptors.create(rows, cols * D, CV_32FC1);   // the compat Mat has no CV_32FC(n) with n > 4: channels are interleaved in the row
    if (rows > 0 && cols > 0)
        check(fd_fhog_image_channels(context(), src.ptr<uchar>(0), src.cols, src.rows, src.channels(), &fp, descriptors.ptr<float>(0)));
    return descriptors;
}

FpdwFeaturesFilter::FpdwFeaturesFilter(bool fastGradient, bool interpolate, int normalizationRadius, double normalizationConstant)
    : fastGradient(fastGradient), interpolate(interpolate), normalizationRadius(normalizationRadius), normalizationConstant(normalizationConstant) {
    if (normalizationRadius < 0)
        throw std::invalid_argument("TriangularConvolutionFilter: size must be greater than zero, but was " + std::to_string(2 * normalizationRadius + 1));
    if (normalizationConstant <= 0)
        throw std::invalid_argument("GradientMagnitudeFilter: normalizationConstant must be bigger than zero, but was " + std::to_string(normalizationConstant));
}
Mat FpdwFeaturesFilter::applyTo(const Mat& image, Mat& descriptors) const {
    const fd_fpdw_params fp = {1, fastGradient, interpolate, normalizationRadius, (float)normalizationConstant};
    return fpdw_apply(image, fp, false, descriptors);
}
AggregationFilter::AggregationFilter(int cellSize, bool interpolate, bool normalize) : cellSize(cellSize) {
    if (cellSize < 1) throw std::invalid_argument("AggregationFilter: cellSize must be bigger than zero, but was " + std::to_string(cellSize));
    if (!interpolate) throw std::logic_error("AggregationFilter: box aggregation (interpolate = false) is not available on this backend");
    if (normalize) throw std::logic_error("AggregationFilter: normalize = true is not available on this backend");
}
Mat AggregationFilter::applyTo(const Mat&, Mat&) const {
    throw std::logic_error("AggregationFilter: on this backend the filter runs fused behind a filtering::FpdwFeaturesFilter "
                           "(ChainedFilter(FpdwFeaturesFilter, AggregationFilter)), not on an image of its own");
}
}  // namespace filtering

// ---- DirectPyramidFeatureExtractor ----------------------------------------------------------------
DirectPyramidFeatureExtractor::DirectPyramidFeatureExtractor(shared_ptr<ImagePyramid> pyramid, int width, int height)
    : pyramid(pyramid), patchWidth(width), patchHeight(height) {}
void DirectPyramidFeatureExtractor::addPatchFilter(shared_ptr<ImageFilter> filter) {
    if (ehog) throw std::logic_error("DirectPyramidFeatureExtractor: ExtendedHogFilter is available as the only patch filter (the ehog feature type); nothing may follow it");
    if (auto rf = std::dynamic_pointer_cast<ReshapingFilter>(filter)) {   // the fused kernels work on flat vectors: nothing to do
        if (rf->rows != 1 || rf->channels > 1) throw std::logic_error("DirectPyramidFeatureExtractor: ReshapingFilter(1) (row vectors) is available in a fused chain");
        reshaping = rf;
        chain->add(filter);
        return;
    }
    if (auto h = std::dynamic_pointer_cast<HistEq64Filter>(filter)) histeq = h;
    else if (auto wf = std::dynamic_pointer_cast<WhiteningFilter>(filter)) {
        if (whiStage != 0) throw std::logic_error("DirectPyramidFeatureExtractor: WhiteningFilter must be the first filter of the whi chain");
        whitening = wf; whiStage = 1;
    } else if (auto ef = std::dynamic_pointer_cast<HistogramEqualizationFilter>(filter)) {
        if (whiStage != 0 && whiStage != 1) throw std::logic_error("DirectPyramidFeatureExtractor: unsupported patch filter order");
        equalization = ef;
        if (whiStage == 1) whiStage = 2;
    } else if (auto cf = std::dynamic_pointer_cast<ConversionFilter>(filter)) {
        if (whiStage == 0 && !hist && cf->type == CV_32F) {   // u8 feature space -> f32 (input of an RVM / f32 SVM)
            conversion = cf;
            chain->add(filter);
            return;
        }
        if (whiStage != 2 || cf->type != CV_32F || cf->alpha != 1.0 / 127.5 || cf->beta != -1.0)
            throw std::logic_error("DirectPyramidFeatureExtractor: ConversionFilter is available as ConversionFilter(CV_32F, alpha, beta) after a u8 "
                                   "feature space, or as ConversionFilter(CV_32F, 1.0/127.5, -1.0) inside the whi chain");
        whiStage = 3;
    } else if (auto uf = std::dynamic_pointer_cast<UnitNormFilter>(filter)) {
        if (whiStage != 3 || uf->normType != cv::NORM_L2)
            throw std::logic_error("DirectPyramidFeatureExtractor: UnitNormFilter is available as UnitNormFilter(cv::NORM_L2) at the end of the whi chain only");
        whiStage = 4;
    } else if (auto xf = std::dynamic_pointer_cast<ExtendedHogFilter>(filter)) {
        if (hasPatchFilters()) throw std::logic_error("DirectPyramidFeatureExtractor: ExtendedHogFilter is available as the only patch filter (the ehog feature type)");
        ehog = xf;   // extract(x, y, width, height) per Mat, extract(samples) fused; no strided scan
    } else if (auto hf = std::dynamic_pointer_cast<HistogramFilter>(filter)) {
        hist = hf;
        auto g = std::dynamic_pointer_cast<HogFilter>(filter);
        // the tuned k_hog_tile path covers the square, non-interpolating HogFilter; everything else runs k_hist_features
        hog = (g && !g->interpolate && g->cellWidth == g->cellHeight && g->blockWidth == g->blockHeight) ? g : nullptr;
    } else throw std::logic_error("DirectPyramidFeatureExtractor: unsupported patch filter (HistEq64Filter and the HistogramFilter family are available)");
    chain->add(filter);
}
vector<cv::Size> DirectPyramidFeatureExtractor::getPatchSizes() const {
    vector<cv::Size> sizes;
    for (const auto& sc : pyramid->getLayerScales())
        sizes.push_back(cv::Size(cv::cvRound(patchWidth / sc.second), cv::cvRound(patchHeight / sc.second)));
    return sizes;
}
int DirectPyramidFeatureExtractor::getLayerIndex(int width, int) const {
    double scaleFactor = (double)patchWidth / (double)width;
    int idx = (int)std::round(std::log(scaleFactor) / std::log(pyramid->getIncrementalScaleFactor()));
    return pyramid->getLayer(idx) ? idx : -1;
}
shared_ptr<Patch> DirectPyramidFeatureExtractor::extractFromLayer(const ImagePyramidLayer& layer, cv::Rect b) const {
    const Mat& image = layer.getScaledImage();
    if (b.x < 0 || b.y < 0 || b.x + b.width > image.cols || b.y + b.height > image.rows) return shared_ptr<Patch>();
    int ow = layer.getOriginal(b.width), oh = layer.getOriginal(b.height);
    int ox = layer.getOriginal(b.x) + ow / 2, oy = layer.getOriginal(b.y) + oh / 2;
    Mat data = Mat(image, b).clone();
    if (hasPatchFilters()) data = chain->applyTo(data);   // per Mat, in the order the filters were added (DirectPyramidFeatureExtractor.cpp:75-123)
    return make_shared<Patch>(ox, oy, ow, oh, data);
}
shared_ptr<Patch> DirectPyramidFeatureExtractor::extract(int x, int y, int width, int height) const {
    int idx = getLayerIndex(width, height);
    auto layer = idx < 0 ? shared_ptr<ImagePyramidLayer>() : pyramid->getLayer(idx);
    if (!layer) return shared_ptr<Patch>();
    return extractFromLayer(*layer, cv::Rect(layer->getScaled(x - width / 2), layer->getScaled(y - height / 2), patchWidth, patchHeight));
}
bool DirectPyramidFeatureExtractor::getSampledChain(int& kind, fd_hist_params& hp, fd_ehog_patch_params& ep) const {
    if (histeq || whitening || equalization || conversion || pyramid->getSourcePyramid()) return false;
    const int layerKind = pyramid->getLayerFilterKind();
    if (layerKind == FD_LAYER_NONE || (ehog && layerKind != FD_LAYER_GRADBIN)) return false;
    if (ehog) {
        kind = FD_SAMPLES_EHOG;
        ep = fd_ehog_patch_params{patchWidth, patchHeight, ehog->binCount, ehog->cellWidth, ehog->cellHeight, ehog->interpolate, ehog->signedAndUnsigned, ehog->alpha};
        return true;
    }
    if (!hist) return false;
    kind = FD_SAMPLES_HIST;
    hp = hist_params_of(*hist, patchWidth, patchHeight, 1, 1);
    return true;
}
bool DirectPyramidFeatureExtractor::getSampledPatchChain(fd_patch_samples_params& pp) const {
    if (pyramid->getSourcePyramid() || pyramid->getLayerFilterKind() != FD_LAYER_NONE || hist || ehog || reshaping) return false;
    const auto& filters = chain->getFilters();
    pp = fd_patch_samples_params{patchWidth, patchHeight, FD_FEATURE_GRAY, 1.f, 0.f, 1.f, 0.390625f};
    if (whiStage == 4 && filters.size() == 4 && !histeq && !conversion) {
        pp.feature_space = FD_FEATURE_WHI;
        pp.whi_alpha = whitening->alpha; pp.whi_cutoff = whitening->cutoffFrequency;
        return fd_patch_feature_length(&pp) > 0;
    }
    if (whiStage != 0 || !conversion || filters.empty() || filters.back() != conversion) return false;
    if (filters.size() == 2 && histeq && !equalization && filters[0] == histeq) pp.feature_space = FD_FEATURE_HQ64;
    else if (filters.size() == 2 && equalization && !histeq && filters[0] == equalization) pp.feature_space = FD_FEATURE_HISTEQ;
    else if (filters.size() != 1 || histeq || equalization) return false;
    pp.conv_scale = (float)conversion->alpha; pp.conv_shift = (float)conversion->beta;   // cv::Mat::convertTo works in float
    return fd_patch_feature_length(&pp) > 0;
}
vector<shared_ptr<Patch>> DirectPyramidFeatureExtractor::extract(const vector<cv::Rect>& samples) const {
    vector<shared_ptr<Patch>> patches(samples.size());
    const SampledChain chain = sampledChainOf(this);
    if (!chain.onPyramid()) {   // the per-sample path
        for (size_t i = 0; i < samples.size(); ++i)
            patches[i] = extract(samples[i].x + samples[i].width / 2, samples[i].y + samples[i].height / 2, samples[i].width, samples[i].height);
        return patches;
    }
    const int n = (int)samples.size();
    if (n == 0) return patches;
    // the centre form the rule works on: x - width / 2 is the rectangle's x again for every width
    vector<int32_t> xywh((size_t)4 * n), windows((size_t)4 * n);
    for (int i = 0; i < n; ++i) {
        xywh[4 * i] = samples[i].x + samples[i].width / 2; xywh[4 * i + 1] = samples[i].y + samples[i].height / 2;
        xywh[4 * i + 2] = samples[i].width; xywh[4 * i + 3] = samples[i].height;
    }
    const vector<Mat> data = chain.extract(xywh);
    check(fd_pyramid_sample_windows(pyramid->native(), patchWidth, patchHeight, n, xywh.data(), windows.data()));
    for (int i = 0; i < n; ++i) {
        if (data[i].empty()) continue;
        int index, lw, lh, ch; double scale;
        fd_pyramid_layer_info(pyramid->native(), windows[4 * i], &index, &scale, &lw, &lh, &ch);
        // extractFromLayer's geometry (ImagePyramidLayer::getOriginal)
        const int ow = cv::cvRound(patchWidth / scale), oh = cv::cvRound(patchHeight / scale);
        const int ox = cv::cvRound(windows[4 * i + 1] / scale) + ow / 2, oy = cv::cvRound(windows[4 * i + 2] / scale) + oh / 2;
        patches[i] = make_shared<Patch>(ox, oy, ow, oh, data[i]);
    }
    return patches;
}

// ---- SampledChain ---------------------------------------------------------------------------------
SampledChain sampledChainOf(const FeatureExtractor* extractor, bool mapsApplied) {
    using Kind = SampledChain::Kind;
    SampledChain c(extractor);
    c.pyramid = dynamic_cast<const DirectPyramidFeatureExtractor*>(c.wrappers.inner());
    c.image = dynamic_cast<const DirectImageFeatureExtractor*>(c.wrappers.inner());
    int kind = 0, gradientCount = 0, cellCount = 0;
    if (c.pyramid && (mapsApplied || !c.wrappers.wrapped())) {   // the extractor itself: a wrapper's map moves the sample off the layer rule
        if (c.pyramid->getSampledChain(kind, c.hist, c.ehog)) c.kind = kind == FD_SAMPLES_EHOG ? Kind::Ehog : Kind::Hist;
        else if (c.pyramid->getSampledPatchChain(c.patch)) c.kind = Kind::Patch;
    } else if (c.image) {
        if ((c.haar = c.image->getHaarChain())) c.kind = Kind::Haar;
        else if (c.image->getSurfChain(gradientCount, cellCount) && gradientCount > 0) { c.surf = fd_surf_params{gradientCount, cellCount}; c.kind = Kind::Surf; }
        else if (c.image->getIntegralHogChain(c.ihog)) c.kind = Kind::IntegralHog;
    }
    return c;
}
bool SampledChain::ready() const { return onPyramid() || (kind != Kind::None && image->native()); }
int SampledChain::featureLength(int channels) const {
    return kind == Kind::Hist ? fd_hist_feature_length(&hist, channels) : kind == Kind::Ehog ? fd_ehog_feature_length(&ehog, channels) :
           kind == Kind::Patch ? fd_patch_feature_length(&patch) : kind == Kind::IntegralHog ? fd_integral_hog_feature_length(&ihog) : -1;
}
int SampledChain::matRows() const {
    // ExtendedHogFilter::applyTo gives cell rows x (cell columns * channels), the histogram filters 1 x F; a gray patch keeps its shape
    const fd_ehog_patch_params* e = kind == Kind::Ehog ? &ehog : (kind == Kind::IntegralHog && ihog.kind == FD_SAMPLES_EHOG ? &ihog.ehog : nullptr);
    if (e) return cv::cvRound(static_cast<double>(e->patch_h) / static_cast<double>(e->cell_h > 0 ? e->cell_h : e->cell_w));
    return kind == Kind::Patch ? patch.patch_h : 1;
}
int SampledChain::cellChannels() const {
    const shared_ptr<ExtendedHogFilter> f = pyramid ? pyramid->getExtendedHogFilter() : (image ? image->getExtendedHogFilter() : nullptr);
    return f ? f->binCount + (f->signedAndUnsigned ? f->binCount / 2 : 0) + 4 : 1;
}
vector<int32_t> SampledChain::mapped(const vector<int32_t>& xywh) const {
    vector<int32_t> m = onPyramid() ? vector<int32_t>() : xywh;   // the pyramid kinds take the samples as they are
    wrappers.map(m.data(), m.size() / 4);
    return m;
}
vector<Mat> SampledChain::extract(const vector<int32_t>& xywh) const {
    const int n = (int)(xywh.size() / 4);
    vector<Mat> data((size_t)n);
    if (n == 0) return data;
    fd_pyramid* native = onPyramid() ? pyramid->getPyramid()->native() : nullptr;
    int index, lw, lh, ch = 1; double scale;
    if (native && fd_pyramid_layer_count(native) > 0) fd_pyramid_layer_info(native, 0, &index, &scale, &lw, &lh, &ch);
    const int F = featureLength(ch);
    if (native && F < 0) throw std::invalid_argument("DirectPyramidFeatureExtractor: invalid histogram filter parameters for this patch size");
    if (!native && (kind != Kind::IntegralHog || !ready() || F <= 0))
        throw std::logic_error("DirectImageFeatureExtractor: extractIntegralHog needs an updated integral image and an integral HOG chain");
    const vector<int32_t> m = mapped(xywh);
    vector<float> rows((size_t)n * F);
    vector<uint8_t> valid((size_t)n);
    if (kind == Kind::Patch) check(fd_patch_extract_samples(context(), native, &patch, n, xywh.data(), valid.data(), rows.data()));
    else if (kind == Kind::Ehog) check(fd_ehog_extract_samples(context(), native, &ehog, n, xywh.data(), valid.data(), rows.data()));
    else if (kind == Kind::Hist) check(fd_hist_extract_samples(context(), native, &hist, n, xywh.data(), valid.data(), rows.data()));
    else check(fd_integral_extract_hog(context(), image->native(), &ihog, n, m.data(), rows.data(), valid.data()));
    const int r = matRows();
    for (int i = 0; i < n; ++i) {
        if (!valid[i]) continue;
        data[i] = Mat(r, F / r, CV_32FC1);
        std::memcpy(data[i].ptr<float>(0), rows.data() + (size_t)i * F, sizeof(float) * (size_t)F);
    }
    return data;
}
SampledChain::DeviceCall SampledChain::deviceCall() const {
    DeviceCall call;
    call.onPyramid = onPyramid();
    if (call.onPyramid) {
        call.pyramid = pyramid->getPyramid()->native();
        call.kind = kind == Kind::Patch ? (int)FD_SAMPLES_PATCH : (kind == Kind::Ehog ? (int)FD_SAMPLES_EHOG : (int)FD_SAMPLES_HIST);
        call.block = kind == Kind::Patch ? (const void*)&patch : (kind == Kind::Ehog ? (const void*)&ehog : (const void*)&hist);
    } else if (kind != Kind::None) {
        call.integral = image->native();
        call.kind = kind == Kind::Haar ? (int)FD_INTEGRAL_HAAR : (kind == Kind::IntegralHog ? (int)FD_INTEGRAL_HOG : (int)FD_INTEGRAL_SURF);
        call.block = kind == Kind::Haar ? nullptr : (kind == Kind::IntegralHog ? (const void*)&ihog : (const void*)&surf);
        if (haar) call.haar = haar->params();
    }
    return call;
}
void SampledChain::svmEvaluate(const fd_svm* svm, const vector<int32_t>& xywh, uint8_t* target, double* weight) const {
    const int n = (int)(xywh.size() / 4);
    const DeviceCall call = deviceCall();
    if (kind == Kind::Patch)
        check(fd_patch_svm_evaluate_samples(context(), call.pyramid, &patch, svm, n, xywh.data(), target, weight, nullptr));
    else if (call.onPyramid)
        check(fd_hist_svm_evaluate_samples(context(), call.pyramid, call.kind, call.params(), svm, n, xywh.data(), target, weight));
    else   // the wrappers are integer maps of the sample, applied here
        check(fd_integral_svm_evaluate_samples(context(), call.integral, call.kind, call.params(), svm, n, mapped(xywh).data(), target, weight));
}
bool SampledChain::hasWindow(int x, int y, int width, int height) const {
    int32_t s[4] = {x, y, width, height};
    if (onPyramid()) {   // the extractor's rule
        int32_t w[4];
        check(fd_pyramid_sample_windows(pyramid->getPyramid()->native(), pyramid->getPatchWidth(), pyramid->getPatchHeight(), 1, s, w));
        return w[3] != 0;
    }
    if (kind != Kind::IntegralHog) throw std::logic_error("SampledChain: hasWindow serves the pyramid kinds and integral HOG");
    wrappers.map(s);   // the rule of the kernels on the mapped sample
    int iw = 0, ih = 0;
    check(fd_integral_size(image->native(), &iw, &ih));
    uint8_t valid = 0;
    if (fd_integral_gradient_samples_valid(iw - 1, ih - 1, ihog.grad_rows, ihog.grad_cols, 1, s, &valid) != FD_OK)
        throw std::invalid_argument("PositionDependentMeasurementModel: the integral image has no size");
    return valid != 0;
}
shared_ptr<Patch> DirectPyramidFeatureExtractor::extract(int layerIndex, int x, int y) const {
    auto layer = pyramid->getLayer(layerIndex);
    if (!layer) return shared_ptr<Patch>();
    return extractFromLayer(*layer, cv::Rect(x - patchWidth / 2, y - patchHeight / 2, patchWidth, patchHeight));
}
vector<shared_ptr<Patch>> DirectPyramidFeatureExtractor::extract(int stepX, int stepY, cv::Rect roi, int firstLayer, int lastLayer,
                                                                 int stepLayer) const {
    // DirectPyramidFeatureExtractor.cpp:75-123: the layer sub-range, the layer step and the region of interest apply to the window
    // enumeration of every chain (fd_pyramid_select); a pyramid built on another pyramid adds its scale range
    auto selection = pyramid->select(firstLayer, lastLayer, stepLayer, &roi);
    int64_t n = 0;
    check(fd_pyramid_window_count(pyramid->native(), patchWidth, patchHeight, stepX, stepY, nullptr, &n));
    vector<int32_t> wins((size_t)n * 7);
    if (n) check(fd_pyramid_windows(pyramid->native(), patchWidth, patchHeight, stepX, stepY, nullptr, wins.data(), n, &n));
    vector<shared_ptr<Patch>> patches;
    patches.reserve((size_t)n);
    if (hog) {
        fd_hog_params hp = {patchWidth, patchHeight, stepX, stepY, hog->binCount, hog->cellWidth, hog->blockWidth, hog->signedAndUnsigned};
        const int F = fd_hog_feature_length(&hp);
        Mat all((int)n, F, CV_32FC1);
        int64_t cnt = 0;
        if (n) check(fd_extract_hog(context(), pyramid->native(), &hp, all.ptr<float>(0), n, &cnt));
        for (int64_t i = 0; i < n; ++i) {
            const int32_t* w = &wins[7 * i];
            patches.push_back(make_shared<Patch>(w[3], w[4], w[5], w[6], Mat(all, cv::Rect(0, (int)i, F, 1))));
        }
        return patches;
    }
    if (whiStage != 0 && whiStage != 4) throw std::logic_error("DirectPyramidFeatureExtractor: incomplete whi filter chain");
    if (ehog) throw std::logic_error("DirectPyramidFeatureExtractor: ExtendedHogFilter is available for sampled windows and per patch, not for a strided scan");
    if (whiStage == 4) {
        fd_whi_params wp = {patchWidth, patchHeight, stepX, stepY, whitening->alpha, whitening->cutoffFrequency};
        const int F = patchWidth * patchHeight;
        Mat all((int)std::max<int64_t>(n, 1), F, CV_32FC1);
        int64_t cnt = 0;
        if (n) check(fd_extract_whi(context(), pyramid->native(), &wp, all.ptr<float>(0), n, &cnt));
        for (int64_t i = 0; i < n; ++i) {
            const int32_t* w = &wins[7 * i];
            Mat data(patchHeight, patchWidth, CV_32FC1);
            std::memcpy(data.data, all.ptr<float>((int)i), sizeof(float) * (size_t)F);
            patches.push_back(make_shared<Patch>(w[3], w[4], w[5], w[6], data));
        }
        return patches;
    }
    if (hist) {
        fd_hist_params hp = hist_params_of(*hist, patchWidth, patchHeight, stepX, stepY);
        int index, lw, lh, ch = 1; double scale;
        if (fd_pyramid_layer_count(pyramid->native()) > 0) fd_pyramid_layer_info(pyramid->native(), 0, &index, &scale, &lw, &lh, &ch);
        const int F = fd_hist_feature_length(&hp, ch);
        if (F < 0) throw std::invalid_argument("DirectPyramidFeatureExtractor: invalid histogram filter parameters for this patch size");
        Mat all((int)std::max<int64_t>(n, 1), F, CV_32FC1);
        int64_t cnt = 0;
        if (n) check(fd_extract_hist(context(), pyramid->native(), &hp, all.ptr<float>(0), n, &cnt));
        for (int64_t i = 0; i < n; ++i) {
            const int32_t* w = &wins[7 * i];
            patches.push_back(make_shared<Patch>(w[3], w[4], w[5], w[6], Mat(all, cv::Rect(0, (int)i, F, 1))));
        }
        return patches;
    }
    const auto& layers = (pyramid->getSourcePyramid() ? pyramid->getSourcePyramid() : pyramid)->getLayers();   // w[0] = position in the underlying pyramid
    const int d = patchWidth * patchHeight;
    Mat raw((int)std::max<int64_t>(n, 1), d, CV_8UC1), eq;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* w = &wins[7 * i];
        const Mat& img = layers[w[0]]->getScaledImage();
        for (int y = 0; y < patchHeight; ++y) std::memcpy(raw.ptr<uchar>((int)i) + y * patchWidth, img.ptr<uchar>(w[2] + y) + w[1], patchWidth);
    }
    if (histeq && n) {
        eq.create((int)n, d, CV_8UC1);
        check(fd_histeq64_batch(context(), raw.data, n, patchWidth, patchHeight, eq.data));
    } else if (equalization && n) {   // feature space "histeq" (ffpDetectApp.cpp:446-448)
        eq.create((int)n, d, CV_8UC1);
        check(fd_equalize_hist_batch(context(), raw.data, n, patchWidth, patchHeight, eq.data));
    } else {
        eq = raw;
    }
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* w = &wins[7 * i];
        if (conversion) {   // cv::Mat::convertTo(CV_32F, alpha, beta): float(u8) * float(alpha) + float(beta)
            Mat data(patchHeight, patchWidth, CV_32FC1);
            const uchar* srcp = eq.ptr<uchar>((int)i);
            float* dstp = data.ptr<float>(0);
            const float a = (float)conversion->alpha, b = (float)conversion->beta;
            for (int k = 0; k < d; ++k) dstp[k] = (float)srcp[k] * a + b;
            patches.push_back(make_shared<Patch>(w[3], w[4], w[5], w[6], data));
            continue;
        }
        Mat data(patchHeight, patchWidth, CV_8UC1);
        std::memcpy(data.data, eq.ptr<uchar>((int)i), d);
        patches.push_back(make_shared<Patch>(w[3], w[4], w[5], w[6], data));
    }
    return patches;
}

// ---- FilteringPyramidFeatureExtractor (FilteringPyramidFeatureExtractor.hpp:20-90) ------------------------------------------
FilteringPyramidFeatureExtractor::FilteringPyramidFeatureExtractor(shared_ptr<PyramidFeatureExtractor> extractor)
    : extractor(extractor), patchFilter(make_shared<ChainedFilter>()) {
    if (!extractor) throw std::invalid_argument("FilteringPyramidFeatureExtractor: the underlying extractor must not be null");
    auto direct = std::dynamic_pointer_cast<DirectPyramidFeatureExtractor>(extractor);
    if (direct && !direct->hasPatchFilters())
        fused = make_shared<DirectPyramidFeatureExtractor>(direct->getPyramid(), direct->getPatchWidth(), direct->getPatchHeight());
}
void FilteringPyramidFeatureExtractor::addPatchFilter(shared_ptr<ImageFilter> filter) {
    patchFilter->add(filter);
    if (fused) {
        try { fused->addPatchFilter(filter); }
        catch (const std::logic_error&) { fused.reset(); }   // not a chain the kernels fuse: per-Mat composition from now on
    }
}
shared_ptr<Patch> FilteringPyramidFeatureExtractor::extract(int x, int y, int width, int height) const {
    shared_ptr<Patch> patch = extractor->extract(x, y, width, height);
    if (patch) patchFilter->applyInPlace(patch->getData());
    return patch;
}
vector<shared_ptr<Patch>> FilteringPyramidFeatureExtractor::extract(int stepX, int stepY, cv::Rect roi, int firstLayer, int lastLayer, int stepLayer) const {
    if (fused) return fused->extract(stepX, stepY, roi, firstLayer, lastLayer, stepLayer);   // batched kernels, same values
    vector<shared_ptr<Patch>> patches = extractor->extract(stepX, stepY, roi, firstLayer, lastLayer, stepLayer);
    for (shared_ptr<Patch>& patch : patches) patchFilter->applyInPlace(patch->getData());
    return patches;
}
shared_ptr<Patch> FilteringPyramidFeatureExtractor::extract(int layer, int x, int y) const {
    shared_ptr<Patch> patch = extractor->extract(layer, x, y);
    if (patch) patchFilter->applyInPlace(patch->getData());
    return patch;
}


// ---- ExtendedHogFeatureExtractor, CellBasedPyramidFeatureExtractor on one fd_ehog_tracker ---------------------------------------------
static shared_ptr<VersionedImage> ehog_update(fd_ehog_tracker* tracker, const shared_ptr<VersionedImage>& image) {
    Mat src = contiguous(image->getData());
    if (src.depth() != CV_8U || (src.channels() != 1 && src.channels() != 3)) throw std::invalid_argument("GrayscaleFilter: the image must be CV_8UC1 or CV_8UC3");
    check(fd_ehog_tracker_update(context(), tracker, src.ptr<uchar>(0), src.cols, src.rows, src.channels(), 0));
    return image;
}
// the layer ImagePyramid::getLayer(scaleFactor) picks (ImagePyramid.cpp:300-310); false when there is none
static bool ehog_layer_of(fd_ehog_tracker* tracker, double scaleFactor, int octaveLayerCount, fd_ehog_layer& layer) {
    fd_ehog_layer layers[256];
    int n = 0;
    if (fd_ehog_tracker_get_layers(tracker, layers, 256, &n) != FD_OK || n == 0) return false;
    const double power = std::log(scaleFactor) / std::log(std::pow(0.5, 1. / octaveLayerCount));
    const long realIndex = std::lround(power) - layers[0].index;
    if (realIndex < 0 || realIndex >= n) return false;
    layer = layers[realIndex];
    return true;
}
ExtendedHogFeatureExtractor::ExtendedHogFeatureExtractor(shared_ptr<CompleteExtendedHogFilter> ehogFilter, int cols, int rows, int minWidth, int maxWidth,
                                                         int octaveLayerCount)
    : tracker(nullptr), cols(cols), rows(rows), cellSize((int)ehogFilter->getCellSize()), channels((int)ehogFilter->getDescriptorSize()),
      patchWidth((cols + 2) * (int)ehogFilter->getCellSize()), patchHeight((rows + 2) * (int)ehogFilter->getCellSize()), octaveLayerCount(octaveLayerCount),
      widthFactor(static_cast<double>(cols + 2) / cols), heightFactor(static_cast<double>(rows + 2) / rows) {
    if (cols <= 0 || rows <= 0) throw std::invalid_argument("ExtendedHogFeatureExtractor: the amount of columns and rows must be greater than zero");
    fd_ehog_tracker_params prm = {ehogFilter->params(), cols, rows, octaveLayerCount, minWidth, maxWidth};
    check(fd_ehog_tracker_create(context(), &prm, &tracker));
}
ExtendedHogFeatureExtractor::~ExtendedHogFeatureExtractor() { fd_ehog_tracker_destroy(tracker); }
void ExtendedHogFeatureExtractor::update(shared_ptr<VersionedImage> image) { ehog_update(tracker, image); }
shared_ptr<Patch> ExtendedHogFeatureExtractor::extract(int x, int y, int width, int height) const {
    const int32_t xywh[4] = {x, y, width, height};
    uint8_t valid = 0;
    Mat data(rows, cols * channels, CV_32FC1);
    check(fd_ehog_tracker_extract_patches(context(), tracker, 1, xywh, &valid, data.ptr<float>(0), nullptr));
    if (!valid) return shared_ptr<Patch>();
    // the patch's place in the image (:96-104,125-129)
    width = static_cast<int>(std::round(widthFactor * width));
    height = static_cast<int>(std::round(heightFactor * height));
    fd_ehog_layer layer;
    if (!ehog_layer_of(tracker, static_cast<double>(patchWidth) / static_cast<double>(width), octaveLayerCount, layer)) return shared_ptr<Patch>();
    auto scaled = [&](int v) { return cv::cvRound(v * layer.scale); };
    auto original = [&](int v) { return cv::cvRound(v / layer.scale); };
    const int bx = scaled(x - width / 2), by = scaled(y - height / 2);
    const int originalWidth = original(patchWidth - 2 * cellSize), originalHeight = original(patchHeight - 2 * cellSize);
    return make_shared<Patch>(original(bx + cellSize) + originalWidth / 2, original(by + cellSize) + originalHeight / 2, originalWidth, originalHeight, data);
}
CellBasedPyramidFeatureExtractor::CellBasedPyramidFeatureExtractor(shared_ptr<ExtendedHogFeatureExtractor> base) : base(base) {
    if (!base) throw std::invalid_argument("CellBasedPyramidFeatureExtractor: the underlying extractor must not be null");
}
shared_ptr<Patch> CellBasedPyramidFeatureExtractor::extract(int x, int y, int width, int height) const {
    const int32_t xywh[4] = {x, y, width, height};
    uint8_t valid = 0;
    const int cols = base->getCols(), rows = base->getRows(), cellSize = base->getCellSize();
    Mat data(rows, cols * base->getChannels(), CV_32FC1);
    check(fd_ehog_tracker_extract_cells(context(), base->native(), 1, xywh, &valid, data.ptr<float>(0)));
    if (!valid) return shared_ptr<Patch>();
    fd_ehog_layer layer;   // getLayer(width) and getScaled / getOriginal in cells (CellBasedPyramidFeatureExtractor.cpp:58-69)
    if (!ehog_layer_of(base->native(), static_cast<double>(cols * cellSize) / static_cast<double>(width), base->getOctaveLayerCount(), layer))
        return shared_ptr<Patch>();
    auto scaled = [&](int v) { return cv::cvRound(v * layer.scale / cellSize); };
    auto original = [&](int v) { return cv::cvRound(v * cellSize / layer.scale); };
    const int bx = scaled(x - width / 2), by = scaled(y - height / 2);
    const int originalWidth = original(cols), originalHeight = original(rows);
    return make_shared<Patch>(original(bx) + originalWidth / 2, original(by) + originalHeight / 2, originalWidth, originalHeight, data);
}

}  // namespace imageprocessing

// =================================================================================================
namespace classification {

double Kernel::compute(const Mat& lhs, const Mat& rhs) const {
    if (!lhs.isContinuous() || !rhs.isContinuous()) throw std::invalid_argument("Kernel: arguments have to be continuous");
    if (lhs.flags != rhs.flags) throw std::invalid_argument("Kernel: arguments have to have the same type");
    if (lhs.total() * lhs.channels() != rhs.total() * rhs.channels()) throw std::invalid_argument("Kernel: arguments have to have the same length");
    if (lhs.depth() != CV_8U && lhs.depth() != CV_32F) throw std::invalid_argument("Kernel: arguments have to be of depth CV_8U or CV_32F on this backend");
    fd_svm_model m;
    std::memset(&m, 0, sizeof(m));
    m.kernel = abiKernel();
    abiParams(m.p0, m.p1, m.p2);
    m.num_sv = 1;
    m.dim = (int)(rhs.total() * rhs.channels());
    m.dtype = rhs.depth() == CV_8U ? FD_DTYPE_U8 : FD_DTYPE_F32;
    m.support_vectors = rhs.data;
    const float one = 1.f;
    m.coefficients = &one;
    fd_svm* h = nullptr;
    check(fd_svm_create(context(), &m, &h));
    double out = 0;
    int rc = fd_svm_distance_batch(context(), h, lhs.data, 1, &out);
    fd_svm_destroy(h);
    check(rc);
    return out;
}

SvmClassifier::SvmClassifier(shared_ptr<Kernel> kernel) : VectorMachineClassifier(kernel) {}
SvmClassifier::~SvmClassifier() {}
void SvmClassifier::setSvmParameters(vector<Mat> sv, vector<float> coeff, double b) {
    supportVectors = sv;
    coefficients = coeff;
    bias = (float)b;
    device.invalidate();
}
const fd_svm* SvmClassifier::native(double la, double lb) const {
    return device.get(la, lb, [&](fd_svm** handle) {
        if (supportVectors.empty() || supportVectors.size() != coefficients.size())
            throw std::runtime_error("SvmClassifier: no support vectors / coefficient count mismatch");
        const Mat& first = supportVectors.front();
        const int dim = (int)(first.total() * first.channels());
        const int depth = first.depth();
        if (depth != CV_8U && depth != CV_32F) throw std::runtime_error("SvmClassifier: support vectors must be CV_8U or CV_32F on this backend");
        const size_t es = depth == CV_8U ? 1 : 4;
        vector<unsigned char> flat(supportVectors.size() * dim * es);
        for (size_t i = 0; i < supportVectors.size(); ++i) {
            Mat s = contiguous(supportVectors[i]);
            if ((int)(s.total() * s.channels()) != dim || s.depth() != depth) throw std::runtime_error("SvmClassifier: inconsistent support vectors");
            std::memcpy(flat.data() + i * dim * es, s.data, dim * es);
        }
        fd_svm_model m;
        std::memset(&m, 0, sizeof(m));
        m.kernel = kernel->abiKernel();
        kernel->abiParams(m.p0, m.p1, m.p2);
        m.num_sv = (int)supportVectors.size();
        m.dim = dim;
        m.dtype = depth == CV_8U ? FD_DTYPE_U8 : FD_DTYPE_F32;
        m.support_vectors = flat.data();
        m.coefficients = coefficients.data();
        m.bias = bias;
        m.threshold = threshold;
        m.logistic_a = la;
        m.logistic_b = lb;
        check(fd_svm_create(context(), &m, handle));
    });
}
double SvmClassifier::computeHyperplaneDistance(const Mat& featureVector) const {
    if (!supportVectors.empty() && featureVector.depth() != supportVectors[0].depth())   // as the reference's kernels (RbfKernel.hpp: lhs.flags != rhs.flags)
        throw std::invalid_argument("SvmClassifier: feature vector and support vectors have to have the same type");
    Mat x = contiguous(featureVector);
    double out = 0;
    check(fd_svm_distance_batch(context(), distanceModel(), x.data, 1, &out));
    return out;
}
bool SvmClassifier::classify(const Mat& featureVector) const { return classify(computeHyperplaneDistance(featureVector)); }
std::pair<bool, double> SvmClassifier::getConfidence(const Mat& featureVector) const {
    double d = computeHyperplaneDistance(featureVector);
    return classify(d) ? std::make_pair(true, d) : std::make_pair(false, -d);
}
void SvmClassifier::store(std::ofstream& file) {   // SvmClassifier.cpp:68-107
    if (!file) throw std::runtime_error("SvmClassifier: Cannot write into stream");
    file << "Kernel ";
    if (dynamic_cast<LinearKernel*>(kernel.get())) file << "Linear\n";
    else if (auto* k = dynamic_cast<PolynomialKernel*>(kernel.get())) file << "Polynomial " << k->getDegree() << ' ' << k->getConstant() << ' ' << k->getAlpha() << '\n';
    else if (auto* k = dynamic_cast<RbfKernel*>(kernel.get())) file << "RBF " << std::setprecision(17) << k->getGamma() << '\n';
    else if (dynamic_cast<HistogramIntersectionKernel*>(kernel.get())) file << "HIK\n";
    else throw std::runtime_error("SvmClassifier: cannot write kernel parameters (unknown kernel type)");
    file << std::setprecision(9) << "Bias " << getBias() << '\n';
    file << "Coefficients " << coefficients.size() << '\n';
    for (float c : coefficients) file << c << '\n';
    const Mat& v = supportVectors.front();
    file << "SupportVectors " << supportVectors.size() << ' ' << v.rows << ' ' << v.cols << ' ' << v.channels() << ' ' << v.depth() << '\n';
    for (const Mat& s : supportVectors) {
        const size_t n = s.total() * s.channels();
        Mat c = contiguous(s);
        for (size_t i = 0; i < n; ++i) {
            if (v.depth() == CV_8U) file << (int)c.ptr<uchar>(0)[i] << ' ';
            else file << c.ptr<float>(0)[i] << ' ';
        }
        file << '\n';
    }
}
shared_ptr<SvmClassifier> SvmClassifier::load(std::ifstream& file) {   // SvmClassifier.cpp:109-159
    if (!file) throw std::runtime_error("SvmClassifier: Cannot read from stream");
    string tmp, kernelType;
    file >> tmp >> kernelType;
    shared_ptr<Kernel> kernel;
    if (kernelType == "Linear") kernel.reset(new LinearKernel());
    else if (kernelType == "Polynomial") { int degree; double constant, scale; file >> degree >> constant >> scale; kernel.reset(new PolynomialKernel(scale, constant, degree)); }
    else if (kernelType == "RBF") { double gamma; file >> gamma; kernel.reset(new RbfKernel(gamma)); }
    else if (kernelType == "HIK") kernel.reset(new HistogramIntersectionKernel());
    else throw std::runtime_error("SvmClassifier: Invalid kernel type: " + kernelType);
    auto svm = make_shared<SvmClassifier>(kernel);
    file >> tmp >> svm->bias;
    size_t count;
    file >> tmp >> count;
    svm->coefficients.resize(count);
    for (size_t i = 0; i < count; ++i) file >> svm->coefficients[i];
    int rows, cols, channels, depth;
    file >> tmp >> count >> rows >> cols >> channels >> depth;
    if (depth != CV_8U && depth != CV_32F)
        throw std::runtime_error("SvmClassifier: cannot load support vectors of depth other than CV_8U or CV_32F on this backend");
    for (size_t i = 0; i < count; ++i) {
        Mat v(rows, cols, CV_MAKETYPE(depth, channels));
        const size_t n = (size_t)rows * cols * channels;
        for (size_t k = 0; k < n; ++k) {
            if (depth == CV_8U) { int t; file >> t; v.ptr<uchar>(0)[k] = (uchar)t; }
            else file >> v.ptr<float>(0)[k];
        }
        svm->supportVectors.push_back(v);
    }
    if (!file) throw std::runtime_error("SvmClassifier: Invalid classifier file");
    return svm;
}

std::pair<bool, double> ProbabilisticSvmClassifier::getProbability(const Mat& featureVector) const {
    return getProbability(svm->computeHyperplaneDistance(featureVector));
}
std::pair<bool, double> ProbabilisticSvmClassifier::getProbability(double d) const {   // ProbabilisticSvmClassifier.cpp:54-58
    double fABp = logisticA + logisticB * d;
    double p = fABp >= 0 ? std::exp(-fABp) / (1.0 + std::exp(-fABp)) : 1.0 / (1.0 + std::exp(fABp));
    return std::make_pair(svm->classify(d), p);
}
void ProbabilisticSvmClassifier::store(std::ofstream& file) {
    svm->store(file);
    file << std::setprecision(17) << "Logistic " << logisticA << ' ' << logisticB << '\n';
}
shared_ptr<ProbabilisticSvmClassifier> ProbabilisticSvmClassifier::load(std::ifstream& file) {
    auto svm = SvmClassifier::load(file);
    string tmp;
    double a, b;
    file >> tmp >> a >> b;
    return make_shared<ProbabilisticSvmClassifier>(svm, a, b);
}
// SvmClassifier::loadFromText (SvmClassifier.cpp:161-239): the line-based text format of the reference's polynomial SVMs --
//   FullPolynomial <degree> <constant> <scale> / Number of SV : n / Dim of SV : d / B0 : b / alphas[i]=a (n lines) /
//   "Support vectors: " / n lines of d floats -- CV_32F support vectors, PolynomialKernel(scale, constant, degree)
shared_ptr<SvmClassifier> SvmClassifier::loadFromText(const string& classifierFilename) {
    std::ifstream file(classifierFilename.c_str());
    if (!file.is_open()) throw std::runtime_error("SvmClassifier: Invalid classifier file");
    string line;
    if (!std::getline(file, line)) throw std::runtime_error("SvmClassifier: Invalid classifier file");
    shared_ptr<Kernel> kernel;
    {
        std::istringstream lineStream(line);
        string kernelType;
        lineStream >> kernelType;
        if (kernelType != "FullPolynomial") throw std::runtime_error("SvmClassifier: Invalid kernel type: " + kernelType);
        int degree = 0;
        double constant = 0, scale = 0;
        lineStream >> degree >> constant >> scale;
        kernel.reset(new PolynomialKernel(scale, constant, degree));
    }
    auto svm = make_shared<SvmClassifier>(kernel);
    auto next = [&]() { if (!std::getline(file, line)) throw std::runtime_error("SvmClassifier: Invalid classifier file"); };
    int svCount = 0, dimensionCount = 0;
    float bias = 0;
    next();
    if (std::sscanf(line.c_str(), "Number of SV : %d", &svCount) != 1 || svCount < 1) throw std::runtime_error("SvmClassifier: Invalid classifier file");
    next();
    if (std::sscanf(line.c_str(), "Dim of SV : %d", &dimensionCount) != 1 || dimensionCount < 1) throw std::runtime_error("SvmClassifier: Invalid classifier file");
    next();
    if (std::sscanf(line.c_str(), "B0 : %f", &bias) != 1) throw std::runtime_error("SvmClassifier: Invalid classifier file");
    vector<float> coefficients((size_t)svCount, 0.f);
    for (int i = 0; i < svCount; ++i) {
        float alpha;
        int index;
        next();
        if (std::sscanf(line.c_str(), "alphas[%d]=%f", &index, &alpha) != 2 || index < 0 || index >= svCount)
            throw std::runtime_error("SvmClassifier: Invalid classifier file");
        coefficients[(size_t)index] = alpha;
    }
    next();   // "Support vectors: "
    vector<Mat> supportVectors;
    supportVectors.reserve((size_t)svCount);
    for (int i = 0; i < svCount; ++i) {
        Mat vec(1, dimensionCount, CV_32FC1);
        next();
        std::istringstream lineStream(line);
        float* values = vec.ptr<float>(0);
        for (int j = 0; j < dimensionCount; ++j)
            if (!(lineStream >> values[j])) throw std::runtime_error("SvmClassifier: Invalid classifier file");
        supportVectors.push_back(vec);
    }
    svm->setSvmParameters(supportVectors, coefficients, (double)bias);
    return svm;
}

// ProbabilisticSvmClassifier.cpp:80-104.  Non-.mat files are text models: the reference's own text format (loadFromText:
// polynomial SVMs, first token "FullPolynomial") -- or, as the stand-in for the Matlab models the reference loads through libmat
// (RBF / HIK SVMs on u8 patches exist upstream only as .mat files), the stream format of SvmClassifier::store (first token
// "Kernel"; see DESIGN.md section "model formats").
shared_ptr<ProbabilisticSvmClassifier> ProbabilisticSvmClassifier::load(const boost::property_tree::ptree& subtree) {
    string classifierFile = subtree.get<string>("classifierFile");
    if (classifierFile.size() > 4 && classifierFile.substr(classifierFile.size() - 4) == ".mat")
        throw std::runtime_error("ProbabilisticSvmClassifier: Cannot load a Matlab classifier (the reference needs libmat; this backend reads text models)");
    shared_ptr<ProbabilisticSvmClassifier> psvm;
    {
        std::ifstream probe(classifierFile.c_str());
        if (!probe.is_open()) throw std::runtime_error("SvmClassifier: Invalid classifier file");
        string first;
        probe >> first;
        if (first == "Kernel") {
            std::ifstream f(classifierFile.c_str());
            psvm = load(f);
        } else {
            psvm = make_shared<ProbabilisticSvmClassifier>(SvmClassifier::loadFromText(classifierFile));
        }
    }
    double la = subtree.get("logisticA", 0.0), lb = subtree.get("logisticB", 0.0);
    if (la != 0.0 && lb != 0.0) psvm->setLogisticParameters(la, lb);
    psvm->getSvm()->setThreshold(subtree.get("threshold", 0.0f));
    return psvm;
}

// ---- WVM ------------------------------------------------------------------------------------------
WvmClassifier::WvmClassifier() : VectorMachineClassifier(nullptr), limitReliabilityFilter(0.f) {}
WvmClassifier::~WvmClassifier() {}
void WvmClassifier::setModel(const Model& m) {
    model = m;
    bias = m.bias;
    setNumUsedFilters(m.num_used);
    setLimitReliabilityFilter(limitReliabilityFilter);
}
void WvmClassifier::setNumUsedFilters(int var) {   // WvmClassifier.cpp:151-158
    model.num_used = (var > model.num_filters || var == 0) ? model.num_filters : var;
    device.invalidate();
}
void WvmClassifier::setLimitReliabilityFilter(float var) {   // WvmClassifier.cpp:165-181
    limitReliabilityFilter = var;
    hierarchicalThresholds = model.thresholdsFromFile;
    if (var != 0.0f)
        for (float& t : hierarchicalThresholds) t = t + limitReliabilityFilter;
    device.invalidate();
}
const fd_wvm* WvmClassifier::native(double la, double lb) const {
    return device.get(la, lb, [&](fd_wvm** handle) {
        fd_wvm_model m;
        std::memset(&m, 0, sizeof(m));
        m.filter_w = model.filter_w; m.filter_h = model.filter_h; m.num_filters = model.num_filters; m.num_used = model.num_used;
        m.num_per_level = model.num_per_level; m.basis_param = model.basis_param; m.bias = model.bias;
        m.thresholds = hierarchicalThresholds.data(); m.hk_weights = model.hk_weights.data(); m.pp = model.pp.data();
        m.val_off = model.val_off.data(); m.val = model.val.data(); m.rec_off = model.rec_off.data(); m.rects = model.rects.data();
        m.logistic_a = la; m.logistic_b = lb;
        m.num_vals = (int32_t)model.val.size(); m.num_rects = (int32_t)(model.rects.size() / 4);   // a truncated model file is rejected
        // a file with too short offset tables would be read out of bounds before the library sees it
        if ((int)model.val_off.size() != model.num_filters + 1 || model.val_off.back() < 0 || (int)model.rec_off.size() != model.val_off.back() + 1)
            throw std::invalid_argument("WvmClassifier: inconsistent offset tables in the model");
        check(fd_wvm_create(context(), &m, handle));
    });
}
std::pair<int, double> WvmClassifier::computeHyperplaneDistance(const Mat& featureVector) const {
    if (featureVector.depth() != CV_8U || (int)(featureVector.total() * featureVector.channels()) != model.filter_w * model.filter_h)
        throw std::invalid_argument("WvmClassifier: feature vector must be a CV_8U patch of the filter size");
    Mat x = contiguous(featureVector);
    int32_t level = 0;
    float fout = 0;
    check(fd_wvm_eval_batch(context(), distanceModel(), x.data, 1, &level, &fout));
    return std::make_pair((int)level, (double)fout);
}
bool WvmClassifier::classify(std::pair<int, double> lad) const {   // WvmClassifier.cpp:91-98
    return lad.first + 1 == model.num_filters && lad.second >= hierarchicalThresholds[lad.first];
}
bool WvmClassifier::classify(const Mat& featureVector) const { return classify(computeHyperplaneDistance(featureVector)); }
std::pair<bool, double> WvmClassifier::getConfidence(const Mat& featureVector) const {
    auto lad = computeHyperplaneDistance(featureVector);
    return classify(lad) ? std::make_pair(true, lad.second) : std::make_pair(false, -lad.second);
}
// Binary model file "FDWVM1": int32 header {fw, fh, F, used, nper, nval, nrect}, float basis, float bias,
// then thresholds[F] f32, hk[F*F] f32, pp[F] f64, val_off[F+1] i32, val[nval] f64, rec_off[nval+1] i32, rects[4*nrect] u8
shared_ptr<WvmClassifier> WvmClassifier::loadFromFile(const string& filename) {
    std::ifstream f(filename.c_str(), std::ios::binary);
    if (!f.is_open()) throw std::invalid_argument("WvmClassifier: Could not open the provided classifier filename: " + filename);
    char magic[8];
    f.read(magic, 8);
    if (std::memcmp(magic, "FDWVM1\0\0", 8) != 0) throw std::runtime_error("WvmClassifier: not a FDWVM1 model file: " + filename);
    int32_t hdr[7];
    f.read((char*)hdr, sizeof(hdr));
    Model m;
    m.filter_w = hdr[0]; m.filter_h = hdr[1]; m.num_filters = hdr[2]; m.num_used = hdr[3]; m.num_per_level = hdr[4];
    const int nval = hdr[5], nrect = hdr[6], F = m.num_filters;
    if (F < 1 || nval < F || nrect < 0) throw std::runtime_error("WvmClassifier: corrupt model header");
    f.read((char*)&m.basis_param, 4);
    f.read((char*)&m.bias, 4);
    m.thresholdsFromFile.resize(F); m.hk_weights.resize((size_t)F * F); m.pp.resize(F); m.val_off.resize(F + 1); m.val.resize(nval);
    m.rec_off.resize(nval + 1); m.rects.resize((size_t)4 * nrect);
    f.read((char*)m.thresholdsFromFile.data(), 4 * F);
    f.read((char*)m.hk_weights.data(), 4 * (size_t)F * F);
    f.read((char*)m.pp.data(), 8 * F);
    f.read((char*)m.val_off.data(), 4 * (F + 1));
    f.read((char*)m.val.data(), 8 * nval);
    f.read((char*)m.rec_off.data(), 4 * (nval + 1));
    f.read((char*)m.rects.data(), 4 * (size_t)nrect);
    if (!f) throw std::runtime_error("WvmClassifier: truncated model file: " + filename);
    auto wvm = make_shared<WvmClassifier>();
    wvm->setModel(m);
    return wvm;
}

// ---- RVM ------------------------------------------------------------------------------------------
RvmClassifier::RvmClassifier(shared_ptr<Kernel> kernel, bool) : VectorMachineClassifier(kernel) {}
RvmClassifier::~RvmClassifier() {}
void RvmClassifier::setNumFiltersToUse(unsigned int numFilters) {   // RvmClassifier.cpp:119-126
    numFiltersToUse = (numFilters == 0 || numFilters > (unsigned int)model.num_filters) ? (unsigned int)model.num_filters : numFilters;
    device.invalidate();
}
const fd_rvm* RvmClassifier::native(double la, double lb) const {
    return device.get(la, lb, [&](fd_rvm** handle) {
        fd_rvm_model m;
        std::memset(&m, 0, sizeof(m));
        m.kernel = model.kernel; m.p0 = model.p0; m.p1 = model.p1; m.p2 = model.p2;
        m.num_filters = model.num_filters; m.num_used = (int)numFiltersToUse; m.filter_w = model.filter_w; m.filter_h = model.filter_h;
        m.support_vectors = model.support_vectors.data(); m.coefficients = model.coefficients.data(); m.thresholds = model.thresholds.data();
        m.bias = model.bias; m.logistic_a = la; m.logistic_b = lb;
        check(fd_rvm_create(context(), &m, handle));
    });
}
std::pair<int, double> RvmClassifier::computeHyperplaneDistance(const Mat& featureVector) const {
    if (featureVector.depth() != CV_32F || (int)(featureVector.total() * featureVector.channels()) != model.filter_w * model.filter_h)
        throw std::invalid_argument("RbfKernel: arguments have to have the same type");   // Kernel::compute contract (RbfKernel.hpp:35-38)
    Mat x = contiguous(featureVector);
    int32_t level = 0;
    double dist = 0;
    check(fd_rvm_eval_batch(context(), distanceModel(), x.ptr<float>(0), 1, &level, &dist));
    return std::make_pair((int)level, dist);
}
bool RvmClassifier::classify(std::pair<int, double> lad) const {   // RvmClassifier.cpp:66-73
    return lad.first + 1 == (int)numFiltersToUse && lad.second >= model.thresholds[lad.first];
}
bool RvmClassifier::classify(const Mat& featureVector) const { return classify(computeHyperplaneDistance(featureVector)); }
std::pair<bool, double> RvmClassifier::getConfidence(std::pair<int, double> lad) const {
    return classify(lad) ? std::make_pair(true, lad.second) : std::make_pair(false, -lad.second);
}
std::pair<bool, double> RvmClassifier::getConfidence(const Mat& featureVector) const { return getConfidence(computeHyperplaneDistance(featureVector)); }
shared_ptr<RvmClassifier> RvmClassifier::loadFromFile(const string& filename) {
    std::ifstream f(filename.c_str(), std::ios::binary);
    if (!f.is_open()) throw std::invalid_argument("RvmClassifier: Could not open the provided classifier filename: " + filename);
    char magic[8];
    f.read(magic, 8);
    if (std::memcmp(magic, "FDRVM1\0\0", 8) != 0) throw std::runtime_error("RvmClassifier: not a FDRVM1 model file: " + filename);
    int32_t hdr[5];
    double prm[3];
    Model m;
    f.read((char*)hdr, sizeof(hdr));
    f.read((char*)prm, sizeof(prm));
    f.read((char*)&m.bias, 4);
    m.kernel = hdr[0]; m.filter_w = hdr[1]; m.filter_h = hdr[2]; m.num_filters = hdr[3];
    m.p0 = prm[0]; m.p1 = prm[1]; m.p2 = prm[2];
    const int F = m.num_filters, dim = m.filter_w * m.filter_h;
    if (F < 1 || dim < 1 || m.kernel < 0 || m.kernel > 3) throw std::runtime_error("RvmClassifier: corrupt model header");
    m.support_vectors.resize((size_t)F * dim); m.coefficients.resize((size_t)F * (F + 1) / 2); m.thresholds.resize(F);
    f.read((char*)m.support_vectors.data(), 4 * m.support_vectors.size());
    f.read((char*)m.coefficients.data(), 4 * m.coefficients.size());
    f.read((char*)m.thresholds.data(), 4 * (size_t)F);
    if (!f) throw std::runtime_error("RvmClassifier: truncated model file: " + filename);
    shared_ptr<Kernel> kernel;
    if (m.kernel == FD_KERNEL_RBF) kernel = make_shared<RbfKernel>(m.p0);
    else if (m.kernel == FD_KERNEL_POLY) kernel = make_shared<PolynomialKernel>(m.p0, m.p1, (int)m.p2);
    else if (m.kernel == FD_KERNEL_HIK) kernel = make_shared<HistogramIntersectionKernel>();
    else kernel = make_shared<LinearKernel>();
    auto rvm = make_shared<RvmClassifier>(kernel);
    rvm->model = m;
    rvm->bias = m.bias;
    rvm->setNumFiltersToUse((unsigned int)hdr[4]);
    return rvm;
}
shared_ptr<RvmClassifier> RvmClassifier::load(const boost::property_tree::ptree& subtree) {
    string classifierFile = subtree.get<string>("classifierFile");
    if (classifierFile.size() > 4 && classifierFile.substr(classifierFile.size() - 4) == ".mat")
        throw std::runtime_error("RvmClassifier: Cannot load a Matlab classifier (the reference needs libmat; this backend reads the FDRVM1 format)");
    return loadFromFile(classifierFile);
}
std::pair<bool, double> ProbabilisticRvmClassifier::getProbability(const Mat& featureVector) const {
    return getProbability(rvm->computeHyperplaneDistance(featureVector));
}
std::pair<bool, double> ProbabilisticRvmClassifier::getProbability(std::pair<int, double> lad) const {   // ProbabilisticRvmClassifier.cpp:62
    double probability = 1.0f / (1.0f + std::exp(logisticA + logisticB * lad.second));
    return std::make_pair(rvm->classify(lad), probability);
}
shared_ptr<ProbabilisticRvmClassifier> ProbabilisticRvmClassifier::load(const boost::property_tree::ptree& subtree) {
    auto rvm = RvmClassifier::load(subtree);
    auto prvm = make_shared<ProbabilisticRvmClassifier>(rvm, subtree.get("logisticA", 0.00556), subtree.get("logisticB", -2.95));
    if (int nf = subtree.get("numFiltersToUse", 0)) rvm->setNumFiltersToUse((unsigned int)nf);
    return prvm;
}

std::pair<bool, double> ProbabilisticWvmClassifier::getProbability(const Mat& featureVector) const {
    return getProbability(wvm->computeHyperplaneDistance(featureVector));
}
std::pair<bool, double> ProbabilisticWvmClassifier::getProbability(std::pair<int, double> lad) const {   // ProbabilisticWvmClassifier.cpp:52
    double probability = 1.0f / (1.0f + std::exp(logisticA + logisticB * lad.second));
    return std::make_pair(wvm->classify(lad), probability);
}
shared_ptr<ProbabilisticWvmClassifier> ProbabilisticWvmClassifier::load(const boost::property_tree::ptree& subtree) {
    auto wvm = WvmClassifier::loadFromFile(subtree.get<string>("classifierFile"));
    auto pwvm = make_shared<ProbabilisticWvmClassifier>(wvm, subtree.get("logisticA", 0.00556), subtree.get("logisticB", -2.95));
    pwvm->getWvm()->setLimitReliabilityFilter(subtree.get("threshold", 0.0f));
    return pwvm;
}

// ---------------- training ----------------
void ConfidenceBasedExampleManagement::add(const vector<Mat>& newExamples) {   // ConfidenceBasedExampleManagement.cpp:28-68
    typedef std::pair<size_t, double> Scored;
    vector<Scored> existing, incoming;
    for (size_t i = keep; i < examples.size(); ++i) existing.push_back(Scored(i, confidence(examples[i])));
    for (size_t i = 0; i < newExamples.size(); ++i) incoming.push_back(Scored(i, confidence(newExamples[i])));
    std::sort(existing.begin(), existing.end(), [](Scored a, Scored b) { return a.second > b.second; });   // most confident first
    std::sort(incoming.begin(), incoming.end(), [](Scored a, Scored b) { return a.second < b.second; });   // least confident first
    size_t in = 0, ex = 0;
    for (; examples.size() < capacity && in < incoming.size(); ++in) examples.push_back(newExamples[incoming[in].first]);
    for (; ex < existing.size() && in < incoming.size() && incoming[in].second < existing[ex].second; ++ex, ++in)
        examples[existing[ex].first] = newExamples[incoming[in].first];
}

TrainableProbabilisticSvmClassifier::TrainableProbabilisticSvmClassifier(shared_ptr<TrainableSvmClassifier> trainableSvm, int positiveCount,
                                                                         int negativeCount, double highProb, double lowProb)
    : probabilisticSvm(make_shared<ProbabilisticSvmClassifier>(trainableSvm->getSvm())), trainableSvm(trainableSvm),
      positiveCapacity(positiveCount > 0 ? positiveCount : 0), negativeCapacity(negativeCount > 0 ? negativeCount : 0), positiveInsertPosition(0),
      negativeInsertPosition(0), highProb(highProb), lowProb(lowProb), adjustThreshold(false), targetProbability(0.5) {}

void TrainableProbabilisticSvmClassifier::addTestExamples(vector<Mat>& examples, size_t capacity, const vector<Mat>& newExamples, size_t& insertPosition) {
    for (const Mat& example : newExamples) {   // .cpp:69-81: fill up, then overwrite the oldest
        if (examples.size() < capacity) {
            examples.push_back(example);
        } else {
            examples[insertPosition] = example;
            if (++insertPosition == examples.size()) insertPosition = 0;
        }
    }
}
void TrainableProbabilisticSvmClassifier::addTestExamples(const vector<Mat>& newPositiveTestExamples, const vector<Mat>& newNegativeTestExamples) {
    if (positiveCapacity > 0 && negativeCapacity > 0) {   // .cpp:52-55
        addTestExamples(positiveTestExamples, positiveCapacity, newPositiveTestExamples, positiveInsertPosition);
        addTestExamples(negativeTestExamples, negativeCapacity, newNegativeTestExamples, negativeInsertPosition);
    }
}
void TrainableProbabilisticSvmClassifier::updateLogisticParameters() {   // .cpp:57-63
    const std::pair<double, double> ab = computeLogisticParameters(probabilisticSvm->getSvm());
    probabilisticSvm->setLogisticParameters(ab.first, ab.second);
    if (adjustThreshold) probabilisticSvm->getSvm()->setThreshold((std::log(1.0 / targetProbability - 1.0) - ab.first) / ab.second);   // setThreshold takes a float, as the reference's
}
bool TrainableProbabilisticSvmClassifier::retrain(const vector<Mat>& newPositiveExamples, const vector<Mat>& newNegativeExamples,
                                                  const vector<Mat>& newPositiveTestExamples, const vector<Mat>& newNegativeTestExamples) {
    addTestExamples(newPositiveTestExamples, newNegativeTestExamples);
    if (!trainableSvm->retrain(newPositiveExamples, newNegativeExamples)) return false;
    updateLogisticParameters();
    return true;
}
void TrainableProbabilisticSvmClassifier::reset() {
    positiveTestExamples.clear();
    negativeTestExamples.clear();
    trainableSvm->reset();
}
std::pair<double, double> TrainableProbabilisticSvmClassifier::computeLogisticParameters(double meanPosOutput, double meanNegOutput) const {
    const double logisticB = (std::log((1 - lowProb) / lowProb) - std::log((1 - highProb) / highProb)) / (meanNegOutput - meanPosOutput);   // .cpp:93-97
    const double logisticA = std::log((1 - highProb) / highProb) - logisticB * meanPosOutput;
    return std::make_pair(logisticA, logisticB);
}
std::pair<double, double> TrainableProbabilisticSvmClassifier::computeLogisticParameters(shared_ptr<SvmClassifier> svm) const {
    const double meanPosOutput = computeMeanOutput(svm, positiveTestExamples);
    return computeLogisticParameters(meanPosOutput, computeMeanOutput(svm, negativeTestExamples));
}
double TrainableProbabilisticSvmClassifier::computeMeanOutput(shared_ptr<SvmClassifier> svm, const vector<Mat>& examples) const {
    double sum = 0;
    for (const Mat& example : examples) sum += svm->computeHyperplaneDistance(example);
    return sum / examples.size();
}

}  // namespace classification

// =================================================================================================
namespace libsvm {
using classification::ExampleManagement;
using classification::Kernel;
using classification::SvmClassifier;

LibSvmClassifier::LibSvmClassifier(shared_ptr<Kernel> kernel, double cnu, bool oneClass, bool compensateImbalance, bool probabilistic)
    : LibSvmClassifier(make_shared<SvmClassifier>(kernel), cnu, oneClass, compensateImbalance, probabilistic) {}
LibSvmClassifier::LibSvmClassifier(shared_ptr<SvmClassifier> svm, double cnu, bool oneClass, bool compensateImbalance, bool probabilistic)
    : TrainableSvmClassifier(svm), compensateImbalance(compensateImbalance), c(cnu),
      probabilisticSvm(make_shared<classification::ProbabilisticSvmClassifier>(svm)),
      positiveExamples(new classification::UnlimitedExampleManagement()), negativeExamples(new classification::UnlimitedExampleManagement()) {
    if (oneClass) throw std::invalid_argument("LibSvmClassifier: one-class SVMs are not trained on this backend");
    if (probabilistic) throw std::invalid_argument("LibSvmClassifier: probabilistic output (libsvm's sigmoid fit) is not available on this backend");
    if (!svm->getKernel() || svm->getKernel()->abiKernel() != FD_KERNEL_LINEAR)
        throw std::invalid_argument("LibSvmClassifier: only a LinearKernel is trained on this backend");
}
LibSvmClassifier::LibSvmClassifier(shared_ptr<SvmClassifier> svm, double c, bool compensateImbalance, KernelForm, bool probabilistic)
    : TrainableSvmClassifier(svm), compensateImbalance(compensateImbalance), kernelForm(true), probabilistic(probabilistic), c(c),
      probabilisticSvm(make_shared<classification::ProbabilisticSvmClassifier>(svm)),
      positiveExamples(new classification::UnlimitedExampleManagement()), negativeExamples(new classification::UnlimitedExampleManagement()) {
    if (!svm->getKernel()) throw std::invalid_argument("LibSvmClassifier: the SVM has no kernel");
}
LibSvmClassifier::LibSvmClassifier(shared_ptr<SvmClassifier> svm, double nu, OneClassForm)   // LibSvmClassifier.cpp:42-44: no negatives are kept
    : TrainableSvmClassifier(svm), compensateImbalance(false), kernelForm(true), oneClassForm(true), c(nu),
      probabilisticSvm(make_shared<classification::ProbabilisticSvmClassifier>(svm)),
      positiveExamples(new classification::UnlimitedExampleManagement()), negativeExamples(new classification::EmptyExampleManagement()) {
    if (!svm->getKernel()) throw std::invalid_argument("LibSvmClassifier: the SVM has no kernel");
}
void LibSvmClassifier::loadStaticNegatives(const string&, int, double) {
    throw std::invalid_argument("LibSvmClassifier: static negatives are not supported on this backend");
}
bool LibSvmClassifier::addAndGather(const vector<Mat>& newPositiveExamples, const vector<Mat>& newNegativeExamples, vector<float>& x, int& positiveCount,
                                    int& negativeCount, int& dimensions, fd_svm_train_params& params, vector<Mat>* examples) {
    positiveExamples->add(newPositiveExamples);   // LibSvmClassifier.cpp:122-125
    negativeExamples->add(newNegativeExamples);
    if (!positiveExamples->hasRequiredSize() || !negativeExamples->hasRequiredSize()) return false;
    x.clear();
    dimensions = -1;
    ExampleManagement* stores[2] = {positiveExamples.get(), negativeExamples.get()};
    for (ExampleManagement* store : stores)   // createProblem (:164-189): the positives, then the negatives, in the stores' order
        for (auto it = store->iterator(); it->hasNext();) {
            const Mat& example = it->next();
            if (example.depth() != CV_32F) throw std::invalid_argument("LibSvmClassifier: examples have to be of depth CV_32F on this backend");
            if (!example.isContinuous()) throw std::invalid_argument("LibSvmUtils: vector has to be continuous");
            const int dim = (int)(example.total() * example.channels());
            if (dimensions < 0) {
                dimensions = dim;
                rows = example.rows;
                cols = example.cols;
                type = example.type();
            } else if (dim != dimensions) {
                throw std::invalid_argument("LibSvmClassifier: examples have to have the same length");
            }
            x.insert(x.end(), example.ptr<float>(), example.ptr<float>() + dim);
            if (examples) examples->push_back(example);
        }
    positiveCount = (int)positiveExamples->size();
    negativeCount = (int)negativeExamples->size();
    params = fd_svm_train_params{c, 1.0, 1.0, 1e-4, 0, 0};   // createParameters (:56-85)
    if (compensateImbalance) {   // :141-146
        params.weight_pos = (double)negativeCount / (double)positiveCount;
        params.weight_neg = (double)positiveCount / (double)negativeCount;
    }
    return true;
}
void LibSvmClassifier::setTrained(const vector<float>& weights, const fd_svm_train_params& params, const fd_svm_train_info& info) {
    Mat w(rows, cols, type);   // extractSupportVectors: one vector of the examples' shape, coefficient 1, bias rho
    std::memcpy(w.data, weights.data(), sizeof(float) * weights.size());
    svm->setSvmParameters(vector<Mat>{w}, vector<float>{1.f}, info.rho);
    lastParams = params;
    lastInfo = info;
    usable = true;
}
// the kernel form: libsvm's model as it is, the support vectors being the stored example Mats (:144-147)
bool LibSvmClassifier::retrainKernelForm(const vector<Mat>& newPositiveExamples, const vector<Mat>& newNegativeExamples) {
    if (trainingTarget) throw std::invalid_argument("LibSvmClassifier: a tracker handle takes one weight vector (createBinarySvm), not support vectors");
    vector<float> x;
    vector<Mat> examples;
    int positiveCount = 0, negativeCount = 0, dimensions = 0;
    fd_svm_train_params params;
    if (!addAndGather(newPositiveExamples, newNegativeExamples, x, positiveCount, negativeCount, dimensions, params, &examples)) return usable;
    if (examples.size() > (size_t)FD_SVM_LARGE_MAX_N)
        throw std::runtime_error("LibSvmClassifier: " + std::to_string(examples.size()) + " training examples, at most " +
                                 std::to_string(FD_SVM_LARGE_MAX_N) + " are trained on this backend");
    fd_svm_kernel kernel;
    kernel.kernel = svm->getKernel()->abiKernel();
    svm->getKernel()->abiParams(kernel.p0, kernel.p1, kernel.p2);
    vector<int32_t> svIndex(examples.size());
    vector<float> coefficients(examples.size());
    float bias = 0;
    fd_svm_train_info info;
    if (oneClassForm) {   // svm_type ONE_CLASS with nu (createParameters :63-65), from the positives alone
        const fd_svm_one_class_params oneClass = {c, params.eps, 0, 0};
        check(fd_one_class_svm_train(context(), x.data(), positiveCount, dimensions, 0, &kernel, &oneClass, svIndex.data(), coefficients.data(), nullptr,
                                     &bias, nullptr, &info));
    } else {
        if (probabilistic) {   // svm_train runs svm_binary_svc_probability, which draws its shuffle from rand(), before the final training
            const int count = positiveCount + negativeCount;
            vector<int32_t> perm(count);
            for (int i = 0; i < count; ++i) perm[i] = i;
            for (int i = 0; i < count; ++i) std::swap(perm[i], perm[i + std::rand() % (count - i)]);
            check(fd_kernel_svm_cv_sigmoid(context(), x.data(), positiveCount, negativeCount, dimensions, 0, &kernel, &params, perm.data(), &lastProbA,
                                           &lastProbB, nullptr, nullptr));
        }
        check(fd_kernel_svm_train(context(), x.data(), positiveCount, negativeCount, dimensions, 0, &kernel, &params, svIndex.data(),
                                  coefficients.data(), nullptr, &bias, nullptr, &info));
    }
    vector<Mat> supportVectors;
    for (int q = 0; q < info.n_sv; ++q) supportVectors.push_back(examples[svIndex[q]]);
    coefficients.resize(info.n_sv);
    svm->setSvmParameters(supportVectors, coefficients, info.rho);
    // libsvm's A and B are ProbabilisticSvmClassifier's B and A (LibSvmClassifier.cpp:148-152)
    if (probabilistic) probabilisticSvm->setLogisticParameters(lastProbB, lastProbA);
    lastPositiveCount = positiveCount;
    lastNegativeCount = negativeCount;
    lastParams = params;
    lastInfo = info;
    usable = true;
    return usable;
}
bool LibSvmClassifier::retrain(const vector<Mat>& newPositiveExamples, const vector<Mat>& newNegativeExamples) {
    if (newPositiveExamples.empty() && newNegativeExamples.empty()) return usable;   // :119-121
    if (kernelForm) return retrainKernelForm(newPositiveExamples, newNegativeExamples);
    vector<float> x;
    int positiveCount = 0, negativeCount = 0, dimensions = 0;
    fd_svm_train_params params;
    if (!addAndGather(newPositiveExamples, newNegativeExamples, x, positiveCount, negativeCount, dimensions, params)) return usable;
    vector<float> weights(dimensions);
    float bias = 0;
    fd_svm_train_info info;
    if (trainingTarget) {
        if (dimensions != targetDimensions) throw std::invalid_argument("LibSvmClassifier: the examples do not have the length of the tracker's weight vector");
        check(fd_ehog_tracker_train_svm(context(), trainingTarget, x.data(), positiveCount, negativeCount, &params, &info));
        check(fd_ehog_tracker_get_svm(context(), trainingTarget, weights.data(), &bias));
    } else {
        const int64_t count = (int64_t)positiveCount + negativeCount;
        if (count > FD_SVM_LARGE_MAX_N)
            throw std::runtime_error("LibSvmClassifier: " + std::to_string(count) + " training examples, at most " + std::to_string(FD_SVM_LARGE_MAX_N) +
                                     " are trained on this backend (DetectorTrainer: bound the negatives with TrainingParams::maxNegatives)");
        if (count > 1024)   // beyond the tracker-sized trainer: the large entry point, the same model
            check(fd_linear_svm_train_large(context(), x.data(), positiveCount, negativeCount, dimensions, 0, &params, weights.data(), &bias, nullptr, &info));
        else
            check(fd_linear_svm_train(context(), x.data(), positiveCount, negativeCount, dimensions, 0, &params, weights.data(), &bias, nullptr, &info));
    }
    lastPositiveCount = positiveCount;
    lastNegativeCount = negativeCount;
    setTrained(weights, params, info);
    return usable;
}
void LibSvmClassifier::reset() {   // :218-223
    usable = false;
    svm->setSvmParameters(vector<Mat>(), vector<float>(), 0.0);
    positiveExamples->clear();
    negativeExamples->clear();
}

}  // namespace libsvm

// =================================================================================================
namespace liblinear {
using classification::ExampleManagement;

LibLinearClassifier::LibLinearClassifier(double c, bool bias)
    : TrainableSvmClassifier(make_shared<classification::LinearKernel>()), c(c), bias(bias),
      positiveExamples(new classification::UnlimitedExampleManagement()), negativeExamples(new classification::UnlimitedExampleManagement()) {}

vector<float> LibLinearClassifier::parseStaticNegative(const string& line, double scale) {
    vector<float> values;
    std::istringstream in(line);
    while (in.good()) {
        double value = 0;   // what a failed read leaves behind, and the reference stores
        in >> value;
        values.push_back((float)(scale * value));
        in >> std::ws;
        if (!in.good()) break;
        const int next = in.peek();
        if (!(std::isdigit(next) || next == '+' || next == '-' || next == '.')) in.get();   // the separator
    }
    return values;
}

void LibLinearClassifier::loadStaticNegatives(const string& negativesFilename, int maxNegatives, double scale) {   // :48-84
    std::ifstream file(negativesFilename.c_str());
    if (!file.is_open()) return;
    string line;
    for (int negatives = 0; file.good() && negatives < maxNegatives && std::getline(file, line); ++negatives)
        staticNegativeExamples.push_back(parseStaticNegative(line, scale));
}

bool LibLinearClassifier::retrain(const vector<Mat>& newPositiveExamples, const vector<Mat>& newNegativeExamples) {   // :86-110
    if (newPositiveExamples.empty() && newNegativeExamples.empty()) return usable;
    positiveExamples->add(newPositiveExamples);
    negativeExamples->add(newNegativeExamples);
    if (!positiveExamples->hasRequiredSize() || !negativeExamples->hasRequiredSize()) return usable;
    vector<float> x;
    int dimensions = -1, rows = 0, cols = 0, type = 0;
    ExampleManagement* stores[2] = {positiveExamples.get(), negativeExamples.get()};
    for (ExampleManagement* store : stores)   // createProblem (:120-148): positives, negatives, static negatives
        for (auto it = store->iterator(); it->hasNext();) {
            const Mat& example = it->next();
            if (example.depth() != CV_32F) throw std::invalid_argument("LibLinearClassifier: examples have to be of depth CV_32F on this backend");
            if (!example.isContinuous()) throw std::invalid_argument("LibLinearUtils: vector has to be continuous");
            const int dim = (int)(example.total() * example.channels());
            if (dimensions < 0) {
                dimensions = dim;
                rows = example.rows;
                cols = example.cols;
                type = example.type();
            } else if (dim != dimensions) {
                throw std::invalid_argument("LibLinearClassifier: examples have to have the same length");
            }
            x.insert(x.end(), example.ptr<float>(), example.ptr<float>() + dim);
        }
    for (const vector<float>& example : staticNegativeExamples) {
        if (dimensions < 0 || (int)example.size() != dimensions)
            throw std::invalid_argument("LibLinearClassifier: a static negative example has " + std::to_string(example.size()) + " values, the examples " +
                                        std::to_string(std::max(dimensions, 0)));
        x.insert(x.end(), example.begin(), example.end());
    }
    const int positiveCount = (int)positiveExamples->size();
    const int negativeCount = (int)(negativeExamples->size() + staticNegativeExamples.size());
    fd_liblinear_params params = {};   // the constructor's parameter (:32-46): L2R_L2LOSS_SVC, eps 0.01, no weights
    params.C = c;
    params.weight_pos = params.weight_neg = 1.0;
    params.eps = 0.01;
    params.bias = bias ? 1 : 0;
    vector<float> weights(std::max(dimensions, 0));
    float b = 0;
    fd_liblinear_info info;
    check(fd_liblinear_train(context(), x.data(), positiveCount, negativeCount, dimensions, 0, &params, weights.data(), &b, nullptr, nullptr, 0, &info));
    Mat w(rows, cols, type);   // LibLinearUtils::extractSupportVectors: one vector of the examples' shape, coefficient 1
    std::memcpy(w.data, weights.data(), sizeof(float) * weights.size());
    svm->setSvmParameters(vector<Mat>{w}, vector<float>{1.f}, b);
    lastParams = params;
    lastInfo = info;
    lastPositiveCount = positiveCount;
    lastNegativeCount = negativeCount;
    usable = true;
    return usable;
}

void LibLinearClassifier::reset() {   // :150-155
    usable = false;
    svm->setSvmParameters(vector<Mat>(), vector<float>(), 0.0);
    positiveExamples->clear();
    negativeExamples->clear();
}

}  // namespace liblinear

// =================================================================================================
namespace detection {
using classification::ProbabilisticRvmClassifier;
using classification::ProbabilisticSvmClassifier;
using classification::ProbabilisticWvmClassifier;
using imageprocessing::DirectPyramidFeatureExtractor;
using imageprocessing::Patch;

static shared_ptr<ClassifiedPatch> to_patch(const fd_detection& d) {
    return make_shared<ClassifiedPatch>(make_shared<Patch>(d.cx, d.cy, d.w, d.h, Mat()), d.positive != 0, d.probability);
}
static vector<shared_ptr<ClassifiedPatch>> to_patches(const vector<fd_detection>& dets) {
    vector<shared_ptr<ClassifiedPatch>> out;
    for (const fd_detection& d : dets) out.push_back(to_patch(d));
    return out;
}
static fd_detection from_patch(const ClassifiedPatch& p) {
    fd_detection d;
    std::memset(&d, 0, sizeof(d));
    d.cx = p.getPatch()->getX(); d.cy = p.getPatch()->getY(); d.w = p.getPatch()->getWidth(); d.h = p.getPatch()->getHeight();
    d.positive = p.isPositive(); d.probability = p.getProbability();
    return d;
}

// ---- the route decision (not in the reference) ------------------------------------------------------------------------------------
bool hasF32SupportVectors(const ProbabilisticSvmClassifier* psvm) {
    return psvm && !psvm->getSvm()->getSupportVectors().empty() && psvm->getSvm()->getSupportVectors()[0].depth() == CV_32F;
}
shared_ptr<DirectPyramidFeatureExtractor> resolveFusedExtractor(const shared_ptr<imageprocessing::PyramidFeatureExtractor>& extractor) {
    if (auto filtering = std::dynamic_pointer_cast<imageprocessing::FilteringPyramidFeatureExtractor>(extractor)) return filtering->getFusedExtractor();
    return std::dynamic_pointer_cast<DirectPyramidFeatureExtractor>(extractor);
}
FusedScan fusedScanRoute(const DirectPyramidFeatureExtractor* fused, const classification::ProbabilisticClassifier* classifier) {
    if (!fused) return FusedScan::Generic;
    auto* psvm = dynamic_cast<const ProbabilisticSvmClassifier*>(classifier);
    const bool f32sv = hasF32SupportVectors(psvm);
    if (dynamic_cast<const ProbabilisticWvmClassifier*>(classifier) && fused->hasHistEq64()) return FusedScan::Wvm;
    if (f32sv && fused->getHogFilter() && std::dynamic_pointer_cast<classification::RbfKernel>(psvm->getSvm()->getKernel())) return FusedScan::HogSvm;
    if (dynamic_cast<const ProbabilisticRvmClassifier*>(classifier) && fused->getConversion() && !fused->getHistogramFilter() && !fused->getWhiChain())
        return FusedScan::Rvm;
    if (f32sv && fused->getWhiChain()) return FusedScan::WhiSvm;
    if (f32sv && fused->getHistogramFilter()) return FusedScan::HistSvm;
    return FusedScan::Generic;
}
FiveStageRoute fiveStageRoute(const DirectPyramidFeatureExtractor* fused, const classification::ProbabilisticClassifier* first,
                              const classification::ProbabilisticClassifier* second) {
    auto* psvm = dynamic_cast<const ProbabilisticSvmClassifier*>(second);
    if (fused && dynamic_cast<const ProbabilisticWvmClassifier*>(first) && psvm && fused->hasHistEq64() && !hasF32SupportVectors(psvm))
        return FiveStageRoute::WvmSvm;
    if (fusedScanRoute(fused, first) != FusedScan::Rvm) return FiveStageRoute::Composition;
    auto* prvm = dynamic_cast<const ProbabilisticRvmClassifier*>(first);
    const classification::RvmClassifier::Model& m1 = prvm->getRvm()->getModel();
    bool fits = false;
    if (hasF32SupportVectors(psvm)) {
        const Mat& sv = psvm->getSvm()->getSupportVectors()[0];
        fits = (int)(sv.total() * sv.channels()) == m1.filter_w * m1.filter_h;
    } else if (auto* prvm2 = dynamic_cast<const ProbabilisticRvmClassifier*>(second)) {
        const classification::RvmClassifier::Model& m2 = prvm2->getRvm()->getModel();
        fits = prvm2->getRvm() != prvm->getRvm() && m2.filter_w == m1.filter_w && m2.filter_h == m1.filter_h;
    }
    return fits ? FiveStageRoute::RvmSecond : FiveStageRoute::Composition;
}

vector<shared_ptr<ClassifiedPatch>> OverlapElimination::eliminate(vector<shared_ptr<ClassifiedPatch>>& classifiedPatches) {
    vector<shared_ptr<ClassifiedPatch>> out;
    if (classifiedPatches.empty()) return out;
    vector<fd_detection> dets;
    for (const auto& p : classifiedPatches) dets.push_back(from_patch(*p));
    vector<int32_t> keep(dets.size());
    int n = 0;
    if (fd_overlap_elimination(dets.data(), (int)dets.size(), dist, ratio, keep.data(), &n) != FD_OK)
        throw std::runtime_error("OverlapElimination: invalid arguments");
    for (int i = 0; i < n; ++i) out.push_back(classifiedPatches[keep[i]]);
    return out;
}

vector<Detection> NonMaximumSuppression::eliminateRedundantDetections(vector<Detection> candidates) const {
    vector<fd_box> in(candidates.size()), out(candidates.size());
    for (size_t i = 0; i < candidates.size(); ++i)
        in[i] = fd_box{candidates[i].score, candidates[i].bounds.x, candidates[i].bounds.y, candidates[i].bounds.width, candidates[i].bounds.height};
    int n = 0;
    const int rc = fd_nms_iou(in.data(), (int)in.size(), overlapThreshold, (int)maximumType, out.data(), &n);
    if (rc == FD_ERR_RUNTIME) throw std::runtime_error("NonMaximumSuppression: the overlap threshold must not exceed one");
    if (rc != FD_OK) throw std::invalid_argument("NonMaximumSuppression: invalid arguments");
    vector<Detection> res;
    for (int i = 0; i < n; ++i) res.push_back(Detection{out[i].score, cv::Rect(out[i].x, out[i].y, out[i].w, out[i].h)});
    return res;
}

}  // namespace detection
namespace imageprocessing { namespace extraction {
static const char* const kExtractorFilters =
    "AggregatedFeaturesExtractor: this backend needs a GrayscaleFilter image filter and a filtering::FhogFilter layer filter, a "
    "filtering::FhogFilter alone (gray images), or ChainedFilter(filtering::FpdwFeaturesFilter, filtering::AggregationFilter) alone";
AggregatedFeaturesExtractor::AggregatedFeaturesExtractor(shared_ptr<ImagePyramid> featurePyramid, cv::Size patchSizeInCells, int cellSizeInPixels,
                                                         bool adjustMinScaleFactor, int minPatchWidthInPixels)
    : featurePyramid(featurePyramid), patchSizeInCells(patchSizeInCells), cellSizeInPixels(cellSizeInPixels),
      minPatchWidthInPixels(minPatchWidthInPixels) {
    if (!featurePyramid) throw std::invalid_argument("AggregatedFeaturesExtractor: the feature pyramid must not be null");
    if (!featurePyramid->isApproximated())
        throw std::logic_error("AggregatedFeaturesExtractor: on this backend the feature pyramid must come from ImagePyramid::createApproximated "
                               "(exact feature pyramids: the filter constructors)");
    if (!adjustMinScaleFactor)
        throw std::logic_error("AggregatedFeaturesExtractor: a fixed minimum scale factor is not available on this backend (adjustMinScaleFactor)");
    if (patchSizeInCells.width < 1 || patchSizeInCells.height < 1 || cellSizeInPixels < 1)
        throw std::invalid_argument("AggregatedFeaturesExtractor: patch and cell sizes must be positive");
    octaveLayerCount = (int)featurePyramid->getOctaveLayerCount();
}
AggregatedFeaturesExtractor::AggregatedFeaturesExtractor(shared_ptr<ImageFilter> layerFilter, cv::Size patchSizeInCells, int cellSizeInPixels,
                                                         int octaveLayerCount, int minPatchWidthInPixels)
    : patchSizeInCells(patchSizeInCells), cellSizeInPixels(cellSizeInPixels), minPatchWidthInPixels(minPatchWidthInPixels),
      octaveLayerCount(octaveLayerCount) {
    init(nullptr, layerFilter.get());
}
AggregatedFeaturesExtractor::AggregatedFeaturesExtractor(shared_ptr<ImageFilter> imageFilter, shared_ptr<ImageFilter> layerFilter,
                                                         cv::Size patchSizeInCells, int cellSizeInPixels, int octaveLayerCount,
                                                         int minPatchWidthInPixels)
    : patchSizeInCells(patchSizeInCells), cellSizeInPixels(cellSizeInPixels), minPatchWidthInPixels(minPatchWidthInPixels),
      octaveLayerCount(octaveLayerCount) {
    if (!imageFilter) throw std::invalid_argument("AggregatedFeaturesExtractor: the image filter must not be null");
    init(imageFilter.get(), layerFilter.get());
}
AggregatedFeaturesExtractor::~AggregatedFeaturesExtractor() { if (handle) fd_aggregated_destroy(handle); }

// the handle of the filter forms (an exact feature pyramid); the model is a placeholder until detectWindows installs one
static fd_aggregated* create_extractor_handle(const filtering::FhogFilter* fhog, const fd_fpdw_params* fpdw, cv::Size patch, int cell, int octaveLayers,
                                              int minPatchWidth, const vector<double>* lambdas, int channels) {
    fd_aggregated_params prm;
    std::memset(&prm, 0, sizeof(prm));
    if (fpdw) prm.fhog.cell_size = fpdw->cell_size;
    else prm.fhog = fd_fhog_params{fhog->cellSize, fhog->unsignedBinCount, fhog->interpolateBins, fhog->interpolateCells, fhog->alpha};
    if (prm.fhog.cell_size != cell) throw std::invalid_argument("AggregatedFeaturesExtractor: cellSizeInPixels differs from the layer filter's");
    prm.window_w = patch.width; prm.window_h = patch.height; prm.octave_layer_count = octaveLayers;
    prm.min_window_width = minPatchWidth; prm.width_scale = 1.f; prm.height_scale = 1.f;
    const vector<float> zeros((size_t)patch.width * patch.height * channels, 0.f);
    prm.svm_weights = zeros.data();
    prm.nms_overlap_threshold = 1.0;   // NonMaximumSuppression(1.0): no suppression
    fd_aggregated* handle = nullptr;
    if (fpdw) check(fd_aggregated_create_fpdw(context(), &prm, fpdw, lambdas != nullptr, lambdas ? lambdas->data() : nullptr,
                                              lambdas ? (int)lambdas->size() : 0, &handle));
    else if (lambdas) check(fd_aggregated_create_approximated(context(), &prm, lambdas->data(), (int)lambdas->size(), &handle));
    else check(fd_aggregated_create(context(), &prm, &handle));
    return handle;
}
void AggregatedFeaturesExtractor::init(const ImageFilter* imageFilter, const ImageFilter* layerFilter) {
    if (patchSizeInCells.width < 1 || patchSizeInCells.height < 1 || cellSizeInPixels < 1 || octaveLayerCount < 1)
        throw std::invalid_argument("AggregatedFeaturesExtractor: patch and cell sizes and the octave layer count must be positive");
    auto fhog = dynamic_cast<const filtering::FhogFilter*>(layerFilter);
    fd_fpdw_params fp;
    if (fhog && (!imageFilter || dynamic_cast<const GrayscaleFilter*>(imageFilter))) {
        channels = 3 * fhog->unsignedBinCount + 4;
        grayOnly = imageFilter == nullptr;
        handle = create_extractor_handle(fhog, nullptr, patchSizeInCells, cellSizeInPixels, octaveLayerCount, minPatchWidthInPixels, nullptr, channels);
    } else if (!imageFilter && fpdw_chain(layerFilter, fp)) {
        channels = 10;
        colorOnly = true;
        handle = create_extractor_handle(nullptr, &fp, patchSizeInCells, cellSizeInPixels, octaveLayerCount, minPatchWidthInPixels, nullptr, channels);
    } else {
        throw std::logic_error(kExtractorFilters);
    }
}
void AggregatedFeaturesExtractor::update(shared_ptr<VersionedImage> versioned) {
    if (!handle) {   // the feature-pyramid form: what AggregatedFeaturesDetector's extractor constructor reads from the pyramid
        auto fhog = std::dynamic_pointer_cast<filtering::FhogFilter>(featurePyramid->getApproximatedLayerFilter());
        fd_fpdw_params fp;
        const bool fpdw = featurePyramid->hasNoImageFilter() && fpdw_chain(featurePyramid->getApproximatedLayerFilter().get(), fp);
        if (!fpdw && (!featurePyramid->hasGrayscaleImageFilter() || !fhog)) throw std::logic_error(kExtractorFilters);
        channels = fpdw ? 10 : 3 * fhog->unsignedBinCount + 4;
        colorOnly = fpdw;
        handle = create_extractor_handle(fpdw ? nullptr : fhog.get(), fpdw ? &fp : nullptr, patchSizeInCells, cellSizeInPixels, octaveLayerCount,
                                         minPatchWidthInPixels, &featurePyramid->getLambdas(), channels);
    }
    Mat img = contiguous(versioned->getData());
    if (img.depth() != CV_8U) throw std::invalid_argument("AggregatedFeaturesExtractor: the image must be of depth CV_8U");
    if (grayOnly && img.channels() != 1) throw std::invalid_argument("FhogFilter: the image must be of type CV_8UC1 (add a GrayscaleFilter as image filter)");
    if (colorOnly && img.channels() != 3) throw std::invalid_argument("FpdwFeaturesFilter: the image must be of type CV_8UC3");
    check(fd_aggregated_update(context(), handle, img.data, img.cols, img.rows, img.channels(), 0));
    image = img;
}
shared_ptr<Patch> AggregatedFeaturesExtractor::extract(int centerX, int centerY, int width, int height) const {
    return extract(cv::Rect(centerX - width / 2, centerY - height / 2, width, height));   // Patch::computeBounds
}
shared_ptr<Patch> AggregatedFeaturesExtractor::extract(cv::Rect bounds) const { return extract(vector<cv::Rect>{bounds})[0]; }
vector<shared_ptr<Patch>> AggregatedFeaturesExtractor::extract(const vector<cv::Rect>& boxes) const {
    if (!handle) throw std::runtime_error("AggregatedFeaturesExtractor: update has to be called before extract");
    const int n = (int)boxes.size();
    vector<shared_ptr<Patch>> patches((size_t)n);
    if (n == 0) return patches;
    const size_t d = (size_t)patchSizeInCells.width * patchSizeInCells.height * channels;
    vector<int32_t> in((size_t)4 * n);
    for (int k = 0; k < n; ++k) {
        in[4 * k] = boxes[k].x; in[4 * k + 1] = boxes[k].y; in[4 * k + 2] = boxes[k].width; in[4 * k + 3] = boxes[k].height;
    }
    vector<float> features(d * n);
    vector<fd_box> bounds((size_t)n);
    vector<uint8_t> valid((size_t)n);
    check(fd_aggregated_extract(context(), handle, n, in.data(), features.data(), 0, bounds.data(), valid.data()));
    for (int k = 0; k < n; ++k) {
        if (!valid[k]) continue;
        Mat data(patchSizeInCells.height, patchSizeInCells.width, CV_32FC(channels));
        std::memcpy(data.data, features.data() + d * k, sizeof(float) * d);
        const fd_box& b = bounds[k];   // Patch(bounds, data): Patch::computeCenter
        patches[k] = make_shared<Patch>(b.x + b.w / 2, b.y + b.h / 2, b.w, b.h, data);
    }
    return patches;
}
vector<std::pair<cv::Rect, float>> AggregatedFeaturesExtractor::detectWindows(const classification::SvmClassifier& svm, float threshold) {
    if (!handle || image.empty()) throw std::runtime_error("AggregatedFeaturesExtractor: update has to be called before detectWindows");
    if (svm.getSupportVectors().size() != 1) throw std::invalid_argument("AggregatedFeaturesExtractor: a linear SVM with one support vector is needed");
    Mat sv = contiguous(svm.getSupportVectors()[0]);
    if (sv.depth() != CV_32F || (int)(sv.total() * sv.channels()) != patchSizeInCells.width * patchSizeInCells.height * channels)
        throw std::invalid_argument("AggregatedFeaturesExtractor: the support vector must hold patchSizeInCells x channels floats");
    check(fd_aggregated_set_svm(context(), handle, sv.ptr<float>(0), svm.getBias(), threshold));
    vector<fd_box> fin(1), cand(1 << 14);
    int n = 0, nc = 0;
    // the candidates are the windows before suppression; the final detections are not asked for (a capacity of 0 reports their count only)
    int rc = fd_aggregated_detect(context(), handle, image.data, image.cols, image.rows, image.channels(), 0, nullptr, 0, &n, cand.data(), (int)cand.size(), &nc);
    check(rc);
    if (nc > (int)cand.size()) {
        cand.resize((size_t)nc);
        check(fd_aggregated_detect(context(), handle, image.data, image.cols, image.rows, image.channels(), 0, nullptr, 0, &n, cand.data(), nc, &nc));
    }
    vector<std::pair<cv::Rect, float>> res;
    for (int i = 0; i < nc; ++i) res.emplace_back(cv::Rect(cand[i].x, cand[i].y, cand[i].w, cand[i].h), cand[i].score);
    return res;
}
}}  // namespace imageprocessing::extraction
namespace detection {
AggregatedFeaturesDetector::AggregatedFeaturesDetector(shared_ptr<imageprocessing::ImageFilter> imageFilter, shared_ptr<imageprocessing::ImageFilter> layerFilter,
                                                       int cellSize, cv::Size windowSize, int octaveLayerCount,
                                                       shared_ptr<classification::SvmClassifier> svm, shared_ptr<NonMaximumSuppression> nms,
                                                       float widthScale, float heightScale, int minWindowWidth)
    : scoreThreshold(svm->getThreshold()) {
    if (!dynamic_cast<classification::LinearKernel*>(svm->getKernel().get()))
        throw std::invalid_argument("AggregatedFeaturesDetector: the SVM must use a LinearKernel");
    auto fhog = std::dynamic_pointer_cast<imageprocessing::filtering::FhogFilter>(layerFilter);
    if (!std::dynamic_pointer_cast<imageprocessing::GrayscaleFilter>(imageFilter) || !fhog)
        throw std::logic_error("AggregatedFeaturesDetector: this backend needs a GrayscaleFilter image filter and a filtering::FhogFilter layer filter");
    if (fhog->cellSize != cellSize) throw std::invalid_argument("AggregatedFeaturesDetector: cellSize differs from the FhogFilter's");
    create(fhog.get(), nullptr, windowSize, octaveLayerCount, *svm, *nms, widthScale, heightScale, minWindowWidth, nullptr);
}
static const char* const kAggregatedFilters =
    "AggregatedFeaturesDetector: this backend needs a GrayscaleFilter image filter and a filtering::FhogFilter layer filter, or no image "
    "filter and ChainedFilter(filtering::FpdwFeaturesFilter, filtering::AggregationFilter) as the only filter";
AggregatedFeaturesDetector::AggregatedFeaturesDetector(shared_ptr<imageprocessing::ImageFilter> filter, int cellSize, cv::Size windowSize,
                                                       int octaveLayerCount, shared_ptr<classification::SvmClassifier> svm,
                                                       shared_ptr<NonMaximumSuppression> nms, float widthScale, float heightScale, int minWindowWidth)
    : scoreThreshold(svm->getThreshold()) {
    if (!dynamic_cast<classification::LinearKernel*>(svm->getKernel().get()))
        throw std::invalid_argument("AggregatedFeaturesDetector: the SVM must use a LinearKernel");
    fd_fpdw_params fp;
    if (!imageprocessing::fpdw_chain(filter.get(), fp)) throw std::logic_error(kAggregatedFilters);
    if (fp.cell_size != cellSize) throw std::invalid_argument("AggregatedFeaturesDetector: cellSize differs from the AggregationFilter's");
    create(nullptr, &fp, windowSize, octaveLayerCount, *svm, *nms, widthScale, heightScale, minWindowWidth, nullptr);
}
AggregatedFeaturesDetector::AggregatedFeaturesDetector(shared_ptr<imageprocessing::extraction::AggregatedFeaturesExtractor> featureExtractor,
                                                       shared_ptr<classification::SvmClassifier> svm, shared_ptr<NonMaximumSuppression> nms,
                                                       float widthScale, float heightScale)
    : scoreThreshold(svm->getThreshold()) {
    if (!featureExtractor) throw std::invalid_argument("AggregatedFeaturesDetector: the feature extractor must not be null");
    if (!dynamic_cast<classification::LinearKernel*>(svm->getKernel().get()))
        throw std::invalid_argument("AggregatedFeaturesDetector: the SVM must use a LinearKernel");
    auto pyramid = featureExtractor->getFeaturePyramid();
    auto fhog = std::dynamic_pointer_cast<imageprocessing::filtering::FhogFilter>(pyramid->getApproximatedLayerFilter());
    fd_fpdw_params fp;
    const bool fpdw = pyramid->hasNoImageFilter() && imageprocessing::fpdw_chain(pyramid->getApproximatedLayerFilter().get(), fp);
    if (!fpdw && (!pyramid->hasGrayscaleImageFilter() || !fhog)) throw std::logic_error(kAggregatedFilters);
    if ((fpdw ? fp.cell_size : fhog->cellSize) != featureExtractor->getCellSizeInPixels())
        throw std::invalid_argument("AggregatedFeaturesDetector: cellSize differs from the layer filter's");
    create(fpdw ? nullptr : fhog.get(), fpdw ? &fp : nullptr, featureExtractor->getPatchSizeInCells(), (int)pyramid->getOctaveLayerCount(), *svm, *nms, widthScale, heightScale,
           featureExtractor->getMinPatchWidthInPixels(), &pyramid->getLambdas());
}
void AggregatedFeaturesDetector::create(const imageprocessing::filtering::FhogFilter* fhog, const fd_fpdw_params* fpdw, cv::Size windowSize,
                                        int octaveLayerCount, const classification::SvmClassifier& svmRef, const NonMaximumSuppression& nmsRef,
                                        float widthScale, float heightScale, int minWindowWidth, const vector<double>* lambdas) {
    const classification::SvmClassifier* svm = &svmRef;
    const NonMaximumSuppression* nms = &nmsRef;
    const int D = fpdw ? 10 : 3 * fhog->unsignedBinCount + 4;
    if (svm->getSupportVectors().size() != 1) throw std::invalid_argument("AggregatedFeaturesDetector: a linear SVM with one support vector is needed");
    Mat sv = contiguous(svm->getSupportVectors()[0]);
    if (sv.depth() != CV_32F || (int)(sv.total() * sv.channels()) != windowSize.width * windowSize.height * D)
        throw std::invalid_argument(fpdw ? "AggregatedFeaturesDetector: the support vector must hold windowSize x 10 floats"
                                         : "AggregatedFeaturesDetector: the support vector must hold windowSize x (3 * unsignedBinCount + 4) floats");
    fd_aggregated_params prm;
    std::memset(&prm, 0, sizeof(prm));
    if (fpdw) prm.fhog.cell_size = fpdw->cell_size;
    else prm.fhog = fd_fhog_params{fhog->cellSize, fhog->unsignedBinCount, fhog->interpolateBins, fhog->interpolateCells, fhog->alpha};
    prm.window_w = windowSize.width; prm.window_h = windowSize.height; prm.octave_layer_count = octaveLayerCount;
    prm.min_window_width = minWindowWidth; prm.width_scale = widthScale; prm.height_scale = heightScale;
    // SvmClassifier: distance = -bias + coefficient * <sv, x>; the reference convolves the raw support vector (coefficients are 1)
    prm.svm_weights = sv.ptr<float>(0);
    prm.svm_bias = svm->getBias(); prm.score_threshold = svm->getThreshold();
    prm.nms_overlap_threshold = nms->getOverlapThreshold(); prm.nms_maximum_type = (int)nms->getMaximumType();
    if (fpdw) check(fd_aggregated_create_fpdw(context(), &prm, fpdw, lambdas != nullptr, lambdas ? lambdas->data() : nullptr,
                                              lambdas ? (int)lambdas->size() : 0, &handle));
    else if (lambdas) check(fd_aggregated_create_approximated(context(), &prm, lambdas->data(), (int)lambdas->size(), &handle));
    else check(fd_aggregated_create(context(), &prm, &handle));
}
vector<double> AggregatedFeaturesDetector::getLambdas() const {
    vector<double> out(64);
    int n = 0;
    check(fd_aggregated_get_lambdas(handle, out.data(), (int)out.size(), &n));
    out.resize((size_t)n);
    return out;
}
AggregatedFeaturesDetector::~AggregatedFeaturesDetector() { fd_aggregated_destroy(handle); }
vector<std::pair<cv::Rect, float>> AggregatedFeaturesDetector::detectWithScores(shared_ptr<imageprocessing::VersionedImage> image) {
    Mat img = contiguous(image->getData());
    const vector<fd_box> out = with_capacity<fd_box>(1 << 14, [&](fd_box* boxes, int cap, int* n) {
        return fd_aggregated_detect(context(), handle, img.data, img.cols, img.rows, img.channels(), 0, boxes, cap, n, nullptr, 0, nullptr);
    });
    vector<std::pair<cv::Rect, float>> res;
    for (const fd_box& b : out) res.emplace_back(cv::Rect(b.x, b.y, b.w, b.h), b.score);
    return res;
}
vector<cv::Rect> AggregatedFeaturesDetector::detect(shared_ptr<imageprocessing::VersionedImage> image) {
    vector<cv::Rect> res;
    for (const auto& d : detectWithScores(image)) res.push_back(d.first);
    return res;
}

SlidingWindowDetector::SlidingWindowDetector(shared_ptr<classification::ProbabilisticClassifier> classifier,
                                             shared_ptr<imageprocessing::PyramidFeatureExtractor> featureExtractor, int sx, int sy)
    : classifier(classifier), featureExtractor(featureExtractor), stepSizeX(sx), stepSizeY(sy) {}

void Detector::fillPatchData(const imageprocessing::PyramidFeatureExtractor& extractor, vector<shared_ptr<ClassifiedPatch>>& patches) const {
    for (auto& cp : patches) {
        auto p = cp->getPatch();
        if (!p || !p->getData().empty()) continue;
        auto q = extractor.extract(p->getX(), p->getY(), p->getWidth(), p->getHeight());
        if (q) p->getData() = q->getData();
    }
}
vector<shared_ptr<ClassifiedPatch>> SlidingWindowDetector::detect(const cv::Rect* roi) const {
    auto out = detectWindows(roi);
    if (patchData) fillPatchData(*featureExtractor, out);
    return out;
}
vector<shared_ptr<ClassifiedPatch>> SlidingWindowDetector::detectWindows(const cv::Rect* roi) const {
    auto direct = resolveFusedExtractor(featureExtractor);   // ffpDetectApp.cpp:445: same pyramid, the chain as patch filters; null = generic composition
    // the region of interest (SlidingWindowDetector.cpp:53-78) and the scale range of a pyramid built on another pyramid
    // apply to the window enumeration of every fused chain
    std::unique_ptr<imageprocessing::ImagePyramid::Selection> selection;
    if (direct) selection.reset(new imageprocessing::ImagePyramid::Selection(direct->getPyramid()->select(-1, -1, 1, roi)));
    auto psvm = std::dynamic_pointer_cast<ProbabilisticSvmClassifier>(classifier);
    int r[4] = {0, 0, 0, 0};
    if (roi) { r[0] = roi->x; r[1] = roi->y; r[2] = roi->width; r[3] = roi->height; }
    const int64_t cap = 1 << 16;
    switch (fusedScanRoute(direct.get(), classifier.get())) {
    case FusedScan::Wvm: {   // fused extract + HistEq64 + WVM cascade
        auto pwvm = std::dynamic_pointer_cast<ProbabilisticWvmClassifier>(classifier);
        const fd_wvm* w = pwvm->getWvm()->native(pwvm->getLogisticA(), pwvm->getLogisticB());
        return to_patches(with_capacity<fd_detection>(cap, [&](fd_detection* dets, int64_t n, int64_t* cnt) {
            return fd_detect_wvm(context(), direct->getPyramid()->native(), w, stepSizeX, stepSizeY, roi ? r : nullptr, dets, n, cnt, nullptr, nullptr);
        }));
    }
    case FusedScan::HogSvm: {   // fused HOG + MFMA RBF-SVM
        auto hog = direct->getHogFilter();
        fd_hog_params hp = {direct->getPatchWidth(), direct->getPatchHeight(), stepSizeX, stepSizeY, hog->binCount, hog->cellWidth, hog->blockWidth,
                            hog->signedAndUnsigned};
        const fd_svm* s = psvm->getSvm()->native(psvm->getLogisticA(), psvm->getLogisticB());
        return to_patches(with_capacity<fd_detection>(cap, [&](fd_detection* dets, int64_t n, int64_t* cnt) {
            return fd_detect_hog_svm(context(), direct->getPyramid()->native(), s, &hp, dets, n, cnt, nullptr);
        }));
    }
    case FusedScan::Rvm: {   // fused RVM cascade ("prvm")
        auto prvm = std::dynamic_pointer_cast<ProbabilisticRvmClassifier>(classifier);
        auto cf = direct->getConversion();
        fd_rvm_detect_params dp = {direct->getU8FeatureSpace(), (float)cf->alpha, (float)cf->beta, stepSizeX, stepSizeY};
        const fd_rvm* rv = prvm->getRvm()->native(prvm->getLogisticA(), prvm->getLogisticB());
        return to_patches(with_capacity<fd_detection>(cap, [&](fd_detection* dets, int64_t n, int64_t* cnt) {
            return fd_detect_rvm(context(), direct->getPyramid()->native(), rv, &dp, roi ? r : nullptr, dets, n, cnt, nullptr, nullptr);
        }));
    }
    case FusedScan::WhiSvm: {   // fused whi chain + SVM (ffpDetectApp.cpp:449-454, "psvm")
        auto wf = direct->getWhiChain();
        fd_whi_params wp = {direct->getPatchWidth(), direct->getPatchHeight(), stepSizeX, stepSizeY, wf->alpha, wf->cutoffFrequency};
        const fd_svm* s = psvm->getSvm()->native(psvm->getLogisticA(), psvm->getLogisticB());
        return to_patches(with_capacity<fd_detection>(cap, [&](fd_detection* dets, int64_t n, int64_t* cnt) {
            return fd_detect_whi_svm(context(), direct->getPyramid()->native(), s, &wp, dets, n, cnt, nullptr);
        }));
    }
    case FusedScan::HistSvm: {   // fused histogram features + SVM (any kernel)
        fd_hist_params hp = hist_params_of(*direct->getHistogramFilter(), direct->getPatchWidth(), direct->getPatchHeight(), stepSizeX, stepSizeY);
        const fd_svm* s = psvm->getSvm()->native(psvm->getLogisticA(), psvm->getLogisticB());
        return to_patches(with_capacity<fd_detection>(cap, [&](fd_detection* dets, int64_t n, int64_t* cnt) {
            return fd_detect_hist_svm(context(), direct->getPyramid()->native(), s, &hp, dets, n, cnt, nullptr);
        }));
    }
    case FusedScan::Generic:
        break;
    }
    // generic composition (SlidingWindowDetector.cpp:87-98): extract all, classify each through the per-Mat interface
    selection.reset();
    vector<shared_ptr<ClassifiedPatch>> out;
    auto patches = roi ? featureExtractor->extract(stepSizeX, stepSizeY, *roi) : featureExtractor->extract(stepSizeX, stepSizeY);
    for (auto& p : patches) {
        auto res = classifier->getProbability(p->getData());
        if (res.first) out.push_back(make_shared<ClassifiedPatch>(p, res));
    }
    return out;
}
vector<shared_ptr<ClassifiedPatch>> SlidingWindowDetector::detect(const Mat& image) {
    featureExtractor->update(image);
    return detect((const cv::Rect*)nullptr);
}
vector<shared_ptr<ClassifiedPatch>> SlidingWindowDetector::detect(const Mat& image, const cv::Rect& roi) {
    featureExtractor->update(image);
    return detect(&roi);
}
vector<shared_ptr<ClassifiedPatch>> SlidingWindowDetector::detect(shared_ptr<imageprocessing::VersionedImage> image) {
    featureExtractor->update(image);
    return detect((const cv::Rect*)nullptr);
}

FiveStageSlidingWindowDetector::FiveStageSlidingWindowDetector(shared_ptr<SlidingWindowDetector> swd, shared_ptr<OverlapElimination> oe,
                                                               shared_ptr<classification::ProbabilisticClassifier> strong)
    : slidingWindowDetector(swd), overlapElimination(oe), strongClassifier(strong) {}

// Three paths, chosen by fiveStageRoute:
//  WvmSvm: ProbabilisticWvmClassifier on HistEq64 patches + ProbabilisticSvmClassifier with u8 support vectors: fd_detect_five_stage
//  RvmSecond: the fused RVM case of SlidingWindowDetector::detectWindows ("prvm": a ConversionFilter behind a u8 feature space) + a
//     ProbabilisticSvmClassifier with f32 support vectors or a ProbabilisticRvmClassifier: fd_detect_five_stage_rvm
//  Composition: anything else: the reference's own composition, one classify() per survivor (FiveStageSlidingWindowDetector.cpp:187-320 / :331-380)
vector<shared_ptr<ClassifiedPatch>> FiveStageSlidingWindowDetector::run(const Mat& image, const cv::Rect* roi) {
    auto direct = resolveFusedExtractor(slidingWindowDetector->getPyramidFeatureExtractor());
    auto weak = slidingWindowDetector->getClassifier();
    auto psvm = std::dynamic_pointer_cast<ProbabilisticSvmClassifier>(strongClassifier);
    int r[4] = {0, 0, 0, 0};
    if (roi) { r[0] = roi->x; r[1] = roi->y; r[2] = roi->width; r[3] = roi->height; }
    const int cap = 4096;
    auto finish = [&](const vector<fd_detection>& dets) {
        auto out = to_patches(dets);
        if (patchData) fillPatchData(*slidingWindowDetector->getPyramidFeatureExtractor(), out);   // the patches of the shared extractor (FiveStageSlidingWindowDetector.cpp:187-380)
        return out;
    };
    switch (fiveStageRoute(direct.get(), weak.get(), strongClassifier.get())) {
    case FiveStageRoute::WvmSvm: {
        auto pwvm = std::dynamic_pointer_cast<ProbabilisticWvmClassifier>(weak);
        direct->update(image);
        auto selection = direct->getPyramid()->select();   // the scale range of a pyramid built on another pyramid
        const fd_wvm* w = pwvm->getWvm()->native(pwvm->getLogisticA(), pwvm->getLogisticB());
        const fd_svm* s = psvm->getSvm()->native(psvm->getLogisticA(), psvm->getLogisticB());
        return finish(with_capacity<fd_detection>(cap, [&](fd_detection* dets, int n, int* cnt) {
            return fd_detect_five_stage(context(), direct->getPyramid()->native(), w, s, overlapElimination->getDist(), overlapElimination->getRatio(),
                                        slidingWindowDetector->getStepSizeX(), slidingWindowDetector->getStepSizeY(), roi ? r : nullptr, dets, n, cnt, nullptr);
        }));
    }
    case FiveStageRoute::RvmSecond: {
        auto prvm = std::dynamic_pointer_cast<ProbabilisticRvmClassifier>(weak);
        auto prvm2 = std::dynamic_pointer_cast<ProbabilisticRvmClassifier>(strongClassifier);
        const bool f32sv = hasF32SupportVectors(psvm.get());
        direct->update(image);
        auto selection = direct->getPyramid()->select();
        auto cf = direct->getConversion();
        fd_rvm_detect_params dp = {direct->getU8FeatureSpace(), (float)cf->alpha, (float)cf->beta, slidingWindowDetector->getStepSizeX(),
                                   slidingWindowDetector->getStepSizeY()};
        const fd_rvm* first = prvm->getRvm()->native(prvm->getLogisticA(), prvm->getLogisticB());
        const fd_svm* s2 = f32sv ? psvm->getSvm()->native(psvm->getLogisticA(), psvm->getLogisticB()) : nullptr;
        const fd_rvm* r2 = f32sv ? nullptr : prvm2->getRvm()->native(prvm2->getLogisticA(), prvm2->getLogisticB());
        return finish(with_capacity<fd_detection>(cap, [&](fd_detection* dets, int n, int* cnt) {
            return fd_detect_five_stage_rvm(context(), direct->getPyramid()->native(), first, &dp, s2, r2, overlapElimination->getDist(),
                                            overlapElimination->getRatio(), roi ? r : nullptr, dets, n, cnt, nullptr);
        }));
    }
    case FiveStageRoute::Composition:
        break;
    }
    // the reference's composition: the first detector's positives with their patch data, overlap elimination, one classify() per survivor
    vector<shared_ptr<ClassifiedPatch>> first;
    {
        struct KeepData {   // the strong classifier needs the survivors' pixels whatever the caller asked this detector to keep
            SlidingWindowDetector& d;
            bool was;
            explicit KeepData(SlidingWindowDetector& d_) : d(d_), was(d_.keepsPatchData()) { d.keepPatchData(true); }
            ~KeepData() { d.keepPatchData(was); }
        } keepData(*slidingWindowDetector);
        first = roi ? slidingWindowDetector->detect(image, *roi) : slidingWindowDetector->detect(image);
    }
    vector<shared_ptr<ClassifiedPatch>> survivors = overlapElimination->eliminate(first), positives;
    for (const auto& p : survivors)
        if (strongClassifier->classify(p->getPatch()->getData())) positives.push_back(make_shared<ClassifiedPatch>(p->getPatch(), true));   // probability 0.5 (ClassifiedPatch.hpp:29-30)
    auto byProb = [](const shared_ptr<ClassifiedPatch>& a, const shared_ptr<ClassifiedPatch>& b) { return *a > *b; };
    if (!roi) {   // block NMS on the probability map (:262-320), as five_stage_nms of the fused paths
        vector<fd_detection> dets;
        for (const auto& p : positives) dets.push_back(from_patch(*p));
        vector<int32_t> xy(2 * dets.size() + 2);
        int n = 0;
        for (int masked = 1; masked >= 0 && n == 0 && !dets.empty(); --masked)
            check(fd_block_nms(dets.data(), (int)dets.size(), image.cols, image.rows, 35, masked, xy.data(), (int)dets.size() + 1, &n));
        if (n == 0) return positives;   // "return svmPatchesPositive; // Should be empty." (:292-294), unsorted
        std::sort(positives.begin(), positives.end(), byProb);
        vector<shared_ptr<ClassifiedPatch>> res;
        for (int i = 0; i < n; ++i) {
            auto it = std::find_if(positives.begin(), positives.end(), [&](const shared_ptr<ClassifiedPatch>& p) {
                return p->getPatch()->getX() == xy[2 * (size_t)i] && p->getPatch()->getY() == xy[2 * (size_t)i + 1];
            });
            if (it != positives.end()) res.push_back(*it);
        }
        positives.swap(res);
    }
    std::sort(positives.begin(), positives.end(), byProb);
    return positives;
}
FiveStageSlidingWindowDetector::~FiveStageSlidingWindowDetector() { if (framesPyramid) fd_pyramid_destroy(framesPyramid); }

vector<vector<shared_ptr<ClassifiedPatch>>> FiveStageSlidingWindowDetector::detectFrames(const vector<Mat>& images) {
    vector<vector<shared_ptr<ClassifiedPatch>>> out(images.size());
    auto direct = resolveFusedExtractor(slidingWindowDetector->getPyramidFeatureExtractor());
    const bool wvmSvm = fiveStageRoute(direct.get(), slidingWindowDetector->getClassifier().get(), strongClassifier.get()) == FiveStageRoute::WvmSvm;
    auto pwvm = std::dynamic_pointer_cast<ProbabilisticWvmClassifier>(slidingWindowDetector->getClassifier());
    auto psvm = std::dynamic_pointer_cast<ProbabilisticSvmClassifier>(strongClassifier);
    size_t i = 0;
    while (i < images.size()) {
        // the longest run of images with the size and type of images[i], 64 at most
        size_t j = i + 1;
        while (j < images.size() && j - i < 64 && images[j].rows == images[i].rows && images[j].cols == images[i].cols && images[j].type() == images[i].type()) ++j;
        const int n = (int)(j - i);
        const int ch = images[i].channels();
        // (keepPatchData: the patches are cut from the extractor's own pyramid, which the multi-frame path never fills: one image at a time)
        bool fused = !patchData && wvmSvm && n > 1 && images[i].depth() == CV_8U && (ch == 1 || ch == 3);
        if (fused && (!framesPyramid || framesCount != n)) {
            if (framesPyramid) { fd_pyramid_destroy(framesPyramid); framesPyramid = nullptr; }
            framesPyramid = direct->getPyramid()->createFramesPyramid(n);
            framesCount = n;
            fused = framesPyramid != nullptr;
        }
        if (!fused) {
            for (size_t k = i; k < j; ++k) out[k] = detect(images[k]);
            i = j;
            continue;
        }
        vector<Mat> cont((size_t)n);
        vector<const uint8_t*> ptrs((size_t)n);
        for (int k = 0; k < n; ++k) {
            cont[(size_t)k] = images[i + (size_t)k].isContinuous() ? images[i + (size_t)k] : images[i + (size_t)k].clone();
            ptrs[(size_t)k] = cont[(size_t)k].data;
        }
        check(fd_pyramid_update_frames(framesPyramid, ptrs.data(), n, images[i].cols, images[i].rows, ch, 0));
        int cap = 1024;
        vector<fd_detection> dets;
        vector<int32_t> counts((size_t)n);
        for (;;) {
            dets.resize((size_t)cap * (size_t)n);
            const int rc = fd_detect_five_stage_frames(context(), framesPyramid, pwvm->getWvm()->native(pwvm->getLogisticA(), pwvm->getLogisticB()),
                                                       psvm->getSvm()->native(psvm->getLogisticA(), psvm->getLogisticB()), overlapElimination->getDist(),
                                                       overlapElimination->getRatio(), slidingWindowDetector->getStepSizeX(),
                                                       slidingWindowDetector->getStepSizeY(), nullptr, dets.data(), cap, counts.data(), nullptr);
            // FD_ERR_CAPACITY: the output buffer was too small; counts[] holds every frame's count, so ONE retry fits.  (An overflow
            // of a device-side buffer is FD_ERR_DEVICE_CAPACITY: a larger output buffer would not help, no retry.)
            if (rc == FD_ERR_CAPACITY) {
                const int need = *std::max_element(counts.begin(), counts.end());
                if (need > cap) { cap = need; continue; }
            }
            check(rc);
            break;
        }
        for (int k = 0; k < n; ++k)
            for (int q = 0; q < counts[(size_t)k]; ++q) out[i + (size_t)k].push_back(to_patch(dets[(size_t)k * (size_t)cap + (size_t)q]));
        i = j;
    }
    return out;
}
vector<shared_ptr<ClassifiedPatch>> FiveStageSlidingWindowDetector::detect(const Mat& image) { return run(image, nullptr); }
vector<shared_ptr<ClassifiedPatch>> FiveStageSlidingWindowDetector::detect(const Mat& image, const cv::Rect& roi) { return run(image, &roi); }
vector<shared_ptr<ClassifiedPatch>> FiveStageSlidingWindowDetector::detect(shared_ptr<imageprocessing::VersionedImage>) {
    // FiveStageSlidingWindowDetector.cpp:324-329: "not yet implemented for a VersionedImage", returns empty
    return vector<shared_ptr<ClassifiedPatch>>();
}

}  // namespace detection

// =================================================================================================
namespace superviseddescent {

Mat VlHogDescriptorExtractor::getDescriptors(const Mat image, vector<cv::Point2f> locations, int windowSizeHalf) {
    if (image.channels() != 1 || image.depth() != CV_8U)
        throw std::invalid_argument("VlHogDescriptorExtractor: this backend expects the CV_8UC1 (gray) image the callers pass (detect-landmarks.cpp:245)");
    Mat img = contiguous(image);
    const int n = (int)locations.size();
    vector<float> px(n), py(n);
    for (int i = 0; i < n; ++i) { px[i] = locations[i].x; py[i] = locations[i].y; }
    const int variant = hogType == VlHogType::Uoctti ? 1 : 0;
    int len = 0;
    check(fd_sdm_descriptors(context(), img.data, img.cols, img.rows, px.data(), py.data(), n, windowSizeHalf, variant, numCells, cellSize, numBins, nullptr, &len));
    Mat out(n, len, CV_32FC1);
    if (n) check(fd_sdm_descriptors(context(), img.data, img.cols, img.rows, px.data(), py.data(), n, windowSizeHalf, variant, numCells, cellSize, numBins,
                                    out.ptr<float>(0), &len));
    return out;
}
string VlHogDescriptorExtractor::getParameterString() const {
    std::ostringstream s;
    s << "numCells " << numCells << " cellSize " << cellSize << " numBins " << numBins;
    return s.str();
}

SdmLandmarkModel::SdmLandmarkModel(Mat mean, vector<string> ids, vector<Mat> regs, vector<shared_ptr<DescriptorExtractor>> ex, vector<string> types)
    : meanLandmarks(mean), landmarkIdentifier(ids), regressorData(regs), descriptorExtractors(ex), descriptorTypes(types) {}
Mat SdmLandmarkModel::getMeanShape() const {   // SdmLandmarkModel.cpp:53-56: clone().t()
    const int n = meanLandmarks.cols;
    Mat col(n, 1, CV_32FC1);
    for (int i = 0; i < n; ++i) col.at<float>(i, 0) = meanLandmarks.at<float>(0, i);
    return col;
}
vector<cv::Point2f> SdmLandmarkModel::getMeanAsPoints() const {
    vector<cv::Point2f> pts;
    const int L = getNumLandmarks();
    for (int i = 0; i < L; ++i) pts.push_back(cv::Point2f(meanLandmarks.at<float>(0, i), meanLandmarks.at<float>(0, i + L)));
    return pts;
}
cv::Point2f SdmLandmarkModel::getLandmarkAsPoint(string id, Mat inst) const {
    auto it = std::find(landmarkIdentifier.begin(), landmarkIdentifier.end(), id);
    if (it == landmarkIdentifier.end()) throw std::invalid_argument("SdmLandmarkModel: unknown landmark " + id);
    const int index = (int)(it - landmarkIdentifier.begin()), L = getNumLandmarks();
    if (inst.empty()) return cv::Point2f(meanLandmarks.at<float>(0, index), meanLandmarks.at<float>(0, index + L));
    return cv::Point2f(inst.at<float>(index), inst.at<float>(index + L));
}
void SdmLandmarkModel::save(string filename, string comment) {   // SdmLandmarkModel.cpp:98-128
    std::ofstream file(filename.c_str());
    file << "# " << comment << std::endl;
    file << "numLandmarks " << getNumLandmarks() << std::endl;
    for (const auto& id : landmarkIdentifier) file << id << std::endl;
    file << std::setprecision(9);
    for (int i = 0; i < 2 * getNumLandmarks(); ++i) file << meanLandmarks.at<float>(0, i) << std::endl;
    file << "numCascadeSteps " << getNumCascadeSteps() << std::endl;
    for (int s = 0; s < getNumCascadeSteps(); ++s) {
        const Mat& R = regressorData[s];
        file << "cascadeStep " << s << " rows " << R.rows << " cols " << R.cols << std::endl;
        file << "descriptorType " << descriptorTypes[s] << std::endl;
        file << "descriptorPostprocessing none" << std::endl;
        file << "descriptorParameters " << descriptorExtractors[s]->getParameterString() << std::endl;
        for (int r = 0; r < R.rows; ++r) {
            for (int c = 0; c < R.cols; ++c) file << R.at<float>(r, c) << " ";
            file << std::endl;
        }
    }
}
static vector<string> split_ws(const string& line) {
    vector<string> out;
    std::istringstream ss(line);
    string t;
    while (std::getline(ss, t, ' ')) out.push_back(t);
    return out;
}
static void chomp(string& s) { while (!s.empty() && s.back() == '\r') s.pop_back(); }
SdmLandmarkModel SdmLandmarkModel::load(string filename) {   // SdmLandmarkModel.cpp:130-233
    SdmLandmarkModel model;
    std::ifstream file(filename.c_str());
    if (!file.is_open()) throw std::runtime_error("Given SDM model file could not be opened: " + filename);
    string line;
    std::getline(file, line);   // description
    std::getline(file, line); chomp(line);
    const int L = std::stoi(split_ws(line).at(1));
    for (int i = 0; i < L; ++i) { std::getline(file, line); chomp(line); model.landmarkIdentifier.push_back(line); }
    model.meanLandmarks = Mat(1, 2 * L, CV_32FC1);
    for (int i = 0; i < 2 * L; ++i) { std::getline(file, line); chomp(line); model.meanLandmarks.at<float>(0, i) = std::stof(line); }
    std::getline(file, line); chomp(line);
    const int S = std::stoi(split_ws(line).at(1));
    for (int s = 0; s < S; ++s) {
        std::getline(file, line); chomp(line);
        auto hdr = split_ws(line);
        const int rows = std::stoi(hdr.at(3)), cols = std::stoi(hdr.at(5));
        std::getline(file, line); chomp(line);
        const string type = split_ws(line).at(1);
        std::getline(file, line);   // descriptorPostprocessing
        std::getline(file, line); chomp(line);
        auto par = split_ws(line);
        if (type == "vlhog-dt") {
            if (par.size() != 7) throw std::logic_error("descriptorParameters must contain numCells, cellSize and numBins.");
            model.descriptorExtractors.push_back(make_shared<VlHogDescriptorExtractor>(VlHogDescriptorExtractor::VlHogType::DalalTriggs, std::stoi(par[2]),
                                                                                       std::stoi(par[4]), std::stoi(par[6])));
        } else if (type == "vlhog-uoctti") {
            if (par.size() <= 2) model.descriptorExtractors.push_back(make_shared<VlHogDescriptorExtractor>(VlHogDescriptorExtractor::VlHogType::Uoctti));
            else if (par.size() == 7)
                model.descriptorExtractors.push_back(make_shared<VlHogDescriptorExtractor>(VlHogDescriptorExtractor::VlHogType::Uoctti, std::stoi(par[2]),
                                                                                           std::stoi(par[4]), std::stoi(par[6])));
            else throw std::logic_error("descriptorParameters must either be empty (=face-size adaptive parameters) or contain numCells, cellSize and numBins.");
        } else {
            throw std::logic_error("descriptorType does not match 'vlhog-dt' or 'vlhog-uoctti' (OpenCVSift is not available on this backend).");
        }
        model.descriptorTypes.push_back(type);
        Mat R(rows, cols, CV_32FC1);
        for (int r = 0; r < rows; ++r) {
            std::getline(file, line);
            std::istringstream ss(line);
            for (int c = 0; c < cols; ++c) ss >> R.at<float>(r, c);
        }
        model.regressorData.push_back(R);
    }
    return model;
}

SdmLandmarkModelFitting::SdmLandmarkModelFitting(SdmLandmarkModel m, bool adaptive) : model(m), handle(nullptr) {
    const int L = model.getNumLandmarks(), S = model.getNumCascadeSteps();
    if (S == 0) return;
    Mat mean = model.getMeanShape();
    vector<float> meanv(2 * L);
    for (int i = 0; i < 2 * L; ++i) meanv[i] = mean.at<float>(i, 0);
    vector<Mat> regs;
    vector<const float*> R;
    vector<int32_t> rows;
    for (int s = 0; s < S; ++s) { regs.push_back(contiguous(model.getRegressorData(s))); R.push_back(regs.back().ptr<float>(0)); rows.push_back(regs.back().rows); }
    auto vl = std::dynamic_pointer_cast<VlHogDescriptorExtractor>(model.getDescriptorExtractor(0));
    if (!vl) throw std::logic_error("SdmLandmarkModelFitting: only VlHog descriptors are available on this backend");
    fd_sdm_model md = {};
    md.num_landmarks = L; md.num_steps = S; md.mean = meanv.data(); md.R = R.data(); md.R_rows = rows.data();
    md.hog_variant = vl->getType() == VlHogDescriptorExtractor::VlHogType::Uoctti ? 1 : 0;
    vector<int32_t> dp;
    if (!adaptive) {   // SdmLandmarkModel.hpp:236-238: "non-adaptive, the descriptorExtractor has all necessary params"
        for (int s = 0; s < S; ++s) {
            auto e = std::dynamic_pointer_cast<VlHogDescriptorExtractor>(model.getDescriptorExtractor(s));
            if (!e || e->getType() != vl->getType()) throw std::logic_error("SdmLandmarkModelFitting: the cascade steps must share one VlHog type");
            dp.push_back(e->getNumCells()); dp.push_back(e->getCellSize()); dp.push_back(e->getNumBins());
        }
        md.desc_params = dp.data();
    }
    check(fd_sdm_create(context(), &md, &handle));
}
SdmLandmarkModelFitting::~SdmLandmarkModelFitting() { fd_sdm_destroy(handle); }
Mat SdmLandmarkModelFitting::alignRigid(Mat modelShape, cv::Rect faceBox) const {   // SdmLandmarkModel.hpp:156-192
    if (modelShape.cols != 1) throw std::runtime_error("The supplied model shape does not have one column (i.e. it doesn't seem to be a column-vector).");
    const int L = modelShape.rows / 2;
    // cv::MatExpr "(x + 0.5f) * w + bx" evaluates as x * float(w) + float(0.5 * w + bx) (convertTo with alpha/beta)
    const float ax = (float)(double)faceBox.width, bx = (float)(0.5 * faceBox.width + faceBox.x);
    const float ay = (float)(double)faceBox.height, by = (float)(0.5 * faceBox.height + faceBox.y);
    for (int i = 0; i < L; ++i) {
        modelShape.at<float>(i, 0) = modelShape.at<float>(i, 0) * ax + bx;
        modelShape.at<float>(i + L, 0) = modelShape.at<float>(i + L, 0) * ay + by;
    }
    return modelShape;
}
vector<Mat> SdmLandmarkModelFitting::optimize(const vector<Mat>& shapes, const vector<Mat>& images) {
    if (!handle) throw std::logic_error("SdmLandmarkModelFitting: model has no cascade steps");
    const int B = (int)images.size(), L = model.getNumLandmarks();
    if (B == 0 || (int)shapes.size() != B) throw std::invalid_argument("SdmLandmarkModelFitting: need one shape per image");
    const int W = images[0].cols, H = images[0].rows;
    vector<unsigned char> stack((size_t)B * W * H);
    vector<float> sh((size_t)B * 2 * L);
    for (int b = 0; b < B; ++b) {
        if (images[b].cols != W || images[b].rows != H || images[b].type() != CV_8UC1)
            throw std::invalid_argument("SdmLandmarkModelFitting: images of a batch must be CV_8UC1 and of equal size");
        Mat im = contiguous(images[b]);
        std::memcpy(stack.data() + (size_t)b * W * H, im.data, (size_t)W * H);
        for (int i = 0; i < 2 * L; ++i) sh[(size_t)b * 2 * L + i] = shapes[b].at<float>(i, 0);
    }
    vector<int32_t> status(B);
    check(fd_sdm_optimize_batch(context(), handle, stack.data(), W, H, B, 0, sh.data(), status.data()));
    vector<Mat> out;
    for (int b = 0; b < B; ++b) {
        if (status[b]) throw std::runtime_error("VlHogDescriptorExtractor: patch window leaves the zero-extended image (cv::Mat roi assertion in the reference)");
        Mat s(2 * L, 1, CV_32FC1);
        for (int i = 0; i < 2 * L; ++i) s.at<float>(i, 0) = sh[(size_t)b * 2 * L + i];
        out.push_back(s);
    }
    return out;
}
Mat SdmLandmarkModelFitting::optimize(Mat modelShape, Mat image) {
    return optimize(vector<Mat>{modelShape}, vector<Mat>{image})[0];
}

}  // namespace superviseddescent

// =================================================================================================
#include <functional>
#include <limits>
#include <typeinfo>
#include <unordered_map>
#include "condensation/condensation_all.hpp"
namespace condensation {

double Sample::aspectRatio = 1;

// the samples as the C ABI takes them: {x, y, width, height} each (Sample::getX / getY / getWidth / getHeight)
static vector<int32_t> pack_samples(const vector<shared_ptr<Sample>>& samples) {
    vector<int32_t> xywh;
    xywh.reserve(4 * samples.size());
    for (const auto& s : samples) xywh.insert(xywh.end(), {s->getX(), s->getY(), s->getWidth(), s->getHeight()});
    return xywh;
}
// what an fd_*_evaluate_samples call returned, back into the samples
static void unpack_samples(const vector<uint8_t>& target, const vector<double>& weight, vector<shared_ptr<Sample>>& samples) {
    for (size_t i = 0; i < samples.size(); ++i) {
        samples[i]->setTarget(target[i] != 0);
        samples[i]->setWeight(weight[i]);
    }
}

WvmSvmModel::WvmSvmModel(shared_ptr<imageprocessing::FeatureExtractor> featureExtractor, shared_ptr<classification::ProbabilisticWvmClassifier> wvm,
                         shared_ptr<classification::ProbabilisticSvmClassifier> svm)
    : featureExtractor(featureExtractor), wvm(wvm), svm(svm) {}
void WvmSvmModel::update(shared_ptr<imageprocessing::VersionedImage> image) { featureExtractor->update(image); }
static imageprocessing::DirectPyramidFeatureExtractor* fused_extractor(const shared_ptr<imageprocessing::FeatureExtractor>& fe) {
    auto* d = dynamic_cast<imageprocessing::DirectPyramidFeatureExtractor*>(fe.get());
    if (!d || !d->hasHistEq64())
        throw std::logic_error("WvmSvmModel: this backend needs a DirectPyramidFeatureExtractor with a HistEq64Filter patch filter");
    return d;
}
void WvmSvmModel::evaluate(Sample& sample) const {   // WvmSvmModel.cpp:44-67 (single sample: no top-8 selection)
    ++loopEvaluations;
    auto patch = featureExtractor->extract(sample.getX(), sample.getY(), sample.getWidth(), sample.getHeight());
    if (!patch) {
        sample.setTarget(false);
        sample.setWeight(0);
        return;
    }
    auto wvmResult = wvm->getProbability(patch->getData());
    if (wvmResult.first) {
        auto svmResult = svm->getProbability(patch->getData());
        sample.setTarget(svmResult.first);
        sample.setWeight(wvmResult.second * svmResult.second);
    } else {
        sample.setTarget(false);
        sample.setWeight(0.5 * wvmResult.second);
    }
}
void WvmSvmModel::evaluate(shared_ptr<imageprocessing::VersionedImage> image, vector<shared_ptr<Sample>>& samples) {   // :69-118
    update(image);
    auto* direct = fused_extractor(featureExtractor);
    ++fusedEvaluations;
    const int n = (int)samples.size();
    if (n == 0) return;
    const vector<int32_t> xywh = pack_samples(samples);
    vector<uint8_t> target((size_t)n);
    vector<double> weight((size_t)n);
    check(fd_wvm_svm_evaluate_samples(context(), direct->getPyramid()->native(), wvm->getWvm()->native(wvm->getLogisticA(), wvm->getLogisticB()),
                                      svm->getSvm()->native(svm->getLogisticA(), svm->getLogisticB()), n, xywh.data(), target.data(), weight.data()));
    unpack_samples(target, weight, samples);
}

// SingleClassifierModel.cpp:22-63
SingleClassifierModel::SingleClassifierModel(shared_ptr<imageprocessing::FeatureExtractor> featureExtractor, shared_ptr<classification::ProbabilisticClassifier> classifier)
    : featureExtractor(featureExtractor), classifier(classifier) {}
void SingleClassifierModel::update(shared_ptr<imageprocessing::VersionedImage> image) { featureExtractor->update(image); }
void SingleClassifierModel::evaluate(Sample& sample) const {
    auto patch = featureExtractor->extract(sample.getX(), sample.getY(), sample.getWidth(), sample.getHeight());
    if (patch) {
        std::pair<bool, double> result = classifier->getProbability(patch->getData());
        sample.setTarget(result.first);
        sample.setWeight(result.second);
    } else {
        sample.setTarget(false);
        sample.setWeight(0);
    }
}
SampledClassifier sampledClassifierOf(classification::ProbabilisticClassifier* classifier) {
    auto* psvm = dynamic_cast<classification::ProbabilisticSvmClassifier*>(classifier);
    if (!psvm)
        if (auto* trainable = dynamic_cast<classification::TrainableProbabilisticSvmClassifier*>(classifier)) psvm = trainable->getProbabilisticSvm().get();
    return SampledClassifier{detection::hasF32SupportVectors(psvm) ? psvm : nullptr, dynamic_cast<classification::ProbabilisticRvmClassifier*>(classifier)};
}
SampledRoute sampledRoute(const imageprocessing::SampledChain& chain, const SampledClassifier& classifier) {
    if (chain.kind == imageprocessing::SampledChain::Kind::None) return SampledRoute::Loop;
    if (classifier.svm) return SampledRoute::Svm;
    return chain.kind == imageprocessing::SampledChain::Kind::Patch && classifier.rvm ? SampledRoute::PatchRvm : SampledRoute::Loop;
}
void SingleClassifierModel::evaluate(shared_ptr<imageprocessing::VersionedImage> image, vector<shared_ptr<Sample>>& samples) {
    update(image);
    const imageprocessing::SampledChain chain = imageprocessing::sampledChainOf(featureExtractor.get());
    const SampledClassifier scorer = sampledClassifierOf(classifier.get());
    const SampledRoute route = chain.ready() ? sampledRoute(chain, scorer) : SampledRoute::Loop;
    if (route == SampledRoute::Loop) {   // MeasurementModel.hpp: the per-sample loop
        ++loopEvaluations;
        for (shared_ptr<Sample> sample : samples) evaluate(*sample);
        return;
    }
    ++fusedEvaluations;
    const int n = (int)samples.size();
    if (n == 0) return;
    const vector<int32_t> xywh = pack_samples(samples);
    vector<uint8_t> target((size_t)n);
    vector<double> weight((size_t)n);
    if (route == SampledRoute::PatchRvm) {   // level and distance from the device, verdict and probability by the classifier's own getProbability
        vector<uint8_t> valid((size_t)n);
        vector<int32_t> level((size_t)n);
        vector<double> distance((size_t)n);
        check(fd_patch_rvm_evaluate_samples(context(), chain.pyramid->getPyramid()->native(), &chain.patch, scorer.rvm->getRvm()->distanceModel(), n, xywh.data(),
                                            valid.data(), level.data(), distance.data(), nullptr));
        for (int i = 0; i < n; ++i) {
            const std::pair<bool, double> result = valid[i] ? scorer.rvm->getProbability(std::make_pair((int)level[i], distance[i])) : std::make_pair(false, 0.0);
            target[i] = result.first ? 1 : 0;
            weight[i] = result.second;
        }
    } else {
        chain.svmEvaluate(scorer.svm->getSvm()->native(scorer.svm->getLogisticA(), scorer.svm->getLogisticB()), xywh, target.data(), weight.data());
    }
    unpack_samples(target, weight, samples);
}

// the integral kind, its parameters and the SVM of a resident evaluation; false where the combination has none
static bool resident_integral(const imageprocessing::SampledChain& chain, const SampledClassifier& scorer, bool needSvm = true) {
    using Kind = imageprocessing::SampledChain::Kind;
    return (chain.kind == Kind::Haar || chain.kind == Kind::Surf || chain.kind == Kind::IntegralHog) && (scorer.svm || !needSvm) &&
           chain.wrappers.sampleMaps().size() <= (size_t)FD_SAMPLE_MAPS_MAX && chain.ready();
}
// the window list of a resident set can be resolved on this pyramid for patches of this width: it holds an image, has no more layers than
// the window table, and its width -> layer table fits (fd_sample_layer_table)
static bool resident_layer_table(const fd_pyramid* native, int patchWidth) {
    const int layers = native ? fd_pyramid_layer_count(native) : 0;
    if (layers < 1 || layers > 64) return false;
    int first = 0, lw, lh, ch, length = 0;
    double scale;
    fd_pyramid_layer_info(native, 0, &first, &scale, &lw, &lh, &ch);
    const int rc = fd_sample_layer_table(layers, first, fd_pyramid_incremental_scale(native), patchWidth, 0, nullptr, &length);
    return (rc == FD_OK || rc == FD_ERR_CAPACITY) && length <= FD_SAMPLE_TABLE_MAX;
}
// fd_particles_evaluate_pyramid serves the chain: a pyramid kind with an f32 SVM behind at most FD_SAMPLE_MAPS_MAX wrappers, all of them
// PatchResizingFeatureExtractors, on a pyramid that holds an image, has no more layers than the window table and whose width -> layer
// table fits (fd_sample_layer_table)
static bool resident_pyramid(const imageprocessing::SampledChain& chain, const SampledClassifier& scorer, bool needSvm = true) {
    if (!chain.onPyramid() || (!scorer.svm && needSvm) || !chain.ready()) return false;
    const vector<fd_sample_map>& maps = chain.wrappers.sampleMaps();
    if (maps.size() > (size_t)FD_SAMPLE_MAPS_MAX) return false;
    for (const fd_sample_map& m : maps)
        if (m.kind != FD_SAMPLE_MAP_RESIZE) return false;
    const int patchWidth = chain.kind == imageprocessing::SampledChain::Kind::Patch ? chain.patch.patch_w
                           : (chain.kind == imageprocessing::SampledChain::Kind::Ehog ? chain.ehog.patch_w : chain.hist.patch_w);
    return resident_layer_table(chain.pyramid->getPyramid()->native(), patchWidth);
}
// The device maps every sample through the wrappers first (fd_particle_sample), so a pyramid chain behind wrappers resolves too
SingleClassifierModel::ResidentPlan SingleClassifierModel::residentPlan() const {
    ResidentPlan plan{ResidentPlan::Family::None, imageprocessing::sampledChainOf(featureExtractor.get(), /*mapsApplied=*/true), sampledClassifierOf(classifier.get())};
    if (resident_integral(plan.chain, plan.scorer)) plan.family = ResidentPlan::Family::Integral;
    else if (resident_pyramid(plan.chain, plan.scorer)) plan.family = ResidentPlan::Family::Pyramid;
    return plan;
}
// while the model is not usable nothing is scored with its classifier: the plan then asks for the extraction alone
SingleClassifierModel::ResidentPlan SelfLearningMeasurementModel::residentPlan() const {
    SingleClassifierModel::ResidentPlan plan = model.residentPlan();
    if (plan.family == SingleClassifierModel::ResidentPlan::Family::None && !usable) {
        if (resident_integral(plan.chain, plan.scorer, false)) plan.family = SingleClassifierModel::ResidentPlan::Family::Integral;
        else if (resident_pyramid(plan.chain, plan.scorer, false)) plan.family = SingleClassifierModel::ResidentPlan::Family::Pyramid;
    }
    return plan;
}
void SingleClassifierModel::evaluateResident(shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles) {
    update(image);
    const ResidentPlan plan = residentPlan();   // after the update: the plan of the frame loop is from before it
    if (plan.family == ResidentPlan::Family::None) throw std::logic_error("SingleClassifierModel: no resident evaluation for this extractor and classifier");
    ++fusedEvaluations;
    const imageprocessing::SampledChain::DeviceCall call = plan.chain.deviceCall();
    const vector<fd_sample_map>& maps = plan.maps();
    const double a = plan.scorer.svm->getLogisticA(), b = plan.scorer.svm->getLogisticB();
    const fd_svm* svm = plan.scorer.svm->getSvm()->native(a, b);
    if (call.onPyramid)
        check(fd_particles_evaluate_pyramid(context(), particles, call.pyramid, call.kind, call.params(), svm, Sample::getAspectRatio(), maps.data(), (int)maps.size()));
    else
        check(fd_particles_evaluate_integral(context(), particles, call.integral, call.kind, call.params(), svm, Sample::getAspectRatio(), maps.data(), (int)maps.size()));
    // SvmClassifier::classify compares with the threshold the device model holds as a float (fd_samples_svm_tail does the same)
    check(fd_particles_weigh_classifier(context(), particles, a, b, (double)(float)plan.scorer.svm->getSvm()->getThreshold()));
}

// WvmSvmModel on a resident set.  The wrappers are walked here: the device maps every sample through them before the layer rule
bool WvmSvmModel::residentPossible() const {
    const imageprocessing::ExtractorWrappers wrappers(featureExtractor.get());
    auto* direct = dynamic_cast<const imageprocessing::DirectPyramidFeatureExtractor*>(wrappers.inner());
    if (!direct || !direct->hasHistEq64() || wrappers.sampleMaps().size() > (size_t)FD_SAMPLE_MAPS_MAX) return false;
    for (const fd_sample_map& m : wrappers.sampleMaps())
        if (m.kind != FD_SAMPLE_MAP_RESIZE) return false;
    if (direct->getPyramid()->getLayerFilterKind() != FD_LAYER_NONE || direct->getPyramid()->getSourcePyramid()) return false;
    return resident_layer_table(direct->getPyramid()->native(), direct->getPatchWidth());
}
void WvmSvmModel::evaluateResident(shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles) {
    update(image);
    if (!residentPossible()) throw std::logic_error("WvmSvmModel: no resident evaluation for this extractor");
    ++fusedEvaluations;
    const imageprocessing::ExtractorWrappers wrappers(featureExtractor.get());
    auto* direct = static_cast<const imageprocessing::DirectPyramidFeatureExtractor*>(wrappers.inner());
    const vector<fd_sample_map>& maps = wrappers.sampleMaps();
    const fd_wvm* nativeWvm = wvm->getWvm()->native(wvm->getLogisticA(), wvm->getLogisticB());
    const fd_svm* nativeSvm = svm->getSvm()->native(svm->getLogisticA(), svm->getLogisticB());
    check(fd_particles_evaluate_wvm_svm(context(), particles, direct->getPyramid()->native(), nativeWvm, nativeSvm, Sample::getAspectRatio(), maps.data(),
                                        (int)maps.size()));
    check(fd_particles_weigh_wvm_svm(context(), particles, nativeWvm, nativeSvm));
}

// ---- FilteringClassifierModel (FilteringClassifierModel.cpp:27-103) --------------------------------------------------------------------
// the RVM behind a binary classifier that is an RvmClassifier or a ProbabilisticRvmClassifier; null: another classifier
static const classification::RvmClassifier* rvm_of(const classification::BinaryClassifier* c) {
    if (auto* rvm = dynamic_cast<const classification::RvmClassifier*>(c)) return rvm;
    if (auto* prvm = dynamic_cast<const classification::ProbabilisticRvmClassifier*>(c)) return prvm->getRvm().get();
    return nullptr;
}
// classifier->classify on the patch of every sample {x, y, width, height} in one fd_patch_rvm_evaluate_samples: possible with an RVM on
// a DirectPyramidFeatureExtractor (itself) with a sampled gray-patch chain; the verdict is the RvmClassifier's own classify(level,
// distance), false for a sample without a patch.  false: not this combination, nothing was done
static bool rvm_classify_samples(const imageprocessing::FeatureExtractor* extractor, const classification::BinaryClassifier* classifier,
                                 const vector<int32_t>& xywh, vector<char>& verdict) {
    const classification::RvmClassifier* rvm = rvm_of(classifier);
    const imageprocessing::SampledChain chain = imageprocessing::sampledChainOf(extractor);
    if (!rvm || chain.kind != imageprocessing::SampledChain::Kind::Patch) return false;
    const int n = (int)(xywh.size() / 4);
    verdict.assign((size_t)n, 0);
    if (n == 0) return true;
    vector<uint8_t> valid((size_t)n);
    vector<int32_t> level((size_t)n);
    vector<double> distance((size_t)n);
    check(fd_patch_rvm_evaluate_samples(context(), chain.pyramid->getPyramid()->native(), &chain.patch, rvm->distanceModel(), n, xywh.data(), valid.data(),
                                        level.data(), distance.data(), nullptr));
    for (int i = 0; i < n; ++i) verdict[i] = valid[i] && rvm->classify(std::make_pair((int)level[i], distance[i])) ? 1 : 0;
    return true;
}

FilteringClassifierModel::FilteringClassifierModel(shared_ptr<imageprocessing::FeatureExtractor> filterFeatureExtractor, shared_ptr<classification::BinaryClassifier> filter,
                                                   shared_ptr<imageprocessing::FeatureExtractor> featureExtractor,
                                                   shared_ptr<classification::ProbabilisticClassifier> classifier, Behavior behavior)
    : FilteringClassifierModel(filterFeatureExtractor, filter, make_shared<SingleClassifierModel>(featureExtractor, classifier), behavior) {}
FilteringClassifierModel::FilteringClassifierModel(shared_ptr<imageprocessing::FeatureExtractor> filterFeatureExtractor, shared_ptr<classification::BinaryClassifier> filter,
                                                   shared_ptr<MeasurementModel> measurementModel, Behavior behavior)
    : behavior(behavior), measurementModel(measurementModel), featureExtractor(filterFeatureExtractor), filter(filter) {}
void FilteringClassifierModel::update(shared_ptr<imageprocessing::VersionedImage> image) {
    featureExtractor->update(image);
    measurementModel->update(image);
}
bool FilteringClassifierModel::passesFilter(const Sample& sample) const {
    auto patch = featureExtractor->extract(sample.getX(), sample.getY(), sample.getWidth(), sample.getHeight());
    return patch && filter->classify(patch->getData());
}
bool FilteringClassifierModel::passFilter(const vector<shared_ptr<Sample>>& samples, vector<char>& passes) const {
    if (rvm_classify_samples(featureExtractor.get(), filter.get(), pack_samples(samples), passes)) return true;
    passes.assign(samples.size(), 0);
    for (size_t i = 0; i < samples.size(); ++i) passes[i] = passesFilter(*samples[i]) ? 1 : 0;
    return false;
}
void FilteringClassifierModel::evaluate(Sample& sample) const {
    if (behavior == Behavior::RESET_WEIGHT) {
        if (passesFilter(sample)) {
            measurementModel->evaluate(sample);
        } else {
            sample.setTarget(false);
            sample.setWeight(0);
        }
    } else {
        measurementModel->evaluate(sample);
        if (sample.isTarget() && !passesFilter(sample)) sample.setTarget(false);
    }
}
void FilteringClassifierModel::evaluate(shared_ptr<imageprocessing::VersionedImage> image, vector<shared_ptr<Sample>>& samples) {
    vector<char> passes;
    vector<shared_ptr<Sample>> asked;
    if (behavior == Behavior::RESET_WEIGHT) {   // the filter on every sample, the model on those that pass
        featureExtractor->update(image);
        (passFilter(samples, passes) ? fusedFilters : loopFilters)++;
        for (size_t i = 0; i < samples.size(); ++i) {
            if (passes[i]) {
                asked.push_back(samples[i]);
            } else {
                samples[i]->setTarget(false);
                samples[i]->setWeight(0);
            }
        }
        measurementModel->evaluate(image, asked);   // (updates the model on the image, as update() does)
    } else {   // the model on every sample, the filter on those it marked as target
        featureExtractor->update(image);
        measurementModel->evaluate(image, samples);
        for (const auto& sample : samples)
            if (sample->isTarget()) asked.push_back(sample);
        (passFilter(asked, passes) ? fusedFilters : loopFilters)++;
        for (size_t i = 0; i < asked.size(); ++i)
            if (!passes[i]) asked[i]->setTarget(false);
    }
}

// ---- ClassificationBasedStateValidator (ClassificationBasedStateValidator.cpp:28-45) ---------------------------------------------------
ClassificationBasedStateValidator::ClassificationBasedStateValidator(shared_ptr<imageprocessing::FeatureExtractor> extractor,
                                                                     shared_ptr<classification::BinaryClassifier> classifier, vector<double> sizes,
                                                                     vector<double> displacements)
    : extractor(extractor), classifier(classifier), sizes(sizes), displacements(displacements) {}
bool ClassificationBasedStateValidator::isValid(const Sample& target, const vector<shared_ptr<Sample>>&, shared_ptr<imageprocessing::VersionedImage> image) {
    extractor->update(image);
    lastCandidates.clear();
    vector<int32_t> xywh;
    for (double factor : sizes) {
        const int size = static_cast<int>(std::round(factor * target.getSize()));
        for (double dx : displacements) {
            const int x = target.getX() + static_cast<int>(std::round(dx * size));
            for (double dy : displacements) {
                const int y = target.getY() + static_cast<int>(std::round(dy * size));
                const Sample candidate(x, y, size);
                lastCandidates.push_back(cv::Rect(x, y, size, size));
                xywh.insert(xywh.end(), {candidate.getX(), candidate.getY(), candidate.getWidth(), candidate.getHeight()});
            }
        }
    }
    vector<char> accepted;
    if (rvm_classify_samples(extractor.get(), classifier.get(), xywh, accepted)) {
        ++fusedValidations;
        return std::find(accepted.begin(), accepted.end(), (char)1) != accepted.end();
    }
    ++loopValidations;
    for (size_t i = 0; i < lastCandidates.size(); ++i) {
        auto patch = extractor->extract(xywh[4 * i], xywh[4 * i + 1], xywh[4 * i + 2], xywh[4 * i + 3]);
        if (patch && classifier->classify(patch->getData())) return true;
    }
    return false;
}

// ---- PositionDependentMeasurementModel (PositionDependentMeasurementModel.cpp:28-274) --------------------------------------------------
PositionDependentMeasurementModel::PositionDependentMeasurementModel(shared_ptr<imageprocessing::FeatureExtractor> featureExtractor,
                                                                     shared_ptr<classification::TrainableProbabilisticClassifier> classifier, unsigned int seed)
    : PositionDependentMeasurementModel(make_shared<SingleClassifierModel>(featureExtractor, classifier), featureExtractor, classifier, seed) {}
PositionDependentMeasurementModel::PositionDependentMeasurementModel(shared_ptr<MeasurementModel> measurementModel,
                                                                     shared_ptr<imageprocessing::FeatureExtractor> featureExtractor,
                                                                     shared_ptr<classification::TrainableProbabilisticClassifier> classifier, unsigned int seed)
    : generator(seed), measurementModel(measurementModel), featureExtractor(featureExtractor), classifier(classifier), usable(false), frameCount(0),
      startFrameCount(3), stopFrameCount(0), targetThreshold(0.7f), confidenceThreshold(0.95f), positiveOffsetFactor(0.05f), negativeOffsetFactor(0.5f),
      sampleNegativesAroundTarget(0), sampleAdditionalNegatives(10), sampleTestNegatives(10), exploitSymmetry(false) {}
SelfLearningMeasurementModel::SelfLearningMeasurementModel(shared_ptr<imageprocessing::FeatureExtractor> featureExtractor,
                                                           shared_ptr<classification::TrainableProbabilisticClassifier> classifier, double positiveThreshold,
                                                           double negativeThreshold)
    : model(featureExtractor, classifier), featureExtractor(featureExtractor), classifier(classifier), positiveThreshold(positiveThreshold),
      negativeThreshold(negativeThreshold) {
    if (!(negativeThreshold <= positiveThreshold) || !std::isfinite(positiveThreshold) || !std::isfinite(negativeThreshold))
        throw std::invalid_argument("SelfLearningMeasurementModel: the thresholds must be finite and negativeThreshold <= positiveThreshold");
}
void SelfLearningMeasurementModel::reset() {   // .cpp:76-79
    classifier->reset();
    usable = false;
}
fd_particles_examples_params SelfLearningMeasurementModel::examplesParams() const {
    fd_particles_examples_params p;
    p.positive_threshold = positiveThreshold; p.negative_threshold = negativeThreshold; p.max_count = 10; p.require_window = usable ? 1 : 0;
    return p;
}
// .cpp:89-125 with the choice made by the library's rule; the patches of the chosen samples become the rows adaptResident takes
bool SelfLearningMeasurementModel::adapt(shared_ptr<imageprocessing::VersionedImage> image, const vector<shared_ptr<Sample>>& samples) {
    const int n = (int)samples.size();
    const fd_particles_examples_params params = examplesParams();
    if (!usable) featureExtractor->update(image);   // :119; a usable model was evaluated on this image already
    vector<double> weight((size_t)n);
    vector<uint8_t> valid((size_t)n, 1);
    vector<shared_ptr<imageprocessing::Patch>> patches((size_t)n);
    auto patchOf = [&](int i) {
        const Sample& s = *samples[i];
        if (!patches[i]) patches[i] = featureExtractor->extract(s.getX(), s.getY(), s.getWidth(), s.getHeight());
        return patches[i];
    };
    for (int i = 0; i < n; ++i) {
        weight[i] = samples[i]->getWeight();
        // only a sample with a patch entered evaluate's lists (:68-71); a positive weight tells that it had one
        if (usable) valid[i] = weight[i] > 0 || patchOf(i) ? 1 : 0;
    }
    int32_t positive[FD_PARTICLES_EXAMPLES_MAX], negative[FD_PARTICLES_EXAMPLES_MAX];
    int nPositive = 0, nNegative = 0;
    check(fd_particles_examples_select(n, weight.data(), valid.data(), &params, &nPositive, positive, &nNegative, negative));
    lastPositives.clear(); lastNegatives.clear(); lastRows.clear();
    lastRowLength = 0;
    auto take = [&](const int32_t* chosen, int count, vector<fd_particles_example>& records) {
        for (int k = 0; k < count; ++k) {
            const int i = chosen[k];
            const Sample& s = *samples[i];
            const shared_ptr<imageprocessing::Patch> patch = patchOf(i);
            fd_particles_example r{};
            r.index = i; r.x = s.getX(); r.y = s.getY(); r.size = s.getSize(); r.valid = patch ? 1 : 0; r.weight = weight[i];
            records.push_back(r);
            if (!patch) continue;
            const Mat& data = patch->getData();
            if (data.depth() != CV_32F) throw std::invalid_argument("SelfLearningMeasurementModel: the feature vectors must be CV_32F");
            const int perRow = data.cols * data.channels();
            lastRowLength = data.rows * perRow;
            for (int y = 0; y < data.rows; ++y) lastRows.insert(lastRows.end(), data.ptr<float>(y), data.ptr<float>(y) + perRow);
        }
    };
    take(positive, nPositive, lastPositives);
    take(negative, nNegative, lastNegatives);
    return adaptResident(image, lastPositives, lastNegatives, lastRows);
}
// rows: one row of the feature length per valid record, the positives' first, in list order
bool SelfLearningMeasurementModel::adaptResident(shared_ptr<imageprocessing::VersionedImage>, const vector<fd_particles_example>& positives,
                                                 const vector<fd_particles_example>& negatives, const vector<float>& rows) {
    size_t validCount = 0;
    for (const fd_particles_example& r : positives) validCount += r.valid ? 1 : 0;
    for (const fd_particles_example& r : negatives) validCount += r.valid ? 1 : 0;
    const size_t length = validCount ? rows.size() / validCount : 0;
    size_t next = 0;
    auto vectors = [&](const vector<fd_particles_example>& records) {
        vector<Mat> out;
        for (const fd_particles_example& r : records)
            if (r.valid) out.push_back(Mat(1, (int)length, CV_32F, const_cast<float*>(rows.data() + length * next++)).clone());
        return out;
    };
    const vector<Mat> positiveExamples = vectors(positives), negativeExamples = vectors(negatives);
    usable = classifier->retrain(positiveExamples, negativeExamples);
    return true;
}
void SelfLearningMeasurementModel::readExamples(shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles, fd_particles_info& info) {
    featureExtractor->update(image);   // the bootstrap branch's update (:119); after evaluateResident it changes nothing
    const SingleClassifierModel::ResidentPlan plan = residentPlan();
    if (plan.family == SingleClassifierModel::ResidentPlan::Family::None)
        throw std::logic_error("SelfLearningMeasurementModel: no resident extraction for this extractor and classifier");
    const imageprocessing::SampledChain::DeviceCall call = plan.chain.deviceCall();
    const vector<fd_sample_map>& maps = plan.maps();
    const fd_particles_examples_params params = examplesParams();
    int channels = 1, length = 0, capacity = 0;
    if (call.onPyramid) {
        int first, lw, lh;
        double scale;
        fd_pyramid_layer_info(call.pyramid, 0, &first, &scale, &lw, &lh, &channels);
    }
    check(fd_particles_examples_bounds(call.onPyramid ? FD_EXAMPLES_PYRAMID : FD_EXAMPLES_INTEGRAL, call.kind, call.params(), channels, params.max_count, &length,
                                       &capacity));
    fd_particles_example positives[FD_PARTICLES_EXAMPLES_MAX], negatives[FD_PARTICLES_EXAMPLES_MAX];
    int nPositive = 0, nNegative = 0, rowLength = 0;
    vector<float> all((size_t)capacity + 1);
    if (call.onPyramid)
        check(fd_particles_state_examples_pyramid(context(), particles, nullptr, call.pyramid, call.kind, call.params(), Sample::getAspectRatio(), maps.data(),
                                                  (int)maps.size(), &params, &info, nullptr, &nPositive, positives, &nNegative, negatives, all.data(),
                                                  capacity, &rowLength));
    else
        check(fd_particles_state_examples_integral(context(), particles, nullptr, call.integral, call.kind, call.params(), Sample::getAspectRatio(), maps.data(),
                                                   (int)maps.size(), &params, &info, nullptr, &nPositive, positives, &nNegative, negatives, all.data(),
                                                   capacity, &rowLength));
    lastPositives.assign(positives, positives + nPositive);
    lastNegatives.assign(negatives, negatives + nNegative);
    lastRows.clear();
    lastRowLength = rowLength;
    for (int r = 0; r < nPositive + nNegative; ++r)   // the library leaves the row of a record without a patch unwritten: keep the others, packed
        if ((r < nPositive ? positives[r] : negatives[r - nPositive]).valid) lastRows.insert(lastRows.end(), all.begin() + (size_t)r * rowLength, all.begin() + (size_t)(r + 1) * rowLength);
}

void PositionDependentMeasurementModel::update(shared_ptr<imageprocessing::VersionedImage> image) { measurementModel->update(image); }
void PositionDependentMeasurementModel::evaluate(Sample& sample) const { measurementModel->evaluate(sample); }
void PositionDependentMeasurementModel::evaluate(shared_ptr<imageprocessing::VersionedImage> image, vector<shared_ptr<Sample>>& samples) {
    measurementModel->evaluate(image, samples);
}
void PositionDependentMeasurementModel::reset() {
    classifier->reset();
    usable = false;
}
bool PositionDependentMeasurementModel::initialize(shared_ptr<imageprocessing::VersionedImage> image, Sample& target) {
    vector<shared_ptr<Sample>> empty;
    return adapt(image, empty, target);
}
int PositionDependentMeasurementModel::draw(int n) {
    if (n <= 0) throw std::invalid_argument("PositionDependentMeasurementModel: the image is too small for random samples (range " + std::to_string(n) + ")");
    return (int)(((uint64_t)generator() * (uint64_t)n) >> 32);
}
Sample PositionDependentMeasurementModel::createRandomSample(const Mat& image) {   // :246-254
    int minSize = (int)(0.1 * std::min(image.cols, image.rows));
    int maxSize = (int)(0.9 * std::min(image.cols, image.rows));
    int size = draw(maxSize - minSize) + minSize;
    int halfSize = size / 2;
    int x = draw(image.cols - size) + halfSize;
    int y = draw(image.rows - size) + halfSize;
    return Sample(x, y, size);
}
bool PositionDependentMeasurementModel::hasWindow(int x, int y, int width, int height) const {
    const imageprocessing::SampledChain chain = imageprocessing::sampledChainOf(featureExtractor.get());
    return chain.extractable() ? chain.hasWindow(x, y, width, height) : (bool)featureExtractor->extract(x, y, width, height);
}
vector<Mat> PositionDependentMeasurementModel::extractAll(const vector<Sample>& samples, bool square) const {
    vector<Mat> data;
    data.reserve(samples.size());
    const imageprocessing::SampledChain chain = imageprocessing::sampledChainOf(featureExtractor.get());
    if (chain.extractable()) {   // one device call for the set
        vector<int32_t> xywh;
        xywh.reserve(4 * samples.size());
        for (const Sample& s : samples) xywh.insert(xywh.end(), {s.getX(), s.getY(), s.getWidth(), square ? s.getSize() : s.getHeight()});
        for (const Mat& m : chain.extract(xywh))
            if (!m.empty()) data.push_back(m);
        return data;
    }
    for (const Sample& s : samples) {
        auto patch = featureExtractor->extract(s.getX(), s.getY(), s.getWidth(), square ? s.getSize() : s.getHeight());
        if (patch) data.push_back(patch->getData());
    }
    return data;
}
vector<double> PositionDependentMeasurementModel::probabilities(const vector<Mat>& vectors) const {
    vector<double> p(vectors.size());
    auto* trainable = dynamic_cast<classification::TrainableProbabilisticSvmClassifier*>(classifier.get());
    const classification::ProbabilisticSvmClassifier* psvm = trainable ? trainable->getProbabilisticSvm().get() : nullptr;
    const bool batch = !vectors.empty() && vectors[0].depth() == CV_32F && detection::hasF32SupportVectors(psvm);
    if (batch) {   // one scoring call for the set
        const size_t d = (size_t)vectors[0].rows * vectors[0].cols * vectors[0].channels();
        vector<float> rows(vectors.size() * d);
        for (size_t i = 0; i < vectors.size(); ++i) {
            Mat v = contiguous(vectors[i]);
            if ((size_t)v.rows * v.cols * v.channels() != d) throw std::invalid_argument("PositionDependentMeasurementModel: feature vectors of different sizes");
            std::memcpy(rows.data() + i * d, v.data, sizeof(float) * d);
        }
        vector<double> dist(vectors.size());
        check(fd_svm_distance_batch(context(), psvm->getSvm()->native(psvm->getLogisticA(), psvm->getLogisticB()), rows.data(), (int64_t)vectors.size(), dist.data()));
        for (size_t i = 0; i < vectors.size(); ++i) p[i] = psvm->getProbability(dist[i]).second;
        return p;
    }
    for (size_t i = 0; i < vectors.size(); ++i) p[i] = classifier->getProbability(vectors[i]).second;
    return p;
}
// cv::flip(data, mirrored, 1) of a Mat whose columns are cells of `channels` floats: the cells of a row in reverse order, each as it is
static Mat flip_cells(const Mat& data, int channels) {
    if (channels <= 1 || data.type() != CV_32FC1 || data.cols % channels != 0) {
        Mat mirrored;
        cv::flip(data, mirrored, 1);
        return mirrored;
    }
    Mat mirrored(data.rows, data.cols, CV_32FC1);
    const int cells = data.cols / channels;
    for (int r = 0; r < data.rows; ++r)
        for (int c = 0; c < cells; ++c)
            std::memcpy(mirrored.ptr<float>(r) + (size_t)(cells - 1 - c) * channels, data.ptr<float>(r) + (size_t)c * channels, sizeof(float) * (size_t)channels);
    return mirrored;
}
vector<Mat> PositionDependentMeasurementModel::getFeatureVectors(const vector<Sample>& samples, int predicate) const {   // :256-274
    vector<Mat> patches = extractAll(samples, false);
    vector<double> p;
    if (predicate != 0) p = probabilities(patches);
    vector<Mat> trainingExamples;
    trainingExamples.reserve(exploitSymmetry ? 2 * patches.size() : patches.size());
    const int channels = exploitSymmetry ? imageprocessing::sampledChainOf(featureExtractor.get()).cellChannels() : 1;
    for (size_t i = 0; i < patches.size(); ++i) {
        if (predicate == 1 && !(p[i] < confidenceThreshold)) continue;
        if (predicate == 2 && !(p[i] > 1 - confidenceThreshold)) continue;
        trainingExamples.push_back(patches[i]);
        if (exploitSymmetry) trainingExamples.push_back(flip_cells(patches[i], channels));
    }
    return trainingExamples;
}
bool PositionDependentMeasurementModel::residentNegatives(fd_particles_negatives_params& params) const {
    const float downScaleBound = (1 - negativeOffsetFactor);
    const float upScaleBound = 1 / downScaleBound;
    params = fd_particles_negatives_params{(int32_t)std::min(sampleAdditionalNegatives, (unsigned int)INT32_MAX), negativeOffsetFactor, downScaleBound, upScaleBound};
    return sampleAdditionalNegatives >= 1 && sampleAdditionalNegatives <= FD_PARTICLES_NEGATIVES_MAX && std::isfinite(negativeOffsetFactor) &&
           std::isfinite(downScaleBound) && std::isfinite(upScaleBound);
}
PositionDependentMeasurementModel::NegativeBounds PositionDependentMeasurementModel::negativeBounds(const Sample& target) const {
    fd_particles_negatives_params params;
    residentNegatives(params);   // the floats, whatever they are
    NegativeBounds bounds;
    check(fd_particles_negatives_bounds(&params, target.getX(), target.getY(), target.getSize(), bounds.v));
    return bounds;
}
// :172-192: the list is ascending by weight; a new element goes before equal ones
vector<Sample> PositionDependentMeasurementModel::chooseAdditionalNegatives(const vector<shared_ptr<Sample>>& samples, const Sample& target) const {
    vector<Sample> additionalNegatives;
    if (sampleAdditionalNegatives == 0) return additionalNegatives;
    const NegativeBounds bounds = negativeBounds(target);
    additionalNegatives.reserve(sampleAdditionalNegatives);
    for (const shared_ptr<Sample>& sample : samples) {
        if (!bounds.outside(*sample)) continue;
        if (additionalNegatives.size() < sampleAdditionalNegatives) {
            auto low = std::lower_bound(additionalNegatives.begin(), additionalNegatives.end(), *sample,
                                        [](const Sample& a, const Sample& b) { return a.getWeight() < b.getWeight(); });
            additionalNegatives.insert(low, *sample);
        } else if (additionalNegatives.front().getWeight() < sample->getWeight()) {
            additionalNegatives.front() = *sample;
            for (unsigned int i = 1; i < additionalNegatives.size() && additionalNegatives[i - 1].getWeight() > additionalNegatives[i].getWeight(); ++i)
                std::swap(additionalNegatives[i - 1], additionalNegatives[i]);
        }
    }
    return additionalNegatives;
}
bool PositionDependentMeasurementModel::adapt(shared_ptr<imageprocessing::VersionedImage> image, const vector<shared_ptr<Sample>>& samples, const Sample& target) {
    return adaptResident(image, target, chooseAdditionalNegatives(samples, target));
}
bool PositionDependentMeasurementModel::adaptResident(shared_ptr<imageprocessing::VersionedImage> image, const Sample& target, const vector<Sample>& chosen) {
    if (!isUsable()) {
        frameCount++;
        if (frameCount < startFrameCount) return false;
    } else {
        frameCount = 0;
    }
    featureExtractor->update(image);
    vector<Mat> targetData = extractAll(vector<Sample>{target}, false);
    if (targetData.empty()) return false;
    if (isUsable() && classifier->getProbability(targetData[0]).second < targetThreshold) return false;

    vector<Sample> positiveSamples;
    if (positiveOffsetFactor == 0) {
        positiveSamples.push_back(target);
    } else {
        int offset = std::max(1, (int)(positiveOffsetFactor * target.getSize()));
        positiveSamples.push_back(target);
        positiveSamples.push_back(Sample(target.getX() - offset, target.getY(), target.getSize()));
        positiveSamples.push_back(Sample(target.getX() + offset, target.getY(), target.getSize()));
        positiveSamples.push_back(Sample(target.getX(), target.getY() - offset, target.getSize()));
        positiveSamples.push_back(Sample(target.getX(), target.getY() + offset, target.getSize()));
    }

    vector<Sample> negativeSamples;
    const NegativeBounds bounds = negativeBounds(target);
    const int xLowBound = bounds.v[0], xHighBound = bounds.v[1], yLowBound = bounds.v[2], yHighBound = bounds.v[3];
    const int sizeLowBound = bounds.v[4], sizeHighBound = bounds.v[5];
    const int tx = target.getX(), ty = target.getY(), ts = target.getSize();
    if (sampleNegativesAroundTarget > 0) {
        negativeSamples.push_back(Sample(xLowBound, ty, ts));
        negativeSamples.push_back(Sample(xHighBound, ty, ts));
        negativeSamples.push_back(Sample(tx, yLowBound, ts));
        negativeSamples.push_back(Sample(tx, yHighBound, ts));
        negativeSamples.push_back(Sample(tx, ty, sizeLowBound));
        negativeSamples.push_back(Sample(tx, ty, sizeHighBound));
        if (sampleNegativesAroundTarget > 1) {
            negativeSamples.push_back(Sample(xLowBound, yLowBound, ts));
            negativeSamples.push_back(Sample(xLowBound, yHighBound, ts));
            negativeSamples.push_back(Sample(xHighBound, yLowBound, ts));
            negativeSamples.push_back(Sample(xHighBound, yHighBound, ts));
            negativeSamples.push_back(Sample(xLowBound, ty, sizeLowBound));
            negativeSamples.push_back(Sample(xLowBound, ty, sizeHighBound));
            negativeSamples.push_back(Sample(xHighBound, ty, sizeLowBound));
            negativeSamples.push_back(Sample(xHighBound, ty, sizeHighBound));
            negativeSamples.push_back(Sample(tx, yLowBound, sizeLowBound));
            negativeSamples.push_back(Sample(tx, yLowBound, sizeHighBound));
            negativeSamples.push_back(Sample(tx, yHighBound, sizeLowBound));
            negativeSamples.push_back(Sample(tx, yHighBound, sizeHighBound));
            if (sampleNegativesAroundTarget > 2) {
                negativeSamples.push_back(Sample(xLowBound, yLowBound, sizeLowBound));
                negativeSamples.push_back(Sample(xLowBound, yLowBound, sizeHighBound));
                negativeSamples.push_back(Sample(xLowBound, yHighBound, sizeLowBound));
                negativeSamples.push_back(Sample(xLowBound, yHighBound, sizeHighBound));
                negativeSamples.push_back(Sample(xHighBound, yLowBound, sizeLowBound));
                negativeSamples.push_back(Sample(xHighBound, yLowBound, sizeHighBound));
                negativeSamples.push_back(Sample(xHighBound, yHighBound, sizeLowBound));
                negativeSamples.push_back(Sample(xHighBound, yHighBound, sizeHighBound));
            }
        }
    }
    auto outside = [&](const Sample& s) { return bounds.outside(s); };
    if (sampleAdditionalNegatives > 0) {
        vector<Sample> additionalNegatives = chosen;
        additionalNegatives.reserve(sampleAdditionalNegatives);
        while (additionalNegatives.size() < sampleAdditionalNegatives) {
            Sample sample = createRandomSample(image->getData());
            if (outside(sample) && hasWindow(sample.getX(), sample.getY(), sample.getSize(), sample.getSize())) additionalNegatives.push_back(sample);
        }
        negativeSamples.insert(negativeSamples.end(), additionalNegatives.begin(), additionalNegatives.end());
    }

    vector<Mat> positiveTestExamples;
    positiveTestExamples.push_back(targetData[0]);
    vector<Sample> testSamples;
    testSamples.reserve(sampleTestNegatives);
    while (testSamples.size() < sampleTestNegatives) {
        Sample sample = createRandomSample(image->getData());
        if (outside(sample) && hasWindow(sample.getX(), sample.getY(), sample.getSize(), sample.getSize())) testSamples.push_back(sample);
    }
    vector<Mat> negativeTestExamples = extractAll(testSamples, true);

    const bool filtered = isUsable() && confidenceThreshold > 0;
    const vector<Mat> positives = getFeatureVectors(positiveSamples, filtered ? 1 : 0);
    const vector<Mat> negatives = getFeatureVectors(negativeSamples, filtered ? 2 : 0);
    AdaptationRecord record;
    auto asRect = [](const Sample& s) { return cv::Rect(s.getX(), s.getY(), s.getSize(), s.getSize()); };
    for (const Sample& s : positiveSamples) record.positives.push_back(asRect(s));
    for (const Sample& s : negativeSamples) record.negatives.push_back(asRect(s));
    for (const Sample& s : testSamples) record.testNegatives.push_back(asRect(s));
    record.positiveVectors = positives;
    record.negativeVectors = negatives;
    lastAdaptation = record;
    ++adaptationCount;
    usable = classifier->retrain(positives, negatives, positiveTestExamples, negativeTestExamples);
    return true;
}
bool PositionDependentMeasurementModel::adapt(shared_ptr<imageprocessing::VersionedImage>, const vector<shared_ptr<Sample>>&) {   // :233-244
    if (isUsable()) frameCount++;
    if (frameCount == stopFrameCount) {
        reset();
        frameCount = 0;
    } else {
        const vector<Mat> empty;
        usable = classifier->retrain(empty, empty);
    }
    return false;
}


// ---- ExtendedHogBasedMeasurementModel, the evaluation half (ExtendedHogBasedMeasurementModel.cpp) -----------------------------------
int Sample::nextClusterId = 0;

ExtendedHogBasedMeasurementModel::ExtendedHogBasedMeasurementModel(shared_ptr<classification::ProbabilisticSvmClassifier> classifier)
    : cellSize(5), cellCount(35), signedAndUnsigned(false), interpolateBins(false), interpolateCells(true), octaveLayerCount(5),
      rejectionThreshold(-1.5), useSlidingWindow(true), conservativeReInit(false), negativeExampleCount(10), initialNegativeExampleCount(50),
      randomExampleCount(50), negativeScoreThreshold(-1.0f), positiveOverlapThreshold(0.5), negativeOverlapThreshold(0.5),
      adaptation(Adaptation::POSITION), adaptationThreshold(0.75), exclusionThreshold(0.0), classifier(classifier) {
    if (!classifier || !dynamic_cast<classification::LinearKernel*>(classifier->getSvm()->getKernel().get()))   // :74-75
        throw std::invalid_argument("ExtendedHogBasedMeasurementKernel: the SVM must use a LinearKernel");
}
ExtendedHogBasedMeasurementModel::ExtendedHogBasedMeasurementModel(shared_ptr<classification::TrainableProbabilisticSvmClassifier> trainable)
    : ExtendedHogBasedMeasurementModel(trainable ? trainable->getProbabilisticSvm() : shared_ptr<classification::ProbabilisticSvmClassifier>()) {
    this->trainable = trainable;
}
ExtendedHogBasedMeasurementModel::~ExtendedHogBasedMeasurementModel() {
    setTrainingTarget(nullptr);
    if (tracker) fd_ehog_tracker_destroy(tracker);
}
// a LibSvmClassifier behind the trainable trains on the model's tracker handle: the weights stay on the device
void ExtendedHogBasedMeasurementModel::setTrainingTarget(fd_ehog_tracker* target) {
    if (!trainable) return;
    auto svm = std::dynamic_pointer_cast<libsvm::LibSvmClassifier>(trainable->getTrainableSvm());
    if (svm) svm->setTrainingTarget(target, (int)(cellRowCount * cellColumnCount * (signedAndUnsigned ? 31 : 13)));
    trainsOnHandle = svm && target;
}

void ExtendedHogBasedMeasurementModel::setHogParams(size_t cellSize, size_t cellCount, bool signedAndUnsigned, bool interpolateBins, bool interpolateCells,
                                                    int octaveLayerCount) {
    this->cellSize = cellSize; this->cellCount = cellCount; this->signedAndUnsigned = signedAndUnsigned;
    this->interpolateBins = interpolateBins; this->interpolateCells = interpolateCells; this->octaveLayerCount = octaveLayerCount;
}
void ExtendedHogBasedMeasurementModel::setNegativeExampleParams(size_t negativeExampleCount, size_t initialNegativeExampleCount, size_t randomExampleCount,
                                                                float negativeScoreThreshold) {
    this->negativeExampleCount = negativeExampleCount; this->initialNegativeExampleCount = initialNegativeExampleCount;
    this->randomExampleCount = randomExampleCount; this->negativeScoreThreshold = negativeScoreThreshold;
}
void ExtendedHogBasedMeasurementModel::setOverlapThresholds(double positiveOverlapThreshold, double negativeOverlapThreshold) {
    this->positiveOverlapThreshold = positiveOverlapThreshold; this->negativeOverlapThreshold = negativeOverlapThreshold;
}
void ExtendedHogBasedMeasurementModel::setAdaptation(Adaptation adaptation, double adaptationThreshold, double exclusionThreshold) {
    this->adaptation = adaptation; this->adaptationThreshold = adaptationThreshold; this->exclusionThreshold = exclusionThreshold;
}

void ExtendedHogBasedMeasurementModel::computeCellGrid(int width, int height, size_t cellCount, size_t& cellColumnCount, size_t& cellRowCount) {   // :221-228
    const double aspectRatio = static_cast<double>(height) / static_cast<double>(width);
    if (aspectRatio < 1) {   // height is less than width, so determine height first
        cellRowCount = cv::cvRound(std::sqrt(aspectRatio * cellCount));
        cellColumnCount = cv::cvRound(cellRowCount / aspectRatio);
    } else {                 // width is less than or equal to height, so determine width first
        cellColumnCount = cv::cvRound(std::sqrt(cellCount / aspectRatio));
        cellRowCount = cv::cvRound(aspectRatio * cellColumnCount);
    }
}

static void model_update(fd_ehog_tracker* tracker, const shared_ptr<imageprocessing::VersionedImage>& image) {
    Mat src = contiguous(image->getData());
    if (src.depth() != CV_8U || (src.channels() != 1 && src.channels() != 3)) throw std::invalid_argument("GrayscaleFilter: the image must be CV_8UC1 or CV_8UC3");
    check(fd_ehog_tracker_update(context(), tracker, src.ptr<uchar>(0), src.cols, src.rows, src.channels(), 0));
}

void ExtendedHogBasedMeasurementModel::update(shared_ptr<imageprocessing::VersionedImage> image) {   // :97-105: one handle holds the three pyramids
    if (!tracker) throw std::runtime_error("ExtendedHogBasedMeasurementModel: model is not yet usable (was not initialized)");
    model_update(tracker, image);
}

void ExtendedHogBasedMeasurementModel::takeClassifierWeights() {   // in place of retrain + :336-340
    const auto svm = classifier->getSvm();
    if (svm->getSupportVectors().size() != 1)
        throw std::runtime_error("ExtendedHogBasedMeasurementModel: the amount of support vectors has to be one (w)");
    const int D = signedAndUnsigned ? 18 + 9 + 4 : 9 + 4;
    Mat w = contiguous(svm->getSupportVectors()[0]);
    if (w.depth() != CV_32F || (size_t)w.total() * w.channels() != cellRowCount * cellColumnCount * D)
        throw std::invalid_argument("ExtendedHogBasedMeasurementModel: the support vector must hold cellRowCount x cellColumnCount x channels floats");
    vector<float> scaled(w.ptr<float>(0), w.ptr<float>(0) + cellRowCount * cellColumnCount * D);
    const float c = svm->getCoefficients().empty() ? 1.f : svm->getCoefficients()[0];   // computeHyperplaneDistance: coefficient * dot - bias
    if (c != 1.f) throw std::invalid_argument("ExtendedHogBasedMeasurementModel: the coefficient of the one support vector (w) has to be one");
    check(fd_ehog_tracker_set_svm(context(), tracker, scaled.data(), svm->getBias()));
}

void ExtendedHogBasedMeasurementModel::scored(Sample& sample, bool valid, double score) const {   // :173-205
    if (!valid) {
        sample.setTarget(false);
        sample.setWeight(0);
        sample.setScore(0);
        return;
    }
    std::pair<bool, double> result = classifier->getProbability(score);
    sample.setWeight(sample.getWeight() * result.second);
    sample.setScore(score);
    if (targetLost) sample.setTarget(result.first);
    else sample.setTarget(useSlidingWindow ? score > rejectionThreshold : true);
}

void ExtendedHogBasedMeasurementModel::evaluate(Sample& sample) const {
    if (!tracker) throw std::runtime_error("ExtendedHogBasedMeasurementModel: model is not yet usable (was not initialized)");
    const int32_t xywh[4] = {sample.getX(), sample.getY(), sample.getWidth(), sample.getHeight()};
    uint8_t valid = 0;
    if (useSlidingWindow) {
        float score = 0;
        check(fd_ehog_tracker_evaluate_samples(context(), tracker, 1, xywh, &valid, &score));
        scored(sample, valid != 0, score);
    } else {
        vector<float> features(cellRowCount * cellColumnCount * (signedAndUnsigned ? 31 : 13));
        double score = 0;
        check(fd_ehog_tracker_extract_patches(context(), tracker, 1, xywh, &valid, features.data(), &score));
        scored(sample, valid != 0, score);
    }
}

// every sample of a frame in one device call; bestScore as :138-142 keeps it
void ExtendedHogBasedMeasurementModel::evaluateAll(vector<shared_ptr<Sample>>& samples, double* bestScore) {
    const int n = (int)samples.size();
    const vector<int32_t> xywh = pack_samples(samples);
    vector<uint8_t> valid((size_t)n);
    vector<double> score((size_t)n);
    if (useSlidingWindow) {
        vector<float> s((size_t)n);
        check(fd_ehog_tracker_evaluate_samples(context(), tracker, n, xywh.data(), valid.data(), s.data()));
        for (int i = 0; i < n; ++i) score[i] = s[i];
    } else {
        vector<float> features((size_t)n * cellRowCount * cellColumnCount * (signedAndUnsigned ? 31 : 13));
        check(fd_ehog_tracker_extract_patches(context(), tracker, n, xywh.data(), valid.data(), features.data(), score.data()));
    }
    ++fusedEvaluations;
    for (int i = 0; i < n; ++i) {
        scored(*samples[i], valid[i] != 0, score[i]);
        if (bestScore) *bestScore = std::max(*bestScore, samples[i]->getScore());
    }
}

void ExtendedHogBasedMeasurementModel::evaluate(shared_ptr<imageprocessing::VersionedImage> image, vector<shared_ptr<Sample>>& samples) {   // :107-168
    update(image);
    if (!useSlidingWindow) {
        evaluateAll(samples, nullptr);
        return;
    }
    std::pair<double, cv::Rect> peak = getHeatPeak();
    auto reinitialize = [&]() {   // :118-129,153-164: the draws in the reference's order, then one evaluation of all samples
        int clusterId = Sample::getNextClusterId();
        for (shared_ptr<Sample>& sample : samples) {
            sample->setX(peak.second.x + peak.second.width / 2 + 0.2 * peak.second.width * normalDistribution(generator));
            sample->setY(peak.second.y + peak.second.height / 2 + 0.2 * peak.second.width * normalDistribution(generator));
            sample->setSize(peak.second.width * (1 + 0.2 * normalDistribution(generator)));
            sample->setVx(0.1 * peak.second.width * normalDistribution(generator));
            sample->setVy(0.1 * peak.second.width * normalDistribution(generator));
            sample->setVSize(1 + 0.1 * normalDistribution(generator));
            sample->setClusterId(clusterId);
            sample->resetAncestor();
        }
        evaluateAll(samples, nullptr);
    };
    if (targetLost) {
        double peakScore = peak.first;
        if (classifier->getSvm()->classify(peakScore) && (!conservativeReInit || peakScore > adaptationThreshold)) {
            reinitialize();
        } else {   // target was lost and could not be re-initialized
            for (shared_ptr<Sample>& sample : samples) {
                sample->setWeight(0);
                sample->setScore(0);
                sample->setTarget(false);
            }
        }
    } else {
        double bestScore = std::numeric_limits<double>::lowest();
        evaluateAll(samples, &bestScore);
        double peakScore = peak.first;
        double initialFeaturesScore = classifier->getSvm()->computeHyperplaneDistance(initialFeatures);
        double scoreThreshold = 0.5 * (bestScore + initialFeaturesScore);
        if (conservativeReInit) scoreThreshold = std::max(scoreThreshold, adaptationThreshold);
        if (bestScore < initialFeaturesScore && classifier->getSvm()->classify(peakScore) && peakScore > scoreThreshold) reinitialize();
    }
}

bool ExtendedHogBasedMeasurementModel::isValid(const Sample& target, const vector<shared_ptr<Sample>>&, shared_ptr<imageprocessing::VersionedImage>) {   // :209-213
    if (!tracker) return false;
    const int32_t xywh[4] = {target.getX(), target.getY(), target.getWidth(), target.getHeight()};
    uint8_t valid = 0;
    double score = 0;
    vector<float> features(cellRowCount * cellColumnCount * (signedAndUnsigned ? 31 : 13));
    check(fd_ehog_tracker_extract_patches(context(), tracker, 1, xywh, &valid, features.data(), &score));
    return valid && score > rejectionThreshold;
}

bool ExtendedHogBasedMeasurementModel::initialize(shared_ptr<imageprocessing::VersionedImage> image, Sample& target) {   // :219-384 without retraining
    if (!initialized) {
        const double aspectRatio = static_cast<double>(target.getHeight()) / static_cast<double>(target.getWidth());
        computeCellGrid(target.getWidth(), target.getHeight(), cellCount, cellColumnCount, cellRowCount);
        if (cellColumnCount < 1 || cellRowCount < 1) throw std::invalid_argument("ExtendedHogFeatureExtractor: the amount of columns and rows must be greater than zero");
        const double newAspectRatio = static_cast<double>(cellRowCount) / static_cast<double>(cellColumnCount);
        if (newAspectRatio < aspectRatio) target.setSize(cv::cvRound(aspectRatio * target.getSize() / newAspectRatio));
        Sample::setAspectRatio((int)cellColumnCount, (int)cellRowCount);
        const Mat& data = image->getData();
        const double imageAspectRatio = static_cast<double>(data.rows) / static_cast<double>(data.cols);
        minWidth = cellSize * cellColumnCount;
        if (aspectRatio > imageAspectRatio) maxWidth = static_cast<size_t>(static_cast<size_t>(data.rows) / aspectRatio);
        else maxWidth = data.cols;
        fd_cehog_params filter = signedAndUnsigned ? fd_cehog_params{(int32_t)cellSize, 18, 1, 1, interpolateBins, interpolateCells, 0.2f}
                                                   : fd_cehog_params{(int32_t)cellSize, 9, 0, 1, interpolateBins, interpolateCells, 0.48f};
        fd_ehog_tracker_params prm = {filter, (int32_t)cellColumnCount, (int32_t)cellRowCount, octaveLayerCount, (int32_t)minWidth, (int32_t)maxWidth};
        setTrainingTarget(nullptr);
        if (tracker) { fd_ehog_tracker_destroy(tracker); tracker = nullptr; }
        check(fd_ehog_tracker_create(context(), &prm, &tracker));
        setTrainingTarget(tracker);
        initialized = true;
    }
    model_update(tracker, image);
    const int32_t xywh[4] = {target.getX(), target.getY(), target.getWidth(), target.getHeight()};
    uint8_t valid = 0;
    const int D = signedAndUnsigned ? 31 : 13;
    Mat features((int)cellRowCount, (int)cellColumnCount * D, CV_32FC1);
    check(fd_ehog_tracker_extract_patches(context(), tracker, 1, xywh, &valid, features.ptr<float>(0), nullptr));
    if (!valid) {
        reset();
        return false;
    }
    initialFeatures = features;
    if (!trainable) {
        takeClassifierWeights();   // builds the heat pyramid of this frame as well (:339-341)
        usable = true;
        targetLost = false;
        return usable;
    }
    // :329-384: the target against random windows, then against the windows the first model scores best
    const cv::Rect targetBounds = target.getBounds();
    const vector<cv::Rect> targetSample{cv::Rect(target.getX(), target.getY(), target.getWidth(), target.getHeight())};
    vector<cv::Rect> bounds;
    vector<Mat> negatives = createRandomNegativeExamples(initialNegativeExampleCount, image->getData(), targetBounds, &bounds);
    usable = retrain(vector<Mat>{initialFeatures}, negatives, targetSample, bounds);
    if (usable) {
        negatives = createNegativeTrainingExamples(image->getData(), targetBounds, bounds);
        if (useSlidingWindow || !negatives.empty()) usable = retrain(vector<Mat>(), negatives, vector<cv::Rect>(), bounds);
    }
    targetLost = false;
    return usable;
}

// trainable->retrain and, when the classifier is usable, its one support vector and bias as the heat pyramid's kernel (:334-340)
bool ExtendedHogBasedMeasurementModel::retrain(const vector<Mat>& positives, const vector<Mat>& negatives, const vector<cv::Rect>& positiveSamples,
                                               const vector<cv::Rect>& negativeBounds) {
    trainingLog.push_back(TrainingRecord{positiveSamples, negativeBounds});
    const bool ok = trainable->retrain(positives, negatives);
    if (!ok) return false;
    if (!trainsOnHandle) {
        takeClassifierWeights();
    } else if (classifier->getSvm()->getSupportVectors().size() != 1) {   // the handle already holds the weights and this frame's heat pyramid
        throw std::runtime_error("ExtendedHogBasedMeasurementModel: the amount of support vectors has to be one (w)");
    }
    return true;
}

bool ExtendedHogBasedMeasurementModel::extractPositive(const Sample& target, Mat& features, double* score) const {
    const int32_t xywh[4] = {target.getX(), target.getY(), target.getWidth(), target.getHeight()};
    uint8_t valid = 0;
    features = Mat((int)cellRowCount, (int)cellColumnCount * (signedAndUnsigned ? 31 : 13), CV_32FC1);
    check(fd_ehog_tracker_extract_patches(context(), tracker, 1, xywh, &valid, features.ptr<float>(0), score));
    return valid != 0;
}

vector<Mat> ExtendedHogBasedMeasurementModel::createPositiveTrainingExamples(const Sample& target, vector<cv::Rect>& samplesUsed) {   // :492-533
    samplesUsed.clear();
    if (adaptation == Adaptation::NONE) return vector<Mat>();
    if (adaptation == Adaptation::CORRECTED_TRAJECTORY)
        throw std::runtime_error("ExtendedHogBasedMeasurementModel: the corrected trajectory needs the feature extractors of past frames, which this backend does not keep");
    Mat features;
    double score = 0;
    if (!extractPositive(target, features, &score)) return vector<Mat>();
    const cv::Rect sample(target.getX(), target.getY(), target.getWidth(), target.getHeight());
    if (adaptation == Adaptation::POSITION) {
        if (score <= adaptationThreshold) return vector<Mat>();
        samplesUsed.push_back(sample);
        return vector<Mat>{features};
    }
    // TRAJECTORY: collect the patches above the exclusion threshold, learn them all once the target scores above the adaptation threshold
    if (score > exclusionThreshold) {
        trajectoryFeatures.push_back(features);
        trajectorySamples.push_back(sample);
    }
    if (score <= adaptationThreshold) return vector<Mat>();
    vector<Mat> examples = trajectoryFeatures;
    samplesUsed = trajectorySamples;
    trajectoryFeatures.clear();
    trajectorySamples.clear();
    return examples;
}

vector<Mat> ExtendedHogBasedMeasurementModel::createNegativeTrainingExamples(const Mat& image, cv::Rect targetBounds, vector<cv::Rect>& bounds) const {   // :593-619
    bounds.clear();
    if (useSlidingWindow) {
        vector<Mat> examples = createGoodNegativeExamples(targetBounds, &bounds);
        if (examples.size() > negativeExampleCount) {
            examples.resize(negativeExampleCount);
            bounds.resize(negativeExampleCount);
        }
        return examples;
    }
    vector<cv::Rect> candidateBounds;
    vector<Mat> candidates = createRandomNegativeExamples(randomExampleCount, image, targetBounds, &candidateBounds);
    vector<std::pair<float, size_t>> classified(candidates.size());
    for (size_t i = 0; i < candidates.size(); ++i) classified[i] = std::make_pair((float)classifier->getSvm()->computeHyperplaneDistance(candidates[i]), i);
    const size_t top = std::min(negativeExampleCount, classified.size());
    std::partial_sort(classified.begin(), classified.begin() + top, classified.end(),
                      [](const std::pair<float, size_t>& a, const std::pair<float, size_t>& b) { return a.first > b.first; });
    size_t count = top;
    while (count > 0 && classified[count - 1].first <= negativeScoreThreshold) count--;
    vector<Mat> examples;
    for (size_t i = 0; i < count; ++i) {
        examples.push_back(candidates[classified[i].second]);
        bounds.push_back(candidateBounds[classified[i].second]);
    }
    return examples;
}

cv::Rect ExtendedHogBasedMeasurementModel::createRandomBounds(const Mat& image) const {   // :685-692; a range of n values is [0, n)
    auto below = [this](long n) { return n > 1 ? std::uniform_int_distribution<int>(0, (int)n - 1)(generator) : 0; };
    const int width = below((long)maxWidth - (long)minWidth) + (int)minWidth;
    const int height = (int)(width * cellRowCount / cellColumnCount);
    const int x = below(image.cols - width);
    const int y = below(image.rows - height);
    return cv::Rect(x, y, width, height);
}

vector<Mat> ExtendedHogBasedMeasurementModel::createRandomNegativeExamples(size_t count, const Mat& image, cv::Rect targetBounds, vector<cv::Rect>* chosen) const {
    if (!tracker) throw std::runtime_error("ExtendedHogBasedMeasurementModel: model is not yet usable (was not initialized)");
    const int D = signedAndUnsigned ? 31 : 13;
    vector<Mat> examples;
    vector<cv::Rect> boxes;
    size_t draws = 0;
    while (examples.size() < count) {
        if (++draws > 1000 * (count + 1)) throw std::runtime_error("ExtendedHogBasedMeasurementModel: no random negative example has a patch in this image");
        const cv::Rect bounds = createRandomBounds(image);
        if (!(computeOverlap(targetBounds, bounds) < positiveOverlapThreshold)) continue;
        const int32_t xywh[4] = {bounds.x + bounds.width / 2, bounds.y + bounds.height / 2, bounds.width, bounds.height};
        uint8_t valid = 0;
        Mat m((int)cellRowCount, (int)cellColumnCount * D, CV_32FC1);
        if (useSlidingWindow) check(fd_ehog_tracker_extract_cells(context(), tracker, 1, xywh, &valid, m.ptr<float>(0)));
        else check(fd_ehog_tracker_extract_patches(context(), tracker, 1, xywh, &valid, m.ptr<float>(0), nullptr));
        if (!valid) continue;
        examples.push_back(m);
        boxes.push_back(bounds);
    }
    if (chosen) *chosen = boxes;
    return examples;
}

bool ExtendedHogBasedMeasurementModel::adapt(shared_ptr<imageprocessing::VersionedImage> image, const vector<shared_ptr<Sample>>&, const Sample& target) {   // :386-404
    if (!usable) throw std::runtime_error("ExtendedHogBasedMeasurementModel: model is not yet usable (was not initialized)");
    targetLost = false;
    if (!trainable) {
        takeClassifierWeights();
        return true;
    }
    vector<cv::Rect> positiveSamples, negativeBounds;
    const vector<Mat> positives = createPositiveTrainingExamples(target, positiveSamples);
    if (positives.empty()) return false;
    const vector<Mat> negatives = createNegativeTrainingExamples(image->getData(), target.getBounds(), negativeBounds);
    usable = retrain(positives, negatives, positiveSamples, negativeBounds);
    return true;
}
bool ExtendedHogBasedMeasurementModel::adapt(shared_ptr<imageprocessing::VersionedImage>, const vector<shared_ptr<Sample>>&) {   // :406-419
    if (!usable) throw std::runtime_error("ExtendedHogBasedMeasurementModel: model is not yet usable (was not initialized)");
    if (trainable) {
        usable = trainable->retrain(vector<Mat>(), vector<Mat>());   // nothing new: the classifier's state
        if (usable) takeClassifierWeights();
    } else {
        takeClassifierWeights();
    }
    targetLost = true;
    return false;
}
void ExtendedHogBasedMeasurementModel::reset() {   // :421-432
    if (trainable) trainable->reset();
    initialized = false;
    usable = false;
    targetLost = false;
    initialFeatures = Mat();
    trajectoryFeatures.clear();
    trajectorySamples.clear();
}

std::pair<double, cv::Rect> ExtendedHogBasedMeasurementModel::getHeatPeak() const {   // :434-456
    if (!tracker) throw std::runtime_error("ExtendedHogBasedMeasurementModel: model is not yet usable (was not initialized)");
    fd_box peak;
    int found = 0;
    check(fd_ehog_tracker_heat_peak(context(), tracker, &peak, &found));
    if (!found) return std::make_pair(std::numeric_limits<double>::lowest(), cv::Rect());
    return std::make_pair((double)peak.score, cv::Rect(peak.x, peak.y, peak.w, peak.h));
}

double ExtendedHogBasedMeasurementModel::computeOverlap(cv::Rect a, cv::Rect b) const {   // :694-698
    const int x0 = std::max(a.x, b.x), y0 = std::max(a.y, b.y);
    const int x1 = std::min(a.x + a.width, b.x + b.width), y1 = std::min(a.y + a.height, b.y + b.height);
    const double intersectionArea = x1 > x0 && y1 > y0 ? (double)(x1 - x0) * (y1 - y0) : 0.0;
    const double unionArea = (double)a.width * a.height + (double)b.width * b.height - intersectionArea;
    return intersectionArea / unionArea;
}

vector<Mat> ExtendedHogBasedMeasurementModel::createGoodNegativeExamples(cv::Rect targetBounds, vector<cv::Rect>* chosen) const {   // :621-669
    if (!tracker) throw std::runtime_error("ExtendedHogBasedMeasurementModel: model is not yet usable (was not initialized)");
    const vector<fd_box> maxima = with_capacity<fd_box>(4096, [&](fd_box* boxes, int cap, int* count) {
        return fd_ehog_tracker_heat_maxima(context(), tracker, negativeScoreThreshold, boxes, cap, count);
    });
    vector<std::pair<float, cv::Rect>> candidates;
    for (const fd_box& m : maxima) {
        cv::Rect bounds(m.x, m.y, m.w, m.h);
        if (computeOverlap(targetBounds, bounds) < positiveOverlapThreshold) candidates.emplace_back(m.score, bounds);
    }
    // reduce overlapping candidates using non-maximum suppression
    std::sort(candidates.begin(), candidates.end(), [](const std::pair<float, cv::Rect>& a, const std::pair<float, cv::Rect>& b) { return a.first < b.first; });
    vector<cv::Rect> boxes;
    while (!candidates.empty()) {
        const cv::Rect box = candidates.back().second;
        candidates.pop_back();
        boxes.push_back(box);
        candidates.erase(std::remove_if(candidates.begin(), candidates.end(),
                                        [&](const std::pair<float, cv::Rect>& elem) { return computeOverlap(box, elem.second) > negativeOverlapThreshold; }),
                         candidates.end());
    }
    const int D = signedAndUnsigned ? 31 : 13;
    const size_t per = cellRowCount * cellColumnCount * D;
    vector<int32_t> xywh;
    for (const cv::Rect& box : boxes) {
        xywh.push_back(box.x + box.width / 2); xywh.push_back(box.y + box.height / 2); xywh.push_back(box.width); xywh.push_back(box.height);
    }
    vector<uint8_t> valid(boxes.size());
    vector<float> features(boxes.size() * per);
    if (!boxes.empty()) check(fd_ehog_tracker_extract_cells(context(), tracker, (int)boxes.size(), xywh.data(), valid.data(), features.data()));
    vector<Mat> examples;
    examples.reserve(boxes.size());
    for (size_t i = 0; i < boxes.size(); ++i) {
        Mat m((int)cellRowCount, (int)cellColumnCount * D, CV_32FC1);
        std::memcpy(m.ptr<float>(0), features.data() + i * per, sizeof(float) * per);
        examples.push_back(m);
    }
    if (chosen) *chosen = boxes;
    return examples;
}

// ---- the rest of the Condensation tracker: samplers, transition model, state extractors, trackers -----------------------

LowVarianceSampling::LowVarianceSampling(unsigned int seed) : generator(seed), distribution(0.0, 1.0) {}

void LowVarianceSampling::resample(const vector<shared_ptr<Sample>>& samples, size_t count, vector<shared_ptr<Sample>>& newSamples) {   // .cpp:20-39
    newSamples.reserve(count);
    if (samples.size() > 0) {
        double weightSum = computeWeightSum(samples);
        double step = weightSum / count;
        if (step > 0) {
            double start = step * draw();
            size_t sample = 0;
            double runningSum = samples[0]->getWeight();
            for (unsigned int i = 0; i < count; ++i) {
                double weightPointer = start + i * step;
                while (weightPointer > runningSum && sample + 1 < samples.size()) {   // the second condition is not the reference's
                    ++sample;
                    runningSum += samples[sample]->getWeight();
                }
                newSamples.emplace_back(new Sample(samples[sample]));
            }
        }
    }
}

double LowVarianceSampling::computeWeightSum(const vector<shared_ptr<Sample>>& samples) {   // .cpp:41-46
    double weightSum = 0;
    for (const shared_ptr<Sample>& sample : samples) weightSum += sample->getWeight();
    return weightSum;
}

SimpleTransitionModel::SimpleTransitionModel(double positionDeviation, double sizeDeviation, unsigned int seed)
    : positionDeviation(positionDeviation), sizeDeviation(sizeDeviation), generator(seed), distribution() {}

void SimpleTransitionModel::init(const Mat&) {}

void SimpleTransitionModel::drawDiffusion(double out[3]) {
    out[0] = positionDeviation * distribution(generator);
    out[1] = positionDeviation * distribution(generator);
    out[2] = pow(2, sizeDeviation * distribution(generator));
}

const vector<double>& SimpleTransitionModel::drawBlock(size_t samples) {
    lastDiffusion.resize(3 * samples);
    for (size_t i = 0; i < samples; ++i) drawDiffusion(&lastDiffusion[3 * i]);
    return lastDiffusion;
}

void SimpleTransitionModel::apply(Sample& sample, const double diffusion[3]) {   // .cpp:27-42
    double vx = sample.getVx();
    double vy = sample.getVy();
    double vs = sample.getVSize();
    vx += diffusion[0];
    vy += diffusion[1];
    vs *= diffusion[2];
    sample.setVx(static_cast<int>(std::round(vx)));
    sample.setVy(static_cast<int>(std::round(vy)));
    sample.setVSize(vs);
    sample.setX(sample.getX() + sample.getVx());
    sample.setY(sample.getY() + sample.getVy());
    sample.setSize(static_cast<int>(std::round(sample.getSize() * sample.getVSize())));   // int * float: a float product
}

void SimpleTransitionModel::predict(vector<shared_ptr<Sample>>& samples, const Mat&, const shared_ptr<Sample>) {
    lastDiffusion.clear();
    for (shared_ptr<Sample>& sample : samples) {
        double diffusion[3];
        drawDiffusion(diffusion);
        lastDiffusion.insert(lastDiffusion.end(), diffusion, diffusion + 3);
        apply(*sample, diffusion);
    }
}

OpticalFlowTransitionModel::OpticalFlowTransitionModel(shared_ptr<TransitionModel> fallback, double positionDeviation, double sizeDeviation,
                                                       cv::Size gridSize, bool circle, cv::Size windowSize, int maxLevel, unsigned int seed)
    : fallback(fallback), gridSize(gridSize), windowSize(windowSize), maxLevel(maxLevel), positionDeviation(positionDeviation),
      sizeDeviation(sizeDeviation), generator(seed), distribution() {
    if (!fallback) throw std::invalid_argument("OpticalFlowTransitionModel: the fallback model is missing");
    int minWindow = 0, maxWindow = 0;
    fd_flow_limits(nullptr, &minWindow, &maxWindow);   // host only, like the grid and the median below: no context, nothing to check() against
    if (windowSize.width < minWindow || windowSize.width > maxWindow || windowSize.height < minWindow || windowSize.height > maxWindow)
        throw std::invalid_argument("OpticalFlowTransitionModel: the window size must be " + std::to_string(minWindow) + " .. " + std::to_string(maxWindow) + " per side");
    if (maxLevel < 0 || maxLevel >= FD_FLOW_MAX_LEVELS) throw std::invalid_argument("OpticalFlowTransitionModel: the maximal level must be 0 .. " + std::to_string(FD_FLOW_MAX_LEVELS - 1));
    int n = 0;
    if (gridSize.width < 1 || gridSize.height < 1 || fd_flow_grid(gridSize.width, gridSize.height, circle ? 1 : 0, nullptr, 0, &n) == FD_ERR_INVALID_ARGUMENT ||
        n > FD_FLOW_MAX_POINTS)
        throw std::invalid_argument("OpticalFlowTransitionModel: invalid grid size");
    vector<float> xy(2 * (size_t)n);
    if (n > 0 && fd_flow_grid(gridSize.width, gridSize.height, circle ? 1 : 0, xy.data(), n, &n) != FD_OK) throw std::logic_error("OpticalFlowTransitionModel: fd_flow_grid failed");
    for (int i = 0; i < n; ++i) templatePoints.push_back(cv::Point2f(xy[2 * i], xy[2 * i + 1]));
    lastMotion.median_ratio = 1.f;
}

OpticalFlowTransitionModel::~OpticalFlowTransitionModel() { fd_flow_destroy(flow); }

void OpticalFlowTransitionModel::updatePyramid(const Mat& image) {
    if (image.empty() || image.depth() != CV_8U || (image.channels() != 1 && image.channels() != 3))
        throw std::invalid_argument("OpticalFlowTransitionModel: the image must be CV_8UC1 or CV_8UC3");
    if (!flow || flowWidth != image.cols || flowHeight != image.rows) {   // another frame size: nothing of the previous frame can be used
        fd_flow_destroy(flow);
        flow = nullptr;
        hasPrevious = false;
        fd_flow_params params;
        check(fd_flow_default_params(&params));
        params.win_w = windowSize.width;
        params.win_h = windowSize.height;
        params.max_level = maxLevel;
        check(fd_flow_create(context(), image.cols, image.rows, &params, &flow));
        flowWidth = image.cols;
        flowHeight = image.rows;
    }
    check(fd_flow_update(context(), flow, image.data, image.channels(), (int)image.step, 0));
}

void OpticalFlowTransitionModel::trackPoints(const vector<cv::Point2f>& points, vector<cv::Point2f>& forwardPoints, vector<cv::Point2f>& backwardPoints,
                                             vector<uchar>& forwardStatus, vector<uchar>& backwardStatus) {
    static_assert(sizeof(cv::Point2f) == 2 * sizeof(float), "Point2f is two floats");
    const size_t n = points.size();
    forwardPoints.resize(n);
    backwardPoints.resize(n);
    forwardStatus.resize(n);
    backwardStatus.resize(n);
    if (n == 0) return;
    check(fd_flow_track_fb(context(), flow, &points[0].x, (int)n, &forwardPoints[0].x, &backwardPoints[0].x, forwardStatus.data(), backwardStatus.data()));
}

void OpticalFlowTransitionModel::init(const Mat& image) {   // .cpp:86-88
    updatePyramid(image);
    hasPrevious = true;
}

void OpticalFlowTransitionModel::apply(Sample& sample, float medianX, float medianY, float medianRatio, double positionDeviation, double sizeDeviation,
                                       const double z[3]) {   // .cpp:174-189
    double vx = medianX;
    double vy = medianY;
    double vs = medianRatio;
    vx += positionDeviation * z[0];
    vy += positionDeviation * z[1];
    vs *= pow(2, sizeDeviation * z[2]);
    sample.setVx(static_cast<int>(std::round(vx)));
    sample.setVy(static_cast<int>(std::round(vy)));
    sample.setVSize(vs);
    sample.setX(sample.getX() + sample.getVx());
    sample.setY(sample.getY() + sample.getVy());
    sample.setSize(static_cast<int>(std::round(sample.getSize() * sample.getVSize())));   // int * float: a float product
}

bool OpticalFlowTransitionModel::residentPossible() const {
    return fallback && typeid(*fallback) == typeid(SimpleTransitionModel) && templatePoints.size() <= (size_t)FD_FLOW_RESIDENT_MAX_POINTS;
}

bool OpticalFlowTransitionModel::beginResident(const Mat& image, const shared_ptr<Sample> target) {   // predict up to the tracking
    points.clear();
    forwardPoints.clear();
    backwardPoints.clear();
    forwardStatus.clear();
    backwardStatus.clear();
    correctFlowIndices.clear();
    lastDraws.clear();
    tracksOnDevice = false;
    flowUsed = false;
    lastMotion = fd_flow_motion{};
    lastMotion.median_ratio = 1.f;
    const bool hadPrevious = hasPrevious;
    updatePyramid(image);   // may reset hasPrevious (another frame size)
    const bool previous = hadPrevious && hasPrevious;
    hasPrevious = true;
    if (!previous || !target) return false;
    for (const cv::Point2f& point : templatePoints)
        points.push_back(cv::Point2f(target->getWidth() * point.x + target->getX(), target->getHeight() * point.y + target->getY()));
    static const float none[2] = {0.f, 0.f};
    check(fd_flow_track_fb_resident(context(), flow, points.empty() ? none : &points[0].x, (int)points.size()));
    tracksOnDevice = true;
    return true;
}

const vector<double>& OpticalFlowTransitionModel::drawResident(size_t samples) {
    generatorBefore = generator;
    distributionBefore = distribution;
    lastDraws.resize(3 * samples);
    residentDiffusion.resize(3 * samples);
    for (size_t i = 0; i < 3 * samples; i += 3) {   // apply's expressions on the draws
        for (int c = 0; c < 3; ++c) lastDraws[i + c] = distribution(generator);
        residentDiffusion[i] = positionDeviation * lastDraws[i];
        residentDiffusion[i + 1] = positionDeviation * lastDraws[i + 1];
        residentDiffusion[i + 2] = pow(2, sizeDeviation * lastDraws[i + 2]);
    }
    return residentDiffusion;
}

void OpticalFlowTransitionModel::endResident(const fd_flow_motion_info& motion) {
    lastMotion.ok = motion.ok;
    lastMotion.n_valid = motion.n_valid;
    lastMotion.n_correct = motion.n_correct;
    lastMotion.median_x = motion.median_x;
    lastMotion.median_y = motion.median_y;
    lastMotion.median_ratio = motion.median_ratio;
    flowUsed = motion.ok != 0;
    if (!flowUsed) {   // the fallback predicted: this model drew nothing
        generator = generatorBefore;
        distribution = distributionBefore;
        lastDraws.clear();
    }
}

void OpticalFlowTransitionModel::fetchTracks() const {
    if (!tracksOnDevice) return;
    tracksOnDevice = false;
    const size_t n = points.size();
    forwardPoints.resize(n);
    backwardPoints.resize(n);
    forwardStatus.resize(n);
    backwardStatus.resize(n);
    vector<int32_t> order(std::max<size_t>(n, 1));
    int count = 0, valid = 0, correct = 0;
    static float none[2];
    static uchar noStatus[1];
    check(fd_flow_get_tracks(context(), flow, (int)n, &count, n ? &forwardPoints[0].x : none, n ? &backwardPoints[0].x : none, n ? forwardStatus.data() : noStatus,
                             n ? backwardStatus.data() : noStatus, order.data(), &valid, &correct));
    correctFlowIndices.assign(order.begin(), order.begin() + correct);
}

void OpticalFlowTransitionModel::predict(vector<shared_ptr<Sample>>& samples, const Mat& image, const shared_ptr<Sample> target) {   // .cpp:90-191
    tracksOnDevice = false;
    points.clear();
    forwardPoints.clear();
    backwardPoints.clear();
    forwardStatus.clear();
    backwardStatus.clear();
    correctFlowIndices.clear();
    lastDraws.clear();
    flowUsed = false;
    lastMotion = fd_flow_motion{};
    lastMotion.median_ratio = 1.f;

    const bool hadPrevious = hasPrevious;
    updatePyramid(image);   // may reset hasPrevious (another frame size)
    if (!(hadPrevious && hasPrevious) || !target) {   // no previous pyramid or no current target
        hasPrevious = true;
        return fallback->predict(samples, image, target);
    }

    for (const cv::Point2f& point : templatePoints)
        points.push_back(cv::Point2f(target->getWidth() * point.x + target->getX(), target->getHeight() * point.y + target->getY()));
    trackPoints(points, forwardPoints, backwardPoints, forwardStatus, backwardStatus);
    if (forwardPoints.size() != points.size() || backwardPoints.size() != points.size() || forwardStatus.size() != points.size() ||
        backwardStatus.size() != points.size())
        throw std::logic_error("OpticalFlowTransitionModel: trackPoints must fill one entry per point");

    const int n = (int)points.size();
    vector<int32_t> order(std::max(n, 1));
    fd_flow_motion motion{};
    motion.order = order.data();
    static const float none[2] = {0.f, 0.f};
    static const uchar noStatus[1] = {0};
    if (fd_flow_median(n ? &points[0].x : none, n ? &forwardPoints[0].x : none, n ? &backwardPoints[0].x : none, n ? forwardStatus.data() : noStatus,
                       n ? backwardStatus.data() : noStatus, n, &motion) != FD_OK)
        throw std::logic_error("OpticalFlowTransitionModel: fd_flow_median failed");
    lastMotion = motion;
    lastMotion.order = nullptr;
    correctFlowIndices.assign(order.begin(), order.begin() + motion.n_correct);
    if (!motion.ok) return fallback->predict(samples, image, target);   // too few points tracked, or too few correct correspondences

    flowUsed = true;
    lastDraws.reserve(3 * samples.size());
    for (shared_ptr<Sample>& sample : samples) {
        double z[3];
        z[0] = distribution(generator);
        z[1] = distribution(generator);
        z[2] = distribution(generator);
        lastDraws.insert(lastDraws.end(), z, z + 3);
        apply(*sample, motion.median_x, motion.median_y, motion.median_ratio, positionDeviation, sizeDeviation, z);
    }
}

ResamplingSampler::ResamplingSampler(unsigned int count, double randomRate, shared_ptr<ResamplingAlgorithm> resamplingAlgorithm,
                                     shared_ptr<TransitionModel> transitionModel, int minSize, int maxSize, unsigned int seed)
    : count(count), randomRate(randomRate), resamplingAlgorithm(resamplingAlgorithm), transitionModel(transitionModel), minSize(minSize), maxSize(maxSize),
      generator(seed), realDistribution(0.0, 1.0) {
    if (minSize < 1) throw std::invalid_argument("ResamplingSampler: the minimum size must be greater than zero");
    if (maxSize < minSize) throw std::invalid_argument("ResamplingSampler: the maximum size must not be smaller than the minimum size");
    setRandomRate(randomRate);
}

void ResamplingSampler::init(const Mat& image) {   // .cpp:42-48
    if (minSize > image.cols || minSize > image.rows)
        throw std::invalid_argument("ResamplingSampler: the minimum size must not be greater than the width and height of the image");
    if (maxSize > image.cols || maxSize > image.rows) maxSize = std::min(image.cols, image.rows);
    transitionModel->init(image);
}

void ResamplingSampler::drawValues(int cols, int rows, int32_t out[3]) {   // .cpp:61-71
    auto upTo = [this](int n) { return n > 0 ? std::uniform_int_distribution<int>(0, n)(generator) : 0; };
    double sizeFactor = realDistribution(generator) * (static_cast<double>(maxSize) / static_cast<double>(minSize) - 1.0) + 1.0;
    int size = cv::cvRound(sizeFactor * minSize);
    int halfSize = size / 2;
    out[2] = size;
    out[0] = upTo(cols - size) + halfSize;
    out[1] = upTo(rows - size) + halfSize;
}

void ResamplingSampler::sampleValues(Sample& sample, const Mat& image) {
    int32_t v[3];
    drawValues(image.cols, image.rows, v);
    lastDraws.fresh.insert(lastDraws.fresh.end(), v, v + 3);
    sample.setSize(v[2]);
    sample.setX(v[0]);
    sample.setY(v[1]);
    sample.setVx(0);
    sample.setVy(0);
    sample.setVSize(1);
}

void ResamplingSampler::sample(const vector<shared_ptr<Sample>>& samples, vector<shared_ptr<Sample>>& newSamples, const Mat& image,
                               const shared_ptr<Sample> target) {   // .cpp:50-59
    lastDraws = Draws();
    auto lowVariance = std::dynamic_pointer_cast<LowVarianceSampling>(resamplingAlgorithm);
    auto simple = std::dynamic_pointer_cast<SimpleTransitionModel>(transitionModel);
    if (lowVariance) lowVariance->forgetLastDraw();
    resamplingAlgorithm->resample(samples, (int)((1 - randomRate) * count), newSamples);
    transitionModel->predict(newSamples, image, target);
    if (lowVariance && lowVariance->hasLastDraw()) { lastDraws.hasU = true; lastDraws.u = lowVariance->getLastDraw(); }
    if (simple) lastDraws.diffusion = simple->getLastDiffusion();
    while (newSamples.size() < count) {
        shared_ptr<Sample> newSample = make_shared<Sample>();
        sampleValues(*newSample, image);
        newSamples.push_back(newSample);
    }
}

const ResamplingSampler::Draws& ResamplingSampler::drawFrame(size_t oldCount, double oldWeightSum, int cols, int rows, SimpleTransitionModel* simple) {
    lastDraws = Draws();
    auto lowVariance = std::dynamic_pointer_cast<LowVarianceSampling>(resamplingAlgorithm);
    if (!simple) simple = dynamic_cast<SimpleTransitionModel*>(transitionModel.get());
    if (!lowVariance || !simple) throw std::logic_error("ResamplingSampler::drawFrame needs LowVarianceSampling and SimpleTransitionModel");
    const size_t resampled = (size_t)(int)((1 - randomRate) * count);
    size_t copies = 0;
    if (oldCount > 0 && oldWeightSum / resampled > 0) {   // LowVarianceSampling.cpp:22-26: the draw is taken even for zero copies
        lastDraws.hasU = true;
        lastDraws.u = lowVariance->draw();
        copies = resampled;
    }
    lastDraws.diffusion = simple->drawBlock(copies);
    for (size_t i = copies; i < count; ++i) {
        int32_t v[3];
        drawValues(cols, rows, v);
        lastDraws.fresh.insert(lastDraws.fresh.end(), v, v + 3);
    }
    return lastDraws;
}

GridSampler::GridSampler(int minSize, int maxSize, float sizeScale, float stepSize) : minSize(minSize), maxSize(maxSize), sizeScale(sizeScale), stepSize(stepSize) {
    if (minSize < 1) throw std::invalid_argument("GridSampler: the minimum size must be greater than zero");
    if (maxSize < minSize) throw std::invalid_argument("GridSampler: the maximum size must not be smaller than the minimum size");
    if (sizeScale <= 1) throw std::invalid_argument("GridSampler: The scale factor of the size must be greater than one");
    if (stepSize <= 0) throw std::invalid_argument("GridSampler: The step size must be greater than zero");
}

void GridSampler::init(const Mat&) {}

void GridSampler::sample(const vector<shared_ptr<Sample>>&, vector<shared_ptr<Sample>>& newSamples, const Mat& image, const shared_ptr<Sample>) {   // .cpp:37-53
    newSamples.clear();
    for (int size = minSize; size <= maxSize; size *= sizeScale) {
        int halfSize = size / 2;
        int minX = halfSize;
        int minY = halfSize;
        int maxX = image.cols - size + halfSize;
        int maxY = image.rows - size + halfSize;
        int step = (int)(stepSize * size + 0.5f);
        if (step < 1) throw std::invalid_argument("GridSampler: the step size rounds to zero pixels");   // the reference would not return
        for (int x = minX; x < maxX; x += step) {
            for (int y = minY; y < maxY; y += step) newSamples.push_back(make_shared<Sample>(x, y, size));
        }
    }
}

FilteringStateExtractor::FilteringStateExtractor(shared_ptr<StateExtractor> extractor) : extractor(extractor) {}

shared_ptr<Sample> FilteringStateExtractor::extract(const vector<shared_ptr<Sample>>& samples) {
    vector<shared_ptr<Sample>> objects;
    for (const shared_ptr<Sample>& sample : samples) {
        if (sample->isTarget()) objects.push_back(sample);
    }
    return extractor->extract(objects);
}

WeightedMeanStateExtractor::WeightedMeanStateExtractor() {}

shared_ptr<Sample> WeightedMeanStateExtractor::extract(const vector<shared_ptr<Sample>>& samples) {   // .cpp:23-62
    std::unordered_map<int, std::pair<size_t, size_t>> clusters;   // id -> (members, index of the first member)
    for (size_t i = 0; i < samples.size(); ++i) {
        auto it = clusters.emplace(samples[i]->getClusterId(), std::make_pair((size_t)0, i)).first;
        ++it->second.first;
    }
    if (clusters.empty()) return shared_ptr<Sample>();
    auto best = clusters.begin();
    for (auto it = clusters.begin(); it != clusters.end(); ++it) {
        if (it->second.first > best->second.first || (it->second.first == best->second.first && it->second.second < best->second.second)) best = it;
    }
    const int clusterId = best->first;
    double weightedSumX = 0;
    double weightedSumY = 0;
    double weightedSumSize = 0;
    double weightedSumVx = 0;
    double weightedSumVy = 0;
    double weightedSumVSize = 0;
    double weightSum = 0;
    for (const shared_ptr<Sample>& sample : samples) {
        if (sample->getClusterId() != clusterId) continue;
        weightedSumX += sample->getWeight() * sample->getX();
        weightedSumY += sample->getWeight() * sample->getY();
        weightedSumSize += sample->getWeight() * sample->getSize();
        weightedSumVx += sample->getWeight() * sample->getVx();
        weightedSumVy += sample->getWeight() * sample->getVy();
        weightedSumVSize += sample->getWeight() * sample->getVSize();
        weightSum += sample->getWeight();
    }
    if (weightSum == 0) return shared_ptr<Sample>();
    double weightedMeanX = weightedSumX / weightSum;
    double weightedMeanY = weightedSumY / weightSum;
    double weightedMeanSize = weightedSumSize / weightSum;
    double weightedMeanVx = weightedSumVx / weightSum;
    double weightedMeanVy = weightedSumVy / weightSum;
    double weightedMeanVSize = weightedSumVSize / weightSum;
    return make_shared<Sample>((int)(weightedMeanX + 0.5), (int)(weightedMeanY + 0.5), (int)(weightedMeanSize + 0.5), (int)(weightedMeanVx + 0.5),
                               (int)(weightedMeanVy + 0.5), (int)(weightedMeanVSize + 0.5));
}

MaxWeightStateExtractor::MaxWeightStateExtractor() {}

shared_ptr<Sample> MaxWeightStateExtractor::extract(const vector<shared_ptr<Sample>>& samples) {   // .cpp:18-30
    shared_ptr<Sample> best;
    double maxWeight = 0;
    for (const shared_ptr<Sample>& sample : samples) {
        if (sample->getWeight() > maxWeight) {
            maxWeight = sample->getWeight();
            best = sample;
        }
    }
    if (maxWeight > 0 && best->isTarget()) return best;
    return shared_ptr<Sample>();
}

// One generation on the host, as fd_particles_get and fd_particles_set move it
struct ParticleArrays {
    explicit ParticleArrays(int n) : n(n), x(n), y(n), size(n), vx(n), vy(n), cluster(n), vsize(n), weight(n), score(n), target(n) {}
    static ParticleArrays of(fd_particles* particles) {   // the current generation of the set
        int n = 0;
        check(fd_particles_get(context(), particles, FD_PARTICLES_MAX, &n, nullptr));
        ParticleArrays g(n);
        fd_particles_arrays arrays = g.view();
        check(fd_particles_get(context(), particles, n, &g.n, &arrays));
        return g;
    }
    void set(fd_particles* particles) {
        fd_particles_arrays arrays = view();
        check(fd_particles_set(context(), particles, n, &arrays));
    }
    fd_particles_arrays view() { return {x.data(), y.data(), size.data(), vx.data(), vy.data(), vsize.data(), weight.data(), score.data(), target.data(), cluster.data()}; }
    int n;
    vector<int32_t> x, y, size, vx, vy, cluster;
    vector<float> vsize;
    vector<double> weight, score;
    vector<uint8_t> target;
};

// evaluate(image, samples) (:107-168) on a resident particle set.  The heat peak is read before the samples are scored only where
// the branch needs it first (target lost); a re-initialisation downloads the generation, rewrites it with the draws of the generic
// route and scores it again.
void ExtendedHogBasedMeasurementModel::evaluateResident(shared_ptr<imageprocessing::VersionedImage> image, fd_particles* particles, fd_particles_info& info) {
    update(image);
    const double a = classifier->getLogisticA(), b = classifier->getLogisticB(), threshold = classifier->getSvm()->getThreshold();
    auto score = [&](int mode) {
        check(fd_particles_evaluate(context(), particles, useSlidingWindow ? 0 : 1, Sample::getAspectRatio()));
        check(fd_particles_weigh(context(), particles, a, b, threshold, mode, rejectionThreshold));
        ++fusedEvaluations;
    };
    const int mode = targetLost ? FD_PARTICLES_TARGET_LOST : (useSlidingWindow ? FD_PARTICLES_SLIDING_WINDOW : FD_PARTICLES_ALL_TARGETS);
    if (!useSlidingWindow) {
        score(mode);
        check(fd_particles_state(context(), particles, &info));
        return;
    }
    // the generation on the host, rewritten by f, and back
    auto rewrite = [&](const std::function<void(int, fd_particles_arrays&)>& f) {
        ParticleArrays generation = ParticleArrays::of(particles);
        fd_particles_arrays arrays = generation.view();
        f(generation.n, arrays);
        generation.set(particles);
    };
    std::pair<double, cv::Rect> peak;
    auto reinitialize = [&]() {
        int clusterId = Sample::getNextClusterId();
        rewrite([&](int n, fd_particles_arrays& s) {
            for (int i = 0; i < n; ++i) {   // the draws and the double -> int conversions of the setters, as evaluate(image, samples) has them
                s.x[i] = peak.second.x + peak.second.width / 2 + 0.2 * peak.second.width * normalDistribution(generator);
                s.y[i] = peak.second.y + peak.second.height / 2 + 0.2 * peak.second.width * normalDistribution(generator);
                s.size[i] = peak.second.width * (1 + 0.2 * normalDistribution(generator));
                s.vx[i] = 0.1 * peak.second.width * normalDistribution(generator);
                s.vy[i] = 0.1 * peak.second.width * normalDistribution(generator);
                s.vsize[i] = 1 + 0.1 * normalDistribution(generator);
                s.cluster_id[i] = clusterId;
            }
        });
        score(mode);
    };
    if (targetLost) {
        peak = getHeatPeak();
        double peakScore = peak.first;
        if (classifier->getSvm()->classify(peakScore) && (!conservativeReInit || peakScore > adaptationThreshold)) {
            reinitialize();
        } else {
            rewrite([&](int n, fd_particles_arrays& s) {
                for (int i = 0; i < n; ++i) { s.weight[i] = 0; s.score[i] = 0; s.target[i] = 0; }
            });
        }
        check(fd_particles_state(context(), particles, &info));
        return;
    }
    score(mode);
    check(fd_particles_state(context(), particles, &info));
    peak = getHeatPeak();
    double bestScore = info.best_score;
    double peakScore = peak.first;
    double initialFeaturesScore = classifier->getSvm()->computeHyperplaneDistance(initialFeatures);
    double scoreThreshold = 0.5 * (bestScore + initialFeaturesScore);
    if (conservativeReInit) scoreThreshold = std::max(scoreThreshold, adaptationThreshold);
    if (bestScore < initialFeaturesScore && classifier->getSvm()->classify(peakScore) && peakScore > scoreThreshold) {
        reinitialize();
        check(fd_particles_state(context(), particles, &info));
    }
}

ParticleFrameLoop::ParticleFrameLoop(shared_ptr<Sampler> sampler, shared_ptr<MeasurementModel> measurementModel, shared_ptr<StateExtractor> extractor)
    : samples(), oldSamples(), state(), image(make_shared<imageprocessing::VersionedImage>()), sampler(sampler), measurementModel(measurementModel),
      extractor(extractor) {}

ParticleFrameLoop::~ParticleFrameLoop() { releaseParticles(); }

void ParticleFrameLoop::releaseParticles() {
    if (particles) fd_particles_destroy(particles);
    particles = nullptr;
    particlesOn = nullptr;
}

// exactly that class: a subclass may override what the device route restates, and keeps the generic route
template <class T, class U>
static bool is_exactly(const shared_ptr<U>& p) { return p && typeid(*p) == typeid(T); }

// the SingleClassifierModel a resident frame would evaluate: the model itself, or the one inside a PositionDependentMeasurementModel
static shared_ptr<SingleClassifierModel> resident_single_model(const shared_ptr<MeasurementModel>& model) {
    if (is_exactly<SingleClassifierModel>(model)) return std::static_pointer_cast<SingleClassifierModel>(model);
    if (is_exactly<SelfLearningMeasurementModel>(model)) return nullptr;   // evaluated through the model's own evaluateResident
    if (is_exactly<PositionDependentMeasurementModel>(model)) {
        auto dependent = std::static_pointer_cast<PositionDependentMeasurementModel>(model);
        if (dependent->isUsable() && is_exactly<SingleClassifierModel>(dependent->getMeasurementModel()))
            return std::static_pointer_cast<SingleClassifierModel>(dependent->getMeasurementModel());
    }
    return nullptr;
}

ParticleFrameLoop::ResidentKind ParticleFrameLoop::residentKind() const {
    if (!fd_particles_route_enabled()) return ResidentKind::None;
    if (!is_exactly<ResamplingSampler>(sampler)) return ResidentKind::None;
    auto resampling = std::static_pointer_cast<ResamplingSampler>(sampler);
    if (!is_exactly<LowVarianceSampling>(resampling->getResamplingAlgorithm())) return ResidentKind::None;
    if (!is_exactly<FilteringStateExtractor>(extractor)) return ResidentKind::None;
    if (!is_exactly<WeightedMeanStateExtractor>(std::static_pointer_cast<FilteringStateExtractor>(extractor)->getExtractor())) return ResidentKind::None;
    const size_t old = resident ? (size_t)residentCount : samples.size();
    if (old > FD_PARTICLES_MAX || resampling->getCount() < 0 || resampling->getCount() > FD_PARTICLES_MAX) return ResidentKind::None;
    const bool simple = is_exactly<SimpleTransitionModel>(resampling->getTransitionModel());
    using Family = SingleClassifierModel::ResidentPlan::Family;
    if (examplesModel) {   // PartiallyAdaptiveCondensationTracker: both models resident, or the generic route
        if (!simple || typeid(*examplesModel) != typeid(SelfLearningMeasurementModel)) return ResidentKind::None;
        const Family family = examplesModel->residentPlan().family;
        if (family == Family::None) return ResidentKind::None;
        if (measurementModel == examplesModel) return family == Family::Integral ? ResidentKind::Integral : ResidentKind::Pyramid;
        return is_exactly<WvmSvmModel>(measurementModel) && std::static_pointer_cast<WvmSvmModel>(measurementModel)->residentPossible() ? ResidentKind::WvmSvm
                                                                                                                                     : ResidentKind::None;
    }
    if (is_exactly<ExtendedHogBasedMeasurementModel>(measurementModel)) {
        auto model = std::static_pointer_cast<ExtendedHogBasedMeasurementModel>(measurementModel);
        if (!simple || !model->native() || !model->isUsable()) return ResidentKind::None;
        if (model->getAdaptation() != ExtendedHogBasedMeasurementModel::Adaptation::NONE && model->getAdaptation() != ExtendedHogBasedMeasurementModel::Adaptation::POSITION)
            return ResidentKind::None;
        return ResidentKind::Ehog;
    }
    // OpticalFlowTransitionModel with this model keeps the generic route, as the pyramid families of SingleClassifierModel do
    if (is_exactly<WvmSvmModel>(measurementModel))
        return simple && std::static_pointer_cast<WvmSvmModel>(measurementModel)->residentPossible() ? ResidentKind::WvmSvm : ResidentKind::None;
    const bool flow = is_exactly<OpticalFlowTransitionModel>(resampling->getTransitionModel()) &&
                      std::static_pointer_cast<OpticalFlowTransitionModel>(resampling->getTransitionModel())->residentPossible();
    if (!simple && !flow) return ResidentKind::None;
    const shared_ptr<SingleClassifierModel> single = resident_single_model(measurementModel);
    const Family family = single ? single->residentPlan().family : Family::None;   // on what the extractor holds from the previous frame
    if (family == Family::None) return ResidentKind::None;
    if (family == Family::Integral) return ResidentKind::Integral;
    // a pyramid chain under OpticalFlowTransitionModel keeps the generic route: the library serves that frame (fd_particles_sample_flow,
    // then _evaluate_pyramid), but the route comparison of tracker_app pins `generic` for this combination
    return simple ? ResidentKind::Pyramid : ResidentKind::None;
}

const vector<shared_ptr<Sample>>& ParticleFrameLoop::currentSamples() const {
    if (resident && !materialized) {   // the Sample objects of the resident generation: no ancestors on this route
        const ParticleArrays g = ParticleArrays::of(particles);
        samples.clear();
        const int nextId = Sample::nextClusterId;
        for (int i = 0; i < g.n; ++i) {
            auto sample = make_shared<Sample>(g.x[i], g.y[i], g.size[i], g.vx[i], g.vy[i], g.vsize[i]);
            sample->setWeight(g.weight[i]);
            sample->setScore(g.score[i]);
            sample->setTarget(g.target[i] != 0);
            sample->setClusterId(g.cluster[i]);
            samples.push_back(sample);
        }
        Sample::nextClusterId = nextId;   // building the objects draws no cluster ids
        materialized = true;
    }
    return samples;
}

void ParticleFrameLoop::replaceSamples(const vector<shared_ptr<Sample>>& newSamples) {
    samples = newSamples;
    resident = false;
    materialized = true;
}

// the generation of the generic route (or of initialize) moves to the device
void ParticleFrameLoop::uploadGeneration() {
    ParticleArrays g((int)samples.size());
    residentWeightSum = 0;
    for (int i = 0; i < g.n; ++i) {
        const Sample& s = *samples[i];
        g.x[i] = s.getX(); g.y[i] = s.getY(); g.size[i] = s.getSize(); g.vx[i] = s.getVx(); g.vy[i] = s.getVy(); g.vsize[i] = s.getVSize();
        g.weight[i] = s.getWeight(); g.score[i] = s.getScore(); g.target[i] = s.isTarget(); g.cluster[i] = s.getClusterId();
        residentWeightSum += g.weight[i];
    }
    g.set(particles);
    residentCount = g.n;
    resident = true;
}

// The set this frame needs: bound to `tracker` (ExtendedHogBasedMeasurementModel), or unbound (NULL).  A set on hand that is another one
// -- the model was initialised again and has another tracker handle -- is released, and a generation that lived in it is lost with it
void ParticleFrameLoop::bindParticles(fd_ehog_tracker* tracker) {
    if (particles && particlesOn != tracker) releaseParticles();
    if (particles) return;
    if (resident)
        throw std::logic_error(tracker ? "ParticleFrameLoop: the resident generation was lost with its tracker"
                                       : "ParticleFrameLoop: the resident generation was lost with its particle set");
    if (tracker) check(fd_particles_create(context(), tracker, FD_PARTICLES_MAX, &particles));
    else check(fd_particles_create_unbound(context(), FD_PARTICLES_MAX, &particles));
    particlesOn = tracker;
}

// The bracket of an OpticalFlowTransitionModel around a resident frame; without one (flow NULL) the plain sample call and state.  The
// branch between the flow and its fallback is the device's: both blocks are drawn behind snapshots and the model that did not predict
// gets its snapshot back after the read-back.
struct ResidentFlow {
    ResidentFlow(OpticalFlowTransitionModel* flow, const Mat& data, const shared_ptr<Sample>& state)
        : flow(flow), tracked(flow && flow->beginResident(data, state)),
          fallback(flow ? static_cast<SimpleTransitionModel*>(flow->getFallback().get()) : nullptr) {   // null: the sampler's own
        if (tracked) before = fallback->drawState();
    }
    void sample(fd_particles* particles, const ResamplingSampler::Draws& draws, int copies, int fresh, int firstFreshId) {
        if (tracked) {
            const vector<double>& flowDiffusion = flow->drawResident((size_t)copies);
            check(fd_particles_sample_flow(context(), particles, flow->native(), copies + fresh, copies, draws.u, flowDiffusion.data(), draws.diffusion.data(),
                                           draws.fresh.data(), firstFreshId));
        } else {
            check(fd_particles_sample(context(), particles, copies + fresh, copies, draws.u, draws.diffusion.data(), draws.fresh.data(), firstFreshId));
        }
    }
    // negatives: the state through fd_particles_state_negatives, *count records into `records` (room for max_count)
    void readState(fd_particles* particles, fd_particles_info& info, const fd_particles_negatives_params* negatives = nullptr, int* count = nullptr,
                   fd_particles_negative* records = nullptr) {
        fd_flow_motion_info motion;
        if (negatives)
            check(fd_particles_state_negatives(context(), particles, tracked ? flow->native() : nullptr, negatives, &info, tracked ? &motion : nullptr, count,
                                               records));
        else if (tracked) check(fd_particles_state_flow(context(), particles, flow->native(), &info, &motion));
        else check(fd_particles_state(context(), particles, &info));
        if (!tracked) return;
        flow->endResident(motion);
        if (motion.ok) fallback->restoreDrawState(before);   // the flow predicted: the fallback drew nothing
    }
    OpticalFlowTransitionModel* flow;
    bool tracked;
    SimpleTransitionModel* fallback;
    SimpleTransitionModel::DrawState before;
};

// One frame on the resident set.  The host draws every random number the generic route would draw: the three generators (resampling,
// transition, fresh samples) are separate, so only the order within each matters.
void ParticleFrameLoop::deviceStep() {
    auto resampling = std::static_pointer_cast<ResamplingSampler>(sampler);
    const bool onTracker = lastKind == ResidentKind::Ehog;
    auto ehog = onTracker ? std::static_pointer_cast<ExtendedHogBasedMeasurementModel>(measurementModel) : nullptr;
    bindParticles(onTracker ? ehog->native() : nullptr);
    if (!resident) uploadGeneration();
    const Mat& data = image->getData();
    ResidentFlow flow(dynamic_cast<OpticalFlowTransitionModel*>(resampling->getTransitionModel().get()), data, state);   // Ehog: never one
    const ResamplingSampler::Draws& draws = resampling->drawFrame((size_t)residentCount, residentWeightSum, data.cols, data.rows, flow.fallback);
    const int copies = (int)(draws.diffusion.size() / 3), fresh = (int)(draws.fresh.size() / 3);
    const int firstFreshId = Sample::nextClusterId;
    Sample::nextClusterId += fresh;   // the ids the random samples of the generic route would have drawn, in order
    flow.sample(particles, draws, copies, fresh, firstFreshId);
    fd_particles_info info;
    residentChose = false;
    residentExamples = false;
    residentChosen.clear();
    if (examplesModel) {   // either model evaluates; the adaptive one reads its examples with the state, in the frame's one wait
        if (measurementModel == examplesModel) examplesModel->evaluateResident(image, particles);
        else std::static_pointer_cast<WvmSvmModel>(measurementModel)->evaluateResident(image, particles);
        examplesModel->readExamples(image, particles, info);
        residentExamples = true;
    } else if (onTracker) {   // the model reads the state itself: its re-initialisation needs the best score in the middle
        ehog->evaluateResident(image, particles, info);
    } else {
        if (lastKind == ResidentKind::WvmSvm) std::static_pointer_cast<WvmSvmModel>(measurementModel)->evaluateResident(image, particles);
        else resident_single_model(measurementModel)->evaluateResident(image, particles);
        // exactly that model: its adapt reads of the samples what the device chooses behind the state (a subclass never gets here)
        fd_particles_negatives_params negatives;
        residentChose = is_exactly<PositionDependentMeasurementModel>(measurementModel) &&
                        std::static_pointer_cast<PositionDependentMeasurementModel>(measurementModel)->residentNegatives(negatives);
        if (residentChose) {
            fd_particles_negative records[FD_PARTICLES_NEGATIVES_MAX];
            int count = 0;
            flow.readState(particles, info, &negatives, &count, records);
            const int nextId = Sample::nextClusterId;
            for (int k = 0; k < count; ++k) {
                residentChosen.emplace_back(records[k].x, records[k].y, records[k].size);
                residentChosen.back().setWeight(records[k].weight);
            }
            Sample::nextClusterId = nextId;   // building the objects draws no cluster ids
        } else {
            flow.readState(particles, info);
        }
    }
    residentCount = info.count;
    residentWeightSum = info.weight_sum;
    materialized = false;
    samples.clear();
    oldSamples.clear();
    state = info.found ? make_shared<Sample>(info.x, info.y, info.size, info.vx, info.vy, info.vsize) : shared_ptr<Sample>();
}

void ParticleFrameLoop::step(const Mat& imageData) {
    image->setData(imageData);
    lastKind = residentKind();
    if (lastKind != ResidentKind::None) {
        lastRoute = Route::DEVICE;
        deviceStep();
        return;
    }
    lastRoute = Route::GENERIC;
    currentSamples();   // a generation that lived on the device comes back as Sample objects
    resident = false;
    samples.swap(oldSamples);
    samples.clear();
    sampler->sample(oldSamples, samples, image->getData(), state);
    measurementModel->evaluate(image, samples);
    state = extractor->extract(samples);
}

CondensationTracker::CondensationTracker(shared_ptr<Sampler> sampler, shared_ptr<MeasurementModel> measurementModel, shared_ptr<StateExtractor> extractor)
    : ParticleFrameLoop(sampler, measurementModel, extractor) {}

boost::optional<cv::Rect> CondensationTracker::process(const Mat& imageData) {   // .cpp:35-47
    step(imageData);
    if (state) return boost::optional<cv::Rect>(state->getBounds());
    return boost::optional<cv::Rect>();
}

PartiallyAdaptiveCondensationTracker::PartiallyAdaptiveCondensationTracker(shared_ptr<Sampler> sampler, shared_ptr<MeasurementModel> initialMeasurementModel,
                                                                           shared_ptr<AdaptiveMeasurementModel> measurementModel, shared_ptr<StateExtractor> extractor)
    : ParticleFrameLoop(sampler, initialMeasurementModel, extractor), initialModel(initialMeasurementModel), adaptiveModel(measurementModel) {
    examplesModel = std::dynamic_pointer_cast<SelfLearningMeasurementModel>(measurementModel);   // null: every frame takes the generic route
}

boost::optional<cv::Rect> PartiallyAdaptiveCondensationTracker::process(const Mat& imageData) {   // .cpp:40-65
    usedAdaptiveModel = useAdaptiveModel && adaptiveModel->isUsable();
    measurementModel = usedAdaptiveModel ? shared_ptr<MeasurementModel>(adaptiveModel) : initialModel;
    const shared_ptr<SelfLearningMeasurementModel> reads = examplesModel;
    if (!useAdaptiveModel || !examplesModel) {   // nothing reads examples: the frame is the measurement model's own
        examplesModel.reset();
    }
    step(imageData);
    examplesModel = reads;
    if (useAdaptiveModel) {
        if (examplesRead()) reads->adaptResident(image);
        else if (state) adaptiveModel->adapt(image, currentSamples(), *state);
        else adaptiveModel->adapt(image, currentSamples());
    }
    if (state) return boost::optional<cv::Rect>(state->getBounds());
    return boost::optional<cv::Rect>();
}

void PartiallyAdaptiveCondensationTracker::setUseAdaptiveModel(bool useAdaptive) {
    useAdaptiveModel = useAdaptive;
    if (!useAdaptive) adaptiveModel->reset();
}

AdaptiveCondensationTracker::AdaptiveCondensationTracker(shared_ptr<Sampler> sampler, shared_ptr<AdaptiveMeasurementModel> measurementModel,
                                                         shared_ptr<StateExtractor> extractor, int initialCount)
    : ParticleFrameLoop(sampler, measurementModel, extractor), initialCount(initialCount), adapted(false), adaptiveModel(measurementModel), validators() {
    shared_ptr<StateValidator> validator = std::dynamic_pointer_cast<StateValidator>(measurementModel);
    if (validator) addValidator(validator);
}

void AdaptiveCondensationTracker::reset() { adaptiveModel->reset(); }

boost::optional<cv::Rect> AdaptiveCondensationTracker::initialize(const Mat& imageData, const cv::Rect& positionData) {   // .cpp:50-65
    image->setData(imageData);
    replaceSamples(vector<shared_ptr<Sample>>());
    Sample::setAspectRatio(positionData.width, positionData.height);
    state = make_shared<Sample>(positionData.x + positionData.width / 2, positionData.y + positionData.height / 2, positionData.width);
    sampler->init(imageData);
    adaptiveModel->initialize(image, *state);
    if (adaptiveModel->isUsable()) {
        vector<shared_ptr<Sample>> initial;
        for (int i = 0; i < initialCount; ++i) initial.push_back(state);
        replaceSamples(initial);
    }
    if (adaptiveModel->isUsable()) return boost::optional<cv::Rect>(state->getBounds());
    return boost::optional<cv::Rect>();
}

boost::optional<cv::Rect> AdaptiveCondensationTracker::process(const Mat& imageData) {   // .cpp:67-95
    if (!adaptiveModel->isUsable()) throw std::runtime_error("AdaptiveCondensationTracker: Is not usable (was not initialized or was resetted)");
    step(imageData);
    // validate target state; the measurement model looks at the state alone and ClassificationBasedStateValidator ignores its samples
    // argument, any other validator gets the samples
    if (state) {
        for (shared_ptr<StateValidator>& validator : validators) {
            const bool isModel = std::dynamic_pointer_cast<StateValidator>(measurementModel) == validator;
            static const vector<shared_ptr<Sample>> none;
            const bool onDevice = (samplesUnread() && isModel) || (samplesOnDeviceOnly() && is_exactly<ClassificationBasedStateValidator>(validator));
            if (!validator->isValid(*state, onDevice ? none : currentSamples(), image)) {
                state.reset();
                break;
            }
        }
    }
    // update model: ExtendedHogBasedMeasurementModel::adapt does not read the samples; PositionDependentMeasurementModel::adapt reads
    // what the device frame has brought back with the state, and nothing without a state
    static const vector<shared_ptr<Sample>> unread;
    if (negativesChosen()) {
        if (state) adapted = std::static_pointer_cast<PositionDependentMeasurementModel>(measurementModel)->adaptResident(image, *state, chosenNegatives());
        else adapted = adaptiveModel->adapt(image, unread);
    } else {
        const vector<shared_ptr<Sample>>& forAdapt = samplesUnread() ? unread : currentSamples();
        if (state) adapted = adaptiveModel->adapt(image, forAdapt, *state);
        else adapted = adaptiveModel->adapt(image, forAdapt);
    }
    if (state) return boost::optional<cv::Rect>(state->getBounds());
    return boost::optional<cv::Rect>();
}

bool AdaptiveCondensationTracker::hasAdapted() { return adapted; }
shared_ptr<Sample> AdaptiveCondensationTracker::getState() { return state; }
const vector<shared_ptr<Sample>>& AdaptiveCondensationTracker::getSamples() const { return currentSamples(); }
shared_ptr<Sampler> AdaptiveCondensationTracker::getSampler() { return sampler; }
void AdaptiveCondensationTracker::setSampler(shared_ptr<Sampler> sampler) { this->sampler = sampler; }
void AdaptiveCondensationTracker::addValidator(shared_ptr<StateValidator> validator) { validators.push_back(validator); }

}  // namespace condensation
