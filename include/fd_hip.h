/* include/fd_hip.h -- C ABI of the MI355X-native FeatureDetection hot path (libfd_hip.so).
 *
 * The reference (elador/FeatureDetection) has no FFI/plugin layer: its extension points are the
 * C++ abstract classes wired by shared_ptr in each app's main().  The drop-in boundary is therefore
 *   C++ subclass of the reference interface (host/ in this repo)  ->  this C ABI  ->  HIP kernels.
 * Every entry point names the reference interface (file:line) whose work it performs.
 *
 * Conventions: opaque handles, int status (0 = FD_OK), caller-owned buffers, no exceptions across
 * the ABI, one HIP stream per context (thread-compatible, not thread-safe -- like the reference,
 * whose const methods mutate scratch buffers, WvmClassifier.hpp:129-130).  Pointers named dev_* are
 * device (HBM) pointers, everything else is host memory.  The library has NO CPU fallback: every
 * compute entry point fails with FD_ERR_HIP when no gfx950 device is usable.
 */
#ifndef FD_HIP_H_
#define FD_HIP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    FD_OK = 0,
    FD_ERR_INVALID_ARGUMENT = 1, /* std::invalid_argument in the reference */
    FD_ERR_RUNTIME = 2,          /* std::runtime_error */
    FD_ERR_LOGIC = 3,            /* std::logic_error */
    FD_ERR_HIP = 4,              /* HIP runtime failure / no device */
    FD_ERR_CAPACITY = 5,         /* caller buffer too small; required count is still reported */
    FD_ERR_DEVICE_CAPACITY = 6   /* a device-side buffer of the library overflowed (FD_WVM_POS_CAP / FD_WVM_DEEP_CAP in the
                                    environment raise them); a larger caller buffer does not help */
};

typedef struct fd_ctx fd_ctx;
typedef struct fd_pyramid fd_pyramid;
typedef struct fd_wvm fd_wvm;
typedef struct fd_svm fd_svm;
typedef struct fd_sdm fd_sdm;

/* ---- context ------------------------------------------------------------------------------ */
/* hip_stream: an existing hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream),
 * or NULL to create a private stream. */
int fd_ctx_create(int device_id, void* hip_stream, fd_ctx** out);
int fd_device_count(int* n);   /* visible HIP devices (a multi-rank launcher checks its --gpus against it before any rank starts) */
void fd_ctx_destroy(fd_ctx* ctx);
/* Optional: creates the streams the batch entry points otherwise create on first use (eight batch streams, the high-priority stream of
 * the SVM stage, an auxiliary one) now.  The HIP runtime deals streams to its hardware queues (four by default) in creation order, so
 * an application that creates other streams in between gets a different -- and, measured, up to 12 % slower -- mapping for them; calling
 * this straight after fd_ctx_create makes the mapping the same in every run. */
int fd_ctx_warm_streams(fd_ctx* ctx);
const char* fd_last_error(const fd_ctx* ctx); /* valid until the next failing call on ctx */
int fd_ctx_synchronize(fd_ctx* ctx);
const char* fd_version(void);

/* ---- image pyramid: imageprocessing::ImagePyramid (ImagePyramid.cpp:67-92 ctors, :116-128 update,
 *      :170-198 createLayers) with the GrayscaleFilter image filter (GrayscaleFilter.cpp:18-24) ---- */
int fd_pyramid_create(fd_ctx* ctx, int octave_layer_count, double min_scale, double max_scale, fd_pyramid** out);
int fd_pyramid_create_inc(fd_ctx* ctx, double incremental_scale, double min_scale, double max_scale, fd_pyramid** out);
void fd_pyramid_destroy(fd_pyramid* p);
/* Layer filters (ImagePyramid::addLayerFilter, ImagePyramid.cpp:112-114):
 *  FD_LAYER_NONE       gray layers (u8, 1 channel)
 *  FD_LAYER_GRADBIN    GradientFilter(grad_kernel, blur) -> GradientBinningFilter(bins, signed, interpolate)
 *                      (GradientFilter.cpp:16-59, GradientBinningFilter.cpp:18-93); 2 or 4 channels.
 *                      grad_kernel: 1, 3, 5, 7 or FD_GRAD_SCHARR (the reference's CV_SCHARR = -1);
 *                      blur: fd_pyramid_set_gradient_blur (blurKernelSize of the reference's constructor, default 0 = none)
 *  FD_LAYER_LBP        LbpFilter(lbp_type) (LbpFilter.cpp:56-85); 1 channel
 *  FD_LAYER_GRADMAG_LBP  GradientFilter(grad_kernel, blur) -> imageprocessing::GradientMagnitudeFilter (GradientMagnitudeFilter.hpp:39-50,
 *                      CV_8U: saturate_cast<uchar>(sqrt(x^2 + y^2)), x = gx - 127, y = gy - 127) -> LbpFilter(lbp_type): the layer
 *                      filters of the "glbp" feature type (HeadTracking.cpp:199-254); 1 channel, one kernel per update, the
 *                      magnitudes never reach memory.  bins, signed_gradients and interpolate are ignored. */
enum { FD_LAYER_NONE = 0, FD_LAYER_GRADBIN = 1, FD_LAYER_LBP = 2, FD_LAYER_GRADMAG_LBP = 3 };
enum { FD_LBP8 = 0, FD_LBP8_UNIFORM = 1, FD_LBP4 = 2, FD_LBP4_ROTATED = 3 };
enum { FD_GRAD_SCHARR = -1 };
int fd_pyramid_set_layer_filter(fd_pyramid* p, int kind, int bins, int signed_gradients, int interpolate,
                                int grad_kernel, int lbp_type);
int fd_pyramid_set_gradient_blur(fd_pyramid* p, int blur_kernel);
/* Image filters (ImagePyramid::addImageFilter, ImagePyramid.cpp:106-110,171), applied to the image before the layers are built:
 *  FD_IMAGE_GRAY            GrayscaleFilter (default)
 *  FD_IMAGE_GREYWORLD_GRAY  GreyWorldNormalizationFilter -> GrayscaleFilter (GreyWorldNormalizationFilter.cpp:20-71 on the BGR
 *                           image, then the gray conversion); the image must have 3 channels
 * Holds for every later update of the pyramid through any entry point (fd_pyramid_update, fd_pyramid_update_frames,
 * fd_detect_five_stage_image, the image of a fd_five_stage_job); every frame of a multi-frame pyramid is normalised with its own
 * statistics.  Does not change the layout; may be set or reset between updates.  The statistics and the scales stay on the device:
 * an update with the filter returns without waiting, like one without. */
enum { FD_IMAGE_GRAY = 0, FD_IMAGE_GREYWORLD_GRAY = 1 };
int fd_pyramid_set_image_filter(fd_pyramid* p, int kind);
int fd_pyramid_image_filter(const fd_pyramid* p);
/* channels 1 (gray) or 3 (BGR, interleaved).  is_device != 0: image already resident in HBM. */
int fd_pyramid_update(fd_pyramid* p, const uint8_t* image, int width, int height, int channels, int is_device);
int fd_pyramid_octave_layer_count(const fd_pyramid* p);
double fd_pyramid_incremental_scale(const fd_pyramid* p);
int fd_pyramid_layer_count(const fd_pyramid* p);
/* ImagePyramidLayer.hpp:34-35: index, theoretical scale, size; channels of the filtered layer */
int fd_pyramid_layer_info(const fd_pyramid* p, int i, int* index, double* scale, int* width, int* height, int* channels);
/* copy the (filtered) layer i to host: width*height*channels bytes */
int fd_pyramid_layer_download(fd_pyramid* p, int i, uint8_t* host_dst);
/* Layer sub-range and default region of interest of every window enumeration that follows on this pyramid -- the firstLayer /
 * lastLayer / stepLayer / roi arguments of DirectPyramidFeatureExtractor::extract(stepX, stepY, roi, firstLayer, lastLayer,
 * stepLayer) (:75-123), for every extraction / detection entry point (also those without a roi argument), and the layer range of
 * an ImagePyramid built on another pyramid (ImagePyramid.cpp:100-104,200-235: same layers, scale factors within [min, max]).
 * first_layer / last_layer: pyramid layer indices, -1 = open; step_layer >= 1 counts over the kept layers from the first one;
 * roi: {x, y, w, h} or NULL (none; an explicit roi argument of a call takes precedence).  Reset with (-1, -1, 1, NULL). */
int fd_pyramid_select(fd_pyramid* p, int first_layer, int last_layer, int step_layer, const int* roi);
/* ImagePyramid(shared_ptr<ImagePyramid> pyramid, minScale, maxScale) (ImagePyramid.cpp:100-104,200-235): a pyramid built on another
 * one shares its layers but exposes only those inside its scale range; its getLayers() -- and therefore the layer step of
 * DirectPyramidFeatureExtractor::extract (:99) -- starts at the first layer of that range.  first_layer / last_layer: pyramid layer
 * indices of the range, -1 = open.  Applies to the window enumerations that follow; reset with (-1, -1). */
int fd_pyramid_select_view(fd_pyramid* p, int first_layer, int last_layer);
/* Window enumeration of DirectPyramidFeatureExtractor::extract(stepX, stepY, roi) (:75-123).
 * roi = {x,y,w,h} or NULL (whole image).  rows of out: {layerPos, lx, ly, cx, cy, ow, oh}. */
int fd_pyramid_window_count(const fd_pyramid* p, int patch_w, int patch_h, int step_x, int step_y,
                            const int* roi, int64_t* count);
int fd_pyramid_windows(const fd_pyramid* p, int patch_w, int patch_h, int step_x, int step_y, const int* roi,
                       int32_t* out, int64_t cap, int64_t* count);

/* Stand-alone image filters (ImageFilter::applyTo): GreyWorldNormalizationFilter.cpp:20-71 */
int fd_greyworld(fd_ctx* ctx, const uint8_t* bgr, int width, int height, uint8_t* dst, int is_device);
/* HistEq64Filter::applyTo (HistEq64Filter.cpp:32-125) on n contiguous patches of w*h bytes (host buffers) */
int fd_histeq64_batch(fd_ctx* ctx, const uint8_t* patches, int64_t n, int w, int h, uint8_t* dst);

/* Stand-alone ImageFilter::applyTo(const Mat&) forms (ImageFilter.hpp:18-57) of the filters the detection kernels fuse into the
 * pyramid / feature kernels; host buffers in, host buffers out.
 *  fd_gradient_image          GradientFilter(grad_kernel 1|3|5|7|FD_GRAD_SCHARR, no blur) (GradientFilter.cpp:16-59): CV_8UC1 -> CV_8UC2 (x, y)
 *  fd_gradient_binning_image  GradientBinningFilter(bins, signed, interpolate) (GradientBinningFilter.cpp:62-93): CV_8UC2 -> CV_8UC2
 *                             (bin, weight) or CV_8UC4 (two bins + weights)
 *  fd_lbp_image               LbpFilter(type) (LbpFilter.cpp:56-85): CV_8UC1 -> CV_8UC1 codes */
int fd_gradient_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, int grad_kernel, uint8_t* dst2ch);
/* ... with GradientFilter's blurKernelSize (cv::blur before the derivatives, GradientFilter.cpp:43-46; 0 = none).
 * grad_kernel: 1, 3, 5, 7 or FD_GRAD_SCHARR (CV_SCHARR), as in the reference */
int fd_gradient_filter_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, int grad_kernel, int blur_kernel, uint8_t* dst2ch);
int fd_gradient_binning_image(fd_ctx* ctx, const uint8_t* grad2ch, int width, int height, int bins, int signed_gradients,
                              int interpolate, uint8_t* dst);
int fd_lbp_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, int lbp_type, uint8_t* dst);
/* imageprocessing::GradientMagnitudeFilter::applyTo (GradientMagnitudeFilter.hpp:39-50) on a CV_8UC2 gradient image (the output of
 * fd_gradient_image): CV_8UC1 magnitudes, the square root rounded to nearest (an exact integer function, at most 181) */
int fd_gradient_magnitude_image(fd_ctx* ctx, const uint8_t* grad2ch, int width, int height, uint8_t* dst);

/* ---- classification::WvmClassifier / ProbabilisticWvmClassifier --------------------------------
 * Field meaning as in WvmClassifier.hpp / the Matlab loader WvmClassifier.cpp:352-769 (values already
 * converted to the 0..255 domain as the loader does). */
typedef struct {
    int32_t filter_w, filter_h;  /* filter_size_x/y */
    int32_t num_filters;         /* numLinFilters */
    int32_t num_used;            /* numUsedFilters (0 or > num_filters => num_filters, :151-158) */
    int32_t num_per_level;       /* numFiltersPerLevel */
    float basis_param;           /* basisParam */
    float bias;                  /* lin_thresholds[i] == bias for all i (:567-570) */
    const float* thresholds;     /* hierarchicalThresholds[num_filters] (limitReliabilityFilter already added) */
    const float* hk_weights;     /* [num_filters][num_filters] row-major; hk_weights[k][p], p <= k */
    const double* pp;            /* app_rsv_convol[num_filters] */
    const int32_t* val_off;      /* [num_filters+1]; grey values of filter k are val[val_off[k]..val_off[k+1]) */
    const double* val;           /* area[k]->val[v] */
    const int32_t* rec_off;      /* [val_off[num_filters]+1]; rects of (k,v) */
    const uint8_t* rects;        /* {x1,y1,x2,y2} inclusive patch coordinates, 4 bytes per rect */
    double logistic_a, logistic_b; /* ProbabilisticWvmClassifier.hpp:36 */
    int32_t num_vals, num_rects; /* lengths of val / rects (entries), so that a truncated model is rejected instead of read out
                                  * of bounds; 0 = not stated (offsets are still checked for order) */
} fd_wvm_model;
int fd_wvm_create(fd_ctx* ctx, const fd_wvm_model* model, fd_wvm** out);
void fd_wvm_destroy(fd_wvm* m);
/* WvmClassifier::computeHyperplaneDistance (WvmClassifier.cpp:100-149) for n feature vectors (already
 * HistEq64-filtered filter_w x filter_h u8 patches, contiguous, host buffers): (lastLevel, fout) each.
 * Backs the per-Mat BinaryClassifier::classify / ProbabilisticClassifier::getProbability. */
int fd_wvm_eval_batch(fd_ctx* ctx, const fd_wvm* m, const uint8_t* patches, int64_t n, int32_t* out_level, float* out_score);

/* ---- classification::SvmClassifier / ProbabilisticSvmClassifier with Kernel{Linear,Polynomial,Rbf,HIK} */
enum { FD_KERNEL_LINEAR = 0, FD_KERNEL_POLY = 1, FD_KERNEL_RBF = 2, FD_KERNEL_HIK = 3 };
enum { FD_DTYPE_U8 = 0, FD_DTYPE_F32 = 1 };
typedef struct {
    int32_t kernel;       /* FD_KERNEL_* */
    double p0, p1, p2;    /* rbf: gamma; poly: alpha, constant, degree */
    int32_t num_sv, dim;
    int32_t dtype;        /* FD_DTYPE_* of the support vectors (and of the feature vectors) */
    const void* support_vectors; /* [num_sv][dim] */
    const float* coefficients;   /* [num_sv] */
    float bias, threshold;       /* VectorMachineClassifier.hpp */
    double logistic_a, logistic_b;
} fd_svm_model;
int fd_svm_create(fd_ctx* ctx, const fd_svm_model* model, fd_svm** out);
void fd_svm_destroy(fd_svm* m);
/* SvmClassifier::computeHyperplaneDistance (SvmClassifier.cpp:55-60) for n feature vectors (host buffers).
 * Backs the per-Mat BinaryClassifier::classify / ProbabilisticClassifier::getProbability. */
int fd_svm_distance_batch(fd_ctx* ctx, const fd_svm* m, const void* features, int64_t n, double* out_distance);

/* ---- detection ------------------------------------------------------------------------------ */
typedef struct {
    int32_t cx, cy, w, h;   /* imageprocessing::Patch centre and size in the original image (Patch.hpp:64-65) */
    int32_t layer, lx, ly;  /* layer position (pyramid order) and top-left corner inside the layer */
    int32_t level;          /* WVM: last evaluated filter (WvmClassifier.cpp:149); else -1 */
    int32_t positive;       /* ClassifiedPatch::isPositive */
    float score;            /* WVM fout / (float) SVM hyperplane distance */
    double probability;     /* ClassifiedPatch::getProbability */
} fd_detection;

/* detection::SlidingWindowDetector::detect (SlidingWindowDetector.cpp:40-98) with
 * DirectPyramidFeatureExtractor + HistEq64Filter patch filter + ProbabilisticWvmClassifier
 * (ffpDetectApp.cpp:407-417).  Positives are returned in extraction order.
 * all_level/all_score (host, may be NULL) receive every window's (lastLevel, fout). */
int fd_detect_wvm(fd_ctx* ctx, fd_pyramid* p, const fd_wvm* wvm, int step_x, int step_y, const int* roi,
                  fd_detection* out, int64_t cap, int64_t* count, int32_t* all_level, float* all_score);

/* detection::FiveStageSlidingWindowDetector::detect(image) (:187-320, roi == NULL) and
 * detect(image, roi) (:331-380): WVM -> OverlapElimination(dist, ratio) -> SVM classify ->
 * positives -> [block NMS, no-roi variant only] -> sort.  stage_counts[4] (may be NULL) =
 * {WVM positives, after OE, SVM positives, final}. */
int fd_detect_five_stage(fd_ctx* ctx, fd_pyramid* p, const fd_wvm* wvm, const fd_svm* svm, float oe_dist,
                         float oe_ratio, int step_x, int step_y, const int* roi, fd_detection* out, int cap,
                         int* count, int32_t* stage_counts);
/* detection::Detector::detect(const Mat& image) (Detector.hpp:59; FiveStageSlidingWindowDetector.cpp:187-190 updates its extractor
 * with the image and detects): fd_pyramid_update + fd_detect_five_stage in one call. */
int fd_detect_five_stage_image(fd_ctx* ctx, fd_pyramid* p, const fd_wvm* wvm, const fd_svm* svm, const uint8_t* image, int width,
                               int height, int channels, int image_is_device, float oe_dist, float oe_ratio, int step_x, int step_y,
                               const int* roi, fd_detection* out, int cap, int* count, int32_t* stage_counts);
/* Several frames of identical size in ONE pyramid, for the small-frame regime where the per-frame chain of dependent launches
 * (pyramid, cascade, SVM) bounds the throughput: fd_pyramid_set_frames(p, n) (1..64; gray pyramids only) makes p hold n frames,
 * fd_pyramid_update_frames builds all of them with one launch per pyramid stage, and fd_detect_five_stage_frames runs
 * FiveStageSlidingWindowDetector::detect (:187-320 / :331-380) on every frame with one cascade run and one SVM launch for the
 * whole call.  out: frames x cap_per_frame records (frame f's detections start at out + f * cap_per_frame); counts[frames];
 * stage_counts (may be NULL): frames x 4.  The results equal fd_detect_five_stage on each frame.  The other entry points
 * reject multi-frame pyramids.  fd_pyramid_frame_layer_download copies layer i of frame f to the host. */
int fd_pyramid_set_frames(fd_pyramid* p, int frames);
int fd_pyramid_update_frames(fd_pyramid* p, const uint8_t* const* images, int n, int width, int height, int channels, int is_device);
int fd_pyramid_frame_layer_download(fd_pyramid* p, int frame, int i, uint8_t* host_dst);
int fd_detect_five_stage_frames(fd_ctx* ctx, fd_pyramid* p, const fd_wvm* wvm, const fd_svm* svm, float oe_dist, float oe_ratio,
                                int step_x, int step_y, const int* roi, fd_detection* out, int cap_per_frame, int32_t* counts,
                                int32_t* stage_counts);
/* The same in two halves (frames in flight: further pyramid + WVM + SVM handles on further contexts): begin queues the cascade run
 * of all frames and returns; the host stages (ordering the positives, overlap elimination, the SVM launch, NMS) follow on the
 * library's queue threads as soon as the kernels retire (FD_FRAMES_ASYNC=0: inside end); end waits for them and fills out /
 * counts / stage_counts, reporting whatever they failed with.  Between begin and end the ticket's pyramid, classifier handles
 * and the context's stream must not be used by the caller.  Every ticket must be ended (end releases it, whatever it returns). */
typedef struct fd_five_stage_frames fd_five_stage_frames;
int fd_detect_five_stage_frames_begin(fd_ctx* ctx, fd_pyramid* p, const fd_wvm* wvm, const fd_svm* svm, float oe_dist, float oe_ratio,
                                      int step_x, int step_y, const int* roi, fd_five_stage_frames** ticket);
int fd_detect_five_stage_frames_end(fd_ctx* ctx, fd_five_stage_frames* ticket, fd_detection* out, int cap_per_frame, int32_t* counts,
                                    int32_t* stage_counts);
/* condensation::WvmSvmModel::evaluate(image, samples) (WvmSvmModel.cpp:69-118): the particle-filter
 * measurement model of the tracking apps on an updated gray pyramid.  xywh: n samples {x, y, width, height} (Sample::getX/
 * getY/getWidth/getHeight).  Every sample maps to one window (DirectPyramidFeatureExtractor::extract(x, y, width, height)),
 * weight = 0.5 p_wvm; the (at most 8) most probable WVM positives are re-scored: target = SVM decision, weight = p_wvm p_svm;
 * samples without a patch get weight 0. */
int fd_wvm_svm_evaluate_samples(fd_ctx* ctx, fd_pyramid* p, const fd_wvm* wvm, const fd_svm* svm, int n, const int32_t* xywh,
                                uint8_t* target, double* weight);

/* Several five-stage detectors in one call (the detector loop of ffpDetectApp.cpp:557-600; BASELINE config 3).  All WVM
 * stages are queued first (spread over a few internal streams, so that the small kernels of different jobs overlap);
 * the host-side stages of detector i overlap the GPU work of detectors i+1...  Two jobs may share a pyramid
 * (identical layers) but not a WVM handle.  Per job: count / stage_counts / status are outputs. */
typedef struct {
    fd_pyramid* pyramid;
    const fd_wvm* wvm;
    const fd_svm* svm;
    float oe_dist, oe_ratio;
    int32_t step_x, step_y;
    const int* roi;             /* {x,y,w,h} or NULL */
    fd_detection* out;
    int32_t cap;
    int32_t count;              /* out */
    int32_t stage_counts[4];    /* out */
    int32_t status;             /* out: FD_OK or the job's error code */
    /* optional: update the job's pyramid with this frame first (fd_pyramid_update arguments), on the job's stream;
     * NULL: the pyramid has been updated by the caller.  A pyramid may be updated by one job of a batch only. */
    const uint8_t* image;
    int32_t image_w, image_h, image_channels, image_is_device;
} fd_five_stage_job;
int fd_detect_five_stage_batch(fd_ctx* ctx, fd_five_stage_job* jobs, int n);
/* The same in two halves, for callers that keep more than one frame in flight: begin validates the jobs, queues the optional
 * pyramid updates and all cascades and returns at once; the host stages (read-back, overlap elimination, the SVM stage, NMS) of
 * every job follow on the library's own threads as its cascade completes (FD_BATCH_THREADS of them, shared by all batches in flight;
 * FD_BATCH_ASYNC=0: inside end) and fill out / count / stage_counts of the job; end waits for them and sets every job's status.
 * `jobs` (and the buffers it points to) must stay alive and untouched from begin until end returns -- the library writes to them in
 * between; every batch that has begun must be ended (end also releases the ticket, whatever it returns).
 * Two batches in flight must not share pyramid or WVM handles: their scratch buffers belong to one run at a time. */
typedef struct fd_five_stage_batch fd_five_stage_batch;
int fd_five_stage_batch_begin(fd_ctx* ctx, fd_five_stage_job* jobs, int n, fd_five_stage_batch** ticket);
int fd_five_stage_batch_end(fd_ctx* ctx, fd_five_stage_batch* ticket);

/* detection::OverlapElimination::eliminate (OverlapElimination.cpp:44-105); host-side, deterministic */
int fd_overlap_elimination(const fd_detection* in, int n, float dist, float ratio, int32_t* keep_idx, int* count);
/* nonMaximaSuppression (FiveStageSlidingWindowDetector.cpp:143-184) applied to the probability map that
 * :276-285 builds from the detections (max probability per centre pixel; masked != 0: only entries > 0.3).
 * maxima_xy receives (x, y) pairs in row-major order (cv::findNonZero order); host-side. */
int fd_block_nms(const fd_detection* in, int n, int image_w, int image_h, int sz, int masked, int32_t* maxima_xy,
                 int cap_pairs, int* count);

/* Single-stage SlidingWindowDetector with the HOG feature chain of benchmarkApp
 * (BenchmarkRunner.cpp:118-126,235-242): pyramid layer filter FD_LAYER_GRADBIN, patch filter
 * HogFilter(bins, cell, block, interpolate=false, signedAndUnsigned) (HogFilter.cpp:58-122) and a
 * ProbabilisticSvmClassifier on the f32 feature vectors.
 * all_distance (host, may be NULL): every window's hyperplane distance, extraction order. */
typedef struct {
    int32_t patch_w, patch_h, step_x, step_y;
    int32_t bins, cell_size, block_size, signed_and_unsigned;
} fd_hog_params;
int fd_hog_feature_length(const fd_hog_params* hp);
int fd_detect_hog_svm(fd_ctx* ctx, fd_pyramid* p, const fd_svm* svm, const fd_hog_params* hp, fd_detection* out,
                      int64_t cap, int64_t* count, double* all_distance);
/* The same in two halves, for callers that keep more than one frame in flight (one context per frame in flight: a context's
 * scratch buffers belong to one run at a time).  begin queues pyramid-layer reads, HOG tiles, the SVM, the positive selection
 * and the read-back of the positives on the context's stream and returns at once; end waits, orders the positives by
 * extraction order and fills out / count.  Every ticket must be ended (end releases it, whatever it returns). */
typedef struct fd_hog_svm_ticket fd_hog_svm_ticket;
int fd_detect_hog_svm_begin(fd_ctx* ctx, fd_pyramid* p, const fd_svm* svm, const fd_hog_params* hp, fd_hog_svm_ticket** ticket);
int fd_detect_hog_svm_end(fd_ctx* ctx, fd_hog_svm_ticket* ticket, fd_detection* out, int64_t cap, int64_t* count);
/* FeatureExtractor::extract for every window: n_windows x feature_length floats to host (tests) */
int fd_extract_hog(fd_ctx* ctx, fd_pyramid* p, const fd_hog_params* hp, float* features, int64_t cap_windows,
                   int64_t* count);

/* detection::NonMaximumSuppression::eliminateRedundantDetections (NonMaximumSuppression.cpp:27-118):
 * IoU clustering around the best remaining detection; maximum_type 0 MAX_SCORE, 1 AVERAGE, 2 WEIGHTED_AVERAGE.  Host only.
 * out: room for n boxes.  FD_ERR_RUNTIME for an overlap threshold > 1 (the reference does not terminate). */
typedef struct {
    float score;
    int32_t x, y, w, h;   /* cv::Rect bounds */
} fd_box;
int fd_nms_iou(const fd_box* in, int n, double overlap_threshold, int maximum_type, fd_box* out, int* count);

/* imageprocessing::filtering::FhogFilter(cellSize, unsignedBinCount, interpolateBins, interpolateCells, alpha)
 * (FhogFilter.cpp:20-132, FhogFilter.hpp:120-207; descriptors by FhogAggregationFilter.cpp:38-168) on CV_8UC1 images:
 * rows = height / cell_size, cols = width / cell_size cells of 3 * unsigned_bins + 4 floats (2B signed, B unsigned
 * orientation features, 4 energy features).  Reference defaults: 8, 9, false, true, 0.2 (FhogFilter.hpp:55-56). */
typedef struct {
    int32_t cell_size, unsigned_bins, interpolate_bins, interpolate_cells;
    float alpha;
} fd_fhog_params;
int fd_fhog_size(const fd_fhog_params* fp, int width, int height, int* rows, int* cols, int* channels);
/* gray: host image (width * height bytes); out: rows * cols * channels floats (host) */
int fd_fhog_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, const fd_fhog_params* fp, float* out);
/* the same for CV_8UC1 (channels 1) or CV_8UC3 (channels 3) host images: with three channels every pixel votes with the channel
 * of the largest gradient magnitude (getBinCoefficients<false>, FhogFilter.hpp:144-172); image: width * height * channels bytes */
int fd_fhog_image_channels(fd_ctx* ctx, const uint8_t* image, int width, int height, int channels, const fd_fhog_params* fp, float* out);
/* the same on kept layer `layer` of an updated gray pyramid (the layer filter of AggregatedFeaturesExtractor's feature pyramid) */
int fd_pyramid_fhog_layer(fd_ctx* ctx, fd_pyramid* p, int layer, const fd_fhog_params* fp, float* out);

/* imageprocessing::CompleteExtendedHogFilter(cellSize, binCount, signedGradients, unsignedGradients, interpolateBins,
 * interpolateCells, alpha) (CompleteExtendedHogFilter.cpp:19-303) on CV_8UC1 images: rows = height / cell_size,
 * cols = width / cell_size cells of bin_count (+ bin_count / 2 when both gradient kinds are set) + 4 floats, in the order
 * [bins][unsigned halves][4 energy features].  The central differences clamp at the area the cells cover, not at the image
 * edge.  Reference defaults: 8, 18, true, true, false, true, 0.2 (CompleteExtendedHogFilter.hpp:49-50).  Invalid: neither
 * gradient kind, both kinds with an odd bin_count, cell_size < 1, bin_count < 1 (this backend: bin_count <= 36). */
typedef struct {
    int32_t cell_size, bin_count, signed_gradients, unsigned_gradients, interpolate_bins, interpolate_cells;
    float alpha;
} fd_cehog_params;
/* host only; an image smaller than a cell gives rows or cols 0 */
int fd_cehog_size(const fd_cehog_params* fp, int width, int height, int* rows, int* cols, int* channels);
/* host only (no context, no device): the gradient look-up table of the constructor (:31-58), 512 * 512 entries each, index
 * dx * 512 + dy with dx, dy the central differences + 256.  Without bin interpolation index2 = index1, weight2 = 0.  Any output
 * may be NULL. */
int fd_cehog_gradient_lut(const fd_cehog_params* fp, int32_t* index1, int32_t* index2, float* weight1, float* weight2);
/* applyTo: gray host image (width * height bytes) -> rows * cols * channels floats (host).  FD_ERR_INVALID_ARGUMENT for an image
 * smaller than a cell. */
int fd_cehog_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, const fd_cehog_params* fp, float* out);
/* the same on kept layer `layer` of an updated gray pyramid (the layer filter of ExtendedHogBasedMeasurementModel's feature pyramid) */
int fd_pyramid_cehog_layer(fd_ctx* ctx, fd_pyramid* p, int layer, const fd_cehog_params* fp, float* out);

/* The per-frame work of condensation::ExtendedHogBasedMeasurementModel with a CompleteExtendedHogFilter
 * (ExtendedHogBasedMeasurementModel.cpp:97-213,243-265,434-456,621-652): the gray pyramid of
 * ExtendedHogFeatureExtractor::createPyramid((cell_cols + 2) * cell, (cell_cols + 2) * min_width / cell_cols,
 * (cell_cols + 2) * max_width / cell_cols, octave_layer_count) (ExtendedHogFeatureExtractor.cpp:32-41,76-84), the filter on every
 * layer (feature pyramid), and, once an SVM is set, the heat pyramid: ConvolutionFilter.cpp:27-43 with the weight vector as kernel,
 * anchor at the kernel centre (cell_cols / 2, cell_rows / 2), BORDER_CONSTANT 0, delta = -bias; heat layers have the size of their
 * feature layers.  The caller supplies the linear SVM's weight vector and bias (fd_ehog_tracker_set_svm) or trains them on the
 * device (fd_ehog_tracker_train_svm). */
typedef struct fd_ehog_tracker fd_ehog_tracker;
typedef struct {
    fd_cehog_params filter;
    int32_t cell_cols, cell_rows;        /* window size in cells */
    int32_t octave_layer_count;
    int32_t min_width, max_width;        /* target widths in pixels the pyramid has to cover */
} fd_ehog_tracker_params;
typedef struct {
    int32_t index;            /* ImagePyramidLayer::getIndex() */
    int32_t width, height;    /* gray layer in pixels */
    int32_t rows, cols;       /* feature / heat layer in cells */
    int32_t reserved;
    double scale;             /* getScaleFactor() */
} fd_ehog_layer;
/* Host only (no context, no device): the layers a handle with these parameters builds for a width x height image.
 * FD_ERR_RUNTIME when fewer than two layers remain (fd_ehog_tracker_update reports the same: the feature pyramid is an
 * ImagePyramid built on another, ImagePyramid.cpp:238-239; *n is set), FD_ERR_CAPACITY when cap is too small (*n is set). */
int fd_ehog_tracker_plan_layers(const fd_ehog_tracker_params* prm, int width, int height, fd_ehog_layer* out, int cap, int* n);
int fd_ehog_tracker_create(fd_ctx* ctx, const fd_ehog_tracker_params* prm, fd_ehog_tracker** out);
void fd_ehog_tracker_destroy(fd_ehog_tracker* t);
/* update(image): gray pyramid, feature layers and, once an SVM is set, heat layers.  image as fd_pyramid_update. */
int fd_ehog_tracker_update(fd_ctx* ctx, fd_ehog_tracker* t, const uint8_t* image, int width, int height, int channels, int is_device);
/* the single support vector, [cell_rows][cell_cols][channels], and the bias (:339-340).  On an updated handle the heat layers
 * of the current frame are rebuilt with it. */
int fd_ehog_tracker_set_svm(fd_ctx* ctx, fd_ehog_tracker* t, const float* weights, float bias);
/* evaluate(Sample&) with the sliding window (:189-205) for n samples {x, y, width, height}: the window is that of
 * CellBasedPyramidFeatureExtractor (.cpp:58-69; DirectPyramidFeatureExtractor.cpp:67-73,133-143), the score the heat value at
 * (by + cell_rows / 2, bx + cell_cols / 2).  Samples without a patch: valid 0, score 0.  FD_ERR_RUNTIME before an update or
 * before an SVM is set (also _heat_peak, _heat_maxima, _heat_layer). */
int fd_ehog_tracker_evaluate_samples(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* xywh, uint8_t* valid, float* score);
/* the same windows: cell_rows * cell_cols * channels floats each (zeros without a patch) */
int fd_ehog_tracker_extract_cells(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* xywh, uint8_t* valid, float* features);
/* ExtendedHogFeatureExtractor::extract (ExtendedHogFeatureExtractor.cpp:95-143): the size widened by (cells + 2) / cells, the
 * layer by patchWidth / width, bounds up to one cell outside the layer (mirrored), the filter on the (cell_cols + 2) * cell x
 * (cell_rows + 2) * cell patch, the inner cells returned.  score (may be NULL; needs an SVM): -bias + dot(features, weights), the
 * double sum in element order of SvmClassifier::computeHyperplaneDistance with a LinearKernel.  One wavefront per sample with the
 * patch in LDS: FD_ERR_INVALID_ARGUMENT when fd_ehog_tracker_patch_lds_bytes exceeds 65536. */
int fd_ehog_tracker_extract_patches(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* xywh, uint8_t* valid, float* features, double* score);
/* host only: LDS bytes fd_ehog_tracker_extract_patches needs per sample; -1 on invalid parameters */
int fd_ehog_tracker_patch_lds_bytes(const fd_ehog_tracker_params* prm);
/* getHeatPeak (:434-456): the reference's loop bounds (the last full position is excluded), strict > in layer / row / column
 * order.  peak: score and the getOriginal bounds; without any position *found = 0, score -FLT_MAX, bounds 0. */
int fd_ehog_tracker_heat_peak(fd_ctx* ctx, fd_ehog_tracker* t, fd_box* peak, int* found);
/* the scan of createGoodNegativeExamples (:621-652): positions with score > threshold and >= all eight neighbours, in scan
 * order.  FD_ERR_CAPACITY with *count set when cap is too small; windows of one cell row or column are FD_ERR_INVALID_ARGUMENT
 * (the reference's scan reads outside the heat map). */
int fd_ehog_tracker_heat_maxima(fd_ctx* ctx, fd_ehog_tracker* t, float threshold, fd_box* out, int cap, int* count);
/* layers of the last update (0 before), and their feature (rows * cols * channels floats) / heat (rows * cols floats) maps */
int fd_ehog_tracker_get_layers(fd_ehog_tracker* t, fd_ehog_layer* out, int cap, int* n);
int fd_ehog_tracker_feature_layer(fd_ctx* ctx, fd_ehog_tracker* t, int layer, float* out);
int fd_ehog_tracker_heat_layer(fd_ctx* ctx, fd_ehog_tracker* t, int layer, float* out);

/* Linear C-SVC training on the device: the model libsvm::LibSvmClassifier::train obtains from svm_train (libsvm 3.17, C_SVC,
 * LINEAR, no shrinking; LibSvmClassifier.cpp:56-85,156-189) and LibSvmUtils::extractSupportVectors turns into one weight vector
 * (LibSvmUtils.cpp:105-118).  A problem is n_pos positive rows followed by n_neg negative rows of an n x d float row-major matrix
 * (n = n_pos + n_neg <= 1024), the order of createProblem.  The solver repeats libsvm's Solver::Solve operation for operation in
 * double on Q_ij = (float)(y_i y_j K_ij); K = X X^T is summed on the f64 matrix pipe, in another order than libsvm's dot, so that
 * single entries of Q may differ from libsvm's by one float ulp.  On the Q that fd_linear_svm_gram returns the result is libsvm's
 * bit for bit. */
typedef struct {
    double C, weight_pos, weight_neg;   /* per-class bound C * weight (libsvm's weighted_C) */
    double eps;                         /* stopping tolerance; 0 -> 1e-4 */
    int32_t max_iterations;             /* 0 -> libsvm's max(10000000, 100 n) */
    int32_t launch_iterations;          /* SMO iterations per kernel launch; 0 -> the default budget */
} fd_svm_train_params;
typedef struct {
    int32_t iterations, converged;      /* converged 0: max_iterations reached, the current model is returned (not an error) */
    int32_t n_sv, n_bounded, launches;  /* alpha > 0; alpha at its bound; launches of the solver kernel */
    double rho, objective;
} fd_svm_train_info;
typedef struct {
    const float* x;                     /* n x d */
    int32_t n_pos, n_neg, d, is_device; /* is_device: x is device memory */
    float* weights;                     /* out, d floats (host) */
    float* bias;                        /* out: (float)rho; the decision value is dot(w, x) - bias */
    double* alpha;                      /* out, n doubles (host); may be NULL */
} fd_svm_train_problem;
/* FD_ERR_INVALID_ARGUMENT for n_pos < 1, n_neg < 1, n > 1024, d < 1, C or a class weight <= 0, eps < 0, negative iteration
 * counts, or a required pointer that is NULL. */
/* Q (n x n floats) and QD (n doubles, K_ii) to host */
int fd_linear_svm_gram(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD);
int fd_linear_svm_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_train_params* params,
                        float* weights, float* bias, double* alpha /* n, may be NULL */, fd_svm_train_info* info);
/* count independent problems (one per tracked target) in one set of launches, one workgroup per problem; infos: count entries */
int fd_linear_svm_train_batch(fd_ctx* ctx, int count, const fd_svm_train_problem* problems, const fd_svm_train_params* params,
                              fd_svm_train_info* infos);
/* Trains on n_pos + n_neg host feature vectors of d = cell_rows * cell_cols * channels floats and installs the model in the
 * tracker: the weight vector is written by the training kernel into the tracker's device weights, then what
 * fd_ehog_tracker_set_svm does (the heat pyramid of the current frame); the handle's host copy of the weights is refreshed. */
int fd_ehog_tracker_train_svm(fd_ctx* ctx, fd_ehog_tracker* t, const float* x, int n_pos, int n_neg, const fd_svm_train_params* params,
                              fd_svm_train_info* info);
/* the handle's host copy of the installed model (fd_ehog_tracker_set_svm / _train_svm): cell_rows * cell_cols * channels floats and the
 * bias; FD_ERR_RUNTIME before an SVM is set */
int fd_ehog_tracker_get_svm(fd_ctx* ctx, fd_ehog_tracker* t, float* weights, float* bias);
/* host only, no context: whether the solver keeps Q in LDS for this size, and the default max_iterations; either may be NULL */
int fd_linear_svm_train_limits(int n_pos, int n_neg, int d, int* q_in_lds, int* max_iterations);

/* The same trainer for up to FD_SVM_LARGE_MAX_N examples (detector training with hard negatives): same parameter
 * and info structs, same row order (positives first), same guarantee -- on the Q that fd_linear_svm_gram_large returns the
 * result is libsvm's bit for bit.  Q (n_pad x n_pad floats, 1 GiB at the limit) lives in the context's training scratch;
 * FD_ERR_RUNTIME with a message when it cannot be allocated.  One problem per call, one workgroup of 1024 threads.  The
 * entry points above keep their limit of 1024 examples. */
#define FD_SVM_LARGE_MAX_N 16384
int fd_linear_svm_gram_large(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD);
int fd_linear_svm_train_large(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_train_params* params,
                              float* weights, float* bias, double* alpha /* n, may be NULL */, fd_svm_train_info* info);
/* host only, no context: the solver's LDS bytes for this size (G and the reduction slots) and the default max_iterations; either
 * may be NULL.  FD_ERR_INVALID_ARGUMENT for n_pos < 1, n_neg < 1, n > FD_SVM_LARGE_MAX_N or d < 1. */
int fd_linear_svm_train_large_limits(int n_pos, int n_neg, int d, int* lds_bytes, int* max_iterations);

/* C-SVC training with any kernel of fd_svm_model: what libsvm::LibSvmClassifier::createBinarySvm(kernel, C) trains
 * in the reference with an RbfKernel, a PolynomialKernel or a HistogramIntersectionKernel.  Problems, parameters and info as
 * above; K is Kernel::kernel_linear / kernel_poly / kernel_rbf / kernel_hik of libsvm (svm.cpp:231-273), Q_ij = (float)(y_i y_j
 * K_ij), QD_i = K_ii, and the solver is the one above.  The model is svm_train's for two classes: the examples with alpha > 0 in
 * ascending index (positives first) as support vectors, the coefficients (float)(alpha_i y_i), the bias rho; the decision value is
 * sum_i coefficient_i K(sv_i, x) - bias.  On the Q that fd_kernel_svm_gram returns the result is libsvm's bit for bit; for the
 * histogram-intersection kernel that Q is libsvm's own, for the others single entries may differ from it by one float ulp.  For
 * the RBF kernel QD is exactly 1.  The linear kernel is accepted (the same Q, alpha and rho as fd_linear_svm_train). */
typedef struct {
    int32_t kernel;       /* FD_KERNEL_* */
    double p0, p1, p2;    /* as in fd_svm_model -- rbf: gamma; poly: alpha (libsvm's gamma), constant (coef0), degree */
} fd_svm_kernel;
typedef struct {
    const float* x;                     /* n x d */
    int32_t n_pos, n_neg, d, is_device; /* is_device: x is device memory */
    int32_t* sv_index;                  /* out, n ints (host): the first n_sv are written */
    float* coefficients;                /* out, n floats (host): the first n_sv are written */
    float* support_vectors;             /* out, n x d floats (host): the first n_sv rows are written; may be NULL */
    float* bias;                        /* out: (float)rho */
    double* alpha;                      /* out, n doubles (host); may be NULL */
} fd_kernel_svm_train_problem;
/* FD_ERR_INVALID_ARGUMENT for what fd_linear_svm_train rejects (n up to FD_SVM_LARGE_MAX_N here, 1024 in the batch), an unknown
 * kernel, gamma < 0 (rbf, poly), a polynomial degree that is negative or not integral, a NULL kernel or required output.
 * One entry point for every size: up to 1024 examples on the solver of fd_linear_svm_train, beyond on that of
 * fd_linear_svm_train_large. */
int fd_kernel_svm_gram(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel, float* Q, double* QD);
int fd_kernel_svm_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                        const fd_svm_train_params* params, int32_t* sv_index /* n */, float* coefficients /* n */,
                        float* support_vectors /* n x d, may be NULL */, float* bias, double* alpha /* n, may be NULL */, fd_svm_train_info* info);
/* trains and creates the f32 model with fd_svm_create (the support vectors, coefficients, (float)rho, the kernel; threshold and
 * logistic parameters as given): *out is scored with fd_svm_distance_batch and freed with fd_svm_destroy.  FD_ERR_RUNTIME when no
 * alpha is positive (eps > 2). */
int fd_kernel_svm_train_model(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                              const fd_svm_train_params* params, float threshold, double logistic_a, double logistic_b, fd_svm** out,
                              fd_svm_train_info* info);
/* count independent problems of at most 1024 examples with one kernel in one set of launches; infos: count entries */
int fd_kernel_svm_train_batch(fd_ctx* ctx, int count, const fd_kernel_svm_train_problem* problems, const fd_svm_kernel* kernel,
                              const fd_svm_train_params* params, fd_svm_train_info* infos);
/* host only, no context: whether the solver keeps Q in LDS, whether the size takes the large solver, and the default
 * max_iterations; each may be NULL */
int fd_kernel_svm_train_limits(int n_pos, int n_neg, int d, int* q_in_lds, int* large, int* max_iterations);

/* One-class SVM training: what libsvm::LibSvmClassifier trains with oneClass set (svm_type ONE_CLASS;
 * solve_one_class svm.cpp:1577-1607).  n rows, every label +1, the dual's linear term 0, both bounds 1, the start state alpha_i = 1
 * for i < (int)(nu n), alpha_(int)(nu n) = nu n - (int)(nu n), 0 behind, and the start gradient G_j = sum_i alpha_i Q_ij summed as
 * Solver::Solve does (i ascending, in double on the float Q).  Q_ij = (float)K_ij, QD_i = K_ii with the kernels and the solver of
 * fd_kernel_svm_train; the model is the examples with alpha > 0, ascending, with the coefficients (float)alpha_i, and rho; the
 * decision value is sum_i coefficient_i K(sv_i, x) - bias.  On the Q that fd_one_class_svm_gram returns the result is libsvm's bit
 * for bit.  nu = 1 puts every alpha at its bound and gives rho = +inf, as libsvm does. */
typedef struct {
    double nu;                          /* in (0, 1] */
    double eps;                         /* stopping tolerance; 0 -> 1e-4 */
    int32_t max_iterations;             /* 0 -> libsvm's max(10000000, 100 n) */
    int32_t launch_iterations;          /* as in fd_svm_train_params */
} fd_svm_one_class_params;
/* FD_ERR_INVALID_ARGUMENT for n < 1, n > FD_SVM_LARGE_MAX_N, d < 1, nu <= 0 or nu > 1 (svm_check_parameter), eps < 0, negative
 * iteration counts, what fd_kernel_svm_train rejects of a kernel, or a required pointer that is NULL.  Up to 1024 examples run on
 * the solver of fd_linear_svm_train, more on that of fd_linear_svm_train_large. */
/* Q (n x n floats), QD (n doubles) and the start gradient G0 (n doubles, may be NULL) of this nu to host */
int fd_one_class_svm_gram(fd_ctx* ctx, const float* x, int n, int d, int is_device, const fd_svm_kernel* kernel, double nu, float* Q, double* QD,
                          double* G0);
int fd_one_class_svm_train(fd_ctx* ctx, const float* x, int n, int d, int is_device, const fd_svm_kernel* kernel,
                           const fd_svm_one_class_params* params, int32_t* sv_index /* n */, float* coefficients /* n */,
                           float* support_vectors /* n x d, may be NULL */, float* bias, double* alpha /* n, may be NULL */, fd_svm_train_info* info);
/* trains and creates the f32 model as fd_kernel_svm_train_model does.  FD_ERR_RUNTIME when rho is not finite (nu = 1). */
int fd_one_class_svm_train_model(fd_ctx* ctx, const float* x, int n, int d, int is_device, const fd_svm_kernel* kernel,
                                 const fd_svm_one_class_params* params, float threshold, double logistic_a, double logistic_b, fd_svm** out,
                                 fd_svm_train_info* info);
/* host only, no context: as fd_kernel_svm_train_limits for n examples */
int fd_one_class_svm_train_limits(int n, int d, int* q_in_lds, int* large, int* max_iterations);

/* libsvm's sigmoid fit for a C-SVC (`probabilistic`): svm_binary_svc_probability (svm.cpp:1940-2024) with the
 * permutation supplied by the caller.  The five folds [i n / 5, (i + 1) n / 5) of the permuted order are held out in turn; a
 * fold's C-SVC is trained on the remaining examples, its positives in permuted order, then its negatives, with C = 1 and the
 * class weights C weight_pos, C weight_neg of `params` -- all folds in one set of launches, each with the alpha, rho and iteration
 * count fd_kernel_svm_train returns for these rows.  The held-out examples get sum_s (alpha_s y_s) k_function(x, sv_s) - rho in
 * double, in libsvm's summation order; a fold whose training part has no positive, no negative or no example gives its examples
 * -1, +1 or 0 and trains nothing.  sigmoid_train (svm.cpp:1752-1863) on these decision values returns libsvm's probA, probB
 * (LibSvmClassifier installs them as logisticB, logisticA).  The final model is not trained here. */
#define FD_SVM_CV_FOLDS 5
#define FD_SVM_SIGMOID_CONVERGED 0            /* both gradient components below 1e-5 */
#define FD_SVM_SIGMOID_MAX_ITERATIONS 1       /* 100 Newton iterations */
#define FD_SVM_SIGMOID_LINE_SEARCH_FAILED 2
typedef struct {
    fd_svm_train_info fold[FD_SVM_CV_FOLDS];  /* of the trained folds; zero for the others */
    int32_t fold_trained[FD_SVM_CV_FOLDS];    /* 1: trained; 0: constant decision values */
    double fold_constant[FD_SVM_CV_FOLDS];    /* the constant of a fold that was not trained: -1, +1 or 0 */
    int32_t newton_iterations, status;        /* of the fit; FD_SVM_SIGMOID_* */
} fd_svm_cv_info;
/* perm: n = n_pos + n_neg ints, a permutation of 0..n-1 (else FD_ERR_INVALID_ARGUMENT); dec_values: n doubles in example order,
 * may be NULL; cv_info may be NULL.  Otherwise the errors of fd_kernel_svm_train. */
int fd_kernel_svm_cv_sigmoid(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                             const fd_svm_train_params* params, const int32_t* perm, double* prob_a, double* prob_b, double* dec_values,
                             fd_svm_cv_info* cv_info);
/* host only, no context: sigmoid_train operation for operation in double with libm's exp and log, on n decision values of which
 * the first n_pos belong to positive examples.  iterations and status may be NULL.  FD_ERR_INVALID_ARGUMENT for n < 1, n_pos
 * outside 0..n or a NULL array or result. */
int fd_svm_sigmoid_train(int n, const double* dec_values, int n_pos, double* prob_a, double* prob_b, int* iterations, int* status);

/* Primal L2-regularised L2-loss SVC training on the device: the model liblinear::LibLinearClassifier::train
 * obtains from liblinear's train with L2R_L2LOSS_SVC (LibLinearClassifier.cpp:32-46,96-148; linear.cpp l2r_l2_svc_fun :191-340,
 * train_one :2181-2230; tron.cpp TRON::tron / trcg :56-221) and LibLinearUtils turns into one weight vector
 * (LibLinearUtils.cpp:70-105).  f(w) = 1/2 w.w + sum_i C_i max(0, 1 - y_i w.x_i)^2 is minimised by the trust-region Newton
 * method, all in double; the state is one weight vector of d + bias doubles and the work is passes over the n x d float matrix,
 * so there is no n x n term.  Rows are positives first; with bias a constant-1 feature is appended (never stored) and regularised
 * like any weight.  TRON's scalar state machine is tron.cpp's, comparison for comparison; sums run in a fixed order that depends
 * on (n, d, bias) only and differs from liblinear's sequential one, so the result is liblinear's up to rounding as long as no
 * comparison of the run is closer than that rounding. */
#define FD_LIBLINEAR_MAX_N 1048576
#define FD_LIBLINEAR_MAX_D 8192          /* d + bias */
#define FD_LIBLINEAR_SMALL_MAX_N 2048    /* rows the single-workgroup form (and a problem of a batch) takes */
enum { FD_LL_STOP_NONE = 0, FD_LL_STOP_GRADIENT = 1, FD_LL_STOP_MAX_ITER = 2, FD_LL_STOP_ACTRED_ZERO = 3, FD_LL_STOP_ACTRED_SMALL = 4,
       FD_LL_STOP_CG_CAP = 5, FD_LL_STOP_NONFINITE = 6 };
typedef struct {
    double C, weight_pos, weight_neg;  /* per-class C * weight; the reference passes 1, 1 */
    double eps;                        /* liblinear's param->eps; 0 -> 0.01.  The solver runs with eps * max(min(pos, neg), 1) / n */
    double solver_tol;                 /* > 0: TRON's eps directly (overrides eps) */
    int32_t bias;                      /* 1: append the constant-1 feature, regularised */
    int32_t max_iterations;            /* 0 -> 1000 (TRON's max_iter) */
    int32_t max_cg_steps;              /* cap on the total number of CG steps (trcg has none); 0 -> 100 (d + bias) + 1000 */
    int32_t launch_steps;              /* (pass, step) pairs per budget; 0 -> default */
} fd_liblinear_params;
typedef struct {
    int32_t iterations, cg_steps, converged, stop;   /* accepted steps; CG steps in all; 1 for FD_LL_STOP_GRADIENT only; FD_LL_STOP_* */
    int32_t n_active;                                 /* |I| at the returned w */
    int32_t trace_len;                                /* outer iterations (trcg calls) run; min(trace_len, trace_cap) triples are written */
    double objective, gnorm, gnorm0, delta;
} fd_liblinear_info;
typedef struct {
    const float* x;                     /* n x d */
    int32_t n_pos, n_neg, d, is_device; /* is_device: x is device memory */
    float* weights;                     /* out, d floats (host) */
    float* bias;                        /* out: (float)(-w[d]), 0 without the bias term; the decision value is dot(w, x) - bias */
    double* w;                          /* out, d + bias doubles (host); may be NULL */
} fd_liblinear_problem;
/* weights: d floats (float)w; *bias_out as above; w (d + bias doubles), trace ({cg_steps, hit_boundary, accepted} per outer
 * iteration, at most trace_cap int32 triples) and info may be NULL.  A run that stops for another reason than the gradient test
 * (the iteration or CG cap, TRON's warnings, a non-finite f or |g|) returns the last accepted w with converged = 0 and is not an
 * error.  FD_ERR_INVALID_ARGUMENT for what fd_linear_svm_train rejects (n up to FD_LIBLINEAR_MAX_N, d + bias up to
 * FD_LIBLINEAR_MAX_D), eps < 0, solver_tol < 0, a bias other than 0 or 1, negative caps, or a required pointer that is NULL;
 * FD_ERR_RUNTIME with a message when the scratch cannot be allocated. */
int fd_liblinear_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_liblinear_params* params,
                       float* weights, float* bias_out, double* w, int32_t* trace, int trace_cap, fd_liblinear_info* info);
/* count independent problems (one per tracked target) of at most FD_LIBLINEAR_SMALL_MAX_N rows in one set of launches, one
 * workgroup per problem; infos: count entries.  A problem's result is that of fd_liblinear_train in its single-workgroup form. */
int fd_liblinear_train_batch(fd_ctx* ctx, int count, const fd_liblinear_problem* problems, const fd_liblinear_params* params,
                             fd_liblinear_info* infos);
/* fun, grad and -- when s is given -- Hv of l2r_l2_svc_fun at the caller's w (d + bias doubles), through the pass and reduction
 * code of the trainer: *f, g (d + bias doubles), Hs (d + bias doubles; the active set is that of grad at w).  Hs may be NULL
 * when s is. */
int fd_liblinear_objective(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_liblinear_params* params,
                           const double* w, const double* s, double* f, double* g, double* Hs);
/* host only, no context: whether fd_liblinear_train takes the single-workgroup form for this size, the rows of a slab, the bytes
 * of training scratch (without a host caller's x) and the LDS bytes of a workgroup; each may be NULL.  The rule:
 * single workgroup for n <= FD_LIBLINEAR_SMALL_MAX_N and n (d + bias) <= 40960; FD_LIBLINEAR_SMALL_ROWS in the environment
 * (0 .. FD_LIBLINEAR_SMALL_MAX_N) replaces the first limit, 0 selecting the multi-workgroup form for every size. */
int fd_liblinear_train_limits(int n_pos, int n_neg, int d, int bias, int* single_workgroup, int* slab_rows, int64_t* scratch_bytes,
                              int* lds_bytes);

/* A particle set of the Condensation tracker resident on the device: two generations of up to `capacity` samples
 * as structure-of-arrays, bound to one fd_ehog_tracker.  A frame of ResamplingSampler(LowVarianceSampling, SimpleTransitionModel) +
 * ExtendedHogBasedMeasurementModel + FilteringStateExtractor(WeightedMeanStateExtractor) is fd_ehog_tracker_update,
 * fd_particles_sample, _evaluate, _weigh and _state: one chain of kernels on the context's stream and one read-back of
 * fd_particles_info.  The host draws every random number; the device adds, multiplies, rounds and compares, so that every integer it
 * produces is reproducible bit for bit. */
typedef struct fd_particles fd_particles;
#define FD_PARTICLES_MAX 8192
typedef struct {
    int32_t *x, *y, *size, *vx, *vy;   /* centre, width, velocity */
    float* vsize;                      /* size factor per frame */
    double *weight, *score;
    uint8_t* target;
    int32_t* cluster_id;               /* any int but INT32_MIN */
} fd_particles_arrays;
typedef struct {
    int32_t found;                     /* a state was extracted: x .. vsize hold it */
    int32_t x, y, size, vx, vy;
    float vsize;
    int32_t cluster_id;                /* the cluster the state was taken from */
    int32_t count, n_valid, n_target;  /* samples of the generation; with a window at the last _evaluate; with the target flag */
    int32_t bad_weight;                /* a weight is negative, infinite or NaN */
    double best_score;                 /* the largest score after _weigh (samples without a window count with 0); -DBL_MAX before */
    double weight_sum;                 /* all weights added in index order: the sum LowVarianceSampling::computeWeightSum returns */
} fd_particles_info;
/* capacity 1 .. FD_PARTICLES_MAX, otherwise FD_ERR_INVALID_ARGUMENT.  The tracker must outlive the set. */
int fd_particles_create(fd_ctx* ctx, fd_ehog_tracker* t, int capacity, fd_particles** out);
void fd_particles_destroy(fd_particles* p);
int fd_particles_capacity(const fd_particles* p);
/* host only: whether FD_COND_DEVICE asks the trackers of the host layer to keep their particles on the device (read at every call) */
int fd_particles_route_enabled(void);
/* fills the current generation with n <= capacity samples from host arrays; score and target may be NULL (0) */
int fd_particles_set(fd_ctx* ctx, fd_particles* p, int n, const fd_particles_arrays* in);
/* downloads the current generation (*n samples, FD_ERR_CAPACITY with *n set when cap is smaller); NULL members, or a NULL out, are
 * skipped */
int fd_particles_get(fd_ctx* ctx, fd_particles* p, int cap, int* n, const fd_particles_arrays* out);
/* what the last _sample and _evaluate left besides the samples: the index in the old generation each sample was copied from (-1: a
 * fresh one), the window {layer, bx, by, valid} and the valid flag of each sample.  Any pointer may be NULL. */
int fd_particles_get_trace(fd_ctx* ctx, fd_particles* p, int32_t* source, int32_t* windows, uint8_t* valid);
/* ResamplingSampler::sample (ResamplingSampler.cpp:50-59): the current generation becomes the old one; the new one is n_resampled
 * copies chosen by LowVarianceSampling::resample (.cpp:20-39) with the uniform draw u in [0, 1), each moved as
 * SimpleTransitionModel::predict (.cpp:25-44) moves it with diffusion[3 i .. 3 i + 2] = {positionDeviation * z, positionDeviation * z,
 * pow(2, sizeDeviation * z)}, followed by count - n_resampled samples {x, y, size} from `fresh` with the cluster ids
 * first_fresh_cluster_id, + 1, ...  Copies have weight 1, score 0, no target flag and their parent's cluster id.  When the old
 * generation is empty or its weight sum / n_resampled is not positive no copy is made (the new generation holds the fresh samples
 * only).  count 0: an empty generation.  FD_ERR_INVALID_ARGUMENT for count > capacity or n_resampled outside [0, count];
 * FD_ERR_RUNTIME when the old generation holds a weight that is negative or not finite (nothing is launched). */
int fd_particles_sample(fd_ctx* ctx, fd_particles* p, int count, int n_resampled, double u, const double* diffusion, const int32_t* fresh,
                        int32_t first_fresh_cluster_id);
/* scores the current generation on the tracker's current frame: each sample {x, y, size, cvRound(aspect_ratio * size)} is resolved to
 * its window on the device and scored by the kernels of fd_ehog_tracker_evaluate_samples (use_patches 0: the heat value) or of
 * fd_ehog_tracker_extract_patches (1).  Nothing is copied back. */
int fd_particles_evaluate(fd_ctx* ctx, fd_particles* p, int use_patches, double aspect_ratio);
#define FD_PARTICLES_TARGET_LOST 0     /* target: score >= svm_threshold */
#define FD_PARTICLES_SLIDING_WINDOW 1  /* target: score > rejection_threshold */
#define FD_PARTICLES_ALL_TARGETS 2
/* ExtendedHogBasedMeasurementModel.cpp:173-205 on the scores of _evaluate: a sample without a window gets weight 0, score 0 and no
 * target flag; any other weight *= p(score) with ProbabilisticSvmClassifier's logistic (a, b).  When a product is negative or not
 * finite no weight is changed and bad_weight is raised. */
int fd_particles_weigh(fd_ctx* ctx, fd_particles* p, double logistic_a, double logistic_b, double svm_threshold, int mode, double rejection_threshold);
/* FilteringStateExtractor(WeightedMeanStateExtractor) on the current generation (WeightedMeanStateExtractor.cpp:23-62): the samples
 * with the target flag, their largest cluster (of equally large ones the cluster whose first member has the lowest index), seven
 * double sums in index order, (int)(mean + 0.5) for all six values.  Fills *out and waits for it: the one read-back of a frame.
 * With bad_weight set no state is reported and FD_ERR_RUNTIME is returned (*out is filled). */
int fd_particles_state(fd_ctx* ctx, fd_particles* p, fd_particles_info* out);

/* Pyramidal Lucas-Kanade optical flow for condensation::OpticalFlowTransitionModel (OpticalFlowTransitionModel.cpp:86-111):
 * cv::buildOpticalFlowPyramid(gray, pyramid, winSize, maxLevel, true, BORDER_REPLICATE, BORDER_REPLICATE) and
 * cv::calcOpticalFlowPyrLK(previous, current, points, ..., winSize, maxLevel) with OpenCV's default criteria, as DESIGN.md 4.14
 * defines their arithmetic.  A handle holds the padded levels and padded Scharr derivatives of two frames of one size (current and
 * previous); one wavefront tracks one point through all levels. */
typedef struct fd_flow fd_flow;
#define FD_FLOW_MAX_POINTS 16384
#define FD_FLOW_MIN_WINDOW 3
#define FD_FLOW_MAX_WINDOW 31
#define FD_FLOW_MAX_LEVELS 8            /* max_level 0 .. 7 */
typedef struct {
    int32_t win_w, win_h;               /* search window, FD_FLOW_MIN_WINDOW .. FD_FLOW_MAX_WINDOW per side */
    int32_t max_level;                  /* 0-based top level asked for; fewer are built when a level would not exceed the window */
    int32_t max_count;                  /* iterations per level, clamped to 0 .. 100 */
    double epsilon;                     /* clamped to 0 .. 10, squared before use */
    double min_eig_threshold;
} fd_flow_params;
/* host only: 15, 15, 2, 30, 0.01, 1e-4 (OpticalFlowTransitionModel's and calcOpticalFlowPyrLK's defaults) */
int fd_flow_default_params(fd_flow_params* out);
/* host only: the largest n of fd_flow_track / _track_fb and the window bounds; each may be NULL */
int fd_flow_limits(int* max_points, int* min_window, int* max_window);
/* FD_ERR_INVALID_ARGUMENT for a window outside the bounds, max_level outside 0 .. FD_FLOW_MAX_LEVELS - 1 or an empty image */
int fd_flow_create(fd_ctx* ctx, int width, int height, const fd_flow_params* params, fd_flow** out);
void fd_flow_destroy(fd_flow* flow);
int fd_flow_levels(const fd_flow* flow);   /* levels built: level l + 1 exists while its width > win_w and its height > win_h */
/* The current pyramid becomes the previous one and the image's pyramid the current one.  image: width x height, channels 1 (gray) or
 * 3 (BGR, converted as the image pyramid converts), rows `stride` bytes apart (0: width * channels), host or device memory.  Queued
 * on the context's stream. */
int fd_flow_update(fd_ctx* ctx, fd_flow* flow, const uint8_t* image, int channels, int stride, int on_device);
/* what ended a level of a point (trace) */
enum {
    FD_FLOW_EXIT_NONE = 0,          /* the level does not exist */
    FD_FLOW_EXIT_SKIP_RANGE = 1,    /* the window of the point lies outside the level: skipped (status 0 at level 0) */
    FD_FLOW_EXIT_SKIP_EIGEN = 2,    /* smallest eigenvalue under the threshold or determinant under FLT_EPSILON: skipped (status 0 at level 0) */
    FD_FLOW_EXIT_EPS = 3,           /* a step of squared length <= epsilon^2 */
    FD_FLOW_EXIT_OSCILLATION = 4,   /* two steps that cancel: half of the last one is taken back */
    FD_FLOW_EXIT_COUNT = 5,         /* max_count steps */
    FD_FLOW_EXIT_LEFT_RANGE = 6     /* the window left the level during the iterations (status 0 at level 0) */
};
/* Tracks n <= FD_FLOW_MAX_POINTS points {x, y} from the previous frame to the current one (backward 0) or from the current to the
 * previous (backward 1).  out_xy: 2 n floats; status: n bytes; trace (may be NULL): per point and level l < FD_FLOW_MAX_LEVELS
 * the two bytes {steps taken, exit reason}.  Waits for the results.  FD_ERR_RUNTIME before the second fd_flow_update. */
int fd_flow_track(fd_ctx* ctx, fd_flow* flow, int backward, const float* pts_xy, int n, float* out_xy, uint8_t* status, uint8_t* trace);
/* forward, then backward from the forward results (all of them, as OpticalFlowTransitionModel.cpp:110-111 does): one submission, one
 * wait.  fwd, bwd: 2 n floats each. */
int fd_flow_track_fb(fd_ctx* ctx, fd_flow* flow, const float* pts_xy, int n, float* fwd, float* bwd, uint8_t* fstatus, uint8_t* bstatus);
/* test hook: level `level` of the current (which 0) or previous (1) frame as it is stored, with its border: *w x *h bytes into
 * image_out and 2 * *w * *h int16 {dx, dy} into deriv_out (either may be NULL) */
int fd_debug_flow_level(fd_ctx* ctx, fd_flow* flow, int which, int level, uint8_t* image_out, int16_t* deriv_out, int* w, int* h);
/* host only: the template grid of OpticalFlowTransitionModel (.cpp:63-75) for grid_w x grid_h points, relative to the target's centre
 * in units of its size.  out_xy: up to cap points; *n the number of points (FD_ERR_CAPACITY when cap is smaller). */
int fd_flow_grid(int grid_w, int grid_h, int circle, float* out_xy, int cap, int* n);
typedef struct {
    int32_t ok;                        /* the median flow is usable: enough valid and enough correct pairs */
    int32_t n_valid, n_correct;        /* pairs with both status flags; of those, with squared forward-backward distance <= 0.5f */
    float median_x, median_y;          /* medians of the correct flows */
    float median_ratio;                /* sqrt of the median ratio of squared point distances after / before */
    int32_t* order;                    /* caller's buffer of n entries or NULL: the valid indices by (distance, index); the first n_correct are the correct ones */
} fd_flow_motion;
/* host only: OpticalFlowTransitionModel.cpp:114-170 on n tracked points */
int fd_flow_median(const float* points, const float* fwd, const float* bwd, const uint8_t* fstatus, const uint8_t* bstatus, int n,
                   fd_flow_motion* out);

/* detection::AggregatedFeaturesDetector (AggregatedFeaturesDetector.cpp:37-128) with imageFilter = GrayscaleFilter,
 * layerFilter = FhogFilter on an extraction::AggregatedFeaturesExtractor (AggregatedFeaturesExtractor.cpp:34-130): a linear
 * SVM convolved over the FHOG cell pyramid (ConvolutionFilter.cpp:27-43), windows with score > threshold, bounds through
 * the layers' actual x / y scales, rescaleWindow, NonMaximumSuppression.  SURVEY.md 8(f) row 2. */
typedef struct fd_aggregated fd_aggregated;
typedef struct {
    fd_fhog_params fhog;              /* layer filter; fhog.cell_size is the detector's cellSize */
    int32_t window_w, window_h;       /* windowSize in cells */
    int32_t octave_layer_count;
    int32_t min_window_width;         /* minWindowWidth in pixels (0: none) */
    float width_scale, height_scale;  /* rescaleWindow */
    const float* svm_weights;         /* the linear SVM's support vector, [window_h][window_w][3 * unsigned_bins + 4] */
    float svm_bias, score_threshold;  /* delta = -bias; getThreshold() */
    double nms_overlap_threshold;
    int32_t nms_maximum_type;         /* 0 MAX_SCORE, 1 AVERAGE, 2 WEIGHTED_AVERAGE */
} fd_aggregated_params;
int fd_aggregated_create(fd_ctx* ctx, const fd_aggregated_params* prm, fd_aggregated** out);
void fd_aggregated_destroy(fd_aggregated* a);
/* detectWithScores(image): final detections in out; candidates (before NMS, layer / row / column order) optionally */
int fd_aggregated_detect(fd_ctx* ctx, fd_aggregated* a, const uint8_t* image, int width, int height, int channels, int is_device,
                         fd_box* out, int cap, int* count, fd_box* candidates, int cand_cap, int* cand_count);

/* The same detector on an approximated feature pyramid: createApproximateDetector (DetectorTrainingApp.cpp:168-191),
 * ImagePyramid::createApproximated (ImagePyramid.cpp:51-63,200-289).  FHOG runs on one gray layer per octave only (a source
 * pyramid with one layer per octave and the limits of the octave_layer_count pyramid); the octave_layer_count - 1 layers
 * between two of them are per-channel bilinear resizes of the octave's feature layer (cv::resize INTER_LINEAR on CV_32F),
 * multiplied by (float)pow(s, -lambda[channel]) with s = pow(inc, i).  lambdas: one per channel (3 * unsigned_bins + 4),
 * or n_lambdas == 0: estimated per image from the channel means of two exact layers (ImagePyramid.cpp:237-275; the means are
 * double sums of the float cells).  fd_aggregated_detect works unchanged on such a handle.  Estimating needs two exact layers:
 * with fewer, fd_aggregated_detect returns FD_ERR_RUNTIME (given lambdas work on a single octave, like in the reference). */
int fd_aggregated_create_approximated(fd_ctx* ctx, const fd_aggregated_params* prm, const double* lambdas, int n_lambdas, fd_aggregated** out);
/* the lambdas the last fd_aggregated_detect used (approximated handles; n = 0 before the first detect on estimating handles) */
int fd_aggregated_get_lambdas(fd_aggregated* a, double* out, int cap, int* n);
typedef struct {
    int32_t index;            /* ImagePyramidLayer::getIndex() */
    int32_t approximated;     /* 0: FHOG of a gray layer; 1: resized from the exact layer at position `parent` */
    int32_t parent;           /* position of that exact layer in this list; -1 for exact layers */
    int32_t rows, cols;       /* size in cells */
    int32_t reserved;
    double scale, scale_x, scale_y;
} fd_aggregated_layer;
/* feature layers of the last fd_aggregated_detect, in layer order (handles of either kind) */
int fd_aggregated_get_layers(fd_aggregated* a, fd_aggregated_layer* out, int cap, int* n);
/* feature layer `layer` (position in that list) of the last fd_aggregated_detect: rows * cols * channels floats (host).  Valid
 * until the next FHOG or aggregated call on the context (FD_ERR_INVALID_ARGUMENT afterwards). */
int fd_aggregated_feature_layer(fd_ctx* ctx, fd_aggregated* a, int layer, float* out);
/* Host only (no context, no device): the layer list fd_aggregated_detect builds on an approximated handle for an image of
 * width x height.  FD_ERR_RUNTIME when fewer than two exact layers remain (what a handle that estimates its lambdas reports; *n is
 * set), FD_ERR_CAPACITY when cap is too small (*n is set). */
int fd_aggregated_plan_layers(int window_w, int window_h, int cell_size, int octave_layer_count, int min_window_width, int width,
                              int height, fd_aggregated_layer* out, int cap, int* n);

/* extraction::AggregatedFeaturesExtractor::update and extract(Rect) on a handle of any kind (AggregatedFeaturesExtractor.cpp:55-60,
 * 83-128).  fd_aggregated_update does what fd_aggregated_detect does up to and including the feature layers (the
 * pyramid, the geometry, the features, the approximated layers) and produces no scores.  fd_aggregated_extract resolves n boxes
 * {x, y, w, h} in image pixels on the host, in double, exactly as the reference does -- layer round(log(patchWidthPx / w) /
 * log(inc)), centre through the layer's actual scales and truncated to cells, Patch::computeBounds, the within-image test -- and
 * copies the window_h x window_w x channels cells of every valid window k into row k of `features` (n x d floats, host or
 * device memory) in one launch.  bounds[k] (may be NULL; score 0) is computeBoundsInImagePixels of the window.  valid[k] = 0
 * where the reference returns a null patch or w < 1: row k and bounds[k] are left untouched.  FD_ERR_RUNTIME when the handle's
 * feature layers are not the context's current ones (another FHOG or aggregated call came in between). */
int fd_aggregated_update(fd_ctx* ctx, fd_aggregated* a, const uint8_t* image, int width, int height, int channels, int is_device);
int fd_aggregated_extract(fd_ctx* ctx, fd_aggregated* a, int n, const int32_t* boxes /* n x {x, y, w, h} */, float* features,
                          int features_on_device, fd_box* bounds, uint8_t* valid);
/* replaces the linear SVM of a handle (weights as in fd_aggregated_params) and its threshold; the feature layers stay */
int fd_aggregated_set_svm(fd_ctx* ctx, fd_aggregated* a, const float* weights, float bias, float threshold);

/* FPDW channel features: ChainedFilter(FpdwFeaturesFilter(fastGradient, interpolate, normalizationRadius, normalizationConstant),
 * AggregationFilter(cellSize, true, false)) on CV_8UC3 images (FpdwFeaturesFilter.cpp:21-205, AggregationFilter.cpp:20-36,
 * TriangularConvolutionFilter.cpp:20-241): ten floats per pixel / cell -- six unsigned gradient-orientation bins, the gradient
 * magnitude normalised by its (2 radius + 1)-tap triangular mean + constant (radius 0: not normalised), L / 354, (u + 134) / 354,
 * (v + 140) / 354 -- and the cells the triangular aggregation filter (2 cell_size or 2 cell_size - 1 taps, sampled every cell_size
 * pixels, alpha = cell_size^2) makes of them.  The sums are fp32 sums of the taps (not the reference's running differences) and
 * L*u*v* is evaluated per pixel from OpenCV's documented formula: parity is by tolerance, DESIGN.md 4.3.  DetectorTrainingApp
 * uses (true, false, cellSize, 0.01). */
typedef struct {
    int32_t cell_size, fast_gradient, interpolate, normalization_radius;
    float normalization_constant;
} fd_fpdw_params;
/* host only: rows = height / cell_size, cols = width / cell_size, channels = 10 */
int fd_fpdw_size(const fd_fpdw_params* fp, int width, int height, int* rows, int* cols, int* channels);
/* host only (no context, no device): the gradient look-up table, 65536 entries each, index gx | gy << 8 (createGradientLut,
 * FpdwFeaturesFilter.cpp:34-64, with the orientation taken as (float)atan2((double)gY, (double)gX)).  Without interpolation
 * bin2 = 0, w1 = 1, w2 = 0.  Any output may be NULL. */
int fd_fpdw_gradient_lut(const fd_fpdw_params* fp, int32_t* bin1, int32_t* bin2, float* w1, float* w2, float* magnitude);
/* FpdwFeaturesFilter::applyTo: bgr host image (width * height * 3 bytes) -> width * height * 10 floats (host).  FD_ERR_INVALID_ARGUMENT
 * with TriangularConvolutionFilter's text when the image is smaller than the normaliser allows (rows <= radius, cols < 2 radius + 2) */
int fd_fpdw_image(fd_ctx* ctx, const uint8_t* bgr, int width, int height, const fd_fpdw_params* fp, float* out);
/* the whole chain: (height / cell_size) * (width / cell_size) * 10 floats (host); the aggregation filter's limits (rows < cell_size,
 * cols < 2 cell_size) are reported in the same way */
int fd_fpdw_cells_image(fd_ctx* ctx, const uint8_t* bgr, int width, int height, const fd_fpdw_params* fp, float* out);
/* AggregatedFeaturesDetector with no image filter and that chain as layer filter (DetectorTrainingApp.cpp:99-113,252-254): the
 * pyramid scales the B, G and R planes, each exactly as the gray pyramid scales a gray image.  prm->fhog.cell_size must equal
 * fp->cell_size (the other fhog fields are ignored); svm_weights is [window_h][window_w][10].  approximated != 0: the
 * approximated feature pyramid with n_lambdas = 10 given lambdas, or 0: estimated per image.  fd_aggregated_detect (3-channel
 * images only), _get_lambdas, _get_layers, _feature_layer and _destroy work unchanged on such a handle. */
int fd_aggregated_create_fpdw(fd_ctx* ctx, const fd_aggregated_params* prm, const fd_fpdw_params* fp, int approximated, const double* lambdas,
                              int n_lambdas, fd_aggregated** out);

/* Generic histogram patch filters on the pyramid's bin-image layers (FD_LAYER_GRADBIN: 2 or 4 channels,
 * FD_LAYER_LBP: 1 channel), all built on HistogramFilter::createCellHistograms (HistogramFilter.cpp:23-197,
 * interpolating and non-interpolating):
 *  FD_HIST_HOG             HogFilter(bins, cell_size, block_size, interpolate, signed_and_unsigned)  HogFilter.cpp:58-122
 *  FD_HIST_SPATIAL         SpatialHistogramFilter(bins, cell_size, block_size, interpolate, concatenate, normalization)
 *                          SpatialHistogramFilter.cpp:56-94
 *  FD_HIST_PYRAMID_HOG     PyramidHogFilter(bins, levels, interpolate, signed_and_unsigned)  PyramidHogFilter.cpp:33-113
 *  FD_HIST_SPATIAL_PYRAMID SpatialPyramidHistogramFilter(bins, levels, interpolate, normalization)
 *                          SpatialPyramidHistogramFilter.cpp:37-81
 * normalization (HistogramFilter::Normalization): 0 none, 1 L2NORM, 2 L2HYS, 3 L1NORM, 4 L1SQRT. */
enum { FD_HIST_HOG = 0, FD_HIST_SPATIAL = 1, FD_HIST_PYRAMID_HOG = 2, FD_HIST_SPATIAL_PYRAMID = 3 };
typedef struct {
    int32_t patch_w, patch_h, step_x, step_y;
    int32_t kind, bins;
    int32_t cell_size, block_size;   /* FD_HIST_HOG, FD_HIST_SPATIAL: cell width / block width (cells) */
    int32_t levels;                  /* pyramid kinds: levelCount */
    int32_t interpolate, signed_and_unsigned, concatenate, normalization;
    int32_t cell_h, block_h;         /* cell height / block height; 0 = same as cell_size / block_size */
} fd_hist_params;
/* feature length for a bin image with `channels` channels; -1 on invalid parameters */
int fd_hist_feature_length(const fd_hist_params* hp, int channels);
/* FeatureExtractor::extract for every window: n_windows x feature_length floats to host.
 * features == NULL: only *count is set. */
int fd_extract_hist(fd_ctx* ctx, fd_pyramid* p, const fd_hist_params* hp, float* features, int64_t cap_windows,
                    int64_t* count);
/* HistogramFilter::applyTo(const Mat&) of the same four patch filters on n contiguous bin-image patches (hp->patch_w x hp->patch_h
 * pixels, `channels` bytes per pixel: 1 bin, 2 bin + weight, 4 two bins + weights; hp->step_x / step_y are ignored).
 * out: n x fd_hist_feature_length(hp, channels) floats. */
int fd_hist_patch_batch(fd_ctx* ctx, const uint8_t* bin_patches, int64_t n, int channels, const fd_hist_params* hp, float* out);
/* imageprocessing::ExtendedHogFilter(binCount, cellWidth, cellHeight, interpolate, signedAndUnsigned, alpha)
 * (ExtendedHogFilter.cpp:54-209) on n contiguous bin-image patches (patch_w x patch_h pixels, `channels` bytes per pixel as above):
 * cvRound(patch_h / cell_h) x cvRound(patch_w / cell_w) cell histograms by HistogramFilter::createCellHistograms, then per cell
 * bins (+ bins / 2 with signed_and_unsigned) + 4 floats in the order [bins][unsigned halves][4 energy features], normalised and
 * truncated as CompleteExtendedHogFilter's.  cell_h 0: same as cell_w.  The "ehog" feature type of createEHogExtractor is
 * GradientFilter -> GradientBinningFilter -> this filter. */
typedef struct {
    int32_t patch_w, patch_h, bins, cell_w, cell_h, interpolate, signed_and_unsigned;
    float alpha;
} fd_ehog_patch_params;
/* host only: floats per patch; -1 where fd_ehog_patch_batch returns FD_ERR_INVALID_ARGUMENT (a grid with zero rows or columns included) */
int fd_ehog_feature_length(const fd_ehog_patch_params* ep, int channels);
int fd_ehog_patch_batch(fd_ctx* ctx, const uint8_t* bin_patches, int64_t n, int channels, const fd_ehog_patch_params* ep, float* out);
/* ---- features of explicit sample windows of a filtered pyramid (DirectPyramidFeatureExtractor::extract(x, y, width, height),
 *      DirectPyramidFeatureExtractor.cpp:67-73,134-153), all samples of a call in one launch ----
 * The sample -> window rule (ImagePyramid::getLayer(double) :307-310): index = lround(log(patch_w / width) / log(incremental
 * scale)); the layer with that pyramid index must be a kept one; bx = cvRound((x - width / 2) * scale), by = cvRound((y - height
 * / 2) * scale) with C integer division; the sample has a window iff width > 0 and the patch_w x patch_h window at (bx, by) lies
 * inside the layer.
 * fd_sample_windows: host only (no context, no device).  The kept layers are given by their pyramid index, scale and size, in
 * increasing index order without gaps (as fd_pyramid_layer_info reports them).  xywh: n x {x, y, width, height};
 * windows: n x {layer position, bx, by, valid}; rows of samples without a window are {-1, 0, 0, 0}.
 * fd_pyramid_sample_windows: the same on the kept layers of an updated pyramid. */
int fd_sample_windows(int n_layers, const int32_t* layer_index, const double* layer_scale, const int32_t* layer_w, const int32_t* layer_h,
                      double incremental_scale, int patch_w, int patch_h, int n, const int32_t* xywh, int32_t* windows);
int fd_pyramid_sample_windows(const fd_pyramid* p, int patch_w, int patch_h, int n, const int32_t* xywh, int32_t* windows);
/* samples per call of the three entry points below */
enum { FD_HIST_SAMPLES_MAX = 1 << 20 };
int fd_hist_samples_limits(int* max_samples);
/* The four FD_HIST_* patch filters on the sampled windows of a FD_LAYER_GRADBIN, FD_LAYER_LBP or FD_LAYER_GRADMAG_LBP pyramid:
 * features is n x fd_hist_feature_length floats, valid n bytes (either may be NULL); the rows of samples without a window are zero.
 * hp->step_x / step_y are ignored.  Bit for bit what fd_hist_patch_batch gives on the patches cut from the layers. */
int fd_hist_extract_samples(fd_ctx* ctx, fd_pyramid* p, const fd_hist_params* hp, int n, const int32_t* xywh, uint8_t* valid, float* features);
/* ExtendedHogFilter on the sampled windows of a FD_LAYER_GRADBIN pyramid: n x fd_ehog_feature_length floats, as fd_ehog_patch_batch */
int fd_ehog_extract_samples(fd_ctx* ctx, fd_pyramid* p, const fd_ehog_patch_params* ep, int n, const int32_t* xywh, uint8_t* valid,
                            float* features);
/* condensation::SingleClassifierModel::evaluate (SingleClassifierModel.cpp:32-52) on a DirectPyramidFeatureExtractor with one of
 * those patch filters and a ProbabilisticSvmClassifier on f32 vectors: kind FD_SAMPLES_HIST (params: const fd_hist_params*) or
 * FD_SAMPLES_EHOG (params: const fd_ehog_patch_params*).  The features stay on the device and are scored by the kernel of
 * fd_svm_distance_batch; target = distance >= threshold, weight = the logistic probability; samples without a window get target
 * 0, weight 0.
 * FD_ERR_INVALID_ARGUMENT, before anything is launched: a multi-frame pyramid, a pyramid without an image, a layer kind the
 * filter does not read, a bin count other than the layer filter's, an SVM of another dimension or on u8 vectors, n < 0 or
 * n > FD_HIST_SAMPLES_MAX.  n == 0 or no sample with a window: FD_OK without a launch. */
enum { FD_SAMPLES_HIST = 0, FD_SAMPLES_EHOG = 1 };
int fd_hist_svm_evaluate_samples(fd_ctx* ctx, fd_pyramid* p, int kind, const void* params, const fd_svm* svm, int n, const int32_t* xywh,
                                 uint8_t* target, double* weight);
/* ... the same call that also reports the hyperplane distances (n doubles; 0 for samples without a window) */
int fd_hist_svm_evaluate_samples_distance(fd_ctx* ctx, fd_pyramid* p, int kind, const void* params, const fd_svm* svm, int n,
                                          const int32_t* xywh, uint8_t* target, double* weight, double* distance);
/* SlidingWindowDetector::detect with the histogram patch filter + ProbabilisticSvmClassifier on the f32
 * vectors (any kernel; wiring of BenchmarkRunner.cpp:185-263) */
int fd_detect_hist_svm(fd_ctx* ctx, fd_pyramid* p, const fd_svm* svm, const fd_hist_params* hp, fd_detection* out,
                       int64_t cap, int64_t* count, double* all_distance);

/* The "whi" feature space of ffpDetectApp.cpp:449-454 on gray pyramid windows: WhiteningFilter(alpha, cutoff)
 * (WhiteningFilter.cpp:20-81) -> HistogramEqualizationFilter (cv::equalizeHist) -> ConversionFilter(CV_32F,
 * 1/127.5, -1) -> UnitNormFilter(NORM_L2).  Reference defaults: alpha 1, cutoff 0.390625 (WhiteningFilter.hpp:31). */
typedef struct {
    int32_t patch_w, patch_h, step_x, step_y;
    float alpha, cutoff;
} fd_whi_params;
/* the chain on n contiguous w x h u8 patches (host) -> n*w*h floats (host) */
int fd_whi_batch(fd_ctx* ctx, const uint8_t* patches, int64_t n, int w, int h, float alpha, float cutoff, float* dst);
/* HistogramEqualizationFilter::applyTo ("histeq" feature space, ffpDetectApp.cpp:446-448) on n patches */
int fd_equalize_hist_batch(fd_ctx* ctx, const uint8_t* patches, int64_t n, int w, int h, uint8_t* dst);
/* the single filters of that chain on n contiguous host patches / vectors (their per-Mat ImageFilter::applyTo):
 *  fd_whitening_batch  WhiteningFilter(alpha, cutoff) alone (WhiteningFilter.cpp:20-58): u8 -> u8 (convertTo(CV_8U, 1, 127))
 *  fd_convert_batch    ConversionFilter(type, alpha, beta) (cv::Mat::convertTo): src/dst dtype FD_DTYPE_U8 | FD_DTYPE_F32, `count` values
 *  fd_unit_norm_batch  UnitNormFilter(normType) (UnitNormFilter.cpp:24-43): n vectors of `len` floats, norm_type = cv::NORM_INF 1,
 *                      NORM_L1 2, NORM_L2 4 */
int fd_whitening_batch(fd_ctx* ctx, const uint8_t* patches, int64_t n, int w, int h, float alpha, float cutoff, uint8_t* dst);
int fd_convert_batch(fd_ctx* ctx, const void* src, int src_dtype, int64_t count, double alpha, double beta, void* dst, int dst_dtype);
int fd_unit_norm_batch(fd_ctx* ctx, const float* src, int64_t n, int len, int norm_type, float* dst);
/* every window of the pyramid: n_windows x (patch_w*patch_h) floats to host; features == NULL: count only */
int fd_extract_whi(fd_ctx* ctx, fd_pyramid* p, const fd_whi_params* wp, float* features, int64_t cap_windows, int64_t* count);
/* SlidingWindowDetector::detect with the whi feature space + ProbabilisticSvmClassifier (any kernel, f32 vectors) */
int fd_detect_whi_svm(fd_ctx* ctx, fd_pyramid* p, const fd_svm* svm, const fd_whi_params* wp, fd_detection* out, int64_t cap,
                      int64_t* count, double* all_distance);

/* ---- integral-image features on sampled windows: the "haar" and "surf" feature types of benchmarkApp (BenchmarkRunner.cpp:225-233,
 * 278-286) and the measurement model of the tracking apps ---------------------------------------------------------------------------
 * Image filters GrayscaleFilter -> IntegralImageFilter (IntegralImageFilter.cpp:18-21: cv::integral, sdepth CV_32S) of a
 * DirectImageFeatureExtractor: (height + 1) x (width + 1) int32, first row and column zero, I[y+1][x+1] = sum of gray[v][u] over
 * v <= y, u <= x.  There is no pyramid: rectangle sums are scale-free.  An image with 255 * width * height > 2^31 - 1 is rejected
 * with FD_ERR_INVALID_ARGUMENT before its data is touched (the reference's sums would wrap silently). */
typedef struct fd_integral fd_integral;
int fd_integral_create(fd_ctx* ctx, fd_integral** out);
void fd_integral_destroy(fd_integral* g);
/* DirectImageFeatureExtractor::update (DirectImageFeatureExtractor.cpp:35-40).  channels 1 (gray) or 3 (BGR, interleaved; the
 * pyramid's BGR -> gray arithmetic); is_device != 0: image already resident in HBM. */
int fd_integral_update(fd_integral* g, const uint8_t* image, int width, int height, int channels, int is_device);
/* an integral image made elsewhere (host, width x height int32, CV_32SC1) instead of an update: what the stand-alone
 * HaarFeatureFilter / IntegralGradientFilter::applyTo(const Mat&) of the host layer are given */
int fd_integral_set_image(fd_integral* g, const int32_t* integral, int width, int height);
/* size of the integral image (image width + 1, image height + 1); 0, 0 before the first update */
int fd_integral_size(const fd_integral* g, int* width, int* height);
/* copy the integral image to host: (height + 1) * (width + 1) int32 */
int fd_integral_download(fd_integral* g, int32_t* host_dst);
/* IntegralImageFilter::applyTo on a CV_8UC1 host image: (height + 1) * (width + 1) int32 to host */
int fd_integral_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, int32_t* dst);

/* Sample windows.  Every extraction call below takes n samples xywh[n][4] = {x, y, width, height} (Sample::getX / getY / getWidth /
 * getHeight) and follows DirectImageFeatureExtractor::extract (DirectImageFeatureExtractor.cpp:42-52) on the integral image: the
 * patch origin is (x - width / 2, y - height / 2) (integer division), and the patch exists iff it lies inside the integral image
 * (and width, height >= 1).  valid[n] receives 1 for every sample whose patch exists and whose filter reads all lie inside the
 * integral image, else 0; the output rows of the other samples are zero.  features / dst2ch and valid may be NULL: the results
 * then stay on the device only (what fd_integral_svm_evaluate_samples consumes). */

/* HaarFeatureFilter (HaarFeatureFilter.hpp:24-32, HaarFeatureFilter.cpp:18-158).  types: bit mask of FD_HAAR_*. */
enum { FD_HAAR_2RECTANGLE = 1, FD_HAAR_3RECTANGLE = 2, FD_HAAR_4RECTANGLE = 4, FD_HAAR_CENTER_SURROUND = 8, FD_HAAR_ALL = 15 };
typedef struct {
    const float* sizes;   /* feature sizes relative to the patch */
    int32_t num_sizes;
    const float* xs;      /* grid coordinates of the feature centres, relative to the patch */
    int32_t num_xs;
    const float* ys;
    int32_t num_ys;
    int32_t types;
} fd_haar_params;
typedef struct {
    float rects[4][4];    /* cv::Rect_<float>: x, y, width, height, relative to the patch */
    float weights[4];
    int32_t num_rects;
    float factor, area;
} fd_haar_feature;
/* Host only (no context, no device).  fd_haar_grid: the equidistant grid of the (sizes, count, types) constructors, coords[i] =
 * (i + 1) * (1.f / (count + 1)) (HaarFeatureFilter.cpp:41-51).  fd_haar_feature_count: number of features buildFeatures
 * (:53-136) makes, -1 on invalid parameters (NULL, a negative count, types outside the mask, a rectangle edge outside [0, 1] or not
 * finite).  fd_haar_features: that feature table, built in float with the reference's expressions and order; FD_ERR_CAPACITY when
 * cap is too small (*count is set). */
int fd_haar_grid(int count, float* coords);
int fd_haar_feature_count(const fd_haar_params* hp);
int fd_haar_features(const fd_haar_params* hp, fd_haar_feature* out, int cap, int* count);
/* HaarFeatureFilter::applyTo (:138-158) per sample: n x fd_haar_feature_count floats.  Corners are cvRound(float product) of the
 * relative coordinates and the patch size, sums are int32, value += weight * (float)sum per rectangle, then
 * value / (factor * area * cols * rows), all in float.  One deviation: a rectangle edge at 1.0 reads column `cols` / row `rows` of
 * the patch, one past the ROI; where that leaves the integral image (a patch flush with its last column or row; the reference
 * reads out of the row there) the sample is invalid. */
int fd_integral_extract_haar(fd_ctx* ctx, fd_integral* g, const fd_haar_params* hp, int n, const int32_t* xywh, float* features,
                             uint8_t* valid);
/* IntegralGradientFilter(rows, cols)::applyTo (IntegralGradientFilter.cpp:23-85) per sample: rows x cols CV_8UC2 (dx + 127,
 * dy + 127) from twelve reads around each grid point; radii, spacings and offsets in double with cvRound, integer divisions
 * truncating.  2 <= rows, cols <= 16384 (below 2 the reference divides by zero).  With patch width and height >= 4 all reads stay inside
 * the patch; for smaller patches they may leave it, and the rule above decides. */
int fd_integral_gradient_patches(fd_ctx* ctx, fd_integral* g, int rows, int cols, int n, const int32_t* xywh, uint8_t* dst2ch,
                                 uint8_t* valid);
/* GradientSumFilter(cell_rows, cell_cols)::applyTo (GradientSumFilter.cpp:22-60) on n contiguous CV_8UC2 host patches of rows x
 * cols pixels: per cell (sum dx, sum dy, sum |dx|, sum |dy|) with dx = (1.f / 127.f) * (g - 127), summed in the reference's
 * order; n x cell_rows * cell_cols * 4 floats to host.  rows % cell_rows != 0 or cols % cell_cols != 0: FD_ERR_INVALID_ARGUMENT. */
int fd_gradient_sum_batch(fd_ctx* ctx, const uint8_t* grad2ch, int64_t n, int rows, int cols, int cell_rows, int cell_cols, float* dst);
/* The SURF-like descriptor of createSurfExtractor (BenchmarkRunner.cpp:278-286): IntegralGradientFilter(gradient_count) ->
 * GradientSumFilter(cell_count) -> UnitNormFilter(NORM_L2) in one launch (the gradient patch never goes to memory):
 * n x 4 * cell_count^2 floats, identical to the three stand-alone calls in a row.  2 <= gradient_count <= 64, divisible by
 * cell_count, and the patch and the descriptor of four samples must fit the 160 KB of LDS of a workgroup:
 * 4 * (2 * gradient_count^2 rounded up to 16 + 16 * cell_count^2) <= 163840 bytes.  That admits every cell_count <= 32 and, with
 * cell_count == gradient_count, up to 47; (48, 48), (56, 56) and (64, 64) are FD_ERR_INVALID_ARGUMENT (the stand-alone calls have
 * no such limit). */
int fd_integral_extract_surf(fd_ctx* ctx, fd_integral* g, int gradient_count, int cell_count, int n, const int32_t* xywh,
                             float* features, uint8_t* valid);
/* condensation::SingleClassifierModel::evaluate (SingleClassifierModel.cpp:32-52) with a ProbabilisticSvmClassifier on f32 vectors:
 * kind FD_INTEGRAL_HAAR (params: const fd_haar_params*) or FD_INTEGRAL_SURF (params: const fd_surf_params*).  The features stay on
 * the device and are scored by the kernel of fd_svm_distance_batch; target = distance >= threshold, weight = the logistic
 * probability; samples without a (valid) patch get target 0, weight 0.  FD_ERR_INVALID_ARGUMENT when the feature length differs
 * from the SVM's dimension. */
enum { FD_INTEGRAL_HAAR = 0, FD_INTEGRAL_SURF = 1 };
typedef struct {
    int32_t gradient_count, cell_count;
} fd_surf_params;
int fd_integral_svm_evaluate_samples(fd_ctx* ctx, fd_integral* g, int kind, const void* params, const fd_svm* svm, int n,
                                     const int32_t* xywh, uint8_t* target, double* weight);
/* The integral HOG family, the "ihog" and "iehog" feature types of the tracking apps (AdaptiveTracking.cpp:189-213):
 * IntegralGradientFilter(grad_rows, grad_cols) -> GradientBinningFilter(bins, signed_gradients, interpolate_bins) -> one of the four
 * FD_HIST_* patch filters (kind FD_SAMPLES_HIST) or ExtendedHogFilter (kind FD_SAMPLES_EHOG), per sample in one launch: the
 * gradient patch and the bin image stay in LDS.  Bit for bit what fd_integral_gradient_patches -> fd_gradient_binning_image ->
 * fd_hist_patch_batch / fd_ehog_patch_batch give.  xywh is what the innermost DirectImageFeatureExtractor::extract receives: the
 * maps of IntegralFeatureExtractor (+1) and PatchResizingFeatureExtractor (scale) are the caller's.
 * FD_ERR_INVALID_ARGUMENT: a grid side outside 2..64, bins outside 1..255, a filter patch other than grad_cols x grad_rows, filter
 * bins other than `bins`, whatever fd_hist_feature_length / fd_ehog_feature_length refuse with interpolate_bins ? 4 : 2 channels,
 * and a configuration whose four samples per workgroup do not fit the 160 KB of LDS (tables + 4 * (2|4 * rows * cols rounded up to
 * 16 + the vector area of the histogram filter); the three stand-alone calls serve those). */
typedef struct {
    int32_t grad_rows, grad_cols;                      /* IntegralGradientFilter(rows, cols): 2..64 each */
    int32_t bins, signed_gradients, interpolate_bins;  /* GradientBinningFilter(bins, signed, interpolate) */
    int32_t kind;                                      /* FD_SAMPLES_HIST: `hist` is read; FD_SAMPLES_EHOG: `ehog` is read */
    fd_hist_params hist;                               /* patch_w == grad_cols, patch_h == grad_rows, bins == bins; step_x / step_y ignored */
    fd_ehog_patch_params ehog;                         /* same three equalities */
} fd_integral_hog_params;
enum { FD_INTEGRAL_HOG = 2 };   /* fd_integral_svm_evaluate_samples: params is a const fd_integral_hog_params* */
/* host only: floats per sample, or -1 where fd_integral_extract_hog returns FD_ERR_INVALID_ARGUMENT */
int fd_integral_hog_feature_length(const fd_integral_hog_params* hp);
/* host only: valid[i] = 1 iff sample i of a width x height image has a patch and every read of IntegralGradientFilter(rows, cols)
 * lies inside the integral image -- the statements the kernels run.  2 <= rows, cols <= 16384. */
int fd_integral_gradient_samples_valid(int width, int height, int rows, int cols, int n, const int32_t* xywh, uint8_t* valid);
/* n x fd_integral_hog_feature_length floats; rows of samples without a valid patch are zero.  features or valid may be NULL. */
int fd_integral_extract_hog(fd_ctx* ctx, fd_integral* g, const fd_integral_hog_params* hp, int n, const int32_t* xywh, float* features,
                            uint8_t* valid);
/* Host only (no context, no device): the argument rules of the calls above, which use these very functions.  Each returns the
 * length of one output, or -1 where the call returns FD_ERR_INVALID_ARGUMENT.  fd_integral_image_length: (width + 1) * (height + 1)
 * ints; -1 for a size below 1 or 255 * width * height > 2^31 - 1.  fd_integral_gradient_length: 2 * rows * cols bytes per sample;
 * -1 unless 2 <= rows, cols <= 16384.  fd_gradient_sum_length: 4 * cell_rows * cell_cols floats per patch; -1 for the two
 * divisibility errors of GradientSumFilter.cpp:25-28, a count below 1 or rows, cols > 16384.  fd_surf_feature_length:
 * 4 * cell_count^2 floats per sample; -1 by the rules of fd_integral_extract_surf. */
int fd_integral_image_length(int width, int height);
int fd_integral_gradient_length(int rows, int cols);
int fd_gradient_sum_length(int rows, int cols, int cell_rows, int cell_cols);
int fd_surf_feature_length(int gradient_count, int cell_count);

/* ---- the resident particle set (fd_particles, above) on the integral-feature models with an optical-flow transition
 *  -----------------
 * A frame of ResamplingSampler(LowVarianceSampling, OpticalFlowTransitionModel(fallback SimpleTransitionModel)) +
 * SingleClassifierModel on a Haar / SURF / integral HOG extractor + FilteringStateExtractor(WeightedMeanStateExtractor) is
 * fd_flow_update, fd_integral_update, fd_flow_track_fb_resident, fd_particles_sample_flow, _evaluate_integral, _weigh_classifier and
 * _state_flow: one chain of kernels on the context's stream and one read-back. */
/* A particle set like fd_particles_create's with no tracker.  fd_particles_evaluate on it is FD_ERR_RUNTIME (nothing is launched);
 * every other call works on it unchanged. */
int fd_particles_create_unbound(fd_ctx* ctx, int capacity, fd_particles** out);
/* The wrapper chain of a feature extractor as data, outer to inner: what each wrapper asks its inner extractor for.
 * FD_SAMPLE_MAP_RESIZE is PatchResizingFeatureExtractor (x = cvRound(x + x_offset * width), y = cvRound(y + y_offset * height),
 * width = cvRound(factor * width), height = cvRound(factor * height), the sums and products in double, cvRound to the nearest even
 * on a tie; a result outside the int range saturates, a NaN gives 0 -- the same on the host and on the device);
 * FD_SAMPLE_MAP_INTEGRAL is IntegralFeatureExtractor (x, y += 1 where the width, height is odd; width, height += 1; sizes are expected
 * below INT32_MAX). */
enum { FD_SAMPLE_MAP_RESIZE = 0, FD_SAMPLE_MAP_INTEGRAL = 1 };
#define FD_SAMPLE_MAPS_MAX 4
typedef struct {
    int32_t kind;                      /* FD_SAMPLE_MAP_* */
    double factor, x_offset, y_offset; /* FD_SAMPLE_MAP_RESIZE only */
} fd_sample_map;
/* host only: the n_maps <= FD_SAMPLE_MAPS_MAX maps applied in order to each of the n samples {x, y, width, height}, in place */
int fd_sample_maps_apply(const fd_sample_map* maps, int n_maps, int n, int32_t* xywh);
/* SingleClassifierModel::evaluate's scoring for the current generation, nothing copied back: every sample {x, y, size,
 * cvRound(aspect_ratio * size)} goes through the maps on the device into g's sample list, the kernels of
 * fd_integral_svm_evaluate_samples (kind, params, svm as there) extract and score it, the distances become the generation's scores
 * and the kernels' validity bytes the set's valid flags.  fd_particles_get_trace then reports the mapped {x, y, width, height} as
 * the windows.  FD_ERR_INVALID_ARGUMENT for more than FD_SAMPLE_MAPS_MAX maps, an unknown map kind, an SVM that is u8 or of
 * another dimension; FD_ERR_RUNTIME when g holds no image. */
int fd_particles_evaluate_integral(fd_ctx* ctx, fd_particles* p, fd_integral* g, int kind, const void* params, const fd_svm* svm,
                                   double aspect_ratio, const fd_sample_map* maps, int n_maps);
/* SingleClassifierModel.cpp:32-42 on the scores of an _evaluate: a sample without a valid patch gets target 0, weight 0, score 0;
 * any other target = score >= threshold and weight = p(score) with ProbabilisticSvmClassifier's logistic (a, b): the weight is set,
 * not multiplied.  best_score, n_valid and bad_weight as fd_particles_weigh leaves them. */
int fd_particles_weigh_classifier(fd_ctx* ctx, fd_particles* p, double logistic_a, double logistic_b, double threshold);
/* OpticalFlowTransitionModel's median flow (fd_flow_median) as the device leaves it */
typedef struct {
    int32_t ok, n_valid, n_correct;
    float median_x, median_y, median_ratio;
} fd_flow_motion_info;
#define FD_FLOW_RESIDENT_MAX_POINTS 1024
/* fd_flow_track_fb whose results stay on the device: uploads the n <= FD_FLOW_RESIDENT_MAX_POINTS points, queues both trackings and
 * the median flow of the tracks (fd_flow_median's values, bit for bit; a median that is a NaN is the default NaN) and waits for
 * nothing.  FD_ERR_RUNTIME before the second fd_flow_update. */
int fd_flow_track_fb_resident(fd_ctx* ctx, fd_flow* flow, const float* pts_xy, int n);
/* what the last fd_flow_track_fb_resident left (FD_ERR_RUNTIME without one): fwd, bwd (2 n floats each), the status bytes, and
 * order / *n_valid / *n_correct as fd_flow_median reports them (the order is computed on the host from the downloaded tracks).  Any
 * pointer may be NULL; *n receives the point count.  Waits; not for the frame path. */
int fd_flow_get_tracks(fd_ctx* ctx, fd_flow* flow, int cap, int* n, float* fwd, float* bwd, uint8_t* fstatus, uint8_t* bstatus, int32_t* order,
                       int* n_valid, int* n_correct);
/* test hook: the median-flow kernel on the caller's arrays (host memory, n <= FD_FLOW_RESIDENT_MAX_POINTS); the result is written to
 * *out and stays in the handle as the motion of a resident track does (fd_flow_get_tracks does not see these arrays) */
int fd_debug_flow_motion(fd_ctx* ctx, fd_flow* flow, const float* pts, const float* fwd, const float* bwd, const uint8_t* fstatus,
                         const uint8_t* bstatus, int n, fd_flow_motion_info* out);
/* fd_particles_sample with the motion the flow handle holds on the device (fd_flow_track_fb_resident): where it is ok, copy i is moved as
 * OpticalFlowTransitionModel::predict moves it (.cpp:173-190: vx = median_x + d0, vy = median_y + d1, vsize = median_ratio * d2 in
 * double with flow_diffusion[3 i .. 3 i + 2] = {positionDeviation * z, positionDeviation * z, pow(2, sizeDeviation * z)}),
 * otherwise as fd_particles_sample moves it with fallback_diffusion.  The device takes the branch; both blocks hold
 * 3 * n_resampled draws.  FD_ERR_RUNTIME when the flow handle holds no motion. */
int fd_particles_sample_flow(fd_ctx* ctx, fd_particles* p, fd_flow* flow, int count, int n_resampled, double u, const double* flow_diffusion,
                             const double* fallback_diffusion, const int32_t* fresh, int32_t first_fresh_cluster_id);
/* fd_particles_state that brings the flow handle's motion back in the same wait: the one read-back of such a frame */
int fd_particles_state_flow(fd_ctx* ctx, fd_particles* p, fd_flow* flow, fd_particles_info* info, fd_flow_motion_info* motion);

/* ---- the additional negatives of condensation::PositionDependentMeasurementModel::adapt (PositionDependentMeasurementModel.cpp:172-192),
 * chosen on the device behind the state: of the samples outside a box around the extracted state the max_count with
 * the largest weights.  The reference walks the samples in index order and keeps a list ascending by weight that puts a new element
 * before equal ones; in closed form the result is the max_count samples largest under (weight descending, index ascending), listed
 * by (weight ascending, index descending).  Every sample of the generation is a candidate, those without a window (weight 0) too.
 * A sample {x, y, size} is outside when x <= xLow || x >= xHigh || y <= yLow || y >= yHigh || size <= sizeLow || size >= sizeHigh
 * with, for the state {X, Y, S}: offset = (int)(offset_factor * S) in float, xLow = X - offset, xHigh = X + offset, the same for y,
 * sizeLow = (int)(down_scale * S), sizeHigh = (int)(up_scale * S).  The caller forms down_scale = 1 - offset_factor and up_scale =
 * 1 / down_scale as floats; the float -> int conversions truncate and saturate, the int sums wrap. */
#define FD_PARTICLES_NEGATIVES_MAX 64
typedef struct {
    int32_t max_count;                 /* 1 .. FD_PARTICLES_NEGATIVES_MAX: sampleAdditionalNegatives */
    float offset_factor;               /* negativeOffsetFactor */
    float down_scale, up_scale;
} fd_particles_negatives_params;
typedef struct {
    int32_t index;                     /* of the sample in the generation */
    int32_t x, y, size;
    double weight;
} fd_particles_negative;
/* host only, no context: the six bounds {xLow, xHigh, yLow, yHigh, sizeLow, sizeHigh} of a state by the expressions above, the one copy
 * the kernel uses as well.  Defined for every float (the host layer's generic route calls it whatever its factor is: a product that
 * is infinite saturates, a NaN gives 0); max_count is not read.  FD_ERR_INVALID_ARGUMENT for NULL. */
int fd_particles_negatives_bounds(const fd_particles_negatives_params* params, int32_t x, int32_t y, int32_t size, int32_t bounds[6]);
/* fd_particles_state (flow NULL, motion NULL) or fd_particles_state_flow with the selection queued behind the state kernel: *info and
 * *motion as those calls report them, *count <= max_count records in out[0 .. *count) (room for max_count), all in the one wait.
 * Without a state, and with bad_weight (FD_ERR_RUNTIME, *info filled), *count is 0.  FD_ERR_INVALID_ARGUMENT before anything is queued
 * for max_count outside 1 .. FD_PARTICLES_NEGATIVES_MAX, floats of params that are not finite, NULL arguments (motion must be NULL
 * exactly when flow is) and objects of different contexts. */
int fd_particles_state_negatives(fd_ctx* ctx, fd_particles* p, fd_flow* flow, const fd_particles_negatives_params* params, fd_particles_info* info,
                                 fd_flow_motion_info* motion, int* count, fd_particles_negative* out);

/* ---- the examples of condensation::SelfLearningMeasurementModel::adapt (SelfLearningMeasurementModel.cpp:89-125), chosen on the
 * device behind the state and extracted there.  Two lists over the generation's weights: the positive candidates have
 * weight > positive_threshold, the negative ones weight < negative_threshold, both strict and in double; with require_window a
 * candidate also needs the valid flag the generation's evaluate left (the usable branch, .cpp:68-71), without it every sample is a
 * candidate (the bootstrap branch, :103-110) and the extraction decides.  A side with at most max_count candidates lists them in index
 * order (the reference does not sort then); a side with more lists the max_count best in sorted order: positives by (weight
 * descending, index ascending), negatives by (weight ascending, index ascending).  The reference's std::sort is unstable; "lower
 * index first" is this project's rule.  The lists do not depend on whether a state was found.  The reference tests the negative
 * threshold only where the positive one was not passed; the two tests here are independent, which is the same for negative_threshold <=
 * positive_threshold, and a negative_threshold above the positive one is refused (FD_ERR_INVALID_ARGUMENT). */
#define FD_PARTICLES_EXAMPLES_MAX 32
typedef struct {
    double positive_threshold, negative_threshold;   /* finite, negative_threshold <= positive_threshold */
    int32_t max_count;                                /* 1 .. FD_PARTICLES_EXAMPLES_MAX per side; the reference's 10 */
    int32_t require_window;                           /* 0 / 1 */
} fd_particles_examples_params;
typedef struct {
    int32_t index;                     /* of the sample in the generation */
    int32_t x, y, size;
    int32_t valid;                     /* the extraction found a patch: the record has a feature row */
    double weight;
} fd_particles_example;
/* host only, no context: the two lists of a generation given as arrays (valid may be NULL when require_window is 0), by the
 * comparisons k_particles_examples runs: the indices of the chosen samples in list order, room for max_count each.
 * FD_ERR_INVALID_ARGUMENT for NULL, n < 0, max_count outside 1 .. FD_PARTICLES_EXAMPLES_MAX, thresholds that are not finite or inverted;
 * FD_ERR_RUNTIME (both counts 0) when a weight is negative or not finite. */
int fd_particles_examples_select(int n, const double* weight, const uint8_t* valid, const fd_particles_examples_params* params, int* n_pos,
                                 int32_t* pos_index, int* n_neg, int32_t* neg_index);
/* host only: floats per feature row of an extractor and the floats `rows` must hold, 2 * max_count rows.  family
 * FD_EXAMPLES_INTEGRAL: kind FD_INTEGRAL_*, params as fd_particles_evaluate_integral takes them; family FD_EXAMPLES_PYRAMID: kind
 * FD_SAMPLES_HIST / _EHOG / _PATCH, params as fd_particles_evaluate_pyramid takes them, channels the channel count of the pyramid's bin
 * image as fd_hist_feature_length / fd_ehog_feature_length take it (not read for the other kinds).  FD_ERR_INVALID_ARGUMENT where the
 * extractor's own length query refuses the parameters, for an unknown family or kind, NULL and max_count outside
 * 1 .. FD_PARTICLES_EXAMPLES_MAX. */
enum { FD_EXAMPLES_INTEGRAL = 0, FD_EXAMPLES_PYRAMID = 1 };
int fd_particles_examples_bounds(int family, int kind, const void* params, int channels, int max_count, int* row_length, int* row_capacity);
/* fd_particles_state (flow NULL, motion NULL) or fd_particles_state_flow with the selection queued behind the state kernel and the
 * chosen samples' feature rows behind that: the up to 2 * max_count samples {x, y, size, cvRound(aspect_ratio * size)} go through the
 * maps on the device (the adaptive extractor's chain, whatever chain the generation was evaluated with) and the family's list kernel
 * of fd_integral_extract_haar / _surf / _hog runs on that list with a fixed launch size; unused slots hold an empty window and are
 * not computed.  *info, *motion, both record lists (room for max_count each) with their valid flags, and the rows come back in one
 * copy and one wait.  Row r of `rows` (*row_length floats) belongs to pos[r] for r < *n_pos and to neg[r - *n_pos] after that, bit for
 * bit the row the extract call returns for that sample; the row of a record that is not valid is not written.  With bad_weight
 * (FD_ERR_RUNTIME, *info filled) both counts are 0.  FD_ERR_INVALID_ARGUMENT before anything is queued: max_count outside
 * 1 .. FD_PARTICLES_EXAMPLES_MAX, thresholds that are not finite or inverted, require_window other than 0 / 1, row_capacity below
 * 2 * max_count * row length, the maps' and the extractor's own rules, NULL arguments (motion NULL exactly when flow is), objects of
 * different contexts.  FD_ERR_RUNTIME with require_window on a generation that has not been evaluated. */
int fd_particles_state_examples_integral(fd_ctx* ctx, fd_particles* p, fd_flow* flow, fd_integral* g, int kind, const void* params,
                                         double aspect_ratio, const fd_sample_map* maps, int n_maps,
                                         const fd_particles_examples_params* examples_params, fd_particles_info* info, fd_flow_motion_info* motion,
                                         int* n_pos, fd_particles_example* pos, int* n_neg, fd_particles_example* neg, float* rows, int row_capacity,
                                         int* row_length);

/* ---- classification::RvmClassifier / ProbabilisticRvmClassifier -----------------
 * Cascaded reduced-vector machine (RvmClassifier.cpp:75-126): level k evaluates kernel(x, rsv_k) on the whole
 * vector; through the reference's cached path the running distance is d_0 = -bias + c[0][0] K_0,
 * d_k = d_{k-1} + c[k][k] K_k; a vector leaves at the first level with d_k < thresholds[k]; positive iff the last
 * used level is passed.  Probability = 1/(1+exp(a + b d)) for every vector (ProbabilisticRvmClassifier.cpp:62). */
typedef struct fd_rvm fd_rvm;
typedef struct {
    int32_t kernel;                 /* FD_KERNEL_* (the reference's loader builds RBF or polynomial, RvmClassifier.cpp:196-204) */
    double p0, p1, p2;              /* like fd_svm_model */
    int32_t num_filters, num_used;  /* num_used: setNumFiltersToUse (0 or > num_filters: all) */
    int32_t filter_w, filter_h;     /* reduced set vectors are filter_h x filter_w f32 images */
    const float* support_vectors;   /* [num_filters][filter_w*filter_h] */
    const float* coefficients;      /* lower triangle, coefficients[k][i] (i <= k) at k(k+1)/2 + i */
    const float* thresholds;        /* [num_filters] hierarchicalThresholds */
    float bias;
    double logistic_a, logistic_b;
} fd_rvm_model;
int fd_rvm_create(fd_ctx* ctx, const fd_rvm_model* model, fd_rvm** out);
void fd_rvm_destroy(fd_rvm* m);
/* computeHyperplaneDistance (RvmClassifier.cpp:75-85) of n f32 vectors (host): last level and distance */
int fd_rvm_eval_batch(fd_ctx* ctx, const fd_rvm* rvm, const float* features, int64_t n, int32_t* out_level, double* out_distance);
/* u8 patch feature spaces of ffpDetectApp.cpp:446-461 */
enum { FD_FEATURE_GRAY = 0, FD_FEATURE_HQ64 = 1, FD_FEATURE_HISTEQ = 2 };
typedef struct {
    int32_t feature_space;          /* FD_FEATURE_* */
    float conv_scale, conv_shift;   /* ConversionFilter(CV_32F, scale, shift): x = float(u8) * scale + shift */
    int32_t step_x, step_y;
} fd_rvm_detect_params;
/* SlidingWindowDetector::detect (SlidingWindowDetector.cpp:87-98) with a ProbabilisticRvmClassifier ("prvm",
 * ffpDetectApp.cpp:484).  all_level / all_distance (may be NULL): per window in extraction order. */
int fd_detect_rvm(fd_ctx* ctx, fd_pyramid* p, const fd_rvm* rvm, const fd_rvm_detect_params* dp, const int* roi, fd_detection* out,
                  int64_t cap, int64_t* count, int32_t* all_level, double* all_distance);
/* FiveStageSlidingWindowDetector::detect (:187-320, roi == NULL; :331-380 with roi) with a ProbabilisticRvmClassifier first stage
 * ("firstClassifier prvm"): RVM cascade -> OverlapElimination(dist, ratio) -> second->classify(patch data) -> positives ->
 * [block NMS, no-roi only] -> sort.  Stage 1 is fd_detect_rvm.  The second classifier sees the first stage's own feature vector,
 * float(u8) * conv_scale + conv_shift: exactly one of second_svm (f32 support vectors of filter_w * filter_h values) and second_rvm
 * (same filter size, another handle than `first`) is non-NULL.  A positive of the second stage carries its hyperplane distance as
 * score and probability 0.5 (classify() gives a bool only).  stage_counts[4] as fd_detect_five_stage.  FD_ERR_INVALID_ARGUMENT, before
 * anything runs, for any other pairing and for a multi-frame or layer-filtered pyramid. */
int fd_detect_five_stage_rvm(fd_ctx* ctx, fd_pyramid* p, const fd_rvm* first, const fd_rvm_detect_params* dp, const fd_svm* second_svm,
                             const fd_rvm* second_rvm, float oe_dist, float oe_ratio, const int* roi, fd_detection* out, int cap, int* count,
                             int32_t* stage_counts);
/* fd_pyramid_update (with the pyramid's image filter) + fd_detect_five_stage_rvm in one call, as fd_detect_five_stage_image */
int fd_detect_five_stage_rvm_image(fd_ctx* ctx, fd_pyramid* p, const fd_rvm* first, const fd_rvm_detect_params* dp, const fd_svm* second_svm,
                                   const fd_rvm* second_rvm, const uint8_t* image, int width, int height, int channels, int image_is_device,
                                   float oe_dist, float oe_ratio, const int* roi, fd_detection* out, int cap, int* count, int32_t* stage_counts);

/* ---- gray-patch features and the RVM cascade on explicit sample windows of a gray pyramid (no layer filter): what the tracking apps
 * put on a DirectPyramidFeatureExtractor with the patch filters of HeadTracking.cpp:144-167 -- condensation::SingleClassifierModel,
 * FilteringClassifierModel (FilteringClassifierModel.cpp:27-103) and ClassificationBasedStateValidator (:28-45) ---------------------
 * Feature spaces: FD_FEATURE_GRAY / HQ64 / HISTEQ followed by ConversionFilter(CV_32F, conv_scale, conv_shift), x = float(u8) *
 * scale + shift; FD_FEATURE_WHI: the whole whi chain of fd_whi_params with (whi_alpha, whi_cutoff), which ignores conv_scale and
 * conv_shift (fd_detect_rvm does not take it).  A feature vector has patch_w * patch_h floats, row-major.
 * The sample -> window rule is fd_sample_windows'.  Samples without a window: a zero feature row; target 0, weight 0, distance 0 from
 * the SVM call; valid 0, level -1, distance 0, target 0 from the RVM call.
 * FD_ERR_INVALID_ARGUMENT, before anything is queued: objects of different contexts, a multi-frame pyramid, a pyramid without an image,
 * a layer-filtered pyramid, n < 0 or n > FD_HIST_SAMPLES_MAX, a patch side outside 1..32 (whi: 2..32), an unknown feature space, an RVM
 * whose filter size is not the patch size, an SVM on u8 vectors or of another dimension.  n == 0 or no sample with a window: FD_OK
 * without a launch. */
enum { FD_FEATURE_WHI = 3 };
typedef struct {
    int32_t patch_w, patch_h, feature_space;
    float conv_scale, conv_shift, whi_alpha, whi_cutoff;
} fd_patch_samples_params;
/* host only: patch_w * patch_h, or -1 where the calls below refuse the parameters */
int fd_patch_feature_length(const fd_patch_samples_params* pp);
/* features: n x fd_patch_feature_length floats, valid: n bytes (either may be NULL).  Bit for bit what the per-patch entry points
 * (fd_histeq64 of the patch, fd_equalize_hist_batch, fd_convert_batch, fd_whi_batch) give on the patches cut from the layers. */
int fd_patch_extract_samples(fd_ctx* ctx, fd_pyramid* p, const fd_patch_samples_params* pp, int n, const int32_t* xywh, uint8_t* valid,
                             float* features);
/* SingleClassifierModel::evaluate with a ProbabilisticSvmClassifier on f32 vectors, as fd_hist_svm_evaluate_samples_distance:
 * target = distance >= threshold, weight = the logistic probability; distance may be NULL */
int fd_patch_svm_evaluate_samples(fd_ctx* ctx, fd_pyramid* p, const fd_patch_samples_params* pp, const fd_svm* svm, int n,
                                  const int32_t* xywh, uint8_t* target, double* weight, double* distance);
/* RvmClassifier::computeHyperplaneDistance and classify (RvmClassifier.cpp:68-85) per sample: level and distance as fd_rvm_eval_batch
 * on the extracted row (the same bits), target = the last used level is reached and passed.  valid, level, distance and target may
 * each be NULL.  Inside a measured range of sample counts one kernel gathers, filters and scores a window without writing its feature
 * row; outside it (and for FD_FEATURE_WHI) the rows are written and the cascade of fd_rvm_eval_batch runs on them. */
int fd_patch_rvm_evaluate_samples(fd_ctx* ctx, fd_pyramid* p, const fd_patch_samples_params* pp, const fd_rvm* rvm, int n,
                                  const int32_t* xywh, uint8_t* valid, int32_t* level, double* distance, uint8_t* target);

/* ---- the resident particle set (fd_particles_create_unbound) on the pyramid families: the feature types hog, ehog, lbp, glbp, grayscale,
 *      h and whi of the tracking apps -------------------------------------------------------------------------------------------------
 * The device resolves a sample to its window itself.  Of the rule of fd_sample_windows the placement in the layer is exact arithmetic and
 * is evaluated there; the layer of a width goes through log and is read from a table of the host's values: */
/* host only: layer_of_width[w] = position in the kept-layer list of a sample of width w (the index expression of fd_sample_window,
 * evaluated by the host for every w), -1 for none; [0] = -1.  *length = 1 + the largest width that maps to a kept layer (0: none;
 * INT32_MAX when that width is INT32_MAX).  FD_ERR_CAPACITY with *length set when length > cap.  FD_ERR_INVALID_ARGUMENT as
 * fd_sample_windows for its arguments, and for more than INT16_MAX layers. */
#define FD_SAMPLE_TABLE_MAX 65536
int fd_sample_layer_table(int n_layers, int first_index, double incremental_scale, int patch_w, int cap, int16_t* layer_of_width, int* length);
enum { FD_SAMPLES_PATCH = 2 };   /* next to FD_SAMPLES_HIST / FD_SAMPLES_EHOG; params: const fd_patch_samples_params* */
/* SingleClassifierModel::evaluate's scoring for the current generation of an unbound or bound set on a pyramid chain, nothing copied
 * back: sample -> maps -> window on the device (k_particles_windows), the kernels of fd_hist_svm_evaluate_samples /
 * fd_patch_svm_evaluate_samples on the list, the distances into the generation's scores, the validity into the set's flags;
 * fd_particles_get_trace reports {layer, bx, by, valid}.  Then fd_particles_weigh_classifier as after _evaluate_integral.
 * Every particle keeps its own slot of the window list; the slot of a particle without a window names a window that exists, and its
 * score means nothing until fd_particles_weigh_classifier has set it to 0.  The table above stays in the pyramid handle and is uploaded
 * again only when the patch width or the kept layers change.
 * The argument rules are those of the two calls named (kind, params, svm, pyr as there), except that a pyramid without an image is
 * FD_ERR_RUNTIME.  FD_ERR_INVALID_ARGUMENT also for more than FD_SAMPLE_MAPS_MAX maps, a map other than FD_SAMPLE_MAP_RESIZE, and a
 * pyramid whose table would be longer than FD_SAMPLE_TABLE_MAX.  A refused call launches nothing and leaves the generation "not
 * evaluated".  An empty generation is FD_OK. */
int fd_particles_evaluate_pyramid(fd_ctx* ctx, fd_particles* p, fd_pyramid* pyr, int kind, const void* params, const fd_svm* svm,
                                  double aspect_ratio, const fd_sample_map* maps, int n_maps);
/* fd_particles_state_examples_integral on a pyramid family: the chosen samples go through the maps (FD_SAMPLE_MAP_RESIZE only) and are
 * resolved to windows of pyr on the device by the rule of fd_pyramid_sample_windows (k_particles_windows in list form); the list kernel
 * of fd_hist_extract_samples, fd_ehog_extract_samples (kind FD_SAMPLES_HIST / FD_SAMPLES_EHOG) or fd_patch_extract_samples
 * (FD_SAMPLES_PATCH; every feature space, FD_FEATURE_WHI among them) runs on the 2 * max_count slots.  A slot without a record or
 * without a window is flagged invalid; it lists a spare window so that the kernel reads valid memory, and its row stays on the device.
 * Rows, flags and errors as there, and the argument rules of fd_particles_evaluate_pyramid for pyr, kind, params and the maps. */
int fd_particles_state_examples_pyramid(fd_ctx* ctx, fd_particles* p, fd_flow* flow, fd_pyramid* pyr, int kind, const void* params,
                                        double aspect_ratio, const fd_sample_map* maps, int n_maps,
                                        const fd_particles_examples_params* examples_params, fd_particles_info* info, fd_flow_motion_info* motion,
                                        int* n_pos, fd_particles_example* pos, int* n_neg, fd_particles_example* neg, float* rows, int row_capacity,
                                        int* row_length);

/* ---- the resident particle set on condensation::WvmSvmModel (WvmSvmModel.cpp:69-118), the measurement model of the face tracker ------
 * A frame of this model is one chain on the context's stream: fd_pyramid_update, fd_particles_sample, _evaluate_wvm_svm, _weigh_wvm_svm,
 * fd_particles_state; the only read-back is fd_particles_state's. */
/* The WVM's part: sample -> maps -> window on the device as for _evaluate_pyramid (the patch is the WVM's filter size), then the exact
 * cascade of fd_wvm_svm_evaluate_samples on the list with per-window outputs.  Waits for nothing, copies nothing back.  Leaves
 * score[i] = (double) the WVM's output of particle i's window, the valid flags and the fd_particles_get_trace records as
 * _evaluate_pyramid does; the positives and their equalised patches stay in the WVM handle until its next run, so nothing else may run on
 * that handle before _weigh_wvm_svm.  Every particle keeps its own slot of the list; one without a window is scored on a window that
 * exists and is never selected.  The positive buffer and the second cascade stage's state are reserved for all particles before the
 * launch, whatever FD_WVM_POS_CAP says; the handle's header and its wishes for a device tail or speculative SVM scores are left as a
 * fd_detect_wvm call with per-window outputs leaves them (nothing is read back, so what such a call learns from the header -- the
 * windows its second stage saw, its positive count -- stays what the previous run left).
 * FD_ERR_INVALID_ARGUMENT, before anything is queued: objects of different contexts, a multi-frame or layer-filtered pyramid, more than
 * FD_SAMPLE_MAPS_MAX maps or a map other than FD_SAMPLE_MAP_RESIZE, an SVM that does not work on u8 vectors of the WVM's dimension, more
 * than 64 kept layers, a width -> layer table longer than FD_SAMPLE_TABLE_MAX.  FD_ERR_DEVICE_CAPACITY when FD_WVM_DEEP_CAP fixes the
 * second stage's state below the particle count.  FD_ERR_RUNTIME for a pyramid without an image.  A refused call launches nothing and
 * leaves the generation "not evaluated".  An empty generation is FD_OK. */
int fd_particles_evaluate_wvm_svm(fd_ctx* ctx, fd_particles* p, fd_pyramid* pyr, const fd_wvm* wvm, const fd_svm* svm, double aspect_ratio,
                                  const fd_sample_map* maps, int n_maps);
/* The rest of the model, behind _evaluate_wvm_svm with the same WVM: of the WVM positives whose particle is valid, the up to 8 with the
 * smallest (t, particle index), t = logistic_a + logistic_b * output (p_wvm = 1 / (1 + exp(t)) falls as t rises; equal t goes to the lower
 * index, a NaN behind every number), are scored by the SVM (a fixed launch of 8 rows).  Then per particle: invalid -> target 0, weight
 * 0, score 0; valid -> target 0, weight 0.5 * p_wvm; selected -> target = distance >= threshold, weight 2 * (0.5 * p_wvm) * p_svm.
 * best_score, n_valid and bad_weight as fd_particles_weigh_classifier leaves them.  Waits for nothing, copies nothing back.
 * FD_ERR_INVALID_ARGUMENT, before anything is queued, for objects of different contexts and for an SVM that does not work on u8 vectors of
 * the WVM's dimension (this call's SVM reads the patch rows; it need not be the handle _evaluate_wvm_svm checked).  FD_ERR_RUNTIME without a
 * preceding _evaluate_wvm_svm with this WVM on the current generation, and when anything else has run on the WVM handle since (its
 * positives are then another run's).  A refused weighing leaves the generation evaluated and unweighed. */
int fd_particles_weigh_wvm_svm(fd_ctx* ctx, fd_particles* p, const fd_wvm* wvm, const fd_svm* svm);
/* for tests, not for the frame path (it waits): the selection of the last _weigh_wvm_svm.  *count of 0..8, index[8] the selected
 * particles, most probable first, distance[8] their SVM outputs; entries from *count on are -1 and 0.  index and distance may be NULL.
 * FD_ERR_RUNTIME unless the current generation has been evaluated and weighed by the two calls above. */
int fd_particles_get_wvm_svm_trace(fd_ctx* ctx, fd_particles* p, int* count, int32_t* index, double* distance);

/* ---- supervised descent: superviseddescent::SdmLandmarkModel / SdmLandmarkModelFitting ---------- */
typedef struct {
    int32_t num_landmarks;      /* L */
    int32_t num_steps;          /* S (numCascadeSteps) */
    const float* mean;          /* 2L: x0..xL-1, y0..yL-1 (SdmLandmarkModel.cpp:53-56) */
    const float* const* R;      /* per step: (feature_dim+1) x 2L row-major regressor (last row = bias) */
    const int32_t* R_rows;      /* per step: feature_dim + 1 */
    int32_t hog_variant;        /* 0 DalalTriggs, 1 UoCTTI (VlHogDescriptorExtractor::VlHogType) */
    const int32_t* desc_params; /* NULL: optimize() as the reference compiles it -- `if (true) { // adaptive` (SdmLandmarkModel.hpp:209,
                                 * 243): every step uses the 30x30 / 3x3 cells / 9 bins descriptor whatever the model file says
                                 * (DescriptorExtractor.hpp:132-139), R_rows[s] = L*279 + 1 (UoCTTI) or L*324 + 1.  Non-NULL: the
                                 * non-adaptive `else` branches of :236-238 and :246-248 (present upstream, compiled out by the `if
                                 * (true)`): per step {numCells, cellSize, numBins} of VlHogDescriptorExtractor(type, numCells, cellSize,
                                 * numBins) (SdmLandmarkModel.cpp:188-204), getDescriptors(image, points) with windowSizeHalf = 0 and
                                 * modelShape + deltaShape.t() without the face-size factor.  This is the only way the regressors of the
                                 * reference's shipped model (detect-landmarks/share/models/SDM_Model_HOG_Zhenhua_11012014.txt: 144 / 144 /
                                 * 64 / 64 / 16 dimensions per landmark) can be applied at all.
                                 * The struct MUST be zero-initialised before its fields are set (`fd_sdm_model md = {0};`): this trailing
                                 * field was added in round 5, and a caller that fills the older fields one by one would otherwise hand
                                 * in a wild pointer.  Values are validated (1 <= numCells <= 8, 2 <= cellSize <= 64, 1 <= numBins <= 32). */
} fd_sdm_model;
int fd_sdm_create(fd_ctx* ctx, const fd_sdm_model* model, fd_sdm** out);
void fd_sdm_destroy(fd_sdm* m);
/* VlHogDescriptorExtractor::getDescriptors (DescriptorExtractor.hpp:106-219), adaptive parameters
 * (window_size_half > 0: 30x30 patch, 3x3 cells of 10, 9 bins) or fixed (num_cells, cell_size, num_bins).
 * gray: host image; out: n x len floats; *len receives the descriptor length. */
int fd_sdm_descriptors(fd_ctx* ctx, const uint8_t* gray, int width, int height, const float* px, const float* py,
                       int n, int window_size_half, int variant, int num_cells, int cell_size, int num_bins,
                       float* out, int* len);
/* SdmLandmarkModelFitting::alignRigid + optimize (SdmLandmarkModel.hpp:156-192,199-256) for a batch of
 * B gray images of identical size (contiguous, host or device) and one face box {x,y,w,h} each.
 * shapes_out: B x 2L floats.  status_out (may be NULL): per face 0 ok / 1 window left the image
 * (the reference would throw). */
int fd_sdm_fit_batch(fd_ctx* ctx, const fd_sdm* m, const uint8_t* gray_images, int width, int height, int batch,
                     const int32_t* face_boxes, int images_on_device, float* shapes_out, int32_t* status_out);
/* SdmLandmarkModelFitting::optimize only (SdmLandmarkModel.hpp:199-256): shapes_inout holds the B initial
 * shapes (2L floats each: x0..xL-1, y0..yL-1) and receives the optimised ones. */
int fd_sdm_optimize_batch(fd_ctx* ctx, const fd_sdm* m, const uint8_t* gray_images, int width, int height, int batch,
                          int images_on_device, float* shapes_inout, int32_t* status_out);
/* Asynchronous form of fd_sdm_fit_batch (the five-stage path has _begin/_end, so has this): _begin queues the whole fit of a batch
 * (its S cascade steps and the read-back) and returns; _end waits and delivers shapes / status.  Several batches of one model can be
 * in flight from ONE host thread; each has its own scratch set.  Host images / boxes of a batch must stay valid until its _end, and the
 * model must outlive its tickets (a ticket holds a plain pointer to it).  Device-resident images are read behind everything queued on
 * the context's stream at the time of _begin. */
typedef struct fd_sdm_ticket fd_sdm_ticket;
int fd_sdm_fit_batch_begin(fd_ctx* ctx, const fd_sdm* model, const uint8_t* gray_images, int width, int height, int batch,
                           const int32_t* face_boxes, int images_on_device, fd_sdm_ticket** ticket);
int fd_sdm_fit_batch_end(fd_ctx* ctx, fd_sdm_ticket* ticket, float* shapes_out, int32_t* status_out);

/* ---- supervised descent training: LandmarkBasedSupervisedDescentTraining::train's cascade loop (.cpp:297-365) and linearRegression
 * (.cpp:439-518) on the device (csrc/sdm_train.hpp).  Per cascade step: the feature matrix A (row r: the L VlHog
 * descriptors of row r's shape on row r's image, landmark-major, then a 1; the non-adaptive geometry of fd_sdm_model.desc_params, the
 * descriptor floats are fd_sdm_descriptors'), AtA and Atb = A^T (groundtruth - shapes) accumulated in double in a fixed order (two
 * calls give the same bits, AtA is exactly symmetric), lambda, Mreg = AtA + lambda I, R = Mreg^-1 Atb by Cholesky factorisation and
 * two triangular solves in double, rounded to float once, and shapes += A R through the kernels fd_sdm_optimize_batch runs: the shapes
 * after step s are bit for bit what fd_sdm_optimize_batch gives on the model of the first s regressors from the same start shapes.
 * Reference quirks and what became of them:
 *  - train() calls linearRegression(A, b, RegularizationType::Automatic) with the defaults of the HEADER (.hpp:187: lambda = 0.5f,
 *    regularizeAffineComponent = true; the .cpp's comment says false) and never reads the member setRegularisation sets.  This ABI
 *    takes the three values as parameters; the host class decides which to pass.
 *  - the reference's solve is a float A.t()*A and Eigen's float full-pivoting LU INVERSE; here double and Cholesky, so the contract
 *    is a tolerance against a float64 model, not bits.  A pivot <= 0 or NaN is FD_ERR_RUNTIME ("the regularised AtA is not positive
 *    definite (pivot k); increase lambda"), the reference's "not invertible ... increase lambda".
 *  - EigenvalueThreshold needs Eigen's FullPivLU::maxPivot() * threshold() and is not built: FD_ERR_INVALID_ARGUMENT naming it.
 *  - the reference draws landmarks and boxes into the training images before it takes features from them (.cpp:263-264,273: debug
 *    output).  Not reproduced: features come from the images as given.
 *  - the reference trains with the extractors' fixed windows, but its compiled optimize() fits with face-size adaptive ones: a trained
 *    model is for fd_sdm_model.desc_params (SdmLandmarkModelFitting(model, adaptive = false), sdm_fit_app --non-adaptive).
 *  - getPerturbedShape seeds a fresh mt19937 from random_device per sample and passes rndN_t_x(engine), rndN_t_y(engine) as two arguments
 *    of one call (unspecified evaluation order).  The start shapes are an INPUT of this ABI; the host class
 *    (superviseddescent/LandmarkBasedSupervisedDescentTraining.hpp) draws them from one seeded std::mt19937 in the order scale, tx, ty. */
enum { FD_SDM_REG_MANUAL = 0, FD_SDM_REG_AUTOMATIC = 1, FD_SDM_REG_EIGENVALUE_THRESHOLD = 2 };
typedef struct {                /* zero-initialise before setting fields */
    int32_t num_landmarks;      /* L */
    int32_t num_steps;          /* S */
    int32_t hog_variant;        /* 0 DalalTriggs, 1 UoCTTI */
    const int32_t* desc_params; /* 3 per step {numCells, cellSize, numBins}, validated as fd_sdm_model.desc_params */
    int32_t regularisation;     /* FD_SDM_REG_MANUAL: lambda as given; FD_SDM_REG_AUTOMATIC: lambda * ||AtA||_F / rows */
    double lambda;
    int32_t regularise_affine;  /* 0: the last diagonal element (the bias) gets no lambda */
} fd_sdm_train_params;
typedef struct {
    const uint8_t* images;      /* count contiguous gray images of width x height, host or device */
    int32_t width, height, count, on_device;
} fd_sdm_train_group;           /* images are numbered through the groups in order */
typedef struct {
    double lambda;              /* the lambda added to the diagonal (entry 0: 0) */
    double err_l1;              /* ||groundtruth - shapes||_1 / (rows * 2L), the number the reference logs (.cpp:293,363) */
    double err_fro;             /* ||groundtruth - shapes||_F */
    int32_t rows, dim;          /* M and D = L * len + 1 of the step (entry 0: dim 0) */
    int32_t pivot_flag;         /* 0, or 1 + the index of the pivot that was not positive */
} fd_sdm_train_step_info;
/* rows = images * samples_per_image (the reference's K + 1 per image); both shape arrays are image-major as the reference lays
 * them out (row = image * samples_per_image + sample, 2L floats x0..xL-1, y0..yL-1).  R_out[s]: (L * len_s + 1) x 2L floats in
 * fd_sdm_model.R's layout, bias row last.  shapes_steps_out (may be NULL): (S + 1) x rows x 2L floats, entry 0 the start shapes.
 * row_status_out (may be NULL): per row 0 ok / 1 a patch window left the image in some step; such a row makes the call fail with
 * FD_ERR_RUNTIME, and R_out is not written.  info_out (may be NULL): S + 1 entries, entry 0 carries the start errors. */
int fd_sdm_train(fd_ctx* ctx, const fd_sdm_train_params* params, const fd_sdm_train_group* groups, int num_groups, int samples_per_image,
                 const float* initial_shapes, const float* groundtruth, float* const* R_out, float* shapes_steps_out,
                 int32_t* row_status_out, fd_sdm_train_step_info* info_out);
/* The reference's free function linearRegression on host matrices: A is M x D (its last column is whatever the caller put there; it
 * is the one regularise_affine == 0 leaves alone), b is M x N, x_out D x N.  lambda_out, ata_out (D x D), atb_out (D x N) may be NULL. */
int fd_sdm_linear_regression(fd_ctx* ctx, const float* A, const float* b, int M, int D, int N, int type, double lambda,
                             int regularise_affine, float* x_out, double* lambda_out, double* ata_out, double* atb_out);
/* host only: device bytes the trainer keeps resident for `rows` rows (A, AtA with the right-hand sides, the update's partial sums, R,
 * shapes, patch origins, row status) and the largest D of the steps.  NOT counted: the images of host groups, which the call uploads
 * (width x height x count bytes per group), and a few hundred bytes of scalars.  An allocation that fails in fd_sdm_train is
 * FD_ERR_RUNTIME naming its byte count.  Either output may be NULL. */
int fd_sdm_train_limits(const fd_sdm_train_params* params, int rows, int64_t* bytes, int* max_dim);
/* host only: dims[s] = L * len_s + 1, the rows of R_out[s], for every step */
int fd_sdm_train_step_dims(const fd_sdm_train_params* params, int32_t* dims);

/* ---- image-shard data parallelism (north_star: "images shard embarrassingly across the 8 GPUs of one node with a single RCCL gather
 * of detections over xGMI").  One process per GPU; image i belongs to rank i mod world; models are replicated; no data-path
 * collective.  The reference has no counterpart (it is single-threaded, ffpDetectApp.cpp:548-659 loops over the images of a
 * source); a maintainer binds these around that loop (ffp_detect_app --gpus N).
 *   fd_dist_unique_id   rank 0 creates the communicator id (ncclGetUniqueId, 128 bytes) and hands it to the other ranks by any means
 *   fd_dist_init        joins the communicator on the context's device (ncclCommInitRank); world 1 needs no id and no librccl: the
 *                       rank gathers from itself, whatever id holds.  (FD_DIST_FORCE_COMM=1 in the environment + an id: a real one-rank
 *                       communicator, the gather goes through ncclAllGather -- what the one-GPU tests use to run librccl itself.)
 *   fd_pack_records     fd_detection -> fixed-stride records {image, detector, cx, cy, w, h, score, probability} (all exact in fp64)
 *   fd_dist_gather_records  a 64-byte header exchange (every rank's count) and ONE ncclAllGather of max-count + 1 rows per rank, on the
 *                       handle's own stream (nothing queued on the context's stream is waited for or held up); every rank receives the
 *                       records of all ranks ordered by (image, detector, original order).  cap_per_rank: the most records a rank
 *                       may contribute; *truncated != 0: a rank had more (the surplus was dropped).
 *                       COLLECTIVE: every rank of the communicator makes the call, with the same cap_per_rank (a rank that packed with
 *                       another stride is reported as FD_ERR_INVALID_ARGUMENT on all ranks).  The collective runs once per set of
 *                       records: with all == NULL the call returns the count, with all_cap too small FD_ERR_CAPACITY -- either way the
 *                       gathered records stay in the handle, and the next call with a large enough buffer delivers them WITHOUT another
 *                       collective (so a retry on some ranks only cannot deadlock).  local / n_local of such a follow-up call are ignored.
 *                       FD_RCCL_LIB names another library with the five nccl entry points (tests: tests/stub_rccl).
 *   fd_dist_gather_begin / _end  the same gather in two halves: _begin exchanges the headers (a wait of tens of microseconds on the
 *                       gather stream) and queues the payload collective, _end waits for it and delivers -- the records of one
 *                       interval travel while the caller processes the next interval's images.  One gather in flight per handle; local
 *                       may be reused as soon as _begin returns.  _end has fd_dist_gather_records' count-only / capacity-retry rules.
 *   fd_dist_gather_discard  drops a gathered set the caller does not want to fetch (after a count-only call or FD_ERR_CAPACITY), so that
 *                       the next fd_dist_gather_records is a new collective.  Every rank must drop or take a set: a rank that still
 *                       holds one would answer the next call from its handle while the others enter ncclAllGather.
 *   fd_dist_gather_pending  1 while the handle holds a gathered set that has not been delivered or dropped. */
#define FD_DIST_ID_BYTES 128
typedef struct fd_dist fd_dist;
typedef struct fd_record {
    double image, detector, cx, cy, w, h, score, probability;
} fd_record;
int fd_dist_owner(int64_t image_index, int world);
int fd_dist_unique_id(uint8_t* id /* FD_DIST_ID_BYTES */);
int fd_dist_init(fd_ctx* ctx, int rank, int world, const uint8_t* id, fd_dist** out);
void fd_dist_destroy(fd_dist* d);
int fd_dist_rank(const fd_dist* d);
int fd_dist_world(const fd_dist* d);
int fd_pack_records(int64_t image_id, int32_t detector_id, const fd_detection* dets, int n, fd_record* out);
int fd_dist_gather_records(fd_dist* d, const fd_record* local, int n_local, int cap_per_rank, fd_record* all, int64_t all_cap,
                           int64_t* n_all, int* truncated);
int fd_dist_gather_begin(fd_dist* d, const fd_record* local, int n_local, int cap_per_rank);
int fd_dist_gather_end(fd_dist* d, fd_record* all, int64_t all_cap, int64_t* n_all, int* truncated);
void fd_dist_gather_discard(fd_dist* d);
int fd_dist_gather_pending(const fd_dist* d);

#ifdef __cplusplus
}
#endif
#endif /* FD_HIP_H_ */
