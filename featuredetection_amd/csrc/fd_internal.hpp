// featuredetection_amd/csrc/fd_internal.hpp -- internal declarations of libfd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <typeindex>
#include <typeinfo>
#include <vector>
#include <stdexcept>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <deque>
#include <exception>
#include "../../include/fd_hip.h"
#include "../../include/fd_hip_bench.h"

struct FdPinned {   // pinned host scratch (allocated lazily): pageable async copies cost ~1 ms each on this stack
    void* p = nullptr;
    size_t cap = 0;
};

// A few persistent host threads for the per-detector host stages of the batch entry points (ordering the positives, overlap
// elimination, the SVM launch, NMS): run(f) executes f on every worker and on the caller and returns when all are done.
struct FdWorkerPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv, cvDone;
    std::function<void()> job;
    uint64_t gen = 0;
    int pending = 0;
    bool stop = false;
    explicit FdWorkerPool(int n) {
        for (int i = 0; i < n; ++i) th.emplace_back([this] { loop(); });
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::function<void()> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                j = job;
            }
            try { j(); } catch (...) {}   // jobs report their errors themselves; an escaping exception would terminate the process
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--pending == 0) cvDone.notify_one();
            }
        }
    }
    void run(const std::function<void()>& f) {
        {
            std::lock_guard<std::mutex> lk(mu);
            job = f;
            pending = (int)th.size();
            ++gen;
        }
        cv.notify_all();
        // the workers reference the caller's stack through f: wait for them even when the caller's own share throws
        std::exception_ptr err;
        try { f(); } catch (...) { err = std::current_exception(); }
        {
            std::unique_lock<std::mutex> lk(mu);
            cvDone.wait(lk, [&] { return pending == 0; });
        }
        if (err) std::rethrow_exception(err);
    }
    ~FdWorkerPool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
};

// Process-wide queue of host continuations (a few persistent threads, FD_ASYNC_THREADS, default 2): the ticket entry points
// (fd_detect_five_stage_frames_begin) hand the host stages that follow their kernels -- wait, order the positives, overlap
// elimination, SVM launch, wait, NMS -- to it, so the calling thread is free to queue the next call's kernels and the GPU never waits
// for a host stage of one call while another call has work ready.  submit() returns a handle; wait() rethrows the task's exception.
struct FdAsyncTask {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::exception_ptr error;
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
        if (error) std::rethrow_exception(error);
    }
};
struct FdAsyncQueue {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<std::function<void()>, std::shared_ptr<FdAsyncTask>>> q;
    bool stop = false;
    explicit FdAsyncQueue(int n) {
        for (int i = 0; i < n; ++i) th.emplace_back([this] { loop(); });
    }
    void loop() {
        for (;;) {
            std::pair<std::function<void()>, std::shared_ptr<FdAsyncTask>> item;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !q.empty(); });
                if (q.empty()) return;   // stop requested and nothing left
                item = std::move(q.front());
                q.pop_front();
            }
            std::exception_ptr err;
            try { item.first(); } catch (...) { err = std::current_exception(); }
            {
                std::lock_guard<std::mutex> lk(item.second->mu);
                item.second->error = err;
                item.second->done = true;
            }
            item.second->cv.notify_all();
        }
    }
    std::shared_ptr<FdAsyncTask> submit(std::function<void()> f) {
        auto t = std::make_shared<FdAsyncTask>();
        {
            std::lock_guard<std::mutex> lk(mu);
            q.emplace_back(std::move(f), t);
        }
        cv.notify_one();
        return t;
    }
    ~FdAsyncQueue() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
};
FdAsyncQueue& fd_async_queue();   // ctx.hip
FdAsyncQueue& fd_batch_queue();   // ctx.hip: the per-detector host stages of batches in flight (FD_BATCH_THREADS threads)

struct fd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string error;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // bracket the dominant kernel of a detect call when kernel_timing is on (fd_hip_bench.h)
    bool kernel_timing = false;
    int kernel_timing_mode = 1;      // WVM cascades: 1 = all cascade kernels of the call, 2 = the dense pre-filter only, 3 = stage B's chain kernels (fd_hip_bench.h)
    hipEvent_t evx[8] = {};          // mode 3: one event pair per stage-B phase around its k_wvb_chain2 launch (created on first use)
    int evxN = 0;                    // pairs recorded by the last timed launch
    hipEvent_t evg[2] = {};          // mode 2: around the last k_wvm_prefilter_group launch (fd_last_group_prefilter_ms)
    int evgMembers = 0;              // its member count (0: none recorded)
    const char* last_kernel = "";
    float last_kernel_ms = 0.f;
    int num_cus = 256;
    FdPinned pinned;
    hipStream_t aux = nullptr;   // second stream (created on first use): small follow-up work that must not queue behind ctx->stream
    hipStream_t pool[8] = {};   // batch jobs are spread over these (created on first use)
    hipStream_t tail = nullptr; // high-priority stream of the batch entry points' follow-up kernels (created on first use)
    std::unique_ptr<FdWorkerPool> workers;   // created on first use by the batch entry points (FD_BATCH_THREADS)
    // per-context device scratch of the translation units (fd_scratch<T>): owned by the context, freed with it
    std::map<std::type_index, std::shared_ptr<void>> scratch;
};

// the context's scratch object of type T (one per context and type, created on first use); contexts are not shared between
// host threads, so no locking
template <class T>
static inline T& fd_scratch(fd_ctx* ctx) {
    std::shared_ptr<void>& slot = ctx->scratch[std::type_index(typeid(T))];
    if (!slot) slot = std::shared_ptr<void>(new T(), [](void* p) { delete static_cast<T*>(p); });
    return *static_cast<T*>(slot.get());
}

struct FdError {
    int code;
    std::string msg;
};

#define FD_THROW(code, ...)                               \
    do {                                                  \
        char _b[512];                                     \
        snprintf(_b, sizeof(_b), __VA_ARGS__);            \
        throw FdError{code, std::string(_b)};             \
    } while (0)

#define HIP_CHECK(expr)                                                                       \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) FD_THROW(FD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// Inside a catch (...): the exception in flight as an FdError (the one place that knows what a foreign exception becomes).
static inline FdError fd_current_error() {
    try {
        throw;
    } catch (const FdError& e) {
        return e;
    } catch (const std::exception& e) {
        return FdError{FD_ERR_RUNTIME, e.what()};
    } catch (...) {
        return FdError{FD_ERR_RUNTIME, "unknown error"};
    }
}

// Runs body, converts exceptions into status codes + ctx->error (no exceptions cross the C ABI).
template <class F>
static inline int fd_guard(fd_ctx* ctx, F&& body) {
    try {
        body();
        return FD_OK;
    } catch (...) {
        const FdError e = fd_current_error();
        if (ctx) ctx->error = e.msg;
        return e.code;
    }
}

// Simple owning device buffer that only grows (reused across calls: no hipMalloc in steady state).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    void reserve(size_t bytes) {
        if (bytes <= cap) return;
        if (p) HIP_CHECK(hipFree(p));
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        HIP_CHECK(hipMalloc(&p, want));
        cap = want;
    }
    template <class T> T* as() const { return (T*)p; }
};

// Pinned host staging buffer
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
    void reserve(size_t bytes) {
        if (bytes <= cap) return;
        if (p) HIP_CHECK(hipHostFree(p));
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
    }
    template <class T> T* as() const { return (T*)p; }
};

// pinned scratch of the context, at least `bytes` large
static inline void* fd_pinned(fd_ctx* ctx, size_t bytes) {
    if (bytes > ctx->pinned.cap) {
        if (ctx->pinned.p) HIP_CHECK(hipHostFree(ctx->pinned.p));
        ctx->pinned.p = nullptr;
        ctx->pinned.cap = 0;
        size_t want = bytes + bytes / 2 + 4096;
        HIP_CHECK(hipHostMalloc(&ctx->pinned.p, want, hipHostMallocDefault));
        ctx->pinned.cap = want;
    }
    return ctx->pinned.p;
}

static inline hipStream_t fd_aux_stream(fd_ctx* ctx) {
    if (!ctx->aux) HIP_CHECK(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
    return ctx->aux;
}

// Stream of the small follow-up kernels of the batch entry points (the SVM stage and read-backs of a detector whose cascade has
// finished): highest priority and never behind the cascades still queued on the pool streams, so that the host can finish the
// detectors one by one while the GPU works through the remaining cascades.
static inline hipStream_t fd_tail_stream(fd_ctx* ctx) {
    if (!ctx->tail) {
        int least = 0, greatest = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&ctx->tail, hipStreamNonBlocking, greatest));
    }
    return ctx->tail;
}

// ---- FD_* environment knobs that more than one place reads: one reader each, holding the default and the clamp.
// Read once per process unless noted.
static inline int fd_env_int(const char* name, int dflt, int lo, int hi) {
    const char* e = getenv(name);
    const int v = e ? atoi(e) : dflt;
    return v < lo ? lo : (v > hi ? hi : v);
}
// host threads of a large batch: the pool that queues its kernels / runs its host stages, and the threads of fd_batch_queue()
static inline int fd_knob_batch_threads() { static const int v = fd_env_int("FD_BATCH_THREADS", 8, 1, 16); return v; }
// rounds of resident workgroups the pre-filter's tiles are dealt over
static inline int fd_knob_wvd_rounds() { static const int v = fd_env_int("FD_WVD_ROUNDS", 2, 1, 64); return v; }
static inline bool fd_knob_trace() { static const bool on = getenv("FD_TRACE") != nullptr; return on; }
// stages 2-3 on the device: 0 never, 1 always (batch jobs too), -1 (unset): multi-frame calls only.  Read per call: the tests flip it.
static inline int fd_knob_fs_tail() { const char* e = getenv("FD_FS_TAIL"); return e ? atoi(e) : -1; }
// single-frame five-stage calls: the second stage over all first-stage positives behind the cascade (one host wait); 0: two waits.
// Read per call: the tests compare both orders.
static inline bool fd_knob_fs_spec() { const char* e = getenv("FD_FS_SPEC"); return !(e && atoi(e) == 0); }
// the trackers of the host layer keep their particle set on the device: 1 on, anything else (and unset) off.  Read per call.
static inline bool fd_knob_cond_device() { const char* e = getenv("FD_COND_DEVICE"); return e && atoi(e) == 1; }
// k_wvm_prefilter's plan: tasks packed 64 to a wavefront across the layers of a frame, balanced row groups; 0: the per-layer plan.
// Read per call: the tests compare both plans in one process.
static inline bool fd_knob_wvd_pack() { const char* e = getenv("FD_WVD_PACK"); return !(e && atoi(e) == 0); }
// k_pyrdown_tiled of a multi-frame pyramid (frames a multiple of 8): frame f's tiles on XCD f % 8; 0: the (tiles, 1, frames) grid.
// Read where the launch is queued.
static inline bool fd_knob_pyr_xcd() { const char* e = getenv("FD_PYR_XCD"); return !(e && atoi(e) == 0); }

// fd_patch_rvm_evaluate_samples: 1 the fused kernel (k_rvm_samples) at every sample count, 0 the composed route (window patches, then the
// cascade's passes) at every count, -1 (unset): the size rule of patch_samples.hpp.  WHI takes the composed route whatever this says.
// Read per call: the tests compare both routes in one process.
static inline int fd_knob_patch_fused() { const char* e = getenv("FD_PATCH_FUSED"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }

// FD_TRACE's stopwatch: lap_ns() is the time since the start (or the previous lap) and starts the next lap; off: no clock is read.
struct FdStopwatch {
    bool on = fd_knob_trace();
    std::chrono::steady_clock::time_point t;
    FdStopwatch() { restart(); }
    void restart() { if (on) t = std::chrono::steady_clock::now(); }
    int64_t lap_ns() {
        if (!on) return 0;
        const std::chrono::steady_clock::time_point n = std::chrono::steady_clock::now();
        const int64_t ns = std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count();
        t = n;
        return ns;
    }
};

static inline hipStream_t fd_pool_stream(fd_ctx* ctx, int i) {
    static const int nstreams = fd_env_int("FD_BATCH_STREAMS", 8, 1, 8);
    hipStream_t& s = ctx->pool[i % nstreams];
    if (!s) HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device): `done` is the caller's static per-kernel bit mask
static inline void fd_allow_lds(fd_ctx* ctx, const void* kernel, int bytes, uint64_t& done) {
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (done & bit) return;
    HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done |= bit;
}
// Workgroups of KERNEL (`threads` threads, no dynamic LDS) a CU holds, `fallback` when the runtime cannot tell.  Asked once per kernel
// instance; the batch's worker threads call it concurrently (they may both ask the first time, and store the same answer).
template <auto KERNEL>
static inline int fd_blocks_per_cu(int threads, int fallback) {
    static std::atomic<int> cached{0};
    int n = cached.load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, KERNEL, threads, 0) != hipSuccess || n < 1) n = fallback;
        cached.store(n, std::memory_order_relaxed);
    }
    return n;
}

struct FdStreamSwap {   // temporarily redirects everything that launches on ctx->stream
    fd_ctx* c;
    hipStream_t keep;
    FdStreamSwap(fd_ctx* c_, hipStream_t s_) : c(c_), keep(c_->stream) { c->stream = s_; }
    ~FdStreamSwap() { c->stream = keep; }
};

static inline int fd_cvRound(double v) { return (int)std::lrint(v); }  // cvRound: half-to-even
// cvRound on the host and on the device (the sample maps and the window placement below): to the nearest even on a tie on both sides.
// A value outside the int range saturates and a NaN gives 0 on both sides (what the device's conversion does by itself).
__host__ __device__ inline int fd_sample_cvround(double v) {
    if (!(v == v)) return 0;
    if (v >= 2147483647.0) return INT32_MAX;
    if (v <= -2147483648.0) return INT32_MIN;
#ifdef __HIP_DEVICE_COMPILE__
    return __double2int_rn(v);
#else
    return fd_cvRound(v);
#endif
}

// ---------------- pyramid ----------------
struct LayerDesc {          // device-visible layer descriptor
    int32_t w, h;           // layer size (pixels)
    int32_t ch;             // channels of the filtered layer
    int32_t pad;
    uint32_t gray_off;      // byte offset of the gray layer in the arena
    uint32_t filt_off;      // byte offset of the filtered layer (== gray_off when no layer filter)
};

struct HostLayer {
    int index;
    double scale;
    int w, h, ch;
    uint32_t gray_off, filt_off;
    bool kept;
    int chain, depth;       // first-octave slot i and pyrDown depth j
    uint32_t blur_off = 0;  // kept layers of a gradient pyramid with blurring: the blurred gray layer (GradientFilter.cpp:43-46)
};

struct WindowLayer {        // per kept layer, for the window enumeration of one (patch, step, roi)
    int32_t layer;          // position in the kept-layer list
    int32_t bx, by;         // first window origin
    int32_t nx, ny;         // number of window positions
    int32_t ow, oh;         // original (image) patch size
    int64_t first;          // index of the first window of this layer
};

struct fd_pyramid {
    fd_ctx* ctx;
    size_t octl;
    double inc, minS, maxS;
    int filter_kind = FD_LAYER_NONE, bins = 9, signed_gradients = 0, interpolate = 0, grad_kernel = 1, lbp_type = 0;
    int grad_blur = 0;               // GradientFilter's blurKernelSize (0: none); blurred copies of the kept layers live at blur_off
    int image_filter = FD_IMAGE_GRAY;   // fd_pyramid_set_image_filter: the chain applied to the image before the layers are built
    DevBuf gw_stats;                 // FD_IMAGE_GREYWORLD_GRAY: channel sums and maxima per frame (pyramid.hip), cleared by every update
    int img_w = 0, img_h = 0;
    std::vector<HostLayer> all;      // every computed layer (kept or only a pyrDown source)
    std::vector<int> kept;           // indices into all, sorted by layer index
    DevBuf arena;                    // gray full-res + all layers + filtered layers
    DevBuf input;                    // staging for host images
    DevBuf lut;                      // gradient binning LUT (65536 * 2|4 bytes)
    DevBuf rtab;                     // cv::resize coordinate / weight tables of the first-octave layers (k_resize_down, pyramid.hip)
    struct Plan;                     // the launches of an update, built with the layout (pyramid.hip)
    std::unique_ptr<Plan> plan;
    DevBuf layer_table;              // LayerDesc per kept layer
    std::vector<LayerDesc> h_layer_table;
    uint32_t gray_full_off = 0;
    size_t arena_bytes = 0;
    uint64_t version = 0;            // bumped by every update
    // several frames of identical size in one pyramid (fd_pyramid_set_frames): frame f's layers live at arena + f * image_stride
    // with the layout of frame 0.  One launch per pyramid stage and ONE cascade / SVM launch serve all frames of a call
    // (fd_detect_five_stage_frames); the per-frame launch chain is what bounds small frames.
    int nimg = 1;
    size_t image_stride = 0;
    // fd_pyramid_select: layer sub-range (pyramid layer indices, -1 = open end), layer step (over the kept layers, starting at the
    // first) and default region of interest of every window enumeration that follows (DirectPyramidFeatureExtractor.cpp:75-123)
    int sel_first = -1, sel_last = -1, sel_step = 1;
    // fd_pyramid_select_view: index range of the layers a pyramid built on this one exposes (ImagePyramid(pyramid, min, max)): the
    // layers outside do not exist for the window enumeration, and the layer step counts from the first layer inside
    int view_first = -1, view_last = -1;
    bool sel_has_roi = false;
    int sel_roi[4] = {0, 0, 0, 0};
    // recorded on the updating stream after the last kernel of an update: consumers on OTHER streams (the stream pool of the
    // batch entry points) wait for it; consumers on the same stream are ordered anyway
    hipEvent_t ready = nullptr;
    hipStream_t readyStream = nullptr;
    // fd_particles_evaluate_pyramid: the uploaded width -> layer table (fd_sample_layer_table) of the patch width and kept-layer layout
    // it was built for; rebuilt only when one of them changes
    struct SampleTable {
        DevBuf dev;
        std::vector<int16_t> host;   // what the upload reads
        int length = -1, patch_w = 0, n_layers = 0, first_index = 0;
        double inc = 0.0;
    } sample_table;
    ~fd_pyramid();                   // pyramid.hip, where Plan is complete (handles are created and destroyed only there)
};

// entry points that only know single-frame pyramids
static inline void fd_pyramid_require_single(const fd_pyramid* p, const char* who) {
    if (p->nimg > 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the pyramid holds %d frames (fd_pyramid_set_frames); use fd_detect_five_stage_frames", who, p->nimg);
}

static inline void fd_pyramid_require_image(const fd_pyramid* p) {
    if (p->all.empty()) FD_THROW(FD_ERR_RUNTIME, "pyramid has not been updated with an image");
}

// makes `consumer` wait for the pyramid's last update when that ran on another stream
static inline void fd_pyramid_wait(const fd_pyramid* p, hipStream_t consumer) {
    if (p->ready && consumer != p->readyStream) HIP_CHECK(hipStreamWaitEvent(consumer, p->ready, 0));
}

// The sample -> window rule of DirectPyramidFeatureExtractor::extract(x, y, width, height) (DirectPyramidFeatureExtractor.cpp:67-73,
// 134-153; ImagePyramid::getLayer(double), ImagePyramid.hpp:307-310), stated once: the layer with pyramid index
// lround(log(patch_w / width) / log(inc)) must be a kept one (the kept layers have consecutive indices from first_index on);
// layer(pos, scale, w, h) reports the kept layer at list position pos.  Returns false for a sample without a window.
// The rule has two parts.  (a) fd_sample_layer_position, width -> layer, goes through libm's log and is the host's alone: the device reads
// it from a table of the host's values (fd_sample_layer_table).  (b) fd_sample_place, the window in that layer, is exact arithmetic (one
// double product, one rounding to the nearest even) and gives the same bits on both sides.
struct FdSampleWindow { int32_t layer, bx, by; };
// (a) the list position of the layer a sample of this width (> 0) is taken from, before the range check: below 0 or from the layer count
// on there is none.  An index that is not finite or not representable is reported on the side its sign names.
static inline long fd_sample_layer_position(int first_index, double inc, int pw, int width) {
    const double power = std::log((double)pw / (double)width) / std::log(inc);
    if (!(std::fabs(power) < 1e9)) return power > 0 ? LONG_MAX : LONG_MIN;   // not a finite, representable index
    const long index = std::lround(power);   // std::round, then the int cast of the reference
    return index - first_index;
}
// (b) the pw x ph window of the sample in a layer of lw x lh pixels; false: it does not lie inside
__host__ __device__ inline bool fd_sample_place(double scale, int lw, int lh, int pw, int ph, int x, int y, int width, int height, int32_t& bx, int32_t& by) {
    const double fx = (double)((int64_t)x - width / 2) * scale, fy = (double)((int64_t)y - height / 2) * scale;
    if (!(fx >= -1.0 && fx <= (double)lw && fy >= -1.0 && fy <= (double)lh)) return false;   // far outside (and nothing the int cast could wrap)
    bx = fd_sample_cvround(fx); by = fd_sample_cvround(fy);   // inside [-1, lw]: fd_cvRound on the host
    return !(bx < 0 || by < 0 || (int64_t)bx + pw > lw || (int64_t)by + ph > lh);
}
template <class LayerAt>
static inline bool fd_sample_window(int n_layers, int first_index, double inc, int pw, int ph, int x, int y, int width, int height, LayerAt&& layer,
                                    FdSampleWindow& out) {
    if (width <= 0 || n_layers <= 0) return false;
    const long realIndex = fd_sample_layer_position(first_index, inc, pw, width);
    if (realIndex < 0 || realIndex >= (long)n_layers) return false;
    double scale;
    int lw, lh;
    layer((int)realIndex, scale, lw, lh);
    int32_t bx, by;
    if (!fd_sample_place(scale, lw, lh, pw, ph, x, y, width, height, bx, by)) return false;
    out.layer = (int32_t)realIndex; out.bx = bx; out.by = by;
    return true;
}

// sample s = {x, y, width, height} -> window by that rule on the kept layers of p; false: no window
static inline bool pyramid_sample_window(const fd_pyramid* p, int pw, int ph, const int32_t* s, FdSampleWindow& w) {
    if (p->kept.empty()) return false;
    return fd_sample_window((int)p->kept.size(), p->all[p->kept[0]].index, p->inc, pw, ph, s[0], s[1], s[2], s[3],
                            [&](int pos, double& scale, int& lw, int& lh) {
                                const HostLayer& L = p->all[p->kept[pos]];
                                scale = L.scale; lw = L.w; lh = L.h;
                            }, w);
}

// Resolves n samples, uploads the windows {layer, bx, by} of those that have one into dlist (pinned staging + one async copy on
// ctx->stream) and fills sampleOf (list position -> sample); valid (may be NULL): one byte per sample.  `extraPinnedPerValid` bytes per
// listed window behind the list in the same pinned block are the caller's, at the returned address.  NULL: no sample has a window,
// nothing was queued.
static inline void* fd_samples_upload(fd_ctx* ctx, const fd_pyramid* p, int pw, int ph, int n, const int32_t* xywh, uint8_t* valid, DevBuf& dlist,
                                      std::vector<int>& sampleOf, size_t extraPinnedPerValid) {
    std::vector<int32_t> list;
    list.reserve(3 * (size_t)n);
    sampleOf.clear();
    for (int i = 0; i < n; ++i) {
        FdSampleWindow w;
        const bool ok = pyramid_sample_window(p, pw, ph, xywh + 4 * (size_t)i, w);
        if (valid) valid[i] = ok ? 1 : 0;
        if (!ok) continue;
        list.push_back(w.layer); list.push_back(w.bx); list.push_back(w.by);
        sampleOf.push_back(i);
    }
    if (sampleOf.empty()) return nullptr;
    HIP_CHECK(hipSetDevice(ctx->device));
    const size_t listBytes = (sizeof(int32_t) * list.size() + 15) & ~(size_t)15;
    char* pin = (char*)fd_pinned(ctx, listBytes + extraPinnedPerValid * sampleOf.size());
    std::copy(list.begin(), list.end(), (int32_t*)pin);
    dlist.reserve(listBytes);
    HIP_CHECK(hipMemcpyAsync(dlist.p, pin, sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, ctx->stream));
    return pin + listBytes;
}

void fd_pyramid_update_on(fd_pyramid* p, const uint8_t* image, int w, int h, int ch, int is_device, hipStream_t st);
constexpr int FD_MAX_FRAMES = 64;
void fd_enumerate_layers(const fd_pyramid* p, int pw, int ph, int sx, int sy, const int* roi,
                         std::vector<WindowLayer>& out, int64_t& total);

// window id -> detection record geometry (wvm.hip)
void fd_window_to_detection(const fd_pyramid* p, const std::vector<WindowLayer>& wls, int sx, int sy, int64_t wid, fd_detection& d);

// ---------------- SVM scoring: what the detectors use of a model (svm.hip) ----------------
// what the fused HOG + SVM kernel (hog_svm_fused.hpp, launched from hog.hip) needs of an f32 RBF model (svm.hip): its kernel argument
struct FdSvmFusedView {
    const float* svFrag;   // fragment-major support vectors [nsvt][KP * 32]
    const float* ss;       // |s|^2 per support vector (padded ones 0)
    const float* coeff;    // coefficients (padded ones 0)
    int32_t nsvt, KP;      // tiles of 32 support vectors, padded vector length
    float bias, negGamma;
};
bool fd_svm_fused_view(const fd_svm* m, FdSvmFusedView* v);
bool fd_svm_has_mfma_path(const fd_svm* m);
int fd_svm_KP(const fd_svm* m);
float fd_svm_threshold(const fd_svm* m);
int fd_svm_dim(const fd_svm* m);
bool fd_svm_is_u8(const fd_svm* m);
double fd_svm_probability(const fd_svm* m, double d);
void fd_svm_rbf_mfma_launch(fd_ctx* ctx, const fd_svm* m, const float* xFrag, const float* xx, int64_t npatches, double* out);
// generic scoring of n device-resident feature vectors (optionally gathered by slot index); _on: explicit stream, touches no context state
void fd_svm_generic_launch(fd_ctx* ctx, const fd_svm* m, const void* dfeat, const uint32_t* didx, int64_t stride_bytes, int64_t n, double* dout);
void fd_svm_generic_launch_on(hipStream_t st, const fd_svm* m, const void* dfeat, const uint32_t* didx, int64_t stride_bytes, int64_t n, double* dout);
// the row count on the device: the launch covers nmax rows, min(*dcount, nmax) are scored
void fd_svm_f32_launch_counted(hipStream_t st, const fd_svm* m, const void* dfeat, int64_t stride_bytes, int64_t nmax, const unsigned int* dcount,
                               double* dout);
bool fd_svm_u8_mfma_available(const fd_svm* m);
void fd_svm_u8_mfma_launch_counted(hipStream_t st, const fd_svm* m, const void* dfeat, const uint32_t* didx, int64_t stride_bytes, int64_t nmax,
                                   const unsigned int* dcount, double* dout);
// classifier positives of N scored windows -> detection records in extraction order (hog.hip)
void fd_svm_positives_to_detections(fd_ctx* ctx, const fd_pyramid* p, const fd_svm* svm, const std::vector<WindowLayer>& wls, int sx, int sy,
                                    const double* ddist, int64_t N, fd_detection* out, int64_t cap, int64_t* count, double* all_distance);

// ---------------- sampled windows: what follows the feature rows (hist_samples.hpp, patch_samples.hpp, integral.hip) ----------------
// nv rows of F floats at dfeat (device, queued on ctx->stream) -> features[n][F] (host, zeroed by the caller): row k belongs to sample
// sampleOf[k].  The rows are in place when every sample has a window; otherwise they are downloaded and scattered.  Synchronises.
static inline void fd_samples_rows_to_host(fd_ctx* ctx, const float* dfeat, int F, int64_t nv, int n, const std::vector<int>& sampleOf, float* features) {
    const size_t rowBytes = sizeof(float) * (size_t)F;
    std::vector<float> rows(nv == n ? 0 : (size_t)nv * F);
    float* dst = nv == n ? features : rows.data();
    HIP_CHECK(hipMemcpyAsync(dst, dfeat, rowBytes * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (nv == n) return;
    for (int64_t k = 0; k < nv; ++k) std::memcpy(features + (size_t)sampleOf[k] * F, dst + (size_t)k * F, rowBytes);
}

static inline void fd_samples_require_f32_svm(const fd_svm* svm, int F, const char* who) {
    if (fd_svm_is_u8(svm) || fd_svm_dim(svm) != F)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the SVM must work on f32 vectors of length %d (it has %d %s values)", who, F, fd_svm_dim(svm),
                 fd_svm_is_u8(svm) ? "u8" : "f32");
}

// what a sample without a window keeps: target 0, weight 0, distance 0 (distance may be NULL)
static inline void fd_samples_clear(int n, uint8_t* target, double* weight, double* distance) {
    std::memset(target, 0, (size_t)n);
    std::fill(weight, weight + n, 0.0);
    if (distance) std::fill(distance, distance + n, 0.0);
}

// The SVM on nv feature rows of F floats at dfeat: one launch, the distances into hdist (host, nv doubles) through ddist, one wait, then
// SvmClassifier::classify (distance >= threshold) and ProbabilisticSvmClassifier::getProbability per row.  With sampleOf (the pyramid
// families) row k is sample sampleOf[k] and the caller has cleared the outputs; without (the integral family) row k is sample k and the
// kernels' validity bytes at dvalid come into target with the distances: an invalid sample gets target 0, weight 0.
static inline void fd_samples_svm_tail(fd_ctx* ctx, const fd_svm* svm, const void* dfeat, int F, int64_t nv, DevBuf& ddist, double* hdist,
                                       const int* sampleOf, const void* dvalid, uint8_t* target, double* weight, double* distance) {
    ddist.reserve(sizeof(double) * (size_t)nv);
    fd_svm_generic_launch(ctx, svm, dfeat, nullptr, (int64_t)F * 4, nv, ddist.as<double>());
    HIP_CHECK(hipMemcpyAsync(hdist, ddist.p, sizeof(double) * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
    if (!sampleOf) HIP_CHECK(hipMemcpyAsync(target, dvalid, (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const double threshold = (double)fd_svm_threshold(svm);
    for (int64_t k = 0; k < nv; ++k) {
        const int64_t i = sampleOf ? sampleOf[k] : k;
        const bool valid = sampleOf || target[i];
        target[i] = valid && hdist[k] >= threshold ? 1 : 0;
        weight[i] = valid ? fd_svm_probability(svm, hdist[k]) : 0.0;
        if (distance) distance[i] = valid ? hdist[k] : 0.0;
    }
}

// ---------------- the whi chain and ConversionFilter on device-resident data (whi.hip), for patch_samples.hpp ----------------
// the whole whi chain on `total` listed windows {layer, bx, by} (device memory) of the gray planes of p: total x (patch_w * patch_h) floats
// into dfeat.  Queued on ctx->stream.  Throws FdError (a patch side outside 2..32) before anything is queued
void fd_whi_list_launch(fd_ctx* ctx, const fd_pyramid* p, const int32_t* dlist, int64_t total, int patch_w, int patch_h, float alpha, float cutoff,
                        float* dfeat);
// ConversionFilter(CV_32F, scale, shift) on count u8 values: dst[i] = float(src[i]) * scale + shift.  Queued on ctx->stream
void fd_convert_u8_f32_launch(fd_ctx* ctx, const uint8_t* dsrc, int64_t count, float scale, float shift, float* ddst);

// ---------------- SVM training (svm_train.hip) ----------------
// Where the support-vector form (fd_kernel_svm_*) leaves one problem's model (host).  The first n_sv entries of sv_index /
// coefficients and the first n_sv rows of support_vectors are written.
struct FdSvmSvOut {
    int32_t* sv_index;
    float* coefficients;
    float* support_vectors;           // n x d, or NULL
    std::vector<float>* sv_store;     // in place of support_vectors: resized to n_sv x d
};
// One run of the trainer
struct FdSvmRunSpec {
    const char* who;                  // the entry point, for the messages
    bool large = false;               // the solver for up to FD_SVM_LARGE_MAX_N examples (Q always in memory); else up to 1024
    float* wOverride = nullptr;       // device memory that receives problem 0's weights in place of its host buffer (the tracker's dweights)
    bool svForm = false;              // the model as support vectors and coefficients of `kernel` (checked); else one linear weight vector
    int32_t kernel = FD_KERNEL_LINEAR, degree = 0;
    double gamma = 0.0, coef0 = 0.0;
    const FdSvmSvOut* outs = nullptr; // svForm: one entry per problem, or NULL (the Gram alone)
    double nu = 0.0;                  // > 0: one-class problems (n_neg = 0, linear term 0, libsvm's start state for this nu); svForm only
};
// trains `count` problems in one set of launches.  Throws FdError; leaves ctx->stream synchronised.
void fd_svm_train_run(fd_ctx* ctx, const FdSvmRunSpec& spec, int count, const fd_svm_train_problem* probs, const fd_svm_train_params* params,
                      fd_svm_train_info* infos);

// ---------------- resident particle set (condensation.hip) on an extended-HOG tracker (ehog_tracker.hpp) ----------------
// scores n samples held in device memory (x, y, size; height = cvRound(aspect * size)): the window list (4 n ints), valid and score are
// the caller's device buffers.  Queued on ctx->stream, no host wait.  Throws FdError.
void fd_ehog_tracker_score_particles(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* x, const int32_t* y, const int32_t* size, double aspect,
                                     int use_patches, int32_t* windows, uint8_t* valid, double* score);

// ---------------- resident particle set on the integral family and the optical flow (condensation.hip, integral.hip, optflow.hip) ----------------
// the current generation as the scoring kernels of another file need it (device memory); checks p against ctx.  Throws FdError.
struct FdParticlesView {
    int n;
    const int32_t *x, *y, *size;
    double* score;
    uint8_t* valid;
    int32_t* windows;   // 4 n ints: the trace of the evaluation
};
// one wrapper's map of a sample {x, y, width, height} (fd_sample_map, fd_hip.h): PatchResizingFeatureExtractor::mapSample and
// IntegralFeatureExtractor::mapSample, the one copy of these expressions for the host (fd_sample_maps_apply) and the device
// (fd_particle_sample).  cvRound is fd_sample_cvround; the sums and products are doubles in this order.
__host__ __device__ inline void fd_sample_map_apply(const fd_sample_map& m, int32_t& x, int32_t& y, int32_t& width, int32_t& height) {
    if (m.kind == FD_SAMPLE_MAP_RESIZE) {
        x = fd_sample_cvround(x + m.x_offset * width);
        y = fd_sample_cvround(y + m.y_offset * height);
        width = fd_sample_cvround(m.factor * width);
        height = fd_sample_cvround(m.factor * height);
    } else {
        x += width % 2 == 0 ? 0 : 1;
        y += height % 2 == 0 ? 0 : 1;
        width += 1;
        height += 1;
    }
}
// the wrapper chain of a call as a kernel argument
struct FdSampleMaps {
    int32_t n;
    fd_sample_map m[FD_SAMPLE_MAPS_MAX];
};
// The chain of a call, checked: FD_ERR_INVALID_ARGUMENT for a negative count or NULL with a positive one ("bad argument"), for more than
// FD_SAMPLE_MAPS_MAX maps, and for a kind whose bit (1 << kind) allowedKindsMask does not hold.  hostalgo.cpp
FdSampleMaps fd_sample_maps_checked(const fd_sample_map* maps, int n_maps, unsigned allowedKindsMask, const char* who);
// the sample of a particle (x, y, size; height = cvRound(aspect * size), Sample.hpp:127-129) through the wrapper chain of its feature
// extractor, outer to inner: what k_particles_xywh and k_particles_windows start from
__host__ __device__ inline void fd_particle_sample(int32_t px, int32_t py, int32_t size, double aspect, const FdSampleMaps& maps, int32_t& x, int32_t& y,
                                                   int32_t& width, int32_t& height) {
    x = px; y = py; width = size; height = fd_sample_cvround(aspect * (double)size);
    for (int k = 0; k < maps.n; ++k) fd_sample_map_apply(maps.m[k], x, y, width, height);
}
FdParticlesView fd_particles_view(fd_ctx* ctx, fd_particles* p, const char* who);
void fd_particles_set_evaluated(fd_particles* p);
// ---- the box of PositionDependentMeasurementModel::adapt's additional negatives (PositionDependentMeasurementModel.cpp:155-170): the one
// copy of these expressions for the host (fd_particles_negatives_bounds, hostalgo.cpp) and the device (k_particles_negatives) ----
// (int) of a float: truncated; saturated where the cast would not be defined, 0 for a NaN (what the device's conversion does by itself)
__host__ __device__ inline int32_t fd_float_to_int(float v) {
    if (!(v == v)) return 0;
    if (v >= 2147483648.f) return INT32_MAX;
    if (v <= -2147483648.f) return INT32_MIN;
    return (int32_t)v;
}
struct FdNegativeBounds { int32_t xLow, xHigh, yLow, yHigh, sizeLow, sizeHigh; };
// float * int is a float product; the sums wrap (the reference's overflow there)
__host__ __device__ inline FdNegativeBounds fd_negative_bounds(float offsetFactor, float downScale, float upScale, int32_t x, int32_t y, int32_t size) {
    const uint32_t offset = (uint32_t)fd_float_to_int(offsetFactor * (float)size);
    FdNegativeBounds b;
    b.xLow = (int32_t)((uint32_t)x - offset); b.xHigh = (int32_t)((uint32_t)x + offset);
    b.yLow = (int32_t)((uint32_t)y - offset); b.yHigh = (int32_t)((uint32_t)y + offset);
    b.sizeLow = fd_float_to_int(downScale * (float)size);
    b.sizeHigh = fd_float_to_int(upScale * (float)size);
    return b;
}
__host__ __device__ inline bool fd_negative_outside(const FdNegativeBounds& b, int32_t x, int32_t y, int32_t size) {
    return x <= b.xLow || x >= b.xHigh || y <= b.yLow || y >= b.yHigh || size <= b.sizeLow || size >= b.sizeHigh;
}
// ---- the examples of SelfLearningMeasurementModel::adapt (SelfLearningMeasurementModel.cpp:89-125): the one copy of the rule's
// comparisons for the host (fd_particles_examples_select, hostalgo.cpp) and the device (k_particles_examples, particle_examples.hpp) ----
__host__ __device__ inline bool fd_example_candidate(bool positive, double weight, double threshold) { return positive ? weight > threshold : weight < threshold; }
// the list order of a side with more than max_count candidates: a before b.  Equal weights (-0 and +0 are equal): the lower index
__host__ __device__ inline bool fd_example_before(bool positive, double wa, int32_t ia, double wb, int32_t ib) {
    if (wa != wb) return positive ? wa > wb : wa < wb;
    return ia < ib;
}
// The device half of fd_particles_state_examples_*, for the family's file (integral.hip).  _check throws FdError for every argument of
// the call that does not belong to the extractor; _begin checks the row capacity, then queues k_particles_state and k_particles_examples and
// returns where the family's rows (2 * max_count x rowLength floats, slot s < max_count: positive s, slot max_count + s: negative s)
// and their validity bytes go in the read-back block.  _xywh queues the chosen samples through the chain as {x, y, width, height}
// into dxywh (2 * max_count entries; an unused slot gets {0, 0, 0, 0}, which no extractor computes).  _end brings the block back in
// one copy and one wait and fills the caller's arguments; throws FD_ERR_RUNTIME with bad_weight.
struct FdExamplesArgs {
    fd_flow* flow;
    const fd_particles_examples_params* params;
    fd_particles_info* info;
    fd_flow_motion_info* motion;
    int *n_pos, *n_neg;
    fd_particles_example *pos, *neg;
    float* rows;
    int row_capacity;
    int* row_length;
};
struct FdExamplesRun {
    float* rows;
    uint8_t* valid;
};
void fd_particles_examples_check(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, const char* who);   // all of a but the row capacity
FdExamplesRun fd_particles_examples_begin(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, int rowLength, const char* who);
void fd_particles_examples_xywh(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, double aspect, const FdSampleMaps& chain, int32_t* dxywh);
void fd_particles_examples_end(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, int rowLength, const char* who);
// ---- resident particle set on the pyramid families (condensation.hip launches k_particles_windows; the scoring kernels are hog.hip's and rvm.hip's) ----
// "Score this device list of n windows {layer, bx, by} of p into this device score array": the kernels of fd_hist_svm_evaluate_samples
// (kind FD_SAMPLES_HIST / FD_SAMPLES_EHOG, hog.hip) and of fd_patch_svm_evaluate_samples (rvm.hip) and the SVM launch, queued on
// ctx->stream, no host wait.  Every argument rule of those entry points is checked first (FdError, nothing queued); with dlist NULL that is
// all the call does.  patch_w / patch_h receive the window size of the parameters.
void fd_hist_samples_score_list(fd_ctx* ctx, const fd_pyramid* p, int kind, const void* params, const fd_svm* svm, const char* who, const int32_t* dlist,
                                int n, double* dscore, int* patch_w, int* patch_h);
void fd_patch_samples_score_list(fd_ctx* ctx, const fd_pyramid* p, const fd_patch_samples_params* pp, const fd_svm* svm, const char* who,
                                 const int32_t* dlist, int n, double* dscore, int* patch_w, int* patch_h);
// "Leave the feature rows of this device list of n windows on the device": the kernels of fd_hist_extract_samples / fd_ehog_extract_samples
// (hog.hip) and of fd_patch_extract_samples (rvm.hip), queued on ctx->stream, no host wait; the rows are the family's scratch and hold
// until its next call.  Every argument rule of those entry points is checked first; with dlist NULL that is all the call does.
const float* fd_hist_samples_features_list(fd_ctx* ctx, const fd_pyramid* p, int kind, const void* params, const char* who, const int32_t* dlist, int n,
                                           int* row_length, int* patch_w, int* patch_h);
const float* fd_patch_samples_features_list(fd_ctx* ctx, const fd_pyramid* p, const fd_patch_samples_params* pp, const char* who, const int32_t* dlist, int n,
                                            int* row_length, int* patch_w, int* patch_h);
// ---- resident particle set on condensation::WvmSvmModel (condensation.hip with particle_wvm_svm.hpp; the cascade is wvm.hip's) ----
// What a list-mode cascade run with per-window outputs leaves on the device, for the kernels queued behind it on ctx->stream.  The
// buffers are the WVM handle's: they hold until its next run.
struct FdWvmResidentRun {
    const uint4* pos;               // positive records {window id low, high, level, fp32 bits of fout}; the record's place is its patch row
    const unsigned int* pos_count;  // their number (at most the windows of the list)
    const uint8_t* patches;         // dim bytes per row: the equalised patch of the positive at that place
    const float* fout;              // per window of the list
    const int32_t* level;
    int dim;
    uint64_t serial;                // fd_wvm_run_serial behind this run: another one afterwards means the buffers are another run's
};
// the rules of the pair: both belong to ctx, the SVM works on u8 vectors of the WVM's dimension (five_stage_check).  Throws FdError
void fd_wvm_svm_pair_check(fd_ctx* ctx, const fd_wvm* m, const fd_svm* svm, const char* who);
// every argument rule of a resident run of (m, svm) on n windows of p; throws FdError before anything is queued
void fd_wvm_resident_check(fd_ctx* ctx, const fd_pyramid* p, const fd_wvm* m, const fd_svm* svm, int n, const char* who);
// counts the cascade runs launched on the handle (every run reuses, and may reallocate, its output buffers)
uint64_t fd_wvm_run_serial(const fd_wvm* m);
// the exact cascade (stage A, stage B) on the n >= 1 windows {layer, bx, by} at dlist, queued on ctx->stream: no wait, no copy.  The positive
// buffer and stage B's state hold all n windows whatever FD_WVM_POS_CAP says.  Leaves the handle as a run with per-window outputs does.
void fd_wvm_list_launch_resident(fd_ctx* ctx, fd_pyramid* p, fd_wvm* m, const int32_t* dlist, int n, FdWvmResidentRun& out);
void fd_wvm_patch_size(const fd_wvm* m, int* fw, int* fh);
void fd_wvm_logistic(const fd_wvm* m, double* a, double* b);
void fd_svm_logistic(const fd_svm* m, double* a, double* b);
const fd_ctx* fd_svm_context(const fd_svm* m);
// the motion a resident track (or fd_debug_flow_motion) left in the handle (device memory); checks flow against ctx, throws FdError
// (FD_ERR_RUNTIME) when there is none
const fd_flow_motion_info* fd_flow_device_motion(fd_ctx* ctx, fd_flow* flow, const char* who);

// ---------------- host-side detection logic (hostalgo.cpp) ----------------
void fd_host_overlap_elimination(const fd_detection* in, int n, float dist, float ratio, std::vector<int>& keep);
void fd_host_block_nms_sparse(const std::vector<fd_detection>& pos, int imgW, int imgH, int sz, bool masked,
                              std::vector<int>& maxima_xy /* pairs x,y in row-major order */);
// feature pyramid of the aggregated-features detector: scale limits, and the layer list of the approximated form
struct FdAggregatedPlan {
    double minScale = 0, maxScale = 0;
    std::vector<fd_aggregated_layer> layers;       // layer order: every exact layer followed by its approximations
    std::vector<std::pair<int, int>> exactPx;      // (w, h) in pixels of the exact layers' gray source layers, in layer order
};
void fd_host_aggregated_limits(int window_w, int window_h, int cell_size, int octave_layer_count, int min_window_width, int width, int height,
                               double& minScale, double& maxScale);
void fd_host_plan_aggregated(int cell_size, int octave_layer_count, double minScale, double maxScale, int width, int height,
                             FdAggregatedPlan& plan);
// HaarFeatureFilter's feature table (HaarFeatureFilter.cpp:41-136); false on invalid parameters
bool fd_host_haar_features(const fd_haar_params* hp, std::vector<fd_haar_feature>& features);
// limits of the integral-image calls (fd_integral_gradient_length, fd_gradient_sum_length, fd_surf_feature_length in hostalgo.cpp)
constexpr int FD_GRADIENT_MAX_GRID = 16384;           // rows / cols of a gradient patch: 2 * rows * cols stays an int
constexpr int FD_SURF_MAX_GRID = 64;                  // gradient_count of the fused SURF kernel
constexpr size_t FD_SURF_LDS_BUDGET = 160 * 1024;     // LDS of one gfx950 workgroup
// dynamic LDS of one workgroup of the fused SURF kernel (four wavefronts)
size_t fd_host_surf_lds_bytes(int gradient_count, int cell_count);

// ---------------- integral HOG: the ihog / iehog chains on sampled windows (integral_hog.hpp, included by hog.hip) ----------------
// GradientBinningFilter's 65536-entry look-up table (pyramid.hip): 2 bytes per entry, 4 with bin interpolation
void fd_build_gradient_lut(int bins, bool signedGradients, bool interpolate, std::vector<uint8_t>& lut);
// every argument rule of fd_integral_hog_params, with a message for each (FdError); returns the floats per sample
int fd_integral_hog_check(const fd_integral_hog_params* p);
// k_integral_hog (and k_ehog_patch_desc for FD_SAMPLES_EHOG) over the n uploaded samples, queued on ctx->stream: `feat` receives
// n x fd_integral_hog_check(p) floats, `valid` n bytes; `raw` is scratch (the cell histograms of the ehog kind).  img: the
// (H + 1) x (W + 1) integral image, lut: the table of (p->bins, p->signed_gradients, p->interpolate_bins) on the device
void fd_integral_hog_launch(fd_ctx* ctx, const fd_integral_hog_params* p, const int32_t* img, int W, int H, const uint8_t* lut, const int32_t* xywh,
                            int n, DevBuf& raw, DevBuf& feat, uint8_t* valid);
