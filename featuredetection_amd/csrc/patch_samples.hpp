// featuredetection_amd/csrc/patch_samples.hpp -- the gray-patch feature spaces (grayscale, HistEq64Filter, HistogramEqualizationFilter, each
// followed by ConversionFilter(CV_32F, scale, shift), and the whi chain) and the RVM cascade on explicit sample windows of a gray pyramid:
// DirectPyramidFeatureExtractor::extract(x, y, width, height) for all samples of a call, and what the tracker puts on top of it
// (condensation::SingleClassifierModel, FilteringClassifierModel.cpp:27-103, ClassificationBasedStateValidator.cpp:28-45).  Included by
// rvm.hip only, at its end.
//
// Two routes to the cascade's verdicts, same bits:
//   fused     k_rvm_samples: one launch.  A wavefront gathers its window from the layer in place (list mode of the window table), filters
//             it in LDS, converts it once to f32 and walks the cascade from level 0 in blocks of 64 levels (rvm_level_blocks, the loop of
//             k_rvm_deep).  No feature row goes to memory, no queue, no counter.
//   composed  k_window_patches (k_whi<0> for the whi chain) in list mode writes the rows, run_cascade's passes score them.
// A row's distance does not depend on the route: both evaluate the fp32 chain in element order and add the terms in level order.  The whi
// chain, the SVM call and fd_patch_extract_samples take the composed kernels; between the two routes of the RVM call patch_rvm_fused()
// decides, by the sample count or by FD_PATCH_FUSED.
#pragma once

namespace {

// the fused kernel serves calls of this many listed windows (measured, DESIGN.md 4.16: its median lies below the composed route's 10th
// percentile at 50 to 8192 windows, not at 27 and not from 12288 on)
constexpr int64_t PATCH_FUSED_MIN_WINDOWS = 50, PATCH_FUSED_MAX_WINDOWS = 8192;

struct PatchScratch {
    DevBuf list, u8, feat, dist;
};
PatchScratch& patch_scratch(fd_ctx* ctx) { return fd_scratch<PatchScratch>(ctx); }

bool patch_params_ok(const fd_patch_samples_params* pp) {
    if (!pp) return false;
    const int lo = pp->feature_space == FD_FEATURE_WHI ? 2 : 1;   // WhiteningFilter's frequency grid divides by (side - 1)
    return pp->feature_space >= FD_FEATURE_GRAY && pp->feature_space <= FD_FEATURE_WHI && pp->patch_w >= lo && pp->patch_h >= lo &&
           pp->patch_w <= RVM_MAX_DIM && pp->patch_h <= RVM_MAX_DIM;
}

// every argument rule of the three entry points, before anything is queued
void patch_samples_check(fd_ctx* ctx, const fd_pyramid* p, const fd_patch_samples_params* pp, int n, const fd_rvm* rvm, const fd_svm* svm,
                         const char* who) {
    if (p->ctx != ctx || (rvm && rvm->ctx != ctx)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: objects belong to different contexts", who);
    fd_pyramid_require_single(p, who);
    if (p->all.empty()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the pyramid has not been updated with an image", who);
    if (p->filter_kind != FD_LAYER_NONE) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: gray-patch features need a gray pyramid (no layer filter)", who);
    if (n < 0 || n > FD_HIST_SAMPLES_MAX) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the sample count %d is outside 0..%d", who, n, (int)FD_HIST_SAMPLES_MAX);
    if (pp->patch_w < 1 || pp->patch_h < 1 || pp->patch_w > RVM_MAX_DIM || pp->patch_h > RVM_MAX_DIM)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the patch size %d x %d is outside 1..%d", who, pp->patch_w, pp->patch_h, RVM_MAX_DIM);
    if (pp->feature_space < FD_FEATURE_GRAY || pp->feature_space > FD_FEATURE_WHI)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown feature space %d", who, pp->feature_space);
    if (!patch_params_ok(pp)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the whi chain needs a patch of at least 2 x 2", who);
    const int dim = pp->patch_w * pp->patch_h;
    if (rvm && (rvm->filter_w != pp->patch_w || rvm->filter_h != pp->patch_h))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the RVM's filter size %d x %d is not the patch size %d x %d", who, rvm->filter_w, rvm->filter_h,
                 pp->patch_w, pp->patch_h);
    if (svm) fd_samples_require_f32_svm(svm, dim, who);
}

// which route fd_patch_rvm_evaluate_samples takes for nv listed windows: the one size rule
bool patch_rvm_fused(const fd_patch_samples_params* pp, int64_t nv) {
    if (pp->feature_space == FD_FEATURE_WHI) return false;
    const int knob = fd_knob_patch_fused();
    return knob >= 0 ? knob == 1 : (nv >= PATCH_FUSED_MIN_WINDOWS && nv <= PATCH_FUSED_MAX_WINDOWS);
}

// what k_rvm_samples leaves per listed window: one record, so that one copy brings a call's results back
struct PatchRvmOut {
    double d;
    int32_t level, pad;
};

int patch_rvm_samples_grid(const fd_ctx* ctx, int64_t nv) { return (int)std::min<int64_t>((nv + 3) / 4, (int64_t)ctx->num_cus * 8); }

// The cascade of m on the listed windows, one wavefront per window, four to a workgroup.  LDS per wavefront: the window's bytes (1 KB), the
// filtered bytes (1 KB), the histogram (1 KB), the LUT (1 KB) and the converted vector (4 KB).  mode: FD_FEATURE_GRAY / HQ64 / HISTEQ.
__global__ __launch_bounds__(256) void k_rvm_samples(const uint8_t* __restrict__ arena, FdWinTable wt, RvmDev m, int pw, int ph, int mode, float scale,
                                                     float shift, PatchRvmOut* __restrict__ out) {
    __shared__ unsigned char px[4][RVM_MAX_DIM * RVM_MAX_DIM];
    __shared__ unsigned char eq[4][RVM_MAX_DIM * RVM_MAX_DIM];
    __shared__ int hist[4][256];
    __shared__ int lut[4][256];
    __shared__ float xs[4][RVM_MAX_DIM * RVM_MAX_DIM];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n = pw * ph;
    unsigned char* p = px[wave];
    unsigned char* q = eq[wave];
    float* x = xs[wave];
    for (int64_t wid = (int64_t)blockIdx.x * 4 + wave; wid < wt.total; wid += (int64_t)gridDim.x * 4) {
        int x0, y0;
        const FdWinLayer& wl = win_locate(wt, wid, x0, y0);
        const uint8_t* src = arena + wl.off + (size_t)y0 * wl.lw + x0;
        for (int i = lane; i < n; i += 64) {
            const int y = i / pw, c = i - y * pw;
            p[i] = src[(size_t)y * wl.lw + c];
        }
        wave_sync();
        const unsigned char* res = p;
        if (mode == FD_FEATURE_HQ64) { histeq64_wave(p, q, n, hist[wave], lane); res = q; }
        else if (mode == FD_FEATURE_HISTEQ) { equalize_hist_wave(p, q, n, hist[wave], lut[wave], lane); res = q; }
        for (int i = lane; i < n; i += 64) x[i] = (float)res[i] * scale + shift;   // cv::Mat::convertTo(CV_32F, scale, shift)
        wave_sync();
        const RvmExit ex = rvm_level_blocks(m, x, 0, 0.0, lane);
        if (lane == ex.lane) out[wid] = PatchRvmOut{ex.d, ex.level, 0};
        wave_sync();
    }
}

// the u8 rows of the nv windows listed at dlist (device) into S.u8 (GRAY / HQ64 / HISTEQ): k_window_patches in list mode
void patch_u8_rows(fd_ctx* ctx, const fd_pyramid* p, const fd_patch_samples_params* pp, const int32_t* dlist, int64_t nv, PatchScratch& S) {
    const int dim = pp->patch_w * pp->patch_h;
    FdWinTable wt;
    fd_win_table_list(p, dlist, nv, /*filtered=*/false, wt);
    S.u8.reserve((size_t)nv * dim + 16);
    hipLaunchKernelGGL(k_window_patches, dim3((unsigned)std::min<int64_t>(nv, (int64_t)ctx->num_cus * 32)), dim3(64), 0, ctx->stream,
                       p->arena.as<uint8_t>(), wt, pp->patch_w, pp->patch_h, pp->feature_space, S.u8.as<uint8_t>());
    HIP_CHECK(hipGetLastError());
}

// the f32 feature rows of the nv windows listed at dlist (device), [nv][dim] on the device: queued on ctx->stream
const float* patch_f32_rows(fd_ctx* ctx, const fd_pyramid* p, const fd_patch_samples_params* pp, const int32_t* dlist, int64_t nv, PatchScratch& S) {
    const int dim = pp->patch_w * pp->patch_h;
    S.feat.reserve(sizeof(float) * (size_t)nv * dim);
    if (pp->feature_space == FD_FEATURE_WHI) {
        fd_whi_list_launch(ctx, p, dlist, nv, pp->patch_w, pp->patch_h, pp->whi_alpha, pp->whi_cutoff, S.feat.as<float>());
    } else {
        patch_u8_rows(ctx, p, pp, dlist, nv, S);
        fd_convert_u8_f32_launch(ctx, S.u8.as<uint8_t>(), nv * dim, pp->conv_scale, pp->conv_shift, S.feat.as<float>());
    }
    return S.feat.as<float>();
}

}  // namespace

// the resident particle set's bridge (fd_internal.hpp): the argument rules of fd_patch_svm_evaluate_samples, then its kernels on the list
void fd_patch_samples_score_list(fd_ctx* ctx, const fd_pyramid* p, const fd_patch_samples_params* pp, const fd_svm* svm, const char* who,
                                 const int32_t* dlist, int n, double* dscore, int* patch_w, int* patch_h) {
    patch_samples_check(ctx, p, pp, n, nullptr, svm, who);
    *patch_w = pp->patch_w; *patch_h = pp->patch_h;
    if (!dlist || n == 0) return;
    fd_pyramid_wait(p, ctx->stream);
    fd_svm_generic_launch(ctx, svm, patch_f32_rows(ctx, p, pp, dlist, n, patch_scratch(ctx)), nullptr, (int64_t)pp->patch_w * pp->patch_h * 4, n, dscore);
}

// the same list's feature rows, left on the device ([n][patch_w * patch_h] floats, the context's scratch: they hold until its next
// call), for fd_particles_state_examples_pyramid; with dlist NULL the argument rules of fd_patch_extract_samples alone
const float* fd_patch_samples_features_list(fd_ctx* ctx, const fd_pyramid* p, const fd_patch_samples_params* pp, const char* who, const int32_t* dlist, int n,
                                            int* row_length, int* patch_w, int* patch_h) {
    patch_samples_check(ctx, p, pp, n, nullptr, nullptr, who);
    *row_length = pp->patch_w * pp->patch_h; *patch_w = pp->patch_w; *patch_h = pp->patch_h;
    if (!dlist || n == 0) return nullptr;
    fd_pyramid_wait(p, ctx->stream);
    return patch_f32_rows(ctx, p, pp, dlist, n, patch_scratch(ctx));
}

extern "C" {

int fd_patch_feature_length(const fd_patch_samples_params* pp) { return patch_params_ok(pp) ? pp->patch_w * pp->patch_h : -1; }

int fd_patch_extract_samples(fd_ctx* ctx, fd_pyramid* p, const fd_patch_samples_params* pp, int n, const int32_t* xywh, uint8_t* valid,
                             float* features) {
    return fd_guard(ctx, [&] {
        const char* who = "fd_patch_extract_samples";
        if (!ctx || !p || !pp || (n > 0 && !xywh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        patch_samples_check(ctx, p, pp, n, nullptr, nullptr, who);
        if (n == 0) return;
        const int dim = pp->patch_w * pp->patch_h;
        if (features) std::memset(features, 0, sizeof(float) * (size_t)n * dim);
        PatchScratch& S = patch_scratch(ctx);
        std::vector<int> sampleOf;
        fd_samples_upload(ctx, p, pp->patch_w, pp->patch_h, n, xywh, valid, S.list, sampleOf, 0);
        const int64_t nv = (int64_t)sampleOf.size();
        if (nv == 0 || !features) return;
        fd_pyramid_wait(p, ctx->stream);
        fd_samples_rows_to_host(ctx, patch_f32_rows(ctx, p, pp, S.list.as<int32_t>(), nv, S), dim, nv, n, sampleOf, features);
    });
}

int fd_patch_svm_evaluate_samples(fd_ctx* ctx, fd_pyramid* p, const fd_patch_samples_params* pp, const fd_svm* svm, int n, const int32_t* xywh,
                                  uint8_t* target, double* weight, double* distance) {
    return fd_guard(ctx, [&] {
        const char* who = "fd_patch_svm_evaluate_samples";
        if (!ctx || !p || !pp || !svm || (n > 0 && (!xywh || !target || !weight))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        patch_samples_check(ctx, p, pp, n, nullptr, svm, who);
        if (n == 0) return;
        fd_samples_clear(n, target, weight, distance);
        PatchScratch& S = patch_scratch(ctx);
        std::vector<int> sampleOf;
        double* hdist = (double*)fd_samples_upload(ctx, p, pp->patch_w, pp->patch_h, n, xywh, nullptr, S.list, sampleOf, sizeof(double));
        const int64_t nv = (int64_t)sampleOf.size();
        if (nv == 0) return;
        fd_pyramid_wait(p, ctx->stream);
        fd_samples_svm_tail(ctx, svm, patch_f32_rows(ctx, p, pp, S.list.as<int32_t>(), nv, S), pp->patch_w * pp->patch_h, nv, S.dist, hdist, sampleOf.data(), nullptr, target, weight,
                            distance);
    });
}

int fd_patch_rvm_evaluate_samples(fd_ctx* ctx, fd_pyramid* p, const fd_patch_samples_params* pp, const fd_rvm* rvm_, int n, const int32_t* xywh,
                                  uint8_t* valid, int32_t* level, double* distance, uint8_t* target) {
    return fd_guard(ctx, [&] {
        const char* who = "fd_patch_rvm_evaluate_samples";
        if (!ctx || !p || !pp || !rvm_ || (n > 0 && !xywh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        patch_samples_check(ctx, p, pp, n, rvm_, nullptr, who);
        if (n == 0) return;
        fd_rvm* m = const_cast<fd_rvm*>(rvm_);
        if (target) std::memset(target, 0, (size_t)n);
        for (int i = 0; i < n; ++i) {
            if (level) level[i] = -1;
            if (distance) distance[i] = 0.0;
        }
        PatchScratch& S = patch_scratch(ctx);
        std::vector<int> sampleOf;
        char* pin = (char*)fd_samples_upload(ctx, p, pp->patch_w, pp->patch_h, n, xywh, valid, S.list, sampleOf, sizeof(PatchRvmOut));
        const int64_t nv = (int64_t)sampleOf.size();
        if (nv == 0 || !(level || distance || target)) return;
        fd_pyramid_wait(p, ctx->stream);
        const int dim = pp->patch_w * pp->patch_h;
        const bool fused = patch_rvm_fused(pp, nv);
        PatchRvmOut* hout = (PatchRvmOut*)pin;                 // fused: the records
        double* hdist = (double*)pin;                          // composed: the cascade's two arrays
        int32_t* hlevel = (int32_t*)(hdist + nv);
        if (fused) {
            FdWinTable wt;
            fd_win_table_list(p, S.list.as<int32_t>(), nv, /*filtered=*/false, wt);
            S.dist.reserve(sizeof(PatchRvmOut) * (size_t)nv);
            hipLaunchKernelGGL(k_rvm_samples, dim3(patch_rvm_samples_grid(ctx, nv)), dim3(256), 0, ctx->stream, p->arena.as<uint8_t>(), wt, m->dev,
                               pp->patch_w, pp->patch_h, pp->feature_space, pp->conv_scale, pp->conv_shift, S.dist.as<PatchRvmOut>());
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(hout, S.dist.p, sizeof(PatchRvmOut) * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            if (pp->feature_space == FD_FEATURE_WHI) {
                run_cascade<false>(ctx, m, patch_f32_rows(ctx, p, pp, S.list.as<int32_t>(), nv, S), (int64_t)dim * 4, 1.f, 0.f, nv, true, 0u);
            } else {
                patch_u8_rows(ctx, p, pp, S.list.as<int32_t>(), nv, S);
                run_cascade<true>(ctx, m, S.u8.p, (int64_t)dim, pp->conv_scale, pp->conv_shift, nv, true, 0u);
            }
            HIP_CHECK(hipMemcpyAsync(hdist, m->dist.p, sizeof(double) * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(hlevel, m->level.p, sizeof(int32_t) * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const int last = m->dev.numUse - 1;
        const double thrLast = (double)m->h_thr[last];
        for (int64_t k = 0; k < nv; ++k) {   // RvmClassifier::classify (RvmClassifier.cpp:68-73): the last used level is reached and passed
            const int i = sampleOf[k];
            const int lv = fused ? hout[k].level : hlevel[k];
            const double d = fused ? hout[k].d : hdist[k];
            if (level) level[i] = lv;
            if (distance) distance[i] = d;
            if (target) target[i] = (lv == last && d >= thrLast) ? 1 : 0;
        }
    });
}

}  // extern "C"
