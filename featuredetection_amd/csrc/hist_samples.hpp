// featuredetection_amd/csrc/hist_samples.hpp -- the histogram family (the four FD_HIST_* patch filters and ExtendedHogFilter) on
// explicit sample windows of a filtered pyramid: DirectPyramidFeatureExtractor::extract(x, y, width, height)
// (DirectPyramidFeatureExtractor.cpp:67-73,134-153) for all samples of a call in one launch, and
// condensation::SingleClassifierModel::evaluate (SingleClassifierModel.cpp:32-52) on top of it.  Included by hog.hip behind
// ehog_patch.hpp: the windows go through k_hist_features in the list mode of the window table (win_table.hpp), which reads the
// layers in place; only samples with a window are in the list, the host keeps sampleOf[] and scatters the results.
#pragma once

namespace {

// what a sampled call needs to know before it launches anything: every argument rule of the three entry points
struct SamplesPlan {
    fd_hist_params hp;     // the cell-histogram stage (for ExtendedHogFilter: its SpatialHistogramFilter stand-in)
    HistDev hd;
    bool ehog = false;
    fd_ehog_patch_params ep;
    int F = 0;             // floats per sample
};
SamplesPlan samples_plan(fd_ctx* ctx, const fd_pyramid* p, int kind, const void* params, int n, const char* who) {
    if (kind != FD_SAMPLES_HIST && kind != FD_SAMPLES_EHOG) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown feature kind %d", who, kind);
    if (p->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: objects belong to different contexts", who);
    fd_pyramid_require_single(p, who);
    if (p->all.empty()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the pyramid has not been updated with an image", who);
    if (n < 0 || n > FD_HIST_SAMPLES_MAX) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the sample count %d is outside 0..%d", who, n, (int)FD_HIST_SAMPLES_MAX);
    SamplesPlan pl;
    std::memset(&pl.ep, 0, sizeof(pl.ep));
    pl.ehog = kind == FD_SAMPLES_EHOG;
    if (pl.ehog) {
        pl.ep = *(const fd_ehog_patch_params*)params;
        pl.hp = ehog_patch_hist_params(&pl.ep);
        if (p->filter_kind != FD_LAYER_GRADBIN)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "ExtendedHogFilter features need a gradient bin image (FD_LAYER_GRADBIN)");
    } else {
        pl.hp = *(const fd_hist_params*)params;
    }
    const int ch = hist_check_layers(p, &pl.hp);
    pl.hd = make_histdev(&pl.hp, ch);
    pl.F = pl.ehog ? pl.hd.rows * pl.hd.cols * (pl.ep.bins + (pl.ep.signed_and_unsigned ? pl.ep.bins / 2 : 0) + 4) : pl.hd.F;
    if (hist_lds_bytes(pl.hd) > 160 * 1024) FD_THROW(FD_ERR_INVALID_ARGUMENT, "histogram feature vector too long for the LDS (%d floats)", pl.hd.F);
    return pl;
}

// resolves the samples, uploads the windows of the valid ones (pinned staging + one async copy; `extraPinned` bytes behind the list
// in the same pinned block are the caller's, at the returned address) and fills sampleOf; valid (may be NULL): one byte per sample
void* samples_upload(fd_ctx* ctx, const fd_pyramid* p, const SamplesPlan& pl, int n, const int32_t* xywh, uint8_t* valid, HogScratch& S,
                     std::vector<int>& sampleOf, size_t extraPinnedPerValid) {
    return fd_samples_upload(ctx, p, pl.hp.patch_w, pl.hp.patch_h, n, xywh, valid, S.list, sampleOf, extraPinnedPerValid);
}

// the features of the nv windows listed at dlist (device), [nv][pl.F] floats on the device: queued on ctx->stream
const float* samples_features(fd_ctx* ctx, const fd_pyramid* p, const SamplesPlan& pl, const int32_t* dlist, int64_t nv, HogScratch& S) {
    fd_pyramid_wait(p, ctx->stream);
    FdWinTable wt;
    fd_win_table_list(p, dlist, nv, /*filtered=*/true, wt);
    launch_hist_features(ctx, p->arena.as<uint8_t>(), wt, pl.hd, S);
    if (!pl.ehog) return S.feat.as<float>();
    const int64_t total = nv * pl.F;   // S.feat: the raw cell histograms, as in fd_ehog_patch_batch
    S.xx.reserve(sizeof(float) * (size_t)total);
    hipLaunchKernelGGL(k_ehog_patch_desc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, S.feat.as<float>(), total, pl.hd.rows,
                       pl.hd.cols, pl.ep.bins, pl.ep.signed_and_unsigned ? 1 : 0, pl.ep.alpha, S.xx.as<float>());
    HIP_CHECK(hipGetLastError());
    return S.xx.as<float>();
}

void extract_samples(fd_ctx* ctx, fd_pyramid* p, int kind, const void* params, int n, const int32_t* xywh, uint8_t* valid, float* features,
                     const char* who) {
    if (!ctx || !p || !params || (n > 0 && !xywh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
    const SamplesPlan pl = samples_plan(ctx, p, kind, params, n, who);
    if (n == 0) return;
    if (features) std::memset(features, 0, sizeof(float) * (size_t)n * pl.F);
    HogScratch& S = scratch(ctx);
    std::vector<int> sampleOf;
    samples_upload(ctx, p, pl, n, xywh, valid, S, sampleOf, 0);
    const int64_t nv = (int64_t)sampleOf.size();
    if (nv == 0 || !features) return;
    fd_samples_rows_to_host(ctx, samples_features(ctx, p, pl, S.list.as<int32_t>(), nv, S), pl.F, nv, n, sampleOf, features);
}

}  // namespace

// the resident particle set's bridge (fd_internal.hpp): the argument rules of fd_hist_svm_evaluate_samples, then its kernels on the list
void fd_hist_samples_score_list(fd_ctx* ctx, const fd_pyramid* p, int kind, const void* params, const fd_svm* svm, const char* who, const int32_t* dlist,
                                int n, double* dscore, int* patch_w, int* patch_h) {
    const SamplesPlan pl = samples_plan(ctx, p, kind, params, n, who);
    fd_samples_require_f32_svm(svm, pl.F, who);
    *patch_w = pl.hp.patch_w; *patch_h = pl.hp.patch_h;
    if (!dlist || n == 0) return;
    fd_svm_generic_launch(ctx, svm, samples_features(ctx, p, pl, dlist, n, scratch(ctx)), nullptr, (int64_t)pl.F * 4, n, dscore);
}

// the same list's feature rows, left on the device ([n][*row_length] floats, the handle's scratch: they hold until its next call), for
// fd_particles_state_examples_pyramid; with dlist NULL the argument rules of fd_hist_extract_samples / fd_ehog_extract_samples alone
const float* fd_hist_samples_features_list(fd_ctx* ctx, const fd_pyramid* p, int kind, const void* params, const char* who, const int32_t* dlist, int n,
                                           int* row_length, int* patch_w, int* patch_h) {
    const SamplesPlan pl = samples_plan(ctx, p, kind, params, n, who);
    *row_length = pl.F; *patch_w = pl.hp.patch_w; *patch_h = pl.hp.patch_h;
    if (!dlist || n == 0) return nullptr;
    return samples_features(ctx, p, pl, dlist, n, scratch(ctx));
}

extern "C" {

int fd_sample_windows(int n_layers, const int32_t* layer_index, const double* layer_scale, const int32_t* layer_w, const int32_t* layer_h,
                      double incremental_scale, int patch_w, int patch_h, int n, const int32_t* xywh, int32_t* windows) {
    if (n_layers < 0 || n < 0 || patch_w < 1 || patch_h < 1 || !(incremental_scale > 0 && incremental_scale < 1)) return FD_ERR_INVALID_ARGUMENT;
    if (n_layers > 0 && (!layer_index || !layer_scale || !layer_w || !layer_h)) return FD_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!xywh || !windows)) return FD_ERR_INVALID_ARGUMENT;
    for (int l = 0; l < n_layers; ++l)   // consecutive pyramid indices, as ImagePyramid keeps them
        if (layer_index[l] != layer_index[0] + l || layer_w[l] < 1 || layer_h[l] < 1 || !(layer_scale[l] > 0)) return FD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) {
        const int32_t* s = xywh + 4 * (size_t)i;
        FdSampleWindow w;
        const bool ok = fd_sample_window(n_layers, n_layers ? layer_index[0] : 0, incremental_scale, patch_w, patch_h, s[0], s[1], s[2], s[3],
                                         [&](int pos, double& scale, int& lw, int& lh) { scale = layer_scale[pos]; lw = layer_w[pos]; lh = layer_h[pos]; }, w);
        int32_t* o = windows + 4 * (size_t)i;
        o[0] = ok ? w.layer : -1; o[1] = ok ? w.bx : 0; o[2] = ok ? w.by : 0; o[3] = ok ? 1 : 0;
    }
    return FD_OK;
}

int fd_pyramid_sample_windows(const fd_pyramid* p, int patch_w, int patch_h, int n, const int32_t* xywh, int32_t* windows) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p || n < 0 || patch_w < 1 || patch_h < 1 || (n > 0 && (!xywh || !windows)))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_sample_windows: bad argument");
        if (p->all.empty()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_sample_windows: the pyramid has not been updated with an image");
        for (int i = 0; i < n; ++i) {
            FdSampleWindow w;
            const bool ok = pyramid_sample_window(p, patch_w, patch_h, xywh + 4 * (size_t)i, w);
            int32_t* o = windows + 4 * (size_t)i;
            o[0] = ok ? w.layer : -1; o[1] = ok ? w.bx : 0; o[2] = ok ? w.by : 0; o[3] = ok ? 1 : 0;
        }
    });
}

int fd_hist_samples_limits(int* max_samples) {
    if (!max_samples) return FD_ERR_INVALID_ARGUMENT;
    *max_samples = FD_HIST_SAMPLES_MAX;
    return FD_OK;
}

int fd_hist_extract_samples(fd_ctx* ctx, fd_pyramid* p, const fd_hist_params* hp, int n, const int32_t* xywh, uint8_t* valid, float* features) {
    return fd_guard(ctx, [&] { extract_samples(ctx, p, FD_SAMPLES_HIST, hp, n, xywh, valid, features, "fd_hist_extract_samples"); });
}

int fd_ehog_extract_samples(fd_ctx* ctx, fd_pyramid* p, const fd_ehog_patch_params* ep, int n, const int32_t* xywh, uint8_t* valid, float* features) {
    return fd_guard(ctx, [&] { extract_samples(ctx, p, FD_SAMPLES_EHOG, ep, n, xywh, valid, features, "fd_ehog_extract_samples"); });
}

int fd_hist_svm_evaluate_samples_distance(fd_ctx* ctx, fd_pyramid* p, int kind, const void* params, const fd_svm* svm, int n, const int32_t* xywh,
                                          uint8_t* target, double* weight, double* distance) {
    return fd_guard(ctx, [&] {
        const char* who = "fd_hist_svm_evaluate_samples";
        if (!ctx || !p || !params || !svm || (n > 0 && (!xywh || !target || !weight))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        const SamplesPlan pl = samples_plan(ctx, p, kind, params, n, who);
        fd_samples_require_f32_svm(svm, pl.F, who);
        if (n == 0) return;
        fd_samples_clear(n, target, weight, distance);
        HogScratch& S = scratch(ctx);
        std::vector<int> sampleOf;
        double* hdist = (double*)samples_upload(ctx, p, pl, n, xywh, nullptr, S, sampleOf, sizeof(double));
        const int64_t nv = (int64_t)sampleOf.size();
        if (nv == 0) return;
        fd_samples_svm_tail(ctx, svm, samples_features(ctx, p, pl, S.list.as<int32_t>(), nv, S), pl.F, nv, S.dist, hdist, sampleOf.data(), nullptr, target, weight, distance);
    });
}

int fd_hist_svm_evaluate_samples(fd_ctx* ctx, fd_pyramid* p, int kind, const void* params, const fd_svm* svm, int n, const int32_t* xywh,
                                 uint8_t* target, double* weight) {
    return fd_hist_svm_evaluate_samples_distance(ctx, p, kind, params, svm, n, xywh, target, weight, nullptr);
}

}  // extern "C"
