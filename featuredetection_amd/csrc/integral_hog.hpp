// featuredetection_amd/csrc/integral_hog.hpp -- the integral HOG family ("ihog" / "iehog" of AdaptiveTracking.cpp:189-213) on sampled
// windows of an integral image: IntegralGradientFilter(rows, cols) -> GradientBinningFilter -> {HogFilter | SpatialHistogramFilter |
// PyramidHogFilter | SpatialPyramidHistogramFilter | ExtendedHogFilter} in one launch.  Included by hog.hip behind hist_samples.hpp:
// the gradient points are integral_geo.hpp's (the functions of k_grad_patches / k_surf), the binning is the look-up table of
// k_gradbin, the histogram stage is hist_patch_features (the body of k_hist_features), the ehog descriptors are k_ehog_patch_desc's.
// The CV_8UC2 gradient patch and the bin image exist in LDS only.  The handle and the entry points are integral.hip's.
#pragma once
#include "integral_geo.hpp"

namespace {

// One wavefront per sample, four samples per workgroup (the shape of k_surf).  LDS: the four interpolation tables once per
// workgroup, then per wavefront [bin-image patch, patchBytes | vector area, ldsFloats floats rounded up to 16 bytes].
// E: bytes per look-up entry == channels of the bin image (2: bin + weight, 4: two bins + weights).
size_t integral_hog_tab_bytes(const HistDev& d) {
    return (sizeof(HistCache) * (size_t)(d.pw + d.ph) + sizeof(int32_t) * (size_t)(d.rows + d.cols) + 15) & ~(size_t)15;
}
size_t integral_hog_wave_bytes(const HistDev& d) { return (size_t)d.patchBytes + ((sizeof(float) * (size_t)d.ldsFloats + 15) & ~(size_t)15); }
size_t integral_hog_lds_bytes(const HistDev& d) { return integral_hog_tab_bytes(d) + 4 * integral_hog_wave_bytes(d); }
constexpr size_t INTEGRAL_HOG_LDS_BUDGET = 160 * 1024;   // LDS of one gfx950 workgroup

template <int E>
__global__ __launch_bounds__(256) void k_integral_hog(const int32_t* __restrict__ img, int W, int H, const uint8_t* __restrict__ lut, HistDev hd,
                                                      HistTables tab, size_t tabBytes, size_t waveBytes, const int32_t* __restrict__ xywh, int n,
                                                      float* __restrict__ feat, uint8_t* __restrict__ valid) {
    using namespace fd_integral_geo;
    extern __shared__ __attribute__((aligned(16))) unsigned char ihogLds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rows = hd.ph, cols = hd.pw, points = rows * cols;
    HistCache* rowCache = (HistCache*)ihogLds;            // [ph]
    HistCache* colCache = rowCache + rows;                // [pw]
    int32_t* rowRange = (int32_t*)(colCache + cols);      // [hd.rows]
    int32_t* colRange = rowRange + hd.rows;               // [hd.cols]
    if (hd.interpolate) {
        for (int i = threadIdx.x; i < rows; i += 256) rowCache[i] = tab.rowCache[i];
        for (int i = threadIdx.x; i < cols; i += 256) colCache[i] = tab.colCache[i];
        for (int i = threadIdx.x; i < hd.rows; i += 256) rowRange[i] = tab.rowRange[i];
        for (int i = threadIdx.x; i < hd.cols; i += 256) colRange[i] = tab.colRange[i];
    }
    __syncthreads();
    unsigned char* patch = ihogLds + tabBytes + (size_t)wave * waveBytes;   // [rows][cols][E]
    float* vec = (float*)(patch + hd.patchBytes);                            // [ldsFloats]
    const size_t S = (size_t)W + 1;
    for (int s = blockIdx.x * 4 + wave; s < n; s += gridDim.x * 4) {
        const SampleGeo g = sample_geo(xywh, s, W, H);
        const GradGeo q = grad_geo(g, rows, cols, W, H);
        if (lane == 0) valid[s] = q.ok ? 1 : 0;
        float* __restrict__ out = feat + (size_t)s * hd.F;
        if (!q.ok) {   // nothing of the sample is read
            for (int i = lane; i < hd.F; i += 64) out[i] = 0.f;
            continue;
        }
        const int32_t* __restrict__ base = img + (size_t)g.py0 * S + g.px0;
        for (int i = lane; i < points; i += 64) {
            const uchar2 gr = grad_point(base, S, q, i / cols, i % cols);
            const uint32_t idx = (uint32_t)gr.x | ((uint32_t)gr.y << 8);   // GradientBinningFilter.cpp:62-93, k_gradbin's index
            if (E == 2) reinterpret_cast<uint16_t*>(patch)[i] = reinterpret_cast<const uint16_t*>(lut)[idx];
            else reinterpret_cast<uint32_t*>(patch)[i] = reinterpret_cast<const uint32_t*>(lut)[idx];
        }
        const float* res = hist_patch_features(hd, patch, rowCache, colCache, rowRange, colRange, vec, lane);
        for (int i = lane; i < hd.F; i += 64) out[i] = res[i];
        wave_sync();
    }
}

struct IntegralHogPlan {
    HistDev hd;
    bool ehog = false;
    fd_ehog_patch_params ep;
    int F = 0;   // floats per sample
};
IntegralHogPlan integral_hog_plan(const fd_integral_hog_params* p) {
    static const char* const who = "fd_integral_hog_params";
    if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL", who);
    if (p->grad_rows < 2 || p->grad_cols < 2 || p->grad_rows > 64 || p->grad_cols > 64)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: IntegralGradientFilter rows and cols must be within 2..64 for the fused call (got %d x %d)", who, p->grad_rows,
                 p->grad_cols);
    if (p->bins < 1 || p->bins > 255) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientBinningFilter: bins must be in 1..255");
    if (p->kind != FD_SAMPLES_HIST && p->kind != FD_SAMPLES_EHOG) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown feature kind %d", who, p->kind);
    IntegralHogPlan pl;
    std::memset(&pl.ep, 0, sizeof(pl.ep));
    pl.ehog = p->kind == FD_SAMPLES_EHOG;
    const int pw = pl.ehog ? p->ehog.patch_w : p->hist.patch_w, ph = pl.ehog ? p->ehog.patch_h : p->hist.patch_h;
    const int fbins = pl.ehog ? p->ehog.bins : p->hist.bins;
    if (pw != p->grad_cols || ph != p->grad_rows)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the histogram filter's patch (%d x %d) differs from the gradient grid (%d x %d)", who, pw, ph, p->grad_cols,
                 p->grad_rows);
    if (fbins != p->bins) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the histogram filter's bins (%d) differ from the binning filter's (%d)", who, fbins, p->bins);
    const int ch = p->interpolate_bins ? 4 : 2;
    fd_hist_params hp;
    if (pl.ehog) {
        pl.ep = p->ehog;
        hp = ehog_patch_hist_params(&pl.ep);
    } else {
        hp = p->hist;
    }
    pl.hd = make_histdev(&hp, ch);
    pl.F = pl.ehog ? pl.hd.rows * pl.hd.cols * (pl.ep.bins + (pl.ep.signed_and_unsigned ? pl.ep.bins / 2 : 0) + 4) : pl.hd.F;
    const size_t lds = integral_hog_lds_bytes(pl.hd);
    if (lds > INTEGRAL_HOG_LDS_BUDGET)
        FD_THROW(FD_ERR_INVALID_ARGUMENT,
                 "fd_integral_extract_hog: this configuration needs %zu bytes of LDS per workgroup, more than the %zu there are (use the stand-alone "
                 "calls fd_integral_gradient_patches, fd_gradient_binning_image, fd_hist_patch_batch / fd_ehog_patch_batch)",
                 lds, INTEGRAL_HOG_LDS_BUDGET);
    return pl;
}

}  // namespace

int fd_integral_hog_check(const fd_integral_hog_params* p) { return integral_hog_plan(p).F; }

void fd_integral_hog_launch(fd_ctx* ctx, const fd_integral_hog_params* p, const int32_t* img, int W, int H, const uint8_t* lut, const int32_t* xywh,
                            int n, DevBuf& raw, DevBuf& feat, uint8_t* valid) {
    const IntegralHogPlan pl = integral_hog_plan(p);
    const HistDev& hd = pl.hd;
    HIP_CHECK(hipSetDevice(ctx->device));
    HistTables tb;
    hist_tables(ctx, scratch(ctx), hd, tb);
    feat.reserve(sizeof(float) * (size_t)n * pl.F);
    float* rows = feat.as<float>();
    if (pl.ehog) {   // raw cell histograms first, as fd_ehog_patch_batch
        raw.reserve(sizeof(float) * (size_t)n * hd.F);
        rows = raw.as<float>();
    }
    const size_t tabBytes = integral_hog_tab_bytes(hd), waveBytes = integral_hog_wave_bytes(hd), lds = integral_hog_lds_bytes(hd);
    const int grid = std::max(1, std::min((n + 3) / 4, ctx->num_cus * 32));
    if (hd.ch == 4) {
        static uint64_t allowed4 = 0;
        fd_allow_lds(ctx, (const void*)k_integral_hog<4>, (int)INTEGRAL_HOG_LDS_BUDGET, allowed4);
        hipLaunchKernelGGL(k_integral_hog<4>, dim3(grid), dim3(256), lds, ctx->stream, img, W, H, lut, hd, tb, tabBytes, waveBytes, xywh, n, rows, valid);
    } else {
        static uint64_t allowed2 = 0;
        fd_allow_lds(ctx, (const void*)k_integral_hog<2>, (int)INTEGRAL_HOG_LDS_BUDGET, allowed2);
        hipLaunchKernelGGL(k_integral_hog<2>, dim3(grid), dim3(256), lds, ctx->stream, img, W, H, lut, hd, tb, tabBytes, waveBytes, xywh, n, rows, valid);
    }
    HIP_CHECK(hipGetLastError());
    if (pl.ehog) {
        const int64_t total = (int64_t)n * pl.F;
        hipLaunchKernelGGL(k_ehog_patch_desc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, raw.as<float>(), total, hd.rows, hd.cols,
                           pl.ep.bins, pl.ep.signed_and_unsigned ? 1 : 0, pl.ep.alpha, feat.as<float>());
        HIP_CHECK(hipGetLastError());
    }
}

extern "C" int fd_integral_hog_feature_length(const fd_integral_hog_params* p) {
    try { return integral_hog_plan(p).F; } catch (...) { return -1; }
}
