// featuredetection_amd/csrc/ehog_patch.hpp -- imageprocessing::ExtendedHogFilter(binCount, cellWidth, cellHeight, interpolate,
// signedAndUnsigned, alpha) (ExtendedHogFilter.cpp:54-209) as a patch filter on bin-image patches.  Included by hog.hip: the cell
// histograms are HistogramFilter::createCellHistograms, i.e. k_hist_features run as a SpatialHistogramFilter with 1 x 1 blocks
// and no normalisation; k_ehog_patch_desc turns them into the extended HOG descriptors of createDescriptors (:63-209), with the
// arithmetic of k_fhog_desc (fp32 1.f / sqrtf, double 0.5 / 0.2357 factors) and the output order [bins][unsigned halves][4].
#pragma once

namespace {

// one thread per output value; the nine neighbouring cell energies are recomputed from the raw histograms (bins fp32 additions
// each, in bin order as :74-80 / :149-153 accumulate them)
__global__ __launch_bounds__(256) void k_ehog_patch_desc(const float* __restrict__ cells, int64_t total, int R, int C, int B, int sau, float alpha,
                                                         float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int half = B / 2, ub = sau ? half : 0, D = B + ub + 4;
    const int per = R * C * D;
    const int64_t i = e / per;
    const int rem = (int)(e - i * per);
    const int cell = rem / D, f = rem - cell * D;
    const int r = cell / C, c = cell - r * C;
    const float* H = cells + (size_t)i * R * C * B;
    auto E = [&](int rr, int cc) {
        const float* h = H + (size_t)(rr * C + cc) * B;
        float en = 0.f;
        if (sau) {
            for (int b = 0; b < half; ++b) { const float s = h[b] + h[b + half]; en = en + s * s; }
        } else {
            for (int b = 0; b < B; ++b) en = en + h[b] * h[b];
        }
        return en;
    };
    const int pr = max(r - 1, 0), nr = min(r + 1, R - 1), pc = max(c - 1, 0), nc = min(c + 1, C - 1);
    const float e00 = E(pr, pc), e01 = E(pr, c), e02 = E(pr, nc), e10 = E(r, pc), e11 = E(r, c), e12 = E(r, nc), e20 = E(nr, pc), e21 = E(nr, c),
                e22 = E(nr, nc);
    const float eps = 1e-4f;
    float n[4];
    n[0] = 1.f / sqrtf(e00 + e01 + e10 + e11 + eps);
    n[1] = 1.f / sqrtf(e01 + e02 + e11 + e12 + eps);
    n[2] = 1.f / sqrtf(e10 + e11 + e20 + e21 + eps);
    n[3] = 1.f / sqrtf(e11 + e12 + e21 + e22 + eps);
    const float* h = H + (size_t)cell * B;
    float v;
    if (f < B) {
        const float x = h[f];
        v = (float)(0.5 * (double)(fminf(alpha, x * n[0]) + fminf(alpha, x * n[1]) + fminf(alpha, x * n[2]) + fminf(alpha, x * n[3])));
    } else if (f < B + ub) {
        const int b = f - B;
        const float x = h[b] + h[b + half];
        v = (float)(0.5 * (double)(fminf(alpha, x * n[0]) + fminf(alpha, x * n[1]) + fminf(alpha, x * n[2]) + fminf(alpha, x * n[3])));
    } else {
        const float ni = n[f - B - ub];
        float t = 0.f;
        for (int b = 0; b < B; ++b) t = t + fminf(alpha, h[b] * ni);
        v = (float)(0.2357 * (double)t);
    }
    out[e] = v;
}

// the constructor's checks (:24-31,42-51) and the histogram stage's own limits; returns the SpatialHistogramFilter stand-in
fd_hist_params ehog_patch_hist_params(const fd_ehog_patch_params* ep) {
    if (!ep) FD_THROW(FD_ERR_INVALID_ARGUMENT, "NULL extended HOG parameters");
    if (ep->bins <= 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "ExtendedHogFilter: binCount must be greater than zero");
    if (ep->cell_w <= 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "ExtendedHogFilter: cellWidth must be greater than zero");
    if (ep->cell_h < 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "ExtendedHogFilter: cellHeight must be greater than zero");
    if (ep->signed_and_unsigned && ep->bins % 2 != 0)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "ExtendedHogFilter: the bin size must be even for signed and unsigned gradients to be combined");
    if (!(ep->alpha > 0)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "ExtendedHogFilter: alpha must be greater than zero");
    fd_hist_params hp;
    std::memset(&hp, 0, sizeof(hp));
    hp.patch_w = ep->patch_w; hp.patch_h = ep->patch_h; hp.step_x = hp.step_y = 1;
    hp.kind = FD_HIST_SPATIAL; hp.bins = ep->bins; hp.cell_size = ep->cell_w; hp.cell_h = ep->cell_h; hp.block_size = 1;
    hp.interpolate = ep->interpolate; hp.normalization = 0;
    return hp;
}

}  // namespace

extern "C" {

int fd_ehog_feature_length(const fd_ehog_patch_params* ep, int channels) {
    try {
        if (channels != 1 && channels != 2 && channels != 4) return -1;
        const fd_hist_params hp = ehog_patch_hist_params(ep);
        const HistDev hd = make_histdev(&hp, channels);   // throws for a grid with zero rows or columns
        return hd.rows * hd.cols * (ep->bins + (ep->signed_and_unsigned ? ep->bins / 2 : 0) + 4);
    } catch (...) { return -1; }
}

int fd_ehog_patch_batch(fd_ctx* ctx, const uint8_t* bin_patches, int64_t n, int channels, const fd_ehog_patch_params* ep, float* out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !ep || n < 0 || (n > 0 && (!bin_patches || !out))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_patch_batch: bad argument");
        if (channels != 1 && channels != 2 && channels != 4) FD_THROW(FD_ERR_INVALID_ARGUMENT, "HistogramFilter: the image must have one, two or four channels");
        const fd_hist_params hp = ehog_patch_hist_params(ep);
        const HistDev hd = make_histdev(&hp, channels);
        if (n == 0) return;
        if (n > (int64_t)1 << 24) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_patch_batch: too many patches in one call");
        HogScratch& S = scratch(ctx);
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t bytes = (size_t)n * hp.patch_w * hp.patch_h * channels;
        S.patchIn.reserve(bytes);
        HIP_CHECK(hipMemcpyAsync(S.patchIn.p, bin_patches, bytes, hipMemcpyHostToDevice, ctx->stream));
        // S.feat: n x rows * cols * bins raw cell histograms
        launch_hist_features(ctx, S.patchIn.as<uint8_t>(), fd_win_table_column(n, hp.patch_w, hp.patch_h), hd, S);
        const int D = ep->bins + (ep->signed_and_unsigned ? ep->bins / 2 : 0) + 4;
        const int64_t total = n * hd.rows * hd.cols * D;
        S.xx.reserve(sizeof(float) * (size_t)total);
        hipLaunchKernelGGL(k_ehog_patch_desc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, S.feat.as<float>(), total, hd.rows, hd.cols,
                           ep->bins, ep->signed_and_unsigned ? 1 : 0, ep->alpha, S.xx.as<float>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, S.xx.p, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"
