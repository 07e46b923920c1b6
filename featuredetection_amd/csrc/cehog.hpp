// featuredetection_amd/csrc/cehog.hpp -- imageprocessing::CompleteExtendedHogFilter(cellSize, binCount, signedGradients,
// unsignedGradients, interpolateBins, interpolateCells, alpha) (CompleteExtendedHogFilter.cpp:19-303) on gray images / gray
// pyramid layers.  Included by fhog.hip: the filter is the 2014 form of the FHOG descriptor and runs through the same kernels
// over the same layer table (k_fhog_grad, k_fhog_hist, k_fhog_desc); what differs is data and geometry, not the kernels' arithmetic:
//   - the gradient look-up table is built in double (:31-58) and indexed dx * 512 + dy; the device copy is transposed on the host,
//     so k_fhog_grad's dy * 512 + dx finds the same entry;
//   - the central differences clamp at the area the cells cover (:126-127), so a layer enters the table with w = cols * cell,
//     h = rows * cell and its real stride;
//   - the cell interpolation table is computed in double (createLut, :72-103): k_fhog_coeff<double> instead of <float>;
//   - signed-only / unsigned-only histograms have no unsigned section (D = binCount + 4), and the energy of an unsigned-only
//     histogram runs over its bins (:181-190): FhogParamsDev::plainEnergy.
// The normalisers and the 0.5 / 0.2357 factors are read as k_fhog_desc reads them (fp32 1.f / sqrtf, double factors).  DESIGN.md 4.5.
#pragma once

namespace {

struct CehogBin { int32_t index1, index2; float weight1, weight2; };   // BinInformation, CompleteExtendedHogFilter.hpp:68-73

// the constructor's rules (:23-26) and this backend's limit (the LDS histogram of k_fhog_hist holds FHOG_MAX_SBINS bins); NULL when the
// parameters are valid, the message otherwise -- one statement of the rules for the host-only calls and the device calls
inline const char* cehog_params_error(const fd_cehog_params& fp) {
    if (fp.cell_size < 1) return "CompleteExtendedHogFilter: cellSize must be bigger than zero";
    if (!fp.signed_gradients && !fp.unsigned_gradients) return "CompleteExtendedHogFilter: signedGradients or unsignedGradients has to be true";
    if (fp.signed_gradients && fp.unsigned_gradients && fp.bin_count % 2 != 0)
        return "CompleteExtendedHogFilter: if both signed and unsigned gradients should be used, the bin count has to be even";
    if (fp.bin_count < 1 || fp.bin_count > FHOG_MAX_SBINS) return "CompleteExtendedHogFilter: binCount must be within 1..36 on this backend";
    return nullptr;
}
inline bool cehog_params_ok(const fd_cehog_params& fp) { return cehog_params_error(fp) == nullptr; }

inline int cehog_channels(const fd_cehog_params& fp) {
    return fp.bin_count + (fp.signed_gradients && fp.unsigned_gradients ? fp.bin_count / 2 : 0) + 4;
}

// the constructor's loop (:31-58), entry dx * 512 + dy, host libm like the reference
void cehog_build_lut(const fd_cehog_params& fp, std::vector<CehogBin>& lut) {
    lut.resize((size_t)512 * 512);
    const int binCount = fp.bin_count;
    for (int x = 0; x < 512; ++x) {
        const double gradientX = static_cast<double>(x - 256) / (2. * 255.);
        for (int y = 0; y < 512; ++y) {
            const double gradientY = static_cast<double>(y - 256) / (2. * 255.);
            double direction = std::atan2(gradientY, gradientX);
            const double magnitude = std::sqrt(gradientX * gradientX + gradientY * gradientY);
            double binIndex;
            if (fp.signed_gradients) {
                direction += M_PI;
                binIndex = direction * binCount / (2 * M_PI);
            } else {
                if (direction < 0) direction += M_PI;
                binIndex = direction * binCount / M_PI;
            }
            CehogBin b;
            if (fp.interpolate_bins) {
                b.index1 = static_cast<int>(std::floor(binIndex)) % binCount;
                b.index2 = static_cast<int>(std::ceil(binIndex)) % binCount;
                b.weight2 = static_cast<float>(magnitude * (binIndex - std::floor(binIndex)));
                b.weight1 = static_cast<float>(magnitude - b.weight2);
            } else {
                b.index1 = static_cast<int>(std::round(binIndex)) % binCount;
                b.weight1 = static_cast<float>(magnitude);
                b.index2 = b.index1;
                b.weight2 = 0;
            }
            lut[(size_t)512 * x + y] = b;
        }
    }
}

struct CehogScratch {
    DevBuf lut;
    fd_cehog_params lutFor;
    bool lutValid = false;
};

void check_cehog_params(const fd_cehog_params& fp) {
    if (const char* what = cehog_params_error(fp)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s (binCount %d, cellSize %d)", what, fp.bin_count, fp.cell_size);
}

// device copy of the look-up table in k_fhog_grad's layout: entry dy * 512 + dx, bin indices as bytes (binCount <= 36)
void cehog_upload_lut(fd_ctx* ctx, CehogScratch& C, const fd_cehog_params& fp) {
    if (C.lutValid && C.lutFor.bin_count == fp.bin_count && !C.lutFor.signed_gradients == !fp.signed_gradients &&
        !C.lutFor.interpolate_bins == !fp.interpolate_bins)
        return;
    std::vector<CehogBin> host;
    cehog_build_lut(fp, host);
    std::vector<FhogLutEntry> lut((size_t)512 * 512);
    std::memset(lut.data(), 0, sizeof(FhogLutEntry) * lut.size());
    for (int dx = 0; dx < 512; ++dx)
        for (int dy = 0; dy < 512; ++dy) {
            const CehogBin& b = host[(size_t)512 * dx + dy];
            FhogLutEntry& e = lut[(size_t)512 * dy + dx];
            e.bins.index1 = (uint8_t)b.index1; e.bins.index2 = (uint8_t)b.index2;
            e.bins.weight1 = b.weight1; e.bins.weight2 = b.weight2;
        }
    C.lut.reserve(sizeof(FhogLutEntry) * lut.size());
    HIP_CHECK(hipMemcpy(C.lut.p, lut.data(), sizeof(FhogLutEntry) * lut.size(), hipMemcpyHostToDevice));
    C.lutFor = fp;
    C.lutValid = true;
}

// a gray image / layer as an entry of the layer table: the filter never looks past the pixels its cells cover (:111-127)
FhogLayerDev cehog_layer(const uint8_t* dimg, int w, int h, int stride, int cell) {
    return layer_entry(dimg, (w / cell) * cell, (h / cell) * cell, stride, 1);
}

// descriptors of every layer of the table at dlayers (entries made by cehog_layer, laid out by layout_layers) into descOut
// (t.cells * channels floats on the device; NULL: S.desc)
void run_cehog(fd_ctx* ctx, FhogScratch& S, const FhogLayerDev* dlayers, int nLayers, const FhogLayoutTotals& t, const fd_cehog_params& fp,
               float* descOut = nullptr) {
    check_cehog_params(fp);
    CehogScratch& C = fd_scratch<CehogScratch>(ctx);
    cehog_upload_lut(ctx, C, fp);
    const bool both = fp.signed_gradients && fp.unsigned_gradients;
    FhogParamsDev d;
    std::memset(&d, 0, sizeof(d));
    d.cell = fp.cell_size; d.sbins = fp.bin_count; d.D = cehog_channels(fp);
    d.interpBins = fp.interpolate_bins != 0; d.interpCells = fp.interpolate_cells != 0; d.alpha = fp.alpha;
    // energy (:168-191): over the unsigned halves when the gradients are signed, over the bins otherwise
    FhogParamsDev dh = d;
    dh.ubins = fp.bin_count / 2;
    dh.plainEnergy = fp.signed_gradients ? 0 : 1;
    // descriptor (:194-302): [bins][unsigned halves, when both][4 energies]
    FhogParamsDev dd = d;
    dd.ubins = both ? fp.bin_count / 2 : 0;
    run_cell_filter(ctx, S, dlayers, nLayers, t, FhogRun{C.lut.as<FhogLutEntry>(), true, dh, dd}, descOut);
}

// one gray image already on the device; an image smaller than a cell is an error
void run_cehog_single(fd_ctx* ctx, FhogScratch& S, const uint8_t* dimg, int w, int h, int stride, const fd_cehog_params& fp, int& rows, int& cols) {
    check_cehog_params(fp);
    FhogLayerDev L = cehog_layer(dimg, w, h, stride, fp.cell_size);
    const FhogLayoutTotals t = single_layer_table(ctx, S.layers, L, fp.cell_size);
    rows = L.rows; cols = L.cols;
    if (rows == 0 || cols == 0)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "CompleteExtendedHogFilter: the image (%d x %d) is smaller than a cell (%d)", w, h, fp.cell_size);
    run_cehog(ctx, S, S.layers.as<FhogLayerDev>(), 1, t, fp);
}

}  // namespace

extern "C" {

int fd_cehog_size(const fd_cehog_params* fp, int width, int height, int* rows, int* cols, int* channels) {
    if (!fp || !cehog_params_ok(*fp) || width < 0 || height < 0) return FD_ERR_INVALID_ARGUMENT;
    if (rows) *rows = height / fp->cell_size;
    if (cols) *cols = width / fp->cell_size;
    if (channels) *channels = cehog_channels(*fp);
    return FD_OK;
}

int fd_cehog_gradient_lut(const fd_cehog_params* fp, int32_t* index1, int32_t* index2, float* weight1, float* weight2) {
    if (!fp || !cehog_params_ok(*fp)) return FD_ERR_INVALID_ARGUMENT;
    std::vector<CehogBin> lut;
    cehog_build_lut(*fp, lut);
    for (size_t i = 0; i < lut.size(); ++i) {
        if (index1) index1[i] = lut[i].index1;
        if (index2) index2[i] = lut[i].index2;
        if (weight1) weight1[i] = lut[i].weight1;
        if (weight2) weight2[i] = lut[i].weight2;
    }
    return FD_OK;
}

int fd_cehog_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, const fd_cehog_params* fp, float* out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !gray || !fp || !out || width < 1 || height < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_cehog_image: bad argument");
        check_cehog_params(*fp);
        if (width < fp->cell_size || height < fp->cell_size)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "CompleteExtendedHogFilter: the image (%d x %d) is smaller than a cell (%d)", width, height, fp->cell_size);
        HIP_CHECK(hipSetDevice(ctx->device));
        FhogScratch& S = scratch(ctx);
        const size_t bytes = (size_t)width * height;
        S.img.reserve(bytes);
        HIP_CHECK(hipMemcpyAsync(S.img.p, gray, bytes, hipMemcpyHostToDevice, ctx->stream));
        int rows, cols;
        run_cehog_single(ctx, S, S.img.as<uint8_t>(), width, height, width, *fp, rows, cols);
        HIP_CHECK(hipMemcpyAsync(out, S.desc.p, sizeof(float) * (size_t)rows * cols * cehog_channels(*fp), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_pyramid_cehog_layer(fd_ctx* ctx, fd_pyramid* p, int layer, const fd_cehog_params* fp, float* out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !p || !fp || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_cehog_layer: NULL argument");
        if (p->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
        if (p->filter_kind != FD_LAYER_NONE) FD_THROW(FD_ERR_INVALID_ARGUMENT, "CompleteExtendedHogFilter needs a gray pyramid (no layer filter)");
        fd_pyramid_require_single(p, "fd_pyramid_cehog_layer");
        if (layer < 0 || layer >= (int)p->kept.size()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "no such pyramid layer: %d", layer);
        HIP_CHECK(hipSetDevice(ctx->device));
        const HostLayer& L = p->all[p->kept[layer]];
        FhogScratch& S = scratch(ctx);
        int rows, cols;
        run_cehog_single(ctx, S, p->arena.as<uint8_t>() + L.gray_off, L.w, L.h, L.w, *fp, rows, cols);
        HIP_CHECK(hipMemcpyAsync(out, S.desc.p, sizeof(float) * (size_t)rows * cols * cehog_channels(*fp), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"
