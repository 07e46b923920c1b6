// featuredetection_amd/csrc/ehog_tracker.hpp -- the per-frame work of condensation::ExtendedHogBasedMeasurementModel
// (ExtendedHogBasedMeasurementModel.cpp:97-213,243-265,434-456,621-652) behind one handle, fd_ehog_tracker: the gray pyramid of
// ExtendedHogFeatureExtractor::createPyramid (ExtendedHogFeatureExtractor.cpp:32-41,76-84), its feature pyramid
// (CompleteExtendedHogFilter on every layer, cehog.hpp), the heat pyramid (ConvolutionFilter.cpp:27-43 with the linear SVM's
// weight vector), the samples of CellBasedPyramidFeatureExtractor / DirectPyramidFeatureExtractor, the patches of
// ExtendedHogFeatureExtractor::extract (:95-143), the heat peak and the local maxima.  Included by fhog.hip.  DESIGN.md 4.5.
//
// Kernels: k_ehog_heat (all layers, LPC lanes per cell, lane == channel), k_ehog_gather_scores / k_ehog_gather_cells (samples),
// k_ehog_patch (one wavefront per sample, patch and histograms in LDS), k_ehog_peak (one workgroup), k_ehog_maxima.
// The sample -> (layer, position) arithmetic is double log / round / cvRound: ehog_cell_window / ehog_patch_window below hold it once
// for the host entry points (libm's log per sample, the window list uploaded) and for the resident particle set of condensation.hip
// (k_ehog_resolve: the layer of a width read from a table the host built with the same libm expression).
#pragma once

struct EhogLayerPx { int32_t w, h; };   // real size of a gray layer (the layer table holds the area its cells cover)

struct EhogPatchGeom {
    int32_t cell, rows, cols;           // inner cells
    int32_t PR, PC, PW, PH;             // cells and pixels of the patch, border included
    int32_t bins, half, D, interpBins, interpCells, plainEnergy, both;
    float alpha;
    int32_t oHist, oEnergy, oDesc, oPart, bytes;   // LDS carve-up (bytes)
};

struct EhogPeakDev { float score; int32_t layer, row, col, found; };
struct EhogMaxDev { int32_t pos; float score; };

struct fd_ehog_tracker {
    fd_ctx* ctx;
    fd_ehog_tracker_params prm;
    int D = 0;
    double minScale = 0, maxScale = 0;
    fd_pyramid* pyr = nullptr;
    int pyrW = 0, pyrH = 0;
    std::vector<FhogLayerDev> layerTable;
    std::vector<EhogLayerPx> layerPx;
    std::vector<fd_ehog_layer> layers;
    FhogLayoutTotals layout;
    void* arenaAt = nullptr;
    DevBuf dlayers, dlayerPx, desc, heat, dweights, list, outScore, outFeat, outValid, peak, maxima, counter, patchCoeff;
    DevBuf dplan, dcellLayerOf, dpatchLayerOf;   // the layer plan and the width -> layer tables of k_ehog_resolve (rebuilt with the plan)
    int cellLayerOfLen = 0, patchLayerOfLen = 0;
    std::vector<float> weights;
    float bias = 0.f;
    bool hasSvm = false, updated = false;
    EhogPatchGeom geom;
    ~fd_ehog_tracker() { if (pyr) fd_pyramid_destroy(pyr); }
};

namespace {

constexpr size_t EHOG_PATCH_LDS_BUDGET = 64 * 1024;

// what turns a sample into a window, apart from the layers
struct EhogWindowRule {
    int32_t cellCols, cellRows, cell, PW, PH, nLayers, firstLayer, octaveLayers;
    double widthFactor, heightFactor;
};

__host__ __device__ inline int ehog_cvround(double v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (int)rint(v);   // half to even, like lrint in the default rounding mode
#else
    return fd_cvRound(v);
#endif
}

// the position in the layer list a width maps to: lround(log(patchWidth / width) / log(inc)) - first index (ImagePyramid.cpp:300-310)
inline long ehog_layer_of_width(const EhogWindowRule& R, int patchWidth, int width) {
    const double inc = std::pow(0.5, 1. / R.octaveLayers);
    const double scaleFactor = static_cast<double>(patchWidth) / static_cast<double>(width);
    return std::lround(std::log(scaleFactor) / std::log(inc)) - R.firstLayer;
}

// samples -> windows in cells (CellBasedPyramidFeatureExtractor.cpp:58-69, DirectPyramidFeatureExtractor.cpp:67-73,133-143):
// {layer, bx, by, valid}.  layerOf(width) is ehog_layer_of_width or a table of it.
template <class LayerOf>
__host__ __device__ inline int4 ehog_cell_window(const EhogWindowRule& R, const fd_ehog_layer* layers, int x, int y, int width, int height, LayerOf layerOf) {
    if (width <= 0 || height <= 0) return make_int4(0, 0, 0, 0);
    const long realIndex = layerOf(width);
    if (realIndex < 0 || realIndex >= (long)R.nLayers) return make_int4(0, 0, 0, 0);
    const fd_ehog_layer& L = layers[realIndex];
    const int bx = ehog_cvround((x - width / 2) * L.scale / R.cell), by = ehog_cvround((y - height / 2) * L.scale / R.cell);
    if (bx < 0 || by < 0 || bx + R.cellCols > L.cols || by + R.cellRows > L.rows) return make_int4(0, 0, 0, 0);
    return make_int4((int)realIndex, bx, by, 1);
}

// ExtendedHogFeatureExtractor::extract (:95-107): widened size, layer, bounds in the layer's pixels.  layerOf takes the widened width.
template <class LayerOf>
__host__ __device__ inline int4 ehog_patch_window(const EhogWindowRule& R, const fd_ehog_layer* layers, int x, int y, int sampleWidth, int sampleHeight,
                                                  LayerOf layerOf) {
    if (sampleWidth <= 0 || sampleHeight <= 0) return make_int4(0, 0, 0, 0);
    const int width = static_cast<int>(round(R.widthFactor * sampleWidth));
    const int height = static_cast<int>(round(R.heightFactor * sampleHeight));
    const long realIndex = layerOf(width);
    if (realIndex < 0 || realIndex >= (long)R.nLayers) return make_int4(0, 0, 0, 0);
    const fd_ehog_layer& L = layers[realIndex];
    const int bx = ehog_cvround((x - width / 2) * L.scale), by = ehog_cvround((y - height / 2) * L.scale);
    if (bx < -R.cell || bx + R.PW > L.width + R.cell || by < -R.cell || by + R.PH > L.height + R.cell) return make_int4(0, 0, 0, 0);
    return make_int4((int)realIndex, bx, by, 1);
}

// the samples of a resident particle set (x, y, size; height = cvRound(aspect * size), Sample.hpp:127-129) -> the window list of
// k_ehog_gather_scores (patches 0) or k_ehog_patch (patches 1).  layerOf[w]: the layer position of width w, -1 for none; widths from
// tableLen on have none.
__global__ __launch_bounds__(256) void k_ehog_resolve(EhogWindowRule R, const fd_ehog_layer* __restrict__ layers, const int16_t* __restrict__ layerOf,
                                                      int tableLen, const int32_t* __restrict__ x, const int32_t* __restrict__ y,
                                                      const int32_t* __restrict__ size, int n, double aspect, int patches, int4* __restrict__ list,
                                                      uint8_t* __restrict__ valid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int width = size[i], height = ehog_cvround(aspect * width);
    auto look = [&](int w) -> long { return w > 0 && w < tableLen ? (long)layerOf[w] : -1L; };
    const int4 w = patches ? ehog_patch_window(R, layers, x[i], y[i], width, height, look) : ehog_cell_window(R, layers, x[i], y[i], width, height, look);
    list[i] = w;
    valid[i] = (uint8_t)w.w;
}

// the float scores of k_ehog_gather_scores as the doubles a Sample keeps
__global__ __launch_bounds__(256) void k_ehog_widen_scores(const float* __restrict__ in, int n, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

// ConvolutionFilter::applyTo (ConvolutionFilter.cpp:27-43) with anchor (-1, -1) = the kernel centre (kw / 2, kh / 2),
// BORDER_CONSTANT 0 and delta = -bias, on every feature layer of the table: heat(y, x) = delta + sum over channels c of
// [sum over the kernel, row-major, of K[ky][kx][c] * F[y + ky - kh / 2][x + kx - kw / 2][c]], fp32, the per-channel sums added in
// channel order -- the arithmetic of k_fhog_score.  Taps outside the layer are skipped (they would add K * 0).  LPC lanes own a
// cell, lane == channel: a tap is one coalesced read of the cell's descriptor; the channel sums meet in LDS.
template <int LPC>
__global__ __launch_bounds__(256) void k_ehog_heat(const FhogLayerDev* __restrict__ layers, int nLayers, int totalCells, const float* __restrict__ descAll,
                                                   int D, const float* __restrict__ K, int kh, int kw, float delta, float* __restrict__ heat) {
    __shared__ float part[256 / LPC][LPC + 1];
    const int grp = threadIdx.x / LPC, c = threadIdx.x & (LPC - 1);
    const int g = blockIdx.x * (256 / LPC) + grp;
    const bool valid = g < totalCells;
    float sacc = 0.f;
    if (valid && c < D) {
        const FhogLayerDev L = layers[layer_of<&FhogLayerDev::cellBase>(layers, nLayers, g)];
        const int cellId = g - L.cellBase;
        const int y = cellId / L.cols, x = cellId - y * L.cols;
        const int ay = kh / 2, ax = kw / 2;
        const float* F = descAll + (size_t)L.cellBase * D + c;
        for (int ky = 0; ky < kh; ++ky) {
            const int yy = y + ky - ay;
            if (yy < 0 || yy >= L.rows) continue;
            for (int kx = 0; kx < kw; ++kx) {
                const int xx = x + kx - ax;
                if (xx < 0 || xx >= L.cols) continue;
                sacc = sacc + K[(size_t)(ky * kw + kx) * D + c] * F[((size_t)yy * L.cols + xx) * D];
            }
        }
    }
    part[grp][c] = sacc;
    __syncthreads();
    if (valid && c == 0) {
        float s = delta;
        for (int ch = 0; ch < D; ++ch) s = s + part[grp][ch];
        heat[g] = s;
    }
}

// sample windows {layer, bx, by, valid} (cells): the heat value at the kernel centre of the window
__global__ __launch_bounds__(256) void k_ehog_gather_scores(const FhogLayerDev* __restrict__ layers, const int4* __restrict__ list, int n, int cr, int cc,
                                                            const float* __restrict__ heat, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 w = list[i];
    float s = 0.f;
    if (w.w) {
        const FhogLayerDev L = layers[w.x];
        s = heat[(size_t)L.cellBase + (size_t)(w.z + cr) * L.cols + w.y + cc];
    }
    out[i] = s;
}

// the same windows: rows x cols x D descriptors each, one thread per value (a window row is one run of cols * D floats)
__global__ __launch_bounds__(256) void k_ehog_gather_cells(const FhogLayerDev* __restrict__ layers, const int4* __restrict__ list, int64_t total, int rows,
                                                           int cols, int D, const float* __restrict__ descAll, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int run = cols * D, per = rows * run;
    const int i = (int)(e / per), rem = (int)(e - (int64_t)i * per);
    const int r = rem / run, q = rem - r * run;
    const int4 w = list[i];
    float v = 0.f;
    if (w.w) {
        const FhogLayerDev L = layers[w.x];
        v = descAll[((size_t)L.cellBase + (size_t)(w.z + r) * L.cols + w.y) * D + q];
    }
    out[e] = v;
}

// getHeatPeak (ExtendedHogBasedMeasurementModel.cpp:434-456): the positions a layer offers are rows [cr, rows + cr - cellRows) x
// columns [cc, cols + cc - cellCols) (vh x vw in the layer table, posBase = their rank in layer / row / column order); strict >
// in that order, so the first of equal scores wins.  One workgroup: every thread walks its positions in rank order, the
// workgroup then keeps the larger score and, among equal ones, the smaller rank.
__global__ __launch_bounds__(1024) void k_ehog_peak(const FhogLayerDev* __restrict__ layers, int nLayers, int cr, int cc, const float* __restrict__ heat,
                                                    EhogPeakDev* __restrict__ out) {
    __shared__ float bs[1024];
    __shared__ int br[1024];
    float best = 0.f;
    int rank = -1, bl = 0, brow = 0, bcol = 0;
    for (int l = 0; l < nLayers; ++l) {
        const FhogLayerDev L = layers[l];
        const int np = L.vw * L.vh;
        for (int i = threadIdx.x; i < np; i += 1024) {
            const int y = i / L.vw, x = i - y * L.vw;
            const float s = heat[(size_t)L.cellBase + (size_t)(y + cr) * L.cols + x + cc];
            // the reference starts from the lowest double: every float but -inf (and NaN) beats it
            if (rank < 0 ? s > -INFINITY : s > best) { best = s; rank = L.posBase + i; bl = l; brow = y + cr; bcol = x + cc; }
        }
    }
    bs[threadIdx.x] = best;
    br[threadIdx.x] = rank;
    __syncthreads();
    for (int step = 512; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
            const float os = bs[threadIdx.x + step], ms = bs[threadIdx.x];
            const int orank = br[threadIdx.x + step], mr = br[threadIdx.x];
            if (orank >= 0 && (mr < 0 || os > ms || (os == ms && orank < mr))) { bs[threadIdx.x] = os; br[threadIdx.x] = orank; }
        }
        __syncthreads();
    }
    const int win = br[0];
    if (threadIdx.x == 0 && win < 0) *out = EhogPeakDev{0.f, 0, 0, 0, 0};
    if (rank >= 0 && rank == win) *out = EhogPeakDev{best, bl, brow, bcol, 1};
}

// the scan of createGoodNegativeExamples (:621-652): score > threshold and >= all eight neighbours.  One thread per offered
// position; hits are appended in any order with their rank, the host sorts by rank (= scan order).  out has room for every
// position.
__global__ __launch_bounds__(256) void k_ehog_maxima(const FhogLayerDev* __restrict__ layers, int nLayers, int totalPos, int cr, int cc, float threshold,
                                                     const float* __restrict__ heat, EhogMaxDev* __restrict__ out, unsigned int* __restrict__ count) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= totalPos) return;
    const FhogLayerDev L = layers[layer_of<&FhogLayerDev::posBase>(layers, nLayers, p)];
    const int i = p - L.posBase;
    const int y = i / L.vw + cr, x = i - (i / L.vw) * L.vw + cc;
    const float* row = heat + (size_t)L.cellBase + (size_t)y * L.cols;
    const float* prev = row - L.cols;
    const float* next = row + L.cols;
    const float s = row[x];
    if (s > threshold && s >= row[x - 1] && s >= row[x + 1] && s >= prev[x - 1] && s >= prev[x] && s >= prev[x + 1] && s >= next[x - 1] &&
        s >= next[x] && s >= next[x + 1]) {
        const unsigned int slot = atomicAdd(count, 1u);
        out[slot] = EhogMaxDev{p, s};
    }
}

// ExtendedHogFeatureExtractor::extract (ExtendedHogFeatureExtractor.cpp:95-143) for one sample per wavefront.  The patch of
// (cols + 2) * cell x (rows + 2) * cell gray pixels is copied into LDS through the mirrored indices of createIndexLut; the filter
// of cehog.hpp then runs on it as on an image: lane == cell, a lane walks the pixels that feed its cell in the reference's scan
// order (the walk and the effective-weight reading of k_fhog_hist), gradients straight from the LDS patch and the look-up table;
// histograms and energies stay in LDS; the inner cells' descriptors are computed as k_fhog_desc computes them, written out, and
// kept in LDS for the decision value: -bias + dot(features, w), the double sum in element order of cv::Mat::dot.
__global__ __launch_bounds__(64) void k_ehog_patch(const FhogLayerDev* __restrict__ layers, const EhogLayerPx* __restrict__ layerPx,
                                                   const int4* __restrict__ list, EhogPatchGeom G, const FhogLutEntry* __restrict__ lut,
                                                   const FhogCoeffDev* __restrict__ coeff, const float* __restrict__ K, double negBias,
                                                   float* __restrict__ features, double* __restrict__ score) {
    extern __shared__ __align__(16) unsigned char ehogLds[];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int4 w = list[i];
    const int nInner = G.rows * G.cols * G.D;
    if (!w.w) {   // no patch: zeros
        for (int e = lane; e < nInner; e += 64) features[(size_t)i * nInner + e] = 0.f;
        if (score && lane == 0) score[i] = 0.0;
        return;
    }
    uint8_t* pix = ehogLds;
    float* hist = (float*)(ehogLds + G.oHist);       // [bin][cell]
    float* energy = (float*)(ehogLds + G.oEnergy);   // [cell]
    float* desc = (float*)(ehogLds + G.oDesc);       // [inner cell][D]
    const FhogLayerDev L = layers[w.x];
    const EhogLayerPx S = layerPx[w.x];
    const int nCells = G.PR * G.PC;
    for (int e = lane; e < G.PW * G.PH; e += 64) {
        const int py = e / G.PW, px = e - py * G.PW;
        int iy = w.z + py, ix = w.y + px;
        if (iy < 0) iy = -iy - 1; else if (iy >= S.h) iy = 2 * S.h - iy - 1;
        if (ix < 0) ix = -ix - 1; else if (ix >= S.w) ix = 2 * S.w - ix - 1;
        pix[e] = L.img[(size_t)iy * L.stride + ix];
    }
    for (int e = lane; e < nCells * G.bins; e += 64) hist[e] = 0.f;
    __syncthreads();
    const FhogCoeffDev* __restrict__ rowCoeff = coeff;
    const FhogCoeffDev* __restrict__ colCoeff = coeff + G.PH;
    const int cs = G.cell;
    const int off = G.interpCells ? (cs + 1) / 2 + 1 : 0, box = cs + 2 * off;
    for (int cell = lane; cell < nCells; cell += 64) {
        const int r = cell / G.PC, c = cell - r * G.PC;
        auto bin = [&](int b) -> float& { return hist[b * nCells + cell]; };
        for (int ii = 0; ii < box; ++ii) {
            const int y = r * cs - off + ii;
            if (y < 0 || y >= G.PH) continue;
            const FhogCoeffDev rc = rowCoeff[y];
            const bool r1 = rc.index1 == r, r2 = G.interpCells && rc.index2 == r;
            if (!r1 && !r2) continue;
            const float wr = (r1 ? rc.weight1 : 0.f) + (r2 ? rc.weight2 : 0.f);
            const uint8_t* up = pix + max(y - 1, 0) * G.PW;
            const uint8_t* dn = pix + min(y + 1, G.PH - 1) * G.PW;
            const uint8_t* mid = pix + y * G.PW;
            for (int jj = 0; jj < box; ++jj) {
                const int x = c * cs - off + jj;
                if (x < 0 || x >= G.PW) continue;
                const FhogCoeffDev cc = colCoeff[(x % cs) * G.PC + x / cs];
                const bool c1 = cc.index1 == c, c2 = G.interpCells && cc.index2 == c;
                if (!c1 && !c2) continue;
                const int dx = (int)mid[min(x + 1, G.PW - 1)] - (int)mid[max(x - 1, 0)] + 256;
                const int dy = (int)dn[x] - (int)up[x] + 256;
                const FhogLut e = lut[dy * 512 + dx].bins;
                fhog_vote(bin, e, wr, cc, c1, c2, G.interpCells, G.interpBins);
            }
        }
        energy[cell] = fhog_energy(bin, G.bins, G.half, G.plainEnergy);
    }
    __syncthreads();
    const int ub = G.both ? G.half : 0;
    for (int e = lane; e < nInner; e += 64) {
        const int ic = e / G.D, f = e - ic * G.D;
        const int r = ic / G.cols + 1, c = ic - (ic / G.cols) * G.cols + 1;
        const int cell = r * G.PC + c;
        float n[4];
        fhog_normalizers([&](int rr, int cc) { return energy[rr * G.PC + cc]; }, r, c, G.PR, G.PC, n);
        const float out = fhog_feature([&](int b) { return hist[b * nCells + cell]; }, n, f, G.bins, ub, G.alpha);
        desc[e] = out;
        features[(size_t)i * nInner + e] = out;
    }
    if (!score) return;
    __syncthreads();
    if (lane == 0) {
        double dot = 0.0;
        for (int e = 0; e < nInner; ++e) dot = dot + (double)desc[e] * (double)K[e];
        score[i] = negBias + dot;
    }
}

EhogPatchGeom ehog_patch_geom(const fd_ehog_tracker_params& P) {
    EhogPatchGeom G;
    std::memset(&G, 0, sizeof(G));
    const fd_cehog_params& f = P.filter;
    G.cell = f.cell_size; G.rows = P.cell_rows; G.cols = P.cell_cols;
    G.PR = (int32_t)std::min<int64_t>((int64_t)P.cell_rows + 2, INT32_MAX); G.PC = (int32_t)std::min<int64_t>((int64_t)P.cell_cols + 2, INT32_MAX);
    G.PW = (int32_t)std::min<int64_t>((int64_t)G.PC * G.cell, INT32_MAX); G.PH = (int32_t)std::min<int64_t>((int64_t)G.PR * G.cell, INT32_MAX);
    G.bins = f.bin_count; G.half = f.bin_count / 2; G.D = cehog_channels(f);
    G.interpBins = f.interpolate_bins != 0; G.interpCells = f.interpolate_cells != 0;
    G.plainEnergy = f.signed_gradients ? 0 : 1; G.both = f.signed_gradients && f.unsigned_gradients;
    G.alpha = f.alpha;
    // the carve-up in 64 bits: cells and cell size are ints, so every product below stays far from overflow; the offsets are only used
    // by launches, which need the total to fit the LDS budget
    auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
    const int64_t PR = (int64_t)P.cell_rows + 2, PC = (int64_t)P.cell_cols + 2, cell = f.cell_size;
    int64_t o = up(PR * cell * PC * cell);
    G.oHist = (int32_t)std::min<int64_t>(o, INT32_MAX); o = up(o + PR * PC * G.bins * 4);
    G.oEnergy = (int32_t)std::min<int64_t>(o, INT32_MAX); o = up(o + PR * PC * 4);
    G.oDesc = (int32_t)std::min<int64_t>(o, INT32_MAX); o = up(o + (int64_t)P.cell_rows * P.cell_cols * G.D * 4);
    G.oPart = (int32_t)std::min<int64_t>(o, INT32_MAX);
    G.bytes = (int32_t)std::min<int64_t>(o, INT32_MAX);
    return G;
}

// ExtendedHogFeatureExtractor::createPyramid (:32-41) with the arguments of its constructor (:76-84)
bool ehog_pyramid_limits(const fd_ehog_tracker_params& P, double& minScale, double& maxScale) {
    const int cols = P.cell_cols, cell = P.filter.cell_size;
    if (cols < 1 || P.cell_rows < 1 || cell < 1 || P.octave_layer_count < 1 || P.min_width < 1 || P.max_width < P.min_width) return false;
    if ((int64_t)(cols + 2) * P.max_width > INT32_MAX || (int64_t)(cols + 2) * cell > INT32_MAX) return false;
    const int width = (cols + 2) * cell, minWidth = (cols + 2) * P.min_width / cols, maxWidth = (cols + 2) * P.max_width / cols;
    if (minWidth < 1 || maxWidth < 1) return false;
    const double incrementalScaleFactor = std::pow(0.5, 1. / P.octave_layer_count);
    double minScaleFactor = static_cast<double>(width) / maxWidth;
    double maxScaleFactor = static_cast<double>(width) / minWidth;
    const int maxLayerIndex = fd_cvRound(std::log(minScaleFactor) / std::log(incrementalScaleFactor));
    const int minLayerIndex = fd_cvRound(std::log(maxScaleFactor) / std::log(incrementalScaleFactor));
    maxScale = std::pow(incrementalScaleFactor, minLayerIndex);
    minScale = std::pow(incrementalScaleFactor, maxLayerIndex);
    return true;
}

// the layers ImagePyramid::createLayers(const Mat&) (ImagePyramid.cpp:170-198) keeps for a width x height image, index order;
// the feature and heat pyramids built on it keep every one of them (scale <= 1)
void ehog_plan_layers(const fd_ehog_tracker_params& P, double minScale, double maxScale, int width, int height, std::vector<fd_ehog_layer>& out) {
    out.clear();
    const int n = P.octave_layer_count, cell = P.filter.cell_size;
    const double inc = std::pow(0.5, 1. / n);
    for (int i = 0; i < n; ++i) {
        double scaleFactor = std::pow(inc, (double)i);
        int pw = fd_cvRound(width * scaleFactor), ph = fd_cvRound(height * scaleFactor);
        if (pw < 1 || ph < 1) break;
        if (scaleFactor <= maxScale && scaleFactor >= minScale) out.push_back(fd_ehog_layer{i, pw, ph, ph / cell, pw / cell, 0, scaleFactor});
        scaleFactor *= 0.5;
        for (int j = 1; scaleFactor >= minScale && pw > 1; ++j, scaleFactor *= 0.5) {
            pw = (pw + 1) / 2;
            ph = (ph + 1) / 2;
            if (scaleFactor <= maxScale) out.push_back(fd_ehog_layer{i + j * n, pw, ph, ph / cell, pw / cell, 0, scaleFactor});
        }
    }
    std::sort(out.begin(), out.end(), [](const fd_ehog_layer& a, const fd_ehog_layer& b) { return a.index < b.index; });
}

void ehog_check_params(const fd_ehog_tracker_params& P) {
    check_cehog_params(P.filter);
    double a, b;
    if (!ehog_pyramid_limits(P, a, b))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker: cell_cols, cell_rows, octave_layer_count and min_width must be positive and max_width >= min_width");
}

void ehog_launch_heat(fd_ctx* ctx, fd_ehog_tracker* t) {
    if (t->layout.cells == 0) return;
    const fd_ehog_tracker_params& P = t->prm;
    const int D = t->D, nLayers = (int)t->layerTable.size(), cells = t->layout.cells;
    t->heat.reserve(sizeof(float) * (size_t)cells);
    const float delta = -t->bias;
#define EHOG_HEAT(LPC)                                                                                                                        \
    hipLaunchKernelGGL(k_ehog_heat<LPC>, dim3((unsigned)(((int64_t)cells * LPC + 255) / 256)), dim3(256), 0, ctx->stream, t->dlayers.as<FhogLayerDev>(), \
                       nLayers, cells, t->desc.as<float>(), D, t->dweights.as<float>(), P.cell_rows, P.cell_cols, delta, t->heat.as<float>())
    if (D <= 16) EHOG_HEAT(16);
    else if (D <= 32) EHOG_HEAT(32);
    else EHOG_HEAT(64);
#undef EHOG_HEAT
    HIP_CHECK(hipGetLastError());
}

fd_ehog_tracker* ehog_checked(fd_ctx* ctx, fd_ehog_tracker* t, const char* what, bool needUpdate, bool needSvm) {
    if (!ctx || !t) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (t->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
    if (needUpdate && !t->updated) FD_THROW(FD_ERR_RUNTIME, "%s: the tracker has not been updated with an image", what);
    if (needSvm && !t->hasSvm) FD_THROW(FD_ERR_RUNTIME, "%s: no SVM has been set (fd_ehog_tracker_set_svm)", what);
    HIP_CHECK(hipSetDevice(ctx->device));
    return t;
}

// samples -> windows in cells (CellBasedPyramidFeatureExtractor.cpp:58-69, DirectPyramidFeatureExtractor.cpp:67-73,133-143,
// ImagePyramid.cpp:300-310) through ehog_cell_window; uploads the list, fills valid
EhogWindowRule ehog_window_rule(const fd_ehog_tracker* t) {
    const fd_ehog_tracker_params& P = t->prm;
    EhogWindowRule R;
    R.cellCols = P.cell_cols; R.cellRows = P.cell_rows; R.cell = P.filter.cell_size; R.PW = t->geom.PW; R.PH = t->geom.PH;
    R.nLayers = (int32_t)t->layers.size(); R.firstLayer = t->layers.empty() ? 0 : t->layers[0].index; R.octaveLayers = P.octave_layer_count;
    R.widthFactor = static_cast<double>(P.cell_cols + 2) / P.cell_cols; R.heightFactor = static_cast<double>(P.cell_rows + 2) / P.cell_rows;
    return R;
}

void ehog_sample_windows(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* xywh, uint8_t* valid) {
    const EhogWindowRule R = ehog_window_rule(t);
    int4* pin = (int4*)fd_pinned(ctx, sizeof(int4) * (size_t)std::max(n, 1));
    for (int i = 0; i < n; ++i) {
        pin[i] = ehog_cell_window(R, t->layers.data(), xywh[4 * i], xywh[4 * i + 1], xywh[4 * i + 2], xywh[4 * i + 3],
                                  [&](int width) { return ehog_layer_of_width(R, R.cellCols * R.cell, width); });
        valid[i] = (uint8_t)pin[i].w;
    }
    t->list.reserve(sizeof(int4) * (size_t)std::max(n, 1));
    if (n) HIP_CHECK(hipMemcpyAsync(t->list.p, pin, sizeof(int4) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
}

// width -> layer for every width that can have one: a width twice the one that maps onto the last layer is an octave past it
void ehog_build_layer_tables(fd_ehog_tracker* t) {
    const EhogWindowRule R = ehog_window_rule(t);
    auto build = [&](int patchWidth, DevBuf& dev, int& len) {
        const double last = t->layers.empty() ? 1.0 : t->layers.back().scale;
        len = (int)std::min<double>(2.0 * patchWidth / last + 2.0, (double)(1 << 20));
        std::vector<int16_t> table((size_t)len, (int16_t)-1);
        for (int w = 1; w < len; ++w) {
            const long realIndex = ehog_layer_of_width(R, patchWidth, w);
            if (realIndex >= 0 && realIndex < (long)R.nLayers) table[w] = (int16_t)realIndex;
        }
        dev.reserve(sizeof(int16_t) * table.size());
        HIP_CHECK(hipMemcpy(dev.p, table.data(), sizeof(int16_t) * table.size(), hipMemcpyHostToDevice));
    };
    build(R.cellCols * R.cell, t->dcellLayerOf, t->cellLayerOfLen);
    build(R.PW, t->dpatchLayerOf, t->patchLayerOfLen);
    t->dplan.reserve(sizeof(fd_ehog_layer) * std::max<size_t>(t->layers.size(), 1));
    if (!t->layers.empty()) HIP_CHECK(hipMemcpy(t->dplan.p, t->layers.data(), sizeof(fd_ehog_layer) * t->layers.size(), hipMemcpyHostToDevice));
}

void ehog_check_patch_lds(const fd_ehog_tracker* t, const char* what) {
    const fd_ehog_tracker_params& P = t->prm;
    const int ldsBytes = fd_ehog_tracker_patch_lds_bytes(&P);
    if (ldsBytes < 0 || (size_t)ldsBytes > EHOG_PATCH_LDS_BUDGET)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: a patch of %d x %d cells of %d pixels with %d bins needs %d bytes of LDS, a workgroup has %zu", what,
                 P.cell_cols + 2, P.cell_rows + 2, P.filter.cell_size, P.filter.bin_count, ldsBytes, EHOG_PATCH_LDS_BUDGET);
}

}  // namespace

extern "C" {

int fd_ehog_tracker_plan_layers(const fd_ehog_tracker_params* prm, int width, int height, fd_ehog_layer* out, int cap, int* n) {
    if (!prm || !n || width < 1 || height < 1 || cap < 0 || (cap > 0 && !out) || !cehog_params_ok(prm->filter)) return FD_ERR_INVALID_ARGUMENT;
    double minScale, maxScale;
    if (!ehog_pyramid_limits(*prm, minScale, maxScale)) return FD_ERR_INVALID_ARGUMENT;
    std::vector<fd_ehog_layer> layers;
    ehog_plan_layers(*prm, minScale, maxScale, width, height, layers);
    *n = (int)layers.size();
    if (layers.size() < 2) return FD_ERR_RUNTIME;   // ImagePyramid::estimateLambdas of the feature pyramid (ImagePyramid.cpp:238-239)
    if (*n > cap) return FD_ERR_CAPACITY;
    std::copy(layers.begin(), layers.end(), out);
    return FD_OK;
}

int fd_ehog_tracker_create(fd_ctx* ctx, const fd_ehog_tracker_params* prm, fd_ehog_tracker** out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !prm || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_create: NULL argument");
        ehog_check_params(*prm);
        HIP_CHECK(hipSetDevice(ctx->device));
        std::unique_ptr<fd_ehog_tracker> t(new fd_ehog_tracker());
        t->ctx = ctx;
        t->prm = *prm;
        t->D = cehog_channels(prm->filter);
        ehog_pyramid_limits(*prm, t->minScale, t->maxScale);
        t->geom = ehog_patch_geom(*prm);
        if ((size_t)t->geom.bytes <= EHOG_PATCH_LDS_BUDGET) {   // createLut (CompleteExtendedHogFilter.cpp:72-103) of the patch's rows and columns
            const EhogPatchGeom& G = t->geom;                   // in k_fhog_coeff's storage order: it depends on the geometry alone
            std::vector<FhogCoeffDev> coeff((size_t)G.PH + G.PW);
            for (int y = 0; y < G.PH; ++y) coeff[y] = cell_coeff<double>(y, G.cell, G.PR, G.interpCells);
            for (int x = 0; x < G.PW; ++x) coeff[(size_t)G.PH + (x % G.cell) * G.PC + x / G.cell] = cell_coeff<double>(x, G.cell, G.PC, G.interpCells);
            t->patchCoeff.reserve(sizeof(FhogCoeffDev) * coeff.size());
            HIP_CHECK(hipMemcpy(t->patchCoeff.p, coeff.data(), sizeof(FhogCoeffDev) * coeff.size(), hipMemcpyHostToDevice));
        }
        int rc = fd_pyramid_create(ctx, prm->octave_layer_count, t->minScale, t->maxScale, &t->pyr);
        if (rc != FD_OK) throw FdError{rc, ctx->error};
        *out = t.release();
    });
}

void fd_ehog_tracker_destroy(fd_ehog_tracker* t) { delete t; }

int fd_ehog_tracker_update(fd_ctx* ctx, fd_ehog_tracker* t, const uint8_t* image, int width, int height, int channels, int is_device) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_update", false, false);
        if (!image) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_update: NULL argument");
        const fd_ehog_tracker_params& P = t->prm;
        t->updated = false;
        int rc = fd_pyramid_update(t->pyr, image, width, height, channels, is_device);
        if (rc != FD_OK) throw FdError{rc, ctx->error};
        fd_pyramid* p = t->pyr;
        if (p->kept.size() < 2)   // the feature pyramid is built on the gray one: ImagePyramid::estimateLambdas (ImagePyramid.cpp:238-239)
            FD_THROW(FD_ERR_RUNTIME, "ImagePyramid: at least two pyramid layers are needed to estimate the lambdas");
        FhogScratch& S = scratch(ctx);
        if (t->layerTable.empty() || t->arenaAt != p->arena.p || t->pyrW != width || t->pyrH != height) {
            std::vector<fd_ehog_layer> plan;
            ehog_plan_layers(P, t->minScale, t->maxScale, width, height, plan);
            bool same = plan.size() == p->kept.size();
            for (size_t li = 0; same && li < plan.size(); ++li) {
                const HostLayer& H = p->all[p->kept[li]];
                same = plan[li].index == H.index && plan[li].width == H.w && plan[li].height == H.h && plan[li].scale == H.scale;
            }
            if (!same) FD_THROW(FD_ERR_RUNTIME, "fd_ehog_tracker_update: the layer plan and the gray pyramid disagree");
            t->layers = plan;
            t->layerTable.clear();
            t->layerPx.clear();
            const int cr = P.cell_rows / 2, cc = P.cell_cols / 2;
            for (size_t li = 0; li < plan.size(); ++li) {
                const HostLayer& H = p->all[p->kept[li]];
                FhogLayerDev T = cehog_layer(p->arena.as<uint8_t>() + H.gray_off, H.w, H.h, H.w, P.filter.cell_size);
                // positions getHeatPeak offers: rows [cr, rows + cr - cell_rows), columns [cc, cols + cc - cell_cols)
                T.vh = std::max(plan[li].rows + cr - P.cell_rows - cr, 0);
                T.vw = std::max(plan[li].cols + cc - P.cell_cols - cc, 0);
                if (T.vw == 0 || T.vh == 0) T.vw = T.vh = 0;
                t->layerTable.push_back(T);
                t->layerPx.push_back(EhogLayerPx{H.w, H.h});
            }
            t->layout = layout_layers(t->layerTable, P.filter.cell_size);
            t->dlayers.reserve(sizeof(FhogLayerDev) * t->layerTable.size());
            HIP_CHECK(hipMemcpy(t->dlayers.p, t->layerTable.data(), sizeof(FhogLayerDev) * t->layerTable.size(), hipMemcpyHostToDevice));
            t->dlayerPx.reserve(sizeof(EhogLayerPx) * t->layerPx.size());
            HIP_CHECK(hipMemcpy(t->dlayerPx.p, t->layerPx.data(), sizeof(EhogLayerPx) * t->layerPx.size(), hipMemcpyHostToDevice));
            ehog_build_layer_tables(t);
            t->arenaAt = p->arena.p;
            t->pyrW = width; t->pyrH = height;
        }
        t->desc.reserve(sizeof(float) * (size_t)std::max(t->layout.cells, 1) * t->D);
        run_cehog(ctx, S, t->dlayers.as<FhogLayerDev>(), (int)t->layerTable.size(), t->layout, P.filter, t->desc.as<float>());
        if (t->hasSvm) ehog_launch_heat(ctx, t);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        t->updated = true;
    });
}

int fd_ehog_tracker_set_svm(fd_ctx* ctx, fd_ehog_tracker* t, const float* weights, float bias) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_set_svm", false, false);
        if (!weights) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_set_svm: NULL argument");
        const size_t nw = (size_t)t->prm.cell_rows * t->prm.cell_cols * t->D;
        t->weights.assign(weights, weights + nw);
        t->bias = bias;
        t->dweights.reserve(sizeof(float) * nw);
        HIP_CHECK(hipMemcpyAsync(t->dweights.p, t->weights.data(), sizeof(float) * nw, hipMemcpyHostToDevice, ctx->stream));
        t->hasSvm = true;
        if (t->updated) ehog_launch_heat(ctx, t);   // the heat pyramid of the current frame (initialize: :339-341)
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_ehog_tracker_train_svm(fd_ctx* ctx, fd_ehog_tracker* t, const float* x, int n_pos, int n_neg, const fd_svm_train_params* params,
                              fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_train_svm", false, false);
        if (!x || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_train_svm: NULL argument");
        const size_t nw = (size_t)t->prm.cell_rows * t->prm.cell_cols * t->D;
        t->dweights.reserve(sizeof(float) * nw);
        fd_svm_train_problem pr = {};
        pr.x = x;
        pr.n_pos = n_pos;
        pr.n_neg = n_neg;
        pr.d = (int)nw;
        fd_svm_train_run(ctx, {"fd_ehog_tracker_train_svm", false, t->dweights.as<float>()}, 1, &pr, params, info);   // k_svm_finish writes dweights
        t->bias = (float)info->rho;
        t->hasSvm = true;
        if (t->updated) ehog_launch_heat(ctx, t);
        t->weights.resize(nw);
        HIP_CHECK(hipMemcpyAsync(t->weights.data(), t->dweights.p, sizeof(float) * nw, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_ehog_tracker_get_svm(fd_ctx* ctx, fd_ehog_tracker* t, float* weights, float* bias) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_get_svm", false, true);
        if (!weights || !bias) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_get_svm: NULL argument");
        std::copy(t->weights.begin(), t->weights.end(), weights);
        *bias = t->bias;
    });
}

int fd_ehog_tracker_get_layers(fd_ehog_tracker* t, fd_ehog_layer* out, int cap, int* n) {
    if (!t || !n || cap < 0 || (cap > 0 && !out)) return FD_ERR_INVALID_ARGUMENT;
    *n = t->updated ? (int)t->layers.size() : 0;
    if (*n > cap) return FD_ERR_CAPACITY;
    std::copy(t->layers.begin(), t->layers.begin() + *n, out);
    return FD_OK;
}

int fd_ehog_tracker_feature_layer(fd_ctx* ctx, fd_ehog_tracker* t, int layer, float* out) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_feature_layer", true, false);
        if (!out || layer < 0 || layer >= (int)t->layers.size()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "no such feature layer: %d", layer);
        const FhogLayerDev& T = t->layerTable[layer];
        const size_t n = (size_t)T.rows * T.cols * t->D;
        if (n) HIP_CHECK(hipMemcpyAsync(out, t->desc.as<float>() + (size_t)T.cellBase * t->D, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_ehog_tracker_heat_layer(fd_ctx* ctx, fd_ehog_tracker* t, int layer, float* out) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_heat_layer", true, true);
        if (!out || layer < 0 || layer >= (int)t->layers.size()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "no such heat layer: %d", layer);
        const FhogLayerDev& T = t->layerTable[layer];
        const size_t n = (size_t)T.rows * T.cols;
        if (n) HIP_CHECK(hipMemcpyAsync(out, t->heat.as<float>() + T.cellBase, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_ehog_tracker_evaluate_samples(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* xywh, uint8_t* valid, float* score) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_evaluate_samples", true, true);
        if (n < 0 || (n > 0 && (!xywh || !valid || !score))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_evaluate_samples: bad argument");
        if (n == 0) return;
        ehog_sample_windows(ctx, t, n, xywh, valid);
        t->outScore.reserve(sizeof(float) * (size_t)n);
        hipLaunchKernelGGL(k_ehog_gather_scores, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, t->dlayers.as<FhogLayerDev>(), t->list.as<int4>(), n,
                           t->prm.cell_rows / 2, t->prm.cell_cols / 2, t->heat.as<float>(), t->outScore.as<float>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(score, t->outScore.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_ehog_tracker_extract_cells(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* xywh, uint8_t* valid, float* features) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_extract_cells", true, false);
        if (n < 0 || (n > 0 && (!xywh || !valid || !features))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_extract_cells: bad argument");
        if (n == 0) return;
        ehog_sample_windows(ctx, t, n, xywh, valid);
        const fd_ehog_tracker_params& P = t->prm;
        const int64_t total = (int64_t)n * P.cell_rows * P.cell_cols * t->D;
        if (total > (int64_t)0x7fffff00 * 64) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_extract_cells: too many values for one call");
        t->outFeat.reserve(sizeof(float) * (size_t)total);
        hipLaunchKernelGGL(k_ehog_gather_cells, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, t->dlayers.as<FhogLayerDev>(),
                           t->list.as<int4>(), total, P.cell_rows, P.cell_cols, t->D, t->desc.as<float>(), t->outFeat.as<float>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(features, t->outFeat.p, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_ehog_tracker_patch_lds_bytes(const fd_ehog_tracker_params* prm) {
    if (!prm || !cehog_params_ok(prm->filter) || prm->cell_cols < 1 || prm->cell_rows < 1) return -1;
    return ehog_patch_geom(*prm).bytes;   // computed in 64 bits; a geometry beyond 2 GB reports INT32_MAX
}

int fd_ehog_tracker_extract_patches(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* xywh, uint8_t* valid, float* features, double* score) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_extract_patches", true, false);
        if (n < 0 || (n > 0 && (!xywh || !valid || !features))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_extract_patches: bad argument");
        if (score && !t->hasSvm) FD_THROW(FD_ERR_RUNTIME, "fd_ehog_tracker_extract_patches: no SVM has been set (fd_ehog_tracker_set_svm)");
        const fd_ehog_tracker_params& P = t->prm;
        const EhogPatchGeom& G = t->geom;
        ehog_check_patch_lds(t, "fd_ehog_tracker_extract_patches");
        if (n == 0) return;
        const EhogWindowRule R = ehog_window_rule(t);
        int4* pin = (int4*)fd_pinned(ctx, sizeof(int4) * (size_t)n);
        for (int i = 0; i < n; ++i) {
            pin[i] = ehog_patch_window(R, t->layers.data(), xywh[4 * i], xywh[4 * i + 1], xywh[4 * i + 2], xywh[4 * i + 3],
                                       [&](int width) { return ehog_layer_of_width(R, R.PW, width); });
            valid[i] = (uint8_t)pin[i].w;
        }
        t->list.reserve(sizeof(int4) * (size_t)n);
        HIP_CHECK(hipMemcpyAsync(t->list.p, pin, sizeof(int4) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        CehogScratch& C = fd_scratch<CehogScratch>(ctx);
        cehog_upload_lut(ctx, C, P.filter);
        const size_t per = (size_t)P.cell_rows * P.cell_cols * t->D;
        t->outFeat.reserve(sizeof(float) * per * (size_t)n);
        if (score) t->outScore.reserve(sizeof(double) * (size_t)n);
        hipLaunchKernelGGL(k_ehog_patch, dim3(n), dim3(64), (size_t)G.bytes, ctx->stream, t->dlayers.as<FhogLayerDev>(), t->dlayerPx.as<EhogLayerPx>(),
                           t->list.as<int4>(), G, C.lut.as<FhogLutEntry>(), t->patchCoeff.as<FhogCoeffDev>(), t->dweights.as<float>(), -(double)t->bias,
                           t->outFeat.as<float>(), score ? t->outScore.as<double>() : nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(features, t->outFeat.p, sizeof(float) * per * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        if (score) HIP_CHECK(hipMemcpyAsync(score, t->outScore.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_ehog_tracker_heat_peak(fd_ctx* ctx, fd_ehog_tracker* t, fd_box* peak, int* found) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_heat_peak", true, true);
        if (!peak) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_heat_peak: NULL argument");
        const fd_ehog_tracker_params& P = t->prm;
        const int cr = P.cell_rows / 2, cc = P.cell_cols / 2, cell = P.filter.cell_size;
        *peak = fd_box{-FLT_MAX, 0, 0, 0, 0};   // bestScore = lowest(), Rect()
        if (found) *found = 0;
        if (t->layout.positions == 0) return;
        t->peak.reserve(sizeof(EhogPeakDev));
        hipLaunchKernelGGL(k_ehog_peak, dim3(1), dim3(1024), 0, ctx->stream, t->dlayers.as<FhogLayerDev>(), (int)t->layerTable.size(), cr, cc,
                           t->heat.as<float>(), t->peak.as<EhogPeakDev>());
        HIP_CHECK(hipGetLastError());
        EhogPeakDev r;
        HIP_CHECK(hipMemcpyAsync(&r, t->peak.p, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (!r.found) return;
        const double scale = t->layers[r.layer].scale;
        auto original = [&](int v) { return fd_cvRound(v / scale); };   // ImagePyramidLayer.hpp:98-100
        *peak = fd_box{r.score, original((r.col - cc) * cell), original((r.row - cr) * cell), original(P.cell_cols * cell), original(P.cell_rows * cell)};
        if (found) *found = 1;
    });
}

int fd_ehog_tracker_heat_maxima(fd_ctx* ctx, fd_ehog_tracker* t, float threshold, fd_box* out, int cap, int* count) {
    return fd_guard(ctx, [&] {
        ehog_checked(ctx, t, "fd_ehog_tracker_heat_maxima", true, true);
        if (!count || cap < 0 || (cap > 0 && !out)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_heat_maxima: bad argument");
        const fd_ehog_tracker_params& P = t->prm;
        if (P.cell_rows < 2 || P.cell_cols < 2)   // the scan looks at column cell_cols / 2 - 1 and row cell_rows / 2 - 1
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_ehog_tracker_heat_maxima: the window needs at least 2 x 2 cells");
        const int cr = P.cell_rows / 2, cc = P.cell_cols / 2, cell = P.filter.cell_size;
        *count = 0;
        const int totalPos = t->layout.positions;
        if (totalPos == 0) return;
        t->maxima.reserve(sizeof(EhogMaxDev) * (size_t)totalPos);
        t->counter.reserve(sizeof(unsigned int));
        HIP_CHECK(hipMemsetAsync(t->counter.p, 0, sizeof(unsigned int), ctx->stream));
        hipLaunchKernelGGL(k_ehog_maxima, dim3((totalPos + 255) / 256), dim3(256), 0, ctx->stream, t->dlayers.as<FhogLayerDev>(), (int)t->layerTable.size(),
                           totalPos, cr, cc, threshold, t->heat.as<float>(), t->maxima.as<EhogMaxDev>(), t->counter.as<unsigned int>());
        HIP_CHECK(hipGetLastError());
        unsigned int found = 0;
        HIP_CHECK(hipMemcpyAsync(&found, t->counter.p, sizeof(found), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *count = (int)found;
        if (found == 0) return;
        std::vector<EhogMaxDev> hits(found);
        HIP_CHECK(hipMemcpy(hits.data(), t->maxima.p, sizeof(EhogMaxDev) * found, hipMemcpyDeviceToHost));
        std::sort(hits.begin(), hits.end(), [](const EhogMaxDev& a, const EhogMaxDev& b) { return a.pos < b.pos; });
        if ((int)found > cap) FD_THROW(FD_ERR_CAPACITY, "fd_ehog_tracker_heat_maxima: %u local maxima, capacity %d", found, cap);
        size_t l = 0;
        for (unsigned int k = 0; k < found; ++k) {
            while (l + 1 < t->layerTable.size() && hits[k].pos >= t->layerTable[l + 1].posBase) ++l;
            const FhogLayerDev& T = t->layerTable[l];
            const int i = hits[k].pos - T.posBase, y = i / T.vw, x = i - y * T.vw;   // y, x: window position (row - cr, column - cc)
            const double scale = t->layers[l].scale;
            auto original = [&](int v) { return fd_cvRound(v / scale); };
            out[k] = fd_box{hits[k].score, original(x * cell), original(y * cell), original(P.cell_cols * cell), original(P.cell_rows * cell)};
        }
    });
}

}  // extern "C"

// fd_particles_evaluate (condensation.hip): the samples of a resident particle set, all in device memory, resolved to windows by
// k_ehog_resolve and scored by the kernels of fd_ehog_tracker_evaluate_samples (use_patches 0) or _extract_patches (1).  Queued on
// the context's stream; nothing is copied back.  The window list {layer, bx, by, valid} goes to `windows` (the caller's, 4 n ints: the
// tracker's own list belongs to its host entry points); the features of the patch form stay in t->outFeat.
void fd_ehog_tracker_score_particles(fd_ctx* ctx, fd_ehog_tracker* t, int n, const int32_t* x, const int32_t* y, const int32_t* size, double aspect,
                                     int use_patches, int32_t* windows, uint8_t* valid, double* score) {
    ehog_checked(ctx, t, "fd_particles_evaluate", true, true);
    if (use_patches) ehog_check_patch_lds(t, "fd_particles_evaluate");
    if (n <= 0) return;
    const EhogWindowRule R = ehog_window_rule(t);
    int4* list = (int4*)windows;
    hipLaunchKernelGGL(k_ehog_resolve, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, R, t->dplan.as<fd_ehog_layer>(),
                       use_patches ? t->dpatchLayerOf.as<int16_t>() : t->dcellLayerOf.as<int16_t>(), use_patches ? t->patchLayerOfLen : t->cellLayerOfLen,
                       x, y, size, n, aspect, use_patches, list, valid);
    HIP_CHECK(hipGetLastError());
    if (!use_patches) {
        t->outScore.reserve(sizeof(float) * (size_t)n);
        hipLaunchKernelGGL(k_ehog_gather_scores, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, t->dlayers.as<FhogLayerDev>(), list, n,
                           t->prm.cell_rows / 2, t->prm.cell_cols / 2, t->heat.as<float>(), t->outScore.as<float>());
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_ehog_widen_scores, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, t->outScore.as<float>(), n, score);
        HIP_CHECK(hipGetLastError());
        return;
    }
    const fd_ehog_tracker_params& P = t->prm;
    const EhogPatchGeom& G = t->geom;
    CehogScratch& C = fd_scratch<CehogScratch>(ctx);
    cehog_upload_lut(ctx, C, P.filter);
    t->outFeat.reserve(sizeof(float) * (size_t)P.cell_rows * P.cell_cols * t->D * (size_t)n);
    hipLaunchKernelGGL(k_ehog_patch, dim3(n), dim3(64), (size_t)G.bytes, ctx->stream, t->dlayers.as<FhogLayerDev>(), t->dlayerPx.as<EhogLayerPx>(),
                       list, G, C.lut.as<FhogLutEntry>(), t->patchCoeff.as<FhogCoeffDev>(), t->dweights.as<float>(), -(double)t->bias,
                       t->outFeat.as<float>(), score);
    HIP_CHECK(hipGetLastError());
}
