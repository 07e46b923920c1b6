// featuredetection_amd/csrc/fhog.hip -- imageprocessing::filtering::FhogFilter (FhogFilter.cpp:20-132,
// FhogFilter.hpp:120-207) + FhogAggregationFilter::computeDescriptors (FhogAggregationFilter.cpp:38-168) on gray
// images / gray pyramid layers: the cell descriptors (2B signed + B unsigned orientation features + 4 energy features)
// the AggregatedFeaturesDetector family convolves its linear SVM over.  SURVEY.md 8(f) row 2, second piece.
//
// All layers of a launch (one image, or every layer of a pyramid) go through the kernels together over a device layer table:
// k_fhog_coeff (bilinear cell-interpolation tables), k_fhog_grad (per-pixel (bin, weight) entries from the same 511 x 511
// gradient look-up table the reference builds with host libm atan2 / sqrt: FhogFilter.cpp:35-57), k_fhog_hist (lane == cell:
// a lane walks the pixels that contribute to its cell in the reference's row-major scan order -- with bilinear cell
// interpolation a pixel feeds up to four cells, so a cell sees a 2c x 2c neighbourhood -- and accumulates into its private
// 2B-bin histogram in LDS, so every fp32 accumulator receives its addends in the reference order), k_fhog_desc (the four
// neighbourhood normalisers, truncation at alpha, the 0.5 / 0.2357 factors) and, for the detector, k_fhog_score.
#include "fd_internal.hpp"
#include "fd_device.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>

struct FhogLut {   // (bin, weight) of a gradient: what k_fhog_hist consumes per pixel
    uint8_t index1, index2;
    uint16_t pad;
    float weight1, weight2;
};
struct FhogLutEntry {   // one entry per (dy, dx) gradient code (FhogFilter.hpp:108-111: bins + magnitude)
    FhogLut bins;
    float magnitude;
};
struct FhogCoeffDev { int32_t index1, index2; float weight1, weight2; };

struct FhogParamsDev {
    int32_t cell, ubins, sbins, D, interpBins, interpCells;
    int32_t plainEnergy;           // k_fhog_hist: energy over the sbins bins themselves (CompleteExtendedHogFilter, unsigned only)
    float alpha;
    const FhogLutEntry* lut;       // [512 * 512], index dy * 512 + dx
    const FhogCoeffDev* coeff;     // all layers: rows of layer 0, columns of layer 0, rows of layer 1, ...
};
struct FhogLayerDev {              // one gray image / pyramid layer of a launch
    const uint8_t* img;
    int32_t w, h, stride;          // stride in bytes
    int32_t channels;              // 1 or 3 (interleaved)
    int32_t rows, cols;            // cells
    int32_t cellBase, coeffBase;   // first cell / first coefficient of the layer in the launch-wide arrays
    int32_t vw, vh, posBase;       // window positions of the score map (aggregated detector only)
    int32_t cellBlockBase;         // first 64-cell block of the layer
    int32_t pixBase, pixBlockBase; // first covered pixel (rows*cell x cols*cell per layer) / first 256-pixel block
    int32_t posBlockBase;          // first 8-position block of the layer
};

struct FhogResizeTab { int32_t i0, i1; float w0, w1; };   // cv::resize INTER_LINEAR, one output row / column: two sources and weights
struct FhogApproxDev {             // one approximated feature layer of a launch of k_fhog_approx
    int32_t layer, parent;         // entries of the layer table: output and the exact layer it is resized from
    int32_t blockBase;             // first 256-value block of the layer
    int32_t xtab, ytab;            // its column / row tables in the launch-wide FhogResizeTab array
    int32_t factorBase;            // its per-channel factors
};

struct FhogLayoutTotals { int cells = 0, coeffs = 0, cellBlocks = 0, positions = 0, posBlocks = 0, pixels = 0, pixBlocks = 0; };

struct fd_aggregated {
    fd_ctx* ctx;
    fd_aggregated_params prm;
    std::vector<float> weights;
    DevBuf dweights, scores;
    fd_pyramid* pyr = nullptr;
    int pyrW = 0, pyrH = 0;
    std::vector<FhogLayerDev> layerTable;   // of the current pyramid geometry
    FhogLayoutTotals layout;
    DevBuf dlayers;
    void* arenaAt = nullptr;
    std::vector<fd_aggregated_layer> layers;   // feature layers of the last detect, layer order
    std::vector<int> tableOf;                  // their entries in layerTable
    // approximated feature pyramid (fd_aggregated_create_approximated): the exact layers are the first entries of layerTable,
    // the approximated ones follow
    bool approx = false;
    std::vector<double> givenLambdas, lambdas;   // as created (empty: estimate per image) / used by the last detect
    FhogLayoutTotals exactLayout;
    std::vector<FhogApproxDev> approxTable;
    std::vector<double> approxScale;             // pow(inc, i) per entry of approxTable
    int approxBlocks = 0, sumChunks = 0, sumLayer[2] = {0, 0};
    DevBuf dapprox, dresize, dfactors, dsums;
    std::vector<float> factors;
    std::vector<double> sums;
    // feature type: FHOG on a gray pyramid, or FPDW channel features (fd_aggregated_create_fpdw, fpdw.hpp) on a pyramid of three
    // frames, the B, G and R planes of the image
    int D = 0;                                   // channels per cell
    bool fpdw = false;
    fd_fpdw_params fpp{};
    int fpdwTiles = 0;                           // k_fpdw workgroups over the exact layers
    uint64_t featureStamp = 0;                   // of its last update (0: none): a new handle at a destroyed owner's address owns nothing
    ~fd_aggregated() { if (pyr) fd_pyramid_destroy(pyr); }
};

namespace {

using namespace fd_dev;

constexpr int FHOG_MAX_SBINS = 36;
constexpr int FHOG_CH = 6;         // pixels whose loads are in flight together in k_fhog_hist

// the layer of a launch-wide index (a block, cell, coefficient, pixel block or position): the last one whose Base is not above it
template <int32_t FhogLayerDev::*Base>
__device__ __forceinline__ int layer_of(const FhogLayerDev* __restrict__ layers, int nLayers, int key) {
    int l = 0;
    for (int i = 1; i < nLayers; ++i)
        if (key >= layers[i].*Base) l = i;
    return l;
}

// createInterpolationCoefficients (FhogFilter.cpp:74-98, Real = float) and createLut (CompleteExtendedHogFilter.cpp:72-103,
// Real = double: the index in double, the weights rounded to float once) for one pixel row / column of sizeInCells cells.
// Add / divide / floor of both types are correctly rounded on the device (no fast-math), so a device table equals the host's.
template <typename Real>
__host__ __device__ inline FhogCoeffDev cell_coeff(int pixel, int cell, int sizeInCells, bool interpCells) {
    if (!interpCells) return FhogCoeffDev{pixel / cell, -1, 1.f, 0.f};
    const Real realCellIndex = ((Real)pixel + (Real)0.5) / (Real)cell - (Real)0.5;
    int index1 = (int)std::floor(realCellIndex);
    int index2 = index1 + 1;
    float weight2 = (float)(realCellIndex - index1);
    float weight1;   // the one place the two filters differ
    if constexpr (std::is_same<Real, float>::value) weight1 = index2 - realCellIndex;
    else weight1 = 1.f - weight2;
    if (index1 < 0) { index1 = index2; weight1 = 0; }
    else if (index2 >= sizeInCells) { index2 = index1; weight2 = 0; }
    return FhogCoeffDev{index1, index2, weight1, weight2};
}

// ---- the arithmetic k_fhog_hist / k_fhog_desc share with k_ehog_patch (ehog_tracker.hpp); `hist(b)` is bin b of the cell's
// histogram ([bin][lane] in LDS, [bin * nCells + cell] in LDS, or the cell's run of the raw histograms) ----

// one pixel's vote into a cell it reaches through row weight wr and column coefficients cc (c1 / c2: which of its two indices
// is the cell): FhogFilter.hpp:174-207
template <class Hist>
__device__ __forceinline__ void fhog_vote(Hist&& hist, const FhogLut& e, float wr, const FhogCoeffDev& cc, bool c1, bool c2, bool interpCells,
                                          bool interpBins) {
    if (interpCells) {
        const float wc = (c1 ? cc.weight1 : 0.f) + (c2 ? cc.weight2 : 0.f);
        hist(e.index1) = hist(e.index1) + e.weight1 * wr * wc;
        if (interpBins) hist(e.index2) = hist(e.index2) + e.weight2 * wr * wc;
    } else {
        hist(e.index1) = hist(e.index1) + e.weight1;
        if (interpBins) hist(e.index2) = hist(e.index2) + e.weight2;
    }
}

// computeGradientEnergy (FhogAggregationFilter.cpp:53-61): over the unsigned halves; plainEnergy: over the sbins bins themselves
// (CompleteExtendedHogFilter.cpp:181-190, unsigned-only histograms)
template <class Hist>
__device__ __forceinline__ float fhog_energy(Hist&& hist, int sbins, int ubins, bool plainEnergy) {
    float energy = 0.f;
    if (plainEnergy) {
        for (int b = 0; b < sbins; ++b) energy = energy + hist(b) * hist(b);
    } else {
        for (int b = 0; b < ubins; ++b) {
            const float u = hist(b) + hist(b + ubins);
            energy = energy + u * u;
        }
    }
    return energy;
}

// computeNormalizers (FhogAggregationFilter.cpp:77-99) of cell (r, c) of a rows x cols map; E(r, c) is a cell's energy
template <class Energy>
__device__ __forceinline__ void fhog_normalizers(Energy&& E, int r, int c, int rows, int cols, float n[4]) {
    const int pr = max(r - 1, 0), nr = min(r + 1, rows - 1), pc = max(c - 1, 0), nc = min(c + 1, cols - 1);
    const float eps = 1e-4f;
    n[0] = 1.f / sqrtf(E(pr, pc) + E(pr, c) + E(r, pc) + E(r, c) + eps);
    n[1] = 1.f / sqrtf(E(pr, c) + E(pr, nc) + E(r, c) + E(r, nc) + eps);
    n[2] = 1.f / sqrtf(E(r, pc) + E(r, c) + E(nr, pc) + E(nr, c) + eps);
    n[3] = 1.f / sqrtf(E(r, c) + E(r, nc) + E(nr, c) + E(nr, nc) + eps);
}

// computeDescriptor (FhogAggregationFilter.cpp:101-148), feature f of [sbins bins][ubins unsigned sums][4 energies]; 0.5 and
// 0.2357 are double literals
template <class Hist>
__device__ __forceinline__ float fhog_feature(Hist&& hist, const float n[4], int f, int sbins, int ubins, float alpha) {
    if (f < sbins) {
        const float v = hist(f);
        const float v0 = fminf(alpha, n[0] * v), v1 = fminf(alpha, n[1] * v), v2 = fminf(alpha, n[2] * v), v3 = fminf(alpha, n[3] * v);
        return (float)(0.5 * (double)(v0 + v1 + v2 + v3));
    }
    if (f < sbins + ubins) {
        const int b = f - sbins;
        const float v = hist(b) + hist(b + ubins);
        const float s = fminf(alpha, n[0] * v) + fminf(alpha, n[1] * v) + fminf(alpha, n[2] * v) + fminf(alpha, n[3] * v);
        return (float)(0.5 * (double)s);
    }
    const float ni = n[f - sbins - ubins];
    float energy = 0.f;
    for (int b = 0; b < sbins; ++b) energy = energy + fminf(alpha, ni * hist(b));
    return (float)(0.2357 * (double)energy);
}

// (bin, weight) entries of every pixel the cells cover: the gradient of FhogFilter.hpp:120-160 (central differences,
// replicated border) as a code into the reference's look-up table, so that k_fhog_hist reads each entry from a dense map
// instead of chasing the table once per neighbouring cell.  The map is stored phase-major, entry (y, x) at
// [(y * cell + x % cell) * cols + x / cell]: in k_fhog_hist lane == cell, so the 64 lanes of a wavefront, which look at the
// same in-cell offset of consecutive cells, read consecutive entries (a lane-per-cell walk over a row-major map touches 64
// cache lines per load and is bound by the L1 tag rate).  Thread order == storage order: coalesced writes.
__global__ __launch_bounds__(256) void k_fhog_grad(const FhogLayerDev* __restrict__ layers, int nLayers, FhogParamsDev d, FhogLut* __restrict__ grad) {
    const FhogLayerDev L = layers[layer_of<&FhogLayerDev::pixBlockBase>(layers, nLayers, blockIdx.x)];
    const int W = L.cols * d.cell, H = L.rows * d.cell;
    const int i = (blockIdx.x - L.pixBlockBase) * 256 + threadIdx.x;
    if (i >= W * H) return;
    const int y = i / W, rem = i - y * W;
    const int o = rem / L.cols, cx = rem - o * L.cols;
    const int x = cx * d.cell + o;
    const int py = max(y - 1, 0), ny = min(y + 1, L.h - 1), px = max(x - 1, 0), nx = min(x + 1, L.w - 1);
    const uint8_t* rowp = L.img + (size_t)y * L.stride;
    FhogLut e;
    if (L.channels == 1) {
        const int dx = (int)rowp[nx] - (int)rowp[px] + 256;
        const int dy = (int)L.img[(size_t)ny * L.stride + x] - (int)L.img[(size_t)py * L.stride + x] + 256;
        e = d.lut[dy * 512 + dx].bins;
    } else {   // getBinCoefficients<false> (FhogFilter.hpp:144-172): the channel with the largest gradient magnitude
        const uint8_t* up = L.img + (size_t)py * L.stride + 3 * x;
        const uint8_t* dn = L.img + (size_t)ny * L.stride + 3 * x;
        const uint8_t* lf = rowp + 3 * px;
        const uint8_t* rt = rowp + 3 * nx;
        const FhogLutEntry e1 = d.lut[((int)dn[0] - (int)up[0] + 256) * 512 + ((int)rt[0] - (int)lf[0] + 256)];
        const FhogLutEntry e2 = d.lut[((int)dn[1] - (int)up[1] + 256) * 512 + ((int)rt[1] - (int)lf[1] + 256)];
        const FhogLutEntry e3 = d.lut[((int)dn[2] - (int)up[2] + 256) * 512 + ((int)rt[2] - (int)lf[2] + 256)];
        if (e1.magnitude > e2.magnitude) e = e1.magnitude > e3.magnitude ? e1.bins : e3.bins;
        else e = e2.magnitude > e3.magnitude ? e2.bins : e3.bins;
    }
    grad[(size_t)L.pixBase + i] = e;
}

// cell_coeff<Real> for every pixel row / column the cells of every layer cover, one thread each
template <typename Real>
__global__ __launch_bounds__(256) void k_fhog_coeff(const FhogLayerDev* __restrict__ layers, int nLayers, int total, FhogParamsDev d,
                                                    FhogCoeffDev* __restrict__ coeff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const FhogLayerDev L = layers[layer_of<&FhogLayerDev::coeffBase>(layers, nLayers, i)];
    const int j = i - L.coeffBase, rowPixels = L.rows * d.cell;
    const int pixel = j < rowPixels ? j : j - rowPixels;
    // rows in pixel order; columns phase-major ([x % cell][x / cell]) like the gradient map
    coeff[j < rowPixels ? i : L.coeffBase + rowPixels + (pixel % d.cell) * L.cols + pixel / d.cell] =
        cell_coeff<Real>(pixel, d.cell, j < rowPixels ? L.rows : L.cols, d.interpCells);
}

__global__ __launch_bounds__(64) void k_fhog_hist(const FhogLayerDev* __restrict__ layers, int nLayers, FhogParamsDev d,
                                                  const FhogLut* __restrict__ gradAll, float* __restrict__ rawHist, float* __restrict__ energies) {
    __shared__ float hist[FHOG_MAX_SBINS][64];
    const FhogLayerDev L = layers[layer_of<&FhogLayerDev::cellBlockBase>(layers, nLayers, blockIdx.x)];
    const int lane = threadIdx.x;
    const int cellId = (blockIdx.x - L.cellBlockBase) * 64 + lane;
    const bool valid = cellId < L.rows * L.cols;
    const int r = valid ? cellId / L.cols : 0, c = valid ? cellId - r * L.cols : 0;
    for (int b = 0; b < d.sbins; ++b) hist[b][lane] = 0.f;
    if (valid) {
        auto bin = [&](int b) -> float& { return hist[b][lane]; };
        const FhogCoeffDev* __restrict__ rowCoeff = d.coeff + L.coeffBase;
        const FhogCoeffDev* __restrict__ colCoeff = rowCoeff + L.rows * d.cell;
        // pixel box feeding this cell: non-interpolated [r*cell, (r+1)*cell); interpolated: every pixel whose index1 or index2
        // is r lies within `off` pixels around it
        const int cs = d.cell;
        const int H = L.rows * cs;
        const int off = d.interpCells ? (cs + 1) / 2 + 1 : 0, box = cs + 2 * off;
        // A pixel reaches a cell through at most one row role and one column role with a non-zero weight: where index1 ==
        // index2 (clamped borders, FhogFilter.cpp:88-95) one of the two weights is exactly 0, and the reference's add of
        // e.weight * 0 * w = +0 leaves the (non-negative) accumulator unchanged.  So the effective weight of a row / column is
        // (index1 hit ? weight1 : 0) + (index2 hit ? weight2 : 0) -- exact, one addend is 0 -- and every pixel costs one
        // read-modify-write per bin, in scan order.
        const FhogLut* __restrict__ gbase = gradAll + (size_t)L.pixBase;
        for (int ii = 0; ii < box; ++ii) {
            const int y = r * cs - off + ii;
            if (y < 0 || y >= H) continue;
            const FhogCoeffDev rc = rowCoeff[y];
            const bool r1 = rc.index1 == r, r2 = d.interpCells && rc.index2 == r;
            if (!r1 && !r2) continue;
            const float wr = (r1 ? rc.weight1 : 0.f) + (r2 ? rc.weight2 : 0.f);
            const size_t yrow = (size_t)y * cs;
            for (int jb = 0; jb < box; jb += FHOG_CH) {
                FhogCoeffDev cc[FHOG_CH];
                FhogLut e[FHOG_CH];
                bool in[FHOG_CH];
#pragma unroll
                for (int j = 0; j < FHOG_CH; ++j) {   // the loads of FHOG_CH pixels are issued together
                    // x = c*cs - off + jb + j = (c + q - 2) * cs + o with wave-uniform q, o
                    const int t = 2 * cs - off + jb + j, q = t / cs, o = t - q * cs;
                    const int cx = c + q - 2;
                    in[j] = jb + j < box && cx >= 0 && cx < L.cols;
                    const int cxs = in[j] ? cx : c;
                    cc[j] = colCoeff[o * L.cols + cxs];
                    e[j] = gbase[(yrow + o) * L.cols + cxs];
                }
#pragma unroll
                for (int j = 0; j < FHOG_CH; ++j) {
                    const bool c1 = cc[j].index1 == c, c2 = d.interpCells && cc[j].index2 == c;
                    if (!in[j] || (!c1 && !c2)) continue;
                    fhog_vote(bin, e[j], wr, cc[j], c1, c2, d.interpCells, d.interpBins);
                }
            }
        }
        energies[L.cellBase + cellId] = fhog_energy(bin, d.sbins, d.ubins, d.plainEnergy);
    }
    // raw histograms [cell][2B] of the block's 64 consecutive cells, written as one contiguous run
    wave_sync();
    const int cellsHere = min(64, L.rows * L.cols - (blockIdx.x - L.cellBlockBase) * 64);
    float* out = rawHist + ((size_t)L.cellBase + (size_t)(blockIdx.x - L.cellBlockBase) * 64) * d.sbins;
    for (int i = lane; i < cellsHere * d.sbins; i += 64) {
        const int cl = i / d.sbins, b = i - cl * d.sbins;
        out[i] = hist[b][cl];
    }
}

// FhogAggregationFilter::computeDescriptors (:63-148) from the raw histograms: LPC (32 or 64) lanes per cell, lane == output
// feature, so that the [cell][2B] reads and the [cell][3B+4] writes are contiguous; every lane derives the cell's four
// normalisers itself (16 cached energy reads).
template <int LPC>
__global__ __launch_bounds__(256) void k_fhog_desc(const FhogLayerDev* __restrict__ layers, int nLayers, int totalCells, FhogParamsDev d,
                                                   const float* __restrict__ energiesAll, const float* __restrict__ rawHist, float* __restrict__ descAll) {
    const int g = (blockIdx.x * 256 + threadIdx.x) / LPC, f = threadIdx.x & (LPC - 1);
    if (g >= totalCells || f >= d.D) return;
    const FhogLayerDev L = layers[layer_of<&FhogLayerDev::cellBase>(layers, nLayers, g)];
    const int cellId = g - L.cellBase;
    const float* energies = energiesAll + L.cellBase;
    const float* h = rawHist + (size_t)g * d.sbins;
    const int r = cellId / L.cols, c = cellId - r * L.cols;
    float n[4];
    fhog_normalizers([&](int rr, int cc) { return energies[rr * L.cols + cc]; }, r, c, L.rows, L.cols, n);
    descAll[(size_t)g * d.D + f] = fhog_feature([&](int b) { return h[b]; }, n, f, d.sbins, d.ubins, d.alpha);
}

// AggregatedFeaturesExtractor::extract for a list of windows: the window_h x window_w cells of window v, D floats each, from
// the descriptor buffer into row `row` of an n x (cells * D) matrix.  A thread per float; consecutive threads are the channels of
// a cell, then the cells of a window row, so that reads are runs of window_w * D floats and the writes of a window are one run.
struct AggWindowDev { int32_t cell, cols, row; };   // first cell in the descriptor buffer, cells per layer row, output row
__global__ __launch_bounds__(256) void k_agg_gather(const AggWindowDev* __restrict__ windows, int nWindows, const float* __restrict__ desc, int D,
                                                   int windowW, int windowCells, float* __restrict__ out) {
    const int64_t d = (int64_t)windowCells * D;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= d * nWindows) return;
    const int v = (int)(idx / d);
    const int f = (int)(idx - (int64_t)v * d);
    const int cell = f / D, c = f - cell * D;
    const int wy = cell / windowW, wx = cell - wy * windowW;
    const AggWindowDev W = windows[v];
    out[(int64_t)W.row * d + f] = desc[((int64_t)W.cell + (int64_t)wy * W.cols + wx) * D + c];
}

struct FhogScratch {
    DevBuf lut, coeff, img, desc, energies, layers, grad, hist;
    DevBuf windows, gathered;          // fd_aggregated_extract: its window list, and the rows of a call that returns them to the host
    fd_fhog_params lutFor;
    bool lutValid = false;
    const void* descOwner = nullptr;   // the fd_aggregated whose last detect's feature layers `desc` still holds
    uint64_t descStamp = 0;            // the count of such updates on this context, as the owner recorded it
};
FhogScratch& scratch(fd_ctx* ctx) { return fd_scratch<FhogScratch>(ctx); }

// gradient look-up table of FhogFilter::createGradientLut (FhogFilter.cpp:35-57), host libm like the reference
void build_lut(fd_ctx* ctx, FhogScratch& S, const fd_fhog_params& fp) {
    if (S.lutValid && S.lutFor.unsigned_bins == fp.unsigned_bins && S.lutFor.interpolate_bins == fp.interpolate_bins) return;
    const int signedBinCount = 2 * fp.unsigned_bins;
    const float TWO_PI = (float)(2 * M_PI);
    const float value2bin = signedBinCount / TWO_PI;
    std::vector<FhogLutEntry> lut((size_t)512 * 512);
    std::memset(lut.data(), 0, sizeof(FhogLutEntry) * lut.size());
    for (int gradientCodeX = 1; gradientCodeX < 512; ++gradientCodeX) {
        const float gradientX = (gradientCodeX - 256) / (255.0f * 2.0f);
        for (int gradientCodeY = 1; gradientCodeY < 512; ++gradientCodeY) {
            const float gradientY = (gradientCodeY - 256) / (255.0f * 2.0f);
            const float magnitude = std::sqrt(gradientX * gradientX + gradientY * gradientY);
            float orientation = std::atan2(gradientY, gradientX);
            if (orientation < 0) orientation += TWO_PI;
            FhogLut e;
            std::memset(&e, 0, sizeof(e));
            if (fp.interpolate_bins) {
                const float bin = orientation * value2bin;
                int i1 = (int)bin, i2 = i1 + 1;
                if (i2 == signedBinCount) i2 = 0;
                e.index1 = (uint8_t)i1; e.index2 = (uint8_t)i2;
                e.weight2 = magnitude * (bin - i1);
                e.weight1 = magnitude - e.weight2;
            } else {
                int bin = (int)(orientation * value2bin + 0.5f);
                if (bin == signedBinCount) bin = 0;
                e.index1 = (uint8_t)bin; e.weight1 = magnitude;
            }
            lut[(size_t)gradientCodeY * 512 + gradientCodeX] = FhogLutEntry{e, magnitude};
        }
    }
    S.lut.reserve(sizeof(FhogLutEntry) * lut.size());
    HIP_CHECK(hipMemcpy(S.lut.p, lut.data(), sizeof(FhogLutEntry) * lut.size(), hipMemcpyHostToDevice));
    S.lutFor = fp;
    S.lutValid = true;
}

void check_fhog_params(const fd_fhog_params& fp) {
    if (fp.cell_size < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "FhogFilter: cellSize must be bigger than zero");
    if (fp.unsigned_bins < 1 || 2 * fp.unsigned_bins > FHOG_MAX_SBINS)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "FhogFilter: unsignedBinCount must be bigger than zero, but was: %d (this backend: <= %d)", fp.unsigned_bins,
                 FHOG_MAX_SBINS / 2);
    if (!(fp.alpha > 0)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "FhogAggregationFilter: alpha must be bigger than zero, but was: %g", (double)fp.alpha);
}

// a gray / interleaved / planar image on the device as an entry of a layer list
FhogLayerDev layer_entry(const uint8_t* dimg, int w, int h, int stride, int channels) {
    FhogLayerDev L;
    std::memset(&L, 0, sizeof(L));
    L.img = dimg; L.w = w; L.h = h; L.stride = stride; L.channels = channels;
    return L;
}

// fills the launch-wide offsets of a layer list (img, w, h, stride, vw, vh set by the caller); returns the launch-wide totals
FhogLayoutTotals layout_layers(std::vector<FhogLayerDev>& layers, int cell) {
    FhogLayoutTotals t;
    for (FhogLayerDev& L : layers) {
        L.rows = L.h / cell;
        L.cols = L.w / cell;
        L.cellBase = t.cells; L.coeffBase = t.coeffs; L.cellBlockBase = t.cellBlocks; L.posBase = t.positions; L.posBlockBase = t.posBlocks;
        L.pixBase = t.pixels; L.pixBlockBase = t.pixBlocks;
        const int64_t npix = (int64_t)L.rows * L.cols * cell * cell;
        if (t.pixels + npix > (int64_t)0x7fffff00) FD_THROW(FD_ERR_INVALID_ARGUMENT, "FhogFilter: the layers of one launch exceed 2^31 pixels");
        t.pixels += (int)npix;
        t.pixBlocks += (int)((npix + 255) / 256);
        t.cells += L.rows * L.cols;
        t.coeffs += (L.rows + L.cols) * cell;
        t.cellBlocks += (L.rows * L.cols + 63) / 64;
        t.positions += L.vw * L.vh;
        t.posBlocks += (((L.vw + 3) / 4) * L.vh + 7) / 8;   // k_fhog_score: 8 groups of FHOG_SP = 4 positions per block
    }
    return t;
}

// one image already on the device as a one-entry layer table: L (made by layer_entry) laid out and uploaded to dtable
FhogLayoutTotals single_layer_table(fd_ctx* ctx, DevBuf& dtable, FhogLayerDev& L, int cell) {
    std::vector<FhogLayerDev> layers(1, L);
    const FhogLayoutTotals t = layout_layers(layers, cell);
    L = layers[0];
    dtable.reserve(sizeof(FhogLayerDev));
    HIP_CHECK(hipMemcpyAsync(dtable.p, &L, sizeof(FhogLayerDev), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));   // L is pageable host memory
    return t;
}

// What a filter of the family hands run_cell_filter: its gradient look-up table on the device, whether its cell interpolation
// table is computed in double, and the parameters of k_fhog_hist and of k_fhog_desc (their lut and coeff are filled in by the
// runner; the coefficient and gradient kernels read cell, interpCells and lut, which the two blocks share).
struct FhogRun {
    const FhogLutEntry* lut;
    bool doubleCoeff;
    FhogParamsDev hist, desc;
};

// descriptors of every layer of the table at dlayers (device copy of a list laid out by layout_layers) into descOut
// (t.cells * channels floats on the device; NULL: S.desc)
void run_cell_filter(fd_ctx* ctx, FhogScratch& S, const FhogLayerDev* dlayers, int nLayers, const FhogLayoutTotals& t, FhogRun f, float* descOut) {
    if (!descOut) S.descOwner = nullptr;
    if (t.cells == 0) return;
    S.coeff.reserve(sizeof(FhogCoeffDev) * (size_t)t.coeffs);
    if (!descOut) {
        S.desc.reserve(sizeof(float) * (size_t)t.cells * f.desc.D);
        descOut = S.desc.as<float>();
    }
    S.energies.reserve(sizeof(float) * (size_t)t.cells);
    S.grad.reserve(sizeof(FhogLut) * (size_t)t.pixels);
    S.hist.reserve(sizeof(float) * (size_t)t.cells * f.hist.sbins);
    f.hist.lut = f.desc.lut = f.lut;
    f.hist.coeff = f.desc.coeff = S.coeff.as<FhogCoeffDev>();
    const auto coeffKernel = f.doubleCoeff ? k_fhog_coeff<double> : k_fhog_coeff<float>;
    hipLaunchKernelGGL(coeffKernel, dim3((t.coeffs + 255) / 256), dim3(256), 0, ctx->stream, dlayers, nLayers, t.coeffs, f.hist, S.coeff.as<FhogCoeffDev>());
    hipLaunchKernelGGL(k_fhog_grad, dim3(t.pixBlocks), dim3(256), 0, ctx->stream, dlayers, nLayers, f.hist, S.grad.as<FhogLut>());
    hipLaunchKernelGGL(k_fhog_hist, dim3(t.cellBlocks), dim3(64), 0, ctx->stream, dlayers, nLayers, f.hist, S.grad.as<FhogLut>(), S.hist.as<float>(),
                       S.energies.as<float>());
    const int LPC = f.desc.D <= 32 ? 32 : 64;   // lanes per cell of k_fhog_desc
    const auto descKernel = LPC == 32 ? k_fhog_desc<32> : k_fhog_desc<64>;
    hipLaunchKernelGGL(descKernel, dim3((unsigned)(((int64_t)t.cells * LPC + 255) / 256)), dim3(256), 0, ctx->stream, dlayers, nLayers, t.cells, f.desc,
                       S.energies.as<float>(), S.hist.as<float>(), descOut);
    HIP_CHECK(hipGetLastError());
}

// FhogFilter descriptors of every layer of the table at dlayers into S.desc
void run_fhog(fd_ctx* ctx, FhogScratch& S, const FhogLayerDev* dlayers, int nLayers, const FhogLayoutTotals& t, const fd_fhog_params& fp) {
    check_fhog_params(fp);
    build_lut(ctx, S, fp);
    FhogParamsDev d;
    std::memset(&d, 0, sizeof(d));
    d.cell = fp.cell_size; d.ubins = fp.unsigned_bins; d.sbins = 2 * fp.unsigned_bins; d.D = 3 * fp.unsigned_bins + 4;
    d.interpBins = fp.interpolate_bins != 0; d.interpCells = fp.interpolate_cells != 0; d.alpha = fp.alpha;
    run_cell_filter(ctx, S, dlayers, nLayers, t, FhogRun{S.lut.as<FhogLutEntry>(), false, d, d}, nullptr);
}

// one gray or BGR image already on the device; an image smaller than a cell has an empty map: nothing is launched
void run_fhog_single(fd_ctx* ctx, FhogScratch& S, const uint8_t* dimg, int w, int h, int stride, const fd_fhog_params& fp, int& rows, int& cols,
                     int channels = 1) {
    check_fhog_params(fp);
    FhogLayerDev L = layer_entry(dimg, w, h, stride, channels);
    const FhogLayoutTotals t = single_layer_table(ctx, S.layers, L, fp.cell_size);
    rows = L.rows; cols = L.cols;
    if (rows == 0 || cols == 0) return;
    run_fhog(ctx, S, S.layers.as<FhogLayerDev>(), 1, t, fp);
}

// ConvolutionFilter(CV_32F) of AggregatedFeaturesDetector (ConvolutionFilter.cpp:27-43 with anchor (0, 0), delta = -bias):
// score(y, x) = delta + sum over channels c of [sum over the kernel window, row-major, of K[ky][kx][c] * F[y+ky][x+kx][c]]:
// the nesting and the fp32 accumulation order of the per-channel cv::filter2D + channel sum.  All layers in one launch;
// a group of 32 lanes (lane == channel, D <= 32: coalesced reads of a cell's descriptor) owns FHOG_SP horizontally adjacent
// window positions and slides a register window over the descriptor row, so a kernel column costs one K and one F load for
// FHOG_SP multiply-adds; every position's per-channel sum still runs in kernel row-major order.  The channel sums are then
// added in channel order onto delta by one lane per position.
constexpr int FHOG_SP = 4;
__global__ __launch_bounds__(256) void k_fhog_score(const FhogLayerDev* __restrict__ layers, int nLayers, const float* __restrict__ descAll, int D,
                                                    const float* __restrict__ K, int kh, int kw, float delta, float* __restrict__ scores) {
    __shared__ float part[8][FHOG_SP][33];
    const FhogLayerDev L = layers[layer_of<&FhogLayerDev::posBlockBase>(layers, nLayers, blockIdx.x)];
    const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int gpr = (L.vw + FHOG_SP - 1) / FHOG_SP;   // groups per score row
    const int g = (blockIdx.x - L.posBlockBase) * 8 + grp;
    const bool valid = g < gpr * L.vh;
    const int y = valid ? g / gpr : 0, x0 = valid ? (g - y * gpr) * FHOG_SP : 0;
    const float* F = descAll + (size_t)L.cellBase * D;
    float sacc[FHOG_SP];
#pragma unroll
    for (int p = 0; p < FHOG_SP; ++p) sacc[p] = 0.f;
    if (valid && lane < D) {
        const int lastCol = L.cols - 1;
        for (int ky = 0; ky < kh; ++ky) {
            const float* frow = F + (size_t)(y + ky) * L.cols * D + lane;
            const float* krow = K + (size_t)ky * kw * D + lane;
            float w[FHOG_SP];
#pragma unroll
            for (int p = 0; p < FHOG_SP; ++p) w[p] = frow[(size_t)min(x0 + p, lastCol) * D];
            for (int kx = 0; kx < kw; ++kx) {
                const float k = krow[(size_t)kx * D];
                const float nxt = frow[(size_t)min(x0 + kx + FHOG_SP, lastCol) * D];
#pragma unroll
                for (int p = 0; p < FHOG_SP; ++p) sacc[p] = sacc[p] + k * w[p];
#pragma unroll
                for (int p = 0; p + 1 < FHOG_SP; ++p) w[p] = w[p + 1];
                w[FHOG_SP - 1] = nxt;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < FHOG_SP; ++p) part[grp][p][lane] = sacc[p];
    __syncthreads();
    if (valid && lane < FHOG_SP && x0 + lane < L.vw) {
        float score = delta;
        for (int c = 0; c < D; ++c) score = score + part[grp][lane][c];
        scores[L.posBase + y * L.vw + x0 + lane] = score;
    }
}

// descriptors wider than 32 channels (more than 9 unsigned bins): one lane per position, one block row per layer
__global__ __launch_bounds__(256) void k_fhog_score_wide(const FhogLayerDev* __restrict__ layers, const float* __restrict__ descAll, int D,
                                                         const float* __restrict__ K, int kh, int kw, float delta, float* __restrict__ scores) {
    const FhogLayerDev L = layers[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.vw * L.vh) return;
    const int y = i / L.vw, x = i - y * L.vw;
    const float* F = descAll + (size_t)L.cellBase * D;
    float score = delta;
    for (int c = 0; c < D; ++c) {
        float sacc = 0.f;
        for (int ky = 0; ky < kh; ++ky) {
            const float* frow = F + ((size_t)(y + ky) * L.cols + x) * D + c;
            const float* krow = K + (size_t)ky * kw * D + c;
            for (int kx = 0; kx < kw; ++kx) sacc = sacc + krow[(size_t)kx * D] * frow[(size_t)kx * D];
        }
        score = score + sacc;
    }
    scores[L.posBase + i] = score;
}

// ---- approximated feature layers (ImagePyramid::createLayers(const ImagePyramid&), ImagePyramid.cpp:200-235,277-289) ----

// Per-channel double sums of two feature layers (ImagePyramid::computeChannelMeans, :254-261), one launch: blockIdx.y picks the
// layer, a block owns FHOG_SUM_CELLS consecutive cells.  Lane == channel (D <= 64), so a wavefront reads a cell's descriptor as one
// run and every lane keeps its channel's sum in a register; the four wavefronts of a block take every fourth cell and meet in LDS,
// where wavefront 0 adds the four in order and writes the block's partial: no atomics, and a fixed order of additions.  The host
// adds the partials of a layer in block order.
constexpr int FHOG_SUM_CELLS = 256;
__global__ __launch_bounds__(256) void k_fhog_channel_sums(const FhogLayerDev* __restrict__ layers, int layerA, int layerB,
                                                           const float* __restrict__ descAll, int D, double* __restrict__ partials) {
    __shared__ double part[4][64];
    const FhogLayerDev L = layers[blockIdx.y == 0 ? layerA : layerB];
    const int c = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nCells = L.rows * L.cols;
    const int first = blockIdx.x * FHOG_SUM_CELLS, last = min(first + FHOG_SUM_CELLS, nCells);
    const float* F = descAll + (size_t)L.cellBase * D;
    double sum = 0.0;
    if (c < D)
        for (int cell = first + wave; cell < last; cell += 4) sum = sum + (double)F[(size_t)cell * D + c];
    part[wave][c] = sum;
    __syncthreads();
    if (wave == 0 && c < D)
        partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * D + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// Every approximated layer of every octave in one launch: ImagePyramid::resize (:277-289) = per channel cv::resize(INTER_LINEAR)
// on CV_32F (float weights, horizontal pass, then vertical pass; the tables come from the host) and a float multiply by
// (float)pow(s, -lambda[channel]).  One thread per output value, channel fastest: the reads of the four source cells and the write
// are runs of D floats.  The file is compiled with -ffp-contract=off, so the products and sums below stay separate roundings.
__global__ __launch_bounds__(256) void k_fhog_approx(const FhogLayerDev* __restrict__ layers, const FhogApproxDev* __restrict__ approx, int nApprox,
                                                     const FhogResizeTab* __restrict__ tabs, const float* __restrict__ factors, int D,
                                                     float* __restrict__ descAll) {
    int ai = 0;
    for (int i = 1; i < nApprox; ++i)
        if ((int)blockIdx.x >= approx[i].blockBase) ai = i;
    const FhogApproxDev A = approx[ai];
    const FhogLayerDev L = layers[A.layer], P = layers[A.parent];
    const int e = ((int)blockIdx.x - A.blockBase) * 256 + (int)threadIdx.x;
    if (e >= L.rows * L.cols * D) return;
    const int cell = e / D, c = e - cell * D;
    const int y = cell / L.cols, x = cell - y * L.cols;
    const FhogResizeTab tx = tabs[A.xtab + x], ty = tabs[A.ytab + y];
    const float* S = descAll + (size_t)P.cellBase * D + c;
    const float* S0 = S + (size_t)ty.i0 * P.cols * D;
    const float* S1 = S + (size_t)ty.i1 * P.cols * D;
    const float r0 = S0[(size_t)tx.i0 * D] * tx.w0 + S0[(size_t)tx.i1 * D] * tx.w1;
    const float r1 = S1[(size_t)tx.i0 * D] * tx.w0 + S1[(size_t)tx.i1 * D] * tx.w1;
    const float v = r0 * ty.w0 + r1 * ty.w1;
    descAll[(size_t)L.cellBase * D + e] = v * factors[A.factorBase + c];
}

// cv::resize(INTER_LINEAR) source indices and float weights of `dn` outputs over `sn` inputs (the coordinate arithmetic of
// OpenCV 2.4's resize, as in the pyramid's own tables); vertical: indices clipped into the image instead of zeroed weights
void resize_tab(int sn, int dn, bool horizontal, std::vector<FhogResizeTab>& out) {
    const double inv_scale = (double)dn / sn, scale = 1. / inv_scale;
    for (int d = 0; d < dn; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (horizontal) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= sn - 1) { f = 0; s = sn - 1; }
            out.push_back(FhogResizeTab{s, std::min(s + 1, sn - 1), 1.f - f, f});
        } else {
            auto clip = [&](int v) { return v < 0 ? 0 : (v >= sn ? sn - 1 : v); };
            out.push_back(FhogResizeTab{clip(s), clip(s + 1), 1.f - f, f});
        }
    }
}

}  // namespace

#include "fpdw.hpp"

extern "C" {

int fd_fhog_size(const fd_fhog_params* fp, int width, int height, int* rows, int* cols, int* channels) {
    if (!fp || fp->cell_size < 1 || fp->unsigned_bins < 1) return FD_ERR_INVALID_ARGUMENT;
    if (rows) *rows = height / fp->cell_size;
    if (cols) *cols = width / fp->cell_size;
    if (channels) *channels = 3 * fp->unsigned_bins + 4;
    return FD_OK;
}

int fd_fhog_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, const fd_fhog_params* fp, float* out) {
    return fd_fhog_image_channels(ctx, gray, width, height, 1, fp, out);
}

int fd_fhog_image_channels(fd_ctx* ctx, const uint8_t* image, int width, int height, int channels, const fd_fhog_params* fp, float* out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !image || !fp || !out || width < 1 || height < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_fhog_image: bad argument");
        if (channels != 1 && channels != 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "FhogFilter: the image type must be CV_8UC1 or CV_8UC3 (%d channels)", channels);
        HIP_CHECK(hipSetDevice(ctx->device));
        FhogScratch& S = scratch(ctx);
        const size_t bytes = (size_t)width * height * channels;
        S.img.reserve(bytes);
        HIP_CHECK(hipMemcpyAsync(S.img.p, image, bytes, hipMemcpyHostToDevice, ctx->stream));
        int rows, cols;
        run_fhog_single(ctx, S, S.img.as<uint8_t>(), width, height, width * channels, *fp, rows, cols, channels);
        if (rows && cols)
            HIP_CHECK(hipMemcpyAsync(out, S.desc.p, sizeof(float) * (size_t)rows * cols * (3 * fp->unsigned_bins + 4), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_pyramid_fhog_layer(fd_ctx* ctx, fd_pyramid* p, int layer, const fd_fhog_params* fp, float* out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !p || !fp || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_fhog_layer: NULL argument");
        if (p->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
        if (p->filter_kind != FD_LAYER_NONE) FD_THROW(FD_ERR_INVALID_ARGUMENT, "FhogFilter needs a gray pyramid (no layer filter)");
        fd_pyramid_require_single(p, "fd_pyramid_fhog_layer");
        if (layer < 0 || layer >= (int)p->kept.size()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "no such pyramid layer: %d", layer);
        HIP_CHECK(hipSetDevice(ctx->device));
        const HostLayer& L = p->all[p->kept[layer]];
        FhogScratch& S = scratch(ctx);
        int rows, cols;
        run_fhog_single(ctx, S, p->arena.as<uint8_t>() + L.gray_off, L.w, L.h, L.w, *fp, rows, cols);
        if (rows && cols)
            HIP_CHECK(hipMemcpyAsync(out, S.desc.p, sizeof(float) * (size_t)rows * cols * (3 * fp->unsigned_bins + 4), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

static int aggregated_create(fd_ctx* ctx, const fd_aggregated_params* prm, bool approx, const double* lambdas, int n_lambdas, fd_aggregated** out,
                             const fd_fpdw_params* fpdw = nullptr) {
    return fd_guard(ctx, [&] {
        if (!ctx || !prm || !out || !prm->svm_weights) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_create: NULL argument");
        if (prm->window_w < 1 || prm->window_h < 1 || prm->octave_layer_count < 1)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "AggregatedFeaturesDetector: window size and octave layer count must be positive");
        if (fpdw) {
            check_fpdw_params(*fpdw);
            if (prm->fhog.cell_size != fpdw->cell_size)
                FD_THROW(FD_ERR_INVALID_ARGUMENT, "AggregatedFeaturesDetector: the detector's cell size (%d) and the aggregation filter's (%d) differ",
                         prm->fhog.cell_size, fpdw->cell_size);
            fpdw_tile_cells(*fpdw);   // throws when the working set of one cell exceeds the tile memory
        } else if (prm->fhog.cell_size < 1 || prm->fhog.unsigned_bins < 1 || 2 * prm->fhog.unsigned_bins > FHOG_MAX_SBINS || !(prm->fhog.alpha > 0))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "AggregatedFeaturesDetector: invalid FhogFilter parameters");
        HIP_CHECK(hipSetDevice(ctx->device));
        std::unique_ptr<fd_aggregated> a(new fd_aggregated());
        a->ctx = ctx;
        a->prm = *prm;
        a->fpdw = fpdw != nullptr;
        if (fpdw) a->fpp = *fpdw;
        a->D = fpdw ? FPDW_CHANNELS : 3 * prm->fhog.unsigned_bins + 4;
        const size_t nw = (size_t)prm->window_w * prm->window_h * a->D;
        a->weights.assign(prm->svm_weights, prm->svm_weights + nw);
        a->prm.svm_weights = nullptr;
        a->dweights.reserve(sizeof(float) * nw);
        HIP_CHECK(hipMemcpy(a->dweights.p, a->weights.data(), sizeof(float) * nw, hipMemcpyHostToDevice));
        a->approx = approx;
        if (approx && n_lambdas != 0) {   // ImagePyramid.cpp:212-213
            if (n_lambdas < 0 || !lambdas) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_create_approximated: bad lambdas");
            if (n_lambdas != a->D)
                FD_THROW(FD_ERR_RUNTIME, "ImagePyramid: the number of lambdas does not match the number of channels");
            a->givenLambdas.assign(lambdas, lambdas + n_lambdas);
        }
        *out = a.release();
    });
}

int fd_aggregated_create(fd_ctx* ctx, const fd_aggregated_params* prm, fd_aggregated** out) {
    return aggregated_create(ctx, prm, false, nullptr, 0, out);
}

int fd_aggregated_create_approximated(fd_ctx* ctx, const fd_aggregated_params* prm, const double* lambdas, int n_lambdas, fd_aggregated** out) {
    return aggregated_create(ctx, prm, true, lambdas, n_lambdas, out);
}

int fd_aggregated_create_fpdw(fd_ctx* ctx, const fd_aggregated_params* prm, const fd_fpdw_params* fp, int approximated, const double* lambdas,
                              int n_lambdas, fd_aggregated** out) {
    if (!fp) return fd_guard(ctx, [&] { FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_create_fpdw: NULL argument"); });
    if (!approximated && n_lambdas != 0)
        return fd_guard(ctx, [&] { FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_create_fpdw: lambdas belong to the approximated feature pyramid"); });
    return aggregated_create(ctx, prm, approximated != 0, lambdas, n_lambdas, out, fp);
}

int fd_aggregated_get_lambdas(fd_aggregated* a, double* out, int cap, int* n) {
    if (!a || !n || cap < 0 || (cap > 0 && !out)) return FD_ERR_INVALID_ARGUMENT;
    *n = (int)a->lambdas.size();
    if (*n > cap) return FD_ERR_CAPACITY;
    std::copy(a->lambdas.begin(), a->lambdas.end(), out);
    return FD_OK;
}

int fd_aggregated_get_layers(fd_aggregated* a, fd_aggregated_layer* out, int cap, int* n) {
    if (!a || !n || cap < 0 || (cap > 0 && !out)) return FD_ERR_INVALID_ARGUMENT;
    *n = (int)a->layers.size();
    if (*n > cap) return FD_ERR_CAPACITY;
    std::copy(a->layers.begin(), a->layers.end(), out);
    return FD_OK;
}

int fd_aggregated_feature_layer(fd_ctx* ctx, fd_aggregated* a, int layer, float* out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !a || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_feature_layer: NULL argument");
        if (a->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
        FhogScratch& S = scratch(ctx);
        if (S.descOwner != a) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_feature_layer: the feature layers of this detector's last detect are gone");
        if (layer < 0 || layer >= (int)a->layers.size()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "no such feature layer: %d", layer);
        HIP_CHECK(hipSetDevice(ctx->device));
        const FhogLayerDev& T = a->layerTable[a->tableOf[layer]];
        const int D = a->D;
        const size_t n = (size_t)T.rows * T.cols * D;
        if (n) HIP_CHECK(hipMemcpyAsync(out, S.desc.as<float>() + (size_t)T.cellBase * D, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

void fd_aggregated_destroy(fd_aggregated* a) { delete a; }

// score maps of every layer of the handle's layer table (exact and approximated alike) from the descriptors in S.desc
static void launch_scores(fd_ctx* ctx, fd_aggregated* a, FhogScratch& S) {
    const fd_aggregated_params& P = a->prm;
    const int D = a->D, nLayers = (int)a->layerTable.size();
    if (a->layout.positions <= 0) return;
    if (D <= 32) {
        hipLaunchKernelGGL(k_fhog_score, dim3(a->layout.posBlocks), dim3(256), 0, ctx->stream, a->dlayers.as<FhogLayerDev>(), nLayers,
                           S.desc.as<float>(), D, a->dweights.as<float>(), P.window_h, P.window_w, -P.svm_bias, a->scores.as<float>());
    } else {
        int maxPos = 0;
        for (const FhogLayerDev& T : a->layerTable) maxPos = std::max(maxPos, T.vw * T.vh);
        hipLaunchKernelGGL(k_fhog_score_wide, dim3((maxPos + 255) / 256, nLayers), dim3(256), 0, ctx->stream, a->dlayers.as<FhogLayerDev>(),
                           S.desc.as<float>(), D, a->dweights.as<float>(), P.window_h, P.window_w, -P.svm_bias, a->scores.as<float>());
    }
    HIP_CHECK(hipGetLastError());
}

// bounds in image pixels of the window at cell (x, y) of a layer: computeBoundsInImagePixels
// (AggregatedFeaturesExtractor.cpp:121-128) through the layer's x / y scales
static inline fd_box aggregated_bounds(const fd_aggregated_params& P, int x, int y, double scaleX, double scaleY) {
    const int cs = P.fhog.cell_size;
    const int bx = (int)std::round((x * cs) / scaleX), by = (int)std::round((y * cs) / scaleY);
    const int bw = (int)std::round((P.window_w * cs) / scaleX), bh = (int)std::round((P.window_h * cs) / scaleY);
    return fd_box{0.f, bx, by, bw, bh};
}

// a window with score > threshold as a candidate: its bounds, Patch::computeCenter, rescaleWindow
// (AggregatedFeaturesDetector.cpp:108-112)
static inline fd_box aggregated_candidate(const fd_aggregated_params& P, float score, int x, int y, double scaleX, double scaleY) {
    const fd_box b = aggregated_bounds(P, x, y, scaleX, scaleY);
    const int cx = b.x + b.w / 2, cy = b.y + b.h / 2;
    const int rw = (int)(P.width_scale * b.w), rh = (int)(P.height_scale * b.h);
    return fd_box{score, cx - rw / 2, cy - rh / 2, rw, rh};
}

// AggregatedFeaturesExtractor::extract(Rect) (AggregatedFeaturesExtractor.cpp:83-119) up to the copy, in double as written: the
// layer round(log(patchWidthPx / width) / log(inc)) (ImagePyramid::getLayer(double), ImagePyramid.cpp:307-310), the centre
// through the layer's actual scales, truncated to cells (computePointInLayerCells), Patch::computeBounds, isPatchWithinImage.
// false where the reference returns a null patch (and for a width < 1, whose scale factor the reference does not define).
// layer: position in a->layers; (x, y): the window's first cell.
static bool aggregated_resolve(const fd_aggregated* a, const int32_t* box, int& layer, int& x, int& y) {
    const fd_aggregated_params& P = a->prm;
    const int cs = P.fhog.cell_size;
    if (box[2] < 1) return false;
    const double inc = std::pow(0.5, 1. / P.octave_layer_count);
    const double scaleFactor = (double)(P.window_w * cs) / (double)box[2];
    const double power = std::log(scaleFactor) / std::log(inc);
    const int index = (int)std::round(power);
    layer = -1;
    for (size_t i = 0; i < a->layers.size(); ++i)
        if (a->layers[i].index == index) layer = (int)i;
    if (layer < 0) return false;
    const fd_aggregated_layer& L = a->layers[layer];
    const FhogLayerDev& T = a->layerTable[a->tableOf[layer]];
    const double cxImage = box[0] + 0.5 * box[2], cyImage = box[1] + 0.5 * box[3];
    const int cxCells = (int)((cxImage * L.scale_x) / cs), cyCells = (int)((cyImage * L.scale_y) / cs);
    x = cxCells - P.window_w / 2;
    y = cyCells - P.window_h / 2;
    return x >= 0 && y >= 0 && x + P.window_w <= T.cols && y + P.window_h <= T.rows;
}

// the image into the detector's pyramid: gray layers, or, for FPDW features, a pyramid of three frames -- the B, G and R planes of
// the image, each scaled exactly as a gray image is (cv::resize and cv::pyrDown treat the channels of a CV_8UC3 image independently)
static void aggregated_update_pyramid(fd_ctx* ctx, fd_aggregated* a, const uint8_t* image, int width, int height, int channels, int is_device) {
    int rc;
    if (a->fpdw) {
        const size_t planeStride = fpdw_planes(ctx, fpdw_scratch(ctx), image, width, height, is_device);
        const uint8_t* planes[3];
        for (int k = 0; k < 3; ++k) planes[k] = fpdw_scratch(ctx).planes.as<uint8_t>() + k * planeStride;
        rc = fd_pyramid_update_frames(a->pyr, planes, 3, width, height, 1, 1);
    } else {
        rc = fd_pyramid_update(a->pyr, image, width, height, channels, is_device);
    }
    if (rc != FD_OK) throw FdError{rc, ctx->error};
}

// what an FPDW handle checks before anything is built: the image type (FpdwFeaturesFilter.cpp:67-69)
static void aggregated_check_image(const fd_aggregated* a, int width, int height, int channels) {
    if (!a->fpdw) return;
    if (width < 1 || height < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update: empty image");
    if (channels != 3)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "FpdwFeaturesFilter: the gradient image type must be CV_8UC3 or CV_32FC3, but was %d", (channels - 1) * 8);
}

// cell descriptors of the first nLayers entries of the handle's layer table (its exact layers) into S.desc
static void aggregated_features(fd_ctx* ctx, fd_aggregated* a, FhogScratch& S, int nLayers, const FhogLayoutTotals& t) {
    if (!a->fpdw) {
        run_fhog(ctx, S, a->dlayers.as<FhogLayerDev>(), nLayers, t, a->prm.fhog);
        return;
    }
    for (int i = 0; i < nLayers; ++i) check_fpdw_image_size(a->fpp, a->layerTable[i].w, a->layerTable[i].h, true);   // the filters see every layer
    S.descOwner = nullptr;
    run_fpdw(ctx, a->dlayers.as<FhogLayerDev>(), nLayers, a->fpdwTiles, a->pyr->image_stride, a->fpp, false, S.desc.as<float>());
}

// The geometry of a handle's feature pyramid, rebuilt when the image size or the pyramid's arena has changed: the layer list, the
// layer table (exact layers first, so that the feature launches see exactly them, with the launch geometry of an exact run; the
// approximated ones follow in the same descriptor buffer), layouts, tiles, uploads and, for the approximated layers, the launch
// table of k_fhog_approx with its resize tables.  An exact handle is the approximated one without approximated layers: its
// layer list is the pyramid's kept layers (octave_layer_count per octave, where the approximated handle's pyramid has one).
static void aggregated_geometry(fd_ctx* ctx, fd_aggregated* a, int width, int height) {
    const fd_aggregated_params& P = a->prm;
    const int D = a->D, cs = P.fhog.cell_size, n = P.octave_layer_count;
    const fd_pyramid* p = a->pyr;
    const size_t E = p->kept.size();
    a->layers.clear();
    if (a->approx) {
        FdAggregatedPlan plan;
        fd_host_plan_aggregated(cs, n, p->minS, p->maxS, width, height, plan);
        bool same = plan.exactPx.size() == E;
        for (size_t li = 0; same && li < E; ++li)
            same = plan.exactPx[li].first == p->all[p->kept[li]].w && plan.exactPx[li].second == p->all[p->kept[li]].h;
        if (!same) FD_THROW(FD_ERR_RUNTIME, "fd_aggregated_detect: the layer plan and the gray pyramid disagree");
        a->layers = plan.layers;
    } else {
        for (size_t li = 0; li < E; ++li) {
            const HostLayer& H = p->all[p->kept[li]];   // scales: ImagePyramid.cpp:178-179,187-188
            a->layers.push_back(fd_aggregated_layer{H.index, 0, -1, H.h / cs, H.w / cs, 0, H.scale, (double)H.w / (double)width, (double)H.h / (double)height});
        }
    }
    const std::vector<fd_aggregated_layer>& list = a->layers;
    a->tableOf.assign(list.size(), -1);
    a->layerTable.assign(list.size(), FhogLayerDev{});
    size_t nextApprox = E;
    for (size_t i = 0, e = 0; i < list.size(); ++i) {
        const fd_aggregated_layer& L = list[i];
        const int ti = L.approximated ? (int)nextApprox++ : (int)e++;
        a->tableOf[i] = ti;
        FhogLayerDev& T = a->layerTable[ti];
        if (!L.approximated) {
            const HostLayer& H = p->all[p->kept[ti]];
            T = layer_entry(p->arena.as<uint8_t>() + H.gray_off, H.w, H.h, H.w, a->fpdw ? 3 : 1);
        } else {   // no pixels: layout_layers derives rows / cols from w / h
            const fd_aggregated_layer& X = list[L.parent];
            const bool empty = X.rows < 1 || X.cols < 1;
            T = layer_entry(nullptr, empty ? 0 : L.cols * cs, empty ? 0 : L.rows * cs, 0, 0);
        }
        T.vh = std::max(T.h / cs - P.window_h + 1, 0);
        T.vw = std::max(T.w / cs - P.window_w + 1, 0);
        if (T.vw == 0 || T.vh == 0) T.vw = T.vh = 0;
    }
    {
        std::vector<FhogLayerDev> exact(a->layerTable.begin(), a->layerTable.begin() + E);
        a->exactLayout = layout_layers(exact, cs);
    }
    a->layout = layout_layers(a->layerTable, cs);
    // k_fpdw's tiles over the exact layers
    if (a->fpdw) a->fpdwTiles = fpdw_assign_tiles(a->layerTable, (int)E, a->fpp.cell_size, fpdw_tile_cells(a->fpp), false);
    // approximated layers: launch table, cv::resize tables, factors
    a->approxTable.clear();
    a->approxScale.clear();
    std::vector<FhogResizeTab> tabs;
    int blocks = 0;
    const double inc = std::pow(0.5, 1. / n);
    for (size_t i = 0; i < list.size(); ++i) {
        const fd_aggregated_layer& L = list[i];
        if (!L.approximated) continue;
        const FhogLayerDev& T = a->layerTable[a->tableOf[i]];
        const FhogLayerDev& X = a->layerTable[a->tableOf[L.parent]];
        if (T.rows < 1 || T.cols < 1) continue;
        FhogApproxDev A;
        A.layer = a->tableOf[i]; A.parent = a->tableOf[L.parent];
        A.blockBase = blocks;
        A.xtab = (int)tabs.size();
        resize_tab(X.cols, T.cols, true, tabs);
        A.ytab = (int)tabs.size();
        resize_tab(X.rows, T.rows, false, tabs);
        A.factorBase = (int)a->approxTable.size() * D;
        blocks += (int)(((int64_t)T.rows * T.cols * D + 255) / 256);
        a->approxTable.push_back(A);
        a->approxScale.push_back(std::pow(inc, L.index - list[L.parent].index));
    }
    a->approxBlocks = blocks;
    a->dlayers.reserve(sizeof(FhogLayerDev) * a->layerTable.size());
    HIP_CHECK(hipMemcpy(a->dlayers.p, a->layerTable.data(), sizeof(FhogLayerDev) * a->layerTable.size(), hipMemcpyHostToDevice));
    if (!a->approxTable.empty()) {
        a->dapprox.reserve(sizeof(FhogApproxDev) * a->approxTable.size());
        HIP_CHECK(hipMemcpy(a->dapprox.p, a->approxTable.data(), sizeof(FhogApproxDev) * a->approxTable.size(), hipMemcpyHostToDevice));
        a->dresize.reserve(sizeof(FhogResizeTab) * tabs.size());
        HIP_CHECK(hipMemcpy(a->dresize.p, tabs.data(), sizeof(FhogResizeTab) * tabs.size(), hipMemcpyHostToDevice));
        a->dfactors.reserve(sizeof(float) * a->approxTable.size() * D);
    }
    a->factors.assign(a->approxTable.size() * D, 0.f);
    // the two exact layers the lambdas are estimated from (ImagePyramid.cpp:240-243)
    if (a->approx && a->givenLambdas.empty()) {
        a->sumLayer[0] = E > 2 ? 1 : 0;
        a->sumLayer[1] = a->sumLayer[0] + 1;
        const FhogLayerDev& SA = a->layerTable[a->sumLayer[0]];
        a->sumChunks = std::max(1, (SA.rows * SA.cols + FHOG_SUM_CELLS - 1) / FHOG_SUM_CELLS);   // the larger of the two
        a->dsums.reserve(sizeof(double) * 2 * a->sumChunks * D);
        a->sums.assign((size_t)2 * a->sumChunks * D, 0.0);
    }
    a->lambdas.clear();
    a->arenaAt = p->arena.p;
}

// One image into a handle's feature layers (AggregatedFeaturesExtractor::update): the pyramid (created anew when the image size
// changes; an approximated handle's has one layer per octave), the geometry when it is stale, the features of the exact layers,
// for an approximated handle [channel sums -> host: lambdas and factors] and k_fhog_approx.  Queued on ctx->stream; the context's
// descriptor buffer is this handle's from here on.
static void aggregated_update(fd_ctx* ctx, fd_aggregated* a, const uint8_t* image, int width, int height, int channels, int is_device) {
    const fd_aggregated_params& P = a->prm;
    const int D = a->D;
    // feature pyramid limits (AggregatedFeaturesExtractor.cpp:30-31,47-52,58-77), recomputed when the image size changes
    if (!a->pyr || a->pyrW != width || a->pyrH != height) {
        if (a->pyr) { fd_pyramid_destroy(a->pyr); a->pyr = nullptr; }
        a->layerTable.clear();
        a->layers.clear();
        double minScale, maxScale;
        fd_host_aggregated_limits(P.window_w, P.window_h, P.fhog.cell_size, P.octave_layer_count, P.min_window_width, width, height, minScale, maxScale);
        // approximated: both setters forward to the source pyramid (ImagePyramid.hpp:241-263), which has one layer per octave
        int rc = fd_pyramid_create(ctx, a->approx ? 1 : P.octave_layer_count, minScale, maxScale, &a->pyr);
        if (rc == FD_OK && a->fpdw) rc = fd_pyramid_set_frames(a->pyr, 3);
        if (rc != FD_OK) throw FdError{rc, ctx->error};
        a->pyrW = width; a->pyrH = height;
    }
    aggregated_update_pyramid(ctx, a, image, width, height, channels, is_device);
    fd_pyramid* p = a->pyr;
    // ImagePyramid::estimateLambdas (ImagePyramid.cpp:238-242): of the score pyramid of an exact handle, of the feature pyramid of an
    // approximated one unless its lambdas are given, which need no second layer (:209-213)
    const bool estimate = a->approx && a->givenLambdas.empty();
    if ((!a->approx || estimate) && p->kept.size() < 2)
        FD_THROW(FD_ERR_RUNTIME, "ImagePyramid: at least two pyramid layers are needed to estimate the lambdas");
    FhogScratch& S = scratch(ctx);
    if (a->layerTable.empty() || a->arenaAt != p->arena.p) aggregated_geometry(ctx, a, width, height);
    const int nExact = (int)p->kept.size(), nApprox = (int)a->approxTable.size();
    S.desc.reserve(sizeof(float) * (size_t)std::max(a->layout.cells, 1) * D);   // before the features: room for the approximated layers too
    aggregated_features(ctx, a, S, nExact, a->exactLayout);
    // factors (float)pow(s, -lambda[c]) (ImagePyramid.cpp:284; Mat *= double on CV_32F multiplies by the float)
    auto set_factors = [&](const std::vector<double>& lambdas) {
        for (int k = 0; k < nApprox; ++k)
            for (int c = 0; c < D; ++c) a->factors[(size_t)k * D + c] = (float)std::pow(a->approxScale[k], -lambdas[c]);
        if (nApprox) HIP_CHECK(hipMemcpyAsync(a->dfactors.p, a->factors.data(), sizeof(float) * a->factors.size(), hipMemcpyHostToDevice, ctx->stream));
    };
    if (estimate) {
        hipLaunchKernelGGL(k_fhog_channel_sums, dim3(a->sumChunks, 2), dim3(256), 0, ctx->stream, a->dlayers.as<FhogLayerDev>(), a->sumLayer[0],
                           a->sumLayer[1], S.desc.as<float>(), D, a->dsums.as<double>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(a->sums.data(), a->dsums.p, sizeof(double) * a->sums.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        // estimateLambdas(layer1, layer2) (ImagePyramid.cpp:246-275): means, ratios, -log(ratio) / log(scale1 / scale2), host libm
        std::vector<double> lambdas(D);
        double mean[2];
        double scaleOf[2];
        for (int k = 0; k < 2; ++k) scaleOf[k] = p->all[p->kept[a->sumLayer[k]]].scale;
        for (int c = 0; c < D; ++c) {
            for (int k = 0; k < 2; ++k) {
                const FhogLayerDev& T = a->layerTable[a->sumLayer[k]];
                double sum = 0.0;
                for (int b = 0; b < a->sumChunks; ++b) sum += a->sums[((size_t)k * a->sumChunks + b) * D + c];
                mean[k] = sum / ((double)T.rows * T.cols);
            }
            lambdas[c] = -std::log(mean[0] / mean[1]) / std::log(scaleOf[0] / scaleOf[1]);
        }
        a->lambdas = lambdas;
        set_factors(a->lambdas);
    } else if (a->approx && a->lambdas.empty()) {   // given lambdas: once per geometry
        a->lambdas = a->givenLambdas;
        set_factors(a->lambdas);
    }
    if (nApprox && a->approxBlocks > 0) {
        hipLaunchKernelGGL(k_fhog_approx, dim3(a->approxBlocks), dim3(256), 0, ctx->stream, a->dlayers.as<FhogLayerDev>(),
                           a->dapprox.as<FhogApproxDev>(), nApprox, a->dresize.as<FhogResizeTab>(), a->dfactors.as<float>(), D, S.desc.as<float>());
        HIP_CHECK(hipGetLastError());
    }
    S.descOwner = a;
    a->featureStamp = ++S.descStamp;
}

// One image through a handle: its feature layers, the score kernel over all of them, and the candidates.
static void aggregated_candidates(fd_ctx* ctx, fd_aggregated* a, const uint8_t* image, int width, int height, int channels, int is_device,
                                  std::vector<fd_box>& cand) {
    const fd_aggregated_params& P = a->prm;
    aggregated_update(ctx, a, image, width, height, channels, is_device);
    FhogScratch& S = scratch(ctx);
    a->scores.reserve(sizeof(float) * std::max<size_t>((size_t)a->layout.positions, 1));
    launch_scores(ctx, a, S);
    std::vector<float> hs((size_t)a->layout.positions);
    if (!hs.empty()) HIP_CHECK(hipMemcpyAsync(hs.data(), a->scores.p, sizeof(float) * hs.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // getPositiveWindows (AggregatedFeaturesDetector.cpp:87-106) over the layers in layer order: layer, row, column
    for (size_t i = 0; i < a->layers.size(); ++i) {
        const FhogLayerDev& T = a->layerTable[a->tableOf[i]];
        const fd_aggregated_layer& L = a->layers[i];
        for (int y = 0; y < T.vh; ++y)
            for (int x = 0; x < T.vw; ++x) {
                const float score = hs[(size_t)T.posBase + (size_t)y * T.vw + x];
                if (score > P.score_threshold) cand.push_back(aggregated_candidate(P, score, x, y, L.scale_x, L.scale_y));
            }
    }
}

int fd_aggregated_detect(fd_ctx* ctx, fd_aggregated* a, const uint8_t* image, int width, int height, int channels, int is_device, fd_box* out,
                         int cap, int* count, fd_box* candidates, int cand_cap, int* cand_count) {
    return fd_guard(ctx, [&] {
        if (!ctx || !a || !image || !count) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_detect: NULL argument");
        if (a->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
        const fd_aggregated_params& P = a->prm;
        HIP_CHECK(hipSetDevice(ctx->device));
        std::vector<fd_box> cand;
        aggregated_check_image(a, width, height, channels);
        aggregated_candidates(ctx, a, image, width, height, channels, is_device, cand);
        if (cand_count) *cand_count = (int)cand.size();
        if (candidates)
            for (size_t i = 0; i < cand.size() && (int)i < cand_cap; ++i) candidates[i] = cand[i];
        std::vector<fd_box> fin(cand.size());
        int nfin = 0;
        const int rc = fd_nms_iou(cand.data(), (int)cand.size(), P.nms_overlap_threshold, P.nms_maximum_type, fin.data(), &nfin);
        if (rc != FD_OK) FD_THROW(rc, "NonMaximumSuppression failed (overlap threshold %g, maximum type %d)", P.nms_overlap_threshold, P.nms_maximum_type);
        *count = nfin;
        for (int i = 0; i < nfin && i < cap && out; ++i) out[i] = fin[i];
        if (out && nfin > cap) FD_THROW(FD_ERR_CAPACITY, "fd_aggregated_detect: %d detections, capacity %d", nfin, cap);
    });
}

int fd_aggregated_update(fd_ctx* ctx, fd_aggregated* a, const uint8_t* image, int width, int height, int channels, int is_device) {
    return fd_guard(ctx, [&] {
        if (!ctx || !a || !image) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_update: NULL argument");
        if (a->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
        HIP_CHECK(hipSetDevice(ctx->device));
        aggregated_check_image(a, width, height, channels);
        aggregated_update(ctx, a, image, width, height, channels, is_device);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_aggregated_extract(fd_ctx* ctx, fd_aggregated* a, int n, const int32_t* boxes, float* features, int features_on_device, fd_box* bounds,
                          uint8_t* valid) {
    return fd_guard(ctx, [&] {
        if (!ctx || !a || n < 0 || (n > 0 && (!boxes || !features || !valid))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_extract: NULL argument");
        if (a->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
        FhogScratch& S = scratch(ctx);
        if (S.descOwner != a || a->featureStamp != S.descStamp || a->featureStamp == 0)
            FD_THROW(FD_ERR_RUNTIME, "fd_aggregated_extract: the feature layers of this detector's last update are gone");
        HIP_CHECK(hipSetDevice(ctx->device));
        const fd_aggregated_params& P = a->prm;
        const int D = a->D, cells = P.window_w * P.window_h;
        const size_t d = (size_t)cells * D;
        std::vector<AggWindowDev> wins;
        std::vector<int> rowOf;   // output row of a gathered window
        for (int k = 0; k < n; ++k) {
            int layer, x, y;
            valid[k] = aggregated_resolve(a, boxes + 4 * (size_t)k, layer, x, y) ? 1 : 0;
            if (!valid[k]) continue;
            const fd_aggregated_layer& L = a->layers[layer];
            const FhogLayerDev& T = a->layerTable[a->tableOf[layer]];
            if (bounds) bounds[k] = aggregated_bounds(P, x, y, L.scale_x, L.scale_y);
            wins.push_back(AggWindowDev{T.cellBase + y * T.cols + x, T.cols, features_on_device ? k : (int)wins.size()});
            rowOf.push_back(k);
        }
        if (wins.empty()) return;
        const int nv = (int)wins.size();
        S.windows.reserve(sizeof(AggWindowDev) * wins.size());
        HIP_CHECK(hipMemcpyAsync(S.windows.p, wins.data(), sizeof(AggWindowDev) * wins.size(), hipMemcpyHostToDevice, ctx->stream));
        float* out = features;
        if (!features_on_device) {
            S.gathered.reserve(sizeof(float) * d * nv);
            out = S.gathered.as<float>();
        }
        const int64_t total = (int64_t)d * nv;
        hipLaunchKernelGGL(k_agg_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, S.windows.as<AggWindowDev>(), nv,
                           S.desc.as<float>(), D, P.window_w, cells, out);
        HIP_CHECK(hipGetLastError());
        if (!features_on_device) {
            std::vector<float> rows(d * nv);
            HIP_CHECK(hipMemcpyAsync(rows.data(), out, sizeof(float) * rows.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            for (int v = 0; v < nv; ++v) std::memcpy(features + (size_t)rowOf[v] * d, rows.data() + (size_t)v * d, sizeof(float) * d);
        } else {
            HIP_CHECK(hipStreamSynchronize(ctx->stream));   // wins is pageable host memory
        }
    });
}

int fd_aggregated_set_svm(fd_ctx* ctx, fd_aggregated* a, const float* weights, float bias, float threshold) {
    return fd_guard(ctx, [&] {
        if (!ctx || !a || !weights) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_aggregated_set_svm: NULL argument");
        if (a->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
        HIP_CHECK(hipSetDevice(ctx->device));
        a->weights.assign(weights, weights + a->weights.size());
        HIP_CHECK(hipMemcpyAsync(a->dweights.p, a->weights.data(), sizeof(float) * a->weights.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        a->prm.svm_bias = bias;
        a->prm.score_threshold = threshold;
    });
}

}  // extern "C"

#include "cehog.hpp"
#include "ehog_tracker.hpp"
