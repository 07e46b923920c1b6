// featuredetection_amd/csrc/fpdw.hpp -- imageprocessing::filtering::FpdwFeaturesFilter(fastGradient, interpolate, radius, constant)
// (FpdwFeaturesFilter.cpp:21-205) chained with AggregationFilter(cellSize, true, false) (AggregationFilter.cpp:20-36,
// TriangularConvolutionFilter.cpp:20-241): ten channels per cell -- six unsigned gradient-orientation bins, the normalised
// gradient magnitude, L*u*v* -- on planar BGR images / pyramid layers.  Included by fhog.hip (same layer table, same descriptor
// buffer, same score / approximation kernels).  DESIGN.md 4.3.
//
// One kernel, k_fpdw, over the layer table.  A workgroup owns a tile of TC x TC cells (TP = TC * cell pixels a side) and keeps
// everything between the BGR bytes and the cell sums in LDS:
//   A  BGR (+ gray) of the tile and a halo of cell / 2 (aggregation) + radius (normaliser) + 1 (gradient) pixels
//   B  gradient codes and LUT magnitudes M                    halo cell / 2 + radius
//   C  horizontal triangular sums of M                        rows: halo cell / 2 + radius, columns: halo cell / 2
//   D  S = tri(M) / (r + 1)^4 + k, Mn = M / S, bins, weight   halo cell / 2
//   E  horizontal aggregation taps, all ten channels          rows: halo cell / 2, one value per cell column
//   F  vertical aggregation taps, scale, store                rows x cols x 10 floats leave the workgroup
// The three filters replicate their own input at the image border, so every stage evaluates an out-of-image position AT the
// clamped position (its centre is clamped, then the neighbours are taken around that centre): the arrays hold, at every tile
// position, the value of the nearest image pixel, which is what the next stage's replicated border reads.
// Every tap is one fmaf (one rounding): with separable sums a cell value passes 2 (2r + 1) + 4 cell + 10 roundings at most.
#pragma once

struct FpdwLutEntry {   // one entry per gradient code gx | gy << 8 (FpdwFeaturesFilter.cpp:34-64)
    float magnitude, w1, w2;
    uint8_t bin1, bin2;
    uint16_t pad;
};

struct FpdwParamsDev {
    int32_t cell, radius, fast, interp, TC, perPixel;
    float k, triNorm, aggNorm;
    size_t planeStride;            // bytes between the B, G and R planes of a layer
    const FpdwLutEntry* lut;       // [65536]
    const float* gamma;            // [256] sRGB -> linear
};

namespace {

constexpr int FPDW_CHANNELS = 10;
constexpr int FPDW_BINS = 6;
constexpr size_t FPDW_LDS_BUDGET = 64 * 1024;

// host and device agree on the LDS carve-up
struct FpdwTile {
    int TP, ha, hm, hf, WF, WM, WS;
    size_t oB, oG, oR, oY, oCode, oM, oH, oMn, oW2, oBins, oT, oGamma, bytes;
};
__host__ __device__ inline FpdwTile fpdw_tile(int cell, int radius, int TC, bool perPixel) {
    FpdwTile t;
    t.TP = TC * cell;
    t.ha = perPixel ? 0 : cell / 2;   // per-pixel descriptors need no aggregation halo
    t.hm = t.ha + radius;
    t.hf = t.hm + 1;
    t.WF = t.TP + 2 * t.hf; t.WM = t.TP + 2 * t.hm; t.WS = t.TP + 2 * t.ha;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t nF = (size_t)t.WF * t.WF, nM = (size_t)t.WM * t.WM, nS = (size_t)t.WS * t.WS;
    size_t o = 0;
    t.oB = o; o = up(o + nF);
    t.oG = o; o = up(o + nF);
    t.oR = o; o = up(o + nF);
    t.oY = o; o = up(o + nF);
    t.oCode = o; o = up(o + 2 * nM);
    t.oM = o; o = up(o + 4 * nM);
    t.oH = o; o = up(o + 4 * (size_t)t.WM * t.WS);
    t.oMn = o; o = up(o + 4 * nS);
    t.oW2 = o; o = up(o + 4 * nS);
    t.oBins = o; o = up(o + nS);
    t.oT = o; o = up(o + 4 * (size_t)t.WS * TC * FPDW_CHANNELS);
    t.oGamma = o; o = up(o + 4 * 256);
    t.bytes = o;
    return t;
}

// GradientFilter(1) on CV_8U (filtering/GradientFilter.cpp:43-57): saturate_cast<uchar>((next - prev) * 0.5 + 127), cvRound = half to even
__device__ __forceinline__ int fpdw_gradient_code(int next, int prev) {
    const int v2 = next - prev + 254;            // twice the value, -1 .. 509
    const int f = (v2 - (v2 & 1)) >> 1;          // floor
    return (v2 & 1) ? f + (f & 1) : f;           // .5 goes to the even neighbour: -0.5 -> 0, 254.5 -> 254
}

// CV_BGR2Luv on floats c / 255 by OpenCV's documented formula, normalised like BgrToLuvConverter(true) (BgrToLuvConverter.cpp:89-93)
__device__ __forceinline__ void fpdw_luv(const float* __restrict__ gamma, int b, int g, int r, float& Ln, float& un, float& vn) {
    const float R = gamma[r], G = gamma[g], B = gamma[b];
    const float X = 0.412453f * R + 0.357580f * G + 0.180423f * B;
    const float Y = 0.212671f * R + 0.715160f * G + 0.072169f * B;
    const float Z = 0.019334f * R + 0.119193f * G + 0.950227f * B;
    const float L = Y > 0.008856f ? 116.f * cbrtf(Y) - 16.f : 903.3f * Y;
    const float d = fmaxf(X + 15.f * Y + 3.f * Z, 1.1920929e-07f);
    const float up = 4.f * X / d, vp = 9.f * Y / d;
    const float u = 13.f * L * (up - 0.19793943f), v = 13.f * L * (vp - 0.46831096f);
    Ln = L / 354.f;
    un = (u + 134.f) / 354.f;
    vn = (v + 140.f) / 354.f;
}

__device__ __forceinline__ int fpdw_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// weight of tap t (0 .. taps - 1) of the triangular aggregation filter: odd size 2R + 1: R + 1 - |t - R|; even size 2R + 2:
// 1, 3, .., 2R + 1, 2R + 1, .., 3, 1 (TriangularConvolutionFilter.cpp:37-69)
__device__ __forceinline__ float fpdw_agg_tap(int t, int cell) {
    if (cell & 1) return (float)(cell - abs(t - (cell - 1)));
    return (float)(t < cell ? 2 * t + 1 : 2 * (2 * cell - 1 - t) + 1);
}

__global__ __launch_bounds__(256) void k_fpdw(const FhogLayerDev* __restrict__ layers, int nLayers, FpdwParamsDev d, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char fpdw_lds[];
    const FhogLayerDev L = layers[layer_of<&FhogLayerDev::cellBlockBase>(layers, nLayers, blockIdx.x)];
    const int cell = d.cell, r = d.radius, TC = d.TC;
    const FpdwTile T = fpdw_tile(cell, r, TC, d.perPixel != 0);
    const int TP = T.TP, WF = T.WF, WM = T.WM, WS = T.WS;
    uint8_t* sB = fpdw_lds + T.oB;
    uint8_t* sG = fpdw_lds + T.oG;
    uint8_t* sR = fpdw_lds + T.oR;
    uint8_t* sY = fpdw_lds + T.oY;
    uint16_t* sCode = reinterpret_cast<uint16_t*>(fpdw_lds + T.oCode);
    float* sM = reinterpret_cast<float*>(fpdw_lds + T.oM);
    float* sH = reinterpret_cast<float*>(fpdw_lds + T.oH);
    float* sMn = reinterpret_cast<float*>(fpdw_lds + T.oMn);
    float* sW2 = reinterpret_cast<float*>(fpdw_lds + T.oW2);
    uint8_t* sBins = fpdw_lds + T.oBins;
    float* sT = reinterpret_cast<float*>(fpdw_lds + T.oT);
    float* sGamma = reinterpret_cast<float*>(fpdw_lds + T.oGamma);
    const int tid = threadIdx.x;
    const int tilesX = d.perPixel ? (L.w + TP - 1) / TP : (L.cols + TC - 1) / TC;
    const int tile = (int)blockIdx.x - L.cellBlockBase;
    const int tileY = tile / tilesX, tileX = tile - tileY * tilesX;
    const int x0 = tileX * TP, y0 = tileY * TP;   // first pixel of the tile's cells
    const int lastX = L.w - 1, lastY = L.h - 1;

    // A: the planes at clamped coordinates
    for (int i = tid; i < 256; i += 256) sGamma[i] = d.gamma[i];
    for (int i = tid; i < WF * WF; i += 256) {
        const int ly = i / WF, lx = i - ly * WF;
        const int gy = fpdw_clampi(y0 - T.hf + ly, 0, lastY), gx = fpdw_clampi(x0 - T.hf + lx, 0, lastX);
        const uint8_t* p = L.img + (size_t)gy * L.stride + gx;
        const int b = p[0], g = p[d.planeStride], rr = p[2 * d.planeStride];
        sB[i] = (uint8_t)b; sG[i] = (uint8_t)g; sR[i] = (uint8_t)rr;
        sY[i] = (uint8_t)((b * 1868 + g * 9617 + rr * 4899 + 8192) >> 14);   // GrayscaleFilter
    }
    __syncthreads();
    // B: gradient code and magnitude of the pixel nearest to every position of the M region
    for (int i = tid; i < WM * WM; i += 256) {
        const int ly = i / WM, lx = i - ly * WM;
        const int fy = fpdw_clampi(y0 - T.hm + ly, 0, lastY) - (y0 - T.hf), fx = fpdw_clampi(x0 - T.hm + lx, 0, lastX) - (x0 - T.hf);
        const int c = fy * WF + fx;
        int code;
        float mag;
        if (d.fast) {
            code = fpdw_gradient_code(sY[c + 1], sY[c - 1]) | (fpdw_gradient_code(sY[c + WF], sY[c - WF]) << 8);
            mag = d.lut[code].magnitude;
        } else {   // reduceToStrongestGradient (FpdwFeaturesFilter.cpp:83-100): B, G, R in turn, a later channel wins only with a larger magnitude
            code = fpdw_gradient_code(sB[c + 1], sB[c - 1]) | (fpdw_gradient_code(sB[c + WF], sB[c - WF]) << 8);
            mag = d.lut[code].magnitude;
            const int cg = fpdw_gradient_code(sG[c + 1], sG[c - 1]) | (fpdw_gradient_code(sG[c + WF], sG[c - WF]) << 8);
            const float mg = d.lut[cg].magnitude;
            if (mag < mg) { code = cg; mag = mg; }
            const int cr = fpdw_gradient_code(sR[c + 1], sR[c - 1]) | (fpdw_gradient_code(sR[c + WF], sR[c - WF]) << 8);
            const float mr = d.lut[cr].magnitude;
            if (mag < mr) { code = cr; mag = mr; }
        }
        sCode[i] = (uint16_t)code;
        sM[i] = mag;
    }
    __syncthreads();
    // C: horizontal pass of the (2r + 1)-tap normaliser
    if (r > 0) {
        for (int i = tid; i < WM * WS; i += 256) {
            const int ly = i / WS, lx = i - ly * WS;
            const float* m = sM + ly * WM + lx;   // position lx + r - r
            float acc = 0.f;
            for (int t = 0; t <= 2 * r; ++t) acc = fmaf((float)(r + 1 - abs(t - r)), m[t], acc);
            sH[i] = acc;
        }
        __syncthreads();
    }
    // D: normalised magnitude, bins and weight of the pixel nearest to every position of the aggregation region
    for (int i = tid; i < WS * WS; i += 256) {
        const int ly = i / WS, lx = i - ly * WS;
        const int sy = fpdw_clampi(y0 - T.ha + ly, 0, lastY) - (y0 - T.ha), sx = fpdw_clampi(x0 - T.ha + lx, 0, lastX) - (x0 - T.ha);
        const int mi = (sy + r) * WM + sx + r;
        float mn = sM[mi];
        if (r > 0) {
            const float* h = sH + sy * WS + sx;   // row sy + r - r
            float acc = 0.f;
            for (int t = 0; t <= 2 * r; ++t) acc = fmaf((float)(r + 1 - abs(t - r)), h[t * WS], acc);
            mn = mn / (acc * d.triNorm + d.k);
        }
        const FpdwLutEntry e = d.lut[sCode[mi]];
        sMn[i] = mn;
        sW2[i] = e.w2;
        sBins[i] = (uint8_t)(e.bin1 | (e.bin2 << 4));
    }
    __syncthreads();
    if (d.perPixel) {   // FpdwFeaturesFilter::applyTo: the descriptors of the tile's pixels, channel fastest
        for (int i = tid; i < TP * TP * FPDW_CHANNELS; i += 256) {
            const int p = i / FPDW_CHANNELS, ch = i - p * FPDW_CHANNELS;
            const int py = p / TP, px = p - py * TP;
            const int gy = y0 + py, gx = x0 + px;
            if (gy > lastY || gx > lastX) continue;
            const int si = (py + T.ha) * WS + px + T.ha;
            float v;
            if (ch < FPDW_BINS) {
                const float mn = sMn[si], w2 = sW2[si];
                const int b1 = sBins[si] & 15, b2 = sBins[si] >> 4;
                v = ch == b1 ? (1.f - w2) * mn : (d.interp && ch == b2 ? w2 * mn : 0.f);
            } else if (ch == FPDW_BINS) {
                v = sMn[si];
            } else {
                const int fi = (py + T.hf) * WF + px + T.hf;
                float luv[3];
                fpdw_luv(sGamma, sB[fi], sG[fi], sR[fi], luv[0], luv[1], luv[2]);
                v = ch == 7 ? luv[0] : (ch == 8 ? luv[1] : luv[2]);
            }
            out[((size_t)gy * L.w + gx) * FPDW_CHANNELS + ch] = v;
        }
        return;
    }
    // E: horizontal aggregation taps.  An item is (row, cell column, channel group): group 0 the six bins and the magnitude,
    // group 1 L*u*v*.  A bin that a pixel does not vote for receives fmaf(tap, 0, acc) == acc.
    const int taps = (cell & 1) ? 2 * cell - 1 : 2 * cell;
    for (int i = tid; i < WS * TC * 2; i += 256) {
        const int grp = i >= WS * TC, item = i - grp * WS * TC;   // the groups in separate runs of lanes
        const int row = item / TC, cc = item - row * TC;
        const int s0 = row * WS + cc * cell;      // first tap: sample cell / 2 + cc * cell, minus the filter's reach, plus the halo
        float* dst = sT + (size_t)item * FPDW_CHANNELS;
        if (grp == 0) {
            float acc[FPDW_BINS + 1];
#pragma unroll
            for (int b = 0; b <= FPDW_BINS; ++b) acc[b] = 0.f;
            for (int t = 0; t < taps; ++t) {
                const float w = fpdw_agg_tap(t, cell);
                const float mn = sMn[s0 + t], w2 = sW2[s0 + t];
                const int b1 = sBins[s0 + t] & 15, b2 = sBins[s0 + t] >> 4;
                const float v1 = (1.f - w2) * mn, v2 = w2 * mn;
#pragma unroll
                for (int b = 0; b < FPDW_BINS; ++b) acc[b] = fmaf(w, b == b1 ? v1 : (d.interp && b == b2 ? v2 : 0.f), acc[b]);
                acc[FPDW_BINS] = fmaf(w, mn, acc[FPDW_BINS]);
            }
#pragma unroll
            for (int b = 0; b <= FPDW_BINS; ++b) dst[b] = acc[b];
        } else {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            const int f0 = (row + T.hf - T.ha) * WF + cc * cell + T.hf - T.ha;
            for (int t = 0; t < taps; ++t) {
                const float w = fpdw_agg_tap(t, cell);
                float l, u, v;
                fpdw_luv(sGamma, sB[f0 + t], sG[f0 + t], sR[f0 + t], l, u, v);
                a0 = fmaf(w, l, a0); a1 = fmaf(w, u, a1); a2 = fmaf(w, v, a2);
            }
            dst[7] = a0; dst[8] = a1; dst[9] = a2;
        }
    }
    __syncthreads();
    // F: vertical taps, alpha / ((even ? 4 : 1) (R + 1)^4), store: channel fastest, then the cells of a tile row
    for (int i = tid; i < TC * TC * FPDW_CHANNELS; i += 256) {
        const int ch = i % FPDW_CHANNELS, cl = i / FPDW_CHANNELS;
        const int cr = cl / TC, cc = cl - cr * TC;
        const int gr = tileY * TC + cr, gc = tileX * TC + cc;
        if (gr >= L.rows || gc >= L.cols) continue;
        const float* src = sT + ((size_t)(cr * cell) * TC + cc) * FPDW_CHANNELS + ch;
        float acc = 0.f;
        for (int t = 0; t < taps; ++t) acc = fmaf(fpdw_agg_tap(t, cell), src[(size_t)t * TC * FPDW_CHANNELS], acc);
        out[((size_t)L.cellBase + (size_t)gr * L.cols + gc) * FPDW_CHANNELS + ch] = acc * d.aggNorm;
    }
}

// interleaved BGR -> three planes, four pixels per thread
__global__ __launch_bounds__(256) void k_bgr_planes(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ planes, size_t planeStride, int n) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (4 * q >= n) return;
    const uint8_t* s = bgr + 12 * (size_t)q;
    if (4 * q + 4 <= n) {
        uint32_t w[3];
        if (((uintptr_t)bgr & 3) == 0) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
            w[0] = s4[0]; w[1] = s4[1]; w[2] = s4[2];
        } else {
            __builtin_memcpy(w, s, 12);
        }
        // bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        const uint32_t b = (w[0] & 255u) | ((w[0] >> 24) << 8) | (((w[1] >> 16) & 255u) << 16) | (((w[2] >> 8) & 255u) << 24);
        const uint32_t g = ((w[0] >> 8) & 255u) | ((w[1] & 255u) << 8) | ((w[1] >> 24) << 16) | (((w[2] >> 16) & 255u) << 24);
        const uint32_t r = ((w[0] >> 16) & 255u) | (((w[1] >> 8) & 255u) << 8) | ((w[2] & 255u) << 16) | ((w[2] >> 24) << 24);
        reinterpret_cast<uint32_t*>(planes)[q] = b;
        reinterpret_cast<uint32_t*>(planes + planeStride)[q] = g;
        reinterpret_cast<uint32_t*>(planes + 2 * planeStride)[q] = r;
    } else {
        for (int i = 4 * q; i < n; ++i)
            for (int k = 0; k < 3; ++k) planes[k * planeStride + i] = bgr[3 * (size_t)i + k];
    }
}

// FpdwFeaturesFilter::createGradientLut with the orientation defined as (float)atan2((double)gY, (double)gX).
// Without interpolation bin2 = 0, weight1 = 1, weight2 = 0 (the reference leaves them unset).
void fpdw_build_lut(bool interpolate, std::vector<FpdwLutEntry>& lut) {
    const float PI = (float)M_PI, TWO_PI = (float)(2 * M_PI);
    const float value2bin = FPDW_BINS / PI;
    lut.assign(65536, FpdwLutEntry{});
    for (int x = 0; x < 256; ++x) {
        const float gX = (x - 127.f) / 255.f;
        for (int y = 0; y < 256; ++y) {
            const float gY = (y - 127.f) / 255.f;
            FpdwLutEntry e{};
            e.magnitude = std::sqrt(gX * gX + gY * gY);
            float o = (float)std::atan2((double)gY, (double)gX);
            if (o < 0) o += TWO_PI;
            if (o >= PI) o -= PI;
            if (interpolate) {
                const float bin = o * value2bin;
                int b1 = (int)bin, b2 = b1 + 1;
                if (b2 == FPDW_BINS) b2 = 0;
                e.bin1 = (uint8_t)b1; e.bin2 = (uint8_t)b2;
                e.w2 = 1.f * (bin - b1);
                e.w1 = 1.f - e.w2;
            } else {
                int b = (int)(o * value2bin + 0.5f);
                if (b == FPDW_BINS) b = 0;
                e.bin1 = (uint8_t)b; e.bin2 = 0; e.w1 = 1.f; e.w2 = 0.f;
            }
            lut[(size_t)x | ((size_t)y << 8)] = e;
        }
    }
}

struct FpdwScratch {
    DevBuf lut[2], gamma, img, planes, layers;   // lut[interpolate]
    bool lutValid[2] = {false, false}, gammaValid = false;
};
FpdwScratch& fpdw_scratch(fd_ctx* ctx) { return fd_scratch<FpdwScratch>(ctx); }

void check_fpdw_params(const fd_fpdw_params& fp) {
    if (fp.cell_size < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "AggregationFilter: cellSize must be bigger than zero, but was %d", fp.cell_size);
    if (fp.normalization_radius < 0)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "TriangularConvolutionFilter: size must be greater than zero, but was %d", 2 * fp.normalization_radius + 1);
    if (!(fp.normalization_constant > 0))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientMagnitudeFilter: normalizationConstant must be bigger than zero, but was %f",
                 (double)fp.normalization_constant);
}

// the unit of a tile: the cell, or, for per-pixel descriptors (where cells play no part), 8 pixels
int fpdw_tile_unit(const fd_fpdw_params& fp, bool perPixel) { return perPixel ? 8 : fp.cell_size; }

// cells a side of a workgroup's tile: the largest of 8, 4, 2, 1 whose working set fits the LDS budget
int fpdw_tile_cells(const fd_fpdw_params& fp, bool perPixel = false) {
    for (int tc = 8; tc >= 1; tc >>= 1)
        if (fpdw_tile(fpdw_tile_unit(fp, perPixel), fp.normalization_radius, tc, perPixel).bytes <= FPDW_LDS_BUDGET) return tc;
    FD_THROW(FD_ERR_INVALID_ARGUMENT, "FpdwFeaturesFilter: cell size %d with normalisation radius %d exceeds this backend's tile memory", fp.cell_size,
             fp.normalization_radius);
}

// the limits TriangularConvolutionFilter::applyTo puts on its input (TriangularConvolutionFilter.cpp:74-79): the normaliser
// (size 2r + 1, on the w x h magnitude image), then, with `aggregate`, the aggregation filter (radius cell - 1, on the w x h descriptors)
void check_fpdw_image_size(const fd_fpdw_params& fp, int w, int h, bool aggregate) {
    auto check = [&](int radius) {
        if (h <= radius) FD_THROW(FD_ERR_INVALID_ARGUMENT, "TriangularConvolutionFilter: image must have at least %d rows, but had only %d", radius + 1, h);
        if (w < 2 * radius + 2)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "TriangularConvolutionFilter: image must have at least %d columns, but had only %d", 2 * radius + 2, w);
    };
    if (fp.normalization_radius > 0) check(fp.normalization_radius);
    if (aggregate) check(fp.cell_size - 1);
}

// cellBlockBase of the first nTiled layers (laid out by layout_layers) as their first k_fpdw tile; returns the number of tiles
int fpdw_assign_tiles(std::vector<FhogLayerDev>& layers, int nTiled, int cell, int TC, bool perPixel) {
    int tiles = 0;
    for (int i = 0; i < nTiled; ++i) {
        FhogLayerDev& L = layers[i];
        L.cellBlockBase = tiles;
        const int tx = perPixel ? (L.w + TC * cell - 1) / (TC * cell) : (L.cols + TC - 1) / TC;
        const int ty = perPixel ? (L.h + TC * cell - 1) / (TC * cell) : (L.rows + TC - 1) / TC;
        tiles += tx * ty;
    }
    return tiles;
}

// k_fpdw over the first nLayers entries of the device layer table (planar layers, tiles assigned by fpdw_assign_tiles)
void run_fpdw(fd_ctx* ctx, const FhogLayerDev* dlayers, int nLayers, int tiles, size_t planeStride, const fd_fpdw_params& fp, bool perPixel, float* dout) {
    check_fpdw_params(fp);
    FpdwScratch& F = fpdw_scratch(ctx);
    const int ip = fp.interpolate != 0;
    if (!F.lutValid[ip]) {
        std::vector<FpdwLutEntry> lut;
        fpdw_build_lut(ip, lut);
        F.lut[ip].reserve(sizeof(FpdwLutEntry) * lut.size());
        HIP_CHECK(hipMemcpy(F.lut[ip].p, lut.data(), sizeof(FpdwLutEntry) * lut.size(), hipMemcpyHostToDevice));
        F.lutValid[ip] = true;
    }
    if (!F.gammaValid) {   // sRGB -> linear of c / 255, evaluated in double
        float gamma[256];
        for (int i = 0; i < 256; ++i) {
            const double c = i / 255.0;
            gamma[i] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
        }
        F.gamma.reserve(sizeof(gamma));
        HIP_CHECK(hipMemcpy(F.gamma.p, gamma, sizeof(gamma), hipMemcpyHostToDevice));
        F.gammaValid = true;
    }
    if (tiles <= 0) return;
    FpdwParamsDev d;
    std::memset(&d, 0, sizeof(d));
    const int c = fpdw_tile_unit(fp, perPixel), r = fp.normalization_radius;
    d.cell = c; d.radius = r; d.fast = fp.fast_gradient != 0; d.interp = ip; d.TC = fpdw_tile_cells(fp, perPixel); d.perPixel = perPixel;
    d.k = fp.normalization_constant;
    const float r1 = (float)(r + 1);
    d.triNorm = 1.f / (r1 * r1 * r1 * r1);                                                  // TriangularConvolutionFilter.cpp:29, alpha = 1
    d.aggNorm = (float)(c * c) / (((c & 1) ? 1.f : 4.f) * ((float)c * c * c * c));          // radius + 1 == cell for both parities
    d.planeStride = planeStride;
    d.lut = F.lut[ip].as<FpdwLutEntry>();
    d.gamma = F.gamma.as<float>();
    const FpdwTile T = fpdw_tile(c, r, d.TC, perPixel);
    hipLaunchKernelGGL(k_fpdw, dim3(tiles), dim3(256), T.bytes, ctx->stream, dlayers, nLayers, d, dout);
    HIP_CHECK(hipGetLastError());
}

// a BGR image (host or device) as three planes in F.planes; returns the plane stride
size_t fpdw_planes(fd_ctx* ctx, FpdwScratch& F, const uint8_t* image, int w, int h, int is_device) {
    const size_t npix = (size_t)w * h;
    if (npix > 0x7ffffff0ull / 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "FpdwFeaturesFilter: image too large");
    const size_t planeStride = (npix + 255) & ~(size_t)255;
    F.planes.reserve(3 * planeStride);
    const uint8_t* src = image;
    if (!is_device) {
        F.img.reserve(3 * npix);
        HIP_CHECK(hipMemcpyAsync(F.img.p, image, 3 * npix, hipMemcpyHostToDevice, ctx->stream));
        src = F.img.as<uint8_t>();
    }
    hipLaunchKernelGGL(k_bgr_planes, dim3((unsigned)((npix / 4 + 1 + 255) / 256)), dim3(256), 0, ctx->stream, src, F.planes.as<uint8_t>(), planeStride, (int)npix);
    HIP_CHECK(hipGetLastError());
    return planeStride;
}

// both stand-alone calls: the per-pixel descriptors (FpdwFeaturesFilter::applyTo) or the cells of the whole chain
void fpdw_image(fd_ctx* ctx, const uint8_t* bgr, int w, int h, const fd_fpdw_params* fp, float* out, bool perPixel) {
    if (!ctx || !bgr || !fp || !out || w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_fpdw_image: bad argument");
    check_fpdw_params(*fp);
    check_fpdw_image_size(*fp, w, h, !perPixel);
    HIP_CHECK(hipSetDevice(ctx->device));
    FpdwScratch& F = fpdw_scratch(ctx);
    FhogScratch& S = scratch(ctx);
    const size_t planeStride = fpdw_planes(ctx, F, bgr, w, h, 0);
    // the one layer's table: its first tile is tile 0, as layout_layers leaves cellBlockBase
    std::vector<FhogLayerDev> layers(1, layer_entry(F.planes.as<uint8_t>(), w, h, w, 3));
    single_layer_table(ctx, F.layers, layers[0], fp->cell_size);
    const int tiles = fpdw_assign_tiles(layers, 1, fpdw_tile_unit(*fp, perPixel), fpdw_tile_cells(*fp, perPixel), perPixel);
    const size_t n = perPixel ? (size_t)w * h * FPDW_CHANNELS : (size_t)layers[0].rows * layers[0].cols * FPDW_CHANNELS;
    if (n == 0) return;
    S.descOwner = nullptr;
    S.desc.reserve(sizeof(float) * n);
    run_fpdw(ctx, F.layers.as<FhogLayerDev>(), 1, tiles, planeStride, *fp, perPixel, S.desc.as<float>());
    HIP_CHECK(hipMemcpyAsync(out, S.desc.p, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

}  // namespace

extern "C" {

int fd_fpdw_size(const fd_fpdw_params* fp, int width, int height, int* rows, int* cols, int* channels) {
    if (!fp || fp->cell_size < 1) return FD_ERR_INVALID_ARGUMENT;
    if (rows) *rows = height / fp->cell_size;
    if (cols) *cols = width / fp->cell_size;
    if (channels) *channels = FPDW_CHANNELS;
    return FD_OK;
}

int fd_fpdw_gradient_lut(const fd_fpdw_params* fp, int32_t* bin1, int32_t* bin2, float* w1, float* w2, float* magnitude) {
    if (!fp) return FD_ERR_INVALID_ARGUMENT;
    std::vector<FpdwLutEntry> lut;
    fpdw_build_lut(fp->interpolate != 0, lut);
    for (size_t i = 0; i < lut.size(); ++i) {
        if (bin1) bin1[i] = lut[i].bin1;
        if (bin2) bin2[i] = lut[i].bin2;
        if (w1) w1[i] = lut[i].w1;
        if (w2) w2[i] = lut[i].w2;
        if (magnitude) magnitude[i] = lut[i].magnitude;
    }
    return FD_OK;
}

int fd_fpdw_image(fd_ctx* ctx, const uint8_t* bgr, int width, int height, const fd_fpdw_params* fp, float* out) {
    return fd_guard(ctx, [&] { fpdw_image(ctx, bgr, width, height, fp, out, true); });
}

int fd_fpdw_cells_image(fd_ctx* ctx, const uint8_t* bgr, int width, int height, const fd_fpdw_params* fp, float* out) {
    return fd_guard(ctx, [&] { fpdw_image(ctx, bgr, width, height, fp, out, false); });
}

}  // extern "C"
