// featuredetection_amd/csrc/integral.hip -- integral-image features on sampled windows (gfx950).
//
// Restates the reference's integral-image family: the image filters GrayscaleFilter -> IntegralImageFilter
// (IntegralImageFilter.cpp:18-21) of a DirectImageFeatureExtractor (DirectImageFeatureExtractor.cpp:35-52), and the patch filters
// HaarFeatureFilter (HaarFeatureFilter.cpp:138-158), IntegralGradientFilter (IntegralGradientFilter.cpp:23-85), GradientSumFilter
// (GradientSumFilter.cpp:22-60) and the SURF-like chain of createSurfExtractor (BenchmarkRunner.cpp:278-286), evaluated for n
// sample windows {x, y, width, height} per call, plus condensation::SingleClassifierModel::evaluate (SingleClassifierModel.cpp:32-52)
// over them.  The arithmetic is integer except for a handful of float / double operations per feature, which are written in the
// reference's order (the file is built with -ffp-contract=off): the outputs are bit-identical to the CPU path.
//
// Integral image, three launches:
//   k_integral_rows     one wavefront per image row: gray conversion (BGR input), 256 pixels per step -- four per lane, a wave64
//                       shuffle scan of the lane totals, a carry -- staged through LDS so that every store instruction writes 64
//                       consecutive ints of the row
//   k_integral_bandsum  column sums of the row prefixes over bands of 32 rows, lanes along the row
//   k_integral_cols     per band: the sums of the bands above, then a running sum down the band's rows, in place; lanes along the
//                       row, so every load / store of a wavefront covers 256 consecutive bytes
// Sample kernels: one wavefront per sample, four samples per workgroup, lanes over features / grid points / cells; the integral
// image is gathered through L2 (a 1080p integral image is 8.3 MB), every output row is written with consecutive lanes.
#include "fd_internal.hpp"
#include "fd_device.hpp"
#include "integral_geo.hpp"
#include <algorithm>
#include <cstring>

struct fd_integral {
    fd_ctx* ctx = nullptr;
    int w = 0, h = 0;            // size of the source image; the integral image is (h + 1) x (w + 1)
    bool ready = false;          // holds an integral image
    DevBuf input;                // staging for host images
    DevBuf img;                  // the integral image
    DevBuf bands;                // k_integral_bandsum's sums, one row of (w + 1) ints per band
    // the device feature table of the last Haar call (rebuilt when the parameters change)
    DevBuf haarTab;
    std::vector<float> haarKey;
    int haarTypes = -1, haarCount = 0;
    float haarMaxX = 0.f, haarMaxY = 0.f;
    // GradientBinningFilter's look-up table of the last integral HOG call (rebuilt when (bins, signed, interpolate) changes)
    DevBuf hogLut;
    int hogLutBins = -1, hogLutSigned = 0, hogLutInterpolate = 0;
    DevBuf hogRaw;               // cell histograms of the ehog kind
    // per-call device buffers
    DevBuf xywh, feat, valid, dist;
};

namespace {
using namespace fd_dev;
using namespace fd_integral_geo;

constexpr int BAND = 32;           // rows per band of the column pass

// Row pass: dst[y + 1][x + 1] = sum of gray[y][u], u <= x; dst[.][0] = 0 and row 0 = 0.  One wavefront per row.
template <int CH>
__global__ __launch_bounds__(256) void k_integral_rows(const uint8_t* __restrict__ src, int32_t* __restrict__ dst, int W, int H) {
    __shared__ int32_t stage[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t S = (size_t)W + 1;
    if (blockIdx.x == 0)
        for (int x = threadIdx.x; x <= W; x += 256) dst[x] = 0;
    for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
        const uint8_t* __restrict__ s = src + (size_t)y * W * CH;
        int32_t* __restrict__ d = dst + (size_t)(y + 1) * S;
        if (lane == 0) d[0] = 0;
        int carry = 0;
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + 4 * lane;
            int v[4] = {0, 0, 0, 0};
            if (x + 3 < W) {
                if (CH == 3) {   // bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
                    const uint32_t a = ld_u32_unaligned(s + 3 * (size_t)x), b = ld_u32_unaligned(s + 3 * (size_t)x + 4), c = ld_u32_unaligned(s + 3 * (size_t)x + 8);
                    v[0] = (int)gray_of(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
                    v[1] = (int)gray_of(a >> 24, b & 255u, (b >> 8) & 255u);
                    v[2] = (int)gray_of((b >> 16) & 255u, b >> 24, c & 255u);
                    v[3] = (int)gray_of((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
                } else {
                    const uint32_t a = ld_u32_unaligned(s + x);
                    v[0] = (int)(a & 255u); v[1] = (int)((a >> 8) & 255u); v[2] = (int)((a >> 16) & 255u); v[3] = (int)(a >> 24);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k < W) v[k] = CH == 3 ? (int)gray_of(s[3 * (size_t)(x + k)], s[3 * (size_t)(x + k) + 1], s[3 * (size_t)(x + k) + 2]) : (int)s[x + k];
            }
            v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
            int incl = v[3];   // inclusive prefix over lanes of the per-lane totals (integer: order-free)
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            const int before = carry + incl - v[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) stage[wave][4 * lane + k] = before + v[k];
            carry += __shfl(incl, 63, 64);
            wave_sync();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xo = x0 + k * 64 + lane;
                if (xo < W) d[1 + xo] = stage[wave][k * 64 + lane];
            }
            wave_sync();
        }
    }
}

// Column pass, first half: bands[b][x] = sum of the row prefixes img[y][x] over the rows 1 + b BAND .. of band b.  blockIdx.y = band.
__global__ __launch_bounds__(64) void k_integral_bandsum(const int32_t* __restrict__ img, int32_t* __restrict__ bands, int W, int H) {
    const int x = 1 + blockIdx.x * 64 + threadIdx.x;
    if (x > W) return;
    const size_t S = (size_t)W + 1;
    const int y0 = 1 + blockIdx.y * BAND, y1 = min(y0 + BAND, H + 1);
    int acc = 0;
#pragma unroll 8
    for (int y = y0; y < y1; ++y) acc += img[(size_t)y * S + x];
    bands[(size_t)blockIdx.y * S + x] = acc;
}

// Column pass, second half: the running sum down the rows of band blockIdx.y, started with the sums of the bands above; in place.
__global__ __launch_bounds__(64) void k_integral_cols(int32_t* __restrict__ img, const int32_t* __restrict__ bands, int W, int H) {
    const int x = 1 + blockIdx.x * 64 + threadIdx.x;
    if (x > W) return;
    const size_t S = (size_t)W + 1;
    const int y0 = 1 + blockIdx.y * BAND, y1 = min(y0 + BAND, H + 1);
    int acc = 0;
#pragma unroll 4
    for (int b = 0; b < (int)blockIdx.y; ++b) acc += bands[(size_t)b * S + x];
#pragma unroll 8
    for (int y = y0; y < y1; ++y) {
        acc += img[(size_t)y * S + x];
        img[(size_t)y * S + x] = acc;
    }
}

// ---- sample windows: DirectImageFeatureExtractor::extract (DirectImageFeatureExtractor.cpp:42-52) on the integral image; sample_geo,
// grad_geo and grad_point are integral_geo.hpp's ----
// HaarFeatureFilter: one feature of the device table.  xe / ye hold rect.x + rect.width / rect.y + rect.height (float sums, made
// on the host exactly as applyTo makes them), fa = factor * area.
struct HaarDev {
    float x[4], xe[4], y[4], ye[4], wt[4];
    float fa;
    int32_t n;
    int32_t pad[2];
};

// HaarFeatureFilter::applyTo (HaarFeatureFilter.cpp:138-158).  maxX / maxY: the largest rectangle edges of the table -- cvRound(edge *
// size) is monotonic in the edge, so they decide whether any read of the sample leaves the integral image.
__global__ __launch_bounds__(256) void k_haar(const int32_t* __restrict__ img, int W, int H, const HaarDev* __restrict__ tab, int F, float maxX,
                                              float maxY, const int32_t* __restrict__ xywh, int n, float* __restrict__ feat, uint8_t* __restrict__ valid) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t S = (size_t)W + 1;
    for (int s = blockIdx.x * 4 + wave; s < n; s += gridDim.x * 4) {
        const SampleGeo g = sample_geo(xywh, s, W, H);
        const float fc = (float)g.w, fr = (float)g.h;   // image.cols, image.rows of the patch
        bool ok = g.exists;
        if (ok) ok = (long long)g.px0 + __float2int_rn(maxX * fc) <= W && (long long)g.py0 + __float2int_rn(maxY * fr) <= H;
        if (lane == 0) valid[s] = ok ? 1 : 0;
        float* __restrict__ out = feat + (size_t)s * F;
        if (!ok) {
            for (int f = lane; f < F; f += 64) out[f] = 0.f;
            continue;
        }
        const int32_t* __restrict__ base = img + (size_t)g.py0 * S + g.px0;
        for (int f = lane; f < F; f += 64) {
            const HaarDev t = tab[f];
            float value = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < t.n) {
                    const int x1 = __float2int_rn(t.x[j] * fc);    // cvRound(rect.x * image.cols): float product, half to even
                    const int x2 = __float2int_rn(t.xe[j] * fc);
                    const int y1 = __float2int_rn(t.y[j] * fr);
                    const int y2 = __float2int_rn(t.ye[j] * fr);
                    const int areaSum = base[(size_t)y1 * S + x1] + base[(size_t)y2 * S + x2] - base[(size_t)y1 * S + x2] - base[(size_t)y2 * S + x1];
                    value += t.wt[j] * (float)areaSum;
                }
            }
            out[f] = value / (t.fa * fc * fr);
        }
    }
}

__global__ __launch_bounds__(256) void k_grad_patches(const int32_t* __restrict__ img, int W, int H, int rows, int cols, const int32_t* __restrict__ xywh,
                                                      int n, uchar2* __restrict__ dst, uint8_t* __restrict__ valid) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t S = (size_t)W + 1;
    const int cells = rows * cols;
    for (int s = blockIdx.x * 4 + wave; s < n; s += gridDim.x * 4) {
        const SampleGeo g = sample_geo(xywh, s, W, H);
        const GradGeo q = grad_geo(g, rows, cols, W, H);
        if (lane == 0) valid[s] = q.ok ? 1 : 0;
        uchar2* __restrict__ out = dst + (size_t)s * cells;
        if (!q.ok) {
            for (int i = lane; i < cells; i += 64) out[i] = make_uchar2(0, 0);
            continue;
        }
        const int32_t* __restrict__ base = img + (size_t)g.py0 * S + g.px0;
        for (int i = lane; i < cells; i += 64) out[i] = grad_point(base, S, q, i / cols, i % cols);
    }
}

// GradientSumFilter::applyTo (GradientSumFilter.cpp:22-60) of one cell of a rows x cols CV_8UC2 patch: the four sums, added in j
// (rows) then i (columns) order
__device__ __forceinline__ float4 gradient_sum_cell(const uchar2* grad, int cols, int row, int col, int cellH, int cellW) {
    const float normalizer = 1.f / 127.f;
    float sdx = 0.f, sdy = 0.f, sadx = 0.f, sady = 0.f;
    for (int j = 0; j < cellH; ++j)
        for (int i = 0; i < cellW; ++i) {
            const uchar2 gr = grad[(size_t)(row * cellH + j) * cols + col * cellW + i];
            const float dx = normalizer * (float)((int)gr.x - 127);
            const float dy = normalizer * (float)((int)gr.y - 127);
            sdx += dx;
            sdy += dy;
            sadx += fabsf(dx);
            sady += fabsf(dy);
        }
    return make_float4(sdx, sdy, sadx, sady);
}

// one lane per cell of every patch
__global__ __launch_bounds__(256) void k_gradient_sum(const uchar2* __restrict__ grad, int64_t n, int rows, int cols, int cellRows, int cellCols,
                                                      float4* __restrict__ dst) {
    const int per = cellRows * cellCols;
    const int64_t total = n * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t im = i / per;
        const int cell = (int)(i - im * per);
        dst[i] = gradient_sum_cell(grad + (size_t)im * rows * cols, cols, cell / cellCols, cell % cellCols, rows / cellRows, cols / cellCols);
    }
}

// IntegralGradientFilter(G) -> GradientSumFilter(C) -> UnitNormFilter(NORM_L2), one wavefront per sample; the gradient patch and the
// unnormalised descriptor live in the wavefront's share of the LDS: [G * G uchar2, padded to 16 bytes | 4 C C floats]
__global__ __launch_bounds__(256) void k_surf(const int32_t* __restrict__ img, int W, int H, int G, int C, const int32_t* __restrict__ xywh, int n,
                                              float* __restrict__ feat, uint8_t* __restrict__ valid) {
    extern __shared__ __align__(16) unsigned char surfLds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t S = (size_t)W + 1;
    const int points = G * G, len = 4 * C * C;
    const size_t gradBytes = ((size_t)points * 2 + 15) & ~(size_t)15;
    unsigned char* mine = surfLds + (size_t)wave * (gradBytes + (size_t)len * 4);
    uchar2* grad = reinterpret_cast<uchar2*>(mine);
    float* desc = reinterpret_cast<float*>(mine + gradBytes);
    for (int s = blockIdx.x * 4 + wave; s < n; s += gridDim.x * 4) {
        const SampleGeo g = sample_geo(xywh, s, W, H);
        const GradGeo q = grad_geo(g, G, G, W, H);
        if (lane == 0) valid[s] = q.ok ? 1 : 0;
        float* __restrict__ out = feat + (size_t)s * len;
        if (!q.ok) {
            for (int i = lane; i < len; i += 64) out[i] = 0.f;
            continue;
        }
        const int32_t* __restrict__ base = img + (size_t)g.py0 * S + g.px0;
        for (int i = lane; i < points; i += 64) grad[i] = grad_point(base, S, q, i / G, i % G);
        wave_sync();
        for (int cell = lane; cell < C * C; cell += 64) reinterpret_cast<float4*>(desc)[cell] = gradient_sum_cell(grad, G, cell / C, cell % C, G / C, G / C);
        wave_sync();
        unit_norm_wave(desc, out, len, 4 /* cv::NORM_L2 */, lane);
        wave_sync();
    }
}

// the samples of a resident particle set (fd_particle_sample) into the sample list the kernels above read; `trace` keeps a copy for
// fd_particles_get_trace
__global__ __launch_bounds__(256) void k_particles_xywh(const int32_t* __restrict__ x, const int32_t* __restrict__ y, const int32_t* __restrict__ size, int n,
                                                        double aspect, FdSampleMaps maps, int4* __restrict__ xywh, int4* __restrict__ trace) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t sx, sy, sw, sh;
    fd_particle_sample(x[i], y[i], size[i], aspect, maps, sx, sy, sw, sh);
    const int4 s = make_int4(sx, sy, sw, sh);
    xywh[i] = s;
    trace[i] = s;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
int sample_grid(fd_ctx* ctx, int n) { return std::max(1, std::min((n + 3) / 4, ctx->num_cus * 32)); }

void check_size(int w, int h, const char* who) {
    if (w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: image size %d x %d", who, w, h);
    if (fd_integral_image_length(w, h) < 0)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: a %d x %d image can overflow the 32-bit sums of the integral image (255 * width * height > 2^31 - 1)", who, w, h);
}

// the three launches; src: device image with ch channels, dst: (h + 1) x (w + 1) ints
void launch_integral(fd_ctx* ctx, const uint8_t* src, int w, int h, int ch, int32_t* dst, DevBuf& bands) {
    const int nb = (h + BAND - 1) / BAND;
    bands.reserve(sizeof(int32_t) * (size_t)nb * (w + 1));
    const int rowBlocks = std::min((h + 3) / 4, 8192);
    if (ch == 3) hipLaunchKernelGGL(k_integral_rows<3>, dim3(rowBlocks), dim3(256), 0, ctx->stream, src, dst, w, h);
    else hipLaunchKernelGGL(k_integral_rows<1>, dim3(rowBlocks), dim3(256), 0, ctx->stream, src, dst, w, h);
    const dim3 grid((w + 63) / 64, nb);
    hipLaunchKernelGGL(k_integral_bandsum, grid, dim3(64), 0, ctx->stream, dst, bands.as<int32_t>(), w, h);
    hipLaunchKernelGGL(k_integral_cols, grid, dim3(64), 0, ctx->stream, dst, bands.as<int32_t>(), w, h);
    HIP_CHECK(hipGetLastError());
}

void require_updated(const fd_ctx* ctx, const fd_integral* g, const char* who) {
    if (g->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the integral image belongs to another context", who);
    if (!g->ready) FD_THROW(FD_ERR_RUNTIME, "%s: the integral image has not been updated with an image (fd_integral_update)", who);
}

void upload_samples(fd_ctx* ctx, fd_integral* g, int n, const int32_t* xywh) {
    HIP_CHECK(hipSetDevice(ctx->device));
    g->xywh.reserve(sizeof(int32_t) * 4 * (size_t)n);
    g->valid.reserve((size_t)n);
    HIP_CHECK(hipMemcpyAsync(g->xywh.p, xywh, sizeof(int32_t) * 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
}

void download_rows(fd_ctx* ctx, fd_integral* g, int n, void* rows, size_t rowBytes, uint8_t* valid) {
    if (rows) HIP_CHECK(hipMemcpyAsync(rows, g->feat.p, rowBytes * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (valid) HIP_CHECK(hipMemcpyAsync(valid, g->valid.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (rows || valid) HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// the device feature table of hp (kept until the parameters change); returns the feature count
int prepare_haar(fd_ctx* ctx, fd_integral* g, const fd_haar_params* hp) {
    static const char* const invalid = "HaarFeatureFilter: invalid parameters (NULL, a negative count, types outside 1|2|4|8, or a rectangle edge outside [0, 1])";
    if (!hp || hp->num_sizes < 0 || hp->num_xs < 0 || hp->num_ys < 0 || (hp->num_sizes > 0 && !hp->sizes) || (hp->num_xs > 0 && !hp->xs) ||
        (hp->num_ys > 0 && !hp->ys))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s", invalid);
    // the key first: the table of the previous call is kept while the parameters stay the same (only valid parameters ever set a key)
    std::vector<float> key;
    key.push_back((float)hp->num_sizes); key.push_back((float)hp->num_xs);
    key.insert(key.end(), hp->sizes, hp->sizes + hp->num_sizes);
    key.insert(key.end(), hp->xs, hp->xs + hp->num_xs);
    key.insert(key.end(), hp->ys, hp->ys + hp->num_ys);
    const bool same = g->haarTypes == hp->types && key.size() == g->haarKey.size() &&
                      std::memcmp(key.data(), g->haarKey.data(), key.size() * sizeof(float)) == 0;
    if (same) return g->haarCount;
    std::vector<fd_haar_feature> features;
    if (!fd_host_haar_features(hp, features)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s", invalid);
    std::vector<HaarDev> tab(features.size());
    float maxX = 0.f, maxY = 0.f;
    for (size_t i = 0; i < features.size(); ++i) {
        const fd_haar_feature& f = features[i];
        HaarDev& t = tab[i];
        std::memset(&t, 0, sizeof(t));
        t.n = f.num_rects;
        t.fa = f.factor * f.area;
        for (int j = 0; j < f.num_rects; ++j) {
            t.x[j] = f.rects[j][0]; t.xe[j] = f.rects[j][0] + f.rects[j][2];
            t.y[j] = f.rects[j][1]; t.ye[j] = f.rects[j][1] + f.rects[j][3];
            t.wt[j] = f.weights[j];
            maxX = std::max(maxX, std::max(t.x[j], t.xe[j]));
            maxY = std::max(maxY, std::max(t.y[j], t.ye[j]));
        }
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));   // a kernel still reading the previous table
    g->haarTab.reserve(sizeof(HaarDev) * std::max<size_t>(tab.size(), 1));
    if (!tab.empty()) HIP_CHECK(hipMemcpy(g->haarTab.p, tab.data(), sizeof(HaarDev) * tab.size(), hipMemcpyHostToDevice));
    g->haarKey = key; g->haarTypes = hp->types; g->haarCount = (int)tab.size(); g->haarMaxX = maxX; g->haarMaxY = maxY;
    return g->haarCount;
}

// features of the n uploaded samples, by the table prepare_haar made (F features), into g->feat / g->valid
void run_haar(fd_ctx* ctx, fd_integral* g, int F, int n) {
    g->feat.reserve(sizeof(float) * std::max<size_t>((size_t)n * F, 1));
    hipLaunchKernelGGL(k_haar, dim3(sample_grid(ctx, n)), dim3(256), 0, ctx->stream, g->img.as<int32_t>(), g->w, g->h, g->haarTab.as<HaarDev>(), F,
                       g->haarMaxX, g->haarMaxY, g->xywh.as<int32_t>(), n, g->feat.as<float>(), g->valid.as<uint8_t>());
    HIP_CHECK(hipGetLastError());
}

// the look-up table of hp's GradientBinningFilter on the device (kept until (bins, signed, interpolate) changes)
const uint8_t* prepare_hog_lut(fd_ctx* ctx, fd_integral* g, const fd_integral_hog_params* hp) {
    const int sg = hp->signed_gradients ? 1 : 0, ib = hp->interpolate_bins ? 1 : 0;
    if (g->hogLutBins == hp->bins && g->hogLutSigned == sg && g->hogLutInterpolate == ib) return g->hogLut.as<uint8_t>();
    std::vector<uint8_t> lut;
    fd_build_gradient_lut(hp->bins, sg != 0, ib != 0, lut);
    HIP_CHECK(hipSetDevice(ctx->device));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));   // a kernel still reading the previous table
    g->hogLutBins = -1;
    g->hogLut.reserve(lut.size());
    HIP_CHECK(hipMemcpy(g->hogLut.p, lut.data(), lut.size(), hipMemcpyHostToDevice));
    g->hogLutBins = hp->bins; g->hogLutSigned = sg; g->hogLutInterpolate = ib;
    return g->hogLut.as<uint8_t>();
}

// features of the n uploaded samples into g->feat / g->valid
void run_hog(fd_ctx* ctx, fd_integral* g, const fd_integral_hog_params* hp, int n) {
    const uint8_t* lut = prepare_hog_lut(ctx, g, hp);
    fd_integral_hog_launch(ctx, hp, g->img.as<int32_t>(), g->w, g->h, lut, g->xywh.as<int32_t>(), n, g->hogRaw, g->feat, g->valid.as<uint8_t>());
}

// the rules of fd_surf_feature_length, with a message for each; returns the descriptor length
int check_surf(int G, int C) {
    const int len = fd_surf_feature_length(G, C);
    if (len >= 0) return len;
    if (G < 2 || G > FD_SURF_MAX_GRID) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_extract_surf: gradient count %d outside 2..%d", G, FD_SURF_MAX_GRID);
    if (C < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_extract_surf: cell count %d", C);
    if (G % C != 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientSumFilter: image row count (%d) is not divisible by cell count (%d)", G, C);
    FD_THROW(FD_ERR_INVALID_ARGUMENT,
             "fd_integral_extract_surf: gradient count %d with cell count %d needs %zu bytes of LDS per workgroup, more than the %zu there are "
             "(use the stand-alone calls fd_integral_gradient_patches, fd_gradient_sum_batch, fd_unit_norm_batch)",
             G, C, fd_host_surf_lds_bytes(G, C), FD_SURF_LDS_BUDGET);
}

int run_surf(fd_ctx* ctx, fd_integral* g, int G, int C, int n) {
    const int len = check_surf(G, C);
    g->feat.reserve(sizeof(float) * (size_t)n * len);
    // four wavefronts of [G G uchar2, padded to 16 bytes | 4 C C floats]: 2.1 KB at (12, 4), 96 KB at (64, 32); check_surf keeps
    // it inside the budget (C == G: up to 47)
    const size_t lds = fd_host_surf_lds_bytes(G, C);
    static uint64_t ldsAllowed = 0;
    fd_allow_lds(ctx, (const void*)k_surf, (int)FD_SURF_LDS_BUDGET, ldsAllowed);
    hipLaunchKernelGGL(k_surf, dim3(sample_grid(ctx, n)), dim3(256), lds, ctx->stream, g->img.as<int32_t>(), g->w, g->h, G, C, g->xywh.as<int32_t>(), n,
                       g->feat.as<float>(), g->valid.as<uint8_t>());
    HIP_CHECK(hipGetLastError());
    return len;
}

// The two halves of a scoring call on any integral kind.  integral_prepare: the kind, the image and the parameters checked, the
// Haar table on the device; returns the feature length.  integral_run: the features of the n samples in g->xywh into g->feat / g->valid
int integral_prepare(fd_ctx* ctx, fd_integral* g, int kind, const void* params, const char* who) {
    if (kind != FD_INTEGRAL_HAAR && kind != FD_INTEGRAL_SURF && kind != FD_INTEGRAL_HOG) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown feature kind %d", who, kind);
    require_updated(ctx, g, who);
    if (kind == FD_INTEGRAL_HAAR) return prepare_haar(ctx, g, (const fd_haar_params*)params);
    if (kind == FD_INTEGRAL_HOG) return fd_integral_hog_check((const fd_integral_hog_params*)params);
    const fd_surf_params* sp = (const fd_surf_params*)params;
    return check_surf(sp->gradient_count, sp->cell_count);
}
void integral_run(fd_ctx* ctx, fd_integral* g, int kind, const void* params, int len, int n) {
    const fd_surf_params* sp = (const fd_surf_params*)params;
    if (kind == FD_INTEGRAL_HAAR) run_haar(ctx, g, len, n);
    else if (kind == FD_INTEGRAL_HOG) run_hog(ctx, g, (const fd_integral_hog_params*)params, n);
    else run_surf(ctx, g, sp->gradient_count, sp->cell_count, n);
}

}  // namespace

extern "C" {

int fd_integral_create(fd_ctx* ctx, fd_integral** out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_create: NULL argument");
        fd_integral* g = new fd_integral();
        g->ctx = ctx;
        *out = g;
    });
}

void fd_integral_destroy(fd_integral* g) { delete g; }

int fd_integral_update(fd_integral* g, const uint8_t* image, int width, int height, int channels, int is_device) {
    return fd_guard(g ? g->ctx : nullptr, [&] {
        if (!g || !image) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_update: NULL argument");
        if (channels != 1 && channels != 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_update: channels must be 1 or 3 (got %d)", channels);
        check_size(width, height, "fd_integral_update");
        fd_ctx* ctx = g->ctx;
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t bytes = (size_t)width * height * channels;
        const uint8_t* src = image;
        if (!is_device) {
            g->input.reserve(bytes);
            HIP_CHECK(hipMemcpyAsync(g->input.p, image, bytes, hipMemcpyHostToDevice, ctx->stream));
            src = g->input.as<uint8_t>();
        }
        g->ready = false;
        g->img.reserve(sizeof(int32_t) * (size_t)(width + 1) * (height + 1));
        launch_integral(ctx, src, width, height, channels, g->img.as<int32_t>(), g->bands);
        if (!is_device) HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the caller's buffer is free again
        g->w = width; g->h = height; g->ready = true;
    });
}

int fd_integral_set_image(fd_integral* g, const int32_t* integral, int width, int height) {
    return fd_guard(g ? g->ctx : nullptr, [&] {
        if (!g || !integral || width < 1 || height < 1 || (long long)width * height > 2147483647LL) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_set_image: bad argument");
        fd_ctx* ctx = g->ctx;
        HIP_CHECK(hipSetDevice(ctx->device));
        g->ready = false;
        const size_t bytes = sizeof(int32_t) * (size_t)width * height;
        g->img.reserve(bytes);
        HIP_CHECK(hipMemcpyAsync(g->img.p, integral, bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        g->w = width - 1; g->h = height - 1; g->ready = true;
    });
}

int fd_integral_size(const fd_integral* g, int* width, int* height) {
    if (!g || !width || !height) return FD_ERR_INVALID_ARGUMENT;
    *width = g->ready ? g->w + 1 : 0;
    *height = g->ready ? g->h + 1 : 0;
    return FD_OK;
}

int fd_integral_download(fd_integral* g, int32_t* host_dst) {
    return fd_guard(g ? g->ctx : nullptr, [&] {
        if (!g || !host_dst) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_download: NULL argument");
        require_updated(g->ctx, g, "fd_integral_download");
        HIP_CHECK(hipSetDevice(g->ctx->device));
        HIP_CHECK(hipMemcpyAsync(host_dst, g->img.p, sizeof(int32_t) * (size_t)(g->w + 1) * (g->h + 1), hipMemcpyDeviceToHost, g->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
    });
}

int fd_integral_image(fd_ctx* ctx, const uint8_t* gray, int width, int height, int32_t* dst) {
    return fd_guard(ctx, [&] {
        if (!ctx || !gray || !dst) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_image: NULL argument");
        check_size(width, height, "fd_integral_image");
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = (size_t)width * height, ib = sizeof(int32_t) * (size_t)(width + 1) * (height + 1);
        DevBuf in, out, bands;
        in.reserve(n);
        out.reserve(ib);
        HIP_CHECK(hipMemcpyAsync(in.p, gray, n, hipMemcpyHostToDevice, ctx->stream));
        launch_integral(ctx, in.as<uint8_t>(), width, height, 1, out.as<int32_t>(), bands);
        HIP_CHECK(hipMemcpyAsync(dst, out.p, ib, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_integral_extract_haar(fd_ctx* ctx, fd_integral* g, const fd_haar_params* hp, int n, const int32_t* xywh, float* features, uint8_t* valid) {
    return fd_guard(ctx, [&] {
        if (!ctx || !g || !hp || n < 0 || (n > 0 && !xywh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_extract_haar: bad argument");
        const int F = integral_prepare(ctx, g, FD_INTEGRAL_HAAR, hp, "fd_integral_extract_haar");
        if (n == 0) return;
        upload_samples(ctx, g, n, xywh);
        integral_run(ctx, g, FD_INTEGRAL_HAAR, hp, F, n);
        download_rows(ctx, g, n, F ? features : nullptr, sizeof(float) * (size_t)F, valid);
    });
}

int fd_integral_gradient_patches(fd_ctx* ctx, fd_integral* g, int rows, int cols, int n, const int32_t* xywh, uint8_t* dst2ch, uint8_t* valid) {
    return fd_guard(ctx, [&] {
        if (!ctx || !g || n < 0 || (n > 0 && !xywh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_gradient_patches: bad argument");
        if (fd_integral_gradient_length(rows, cols) < 0)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "IntegralGradientFilter: rows and cols must be at least 2 and at most %d (got %d x %d)", FD_GRADIENT_MAX_GRID, rows, cols);
        require_updated(ctx, g, "fd_integral_gradient_patches");
        if (n == 0) return;
        upload_samples(ctx, g, n, xywh);
        const size_t rowBytes = (size_t)rows * cols * 2;
        g->feat.reserve(rowBytes * (size_t)n);
        hipLaunchKernelGGL(k_grad_patches, dim3(sample_grid(ctx, n)), dim3(256), 0, ctx->stream, g->img.as<int32_t>(), g->w, g->h, rows, cols,
                           g->xywh.as<int32_t>(), n, g->feat.as<uchar2>(), g->valid.as<uint8_t>());
        HIP_CHECK(hipGetLastError());
        download_rows(ctx, g, n, dst2ch, rowBytes, valid);
    });
}

int fd_gradient_sum_batch(fd_ctx* ctx, const uint8_t* grad2ch, int64_t n, int rows, int cols, int cell_rows, int cell_cols, float* dst) {
    return fd_guard(ctx, [&] {
        if (!ctx || n < 0 || rows < 1 || cols < 1 || cell_rows < 1 || cell_cols < 1 || (n > 0 && (!grad2ch || !dst)))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_gradient_sum_batch: bad argument");
        if (rows % cell_rows != 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientSumFilter: image row count (%d) is not divisible by cell count (%d)", rows, cell_rows);
        if (cols % cell_cols != 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientSumFilter: image column count (%d) is not divisible by cell count (%d)", cols, cell_cols);
        if (fd_gradient_sum_length(rows, cols, cell_rows, cell_cols) < 0)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_gradient_sum_batch: %d x %d patches are larger than %d x %d", rows, cols, FD_GRADIENT_MAX_GRID, FD_GRADIENT_MAX_GRID);
        if (n == 0) return;
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t ib = (size_t)n * rows * cols * 2, ob = sizeof(float) * 4 * (size_t)n * cell_rows * cell_cols;
        DevBuf in, out;
        in.reserve(ib);
        out.reserve(ob);
        HIP_CHECK(hipMemcpyAsync(in.p, grad2ch, ib, hipMemcpyHostToDevice, ctx->stream));
        const int64_t total = n * cell_rows * cell_cols;
        hipLaunchKernelGGL(k_gradient_sum, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 65535)), dim3(256), 0, ctx->stream, in.as<uchar2>(), n, rows, cols,
                           cell_rows, cell_cols, out.as<float4>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(dst, out.p, ob, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_integral_extract_surf(fd_ctx* ctx, fd_integral* g, int gradient_count, int cell_count, int n, const int32_t* xywh, float* features, uint8_t* valid) {
    return fd_guard(ctx, [&] {
        if (!ctx || !g || n < 0 || (n > 0 && !xywh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_extract_surf: bad argument");
        check_surf(gradient_count, cell_count);
        require_updated(ctx, g, "fd_integral_extract_surf");
        if (n == 0) return;
        upload_samples(ctx, g, n, xywh);
        const int len = run_surf(ctx, g, gradient_count, cell_count, n);
        download_rows(ctx, g, n, features, sizeof(float) * (size_t)len, valid);
    });
}

int fd_integral_gradient_samples_valid(int width, int height, int rows, int cols, int n, const int32_t* xywh, uint8_t* valid) {
    if (width < 1 || height < 1 || fd_integral_gradient_length(rows, cols) < 0 || n < 0 || (n > 0 && (!xywh || !valid))) return FD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) {
        alignas(16) int32_t s[4];   // sample_geo reads an aligned int4
        std::memcpy(s, xywh + 4 * (size_t)i, sizeof(s));
        valid[i] = grad_geo(sample_geo(s, 0, width, height), rows, cols, width, height).ok ? 1 : 0;
    }
    return FD_OK;
}

int fd_integral_extract_hog(fd_ctx* ctx, fd_integral* g, const fd_integral_hog_params* hp, int n, const int32_t* xywh, float* features, uint8_t* valid) {
    return fd_guard(ctx, [&] {
        if (!ctx || !g || !hp || n < 0 || (n > 0 && !xywh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_extract_hog: bad argument");
        const int len = fd_integral_hog_check(hp);
        require_updated(ctx, g, "fd_integral_extract_hog");
        if (n == 0) return;
        upload_samples(ctx, g, n, xywh);
        run_hog(ctx, g, hp, n);
        download_rows(ctx, g, n, features, sizeof(float) * (size_t)len, valid);
    });
}

int fd_integral_svm_evaluate_samples(fd_ctx* ctx, fd_integral* g, int kind, const void* params, const fd_svm* svm, int n, const int32_t* xywh,
                                     uint8_t* target, double* weight) {
    return fd_guard(ctx, [&] {
        if (!ctx || !g || !params || !svm || n < 0 || (n > 0 && (!xywh || !target || !weight)))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_integral_svm_evaluate_samples: bad argument");
        const int len = integral_prepare(ctx, g, kind, params, "fd_integral_svm_evaluate_samples");
        fd_samples_require_f32_svm(svm, len, "fd_integral_svm_evaluate_samples");
        if (n == 0) return;
        upload_samples(ctx, g, n, xywh);
        integral_run(ctx, g, kind, params, len, n);
        std::vector<double> dist(n);   // the validity comes from the kernels: no sampleOf
        fd_samples_svm_tail(ctx, svm, g->feat.p, len, n, g->dist, dist.data(), nullptr, g->valid.p, target, weight, nullptr);
    });
}

int fd_particles_evaluate_integral(fd_ctx* ctx, fd_particles* p, fd_integral* g, int kind, const void* params, const fd_svm* svm, double aspect_ratio,
                                   const fd_sample_map* maps, int n_maps) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_evaluate_integral";
        if (!ctx || !p || !g || !params || !svm) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        const FdSampleMaps chain = fd_sample_maps_checked(maps, n_maps, 1u << FD_SAMPLE_MAP_RESIZE | 1u << FD_SAMPLE_MAP_INTEGRAL, who);
        const FdParticlesView v = fd_particles_view(ctx, p, who);
        const int len = integral_prepare(ctx, g, kind, params, who);
        fd_samples_require_f32_svm(svm, len, who);
        const int n = v.n;
        if (n > 0) {
            g->xywh.reserve(sizeof(int32_t) * 4 * (size_t)n);
            g->valid.reserve((size_t)n);
            hipLaunchKernelGGL(k_particles_xywh, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, v.x, v.y, v.size, n, aspect_ratio, chain, g->xywh.as<int4>(),
                               (int4*)v.windows);
            HIP_CHECK(hipGetLastError());
            integral_run(ctx, g, kind, params, len, n);
            fd_svm_generic_launch(ctx, svm, g->feat.p, nullptr, (int64_t)len * 4, n, v.score);
            HIP_CHECK(hipMemcpyAsync(v.valid, g->valid.p, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        }
        fd_particles_set_evaluated(p);
    });
}

int fd_particles_state_examples_integral(fd_ctx* ctx, fd_particles* p, fd_flow* flow, fd_integral* g, int kind, const void* params, double aspect_ratio,
                                         const fd_sample_map* maps, int n_maps, const fd_particles_examples_params* examples_params, fd_particles_info* info,
                                         fd_flow_motion_info* motion, int* n_pos, fd_particles_example* pos, int* n_neg, fd_particles_example* neg, float* rows,
                                         int row_capacity, int* row_length) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_state_examples_integral";
        if (!ctx || !p || !g || !params) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
        const FdExamplesArgs a{flow, examples_params, info, motion, n_pos, n_neg, pos, neg, rows, row_capacity, row_length};
        fd_particles_examples_check(ctx, p, a, who);
        const FdSampleMaps chain = fd_sample_maps_checked(maps, n_maps, 1u << FD_SAMPLE_MAP_RESIZE | 1u << FD_SAMPLE_MAP_INTEGRAL, who);
        const int len = integral_prepare(ctx, g, kind, params, who);
        const int slots = 2 * examples_params->max_count;   // the launch size does not depend on what was chosen
        g->xywh.reserve(sizeof(int32_t) * 4 * (size_t)slots);
        g->valid.reserve((size_t)slots);
        const FdExamplesRun run = fd_particles_examples_begin(ctx, p, a, len, who);
        fd_particles_examples_xywh(ctx, p, a, aspect_ratio, chain, g->xywh.as<int32_t>());
        integral_run(ctx, g, kind, params, len, slots);
        if (len > 0) HIP_CHECK(hipMemcpyAsync(run.rows, g->feat.p, sizeof(float) * (size_t)len * slots, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(run.valid, g->valid.p, (size_t)slots, hipMemcpyDeviceToDevice, ctx->stream));
        fd_particles_examples_end(ctx, p, a, len, who);
    });
}

}  // extern "C"
