// featuredetection_amd/csrc/fd_device.hpp -- small wave-level device helpers shared by the patch-filter kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fd_dev {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ unsigned char sat_u8_d(double v) {   // saturate_cast<uchar>(double): cvRound, clamp
    const int i = (int)rint(v);
    return (unsigned char)(i < 0 ? 0 : (i > 255 ? 255 : i));
}


// cv::equalizeHist of the n-pixel image `px` (LDS) by one wave; hist/lut: 256 ints each (LDS)
__device__ __forceinline__ void equalize_hist_wave(const unsigned char* px, unsigned char* out, int n, int* hist, int* lut, int lane) {
    for (int i = lane; i < 256; i += 64) hist[i] = 0;
    wave_sync();
    for (int i = lane; i < n; i += 64) atomicAdd(&hist[px[i]], 1);
    wave_sync();
    // lane l owns bins 4l..4l+3
    int c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = hist[4 * lane + k];
    const int mine = c[0] + c[1] + c[2] + c[3];
    const unsigned long long nz = __ballot(mine != 0);
    const int l0 = __builtin_ctzll(nz);                        // lane holding the first non-empty bin
    int i0 = 0;
    if (lane == l0) i0 = c[0] ? 0 : (c[1] ? 1 : (c[2] ? 2 : 3));
    i0 = 4 * l0 + __builtin_amdgcn_readlane(i0, l0);
    const int h0 = hist[i0];
    if (h0 == n) {
        for (int i = lane; i < n; i += 64) out[i] = (unsigned char)i0;
        wave_sync();
        return;
    }
    const float scale = (256 - 1.f) / (float)(n - h0);
    // inclusive prefix over lanes of the per-lane totals (integer: order-free)
    int incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    int run = incl - mine;   // sum of all bins before 4*lane
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int bin = 4 * lane + k;
        run += c[k];
        // lut[i0] = 0; lut[i] = saturate(sum_{j in (i0, i]} hist[j] * scale)
        lut[bin] = bin <= i0 ? 0 : (int)sat_u8_d((double)((float)(run - h0) * scale));
    }
    wave_sync();
    for (int i = lane; i < n; i += 64) out[i] = (unsigned char)lut[px[i]];
    wave_sync();
}


// HistEq64Filter::applyTo (HistEq64Filter.cpp:32-125) of the n-pixel image px (LDS) by one wave; hist: 64 ints (LDS).
// The fp32 cdf is summed in bin order (63-step DPP chain: lane l holds cdf[l] from step l on).
__device__ __forceinline__ void histeq64_wave(const unsigned char* px, unsigned char* out, int n, int* hist, int lane) {
    hist[lane] = 0;
    wave_sync();
    for (int i = lane; i < n; i += 64) atomicAdd(&hist[px[i] >> 2], 1);
    wave_sync();
    const float stretch = 255.0f / (float)n;
    const float pdf = (float)hist[lane] * stretch;
    float x = pdf;
#pragma unroll
    for (int t = 1; t < 64; ++t) {
        const float sh = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
        x = sh + pdf;
    }
    wave_sync();
    hist[lane] = (int)(unsigned int)(unsigned char)floor((double)x + 0.5);   // becomes the LUT
    wave_sync();
    for (int i = lane; i < n; i += 64) out[i] = (unsigned char)hist[px[i] >> 2];
    wave_sync();
}

// cv::cvtColor(BGR2GRAY), 8U: (B*1868 + G*9617 + R*4899 + 8192) >> 14 (GrayscaleFilter.cpp:18-24)
__device__ __forceinline__ uint32_t gray_of(uint32_t b, uint32_t g, uint32_t r) { return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14; }

// four bytes at any address as one little-endian word
__device__ __forceinline__ uint32_t ld_u32_unaligned(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// UnitNormFilter::applyTo (UnitNormFilter.cpp:24-43) of one vector by one wave: s / (cv::norm(s, normType) + 1e-4f); the norm is
// accumulated in double over the float values like cv::norm.  s may be LDS or global memory, d likewise.
__device__ __forceinline__ void unit_norm_wave(const float* s, float* d, int len, int normType, int lane) {
    double part = 0;
    for (int i = lane; i < len; i += 64) {
        const double v = (double)s[i];
        if (normType == 4) part += v * v;             // cv::NORM_L2
        else if (normType == 2) part += fabs(v);      // cv::NORM_L1
        else part = fmax(part, fabs(v));              // cv::NORM_INF
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(part, o, 64);
        part = (normType == 4 || normType == 2) ? part + other : fmax(part, other);
    }
    const double norm = normType == 4 ? sqrt(part) : part;
    const float inv = (float)(1.0 / (norm + (double)1e-4f));   // image / (norm + eps): MatExpr scale 1/d, applied in float
    for (int i = lane; i < len; i += 64) d[i] = s[i] * inv;
}

}  // namespace fd_dev
