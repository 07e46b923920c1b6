// featuredetection_amd/csrc/integral_geo.hpp -- the sample geometry of the integral-image family, one copy for every caller:
// DirectImageFeatureExtractor::extract (DirectImageFeatureExtractor.cpp:42-52) on the (H + 1) x (W + 1) integral image and the
// per-patch constants and grid points of IntegralGradientFilter::applyTo (IntegralGradientFilter.cpp:23-85).  sample_geo / grad_geo
// are __host__ __device__: the kernels of integral.hip and hog.hip and the host-only validity rule
// (fd_integral_gradient_samples_valid) run the same statements.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace fd_integral_geo {

// cvRound of a double: half to even on both sides
__host__ __device__ __forceinline__ int round_d(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2int_rn(v);
#else
    return (int)std::lrint(v);
#endif
}

struct SampleGeo {
    int px0, py0, w, h;   // patch origin and size inside the (H + 1) x (W + 1) integral image
    bool exists;
};
__host__ __device__ __forceinline__ SampleGeo sample_geo(const int32_t* __restrict__ xywh, int i, int W, int H) {
    const int4 s = reinterpret_cast<const int4*>(xywh)[i];
    SampleGeo g;
    g.w = s.z; g.h = s.w;
    g.px0 = s.x - s.z / 2;
    g.py0 = s.y - s.w / 2;
    g.exists = s.z >= 1 && s.w >= 1 && g.px0 >= 0 && g.py0 >= 0 && (long long)g.px0 + s.z <= (long long)W + 1 && (long long)g.py0 + s.w <= (long long)H + 1;
    return g;
}

// IntegralGradientFilter::applyTo (IntegralGradientFilter.cpp:23-85): the per-patch constants
struct GradGeo {
    int rX, rY;
    double spX, spY;
    bool ok;   // every read lies inside the integral image
};
__host__ __device__ __forceinline__ GradGeo grad_geo(const SampleGeo& g, int rows, int cols, int W, int H) {
    GradGeo q;
    const int width = g.w - 1, height = g.h - 1;
    const int rx = round_d((double)(width - 1) / (double)(cols + 2)), ry = round_d((double)(height - 1) / (double)(rows + 2));
    q.rX = rx > 1 ? rx : 1;
    q.rY = ry > 1 ? ry : 1;
    q.spX = (double)(width - 3 * q.rX) / (double)(cols - 1);
    q.spY = (double)(height - 3 * q.rY) / (double)(rows - 1);
    // the grid coordinates cvRound(radius + i * spacing) are monotonic in i: the first (== radius) and the last bound all reads
    const int cLast = round_d((double)q.rX + (double)(cols - 1) * q.spX), rLast = round_d((double)q.rY + (double)(rows - 1) * q.spY);
    const int cMin = q.rX < cLast ? q.rX : cLast, cMax = q.rX < cLast ? cLast : q.rX;
    const int rMin = q.rY < rLast ? q.rY : rLast, rMax = q.rY < rLast ? rLast : q.rY;
    const long long xmin = (long long)g.px0 + cMin - q.rX, xmax = (long long)g.px0 + cMax + 2 * q.rX;
    const long long ymin = (long long)g.py0 + rMin - q.rY, ymax = (long long)g.py0 + rMax + 2 * q.rY;
    q.ok = g.exists && xmin >= 0 && ymin >= 0 && xmax <= W && ymax <= H;
    return q;
}
// one grid point: (dx + 127, dy + 127) as uchar
__device__ __forceinline__ uchar2 grad_point(const int32_t* __restrict__ base, size_t S, const GradGeo& q, int row, int col) {
    const int r = __double2int_rn((double)q.rY + (double)row * q.spY), c = __double2int_rn((double)q.rX + (double)col * q.spX);
    const int32_t* __restrict__ p = base + (ptrdiff_t)r * (ptrdiff_t)S + c;
    const ptrdiff_t oy0 = -(ptrdiff_t)q.rY * (ptrdiff_t)S, oy2 = (ptrdiff_t)q.rY * (ptrdiff_t)S, oy3 = 2 * oy2;
    const int ox0 = -q.rX, ox2 = q.rX, ox3 = 2 * q.rX;
    //     p1  p2
    // p3  p4  p5  p6
    // p7  p8  p9  p10
    //     p11 p12
    const int p1 = p[oy0], p2 = p[oy0 + ox2];
    const int p3 = p[ox0], p4 = p[0], p5 = p[ox2], p6 = p[ox3];
    const int p7 = p[oy2 + ox0], p8 = p[oy2], p9 = p[oy2 + ox2], p10 = p[oy2 + ox3];
    const int p11 = p[oy3], p12 = p[oy3 + ox2];
    const int top = p1 - p2 - p4 + p5, bottom = p8 - p9 - p11 + p12, left = p3 - p4 - p7 + p8, right = p5 - p6 - p9 + p10;
    const int half = q.rY * q.rX;
    const int dx = (right - left) / (2 * half), dy = (bottom - top) / (2 * half);   // truncating, like the reference's int division
    return make_uchar2((unsigned char)(dx + 127), (unsigned char)(dy + 127));
}

}  // namespace fd_integral_geo
