// featuredetection_amd/csrc/pyramid.hip -- image pyramid on the GPU (gfx950).
//
// Restates imageprocessing::ImagePyramid (ImagePyramid.cpp:67-92,116-128,170-198) with the
// GrayscaleFilter image filter (optionally behind GreyWorldNormalizationFilter: fd_pyramid_set_image_filter)
// and optional layer filters.  All arithmetic is the integer-exact
// OpenCV 2.4 fixed-point arithmetic (cvtColor, resize INTER_LINEAR, pyrDown, Sobel), so layers are
// bit-identical to the CPU path.  Layout in HBM: ONE arena per pyramid holding the full-resolution
// gray image, every computed layer (kept or only a pyrDown source) and the filtered kept layers,
// each 256-byte aligned, rows densely packed.  The whole pyramid of a 640x480 frame is ~1.6 MB and
// stays L2/MALL resident for the scoring kernels that follow.
//
// HBM-bound stage: algorithmic bytes = 3WH (BGR read) + WH (gray write) + per layer (src read +
// dst write); see DESIGN.md.  One launch covers all chains of a pyramid depth (blockIdx.y = chain).
#include "fd_internal.hpp"
#include "fd_device.hpp"
#include <algorithm>
#include <cstring>

namespace {

constexpr int MAXJ = 16;

struct ResizeJob {
    int dw, dh;
    uint32_t dst_off;
    double scale_x, scale_y;
};
struct ResizeJobs {
    int n;
    ResizeJob j[MAXJ];
};
// one first-octave chain of k_resize_down: cv::resize of the frame to dw0 x dh0 and its pyrDown to dw1 x dh1
struct FusedJob {
    int dw0, dh0, dw1, dh1;
    uint32_t dst0_off;      // resized layer, written only when it is a kept layer (0xffffffff: stays in LDS)
    uint32_t dst1_off;      // its pyrDown
    uint32_t xtab;          // offset (in int2 entries) of the column table
    double scale_y;         // cv::resize's vertical scale: the rows' coordinates are computed in the kernel, once per tile
};
struct FusedJobs {
    int n;
    FusedJob j[MAXJ];
};
// one tile of k_pyrdown_tiled (62 x 16 outputs): everything a workgroup needs, built on the host with the launch plan and read with
// one scalar load (pd_tile_entry)
struct PdTile {
    uint32_t src_off;   // source layer
    uint32_t dst_off;   // output (dx0, dy0) of the destination layer
    int sw, sh;         // source layer
    int dx0, dy0;       // first output of the tile
    int nx, ny;         // outputs the tile stores: min(62, dw - dx0) x min(16, dh - dy0)
};
static_assert(sizeof(PdTile) == 32, "a tile entry is eight dwords");
struct FilterJob {
    int w, h;
    uint32_t src_off, dst_off;
};
struct FilterJobs {
    int n;
    FilterJob j[MAXJ];
};

__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    }
    return p;
}
// BORDER_REFLECT_101 for a coordinate at most one reflection away; anything further out is clamped (the tiled kernels only meet
// such coordinates under outputs that lie outside the layer and are not stored)
__device__ __forceinline__ int reflect1(int p, int len) {
    if (len < 3) return reflect101(p, len);   // the 5-tap halo reaches two pixels out: one reflection needs three pixels
    const int q = p < 0 ? -p : (p >= len ? 2 * len - 2 - p : p);
    return min(max(q, 0), len - 1);
}

// cv::cvtColor(BGR2GRAY), 8U: (B*1868 + G*9617 + R*4899 + 8192) >> 14
struct FramePtrs {
    const uint8_t* p[FD_MAX_FRAMES];
};
// 24-bit multiplies by name: __umul24 became v_and + v_mul_lo_u32 (quarter rate) wherever the compiler could not see the operand ranges
__device__ __forceinline__ unsigned int mul24(unsigned int a, unsigned int b) {
    unsigned int r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ unsigned int mul24_s(unsigned int a_uniform, unsigned int b) {   // a wave-uniform factor stays in its SGPR
    unsigned int r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "s"(a_uniform), "v"(b));
    return r;
}
__device__ __forceinline__ unsigned int mad24(unsigned int a, unsigned int b, unsigned int c) {
    unsigned int r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned int mulhi24(unsigned int a, unsigned int b) {   // (a * b) >> 32 of two 24-bit factors
    unsigned int r;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
using fd_dev::gray_of;            // both shared with the integral image (integral.hip)
using fd_dev::ld_u32_unaligned;

// the frames of a multi-frame pyramid: BGR -> gray (ch == 3) or copy (ch == 1) into frame blockIdx.y's arena.  Four pixels per
// thread: three dword loads, one dword store (the stage is bound by the number of memory instructions, not by their bytes).
__global__ void k_frames_to_gray(FramePtrs frames, uint8_t* __restrict__ grayBase, size_t imageStride, int n, int ch) {
    const uint8_t* __restrict__ src = frames.p[blockIdx.y];
    uint8_t* __restrict__ gray = grayBase + (size_t)blockIdx.y * imageStride;
    const int nq = n >> 2;
    const bool aligned = ((uintptr_t)src & 3) == 0;
    const int stride = gridDim.x * blockDim.x;
    auto load3 = [&](int q, uint32_t (&w)[3]) {
        if (aligned) {
            const uint32_t* s3 = reinterpret_cast<const uint32_t*>(src) + 3 * (size_t)q;
            w[0] = s3[0]; w[1] = s3[1]; w[2] = s3[2];
        } else {
            const uint8_t* s1 = src + 12 * (size_t)q;
            w[0] = ld_u32_unaligned(s1); w[1] = ld_u32_unaligned(s1 + 4); w[2] = ld_u32_unaligned(s1 + 8);
        }
    };
    auto gray4 = [&](const uint32_t (&w)[3]) {
        // bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        const uint32_t g0 = gray_of(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u);
        const uint32_t g1 = gray_of(w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
        const uint32_t g2 = gray_of((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u);
        const uint32_t g3 = gray_of((w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
        return g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    };
    // GQ quads per thread and pass, their loads in flight together: with one 12-byte load per thread the stage moved 4.5 TB/s -- the
    // bytes a full chip of wavefronts keeps in flight (6 MB) over the memory latency -- not what the memory can deliver
    constexpr int GQ = 4;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += GQ * stride) {
        if (ch == 3) {
            uint32_t w[GQ][3];
#pragma unroll
            for (int i = 0; i < GQ; ++i) load3(min(q + i * stride, nq - 1), w[i]);
#pragma unroll
            for (int i = 0; i < GQ; ++i)
                if (q + i * stride < nq) reinterpret_cast<uint32_t*>(gray)[q + i * stride] = gray4(w[i]);
        } else {
            uint32_t w[GQ];
#pragma unroll
            for (int i = 0; i < GQ; ++i) w[i] = ld_u32_unaligned(src + 4 * (size_t)min(q + i * stride, nq - 1));
#pragma unroll
            for (int i = 0; i < GQ; ++i)
                if (q + i * stride < nq) reinterpret_cast<uint32_t*>(gray)[q + i * stride] = w[i];
        }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < (n & 3)) {   // tail
        const int i = (nq << 2) + threadIdx.x;
        gray[i] = ch == 3 ? (uint8_t)gray_of(src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]) : src[i];
    }
}

__global__ void k_bgr2gray(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ gray, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int stride = gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int b = bgr[3 * (size_t)i], g = bgr[3 * (size_t)i + 1], r = bgr[3 * (size_t)i + 2];
        gray[i] = (uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14);
    }
}

// ---- LDS-tiled cv::resize and cv::pyrDown ----------------------------------------------------------------------------------
// k_resize_tiled: cv::resize INTER_LINEAR 8UC1 -> all first-octave layers from the full-resolution gray image.  Per destination
// pixel: fx = (dx + 0.5) * scale_x - 0.5 in double, rounded to float; sx = floor(fx), fx -= sx, clamped to the row (fx = 0 there);
// weights a0 = rn((1 - fx) * 2048), a1 = rn(fx * 2048); the same for the rows (b0, b1; the row indices clamped, the weights not); the
// pixel is ((b0 * ((S[y0][sx] * a0 + S[y0][sx + 1] * a1) >> 4) >> 16) + (b1 * ((S[y1][sx] * a0 + S[y1][sx + 1] * a1) >> 4) >> 16) + 2) >> 2.
// k_pyrdown_tiled: cv::pyrDown 8UC1: separable [1 4 6 4 1], (sum + 128) >> 8, BORDER_REFLECT_101; output (x, y) is centred on
// source (2 x, 2 y).  A thread computes four vertically adjacent outputs of one column: the 11 horizontal 5-tap sums it needs are
// formed once each.
// A workgroup stages the source rectangle of an output tile in LDS with dword loads (unaligned where the row start is) and every
// tap is an LDS byte read: read straight from memory, a resize issues four and a pyrDown 14 byte loads per output pixel and is
// bound by the number of memory instructions.
constexpr int TL_W = 64, TL_H = 32, TL_PITCH = 136;   // 64 x 32 output pixels per tile, 8 rows per thread: the per-thread column set-up is the
                                                        // larger part of the work of a row
constexpr int PD_TH = 16;                               // pyrDown: 64 x 16 tiles (its layers are small: 32-row tiles leave CUs idle)
constexpr int TL_ROWS = 72;                             // resize: 31 * 2.05 + 3 source rows

// cv::pyrDown of four vertically adjacent outputs of one column from a staged tile (k_pyrdown_tiled, and the tail of k_resize_down):
// T points at the byte of the column's first tap in the first of the 11 rows the outputs reach; PITCH bytes between rows.
// The row sums [1 4 6 4] . (s0 s1 s2 s3) + s4 are one byte dot product each (v_dot4_u32_u8: exact integers, a third of the
// instructions); h <= 16 * 255, so h * 6 is a 24-bit multiply-add (v_mul_lo_u32 runs at a quarter of the rate).
// T is an LDS pointer by type: through a generic one the compiler joins the two 16-bit reads of a row into one 32-bit read before it
// knows the address space, and that read is only 2-byte aligned in every other lane.
typedef const __attribute__((address_space(3))) uint8_t* lds_bytes;
template <int PITCH>
__device__ __forceinline__ void pyrdown_col4(lds_bytes T, uint32_t out[4]) {
    uint32_t h[11];
#pragma unroll
    for (int r = 0; r < 11; ++r) {
        lds_bytes S = T + r * PITCH;
        typedef const __attribute__((address_space(3))) uint16_t* lds_u16;
        const uint32_t p01 = *(lds_u16)S, p23 = *(lds_u16)(S + 2);
        h[r] = __builtin_amdgcn_udot4(p01 | (p23 << 16), 0x04060401u, (uint32_t)S[4], false);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        out[j] = (mad24(h[2 * j + 2], 6u, ((h[2 * j + 1] + h[2 * j + 3]) << 2) + h[2 * j]) + h[2 * j + 4] + 128u) >> 8;
}

// resize: valid while a tile's source rectangle fits the stage from its conservative origin, i.e. 1 <= scale_x, scale_y <= 2.05
// (first-octave layers: 1 <= scale <= 2, checked where the launch plan is built)
__global__ __launch_bounds__(256) void k_resize_tiled(const uint8_t* __restrict__ arena, uint8_t* __restrict__ out, uint32_t src_off, int sw,
                                                      int sh, ResizeJobs jobs, size_t imageStride) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[TL_ROWS * TL_PITCH];
    __shared__ int4 rowTab[TL_H];   // per dst row of the tile: LDS offsets of its two source rows, vertical weights
    const ResizeJob jb = jobs.j[blockIdx.y];
    const uint8_t* src = arena + (size_t)blockIdx.z * imageStride + src_off;   // blockIdx.z = frame of a multi-frame pyramid
    uint8_t* dst = out + (size_t)blockIdx.z * imageStride + jb.dst_off;
    const int tilesX = (jb.dw + TL_W - 1) / TL_W, tilesY = (jb.dh + TL_H - 1) / TL_H;
    auto srcX = [&](int dx, float& fx) {   // cv::resize: left source column of dst column dx and its fraction
        fx = (float)((dx + 0.5) * jb.scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        return sx;
    };
    auto srcY = [&](int dy, float& fy) {
        fy = (float)((dy + 0.5) * jb.scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= sy;
        return sy;
    };
    auto clampY = [&](int y) { return y < 0 ? 0 : (y >= sh ? sh - 1 : y); };
    const int c = threadIdx.x & 63, rq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // rq scalar: row offsets on the scalar unit
    for (int t = blockIdx.x; t < tilesX * tilesY; t += gridDim.x) {
        const int ty = t / tilesX, tx = t - ty * tilesX;
        const int dx0 = tx * TL_W, dy0 = ty * TL_H;
        // source rectangle of the tile: a conservative origin (one below the smallest coordinate any of its pixels can ask for:
        // sx >= floor(dx * scale) for scale >= 1) and the full stage, TL_ROWS x TL_PITCH bytes -- cheaper than the exact extents,
        // which need the fp64 coordinate of cv::resize per tile and thread
        const int X0 = max(0, (int)((float)dx0 * (float)jb.scale_x) - 1), Y0 = max(0, (int)((float)dy0 * (float)jb.scale_y) - 1);
        {   // lane == dword of a source row (34 per row), wave + 4 k == row: no index arithmetic, all loads of a thread in flight together
            const int x = X0 + 4 * c;
            const bool colok = c < TL_PITCH / 4;
            uint32_t v[TL_ROWS / 4];
#pragma unroll
            for (int k = 0; k < TL_ROWS / 4; ++k) {
                const int sy = min(Y0 + rq + 4 * k, sh - 1);
                v[k] = 0;
                if (colok && x + 3 < sw) v[k] = ld_u32_unaligned(src + (uint32_t)(sy * sw) + x);
            }
            if (colok && x + 3 >= sw) {   // right edge of the image: never past the row
#pragma unroll 1
                for (int k = 0; k < TL_ROWS / 4; ++k) {
                    const uint8_t* row = src + (uint32_t)(min(Y0 + rq + 4 * k, sh - 1) * sw);
                    uint32_t w = 0;
                    for (int b = 0; b < 4; ++b) w |= (uint32_t)row[min(x + b, sw - 1)] << (8 * b);
                    v[k] = w;
                }
            }
            if (colok) {
#pragma unroll
                for (int k = 0; k < TL_ROWS / 4; ++k) *reinterpret_cast<uint32_t*>(&tile[(rq + 4 * k) * TL_PITCH + 4 * c]) = v[k];
            }
        }
        if (threadIdx.x < TL_H) {   // vertical taps of the tile's rows, once per tile instead of once per thread and row
            float fy;
            const int sy = srcY(dy0 + threadIdx.x, fy);
            rowTab[threadIdx.x] = make_int4((clampY(sy) - Y0) * TL_PITCH, (clampY(sy + 1) - Y0) * TL_PITCH, __float2int_rn((1.f - fy) * 2048),
                                            __float2int_rn(fy * 2048));
        }
        __syncthreads();
        const int dx = dx0 + c;
        if (dx < jb.dw) {
            float fx;
            const int sx = srcX(dx, fx);
            const int a0 = __float2int_rn((1.f - fx) * 2048), a1 = __float2int_rn(fx * 2048);
            const int lx = sx - X0, lx1 = (sx + 1 < sw ? sx + 1 : sx) - X0;
            // 24-bit multiplies (full rate; every factor is below 2^16) and a running destination pointer: the 32-bit multiplies /
            // 64-bit multiply-adds the plain expressions compile to run at a quarter of the rate and made this kernel VALU-bound
            uint8_t* dp = dst + (uint32_t)((dy0 + rq * (TL_H / 4)) * jb.dw) + dx;
#pragma unroll
            for (int k = 0; k < TL_H / 4; ++k, dp += jb.dw) {
                const int rr = rq * (TL_H / 4) + k;
                if (dy0 + rr < jb.dh) {
                    const int4 rt = rowTab[rr];
                    const uint8_t* S0 = tile + rt.x;
                    const uint8_t* S1 = tile + rt.y;
                    const unsigned int r0 = __umul24(S0[lx], a0) + __umul24(S0[lx1], a1);
                    const unsigned int r1 = __umul24(S1[lx], a0) + __umul24(S1[lx1], a1);
                    *dp = (uint8_t)(((__umul24(rt.z, r0 >> 4) >> 16) + (__umul24(rt.w, r1 >> 4) >> 16) + 2) >> 2);
                }
            }
        }
        __syncthreads();
    }
}

// ---- cv::resize of the frame + the first cv::pyrDown of the result in one kernel ---------------------------------------------
// Most first-octave layers of a detection pyramid are not kept themselves (FaceFrontal keeps scales 0.05 .. 0.16): they only exist as the
// source of their pyrDown chain, and writing 1.2 Mpixels per frame to memory only to read them back in the next launch is what the
// pyramid stage spent its time on.  A workgroup computes the resized pixels under one 62 x 16 tile of the pyrDown layer (127 x 35, the
// 5-tap halo included; BORDER_REFLECT_101 columns / rows are the resized pixels at the reflected coordinates) into LDS and takes the
// pyrDown from there; the resized layer goes to memory only when it is a kept layer.  Same integer arithmetic as k_resize_tiled /
// k_pyrdown_tiled, value for value (ImagePyramid.cpp:177,186):
//   * the cv::resize column coordinates and fixed-point weights come from a per-layer table built on the host with the kernel's own
//     float expressions (xtab[dx] = {left source column, a0 | a1 << 16}); the rows' (k_resize_tiled's srcY) are worked out with the
//     next tile's loads, one resized row per lane;
//   * the stage holds the two source rows of every resized row of the tile in a slot of their own, interleaved byte-wise (y0 at the
//     even bytes, y1 at the odd ones), so a resized row reads its four bytes as two aligned 16-bit words at fixed offsets: no row
//     record, scalar unpacking or address arithmetic per row.
// -DFD_PYR_PROF (tools/build_prof_lib.sh, tools/pyr_phases.py): ticks thread 0 of every workgroup spends in the phases of k_resize_down
#ifdef FD_PYR_PROF
constexpr int PYR_PROF_WGS = 65536;
__device__ unsigned long long fd_pyr_prof[PYR_PROF_WGS * 8];   // one record per workgroup: same-address atomics would serialise the launch
#define PYR_T(x) const unsigned long long x = __builtin_amdgcn_s_memtime()
#else
#define PYR_T(x)
#endif
constexpr int FT_W1 = 62, FT_H1 = 16;                    // pyrDown tile
constexpr int G0_W = 2 * FT_W1 + 3, G0_H = 2 * FT_H1 + 3, G0_PITCH = 128;   // resized pixels under it: 127 x 35
constexpr int FS_PITCH = 256;                           // source stage: 126 * 2.0 + 3 columns (64 dwords: one per lane) of a source row
constexpr int FS_LOADS = (2 * G0_H + 3) / 4;            // 18 dwords per lane: rows y0 and y1 of the FS_ROWS resized rows of its wavefront
constexpr int FS_ROWS = FS_LOADS / 2;                   // wavefront w fetches and stages the resized rows 9 w .. 9 w + 8
constexpr int FS_SLOT = 2 * FS_PITCH;                   // pair slot of a resized row: byte 2 x = row y0, byte 2 x + 1 = row y1 of source column X0 + x
constexpr int FS_SLOTS = 2 * FS_LOADS;                  // 36 slots; the tile has 35 rows, slot 35 repeats row 34
static_assert(FS_SLOTS >= G0_H + 1, "the last column's neighbour read of the tile's last row lands in the next slot");
// Persistent workgroups walk a host-built list of tiles ({source columns, tile position, chain} per entry: the layout is static) and keep
// the NEXT tile's global loads -- 18 source dwords and the column's xtab entry per thread -- in flight in registers while they resize the
// current one: a tile used to spend 45 % of its 7.6 us waiting for them (in-kernel timestamps, tools/pyr_phases.py).
// Multi-frame pyramids: workgroup b runs on XCD b % 8 and takes the frames b % 8, b % 8 + 8, ...: a frame's gray image is read by one L2.
//
// The row arithmetic and the stage addressing are __host__ __device__ functions: the host hook fd_debug_resize_stage stages a tile
// with the kernel's own code.
struct FusedRow {
    int y0, y1;      // the two source rows of a resized row, clamped into the image
    uint32_t taps;   // its vertical weights b0 | b1 << 16
};
__host__ __device__ inline int fused_rn(float v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __float2int_rn(v);
#else
    return (int)nearbyintf(v);
#endif
}
// Row i of the tile whose first resized row (before the reflection) is gy0: BORDER_REFLECT_101 of the resized rows the kept pyrDown
// rows reach (one reflection; rows further out only feed pyrDown rows past the layer's end, any valid row will do for them), then
// k_resize_tiled's srcY / clampY
__host__ __device__ inline FusedRow fused_row(int i, int gy0, int dh0, double scale_y, int sh) {
    const int py = gy0 + (i < G0_H - 1 ? i : G0_H - 1), pr = py < 0 ? -py : (py >= dh0 ? 2 * dh0 - 2 - py : py);
    const int pc = pr < 0 ? 0 : (pr > dh0 - 1 ? dh0 - 1 : pr);
    float fy = (float)((pc + 0.5) * scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= sy;
    FusedRow r;
    r.taps = (uint32_t)fused_rn((1.f - fy) * 2048) | (uint32_t)fused_rn(fy * 2048) << 16;
    r.y0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy);
    r.y1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
    return r;
}
// the first of the four source columns lane `lane` fetches of every row: lanes right of the tile's ncol columns take its last dword again
__host__ __device__ inline uint32_t fs_fetch_col(int lane, int X0, int ncol) {
    const int last = (ncol - 1) >> 2;
    return (uint32_t)(4 * (lane < last ? lane : last) + X0);
}
__host__ __device__ inline uint32_t fs_perm(uint32_t hi, uint32_t lo, uint32_t sel) {   // v_perm_b32: selector byte 0..3 = byte of lo, 4..7 = of hi, 12 = 0
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t b = (sel >> (8 * i)) & 255u;
        const uint32_t v = b < 4 ? lo >> (8 * b) : (b < 8 ? hi >> (8 * (b - 4)) : 0u);
        r |= (v & 255u) << (8 * i);
    }
    return r;
#endif
}
// what a lane stores into the slot of a resized row: its dword a of row y0 and b of row y1 as {a0 b0 a1 b1 | a2 b2 a3 b3} ...
__host__ __device__ inline uint2 fs_pair(uint32_t a, uint32_t b) {
    uint2 r;
    r.x = fs_perm(b, a, 0x05010400u);
    r.y = fs_perm(b, a, 0x07030602u);
    return r;
}
// ... at this byte of the stage (8-byte aligned)
__host__ __device__ inline int fs_store_off(int row, int lane) { return row * FS_SLOT + 8 * lane; }
// The byte of the stage where the thread of left source column sx reads rows y0 | y1 << 8 of that column for resized row `row` of the
// tile; the right neighbour's pair is the 16-bit word behind it (+ 2).  Both are even: the LDS serves an odd 16-bit read slowly.
// A column that the reflection on a layer's right edge takes back left of the tile's first source column (e.g. 374 against 494 on
// the last tile of a 498-wide layer) only feeds pyrDown outputs past the layer's end: the clamp keeps its reads inside its slot.
// Columns the tile keeps lie in 0 .. FS_PITCH - 1 already; 255 is the image's last column there, whose neighbour -- the first word
// of the next slot, and slot 35 exists -- weighs 0.
__host__ __device__ inline int fs_read_off(int sx, int X0, int row) {
    const int x = sx - X0;
    return 2 * (x < 0 ? 0 : (x > FS_PITCH - 1 ? FS_PITCH - 1 : x)) + row * FS_SLOT;
}

struct FusedFetch {   // what a thread holds for a tile before it is in LDS
    uint32_t v[FS_LOADS];   // v[2 q], v[2 q + 1]: its dword of rows y0, y1 of the resized row FS_ROWS w + q
    int2 ex;         // thread = column of the tile: its xtab entry
    uint32_t taps;   // lane q < FS_ROWS = resized row FS_ROWS w + q of the tile: its vertical weights b0 | b1 << 16
};
__device__ __forceinline__ void fused_issue(FusedFetch& f, const uint8_t* __restrict__ src, int sw, int sh, const int2* __restrict__ tabs,
                                            const FusedJob& jb, const int4 d) {
    const int X0 = d.x, ncol = d.y;
    const int gx0 = 2 * (d.z & 0xffff) * FT_W1 - 2, gy0 = 2 * (int)((uint32_t)d.z >> 16) * FT_H1 - 2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // wavefront w fetches both source rows of the resized rows FS_ROWS w + q, and lane q works that row out (the lanes from FS_ROWS on
    // work out rows nobody asks them for)
    const FusedRow r = fused_row(FS_ROWS * wave + lane, gy0, jb.dh0, jb.scale_y, sh);
    f.taps = r.taps;
    const uint32_t rowOff0 = mul24((uint32_t)r.y0, (uint32_t)sw), rowOff1 = mul24((uint32_t)r.y1, (uint32_t)sw);
    // A dword that hangs over the right edge of the image takes its last bytes from the next row (or, in the last row, from the arena
    // behind the gray image): they stand for columns >= sw, which no tap reads (the last column's right neighbour has weight 0).
    // No predication: lanes right of the rectangle load its last dword again (valid addresses, values nobody reads) -- with a test per
    // load the loads were as many basic blocks of exec-mask bookkeeping, 400 instructions per tile.
    const uint32_t voff = fs_fetch_col(lane, X0, ncol);
#pragma unroll
    for (int q = 0; q < FS_ROWS; ++q) {
        f.v[2 * q] = ld_u32_unaligned(src + ((uint32_t)__builtin_amdgcn_readlane((int)rowOff0, q) + voff));
        f.v[2 * q + 1] = ld_u32_unaligned(src + ((uint32_t)__builtin_amdgcn_readlane((int)rowOff1, q) + voff));
    }
    f.ex = tabs[jb.xtab + reflect101(gx0 + (int)(threadIdx.x & 127), jb.dw0)];
}

__global__ __launch_bounds__(256) void k_resize_down(uint8_t* __restrict__ arena0, uint32_t src_off, int sw, int sh, const int2* __restrict__ tabs,
                                                     FusedJobs jobs, uint32_t tileTab, int tilesPerFrame, int nimg, size_t imageStride) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[FS_SLOTS * FS_SLOT];
    __shared__ __attribute__((aligned(16))) uint8_t g0[G0_H * G0_PITCH];
    __shared__ __attribute__((aligned(16))) uint2 taps[G0_H];   // per resized row of the tile: b0 << 12, b1 << 12 (read as a broadcast beside the row's bytes)
    const int4* tiles = reinterpret_cast<const int4*>(tabs + tileTab);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool byXcd = nimg >= 8 && (gridDim.x & 7u) == 0;
    const int xcd = blockIdx.x & 7;
    const int slot = byXcd ? (int)(blockIdx.x >> 3) : (int)blockIdx.x, nslot = byXcd ? (int)(gridDim.x >> 3) : (int)gridDim.x;
    const int items = (byXcd ? (nimg - xcd + 7) >> 3 : nimg) * tilesPerFrame;
    auto frame_of = [&](int item) { const int fi = item / tilesPerFrame; return byXcd ? xcd + 8 * fi : fi; };
    auto desc_of = [&](int item) { return item < items ? tiles[item % tilesPerFrame] : make_int4(0, 0, 0, 0); };

    int item = slot;
    if (item >= items) return;
    int4 d = desc_of(item);
    FusedFetch f;
    fused_issue(f, arena0 + (size_t)frame_of(item) * imageStride + src_off, sw, sh, tabs, jobs.j[d.w], d);
    int itemN = item + nslot;
    int4 dN = desc_of(itemN);

#ifdef FD_PYR_PROF
    unsigned long long pacc[6] = {0, 0, 0, 0, 0, 0}, ptiles = 0;
#endif
    for (; item < items; item = itemN, d = dN, itemN += nslot, dN = desc_of(itemN)) {
        PYR_T(p0);
        const FusedJob jb = jobs.j[d.w];
        uint8_t* arena = arena0 + (size_t)frame_of(item) * imageStride;
        const int X0 = d.x;
        const int x1 = (d.z & 0xffff) * FT_W1, y1 = (int)((uint32_t)d.z >> 16) * FT_H1;   // first pyrDown pixel of the tile
        const int gx0 = 2 * x1 - 2, gy0 = 2 * y1 - 2;                      // resized pixel of tile entry (0, 0), before the border reflection
        {   // the fetched source rows and vertical taps -> LDS
            // every lane stores its two dwords of every row, interleaved (what lies right of the rectangle is never read); a row's taps
            // come from the lane that worked the row out: nine adjacent entries per wavefront, no two on one bank
            static_assert(FS_LOADS % 2 == 0 && 4 * FS_ROWS >= G0_H && FS_PITCH == 256, "stage holds a dword pair per lane for rows FS_ROWS wave + q");
#pragma unroll
            for (int q = 0; q < FS_ROWS; ++q)
                *reinterpret_cast<uint2*>(&stage[fs_store_off(FS_ROWS * wave + q, lane)]) = fs_pair(f.v[2 * q], f.v[2 * q + 1]);
            const int i = FS_ROWS * wave + lane;
            if (lane < FS_ROWS && i < G0_H) taps[i] = make_uint2((f.taps & 0xffffu) << 12, (f.taps >> 16) << 12);
        }
        const int2 ex = f.ex;
        PYR_T(p1);
        __syncthreads();
        PYR_T(p2);
        if (itemN < items)   // the next tile's loads fly while this one is resized
            fused_issue(f, arena0 + (size_t)frame_of(itemN) * imageStride + src_off, sw, sh, tabs, jobs.j[dN.w], dN);
        PYR_T(p3);
        {   // ---- resize: thread = one column of the tile, half of its rows (0..17 / 18..34).  A row: the pairs y0 | y1 << 8 of its column
            //      and of the right neighbour at fixed offsets (two permutes make s0 | s1 << 16 of either row for v_dot2_u32_u16 against
            //      a0 | a1 << 16) and its taps as an LDS broadcast that no address waits for, two rows per 16-byte read
            const int c = threadIdx.x & 127, half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
            if (c < G0_W) {
                constexpr int HR = (G0_H + 1) / 2;   // 18 rows for the first half, 17 for the second
                static_assert(HR % 2 == 0 && (HR * sizeof(uint2)) % 16 == 0 && 2 * HR - 1 == G0_H, "either half reads its taps as aligned row pairs");
                const int rBase = half * HR;
                const int lx = fs_read_off(ex.x, X0, rBase);
                // the right neighbour through an offset the compiler cannot relate to lx: it would otherwise merge the two 16-bit reads
                // into one ds_read_b32 that is only 2-byte aligned in the odd columns (an odd-address ds_read_u16 once made this kernel
                // 4x as slow: 363 against 85 us)
                int lx1 = lx + 2;
                asm("" : "+v"(lx1));
                typedef const __attribute__((address_space(3))) uint16_t* lds_u16;
                lds_bytes sp = (lds_bytes)stage + lx, sp1 = (lds_bytes)stage + lx1;
                const uint2* tp = taps + rBase;
                const u16x2 aw = __builtin_bit_cast(u16x2, ex.y);
                uint8_t* gp = g0 + rBase * G0_PITCH + c;
                auto row = [&](int i, const uint2 t) {
                    const uint32_t P = *(lds_u16)(sp + i * FS_SLOT), Q = *(lds_u16)(sp1 + i * FS_SLOT);
                    const u16x2 p0 = __builtin_bit_cast(u16x2, fs_perm(Q, P, 0x0c040c00u)), p1 = __builtin_bit_cast(u16x2, fs_perm(Q, P, 0x0c050c01u));
                    const unsigned int h0 = __builtin_amdgcn_udot2(p0, aw, 0u, false) & ~15u;   // cv::resize's horizontal intermediate, times 16
                    const unsigned int h1 = __builtin_amdgcn_udot2(p1, aw, 0u, false) & ~15u;
                    // b << 12 (<= 2^23): (b << 12) * (h & ~15) >> 32 == (b * (h >> 4)) >> 16
                    gp[i * G0_PITCH] = (uint8_t)((mulhi24(t.x, h0) + mulhi24(t.y, h1) + 2) >> 2);
                };
#pragma unroll
                for (int i = 0; i < HR - 2; i += 2) {
                    const uint4 t2 = *reinterpret_cast<const uint4*>(tp + i);
                    row(i, make_uint2(t2.x, t2.y));
                    row(i + 1, make_uint2(t2.z, t2.w));
                }
                row(HR - 2, tp[HR - 2]);
                if (half == 0) row(HR - 1, tp[HR - 1]);   // row 35 does not exist
            }
        }
        PYR_T(p4);
        __syncthreads();
        PYR_T(p5);
        {   // ---- pyrDown of the tile (k_pyrdown_tiled's arithmetic on the LDS copy)
            const int c1 = lane;
            const int x = x1 + c1;
            if (c1 < FT_W1 && x < jb.dw1) {
                constexpr int PR = FT_H1 / 4;   // output rows per thread
                static_assert(PR == 4, "pyrdown_col4");
                uint32_t v[PR];
                pyrdown_col4<G0_PITCH>((lds_bytes)g0 + (2 * wave * PR) * G0_PITCH + 2 * c1, v);
                uint8_t* dp = arena + jb.dst1_off + (uint32_t)((y1 + wave * PR) * jb.dw1) + x;
#pragma unroll
                for (int j = 0; j < PR; ++j, dp += jb.dw1)
                    if (y1 + wave * PR + j < jb.dh1) *dp = (uint8_t)v[j];
            }
        }
        if (jb.dst0_off != 0xffffffffu) {   // the resized layer is a kept layer: the tile's own 124 x 32 pixels of it
            uint8_t* d0 = arena + jb.dst0_off;
            for (int i = threadIdx.x; i < 32 * 128; i += 256) {
                const int r = 2 + (i >> 7), c = 2 + (i & 127);
                const int gx = gx0 + c, gy = gy0 + r;
                if (c < 2 + 2 * FT_W1 && gx < jb.dw0 && gy < jb.dh0) d0[(uint32_t)(gy * jb.dw0) + gx] = g0[r * G0_PITCH + c];
            }
        }
#ifdef FD_PYR_PROF
        {
            const unsigned long long p6 = __builtin_amdgcn_s_memtime();
            pacc[0] += p1 - p0; pacc[1] += p2 - p1; pacc[2] += p3 - p2; pacc[3] += p4 - p3; pacc[4] += p5 - p4; pacc[5] += p6 - p5; ++ptiles;
        }
#endif
        // no barrier here: the next tile's stage is free since the barrier after the resize, and its resize writes g0 only behind the
        // next barrier, which every wavefront reaches after its pyrDown reads above
    }
#ifdef FD_PYR_PROF
    if (threadIdx.x == 0 && blockIdx.x < (unsigned int)PYR_PROF_WGS) {
        for (int i = 0; i < 6; ++i) fd_pyr_prof[blockIdx.x * 8 + i] = pacc[i];
        fd_pyr_prof[blockIdx.x * 8 + 6] = ptiles;
    }
#endif
}

// ---- k_pyrdown_tiled ------------------------------------------------------------------------------------------------------
// A workgroup takes one 62 x 16 tile of a destination layer: its 127 x 35 source bytes (5-tap halo included) go to LDS as 32 dwords
// per row, then every thread computes four vertically adjacent outputs of one column (pyrdown_col4).  What a tile is comes from a
// host-built entry (PdTile, one scalar load); the functions below are __host__ __device__ so that the host hook
// fd_debug_pyrdown_stage stages a tile with the kernel's own code.
constexpr int PD_W = 62;                 // 62 x 16 outputs = 127 x 35 source bytes = 32 dwords per row: two rows per wavefront load
constexpr int PD_LD = 5;                 // wavefront rq stages rows 2 (rq + 4 k) and 2 (rq + 4 k) + 1 (its lanes 0..31 / 32..63), k < PD_LD
constexpr int PD_ROWS = 8 * PD_LD;       // 40 staged rows; the outputs read 35
constexpr int PD_PITCH = 136;
static_assert(2 * PD_TH + 3 <= PD_ROWS && 2 * PD_W + 3 <= 128 && 128 <= PD_PITCH, "pyrDown stage");

// BORDER_REFLECT_101 without branches for the coordinates a 5-tap pyrDown USES (two pixels out on either side): |p|, one reflection
// at the far end, then a clamp.  Exact for every len >= 1 there (len 1: everything is 0; len 2: -2 -> 0, -1 -> 1, 2 -> 0); coordinates
// further out only feed outputs outside the layer and may be anything valid.
__host__ __device__ inline int reflect_cf(int p, int len) {
    int q = p < 0 ? -p : p;
    q = q >= len ? 2 * len - 2 - q : q;
    q = q < 0 ? 0 : q;
    return q > len - 1 ? len - 1 : q;
}
__host__ __device__ inline int pd_tiles(int sw, int sh) { return (((sw + 1) / 2 + PD_W - 1) / PD_W) * (((sh + 1) / 2 + PD_TH - 1) / PD_TH); }
// tile t (row-major over the destination layer) of the pyrDown of a sw x sh layer
__host__ __device__ inline PdTile pd_tile_entry(int sw, int sh, uint32_t src_off, uint32_t dst_off, int t) {
    const int dw = (sw + 1) / 2, dh = (sh + 1) / 2, tilesX = (dw + PD_W - 1) / PD_W;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    PdTile e;
    e.src_off = src_off;
    e.sw = sw; e.sh = sh;
    e.dx0 = tx * PD_W; e.dy0 = ty * PD_TH;
    e.dst_off = dst_off + (uint32_t)(e.dy0 * dw + e.dx0);
    e.nx = dw - e.dx0 < PD_W ? dw - e.dx0 : PD_W;
    e.ny = dh - e.dy0 < PD_TH ? dh - e.dy0 : PD_TH;
    return e;
}
// The dword of source columns xs .. xs + 3 of a row of sw >= 8 pixels, xs even and >= -2: the dword to load (clamped into the row) and
// the byte selector that makes it the wanted one.  Inside the row the two coincide (identity).  Left of it (xs == -2, tile column 0
// only) columns -2 .. 1 are bytes {2, 1, 0, 1} of the dword at 0.  Over the right end the dword at sw - 4 is loaded, d = xs - (sw - 4)
// columns too far left: column sw - 4 + i is byte i for i <= 3, sw reflects to sw - 2 (byte 2), sw + 1 to sw - 3 (byte 1); no stored
// output reads beyond sw + 1, those bytes may be anything.  Byte i of the constant is that map, so the selector is the constant
// shifted down by d bytes.  sw >= 8: the two overhangs never meet in one dword.
struct PdCol {
    int xc;
    uint32_t sel;
};
__host__ __device__ inline PdCol pd_col(int xs, int sw) {
    PdCol pc;
    pc.xc = xs < 0 ? 0 : (xs > sw - 4 ? sw - 4 : xs);
    const int d = xs - pc.xc;
    const uint32_t right = (uint32_t)(0x0000010203020100ull >> (8 * ((d > 5 ? 5 : d) & 7)));
    pc.sel = d < 0 ? 0x01000102u : right;
    return pc;
}
__host__ __device__ inline uint32_t pd_perm(uint32_t v, uint32_t sel) {   // byte i of the result = byte (sel >> 8 i) & 3 of v
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(v, v, sel);   // v_perm_b32
#else
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= ((v >> (8 * ((sel >> (8 * i)) & 3u))) & 0xffu) << (8 * i);
    return r;
#endif
}
// What lane `lane` of wavefront rq stages: v[k] = source columns X0 + 4 (lane & 31) .. + 3 of tile row 2 (rq + 4 k) + (lane >> 5), border
// reflected.  One clamped dword load and one byte permute per row, no tests, nothing per row but the address: rq is wave-uniform in
// the kernel, so the reflected row offsets of both halves are scalar and a lane picks its own with an AND.
// Layers narrower than 8 pixels (one tile column, a handful of bytes per row) gather reflected bytes instead.
__host__ __device__ inline void pd_stage(const uint8_t* __restrict__ src, const PdTile& e, int rq, int lane, uint32_t v[PD_LD]) {
    const int sw = e.sw, sh = e.sh;
    const int xs = 2 * e.dx0 - 2 + 4 * (lane & 31), Y0 = 2 * e.dy0 - 2 + 2 * rq;
    const uint32_t odd = 0u - (uint32_t)(lane >> 5);
    if (sw >= 8) {
        const PdCol pc = pd_col(xs, sw);
#pragma unroll
        for (int k = 0; k < PD_LD; ++k) {
            const uint32_t o0 = (uint32_t)(reflect_cf(Y0 + 8 * k, sh) * sw), o1 = (uint32_t)(reflect_cf(Y0 + 8 * k + 1, sh) * sw);
            uint32_t w;
            __builtin_memcpy(&w, src + (o0 + ((o1 - o0) & odd) + (uint32_t)pc.xc), 4);
            v[k] = pd_perm(w, pc.sel);
        }
    } else {
#pragma unroll
        for (int k = 0; k < PD_LD; ++k) {
            const uint8_t* row = src + (uint32_t)(reflect_cf(Y0 + 8 * k + (int)(odd & 1u), sh) * sw);
            uint32_t w = 0;
            for (int b = 0; b < 4; ++b) w |= (uint32_t)row[reflect_cf(xs + b, sw)] << (8 * b);
            v[k] = w;
        }
    }
}

// grid (tiles << xcdShift, frames >> xcdShift, 1) with xcdShift = 3, or (tiles, 1, frames) with xcdShift = 0.  With 3, workgroup
// (b, y) runs on XCD b % 8 (observed dispatch order, the grid's x extent being a multiple of 8; only speed depends on it) and takes
// tile b >> 3 of frame (b & 7) + 8 y, like k_resize_down before and k_wvm_prefilter behind this kernel: a frame's generations stay
// in one L2 instead of going round-robin over all eight.
__global__ __launch_bounds__(256) void k_pyrdown_tiled(uint8_t* __restrict__ arena0, const PdTile* __restrict__ tiles, size_t imageStride, int xcdShift) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[PD_ROWS * PD_PITCH];
    const int c = threadIdx.x & 63, rq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // rq scalar: row offsets on the scalar unit
    const uint32_t frame = (blockIdx.x & ((1u << xcdShift) - 1u)) + 8u * blockIdx.y + blockIdx.z;
    const PdTile e = tiles[blockIdx.x >> xcdShift];
    uint8_t* __restrict__ arena = arena0 + (size_t)frame * imageStride;
    {
        uint32_t v[PD_LD];
        pd_stage(arena + e.src_off, e, rq, c, v);
        uint8_t* sp = tile + 2 * rq * PD_PITCH + ((0u - (uint32_t)(c >> 5)) & (uint32_t)PD_PITCH) + 4 * (c & 31);
#pragma unroll
        for (int k = 0; k < PD_LD; ++k) *reinterpret_cast<uint32_t*>(sp + 8 * k * PD_PITCH) = v[k];
    }
    __syncthreads();
    if (c < e.nx) {
        constexpr int PR = PD_TH / 4;   // output rows per thread
        static_assert(PR == 4, "pyrdown_col4");
        uint32_t v[PR];
        pyrdown_col4<PD_PITCH>((lds_bytes)tile + (2 * rq * PR) * PD_PITCH + 2 * c, v);
        const int dw = (e.sw + 1) >> 1;
        uint8_t* dst = arena + e.dst_off + (uint32_t)(rq * PR * dw);   // scalar row pointers, the column as the lane's offset
#pragma unroll
        for (int j = 0; j < PR; ++j, dst += dw)
            if (rq * PR + j < e.ny) {
                uint32_t col = (uint32_t)c;
                asm("" : "+v"(col));   // the offset's zero extension inside the block of its store: global_store with a scalar base
                dst[col] = (uint8_t)v[j];
            }
    }
}

// cv::Sobel derivatives of GradientFilter (GradientFilter.cpp:16-59; taps of getDerivKernels, see oracle/orc_image.cpp): ksize 1, 3
// take the short forms; 5, 7 and CV_SCHARR (-1) the separable sums.  Returns the scale 1 / 2^(2 ksize - 3) (1/2, 1/32 for ksize 1 /
// Scharr).  Everything is an exact integer; 127 + scale * g is exact in float.
__device__ __forceinline__ float grad_pair(const uint8_t* __restrict__ src, int w, int h, int x, int y, int ksize, int& gx, int& gy) {
    if (ksize == 1 || ksize == 3) {
        const int xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
        const int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h);
        const uint8_t *S0 = src + (size_t)ym * w, *S1 = src + (size_t)y * w, *S2 = src + (size_t)yp * w;
        if (ksize == 1) {
            gx = S1[xp] - S1[xm];
            gy = S2[x] - S0[x];
            return 0.5f;
        }
        gx = (S0[xp] - S0[xm]) + 2 * (S1[xp] - S1[xm]) + (S2[xp] - S2[xm]);
        gy = (S2[xm] - S0[xm]) + 2 * (S2[x] - S0[x]) + (S2[xp] - S0[xp]);
        return 0.125f;
    }
    // derivative taps d (odd symmetry) and smoothing taps s (even symmetry), both of length n = 2 a + 1
    int a, d1, d2, d3, s0, s1, s2, s3;
    float scale;
    if (ksize == 5) { a = 2; d1 = 2; d2 = 1; d3 = 0; s0 = 6; s1 = 4; s2 = 1; s3 = 0; scale = 1.f / 128.f; }
    else if (ksize == 7) { a = 3; d1 = 5; d2 = 4; d3 = 1; s0 = 20; s1 = 15; s2 = 6; s3 = 1; scale = 1.f / 2048.f; }
    else { a = 1; d1 = 1; d2 = 0; d3 = 0; s0 = 10; s1 = 3; s2 = 0; s3 = 0; scale = 1.f / 32.f; }   // CV_SCHARR
    const int dk[4] = {0, d1, d2, d3}, sk[4] = {s0, s1, s2, s3};
    int cx[7], cy[7];
    for (int t = -a; t <= a; ++t) { cx[t + a] = reflect101(x + t, w); cy[t + a] = reflect101(y + t, h); }
    gx = 0;
    gy = 0;
    for (int j = -a; j <= a; ++j) {
        const uint8_t* S = src + (size_t)cy[j + a] * w;
        int rd = 0, rs = 0;   // derivative / smoothing along x of row y + j
        for (int i = 1; i <= a; ++i) {
            const int hi = S[cx[a + i]], lo = S[cx[a - i]];
            rd += dk[i] * (hi - lo);
            rs += sk[i] * (hi + lo);
        }
        rs += sk[0] * S[cx[a]];
        const int aj = j < 0 ? -j : j;
        gx += sk[aj] * rd;
        gy += (j < 0 ? -dk[aj] : dk[aj]) * rs;
    }
    return scale;
}

// cv::blur(image, Size(k, k)) of GradientFilter's optional blur (GradientFilter.cpp:43-46): normalised box filter, anchor k / 2,
// BORDER_REFLECT_101, saturate_cast<uchar>(sum * (1.0 / (k * k))) in double
__global__ void k_box_blur(uint8_t* __restrict__ arena, int k, FilterJobs jobs) {
    const FilterJob jb = jobs.j[blockIdx.y];
    const uint8_t* src = arena + jb.src_off;
    uint8_t* dst = arena + jb.dst_off;
    const int w = jb.w, h = jb.h, a = k / 2;
    const double scale = 1.0 / ((double)k * k);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w * h; i += gridDim.x * blockDim.x) {
        const int y = i / w, x = i - y * w;
        int s = 0;
        for (int j = 0; j < k; ++j) {
            const uint8_t* S = src + (size_t)reflect101(y - a + j, h) * w;
            for (int q = 0; q < k; ++q) s += S[reflect101(x - a + q, w)];
        }
        dst[i] = (uint8_t)min(255, max(0, __double2int_rn((double)s * scale)));
    }
}

// GradientFilter (delta 127, 8U saturate + cvRound) fused with the GradientBinningFilter 64K-entry look-up (index = gx | gy << 8).
template <int E>  // bytes per LUT entry: 2 (one bin + weight) or 4 (two bins + weights)
__global__ void k_gradbin(uint8_t* __restrict__ arena, const uint8_t* __restrict__ lut, int ksize, FilterJobs jobs) {
    const FilterJob jb = jobs.j[blockIdx.y];
    const uint8_t* src = arena + jb.src_off;
    uint8_t* dst = arena + jb.dst_off;
    const int w = jb.w, h = jb.h;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w * h; i += gridDim.x * blockDim.x) {
        int y = i / w, x = i - y * w;
        int gx, gy;
        const float scale = grad_pair(src, w, h, x, y, ksize, gx, gy);
        // exact in float; cvRound = round-half-even; saturate to 0..255
        int vx = __float2int_rn(127.f + scale * gx), vy = __float2int_rn(127.f + scale * gy);
        vx = min(255, max(0, vx));
        vy = min(255, max(0, vy));
        uint32_t idx = (uint32_t)vx | ((uint32_t)vy << 8);
        if (E == 2) {
            *(uint16_t*)(dst + 2 * (size_t)i) = *(const uint16_t*)(lut + 2 * (size_t)idx);
        } else {
            *(uint32_t*)(dst + 4 * (size_t)i) = *(const uint32_t*)(lut + 4 * (size_t)idx);
        }
    }
}

// GradientFilter::applyTo alone (GradientFilter.cpp:38-59): the CV_8UC2 gradient image (x, y), same arithmetic as k_gradbin
__global__ void k_gradient_image(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int ksize) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w * h; i += gridDim.x * blockDim.x) {
        int y = i / w, x = i - y * w;
        int gx, gy;
        const float scale = grad_pair(src, w, h, x, y, ksize, gx, gy);
        int vx = __float2int_rn(127.f + scale * gx), vy = __float2int_rn(127.f + scale * gy);
        dst[2 * (size_t)i] = (uint8_t)min(255, max(0, vx));
        dst[2 * (size_t)i + 1] = (uint8_t)min(255, max(0, vy));
    }
}
// GradientBinningFilter::applyTo alone (GradientBinningFilter.cpp:62-93): LUT look-up of a CV_8UC2 gradient image
template <int E>
__global__ void k_binning_image(const uint8_t* __restrict__ grad, const uint8_t* __restrict__ lut, uint8_t* __restrict__ dst, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t idx = (uint32_t)grad[2 * (size_t)i] | ((uint32_t)grad[2 * (size_t)i + 1] << 8);
        for (int e = 0; e < E; ++e) dst[(size_t)E * i + e] = lut[(size_t)E * idx + e];
    }
}

// LbpFilter.cpp:20-44: uniform patterns (<= 2 circular transitions) get indices 1..58 in increasing code order, all others 0.
// index = 1 + #uniform codes below this one.
__device__ __forceinline__ int lbp_uniform_index(int code) {
    int rot = ((code << 1) | (code >> 7)) & 0xff;  // bit pos compared with bit pos-1 (pos 0 with 7)
    int transitions = __popc((code ^ rot) & 0xff);
    if (transitions > 2) return 0;
    int cnt = 0;
    for (int q = 0; q < code; ++q) {
        int rq = ((q << 1) | (q >> 7)) & 0xff;
        cnt += __popc((q ^ rq) & 0xff) <= 2;
    }
    return 1 + cnt;
}

// one LBP code (LbpFilter.hpp:88-180) from the rows P (y - 1), C (y), N (y + 1) at the columns xm, x, xp; the caller resolves the
// border.  FD_LBP8_UNIFORM: the raw 8-bit code (the callers map it: lbp_uniform_index, or a table of it)
__device__ __forceinline__ int lbp_raw_code(const uint8_t* P, const uint8_t* C, const uint8_t* N, int xm, int x, int xp, int type) {
    const int c = C[x];
    int code = 0;
    if (type == FD_LBP8 || type == FD_LBP8_UNIFORM) {
        code |= (P[xm] > c) << 7;
        code |= (P[x] > c) << 6;
        code |= (P[xp] > c) << 5;
        code |= (C[xp] > c) << 4;
        code |= (N[xp] > c) << 3;
        code |= (N[x] > c) << 2;
        code |= (N[xm] > c) << 1;
        code |= (C[xm] > c) << 0;
    } else if (type == FD_LBP4) {
        code |= (P[x] > c) << 3;
        code |= (C[xp] > c) << 2;
        code |= (N[x] > c) << 1;
        code |= (C[xm] > c) << 0;
    } else {
        code |= (P[xm] > c) << 3;
        code |= (P[xp] > c) << 2;
        code |= (N[xp] > c) << 1;
        code |= (N[xm] > c) << 0;
    }
    return code;
}

// LbpFilter 3x3 codes with BORDER_REPLICATE (LbpFilter.hpp:88-180), optional uniform map
__global__ void k_lbp(uint8_t* __restrict__ arena, int type, FilterJobs jobs) {
    const FilterJob jb = jobs.j[blockIdx.y];
    const uint8_t* src = arena + jb.src_off;
    uint8_t* dst = arena + jb.dst_off;
    const int w = jb.w, h = jb.h;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w * h; i += gridDim.x * blockDim.x) {
        int y = i / w, x = i - y * w;
        int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
        int code = lbp_raw_code(src + (size_t)ym * w, src + (size_t)y * w, src + (size_t)yp * w, xm, x, xp, type);
        if (type == FD_LBP8_UNIFORM) code = lbp_uniform_index(code);
        dst[i] = (uint8_t)code;
    }
}

// imageprocessing::GradientMagnitudeFilter (GradientMagnitudeFilter.hpp:39-50, CV_8U branch) of one GradientFilter pixel (vx, vy):
// saturate_cast<uchar>(sqrt(x^2 + y^2)) with x = vx - 127, y = vy - 127.  s = x^2 + y^2 <= 32768 is an integer, its root is never
// k + 1/2, so the rounded root is the r with r^2 - r < s <= r^2 + r (at most 181): the largest r with r (r - 1) < s, bit by bit
__device__ __forceinline__ int grad_magnitude(int vx, int vy) {
    const int x = vx - 127, y = vy - 127;
    const int s = x * x + y * y;
    int r = 0;
#pragma unroll
    for (int b = 128; b > 0; b >>= 1) {
        const int t = r + b;
        r = t * t - t < s ? t : r;
    }
    return r;
}

// GradientMagnitudeFilter::applyTo alone: CV_8UC2 gradient image -> CV_8UC1 magnitudes
__global__ void k_gradient_magnitude_image(const uint8_t* __restrict__ grad, uint8_t* __restrict__ dst, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        dst[i] = (uint8_t)grad_magnitude(grad[2 * (size_t)i], grad[2 * (size_t)i + 1]);
}

// FD_LAYER_GRADMAG_LBP: GradientFilter -> GradientMagnitudeFilter -> LbpFilter in one pass, no magnitude plane in memory.  A
// workgroup takes GL_TW x GL_TH pixel tiles of a layer: it stages the magnitudes of the tile and of a one-pixel halo in LDS (a halo
// position outside the layer holds the magnitude AT THE CLAMPED COORDINATE: LbpFilter's BORDER_REPLICATE replicates its own input,
// the magnitude image, not the gray layer under it) and writes the LBP codes of the tile's pixels from there.
// LDS: mag[(GL_TH + 2) * GL_PITCH] bytes, then the 256 uniform-map entries (FD_LBP8_UNIFORM only; one entry per thread).
constexpr int GL_TW = 64, GL_TH = 16, GL_PITCH = GL_TW + 4;
__global__ __launch_bounds__(256) void k_gradmag_lbp(uint8_t* __restrict__ arena, int ksize, int type, FilterJobs jobs) {
    __shared__ uint8_t mag[(GL_TH + 2) * GL_PITCH];
    __shared__ uint8_t utab[256];
    const FilterJob jb = jobs.j[blockIdx.y];
    const uint8_t* src = arena + jb.src_off;
    uint8_t* dst = arena + jb.dst_off;
    const int w = jb.w, h = jb.h;
    const int tilesX = (w + GL_TW - 1) / GL_TW, ntiles = tilesX * ((h + GL_TH - 1) / GL_TH);
    if ((int)blockIdx.x >= ntiles) return;   // the grid is sized for the layer with the most tiles
    if (type == FD_LBP8_UNIFORM) utab[threadIdx.x] = (uint8_t)lbp_uniform_index(threadIdx.x);   // visible behind the first barrier below
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // the same trip count for every thread of the workgroup
        const int ty = tile / tilesX, tx = tile - ty * tilesX;
        const int x0 = tx * GL_TW, y0 = ty * GL_TH;
        for (int i = threadIdx.x; i < (GL_TW + 2) * (GL_TH + 2); i += 256) {
            const int hy = i / (GL_TW + 2), hx = i - hy * (GL_TW + 2);
            const int x = min(max(x0 + hx - 1, 0), w - 1), y = min(max(y0 + hy - 1, 0), h - 1);
            int gx, gy;
            const float scale = grad_pair(src, w, h, x, y, ksize, gx, gy);
            const int vx = min(255, max(0, __float2int_rn(127.f + scale * gx))), vy = min(255, max(0, __float2int_rn(127.f + scale * gy)));
            mag[hy * GL_PITCH + hx] = (uint8_t)grad_magnitude(vx, vy);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < GL_TW * GL_TH; i += 256) {
            const int ly = i / GL_TW, lx = i - ly * GL_TW;
            const int x = x0 + lx, y = y0 + ly;
            if (x < w && y < h) {
                const uint8_t* C = mag + (ly + 1) * GL_PITCH + 1;   // the halo resolves the border
                int code = lbp_raw_code(C - GL_PITCH, C, C + GL_PITCH, lx - 1, lx, lx + 1, type);
                if (type == FD_LBP8_UNIFORM) code = utab[code];
                dst[(size_t)y * w + x] = (uint8_t)code;
            }
        }
        __syncthreads();   // the next tile overwrites mag
    }
}

// GreyWorldNormalizationFilter.cpp:20-71 -- pass 1: per-channel sum and max
__global__ void k_greyworld_stats(const uint8_t* __restrict__ bgr, int n, unsigned long long* sums, unsigned int* maxs) {
    unsigned long long s[3] = {0, 0, 0};
    unsigned int m[3] = {0, 0, 0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        for (int c = 0; c < 3; ++c) {
            unsigned int v = bgr[3 * (size_t)i + c];
            s[c] += v;
            m[c] = max(m[c], v);
        }
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) {
            s[c] += __shfl_down(s[c], o, 64);
            m[c] = max(m[c], (unsigned int)__shfl_down((int)m[c], o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&sums[c], s[c]);
            atomicMax(&maxs[c], m[c]);
        }
    }
}
__global__ void k_greyworld_apply(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ dst, int n, double s0, double s1,
                                  double s2) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double sc[3] = {s0, s1, s2};
        for (int c = 0; c < 3; ++c) {
            int v = __double2int_rn(sc[c] * (double)bgr[3 * (size_t)i + c]);
            dst[3 * (size_t)i + c] = (uint8_t)min(255, max(0, v));
        }
    }
}

// ---- FD_IMAGE_GREYWORLD_GRAY: GreyWorldNormalizationFilter -> GrayscaleFilter in front of the layers, no host round trip ----
// Two launches replace the gray conversion, blockIdx.y = frame like k_frames_to_gray: k_gw_stats leaves every frame's channel sums
// and maxima in the pyramid's GwStats records (integer atomics: the result does not depend on the arrival order), k_gw_gray turns
// them into the three scales and converts.  The kernel boundary is the fence between the two.
struct GwStats {   // one 64-byte record per frame, cleared on the stream before every update
    unsigned long long sum[3];
    unsigned int max[3];
    unsigned int pad[7];
};
static_assert(sizeof(GwStats) == 64, "one record per 64-byte line");
constexpr int GW_GQ = 4;   // quads (four pixels, three dwords) per thread and pass, their loads in flight together

// three dwords = four BGR pixels (bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3), from an aligned or an unaligned frame
__device__ __forceinline__ void gw_load3(const uint8_t* __restrict__ src, bool aligned, int q, uint32_t (&w)[3]) {
    if (aligned) {
        const uint32_t* s3 = reinterpret_cast<const uint32_t*>(src) + 3 * (size_t)q;
        w[0] = s3[0]; w[1] = s3[1]; w[2] = s3[2];
    } else {
        const uint8_t* s1 = src + 12 * (size_t)q;
        w[0] = ld_u32_unaligned(s1); w[1] = ld_u32_unaligned(s1 + 4); w[2] = ld_u32_unaligned(s1 + 8);
    }
}

// A thread's sums stay in 32 bits: with 256 threads per workgroup a thread meets fewer than 2^31 / 256 pixels of at most 255.
__global__ __launch_bounds__(256) void k_gw_stats(FramePtrs frames, GwStats* __restrict__ stats, int n) {
    const uint8_t* __restrict__ src = frames.p[blockIdx.y];
    const int nq = n >> 2;
    const bool aligned = ((uintptr_t)src & 3) == 0;
    const int stride = gridDim.x * blockDim.x;
    uint32_t s[3] = {0, 0, 0}, m[3] = {0, 0, 0};
    auto pixel = [&](uint32_t b, uint32_t g, uint32_t r) {
        s[0] += b; s[1] += g; s[2] += r;
        m[0] = max(m[0], b); m[1] = max(m[1], g); m[2] = max(m[2], r);
    };
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += GW_GQ * stride) {
        uint32_t w[GW_GQ][3];
#pragma unroll
        for (int i = 0; i < GW_GQ; ++i) gw_load3(src, aligned, min(q + i * stride, nq - 1), w[i]);
#pragma unroll
        for (int i = 0; i < GW_GQ; ++i)
            if (q + i * stride < nq) {
                pixel(w[i][0] & 255u, (w[i][0] >> 8) & 255u, (w[i][0] >> 16) & 255u);
                pixel(w[i][0] >> 24, w[i][1] & 255u, (w[i][1] >> 8) & 255u);
                pixel((w[i][1] >> 16) & 255u, w[i][1] >> 24, w[i][2] & 255u);
                pixel((w[i][2] >> 8) & 255u, (w[i][2] >> 16) & 255u, w[i][2] >> 24);
            }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < (n & 3)) {   // tail
        const size_t i = ((size_t)nq << 2) + threadIdx.x;
        pixel(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
    }
    // registers -> wave -> workgroup -> one atomic per statistic
    __shared__ unsigned long long ls[4][3];
    __shared__ unsigned int lm[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned long long sc = s[c];
        unsigned int mc = m[c];
        for (int o = 32; o > 0; o >>= 1) {
            sc += __shfl_down(sc, o, 64);
            mc = max(mc, (unsigned int)__shfl_down((int)mc, o, 64));
        }
        if ((threadIdx.x & 63) == 0) { ls[threadIdx.x >> 6][c] = sc; lm[threadIdx.x >> 6][c] = mc; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        atomicAdd(&stats[blockIdx.y].sum[c], ls[0][c] + ls[1][c] + ls[2][c] + ls[3][c]);
        atomicMax(&stats[blockIdx.y].max[c], max(max(lm[0][c], lm[1][c]), max(lm[2][c], lm[3][c])));
    }
}

// The scales in double and in the reference's operation order (GreyWorldNormalizationFilter.cpp:46-60; the same operations and
// comparisons as fd_greyworld's host code, so NaN and infinity propagate alike).  saturate(cvRound(scale_c * v)) depends only on
// the channel and the byte value: the workgroup builds the three tables once, with the gray weights (and the rounding term)
// folded in -- (tab[0][b] + tab[1][g] + tab[2][r]) >> 14 is gray_of() of the normalised pixel, which is never written to memory.
// The first pass's loads are issued before the tables are built.
__global__ __launch_bounds__(256) void k_gw_gray(FramePtrs frames, const GwStats* __restrict__ stats, uint8_t* __restrict__ grayBase,
                                                 size_t imageStride, int n) {
    __shared__ double scale[3];
    __shared__ uint32_t tab[3][256];
    const uint8_t* __restrict__ src = frames.p[blockIdx.y];
    uint8_t* __restrict__ gray = grayBase + (size_t)blockIdx.y * imageStride;
    const int nq = n >> 2;
    const bool aligned = ((uintptr_t)src & 3) == 0;
    const int stride = gridDim.x * blockDim.x;
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t w[GW_GQ][3] = {};
    if (q < nq) {
#pragma unroll
        for (int i = 0; i < GW_GQ; ++i) gw_load3(src, aligned, min(q + i * stride, nq - 1), w[i]);
    }
    if (threadIdx.x < 64) {   // one wave, every lane the same values
        const GwStats& S = stats[blockIdx.y];
        double mean[3], maxNew[3];
        for (int c = 0; c < 3; ++c) { mean[c] = (double)S.sum[c] / n; maxNew[c] = (uint8_t)S.max[c] / mean[c]; }
        double mx = maxNew[0];
        if (maxNew[1] > mx) mx = maxNew[1];
        if (maxNew[2] > mx) mx = maxNew[2];
        if (threadIdx.x == 0)
            for (int c = 0; c < 3; ++c) scale[c] = 255.0 / (mean[c] * mx);
    }
    __syncthreads();
    {
        const uint32_t v = threadIdx.x;
        const uint32_t wgt[3] = {1868u, 9617u, 4899u};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int r = __double2int_rn(scale[c] * (double)v);
            tab[c][v] = (uint32_t)min(255, max(0, r)) * wgt[c] + (c == 0 ? 8192u : 0u);
        }
    }
    __syncthreads();
    auto gray1 = [&](uint32_t b, uint32_t g, uint32_t r) { return (tab[0][b] + tab[1][g] + tab[2][r]) >> 14; };
    auto gray4 = [&](const uint32_t (&x)[3]) {
        const uint32_t g0 = gray1(x[0] & 255u, (x[0] >> 8) & 255u, (x[0] >> 16) & 255u);
        const uint32_t g1 = gray1(x[0] >> 24, x[1] & 255u, (x[1] >> 8) & 255u);
        const uint32_t g2 = gray1((x[1] >> 16) & 255u, x[1] >> 24, x[2] & 255u);
        const uint32_t g3 = gray1((x[2] >> 8) & 255u, (x[2] >> 16) & 255u, x[2] >> 24);
        return g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    };
    while (q < nq) {
        const int qn = q + GW_GQ * stride;
        uint32_t wn[GW_GQ][3] = {};
        if (qn < nq) {   // the next pass's loads in flight under this pass's table reads
#pragma unroll
            for (int i = 0; i < GW_GQ; ++i) gw_load3(src, aligned, min(qn + i * stride, nq - 1), wn[i]);
        }
#pragma unroll
        for (int i = 0; i < GW_GQ; ++i)
            if (q + i * stride < nq) reinterpret_cast<uint32_t*>(gray)[q + i * stride] = gray4(w[i]);
#pragma unroll
        for (int i = 0; i < GW_GQ; ++i) { w[i][0] = wn[i][0]; w[i][1] = wn[i][1]; w[i][2] = wn[i][2]; }
        q = qn;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < (n & 3)) {   // tail
        const size_t i = ((size_t)nq << 2) + threadIdx.x;
        gray[i] = (uint8_t)gray1(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
    }
}

inline uint32_t align256(size_t v) { return (uint32_t)((v + 255) & ~(size_t)255); }

// GradientBinningFilter.cpp:18-60 -- built on the host with libm, exactly like the reference ctor
void build_gradient_lut(int bins, bool signedGradients, bool interpolate, std::vector<uint8_t>& lut) {
    const double PI = 3.1415926535897932384626433832795;
    const int E = interpolate ? 4 : 2;
    lut.resize((size_t)65536 * E);
    for (int x = 0; x < 256; ++x) {
        double gradientX = ((double)x - 127) / 255;
        for (int y = 0; y < 256; ++y) {
            double gradientY = ((double)y - 127) / 255;
            double direction = std::atan2(gradientY, gradientX);
            double magnitude = std::sqrt(gradientX * gradientX + gradientY * gradientY);
            double bin;
            if (signedGradients) {
                direction += PI;
                bin = direction * bins / (2 * PI);
            } else {
                if (direction < 0) direction += PI;
                bin = direction * bins / PI;
            }
            auto sat = [](double v) { int r = fd_cvRound(v); return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r)); };
            size_t index = (size_t)x | ((size_t)y << 8);
            if (!interpolate) {
                lut[2 * index] = (uint8_t)((uint8_t)std::round(bin) % (unsigned)bins);
                lut[2 * index + 1] = sat(255 * magnitude);
            } else {
                uint8_t w1 = sat(255 * magnitude * (bin - std::floor(bin)));
                lut[4 * index] = (uint8_t)((uint8_t)std::floor(bin) % (unsigned)bins);
                lut[4 * index + 1] = sat(255 * magnitude - w1);
                lut[4 * index + 2] = (uint8_t)((uint8_t)std::ceil(bin) % (unsigned)bins);
                lut[4 * index + 3] = w1;
            }
        }
    }
}

// layer filters that start with GradientFilter (and so with its optional blur)
bool layer_takes_gradients(int kind) { return kind == FD_LAYER_GRADBIN || kind == FD_LAYER_GRADMAG_LBP; }
int grid_for(int npix) { return std::max(1, std::min(1024, (npix + 255) / 256)); }
int tile_grid_for(int ntiles) { return std::max(1, std::min(1024, ntiles)); }
int gradmag_lbp_tiles(int w, int h) { return ((w + GL_TW - 1) / GL_TW) * ((h + GL_TH - 1) / GL_TH); }

// ---- the launch plan: what an update enqueues behind the gray image ----------------------------------------------------------
// All of it depends only on what build_layout fixes (frame size, pyramid parameters, layer filter, number of frames), so it is
// built once with the layout and an update only walks it.  Offsets and sizes only, never a device pointer: a DevBuf may move.
struct ResizeLaunch {   // k_resize_tiled
    ResizeJobs jobs;
    int grid;
};
struct FusedLaunch {    // k_resize_down
    FusedJobs jobs;
    uint32_t tileTab;   // its tile list in rtab (offset in int2 entries) ...
    int tilesPerFrame;  // ... and the number of tiles per frame
    int grid;
};
struct DownLaunch {     // k_pyrdown_tiled: the pyrDowns of up to MAXJ layers of one generation
    int njobs;
    int ntile;          // tiles per frame: the grid
    uint32_t tileTab;   // its PdTile list in rtab (offset in int2 entries)
};
struct FilterLaunch {   // k_gradbin / k_lbp / k_gradmag_lbp, behind k_box_blur where GradientFilter blurs (blur.n == jobs.n then, 0 otherwise)
    FilterJobs jobs, blur;
    int grid;       // workgroups per job of the per-pixel kernels
    int tileGrid;   // ... of k_gradmag_lbp: the tiles of the job with the most
};

}  // namespace

void fd_build_gradient_lut(int bins, bool signedGradients, bool interpolate, std::vector<uint8_t>& lut) {
    build_gradient_lut(bins, signedGradients, interpolate, lut);
}

struct fd_pyramid::Plan {   // in launch order
    std::vector<ResizeLaunch> resize;   // depth 0: resize from the full-resolution gray image
    std::vector<FusedLaunch> fused;     // first-octave layers with a pyrDown chain: resize + first pyrDown, the resized pixels stay in LDS
    std::vector<DownLaunch> down;       // generation 1 of the chains k_resize_down does not cover, then generation 2, 3, ...
    std::vector<FilterLaunch> filter;   // the layer filter over the kept layers
};
fd_pyramid::~fd_pyramid() { if (ready) (void)hipEventDestroy(ready); }

namespace {

// The slot of a stage's next job.  A launch takes MAXJ jobs (they travel by value).
template <class Launch>
auto& next_job(std::vector<Launch>& launches) {
    if (launches.empty() || launches.back().jobs.n == MAXJ) launches.emplace_back();   // value-initialised: no jobs yet
    auto& jobs = launches.back().jobs;
    return jobs.j[jobs.n++];
}

// The cv::resize column table of a fused layer of width dw0 from a frame of width W: the kernel's own float expressions
// (k_resize_tiled's srcX), evaluated once per geometry on the host (this file is built with -ffp-contract=off)
std::vector<int2> fused_xtab(int dw0, int W, double scale_x) {
    std::vector<int2> xt((size_t)dw0);
    for (int dx = 0; dx < dw0; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= W - 1) { fx = 0; sx = W - 1; }
        const int a0 = (int)nearbyintf((1.f - fx) * 2048), a1 = (int)nearbyintf(fx * 2048);
        xt[(size_t)dx] = make_int2(sx, a0 | (a1 << 16));
    }
    return xt;
}
// the source columns of tile column tx, exactly as the kernel's addressing expects them: {X0, ncol}
int2 fused_tile_cols(const std::vector<int2>& xt, int W, int tx) {
    const int dw0 = (int)xt.size(), gx0 = 2 * tx * FT_W1 - 2;
    const int cLo = std::max(0, gx0), cHi = std::min(dw0 - 1, gx0 + G0_W - 1);
    const int X0 = xt[(size_t)cLo].x;
    return make_int2(X0, std::min(W - 1, xt[(size_t)cHi].x + 1) - X0 + 1);
}
// every tile's source columns must fit the kernel's stage (its rows are staged per resized row: no limit there)
bool fused_fits(const std::vector<int2>& xt, int W, int dw1) {
    for (int tx = 0; tx * FT_W1 < dw1; ++tx)
        if (fused_tile_cols(xt, W, tx).y > FS_PITCH) return false;
    return true;
}

void build_plan(fd_pyramid* p, int W, int H) {
    p->plan.reset(new fd_pyramid::Plan());
    fd_pyramid::Plan& plan = *p->plan;
    const std::vector<HostLayer>& all = p->all;
    const int NI = p->nimg;
    static const int mode = [] { const char* e = getenv("FD_PYR_FUSED"); return e ? atoi(e) : 1; }();   // 0: never, 1: default, 2: kept layers too
    std::vector<char> fused(all.size(), 0);   // the depth-0 layers that k_resize_down resizes, together with their pyrDown
    // rtab: the cv::resize column tables of the fused layers -- the kernel's own float expressions (k_resize_tiled's srcX), evaluated
    // once per geometry on the host (this file is built with -ffp-contract=off) --, behind them one tile list per k_resize_down
    // launch, then one per k_pyrdown_tiled launch
    std::vector<int2> tab;
    std::vector<std::vector<int4>> tiles;     // {X0, ncol, tx | ty << 16, chain of the launch}
    for (size_t k = 0; k < all.size(); ++k) {
        const HostLayer& L = all[k];
        if (L.depth != 0) continue;
        // the scale-1 layer IS the gray image (build_layout): nothing to resize, and its pyrDown stays with k_pyrdown_tiled (through
        // k_resize_down with identity tables it costs +35 us per 64-frame call against 15 us saved: the resize arithmetic is not free)
        if (L.w == W && L.h == H && L.gray_off == p->gray_full_off) continue;
        const double scale_x = 1. / ((double)L.w / W), scale_y = 1. / ((double)L.h / H);
        // k_resize_tiled stages at most TL_ROWS x TL_PITCH source bytes per 64 x 32 tile: 1 <= scale <= 2.05.  build_layout only makes
        // depth-0 layers of w = cvRound(W * s) with s = inc^i, i < octl, inc = 0.5^(1 / octl), so 0.5 < s <= 1.  s <= 1 gives W / w >= 1.
        // Odd W = 2 k + 1: W * s > k + 0.5, so w >= k + 1 and W / w < 2; even W = 2 k: W * s > k, so w >= k and W / w <= 2 (reached at
        // W = 2).  The same holds for H.
        if (!(scale_x >= 1.0 && scale_x <= 2.05 && scale_y >= 1.0 && scale_y <= 2.05))
            FD_THROW(FD_ERR_RUNTIME, "ImagePyramid: first-octave layer %d x %d of a %d x %d image is outside the resize kernel's range", L.w, L.h, W, H);
        // A first-octave layer that is itself a kept layer (config 2's pyramid: scales up to 1) has to be written anyway: the fusion saves
        // nothing there and the fused kernel is the slower resize (round 3: 699 us per 640x480 frame; k_resize_tiled + k_pyrdown_tiled:
        // 101 + 4 x 68 us, round 4).  FD_PYR_FUSED=2 fuses those too (A/B).  Also measured in round 4 and dropped: persistent
        // k_pyrdown_tiled workgroups with the next tile's loads in flight (69 vs 63 us per 64-frame headline call).
        const bool chain = k + 1 < all.size() && all[k + 1].depth == 1 && all[k + 1].chain == L.chain;
        if (chain && mode != 0 && (!L.kept || mode == 2) && L.w >= 3 && L.h >= 3 && W <= 65535 && H <= 65535) {
            const HostLayer& D = all[k + 1];
            const std::vector<int2> xt = fused_xtab(L.w, W, scale_x);
            const bool fits = fused_fits(xt, W, D.w);
            if (fits) {
                FusedJob& j = next_job(plan.fused);
                j.dw0 = L.w; j.dh0 = L.h; j.dw1 = D.w; j.dh1 = D.h;
                j.dst0_off = L.kept ? L.gray_off : 0xffffffffu;
                j.dst1_off = D.gray_off;
                j.xtab = (uint32_t)tab.size();
                j.scale_y = scale_y;
                tab.insert(tab.end(), xt.begin(), xt.end());
                tiles.resize(plan.fused.size());
                for (int ty = 0; ty * FT_H1 < D.h; ++ty)
                    for (int tx = 0; tx * FT_W1 < D.w; ++tx) {
                        const int2 cols = fused_tile_cols(xt, W, tx);
                        tiles.back().push_back(make_int4(cols.x, cols.y, (int)((uint32_t)tx | (uint32_t)ty << 16), plan.fused.back().jobs.n - 1));
                    }
                fused[k] = 1;
                continue;
            }
        }
        ResizeJob& j = next_job(plan.resize);
        j.dw = L.w; j.dh = L.h; j.dst_off = L.gray_off;
        j.scale_x = scale_x;
        j.scale_y = scale_y;
        ResizeLaunch& R = plan.resize.back();
        R.grid = std::max(R.grid, tile_grid_for(((L.w + TL_W - 1) / TL_W) * ((L.h + TL_H - 1) / TL_H)));
    }
    if (!plan.fused.empty()) {
        const int perCu = fd_blocks_per_cu<k_resize_down>(256, 4);
        for (size_t g = 0; g < plan.fused.size(); ++g) {   // 16-byte entries behind the 8-byte ones, 16-byte aligned
            FusedLaunch& F = plan.fused[g];
            if (tab.size() & 1) tab.push_back(make_int2(0, 0));
            F.tileTab = (uint32_t)tab.size();
            F.tilesPerFrame = (int)tiles[g].size();
            for (const int4& t : tiles[g]) { tab.push_back(make_int2(t.x, t.y)); tab.push_back(make_int2(t.z, t.w)); }
            // persistent workgroups; a multiple of the 8 XCDs for a multi-frame pyramid (every frame is then resized on one XCD)
            F.grid = (int)std::min<int64_t>((int64_t)F.tilesPerFrame * NI, (int64_t)p->ctx->num_cus * perCu);
            if (NI >= 8 && F.grid >= 64) F.grid &= ~7;
        }
    }
    // (Measured and dropped, twice.  Round 3: one workgroup walking all deeper generations of a chain tile by tile -- 160 us per 64-frame
    // call against 57 us for the per-generation launches, 32 serial tiles per workgroup.  Round 5: k_pyrdown_chain, a workgroup owning a
    // 16 x 16 tile of the deepest generation and computing the 35 / 73 / 149-pixel boxes above it in LDS (halo recomputed, reflected
    // borders materialised; bit-exact on every pyramid test) -- ONE launch of 121 us instead of three of 11.4 us, headline 3270 -> 2690
    // Mpatches/s: 1.8x the outputs (halo) at ~60 instructions each, against ~12 per output of the column walk of k_pyrdown_tiled, which
    // shares the row dot products between vertically adjacent outputs.  The per-generation launches are latency-bound but cheap.)
    int maxDepth = 0;
    for (const HostLayer& L : all) maxDepth = std::max(maxDepth, L.depth);
    // One flat tile list per launch, layer after layer (exact grids: no empty workgroups).  A launch takes MAXJ layers, and a
    // generation never tops up the last launch of the generation it reads.
    static_assert(sizeof(PdTile) == 4 * sizeof(int2), "PdTile entries in rtab");
    for (int d = 1; d <= maxDepth; ++d) {
        const size_t first = plan.down.size();
        for (size_t k = 1; k < all.size(); ++k) {
            const HostLayer& L = all[k];
            if (L.depth != d || fused[k - 1]) continue;
            const HostLayer& S = all[k - 1];   // previous entry of the same chain
            if (plan.down.size() == first || plan.down.back().njobs == MAXJ) {
                if (tab.size() & 1) tab.push_back(make_int2(0, 0));
                plan.down.push_back(DownLaunch{0, 0, (uint32_t)tab.size()});
            }
            DownLaunch& D = plan.down.back();
            const int nt = pd_tiles(S.w, S.h);
            for (int t = 0; t < nt; ++t) {
                const PdTile e = pd_tile_entry(S.w, S.h, S.gray_off, L.gray_off, t);
                int2 q[4];
                std::memcpy(q, &e, sizeof(e));
                tab.insert(tab.end(), q, q + 4);
            }
            D.njobs++;
            D.ntile += nt;
        }
    }
    if (!tab.empty()) {
        p->rtab.reserve(sizeof(int2) * tab.size());
        HIP_CHECK(hipMemcpy(p->rtab.p, tab.data(), sizeof(int2) * tab.size(), hipMemcpyHostToDevice));
    }
    if (p->filter_kind != FD_LAYER_NONE) {
        const bool blur = layer_takes_gradients(p->filter_kind) && p->grad_blur > 0;
        for (int k : p->kept) {
            const HostLayer& L = all[k];
            FilterJob& j = next_job(plan.filter);
            j.w = L.w; j.h = L.h; j.src_off = blur ? L.blur_off : L.gray_off; j.dst_off = L.filt_off;
            FilterLaunch& F = plan.filter.back();
            if (blur) {   // GradientFilter's blur: gray layer -> blurred copy; the gradients are then taken of the copy
                FilterJob& b = F.blur.j[F.blur.n++];
                b.w = L.w; b.h = L.h; b.src_off = L.gray_off; b.dst_off = L.blur_off;
            }
            F.grid = std::max(F.grid, grid_for(L.w * L.h));
            F.tileGrid = std::max(F.tileGrid, tile_grid_for(gradmag_lbp_tiles(L.w, L.h)));
        }
    }
}

// the settings a layout depends on have changed: the next update builds a new one, and with it a new launch plan
void invalidate_layout(fd_pyramid* p) {
    p->all.clear();
    p->img_w = p->img_h = 0;
}

void build_layout(fd_pyramid* p, int W, int H) {
    invalidate_layout(p);   // until the layout and its plan are complete: a throw below leaves nothing half-built to be used
    p->kept.clear();
    size_t off = 0;
    p->gray_full_off = 0;
    off = align256((size_t)W * H);
    const int fch = p->filter_kind == FD_LAYER_GRADBIN ? (p->interpolate ? 4 : 2) : 1;
    for (size_t i = 0; i < p->octl; ++i) {
        double scaleFactor = std::pow(p->inc, (double)i);
        int w = fd_cvRound(W * scaleFactor), h = fd_cvRound(H * scaleFactor);
        if (w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "ImagePyramid: layer %zu would be empty", i);
        int depth = 0;
        // a first-octave layer of the image's own size (scale 1) IS the gray image: cv::resize to the same size copies every pixel
        // (weights 2048 / 0: ((2048 * (S * 128)) >> 16) + 2 >> 2 == S), so it shares the gray image's storage and costs no launch
        const bool isFull = (w == W && h == H);
        HostLayer L{(int)i, scaleFactor, w, h, 1, (uint32_t)(isFull ? p->gray_full_off : off), 0, scaleFactor <= p->maxS && scaleFactor >= p->minS, (int)i, depth};
        if (!isFull) off = align256(off + (size_t)w * h);
        p->all.push_back(L);
        int pw = w, ph = h;
        scaleFactor *= 0.5;
        for (size_t j = 1; scaleFactor >= p->minS && pw > 1; ++j, scaleFactor *= 0.5) {
            int dw = (pw + 1) / 2, dh = (ph + 1) / 2;
            HostLayer D{(int)(i + j * p->octl), scaleFactor, dw, dh, 1, (uint32_t)off, 0, scaleFactor <= p->maxS, (int)i, (int)j};
            off = align256(off + (size_t)dw * dh);
            p->all.push_back(D);
            pw = dw;
            ph = dh;
        }
    }
    for (size_t k = 0; k < p->all.size(); ++k) {
        HostLayer& L = p->all[k];
        if (!L.kept) continue;
        L.ch = fch;
        if (p->filter_kind == FD_LAYER_NONE) L.filt_off = L.gray_off;
        else {
            L.filt_off = (uint32_t)off;
            off = align256(off + (size_t)L.w * L.h * fch);
            if (layer_takes_gradients(p->filter_kind) && p->grad_blur > 0) {
                L.blur_off = (uint32_t)off;
                off = align256(off + (size_t)L.w * L.h);
            }
        }
        p->kept.push_back((int)k);
    }
    if (off > 0xfffffff0ull) FD_THROW(FD_ERR_INVALID_ARGUMENT, "ImagePyramid: pyramid exceeds 4 GB arena");
    std::sort(p->kept.begin(), p->kept.end(), [&](int a, int b) { return p->all[a].index < p->all[b].index; });
    p->arena_bytes = off + 256;
    p->image_stride = (p->arena_bytes + 255) & ~(size_t)255;
    if (p->nimg > 1 && p->image_stride * (size_t)p->nimg > 0xfffffff0ull * 16) FD_THROW(FD_ERR_INVALID_ARGUMENT, "ImagePyramid: multi-frame pyramid too large");
    p->arena.reserve(p->image_stride * (size_t)p->nimg);
    p->h_layer_table.clear();
    for (int k : p->kept) {
        const HostLayer& L = p->all[k];
        p->h_layer_table.push_back(LayerDesc{L.w, L.h, L.ch, 0, L.gray_off, L.filt_off});
    }
    p->layer_table.reserve(sizeof(LayerDesc) * std::max<size_t>(1, p->h_layer_table.size()));
    if (!p->h_layer_table.empty())
        HIP_CHECK(hipMemcpyAsync(p->layer_table.p, p->h_layer_table.data(), sizeof(LayerDesc) * p->h_layer_table.size(),
                                 hipMemcpyHostToDevice, p->ctx->stream));
    build_plan(p, W, H);
    p->img_w = W;
    p->img_h = H;
}

// (Measured and dropped in round 5: single-image updates replayed as a hipGraph -- captured with hipStreamBeginCapture around the launch
// code below on the second update with the same layout, the image address patched into the k_bgr2gray node with
// hipGraphExecKernelNodeSetParams.  Bit-exact and the call returned after 10 instead of 18 us, but a blocking 640x480 frame took
// 153.5 us p50 against 146 with plain launches (ROCm 7.2: the graph's first node starts later than a plain kernel would), and the
// 15-detector batch 5723 against 5871 Mpatches/s.  The rocprofv3 timeline that motivated it: k_bgr2gray 3.3 + k_resize_down 5.9 + 4 x
// k_pyrdown_tiled ~4.5 us = 27 us of kernels spread over 48 us, the host's ~3.5 us per launch between them.)
void pyramid_update(fd_pyramid* p, const uint8_t* image, int W, int H, int ch, int is_device, hipStream_t st, const uint8_t* const* frames = nullptr) {
    if (!image && !frames) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update: image is NULL");
    if (p->nimg > 1 && !frames) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update: the pyramid holds %d frames, use fd_pyramid_update_frames", p->nimg);
    if (p->nimg > 1 && p->filter_kind != FD_LAYER_NONE) FD_THROW(FD_ERR_INVALID_ARGUMENT, "multi-frame pyramids have no layer filters");
    if (W < 1 || H < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update: empty image");
    if (ch != 1 && ch != 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update: image must have 1 or 3 channels");
    const bool greyworld = p->image_filter != FD_IMAGE_GRAY;
    if (greyworld && ch != 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GreyWorldNormalizationFilter: The image type must be CV_8UC3");
    if (greyworld && (size_t)W * H > 0x7fffffffull) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GreyWorldNormalizationFilter: image too large");
    if (W != p->img_w || H != p->img_h || p->all.empty()) build_layout(p, W, H);
    uint8_t* arena = p->arena.as<uint8_t>();
    uint8_t* gray = arena + p->gray_full_off;
    const size_t npix = (size_t)W * H, bytes = npix * ch;
    const int NI = p->nimg;   // a single image is one frame: without `frames` the pyramid holds one (checked above)
    const size_t IS = p->image_stride;
    // the caller's image(s) as device addresses: host images pass through the staging buffer
    FramePtrs fp{};
    if (!is_device) p->input.reserve(bytes * NI);
    for (int f = 0; f < NI; ++f) {
        fp.p[f] = frames ? frames[f] : image;
        if (!is_device) {
            uint8_t* staged = p->input.as<uint8_t>() + (size_t)f * bytes;
            HIP_CHECK(hipMemcpyAsync(staged, fp.p[f], bytes, hipMemcpyHostToDevice, st));
            fp.p[f] = staged;
        }
    }
    if (greyworld) {   // FD_IMAGE_GREYWORLD_GRAY: the statistics of every frame, then normalisation + gray conversion in one pass
        GwStats* stats = p->gw_stats.as<GwStats>();
        HIP_CHECK(hipMemsetAsync(stats, 0, sizeof(GwStats) * (size_t)NI, st));
        // persistent workgroups, one pass of 1024 quads each where the frame is small.  At most one workgroup per CU and frame (a
        // 1080p frame: 256 workgroups, 256 atomics per statistic) and about four per CU in all (64 frames: 16 per frame).  Twice
        // and four times as many were slower in both shapes (one frame: the atomics on six addresses)
        const int cus = std::max(1, p->ctx->num_cus);
        const int perFrame = std::max(1, std::min(cus, 4 * cus / NI));
        const int gx = std::max(1, std::min((int)((npix / 4 + 1023) / 1024), perFrame));
        hipLaunchKernelGGL(k_gw_stats, dim3(gx, NI), dim3(256), 0, st, fp, stats, (int)npix);
        hipLaunchKernelGGL(k_gw_gray, dim3(gx, NI), dim3(256), 0, st, fp, stats, gray, IS, (int)npix);
    } else if (frames) {   // one launch converts / copies all frames into their arenas, four quads per thread
        hipLaunchKernelGGL(k_frames_to_gray, dim3(grid_for((int)(npix / 16 + 1)), NI), dim3(256), 0, st, fp, gray, IS, (int)npix, ch);
    } else if (ch == 3) {
        hipLaunchKernelGGL(k_bgr2gray, dim3(grid_for((int)npix)), dim3(256), 0, st, fp.p[0], gray, (int)npix);
    } else {
        HIP_CHECK(hipMemcpyAsync(gray, fp.p[0], npix, hipMemcpyDeviceToDevice, st));
    }
    // everything behind the gray image: the resizes, the pyrDown chains, the layer filters
    const fd_pyramid::Plan& plan = *p->plan;
    for (const ResizeLaunch& R : plan.resize)
        hipLaunchKernelGGL(k_resize_tiled, dim3(R.grid, R.jobs.n, NI), dim3(256), 0, st, arena, arena, p->gray_full_off, W, H, R.jobs, IS);
    for (const FusedLaunch& F : plan.fused)
        hipLaunchKernelGGL(k_resize_down, dim3(F.grid), dim3(256), 0, st, arena, p->gray_full_off, W, H, p->rtab.as<int2>(), F.jobs, F.tileTab, F.tilesPerFrame, NI, IS);
    const bool downByXcd = NI >= 8 && NI % 8 == 0 && fd_knob_pyr_xcd();   // multi-frame: frame f's tiles on XCD f % 8
    for (const DownLaunch& D : plan.down) {   // one tile per workgroup
        const PdTile* tiles = reinterpret_cast<const PdTile*>(p->rtab.as<int2>() + D.tileTab);
        if (downByXcd)
            hipLaunchKernelGGL(k_pyrdown_tiled, dim3(8 * D.ntile, NI / 8), dim3(256), 0, st, arena, tiles, IS, 3);
        else
            hipLaunchKernelGGL(k_pyrdown_tiled, dim3(D.ntile, 1, NI), dim3(256), 0, st, arena, tiles, IS, 0);
    }
    for (const FilterLaunch& F : plan.filter) {
        const dim3 g(F.grid, F.jobs.n);
        if (F.blur.n) hipLaunchKernelGGL(k_box_blur, g, dim3(256), 0, st, arena, p->grad_blur, F.blur);
        if (p->filter_kind == FD_LAYER_GRADMAG_LBP)
            hipLaunchKernelGGL(k_gradmag_lbp, dim3(F.tileGrid, F.jobs.n), dim3(256), 0, st, arena, p->grad_kernel, p->lbp_type, F.jobs);
        else if (p->filter_kind != FD_LAYER_GRADBIN)
            hipLaunchKernelGGL(k_lbp, g, dim3(256), 0, st, arena, p->lbp_type, F.jobs);
        else if (p->interpolate)
            hipLaunchKernelGGL(k_gradbin<4>, g, dim3(256), 0, st, arena, p->lut.as<uint8_t>(), p->grad_kernel, F.jobs);
        else
            hipLaunchKernelGGL(k_gradbin<2>, g, dim3(256), 0, st, arena, p->lut.as<uint8_t>(), p->grad_kernel, F.jobs);
    }
    HIP_CHECK(hipGetLastError());
    if (!p->ready) HIP_CHECK(hipEventCreateWithFlags(&p->ready, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(p->ready, st));
    p->readyStream = st;
    p->version++;
}

}  // namespace

// fd_pyramid_update on an explicit stream (worker threads of the batch entry points); throws FdError
void fd_pyramid_update_on(fd_pyramid* p, const uint8_t* image, int w, int h, int ch, int is_device, hipStream_t st) {
    if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update: NULL pyramid");
    HIP_CHECK(hipSetDevice(p->ctx->device));
    pyramid_update(p, image, w, h, ch, is_device, st);
}

// DirectPyramidFeatureExtractor::extract(stepX, stepY, roi) window grid, :75-123
void fd_enumerate_layers(const fd_pyramid* p, int pw, int ph, int sx, int sy, const int* roiIn,
                         std::vector<WindowLayer>& out, int64_t& total) {
    if (sx < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "DirectPyramidFeatureExtractor: stepX has to be greater than zero");
    if (sy < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "DirectPyramidFeatureExtractor: stepY has to be greater than zero");
    if (pw < 1 || ph < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "DirectPyramidFeatureExtractor: empty patch size");
    int rx = 0, ry = 0, rw = 0, rh = 0;
    if (!roiIn && p->sel_has_roi) roiIn = p->sel_roi;   // fd_pyramid_select
    if (roiIn) { rx = roiIn[0]; ry = roiIn[1]; rw = roiIn[2]; rh = roiIn[3]; }
    if (rx == 0 && ry == 0 && rw == 0 && rh == 0) {
        rw = p->img_w;
        rh = p->img_h;
    } else {
        int nx = std::max(0, rx), ny = std::max(0, ry);
        rw = std::min(p->img_w, rw + nx) - nx;
        rh = std::min(p->img_h, rh + ny) - ny;
        rx = nx;
        ry = ny;
    }
    out.clear();
    total = 0;
    size_t viewCount = 0;
    for (size_t li = 0; li < p->kept.size(); ++li) {
        const HostLayer& L = p->all[p->kept[li]];
        auto scaled = [&](int v) { return fd_cvRound(v * L.scale); };     // ImagePyramidLayer.hpp:65-67
        auto original = [&](int v) { return fd_cvRound(v / L.scale); };   // :98-100
        WindowLayer wl;
        wl.layer = (int)li;
        wl.ow = original(pw);
        wl.oh = original(ph);
        wl.bx = scaled(rx);
        wl.by = scaled(ry);
        int ex = scaled(rx + rw), ey = scaled(ry + rh);
        // positions x = bx + k*sx with x + pw < ex  (strict)
        long spanx = (long)ex - pw - wl.bx, spany = (long)ey - ph - wl.by;
        wl.nx = spanx > 0 ? (int)((spanx - 1) / sx + 1) : 0;
        wl.ny = spany > 0 ? (int)((spany - 1) / sy + 1) : 0;
        // layer selection (DirectPyramidFeatureExtractor.cpp:99-107): every sel_step-th layer counted from the first one,
        // skipping indices below sel_first, stopping above sel_last
        // The step walks pyramid->getLayers() from its begin(): for a pyramid built on another one that is the first layer of its
        // scale range (fd_pyramid_select_view), not the source's first layer.
        const bool inView = (p->view_first < 0 || L.index >= p->view_first) && (p->view_last < 0 || L.index <= p->view_last);
        const size_t viewPos = viewCount;
        if (inView) ++viewCount;
        const bool selected = inView && (viewPos % (size_t)p->sel_step == 0) && (p->sel_first < 0 || L.index >= p->sel_first) &&
                              (p->sel_last < 0 || L.index <= p->sel_last);
        if (!selected) wl.nx = wl.ny = 0;
        // windows must lie inside the layer (cv::Mat(image, bounds) would assert otherwise)
        if (wl.nx > 0 && wl.ny > 0) {
            if (wl.bx < 0 || wl.by < 0 || wl.bx + (wl.nx - 1) * sx + pw > L.w || wl.by + (wl.ny - 1) * sy + ph > L.h)
                FD_THROW(FD_ERR_RUNTIME, "DirectPyramidFeatureExtractor: window outside of pyramid layer %d", L.index);
        } else {
            wl.nx = wl.ny = 0;
        }
        wl.first = total;
        total += (int64_t)wl.nx * wl.ny;
        out.push_back(wl);
    }
}

extern "C" {

int fd_pyramid_create(fd_ctx* ctx, int octl, double minS, double maxS, fd_pyramid** out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_create: NULL argument");
        if (octl <= 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "the number of layers per octave must be greater than zero");
        if (minS <= 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "the minimum scale factor must be greater than zero");
        if (maxS > 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "the maximum scale factor must not exceed one");
        fd_pyramid* p = new fd_pyramid();
        p->ctx = ctx;
        p->octl = (size_t)octl;
        p->inc = std::pow(0.5, 1. / octl);
        p->minS = minS;
        p->maxS = maxS;
        *out = p;
    });
}

int fd_pyramid_create_inc(fd_ctx* ctx, double inc, double minS, double maxS, fd_pyramid** out) {
    return fd_guard(ctx, [&] {
        if (inc <= 0 || inc >= 1)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "the incremental scale factor must be greater than zero and smaller than one");
    }) ?: fd_pyramid_create(ctx, (int)std::round(std::log(0.5) / std::log(inc)), minS, maxS, out);
}

void fd_pyramid_destroy(fd_pyramid* p) { delete p; }

int fd_pyramid_set_layer_filter(fd_pyramid* p, int kind, int bins, int signed_gradients, int interpolate, int grad_kernel,
                                int lbp_type) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_set_layer_filter: NULL pyramid");
        if (kind == FD_LAYER_GRADBIN) {
            if (grad_kernel != 1 && grad_kernel != 3 && grad_kernel != 5 && grad_kernel != 7 && grad_kernel != FD_GRAD_SCHARR)
                FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientFilter: the kernel size must be 1, 3, 5, 7 or CV_SCHARR");
            if (bins < 1 || bins > 255) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientBinningFilter: bins must be in 1..255");
            std::vector<uint8_t> lut;
            build_gradient_lut(bins, signed_gradients != 0, interpolate != 0, lut);
            p->lut.reserve(lut.size());
            HIP_CHECK(hipMemcpyAsync(p->lut.p, lut.data(), lut.size(), hipMemcpyHostToDevice, p->ctx->stream));
            HIP_CHECK(hipStreamSynchronize(p->ctx->stream));
        } else if (kind == FD_LAYER_LBP) {
            if (lbp_type < 0 || lbp_type > 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "LbpFilter: invalid type");
        } else if (kind == FD_LAYER_GRADMAG_LBP) {   // bins, signed_gradients and interpolate are not used
            if (grad_kernel != 1 && grad_kernel != 3 && grad_kernel != 5 && grad_kernel != 7 && grad_kernel != FD_GRAD_SCHARR)
                FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientFilter: the kernel size must be 1, 3, 5, 7 or CV_SCHARR");
            if (lbp_type < 0 || lbp_type > 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "LbpFilter: invalid type");
        } else if (kind != FD_LAYER_NONE) {
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_set_layer_filter: unknown kind %d", kind);
        }
        p->filter_kind = kind;
        p->bins = bins;
        p->signed_gradients = signed_gradients;
        p->interpolate = interpolate;
        p->grad_kernel = grad_kernel;
        p->lbp_type = lbp_type;
        invalidate_layout(p);
    });
}

int fd_pyramid_set_image_filter(fd_pyramid* p, int kind) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_set_image_filter: NULL pyramid");
        if (kind != FD_IMAGE_GRAY && kind != FD_IMAGE_GREYWORLD_GRAY)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_set_image_filter: unknown kind %d", kind);
        if (kind == FD_IMAGE_GREYWORLD_GRAY) {   // allocated here: an update allocates nothing
            HIP_CHECK(hipSetDevice(p->ctx->device));
            p->gw_stats.reserve(sizeof(GwStats) * FD_MAX_FRAMES);
        }
        p->image_filter = kind;   // the layout does not depend on it
    });
}

int fd_pyramid_image_filter(const fd_pyramid* p) { return p ? p->image_filter : FD_IMAGE_GRAY; }

int fd_pyramid_update(fd_pyramid* p, const uint8_t* image, int w, int h, int ch, int is_device) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update: NULL pyramid");
        HIP_CHECK(hipSetDevice(p->ctx->device));
        pyramid_update(p, image, w, h, ch, is_device, p->ctx->stream);
    });
}

int fd_pyramid_set_frames(fd_pyramid* p, int frames) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_set_frames: NULL pyramid");
        if (frames < 1 || frames > FD_MAX_FRAMES) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_set_frames: 1..%d frames", FD_MAX_FRAMES);
        if (frames > 1 && p->filter_kind != FD_LAYER_NONE) FD_THROW(FD_ERR_INVALID_ARGUMENT, "multi-frame pyramids have no layer filters");
        if (frames != p->nimg) { p->nimg = frames; invalidate_layout(p); }
    });
}

int fd_pyramid_update_frames(fd_pyramid* p, const uint8_t* const* images, int n, int w, int h, int ch, int is_device) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p || !images) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update_frames: NULL argument");
        if (n != p->nimg) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update_frames: %d images for a pyramid of %d frames", n, p->nimg);
        for (int f = 0; f < n; ++f)
            if (!images[f]) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_update_frames: image %d is NULL", f);
        HIP_CHECK(hipSetDevice(p->ctx->device));
        pyramid_update(p, nullptr, w, h, ch, is_device, p->ctx->stream, images);
    });
}

int fd_pyramid_select(fd_pyramid* p, int first_layer, int last_layer, int step_layer, const int* roi) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_select: NULL pyramid");
        if (step_layer < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "DirectPyramidFeatureExtractor: stepLayer has to be greater than zero");
        p->sel_first = first_layer < 0 ? -1 : first_layer;
        p->sel_last = last_layer < 0 ? -1 : last_layer;
        p->sel_step = step_layer;
        p->sel_has_roi = roi != nullptr;
        if (roi) std::memcpy(p->sel_roi, roi, sizeof(p->sel_roi));
    });
}

int fd_pyramid_set_gradient_blur(fd_pyramid* p, int blur_kernel) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_set_gradient_blur: NULL pyramid");
        if (blur_kernel < 0 || blur_kernel > 31) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientFilter: the blur kernel size must be in 0..31");
        if (blur_kernel != p->grad_blur) {
            p->grad_blur = blur_kernel;
            invalidate_layout(p);
        }
    });
}

int fd_pyramid_select_view(fd_pyramid* p, int first_layer, int last_layer) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_select_view: NULL pyramid");
        p->view_first = first_layer < 0 ? -1 : first_layer;
        p->view_last = last_layer < 0 ? -1 : last_layer;
    });
}

int fd_pyramid_octave_layer_count(const fd_pyramid* p) { return p ? (int)p->octl : 0; }
double fd_pyramid_incremental_scale(const fd_pyramid* p) { return p ? p->inc : 0.0; }
int fd_pyramid_layer_count(const fd_pyramid* p) { return p ? (int)p->kept.size() : 0; }

int fd_pyramid_layer_info(const fd_pyramid* p, int i, int* index, double* scale, int* w, int* h, int* ch) {
    if (!p || i < 0 || i >= (int)p->kept.size()) return FD_ERR_INVALID_ARGUMENT;
    const HostLayer& L = p->all[p->kept[i]];
    if (index) *index = L.index;
    if (scale) *scale = L.scale;
    if (w) *w = L.w;
    if (h) *h = L.h;
    if (ch) *ch = L.ch;
    return FD_OK;
}

int fd_pyramid_layer_download(fd_pyramid* p, int i, uint8_t* host_dst) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p || !host_dst || i < 0 || i >= (int)p->kept.size()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_layer_download: bad argument");
        if (p->nimg > 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_layer_download: the pyramid holds %d frames; use fd_pyramid_frame_layer_download", p->nimg);
        const HostLayer& L = p->all[p->kept[i]];
        HIP_CHECK(hipMemcpyAsync(host_dst, p->arena.as<uint8_t>() + L.filt_off, (size_t)L.w * L.h * L.ch, hipMemcpyDeviceToHost, p->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(p->ctx->stream));
    });
}

int fd_pyramid_frame_layer_download(fd_pyramid* p, int frame, int i, uint8_t* host_dst) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p || !host_dst || i < 0 || i >= (int)p->kept.size() || frame < 0 || frame >= p->nimg)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_frame_layer_download: bad argument");
        const HostLayer& L = p->all[p->kept[i]];
        HIP_CHECK(hipMemcpyAsync(host_dst, p->arena.as<uint8_t>() + (size_t)frame * p->image_stride + L.filt_off, (size_t)L.w * L.h * L.ch,
                                 hipMemcpyDeviceToHost, p->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(p->ctx->stream));
    });
}

int fd_pyramid_window_count(const fd_pyramid* p, int pw, int ph, int sx, int sy, const int* roi, int64_t* count) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p || !count) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_window_count: NULL argument");
        std::vector<WindowLayer> wl;
        fd_enumerate_layers(p, pw, ph, sx, sy, roi, wl, *count);
    });
}

int fd_pyramid_windows(const fd_pyramid* p, int pw, int ph, int sx, int sy, const int* roi, int32_t* out, int64_t cap,
                       int64_t* count) {
    return fd_guard(p ? p->ctx : nullptr, [&] {
        if (!p || !count) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_pyramid_windows: NULL argument");
        std::vector<WindowLayer> wl;
        int64_t total;
        fd_enumerate_layers(p, pw, ph, sx, sy, roi, wl, total);
        *count = total;
        if (!out) return;
        int64_t n = 0;
        for (const WindowLayer& w : wl) {
            const HostLayer& L = p->all[p->kept[w.layer]];
            for (int iy = 0; iy < w.ny; ++iy)
                for (int ix = 0; ix < w.nx; ++ix, ++n) {
                    if (n >= cap) continue;
                    int x = w.bx + ix * sx, y = w.by + iy * sy;
                    int32_t* o = out + 7 * n;
                    o[0] = w.layer; o[1] = x; o[2] = y;
                    o[3] = fd_cvRound(x / L.scale) + w.ow / 2;
                    o[4] = fd_cvRound(y / L.scale) + w.oh / 2;
                    o[5] = w.ow; o[6] = w.oh;
                }
        }
        if (total > cap) FD_THROW(FD_ERR_CAPACITY, "fd_pyramid_windows: %lld windows, capacity %lld", (long long)total, (long long)cap);
    });
}

int fd_greyworld(fd_ctx* ctx, const uint8_t* bgr, int w, int h, uint8_t* dst, int is_device) {
    return fd_guard(ctx, [&] {
        if (!ctx || !bgr || !dst || w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_greyworld: bad argument");
        HIP_CHECK(hipSetDevice(ctx->device));
        const int n = w * h;
        DevBuf in, out, stats;
        const uint8_t* din = bgr;
        uint8_t* dout = dst;
        if (!is_device) {
            in.reserve((size_t)n * 3);
            out.reserve((size_t)n * 3);
            HIP_CHECK(hipMemcpyAsync(in.p, bgr, (size_t)n * 3, hipMemcpyHostToDevice, ctx->stream));
            din = in.as<uint8_t>();
            dout = out.as<uint8_t>();
        }
        stats.reserve(64);
        HIP_CHECK(hipMemsetAsync(stats.p, 0, 64, ctx->stream));
        unsigned long long* sums = stats.as<unsigned long long>();
        unsigned int* maxs = (unsigned int*)(sums + 3);
        hipLaunchKernelGGL(k_greyworld_stats, dim3(grid_for(n)), dim3(256), 0, ctx->stream, din, n, sums, maxs);
        HIP_CHECK(hipGetLastError());
        unsigned long long hs[5] = {0, 0, 0, 0, 0};
        HIP_CHECK(hipMemcpyAsync(hs, stats.p, 40, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        unsigned int hm[3];
        std::memcpy(hm, (char*)hs + 24, 12);
        // scalar part exactly as GreyWorldNormalizationFilter.cpp:45-60 (double, host)
        double mean[3], maxNew[3], scale[3];
        for (int c = 0; c < 3; ++c) { mean[c] = (double)hs[c] / n; maxNew[c] = (uint8_t)hm[c] / mean[c]; }
        double mx = maxNew[0];
        if (maxNew[1] > mx) mx = maxNew[1];
        if (maxNew[2] > mx) mx = maxNew[2];
        for (int c = 0; c < 3; ++c) scale[c] = 255.0 / (mean[c] * mx);
        hipLaunchKernelGGL(k_greyworld_apply, dim3(grid_for(n)), dim3(256), 0, ctx->stream, din, dout, n, scale[0], scale[1], scale[2]);
        HIP_CHECK(hipGetLastError());
        if (!is_device) HIP_CHECK(hipMemcpyAsync(dst, dout, (size_t)n * 3, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

// ---- stand-alone ImageFilter::applyTo(Mat) forms of the layer filters (ImageFilter.hpp:18-57) on one host image ----------
int fd_gradient_filter_image(fd_ctx* ctx, const uint8_t* gray, int w, int h, int grad_kernel, int blur_kernel, uint8_t* dst2ch) {
    return fd_guard(ctx, [&] {
        if (!ctx || !gray || !dst2ch || w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_gradient_filter_image: bad argument");
        if (grad_kernel != 1 && grad_kernel != 3 && grad_kernel != 5 && grad_kernel != 7 && grad_kernel != FD_GRAD_SCHARR)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientFilter: the kernel size must be 1, 3, 5, 7 or CV_SCHARR");
        if (blur_kernel < 0 || blur_kernel > 31) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientFilter: the blur kernel size must be in 0..31");
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = (size_t)w * h, boff = (n + 255) & ~(size_t)255;
        DevBuf in, out;   // in: [gray | blurred]: k_box_blur addresses both through one base pointer
        in.reserve(boff + n);
        out.reserve(2 * n);
        HIP_CHECK(hipMemcpyAsync(in.p, gray, n, hipMemcpyHostToDevice, ctx->stream));
        const uint8_t* src = in.as<uint8_t>();
        if (blur_kernel > 0) {
            FilterJobs jobs;
            jobs.n = 1;
            jobs.j[0].w = w; jobs.j[0].h = h; jobs.j[0].src_off = 0; jobs.j[0].dst_off = (uint32_t)boff;
            hipLaunchKernelGGL(k_box_blur, dim3(grid_for((int)n), 1), dim3(256), 0, ctx->stream, in.as<uint8_t>(), blur_kernel, jobs);
            src += boff;
        }
        hipLaunchKernelGGL(k_gradient_image, dim3(grid_for((int)n)), dim3(256), 0, ctx->stream, src, out.as<uint8_t>(), w, h, grad_kernel);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(dst2ch, out.p, 2 * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}
int fd_gradient_image(fd_ctx* ctx, const uint8_t* gray, int w, int h, int grad_kernel, uint8_t* dst2ch) {
    return fd_gradient_filter_image(ctx, gray, w, h, grad_kernel, 0, dst2ch);
}

int fd_gradient_binning_image(fd_ctx* ctx, const uint8_t* grad2ch, int w, int h, int bins, int signed_gradients, int interpolate, uint8_t* dst) {
    return fd_guard(ctx, [&] {
        if (!ctx || !grad2ch || !dst || w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_gradient_binning_image: bad argument");
        if (bins < 1 || bins > 255) FD_THROW(FD_ERR_INVALID_ARGUMENT, "GradientBinningFilter: bins must be in 1..255");
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = (size_t)w * h;
        const int E = interpolate ? 4 : 2;
        std::vector<uint8_t> lut;
        build_gradient_lut(bins, signed_gradients != 0, interpolate != 0, lut);
        DevBuf in, out, dl;
        in.reserve(2 * n);
        out.reserve((size_t)E * n);
        dl.reserve(lut.size());
        HIP_CHECK(hipMemcpyAsync(dl.p, lut.data(), lut.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(in.p, grad2ch, 2 * n, hipMemcpyHostToDevice, ctx->stream));
        if (E == 2) hipLaunchKernelGGL(k_binning_image<2>, dim3(grid_for((int)n)), dim3(256), 0, ctx->stream, in.as<uint8_t>(), dl.as<uint8_t>(), out.as<uint8_t>(), (int)n);
        else hipLaunchKernelGGL(k_binning_image<4>, dim3(grid_for((int)n)), dim3(256), 0, ctx->stream, in.as<uint8_t>(), dl.as<uint8_t>(), out.as<uint8_t>(), (int)n);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(dst, out.p, (size_t)E * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_gradient_magnitude_image(fd_ctx* ctx, const uint8_t* grad2ch, int w, int h, uint8_t* dst) {
    return fd_guard(ctx, [&] {
        if (!ctx || !grad2ch || !dst || w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_gradient_magnitude_image: bad argument");
        if ((size_t)w * h > 0x3fffffffull) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_gradient_magnitude_image: image too large");
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = (size_t)w * h;
        DevBuf in, out;
        in.reserve(2 * n);
        out.reserve(n);
        HIP_CHECK(hipMemcpyAsync(in.p, grad2ch, 2 * n, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_gradient_magnitude_image, dim3(grid_for((int)n)), dim3(256), 0, ctx->stream, in.as<uint8_t>(), out.as<uint8_t>(), (int)n);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(dst, out.p, n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_lbp_image(fd_ctx* ctx, const uint8_t* gray, int w, int h, int lbp_type, uint8_t* dst) {
    return fd_guard(ctx, [&] {
        if (!ctx || !gray || !dst || w < 1 || h < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_lbp_image: bad argument");
        if (lbp_type < 0 || lbp_type > 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "LbpFilter: invalid type");
        HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n = (size_t)w * h, doff = (n + 255) & ~(size_t)255;
        DevBuf buf;   // [gray | codes]: k_lbp addresses both through one base pointer
        buf.reserve(doff + n);
        HIP_CHECK(hipMemcpyAsync(buf.p, gray, n, hipMemcpyHostToDevice, ctx->stream));
        FilterJobs jobs;
        jobs.n = 1;
        jobs.j[0].w = w; jobs.j[0].h = h; jobs.j[0].src_off = 0; jobs.j[0].dst_off = (uint32_t)doff;
        hipLaunchKernelGGL(k_lbp, dim3(grid_for((int)n), 1), dim3(256), 0, ctx->stream, buf.as<uint8_t>(), lbp_type, jobs);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(dst, buf.as<uint8_t>() + doff, n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

// Test hook (include/fd_hip_bench.h; needs no GPU): tile `tile` of the pyrDown of a sw x sh image as k_pyrdown_tiled stages it, by
// the kernel's own entry builder and staging function, lane by lane
int fd_debug_pyrdown_stage(const uint8_t* image, int sw, int sh, int tile, uint8_t* staged, int32_t* entry) {
    if (sw < 1 || sh < 1 || (int64_t)sw * sh > 0x7fffffff) return -1;
    const int nt = pd_tiles(sw, sh);
    if (!image && !staged && !entry) return nt;
    if (!image || tile < 0 || tile >= nt) return -1;
    const PdTile e = pd_tile_entry(sw, sh, 0, 0, tile);
    if (entry) std::memcpy(entry, &e, sizeof(e));
    if (staged) {
        for (int rq = 0; rq < 4; ++rq)
            for (int lane = 0; lane < 64; ++lane) {
                uint32_t v[PD_LD];
                pd_stage(image, e, rq, lane, v);
                for (int k = 0; k < PD_LD; ++k) {
                    const int r = 2 * (rq + 4 * k) + (lane >> 5);
                    if (r < 2 * PD_TH + 3) std::memcpy(staged + r * 128 + 4 * (lane & 31), &v[k], 4);
                }
            }
    }
    return nt;
}

// Test hook (include/fd_hip_bench.h; needs no GPU): tile `tile` of the fused resize + pyrDown of a sw x sh image to a dw0 x dh0
// first-octave layer as k_resize_down stages it, by the plan's own column table and tile columns and the kernel's own row, fetch,
// interleave and addressing functions, wavefront by wavefront and lane by lane
int fd_debug_resize_stage(const uint8_t* image, int sw, int sh, int dw0, int dh0, int tile, uint8_t* staged, int32_t* read_off, int32_t* entry) {
    if (sw < 1 || sh < 1 || sw > 65535 || sh > 65535 || dw0 < 3 || dh0 < 3 || dw0 > sw || dh0 > sh) return -1;
    const double scale_x = 1. / ((double)dw0 / sw), scale_y = 1. / ((double)dh0 / sh);
    if (!(scale_x >= 1.0 && scale_x <= 2.05 && scale_y >= 1.0 && scale_y <= 2.05)) return -1;
    const int dw1 = (dw0 + 1) / 2, dh1 = (dh0 + 1) / 2;
    const int tilesX = (dw1 + FT_W1 - 1) / FT_W1, nt = tilesX * ((dh1 + FT_H1 - 1) / FT_H1);
    const std::vector<int2> xt = fused_xtab(dw0, sw, scale_x);
    if (!fused_fits(xt, sw, dw1)) return -1;
    if (!image && !staged && !read_off && !entry) return nt;
    if (tile < 0 || tile >= nt) return -1;
    const int ty = tile / tilesX, tx = tile - ty * tilesX;
    const int2 cols = fused_tile_cols(xt, sw, tx);
    const int X0 = cols.x, ncol = cols.y, gx0 = 2 * tx * FT_W1 - 2, gy0 = 2 * ty * FT_H1 - 2;
    if (entry) {
        const int32_t e[8] = {X0, ncol, tx, ty, gx0, gy0, dw1, dh1};
        std::memcpy(entry, e, sizeof(e));
    }
    if (staged) {
        if (!image) return -1;
        const size_t n = (size_t)sw * sh;
        auto dword_at = [&](uint32_t off) {   // the kernel's unaligned dword load; what hangs over the image's end reads as 0 here
            uint32_t w = 0;
            for (uint32_t b = 0; b < 4; ++b)
                if ((size_t)off + b < n) w |= (uint32_t)image[off + b] << (8 * b);
            return w;
        };
        std::memset(staged, 0, (size_t)FS_SLOTS * FS_SLOT);
        for (int wave = 0; wave < 4; ++wave)
            for (int q = 0; q < FS_ROWS; ++q) {
                const FusedRow r = fused_row(FS_ROWS * wave + q, gy0, dh0, scale_y, sh);   // lane q of the wavefront works the row out
                for (int lane = 0; lane < 64; ++lane) {
                    const uint32_t voff = fs_fetch_col(lane, X0, ncol);
                    const uint2 pr = fs_pair(dword_at((uint32_t)r.y0 * (uint32_t)sw + voff), dword_at((uint32_t)r.y1 * (uint32_t)sw + voff));
                    std::memcpy(staged + fs_store_off(FS_ROWS * wave + q, lane), &pr, 8);
                }
            }
    }
    if (read_off) {   // thread = column c of the tile, rows 0 .. 34 (two halves in the kernel, at the same offsets)
        for (int r = 0; r < G0_H; ++r)
            for (int c = 0; c < G0_W; ++c) {
                int gx = gx0 + c;   // the kernel's reflect101
                if (dw0 == 1) gx = 0;
                else while (gx < 0 || gx >= dw0) gx = gx < 0 ? -gx : 2 * dw0 - 2 - gx;
                read_off[r * G0_W + c] = fs_read_off(xt[(size_t)gx].x, X0, r);
            }
    }
    return nt;
}

}  // extern "C"

#ifdef FD_PYR_PROF
extern "C" int fd_debug_pyr_prof(unsigned long long* out) {   // the records of the last k_resize_down launch; returns the capacity
    if (out) (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(fd_pyr_prof), sizeof(unsigned long long) * 8 * PYR_PROF_WGS);
    return PYR_PROF_WGS;
}
#endif
