// featuredetection_amd/csrc/optflow.hip -- pyramidal Lucas-Kanade optical flow for condensation::OpticalFlowTransitionModel
// (OpticalFlowTransitionModel.cpp:86-111): cv::buildOpticalFlowPyramid with derivatives and replicated borders, and
// cv::calcOpticalFlowPyrLK with OpenCV's default criteria.  Their arithmetic is not in the reference tree; DESIGN.md 4.14 writes it
// down and is this file's specification.  The template grid and the median flow (host only) are in hostalgo.cpp.
//
// Kernels: k_flow_level0 (gray conversion + border of level 0), k_flow_pyrdown_pad (cv::pyrDown of a level + border),
// k_flow_scharr_pad (Scharr derivatives of a level + border) -- one thread per stored pixel, border pixels compute the value of the
// edge pixel they replicate, so a level is written once and no second pass touches it; k_lk_track -- one wavefront per point, all
// levels and iterations inside, the five window sums exact in int64; k_flow_motion -- one workgroup, the median flow of a resident
// track (fd_flow_median restated by radix selection).  All loops are counted; nothing waits on another workgroup.
#include "fd_internal.hpp"
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <memory>

namespace {

constexpr int FLOW_WIN_PIXELS = FD_FLOW_MAX_WINDOW * FD_FLOW_MAX_WINDOW;
constexpr int FLOW_W_BITS = 14;

struct FlowLevel {          // one level of a frame, device-visible; offsets from the frame's slot
    int32_t w, h;           // the level without its border
    int32_t pw, ph;         // with it: w + 2 win_w, h + 2 win_h
    uint32_t img_off;       // u8 [ph][pw]
    uint32_t der_off;       // int16 [ph][pw][2] {dx, dy}
};

__host__ __device__ inline int flow_reflect101(int p, int len) {
    if (len == 1) return 0;
    for (int it = 0; it < 4 && (p < 0 || p >= len); ++it) p = p < 0 ? -p : 2 * len - 2 - p;   // the taps reach two pixels out: one reflection for len >= 3
    return p < 0 ? 0 : (p >= len ? len - 1 : p);
}

__device__ inline int flow_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// level 0 with its border: the gray image (cv::cvtColor(BGR2GRAY) 8U as pyramid.hip converts: (B 1868 + G 9617 + R 4899 + 8192) >> 14)
__global__ __launch_bounds__(256) void k_flow_level0(const uint8_t* __restrict__ src, int channels, int stride, uint8_t* __restrict__ dst, int w, int h,
                                                     int winW, int winH) {
    const int pw = w + 2 * winW, ph = h + 2 * winH;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pw * ph) return;
    const int Y = i / pw, X = i - Y * pw;
    const int x = flow_clamp(X - winW, w - 1), y = flow_clamp(Y - winH, h - 1);
    const uint8_t* s = src + (size_t)y * stride + (size_t)x * channels;
    dst[i] = channels == 1 ? s[0] : (uint8_t)((s[0] * 1868 + s[1] * 9617 + s[2] * 4899 + 8192) >> 14);
}

// cv::pyrDown 8UC1 of the level inside `src` (sw x sh at (winW, winH), row pitch spw): [1 4 6 4 1] x [1 4 6 4 1], (sum + 128) >> 8,
// BORDER_REFLECT_101 inside the level; the border of the result replicates its edge
__global__ __launch_bounds__(256) void k_flow_pyrdown_pad(const uint8_t* __restrict__ src, int spw, int sw, int sh, uint8_t* __restrict__ dst, int dw, int dh,
                                                          int winW, int winH) {
    const int pw = dw + 2 * winW, ph = dh + 2 * winH;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pw * ph) return;
    const int Y = i / pw, X = i - Y * pw;
    const int x = flow_clamp(X - winW, dw - 1), y = flow_clamp(Y - winH, dh - 1);
    const uint8_t* level = src + (size_t)winH * spw + winW;
    int cx[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) cx[t] = flow_reflect101(2 * x - 2 + t, sw);
    int sum = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* row = level + (size_t)flow_reflect101(2 * y - 2 + j, sh) * spw;
        const int r = row[cx[0]] + 4 * row[cx[1]] + 6 * row[cx[2]] + 4 * row[cx[3]] + row[cx[4]];
        sum += (j == 0 || j == 4) ? r : ((j == 2) ? 6 * r : 4 * r);
    }
    dst[i] = (uint8_t)((sum + 128) >> 8);
}

// calcSharrDeriv of the level inside `img` (w x h at (winW, winH), row pitch pw) into the level's derivative image of the same
// pitch: BORDER_REFLECT_101 inside the level, no scaling; the border replicates the derivative's own edge values
__global__ __launch_bounds__(256) void k_flow_scharr_pad(const uint8_t* __restrict__ img, int16_t* __restrict__ der, int w, int h, int winW, int winH) {
    const int pw = w + 2 * winW, ph = h + 2 * winH;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pw * ph) return;
    const int Y = i / pw, X = i - Y * pw;
    const int x = flow_clamp(X - winW, w - 1), y = flow_clamp(Y - winH, h - 1);
    const uint8_t* level = img + (size_t)winH * pw + winW;
    const uint8_t* r0 = level + (size_t)flow_reflect101(y - 1, h) * pw;
    const uint8_t* r1 = level + (size_t)y * pw;
    const uint8_t* r2 = level + (size_t)flow_reflect101(y + 1, h) * pw;
    const int xs[3] = {flow_reflect101(x - 1, w), x, flow_reflect101(x + 1, w)};
    int t0[3], t1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t0[c] = 3 * (r0[xs[c]] + r2[xs[c]]) + 10 * r1[xs[c]];
        t1[c] = r2[xs[c]] - r0[xs[c]];
    }
    der[2 * (size_t)i] = (int16_t)(t0[2] - t0[0]);
    der[2 * (size_t)i + 1] = (int16_t)(3 * (t1[0] + t1[2]) + 10 * t1[1]);
}

// the sum of v over the 64 lanes, in every lane: integer additions, so the value does not depend on the order
__device__ inline long long flow_wave_sum(long long v) {
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) {
        const int lo = __shfl_xor((int)(unsigned int)((unsigned long long)v & 0xffffffffull), offset);
        const int hi = __shfl_xor((int)(v >> 32), offset);
        v += (long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo);
    }
    return v;
}

struct FlowWeights { int w00, w01, w10, w11; };
// the bilinear weights of a window whose corner lies (a, b) behind a pixel: cvRound (half to even) of float products
__device__ inline FlowWeights flow_weights(float a, float b) {
    FlowWeights q;
    const float na = 1.f - a, nb = 1.f - b;
    q.w00 = __float2int_rn((na * nb) * 16384.f);
    q.w01 = __float2int_rn((a * nb) * 16384.f);
    q.w10 = __float2int_rn((na * b) * 16384.f);
    q.w11 = (1 << FLOW_W_BITS) - q.w00 - q.w01 - q.w10;
    return q;
}

// the window's corner in float, and whether a window there stays inside the level and its border (a NaN does not)
__device__ inline bool flow_inside(float fx, float fy, int winW, int winH, int w, int h) {
    return fx >= (float)-winW && fx < (float)w && fy >= (float)-winH && fy < (float)h;
}

// calcOpticalFlowPyrLK for one point per wavefront.  `from` holds the frame the points lie in, `to` the frame they
// are looked for in.  The window's pixels are dealt to the lanes (pixel i to lane i % 64); I, Ix, Iy of the window stay in LDS as int16
// for the iterations of the level, every lane reading only what it wrote.  After flow_wave_sum every lane holds the same integers
// and runs the same float32 operations on them: the control flow is uniform over the wavefront.
__global__ __launch_bounds__(64) void k_lk_track(const uint8_t* __restrict__ from, const uint8_t* __restrict__ to, const FlowLevel* __restrict__ levels,
                                                 int nLevels, int winW, int winH, int maxCount, float eps2, float minEigThreshold,
                                                 const float* __restrict__ pts, int n, float* __restrict__ out, uint8_t* __restrict__ status,
                                                 uint8_t* __restrict__ trace) {
    __shared__ int16_t sI[FLOW_WIN_PIXELS], sIx[FLOW_WIN_PIXELS], sIy[FLOW_WIN_PIXELS];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= n) return;
    const int npix = winW * winH;
    const float FLT_SCALE = 1.f / (float)(1 << 20);
    const float ptX = pts[2 * p], ptY = pts[2 * p + 1];
    const float halfX = (float)(winW - 1) * 0.5f, halfY = (float)(winH - 1) * 0.5f;
    const float eigDen = (float)(2 * winW * winH);
    float resX = 0.f, resY = 0.f;
    int ok = 1;
    if (trace && lane >= 2 * nLevels && lane < 2 * FD_FLOW_MAX_LEVELS) trace[(size_t)p * 2 * FD_FLOW_MAX_LEVELS + lane] = 0;
    for (int level = nLevels - 1; level >= 0; --level) {
        const FlowLevel L = levels[level];
        const float scale = (float)(1.0 / (double)(1 << level));
        float prevX = ptX * scale, prevY = ptY * scale;
        if (level == nLevels - 1) { resX = prevX; resY = prevY; }
        else { resX = 2.f * resX; resY = 2.f * resY; }
        int steps = 0, reason = FD_FLOW_EXIT_COUNT;
        prevX = prevX - halfX;
        prevY = prevY - halfY;
        const float fpx = floorf(prevX), fpy = floorf(prevY);
        if (!flow_inside(fpx, fpy, winW, winH, L.w, L.h)) {
            reason = FD_FLOW_EXIT_SKIP_RANGE;
            if (level == 0) ok = 0;
        } else {
            const int ipx = (int)fpx + winW, ipy = (int)fpy + winH;   // in the stored level: 0 <= ipx, ipx + winW <= pw - 1
            const FlowWeights q = flow_weights(prevX - fpx, prevY - fpy);
            const uint8_t* img = from + L.img_off;
            const int16_t* der = (const int16_t*)(from + L.der_off);
            long long a11 = 0, a12 = 0, a22 = 0;
            for (int i = lane; i < npix; i += 64) {
                const int y = i / winW, x = i - y * winW;
                const size_t at = (size_t)(ipy + y) * L.pw + (ipx + x);
                const uint8_t* s = img + at;
                const int16_t* d = der + 2 * at;
                const int I = (s[0] * q.w00 + s[1] * q.w01 + s[L.pw] * q.w10 + s[L.pw + 1] * q.w11 + (1 << 8)) >> 9;
                const int ix = (d[0] * q.w00 + d[2] * q.w01 + d[2 * L.pw] * q.w10 + d[2 * L.pw + 2] * q.w11 + (1 << 13)) >> 14;
                const int iy = (d[1] * q.w00 + d[3] * q.w01 + d[2 * L.pw + 1] * q.w10 + d[2 * L.pw + 3] * q.w11 + (1 << 13)) >> 14;
                sI[i] = (int16_t)I; sIx[i] = (int16_t)ix; sIy[i] = (int16_t)iy;
                a11 += (long long)(ix * ix); a12 += (long long)(ix * iy); a22 += (long long)(iy * iy);
            }
            const float A11 = (float)flow_wave_sum(a11) * FLT_SCALE, A12 = (float)flow_wave_sum(a12) * FLT_SCALE, A22 = (float)flow_wave_sum(a22) * FLT_SCALE;
            float D = A11 * A22 - A12 * A12;
            const float diffA = A11 - A22;
            const float minEig = ((A22 + A11) - sqrtf(diffA * diffA + (4.f * A12) * A12)) / eigDen;
            if (minEig < minEigThreshold || D < FLT_EPSILON) {
                reason = FD_FLOW_EXIT_SKIP_EIGEN;
                if (level == 0) ok = 0;
            } else {
                D = 1.f / D;
                float nextX = resX - halfX, nextY = resY - halfY;
                float prevDX = 0.f, prevDY = 0.f;
                const uint8_t* J = to + L.img_off;
                for (int j = 0; j < maxCount; ++j) {
                    const float fnx = floorf(nextX), fny = floorf(nextY);
                    if (!flow_inside(fnx, fny, winW, winH, L.w, L.h)) {
                        reason = FD_FLOW_EXIT_LEFT_RANGE;
                        if (level == 0) ok = 0;
                        break;
                    }
                    const int inx = (int)fnx + winW, iny = (int)fny + winH;
                    const FlowWeights r = flow_weights(nextX - fnx, nextY - fny);
                    long long b1 = 0, b2 = 0;
                    for (int i = lane; i < npix; i += 64) {
                        const int y = i / winW, x = i - y * winW;
                        const uint8_t* s = J + (size_t)(iny + y) * L.pw + (inx + x);
                        const int diff = ((s[0] * r.w00 + s[1] * r.w01 + s[L.pw] * r.w10 + s[L.pw + 1] * r.w11 + (1 << 8)) >> 9) - sI[i];
                        b1 += (long long)(diff * sIx[i]);
                        b2 += (long long)(diff * sIy[i]);
                    }
                    const float B1 = (float)flow_wave_sum(b1) * FLT_SCALE, B2 = (float)flow_wave_sum(b2) * FLT_SCALE;
                    const float dX = (A12 * B2 - A22 * B1) * D, dY = (A12 * B1 - A11 * B2) * D;
                    nextX = nextX + dX;
                    nextY = nextY + dY;
                    resX = nextX + halfX;
                    resY = nextY + halfY;
                    ++steps;
                    if (dX * dX + dY * dY <= eps2) { reason = FD_FLOW_EXIT_EPS; break; }
                    if (j > 0 && fabsf(dX + prevDX) < 0.01f && fabsf(dY + prevDY) < 0.01f) {
                        resX = resX - dX * 0.5f;
                        resY = resY - dY * 0.5f;
                        reason = FD_FLOW_EXIT_OSCILLATION;
                        break;
                    }
                    prevDX = dX;
                    prevDY = dY;
                }
            }
        }
        if (trace && lane == 0) {
            trace[((size_t)p * FD_FLOW_MAX_LEVELS + level) * 2] = (uint8_t)steps;
            trace[((size_t)p * FD_FLOW_MAX_LEVELS + level) * 2 + 1] = (uint8_t)reason;
        }
    }
    if (lane == 0) {
        out[2 * p] = resX;
        out[2 * p + 1] = resY;
        status[p] = (uint8_t)ok;
    }
}

// ---- the median flow of n tracked points on the device: fd_flow_median (hostalgo.cpp) restated, DESIGN.md 4.7 ----
constexpr int MT = FD_FLOW_RESIDENT_MAX_POINTS;   // threads of k_flow_motion: one per point

// an unsigned key in the host's nanLast order: a < b as floats <=> key(a) < key(b); every NaN has the largest key
__device__ inline uint32_t flow_key(float v) {
    if (v != v) return 0xffffffffu;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float flow_unkey(uint32_t k) {
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// one more key in its bin.  The lanes that share the bin of the first taking lane go in as one addition (the ratios of a rigid motion
// crowd into one bin); integer additions, so the histogram does not depend on who adds first.
__device__ inline void flow_hist_add(unsigned int* hist, unsigned int bin, bool take) {
    const unsigned long long takers = __ballot(take);
    if (!takers) return;
    const int leader = __ffsll((long long)takers) - 1;
    const unsigned int leaderBin = (unsigned int)__shfl((int)bin, leader);
    const unsigned long long same = __ballot(take && bin == leaderBin);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[leaderBin], (unsigned int)__popcll(same));
    else if (take && bin != leaderBin) atomicAdd(&hist[bin], 1u);
}

// The k-th smallest (from 0) of the keys `each` emits, by radix selection: four passes of eight bits from the top; a pass counts the
// keys that agree with the digits chosen so far by their next digit, and the first wavefront walks the 256 counts to the digit that
// holds rank k.  `each` emits the same multiset of keys in every pass; every thread of the workgroup calls this.
template <class Each>
__device__ uint32_t flow_select(unsigned int* hist, unsigned int* chosen, unsigned int k, Each each) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t above = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        each([&](uint32_t key, bool take) { flow_hist_add(hist, (key >> shift) & 255u, take && (key & above) == prefix); });
        __syncthreads();
        if (tid < 64) {   // lane l: bins 4 l .. 4 l + 3
            const unsigned int c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
            const unsigned int mine = c0 + c1 + c2 + c3;
            unsigned int incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int t = (unsigned int)__shfl_up((int)incl, o, 64);
                if (tid >= o) incl += t;
            }
            const unsigned int before = incl - mine;
            if (before <= k && k < incl) {   // one lane: the counts add up to more than k
                unsigned int r = k - before, bin = 4 * tid;
                if (r >= c0) { r -= c0; ++bin; if (r >= c1) { r -= c1; ++bin; if (r >= c2) { r -= c2; ++bin; } } }
                chosen[0] = bin;
                chosen[1] = r;
            }
        }
        __syncthreads();
        prefix |= chosen[0] << shift;
        k = chosen[1];
    }
    return prefix;
}

// OpticalFlowTransitionModel.cpp:114-170 as fd_flow_median has it, one workgroup, thread i owns point i.  A pair is correct when both
// status bytes are set and its squared forward-backward distance d is a number not above 0.5f: that is the set fd_flow_median's sort
// puts in front, and only its members matter, not their order (each median is an order statistic of a multiset; the ratio of a pair
// is symmetric in its two points because (-v) * (-v) == v * v).  The correct points are compacted in index order.  The medians of
// x and y are the keys of rank n_correct / 2; the ratio median is the key of rank pairs / 2 over all pairs, every ratio recomputed
// in each pass (thread j: the pairs (i, j), i < j).  All loops are counted; nothing waits on another workgroup.
__global__ __launch_bounds__(MT) void k_flow_motion(const float2* __restrict__ pts, const float2* __restrict__ fwd, const float2* __restrict__ bwd,
                                                    const uint8_t* __restrict__ fstatus, const uint8_t* __restrict__ bstatus, int n,
                                                    fd_flow_motion_info* __restrict__ out) {
    __shared__ float2 sP[MT], sF[MT];
    __shared__ unsigned int hist[256], chosen[2], waveValid[MT / 64], waveCorrect[MT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool valid = false, correct = false;
    float2 P = make_float2(0.f, 0.f), F = P;
    if (tid < n) {
        P = pts[tid];
        F = fwd[tid];
        if (fstatus[tid] && bstatus[tid]) {
            const float2 B = bwd[tid];
            const float dx = B.x - P.x, dy = B.y - P.y;
            const float d = dx * dx + dy * dy;
            valid = d == d;
            correct = valid && !(d > 0.5f);
        }
    }
    const unsigned long long validMask = __ballot(valid), correctMask = __ballot(correct);
    if (lane == 0) { waveValid[wave] = (unsigned int)__popcll(validMask); waveCorrect[wave] = (unsigned int)__popcll(correctMask); }
    __syncthreads();
    int nValid = 0, m = 0, before = 0;
    for (int w = 0; w < MT / 64; ++w) {
        nValid += (int)waveValid[w];
        if (w < wave) before += (int)waveCorrect[w];
        m += (int)waveCorrect[w];
    }
    if (correct) {
        const int slot = before + __popcll(correctMask & ((1ull << lane) - 1ull));
        sP[slot] = P;
        sF[slot] = F;
    }
    __syncthreads();
    const int half = n / 2;
    const bool ok = nValid >= half && m >= half && m >= 2;   // uniform over the workgroup
    float medianX = 0.f, medianY = 0.f, medianRatio = 1.f;
    if (ok) {
        const bool mine = tid < m;
        const float fx = mine ? sF[tid].x - sP[tid].x : 0.f, fy = mine ? sF[tid].y - sP[tid].y : 0.f;
        medianX = flow_unkey(flow_select(hist, chosen, (unsigned int)(m / 2), [&](auto emit) { emit(flow_key(fx), mine); }));
        medianY = flow_unkey(flow_select(hist, chosen, (unsigned int)(m / 2), [&](auto emit) { emit(flow_key(fy), mine); }));
        const unsigned int pairs = (unsigned int)m * (unsigned int)(m - 1) / 2u;
        const int rows = mine ? tid : 0;
        const float2 Pj = mine ? sP[tid] : make_float2(0.f, 0.f), Fj = mine ? sF[tid] : make_float2(0.f, 0.f);
        const float ratio = flow_unkey(flow_select(hist, chosen, pairs / 2u, [&](auto emit) {
            for (int i = 0; i < rows; ++i) {
                const float2 Pi = sP[i], Fi = sF[i];
                const float bx = Pi.x - Pj.x, by = Pi.y - Pj.y;
                const float ax = Fi.x - Fj.x, ay = Fi.y - Fj.y;
                emit(flow_key((ax * ax + ay * ay) / (bx * bx + by * by)), true);
            }
        }));
        medianRatio = sqrtf(ratio);
    }
    if (tid == 0) {
        out->ok = ok ? 1 : 0;
        out->n_valid = nValid;
        out->n_correct = nValid >= half ? m : 0;
        out->median_x = medianX;
        out->median_y = medianY;
        out->median_ratio = medianRatio;
    }
}

}  // namespace

struct fd_flow {
    fd_ctx* ctx = nullptr;
    int width = 0, height = 0;
    fd_flow_params params{};
    float eps2 = 0.f;
    std::vector<FlowLevel> levels;   // of one frame
    size_t slotBytes = 0;
    int cur = 0;                     // the slot of the current frame
    int updates = 0;                 // saturates at 2: both slots hold a frame
    DevBuf arena, table, input, points;
    DevBuf motion, motionIn;         // fd_flow_motion_info of the last resident track; the arrays of fd_debug_flow_motion
    bool hasMotion = false;
    int residentN = -1;              // points of the resident track whose results `points` still holds, or -1
    HostBuf pinnedPts;               // the points of a resident track on their way to the device
    hipEvent_t ptsUploaded = nullptr;
    HostBuf pinned;                  // a host image on its way to the device
    hipEvent_t uploaded = nullptr;   // recorded behind the copy out of `pinned`
    ~fd_flow() {
        if (uploaded) (void)hipEventDestroy(uploaded);
        if (ptsUploaded) (void)hipEventDestroy(ptsUploaded);
    }
};

namespace {

fd_flow* flow_checked(fd_ctx* ctx, fd_flow* f, const char* what) {
    if (!ctx || !f) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (f->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
    HIP_CHECK(hipSetDevice(ctx->device));
    return f;
}

int flow_blocks(const FlowLevel& L) { return (L.pw * L.ph + 255) / 256; }

// device layout of the points of a call: pts, fwd, bwd (2 n floats each), fstatus, bstatus (n bytes each), trace
struct FlowPointBufs {
    float *pts, *fwd, *bwd;
    uint8_t *fstatus, *bstatus, *trace;
};
FlowPointBufs flow_point_bufs(const fd_flow* f) {
    const size_t N = FD_FLOW_MAX_POINTS;
    unsigned char* b = f->points.as<unsigned char>();
    FlowPointBufs q;
    q.pts = (float*)b; q.fwd = q.pts + 2 * N; q.bwd = q.fwd + 2 * N;
    q.fstatus = b + 24 * N; q.bstatus = q.fstatus + N; q.trace = q.bstatus + N;
    return q;
}

void flow_check_points(const fd_flow* f, const char* what, const float* pts, int n) {
    if (n < 0 || n > FD_FLOW_MAX_POINTS) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %d points, at most %d per call", what, n, FD_FLOW_MAX_POINTS);
    if (n > 0 && !pts) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (f->updates < 2) FD_THROW(FD_ERR_RUNTIME, "%s: needs two frames (fd_flow_update)", what);
}

void flow_launch_track(fd_ctx* ctx, const fd_flow* f, int backward, const float* dpts, int n, float* dout, uint8_t* dstatus, uint8_t* dtrace) {
    const uint8_t* current = f->arena.as<uint8_t>() + f->slotBytes * (size_t)f->cur;
    const uint8_t* previous = f->arena.as<uint8_t>() + f->slotBytes * (size_t)(f->cur ^ 1);
    hipLaunchKernelGGL(k_lk_track, dim3(n), dim3(64), 0, ctx->stream, backward ? current : previous, backward ? previous : current,
                       f->table.as<FlowLevel>(), (int)f->levels.size(), f->params.win_w, f->params.win_h, f->params.max_count, f->eps2,
                       (float)f->params.min_eig_threshold, dpts, n, dout, dstatus, dtrace);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int fd_flow_default_params(fd_flow_params* out) {
    if (!out) return FD_ERR_INVALID_ARGUMENT;
    out->win_w = 15; out->win_h = 15; out->max_level = 2; out->max_count = 30; out->epsilon = 0.01; out->min_eig_threshold = 1e-4;
    return FD_OK;
}

int fd_flow_limits(int* max_points, int* min_window, int* max_window) {
    if (max_points) *max_points = FD_FLOW_MAX_POINTS;
    if (min_window) *min_window = FD_FLOW_MIN_WINDOW;
    if (max_window) *max_window = FD_FLOW_MAX_WINDOW;
    return FD_OK;
}

int fd_flow_create(fd_ctx* ctx, int width, int height, const fd_flow_params* params, fd_flow** out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !params || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_create: NULL argument");
        if (width < 1 || height < 1 || width > 16384 || height > 16384) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_create: image of %d x %d", width, height);
        if (params->win_w < FD_FLOW_MIN_WINDOW || params->win_w > FD_FLOW_MAX_WINDOW || params->win_h < FD_FLOW_MIN_WINDOW || params->win_h > FD_FLOW_MAX_WINDOW)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_create: window of %d x %d, each side must be %d .. %d", params->win_w, params->win_h, FD_FLOW_MIN_WINDOW,
                     FD_FLOW_MAX_WINDOW);
        if (params->max_level < 0 || params->max_level >= FD_FLOW_MAX_LEVELS)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_create: max_level %d, must be 0 .. %d", params->max_level, FD_FLOW_MAX_LEVELS - 1);
        if (!(params->min_eig_threshold == params->min_eig_threshold) || !(params->epsilon == params->epsilon))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_create: a parameter is not a number");
        HIP_CHECK(hipSetDevice(ctx->device));
        std::unique_ptr<fd_flow> f(new fd_flow());
        f->ctx = ctx;
        f->width = width;
        f->height = height;
        f->params = *params;
        f->params.max_count = std::min(std::max(params->max_count, 0), 100);       // cv::TermCriteria as calcOpticalFlowPyrLK clamps it
        f->params.epsilon = std::min(std::max(params->epsilon, 0.0), 10.0);
        f->eps2 = (float)(f->params.epsilon * f->params.epsilon);
        size_t off = 0;
        int w = width, h = height;
        for (int level = 0; level <= params->max_level; ++level) {
            if (level > 0 && (w <= params->win_w || h <= params->win_h)) break;   // buildOpticalFlowPyramid: this level is not built
            FlowLevel L;
            L.w = w; L.h = h; L.pw = w + 2 * params->win_w; L.ph = h + 2 * params->win_h;
            L.img_off = (uint32_t)off;
            off = (off + (size_t)L.pw * L.ph + 63) & ~(size_t)63;
            L.der_off = (uint32_t)off;
            off = (off + 4 * (size_t)L.pw * L.ph + 63) & ~(size_t)63;
            f->levels.push_back(L);
            w = (w + 1) / 2;
            h = (h + 1) / 2;
        }
        f->slotBytes = off;   // under 2^32 for the largest image: the offsets of a level are uint32
        f->arena.reserve(2 * off);
        HIP_CHECK(hipMemset(f->arena.p, 0, 2 * off));
        f->table.reserve(sizeof(FlowLevel) * f->levels.size());
        HIP_CHECK(hipMemcpy(f->table.p, f->levels.data(), sizeof(FlowLevel) * f->levels.size(), hipMemcpyHostToDevice));
        f->points.reserve((size_t)FD_FLOW_MAX_POINTS * (24 + 2 + 2 * FD_FLOW_MAX_LEVELS));
        HIP_CHECK(hipEventCreateWithFlags(&f->uploaded, hipEventDisableTiming));
        *out = f.release();
    });
}

void fd_flow_destroy(fd_flow* flow) { delete flow; }

int fd_flow_levels(const fd_flow* flow) { return flow ? (int)flow->levels.size() : 0; }

int fd_flow_update(fd_ctx* ctx, fd_flow* flow, const uint8_t* image, int channels, int stride, int on_device) {
    return fd_guard(ctx, [&] {
        fd_flow* f = flow_checked(ctx, flow, "fd_flow_update");
        if (!image) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_update: NULL argument");
        if (channels != 1 && channels != 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_update: %d channels, must be 1 (gray) or 3 (BGR)", channels);
        const int row = f->width * channels;
        if (stride == 0) stride = row;
        if (stride < row) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_update: stride %d is shorter than a row of %d bytes", stride, row);
        const uint8_t* src = image;
        int srcStride = stride;
        if (!on_device) {
            // through pinned memory: the caller's image is free when the call returns, and the copy does not wait for the stream
            const size_t bytes = (size_t)row * f->height;
            f->input.reserve(bytes);
            HIP_CHECK(hipEventSynchronize(f->uploaded));
            f->pinned.reserve(bytes);
            for (int y = 0; y < f->height; ++y) std::memcpy(f->pinned.as<uint8_t>() + (size_t)y * row, image + (size_t)y * stride, row);
            HIP_CHECK(hipMemcpyAsync(f->input.p, f->pinned.p, bytes, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipEventRecord(f->uploaded, ctx->stream));
            src = f->input.as<uint8_t>();
            srcStride = row;
        }
        const int next = f->cur ^ 1;
        uint8_t* slot = f->arena.as<uint8_t>() + f->slotBytes * (size_t)next;
        const int winW = f->params.win_w, winH = f->params.win_h;
        for (size_t l = 0; l < f->levels.size(); ++l) {
            const FlowLevel& L = f->levels[l];
            if (l == 0) {
                hipLaunchKernelGGL(k_flow_level0, dim3(flow_blocks(L)), dim3(256), 0, ctx->stream, src, channels, srcStride, slot + L.img_off, L.w, L.h, winW, winH);
            } else {
                const FlowLevel& S = f->levels[l - 1];
                hipLaunchKernelGGL(k_flow_pyrdown_pad, dim3(flow_blocks(L)), dim3(256), 0, ctx->stream, slot + S.img_off, S.pw, S.w, S.h, slot + L.img_off, L.w, L.h,
                                   winW, winH);
            }
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_flow_scharr_pad, dim3(flow_blocks(L)), dim3(256), 0, ctx->stream, slot + L.img_off, (int16_t*)(slot + L.der_off), L.w, L.h, winW, winH);
            HIP_CHECK(hipGetLastError());
        }
        f->cur = next;
        if (f->updates < 2) ++f->updates;
    });
}

int fd_flow_track(fd_ctx* ctx, fd_flow* flow, int backward, const float* pts_xy, int n, float* out_xy, uint8_t* status, uint8_t* trace) {
    return fd_guard(ctx, [&] {
        fd_flow* f = flow_checked(ctx, flow, "fd_flow_track");
        flow_check_points(f, "fd_flow_track", pts_xy, n);
        if (n == 0) return;
        if (!out_xy || !status) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_track: NULL argument");
        f->residentN = -1;
        const FlowPointBufs q = flow_point_bufs(f);
        const size_t N = (size_t)n;
        HIP_CHECK(hipMemcpyAsync(q.pts, pts_xy, 8 * N, hipMemcpyHostToDevice, ctx->stream));
        flow_launch_track(ctx, f, backward != 0, q.pts, n, q.fwd, q.fstatus, trace ? q.trace : nullptr);
        HIP_CHECK(hipMemcpyAsync(out_xy, q.fwd, 8 * N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(status, q.fstatus, N, hipMemcpyDeviceToHost, ctx->stream));
        if (trace) HIP_CHECK(hipMemcpyAsync(trace, q.trace, 2 * FD_FLOW_MAX_LEVELS * N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_flow_track_fb(fd_ctx* ctx, fd_flow* flow, const float* pts_xy, int n, float* fwd, float* bwd, uint8_t* fstatus, uint8_t* bstatus) {
    return fd_guard(ctx, [&] {
        fd_flow* f = flow_checked(ctx, flow, "fd_flow_track_fb");
        flow_check_points(f, "fd_flow_track_fb", pts_xy, n);
        if (n == 0) return;
        if (!fwd || !bwd || !fstatus || !bstatus) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_track_fb: NULL argument");
        f->residentN = -1;
        const FlowPointBufs q = flow_point_bufs(f);
        const size_t N = (size_t)n;
        HIP_CHECK(hipMemcpyAsync(q.pts, pts_xy, 8 * N, hipMemcpyHostToDevice, ctx->stream));
        flow_launch_track(ctx, f, 0, q.pts, n, q.fwd, q.fstatus, nullptr);
        flow_launch_track(ctx, f, 1, q.fwd, n, q.bwd, q.bstatus, nullptr);
        HIP_CHECK(hipMemcpyAsync(fwd, q.fwd, 8 * N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(bwd, q.bwd, 8 * N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(fstatus, q.fstatus, N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(bstatus, q.bstatus, N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_flow_track_fb_resident(fd_ctx* ctx, fd_flow* flow, const float* pts_xy, int n) {
    return fd_guard(ctx, [&] {
        fd_flow* f = flow_checked(ctx, flow, "fd_flow_track_fb_resident");
        if (n > FD_FLOW_RESIDENT_MAX_POINTS)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_track_fb_resident: %d points, at most %d stay on the device", n, FD_FLOW_RESIDENT_MAX_POINTS);
        flow_check_points(f, "fd_flow_track_fb_resident", pts_xy, n);
        const FlowPointBufs q = flow_point_bufs(f);
        f->motion.reserve(sizeof(fd_flow_motion_info));
        if (n > 0) {
            // through pinned memory: the caller's points are free when the call returns, and the copy does not wait for the stream
            if (!f->ptsUploaded) HIP_CHECK(hipEventCreateWithFlags(&f->ptsUploaded, hipEventDisableTiming));
            HIP_CHECK(hipEventSynchronize(f->ptsUploaded));
            f->pinnedPts.reserve(8 * (size_t)FD_FLOW_RESIDENT_MAX_POINTS);
            std::memcpy(f->pinnedPts.p, pts_xy, 8 * (size_t)n);
            HIP_CHECK(hipMemcpyAsync(q.pts, f->pinnedPts.p, 8 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipEventRecord(f->ptsUploaded, ctx->stream));
            flow_launch_track(ctx, f, 0, q.pts, n, q.fwd, q.fstatus, nullptr);
            flow_launch_track(ctx, f, 1, q.fwd, n, q.bwd, q.bstatus, nullptr);
        }
        hipLaunchKernelGGL(k_flow_motion, dim3(1), dim3(MT), 0, ctx->stream, (const float2*)q.pts, (const float2*)q.fwd, (const float2*)q.bwd, q.fstatus,
                           q.bstatus, n, f->motion.as<fd_flow_motion_info>());
        HIP_CHECK(hipGetLastError());
        f->hasMotion = true;
        f->residentN = n;
    });
}

int fd_flow_get_tracks(fd_ctx* ctx, fd_flow* flow, int cap, int* n, float* fwd, float* bwd, uint8_t* fstatus, uint8_t* bstatus, int32_t* order,
                       int* n_valid, int* n_correct) {
    return fd_guard(ctx, [&] {
        fd_flow* f = flow_checked(ctx, flow, "fd_flow_get_tracks");
        if (cap < 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_flow_get_tracks: bad argument");
        if (f->residentN < 0) FD_THROW(FD_ERR_RUNTIME, "fd_flow_get_tracks: the handle holds no resident track (fd_flow_track_fb_resident)");
        const int count = f->residentN;
        if (n) *n = count;
        if (count > cap) FD_THROW(FD_ERR_CAPACITY, "fd_flow_get_tracks: %d points, capacity %d", count, cap);
        const size_t N = (size_t)count;
        const FlowPointBufs q = flow_point_bufs(f);
        std::vector<float> host(6 * N);
        std::vector<uint8_t> st(2 * N);
        if (N) {
            HIP_CHECK(hipMemcpyAsync(host.data(), q.pts, 8 * N, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(host.data() + 2 * N, q.fwd, 8 * N, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(host.data() + 4 * N, q.bwd, 8 * N, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(st.data(), q.fstatus, N, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(st.data() + N, q.bstatus, N, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (fwd && N) std::memcpy(fwd, host.data() + 2 * N, 8 * N);
        if (bwd && N) std::memcpy(bwd, host.data() + 4 * N, 8 * N);
        if (fstatus && N) std::memcpy(fstatus, st.data(), N);
        if (bstatus && N) std::memcpy(bstatus, st.data() + N, N);
        if (order || n_valid || n_correct) {
            fd_flow_motion m;
            m.order = order;
            const int rc = fd_flow_median(host.data(), host.data() + 2 * N, host.data() + 4 * N, st.data(), st.data() + N, count, &m);
            if (rc != FD_OK) FD_THROW(rc, "fd_flow_get_tracks: fd_flow_median refused the tracks");
            if (n_valid) *n_valid = m.n_valid;
            if (n_correct) *n_correct = m.n_correct;
        }
    });
}

int fd_debug_flow_motion(fd_ctx* ctx, fd_flow* flow, const float* pts, const float* fwd, const float* bwd, const uint8_t* fstatus,
                         const uint8_t* bstatus, int n, fd_flow_motion_info* out) {
    return fd_guard(ctx, [&] {
        fd_flow* f = flow_checked(ctx, flow, "fd_debug_flow_motion");
        if (n < 0 || n > FD_FLOW_RESIDENT_MAX_POINTS)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_debug_flow_motion: %d points, must be 0 .. %d", n, FD_FLOW_RESIDENT_MAX_POINTS);
        if (!out || (n > 0 && (!pts || !fwd || !bwd || !fstatus || !bstatus))) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_debug_flow_motion: NULL argument");
        const size_t M = FD_FLOW_RESIDENT_MAX_POINTS, N = (size_t)n;
        f->motionIn.reserve(26 * M);   // pts, fwd, bwd (8 M each), fstatus, bstatus (M each)
        f->motion.reserve(sizeof(fd_flow_motion_info));
        unsigned char* b = f->motionIn.as<unsigned char>();
        if (N) {
            HIP_CHECK(hipMemcpyAsync(b, pts, 8 * N, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(b + 8 * M, fwd, 8 * N, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(b + 16 * M, bwd, 8 * N, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(b + 24 * M, fstatus, N, hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(b + 25 * M, bstatus, N, hipMemcpyHostToDevice, ctx->stream));
        }
        hipLaunchKernelGGL(k_flow_motion, dim3(1), dim3(MT), 0, ctx->stream, (const float2*)b, (const float2*)(b + 8 * M), (const float2*)(b + 16 * M),
                           b + 24 * M, b + 25 * M, n, f->motion.as<fd_flow_motion_info>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, f->motion.p, sizeof(*out), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        f->hasMotion = true;
    });
}

int fd_debug_flow_level(fd_ctx* ctx, fd_flow* flow, int which, int level, uint8_t* image_out, int16_t* deriv_out, int* w, int* h) {
    return fd_guard(ctx, [&] {
        fd_flow* f = flow_checked(ctx, flow, "fd_debug_flow_level");
        if (which != 0 && which != 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_debug_flow_level: which must be 0 (current) or 1 (previous)");
        if (level < 0 || level >= (int)f->levels.size()) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_debug_flow_level: level %d of %d", level, (int)f->levels.size());
        if (f->updates < 1 + which) FD_THROW(FD_ERR_RUNTIME, "fd_debug_flow_level: that frame has not been given (fd_flow_update)");
        const FlowLevel& L = f->levels[level];
        if (w) *w = L.pw;
        if (h) *h = L.ph;
        const uint8_t* slot = f->arena.as<uint8_t>() + f->slotBytes * (size_t)(which ? f->cur ^ 1 : f->cur);
        const size_t px = (size_t)L.pw * L.ph;
        if (image_out) HIP_CHECK(hipMemcpyAsync(image_out, slot + L.img_off, px, hipMemcpyDeviceToHost, ctx->stream));
        if (deriv_out) HIP_CHECK(hipMemcpyAsync(deriv_out, slot + L.der_off, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"

const fd_flow_motion_info* fd_flow_device_motion(fd_ctx* ctx, fd_flow* flow, const char* who) {
    fd_flow* f = flow_checked(ctx, flow, who);
    if (!f->hasMotion) FD_THROW(FD_ERR_RUNTIME, "%s: the flow handle holds no motion (fd_flow_track_fb_resident)", who);
    return f->motion.as<fd_flow_motion_info>();
}
