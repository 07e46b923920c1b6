// featuredetection_amd/csrc/win_table.hpp -- what every "scan all windows of the pyramid" family beside the WVM cascade shares (HOG,
// the histogram filters, the whi chain, the RVM detector): the device window table and its host builders, the device window id ->
// position search, the device append of positive records, and the host tail that turns them into fd_detections.
//
// One numbering rule, the one of fd_enumerate_layers and fd_window_to_detection: windows are numbered layer by layer in extraction
// order (DirectPyramidFeatureExtractor.cpp:75-123), row-major inside a layer.  Layers without windows are left out of the table
// (in the host's layer list they share their successor's `first`).  Kernels that work in tiles repeat the last window behind the end.
#pragma once
#include "fd_internal.hpp"
#include <algorithm>
#include <cstring>

constexpr int FD_WIN_MAX_LAYERS = 64;

struct FdWinLayer {
    int32_t bx, by, nx, ny;
    int32_t lw;          // layer width in pixels
    uint32_t off;        // byte offset of the layer's plane in the arena
    int64_t first;
};
struct FdWinTable {
    int32_t n, sx, sy, raw;   // raw != 0 (whi.hip): `total` contiguous patches, no layers
    int64_t total;
    // list mode (fd_win_table_list): `total` explicit windows, window wid is the triple {layer, bx, by} at list[3 * wid]; l[layer]
    // names the plane (lw, off).  NULL: the windows of a strided scan, as every other builder leaves it
    const int32_t* list;
    FdWinLayer l[FD_WIN_MAX_LAYERS];
};

// the windows of (patch, step, roi) over the pyramid's layers; `off` names the filtered plane of a layer or its gray plane
static inline void fd_win_table_build(const fd_pyramid* p, int pw, int ph, int sx, int sy, const int* roi, bool filtered, FdWinTable& wt,
                                      std::vector<WindowLayer>& wls) {
    fd_pyramid_require_image(p);
    int64_t total;
    fd_enumerate_layers(p, pw, ph, sx, sy, roi, wls, total);
    if (wls.size() > (size_t)FD_WIN_MAX_LAYERS) FD_THROW(FD_ERR_INVALID_ARGUMENT, "too many pyramid layers (%zu)", wls.size());
    std::memset(&wt, 0, sizeof(wt));
    wt.sx = sx; wt.sy = sy; wt.total = total;
    for (const WindowLayer& w : wls) {
        if (w.nx == 0 || w.ny == 0) continue;
        const HostLayer& L = p->all[p->kept[w.layer]];
        FdWinLayer& dl = wt.l[wt.n++];
        dl.bx = w.bx; dl.by = w.by; dl.nx = w.nx; dl.ny = w.ny; dl.lw = L.w; dl.off = filtered ? L.filt_off : L.gray_off; dl.first = w.first;
    }
}

// n contiguous patches
static inline FdWinTable fd_win_table_raw(int64_t n) {
    FdWinTable wt;
    std::memset(&wt, 0, sizeof(wt));
    wt.raw = 1;
    wt.total = n;
    return wt;
}

// n contiguous patch_w x patch_h patches addressed as one layer patch_w wide whose windows are patch_h rows apart
static inline FdWinTable fd_win_table_column(int64_t n, int patch_w, int patch_h) {
    FdWinTable wt;
    std::memset(&wt, 0, sizeof(wt));
    wt.n = 1; wt.sx = 1; wt.sy = patch_h; wt.total = n;
    wt.l[0].nx = 1; wt.l[0].ny = (int32_t)n; wt.l[0].lw = patch_w;
    return wt;
}

// `total` explicit windows {layer, bx, by} (device memory, layer = position in the kept-layer list) on the filtered planes of p or on
// its gray planes
static inline void fd_win_table_list(const fd_pyramid* p, const int32_t* dlist, int64_t total, bool filtered, FdWinTable& wt) {
    fd_pyramid_require_image(p);
    if (p->kept.size() > (size_t)FD_WIN_MAX_LAYERS) FD_THROW(FD_ERR_INVALID_ARGUMENT, "too many pyramid layers (%zu)", p->kept.size());
    std::memset(&wt, 0, sizeof(wt));
    wt.n = (int32_t)p->kept.size(); wt.sx = wt.sy = 1; wt.total = total; wt.list = dlist;
    for (size_t i = 0; i < p->kept.size(); ++i) {
        const HostLayer& L = p->all[p->kept[i]];
        wt.l[i].nx = 1; wt.l[i].ny = 1; wt.l[i].lw = L.w; wt.l[i].off = filtered ? L.filt_off : L.gray_off;
    }
}

namespace fd_dev {

// window wid < total -> its layer record and the window's pixel origin (x, y) in that layer
__device__ __forceinline__ const FdWinLayer& win_locate(const FdWinTable& wt, int64_t wid, int& x, int& y) {
    if (wt.list) {
        const int32_t* t = wt.list + 3 * wid;
        x = t[1];
        y = t[2];
        return wt.l[t[0]];
    }
    int li = 0;
    for (int l = 1; l < wt.n; ++l) li = wt.l[l].first <= wid ? l : li;
    const FdWinLayer& wl = wt.l[li];
    const int local = (int)(wid - wl.first);
    const int iy = local / wl.nx, ix = local - iy * wl.nx;
    x = wl.bx + ix * wt.sx;
    y = wl.by + iy * wt.sy;
    return wl;
}

}  // namespace fd_dev

// ---- positives: the record the kernels append, and its way to the caller's fd_detection ----
struct FdPosRec {
    uint32_t wid_lo, wid_hi;
    double d;   // hyperplane distance (RVM: also the running distance of a survivor between passes)
};
__host__ __device__ inline uint64_t fd_pos_wid(const FdPosRec& r) { return ((uint64_t)r.wid_hi << 32) | r.wid_lo; }

namespace fd_dev {

// appends the records of this wavefront's `positive` lanes to recs (one atomic on *counter per wavefront; records from slot cap on
// are counted, not written).  Every lane of the wavefront must reach the call: wavefront-uniform control flow around it.  The order
// of the records in the buffer is not defined (the hosts sort by window id)
__device__ __forceinline__ void pos_append(FdPosRec* recs, unsigned int* counter, unsigned int cap, bool positive, int64_t wid, double d) {
    const unsigned long long mask = __ballot(positive);
    if (!mask) return;
    const int lane = threadIdx.x & 63;
    unsigned int base = 0;
    if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(counter, (unsigned int)__popcll(mask));
    base = __shfl(base, __ffsll((long long)mask) - 1, 64);
    if (positive) {
        const unsigned int slot = base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
        if (slot < cap) recs[slot] = FdPosRec{(uint32_t)wid, (uint32_t)(wid >> 32), d};
    }
}

}  // namespace fd_dev

// extraction order
static inline bool fd_pos_before(const FdPosRec& a, const FdPosRec& b) { return fd_pos_wid(a) < fd_pos_wid(b); }
static inline void fd_pos_sort(FdPosRec* r, size_t n) {
    std::sort(r, r + n, [](const FdPosRec& a, const FdPosRec& b) { return fd_pos_before(a, b); });   // (a lambda: inlined into the sort)
}

// a positive record -> the ClassifiedPatch of SlidingWindowDetector::detect
static inline fd_detection fd_pos_detection(const fd_pyramid* p, const std::vector<WindowLayer>& wls, int sx, int sy, const FdPosRec& r, int level,
                                            double probability) {
    fd_detection d;
    std::memset(&d, 0, sizeof(d));
    fd_window_to_detection(p, wls, sx, sy, (int64_t)fd_pos_wid(r), d);
    d.level = level;
    d.positive = 1;
    d.score = (float)r.d;
    d.probability = probability;
    return d;
}
