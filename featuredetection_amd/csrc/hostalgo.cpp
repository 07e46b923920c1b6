// featuredetection_amd/csrc/hostalgo.cpp -- host-side stage glue of the detection path: the greedy,
// order-dependent steps that the reference runs on a handful of survivors per image
// (OverlapElimination, block non-maxima suppression).  They stay on the host: n is tens to a few
// thousand records and the algorithms are sequential by definition (sort + greedy erase).
#include "fd_internal.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>

// detection::OverlapElimination::eliminate (OverlapElimination.cpp:44-105).  std::sort on the
// probability only (boost::indirect_iterator + std::greater<ClassifiedPatch>), then the greedy erase:
// an element survives iff no earlier *surviving* element (in sorted order) overlaps it.  The reference
// is O(n^2) with vector::erase; here survivors are bucketed in a (hashed) uniform grid whose cell is at least
// the largest possible distance threshold, so only the 3x3 neighbouring cells are examined.  The
// result (content and order) is identical for any n.
void fd_host_overlap_elimination(const fd_detection* in, int n, float distIn, float ratioIn, std::vector<int>& keep) {
    keep.clear();
    if (n <= 0) return;
    // descending probability.  Sorting (probability, index) pairs makes the same comparisons with the same outcomes as sorting the
    // indices through the detections, so std::sort produces the same permutation (ties included) without chasing 48-byte records
    struct Key { double p; int i; };
    std::vector<Key> keyed(n);
    for (int i = 0; i < n; ++i) keyed[i] = Key{in[i].probability, i};
    std::sort(keyed.begin(), keyed.end(), [](const Key& a, const Key& b) { return a.p > b.p; });
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = keyed[i].i;
    const float dist = distIn;
    const float ratio = ((ratioIn > 0.0f) && (ratioIn <= 1.0f)) ? ratioIn : 0.0f;
    int maxw = 1;
    for (int i = 0; i < n; ++i) maxw = std::max(maxw, in[i].w);
    const float dmax = dist <= 1.0 ? dist * maxw : dist;
    const int cell = std::max(1, (int)std::ceil(dmax > 0 ? dmax : 1.f));
    auto cellOf = [&](int v) { return v >= 0 ? v / cell : -((-v + cell - 1) / cell); };
    std::vector<int> next(n, -1);
    auto overlaps = [&](const fd_detection& A, const fd_detection& P) {
        const float d = dist <= 1.0 ? dist * std::max(A.w, P.w) : dist;
        return (std::abs(A.cx - P.cx) < d) && (std::abs(A.cy - P.cy) < d) && (((float)std::min(A.w, P.w) / (float)std::max(A.w, P.w)) > ratio);
    };
    keep.reserve(n);
    // The usual parameters -- an absolute distance and no size ratio (dist > 1, ratio == 0: FaceFrontal.cfg's 5 / 0 and every other cfg of
    // ffpDetectApp) -- make the test a function of the two centres alone: |dx| < d and |dy| < d with integer dx, dy is |dx|, |dy| <= ceil(d) -
    // 1, and min(w) / max(w) > 0 holds for positive widths.  An element is then removed iff its centre lies inside the square around the
    // centre of an element accepted before it, so the accepted squares are painted into a byte map over the centres' bounding box and
    // every element costs ONE lookup (a survivor (2 ceil(d) - 1)^2 stores) instead of nine list walks: 12 K WVM positives of a 1080p
    // detector 1.4 -> 0.2 ms behind the sort.  The greedy order, and with it the result, is unchanged.
    {
        bool positiveW = true;
        int cx0 = INT32_MAX, cx1 = INT32_MIN, cy0 = INT32_MAX, cy1 = INT32_MIN;
        for (int i = 0; i < n; ++i) {
            positiveW = positiveW && in[i].w > 0;
            cx0 = std::min(cx0, in[i].cx); cx1 = std::max(cx1, in[i].cx); cy0 = std::min(cy0, in[i].cy); cy1 = std::max(cy1, in[i].cy);
        }
        const bool simple = dist > 1.0f && dist < 4096.0f && ratio == 0.0f && positiveW;
        const int r = simple ? (int)std::ceil(dist) - 1 : 0;   // |dx| <= r
        const int64_t mw = (int64_t)cx1 - cx0 + 1 + 2 * (int64_t)r, mh = (int64_t)cy1 - cy0 + 1 + 2 * (int64_t)r;
        if (simple && mw * mh <= (int64_t)1 << 24) {
            std::vector<uint8_t> blocked((size_t)(mw * mh), 0);
            for (int bi = 0; bi < n; ++bi) {
                const fd_detection& P = in[order[bi]];
                const int64_t x = (int64_t)P.cx - cx0 + r, y = (int64_t)P.cy - cy0 + r;
                if (blocked[(size_t)(y * mw + x)]) continue;
                keep.push_back(order[bi]);
                for (int64_t yy = y - r; yy <= y + r; ++yy) std::fill_n(blocked.begin() + (size_t)(yy * mw + x - r), (size_t)(2 * r + 1), (uint8_t)1);
            }
            return;
        }
    }
    // accepted elements per grid cell (singly linked lists).  The centres of a frame's detections span a small range, so the
    // grid is a dense array (with a one-cell border); an open-addressed hash table takes over for pathological extents.
    int gx0 = INT32_MAX, gx1 = INT32_MIN, gy0 = INT32_MAX, gy1 = INT32_MIN;
    for (int i = 0; i < n; ++i) {
        const int gx = cellOf(in[i].cx), gy = cellOf(in[i].cy);
        gx0 = std::min(gx0, gx); gx1 = std::max(gx1, gx); gy0 = std::min(gy0, gy); gy1 = std::max(gy1, gy);
    }
    const int64_t gw = (int64_t)gx1 - gx0 + 3, gh = (int64_t)gy1 - gy0 + 3;
    if (gw * gh <= (int64_t)1 << 22) {
        std::vector<int> head((size_t)(gw * gh), -1);
        for (int bi = 0; bi < n; ++bi) {
            const fd_detection& P = in[order[bi]];
            const int64_t base = (int64_t)(cellOf(P.cy) - gy0 + 1) * gw + (cellOf(P.cx) - gx0 + 1);
            bool removed = false;
            for (int dy = -1; dy <= 1 && !removed; ++dy)
                for (int dx = -1; dx <= 1 && !removed; ++dx)
                    for (int ai = head[(size_t)(base + dy * gw + dx)]; ai >= 0; ai = next[ai])
                        if (overlaps(in[ai], P)) { removed = true; break; }
            if (!removed) {
                keep.push_back(order[bi]);
                next[order[bi]] = head[(size_t)base];
                head[(size_t)base] = order[bi];
            }
        }
        return;
    }
    size_t cap = 16;
    while (cap < (size_t)n * 4) cap <<= 1;
    std::vector<uint64_t> keys(cap, ~0ull);
    std::vector<int> head(cap, -1);
    auto slotOf = [&](int gy, int gx, bool insert) -> int64_t {
        const uint64_t key = ((uint64_t)(uint32_t)gy << 32) | (uint32_t)gx;
        size_t h = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1);
        while (keys[h] != ~0ull && keys[h] != key) h = (h + 1) & (cap - 1);
        if (keys[h] == key) return (int64_t)h;
        if (!insert) return -1;
        keys[h] = key;
        return (int64_t)h;
    };
    for (int bi = 0; bi < n; ++bi) {
        const fd_detection& P = in[order[bi]];
        const int gx = cellOf(P.cx), gy = cellOf(P.cy);
        bool removed = false;
        for (int dy = -1; dy <= 1 && !removed; ++dy)
            for (int dx = -1; dx <= 1 && !removed; ++dx) {
                const int64_t h = slotOf(gy + dy, gx + dx, false);
                if (h < 0) continue;
                for (int ai = head[h]; ai >= 0; ai = next[ai])
                    if (overlaps(in[ai], P)) { removed = true; break; }
            }
        if (!removed) {
            keep.push_back(order[bi]);
            const int64_t h = slotOf(gy, gx, true);
            next[order[bi]] = head[h];
            head[h] = order[bi];
        }
    }
}

// nonMaximaSuppression (FiveStageSlidingWindowDetector.cpp:143-184) evaluated on the sparse set of
// non-zero map entries instead of a dense H x W probability map.  Equivalent because (a) blocks
// without a (masked) entry can never produce a maximum (candidate value 0 is never > neighbour
// maximum >= 0), and (b) cv::minMaxLoc returns the first row-major maximum, which the ordered
// std::map reproduces.  masked: only entries with value > 0.3 take part (mask = map > 0.3f, :286).
void fd_host_block_nms_sparse(const std::vector<fd_detection>& pos, int imgW, int imgH, int sz, bool masked,
                              std::vector<int>& maxima_xy) {
    maxima_xy.clear();
    // probabilityMap(py, px) = max probability at that pixel (:277-284), as float: the reference's running
    // "if (map(y, x) < p) map(y, x) = p" ends at (float)(largest p) whatever the order (float rounding is monotonic), and pixels
    // whose probabilities are all <= 0 keep the map's 0.  Sorted vectors instead of node-based maps.
    struct Pt { int x, y; float v; };
    std::vector<Pt> all;
    all.reserve(pos.size());
    for (const fd_detection& d : pos) {
        if (d.cx < 0 || d.cy < 0 || d.cx >= imgW || d.cy >= imgH) continue;  // (reference: out-of-range Mat::at, UB)
        if (!(0.f < d.probability)) continue;
        all.push_back(Pt{d.cx, d.cy, (float)d.probability});
    }
    std::sort(all.begin(), all.end(), [](const Pt& a, const Pt& b) { return a.y != b.y ? a.y < b.y : (a.x != b.x ? a.x < b.x : a.v > b.v); });
    std::vector<Pt> pts;   // row-major order, one entry per pixel (its maximum)
    pts.reserve(all.size());
    for (size_t i = 0; i < all.size(); ++i) {
        if (i > 0 && all[i].x == all[i - 1].x && all[i].y == all[i - 1].y) continue;
        if (masked && !(all[i].v > 0.3f)) continue;
        pts.push_back(all[i]);
    }
    // group by block, keeping row-major order inside each block: indices sorted (stably) by block id
    const int bs = sz + 1;
    const int64_t bcols = (int64_t)imgW / bs + 2;
    auto blockId = [&](const Pt& q) { return (int64_t)(q.y / bs) * bcols + q.x / bs; };
    std::vector<int> byBlock(pts.size());
    for (size_t i = 0; i < pts.size(); ++i) byBlock[i] = (int)i;
    std::stable_sort(byBlock.begin(), byBlock.end(), [&](int a, int b) { return blockId(pts[a]) < blockId(pts[b]); });
    struct Blk { int64_t id; int begin, end; };
    std::vector<Blk> blocks;
    for (size_t i = 0; i < byBlock.size();) {
        size_t j = i;
        const int64_t id = blockId(pts[byBlock[i]]);
        while (j < byBlock.size() && blockId(pts[byBlock[j]]) == id) ++j;
        blocks.push_back(Blk{id, (int)i, (int)j});
        i = j;
    }
    auto findBlock = [&](int64_t id) -> const Blk* {
        auto it = std::lower_bound(blocks.begin(), blocks.end(), id, [](const Blk& b, int64_t v) { return b.id < v; });
        return it != blocks.end() && it->id == id ? &*it : nullptr;
    };
    std::vector<Pt> accepted;
    for (const Blk& blk : blocks) {
        const int brow = (int)(blk.id / bcols), bcol = (int)(blk.id % bcols);
        const int m = brow * bs, n = bcol * bs;
        // candidate: first maximum of the block (row-major order inside the block)
        int best = -1;
        for (int t = blk.begin; t < blk.end; ++t) {
            const int i = byBlock[t];
            if (best < 0 || pts[i].v > pts[best].v) best = i;
        }
        const Pt c = pts[best];
        if (!masked && !(c.v > 0.f)) continue;
        const double vcmax = c.v;
        // neighbourhood (2sz+1)^2 around the candidate, minus the candidate's own block
        const int y0 = std::max(c.y - sz, 0), y1 = std::min(c.y + sz + 1, imgH);
        const int x0 = std::max(c.x - sz, 0), x1 = std::min(c.x + sz + 1, imgW);
        const int by0 = m, by1 = std::min(m + sz + 1, imgH), bx0 = n, bx1 = std::min(n + sz + 1, imgW);
        double vnmax = 0;  // all-zero mask => 0; unmasked => zeros of the map
        bool any = false;
        // the neighbourhood reaches at most one block in every direction: only the points of those blocks are looked at
        // (a maximum, so the visiting order does not matter)
        for (int br = brow - 1; br <= brow + 1; ++br)
            for (int bc = bcol - 1; bc <= bcol + 1; ++bc) {
                if (br < 0 || bc < 0 || (br == brow && bc == bcol)) continue;
                const Blk* nb = findBlock((int64_t)br * bcols + bc);
                if (!nb) continue;
                for (int t = nb->begin; t < nb->end; ++t) {
                    const Pt& q = pts[byBlock[t]];
                    if (q.y < y0 || q.y >= y1 || q.x < x0 || q.x >= x1) continue;
                    if (!any || q.v > vnmax) { vnmax = q.v; any = true; }
                }
            }
        if (!masked) {
            // unmasked: zeros of the map inside the neighbourhood also count (value 0) whenever the
            // neighbourhood has at least one pixel outside the block
            bool outside = (y0 < by0) || (y1 > by1) || (x0 < bx0) || (x1 > bx1);
            if (!any) vnmax = 0;
            else if (outside && vnmax < 0) vnmax = 0;
        }
        if (vcmax > vnmax) accepted.push_back(c);
    }
    std::sort(accepted.begin(), accepted.end(), [](const Pt& a, const Pt& b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
    for (const Pt& a : accepted) { maxima_xy.push_back(a.x); maxima_xy.push_back(a.y); }
}

extern "C" int fd_overlap_elimination(const fd_detection* in, int n, float dist, float ratio, int32_t* keep_idx, int* count) {
    if (!count || (n > 0 && (!in || !keep_idx))) return FD_ERR_INVALID_ARGUMENT;
    std::vector<int> keep;
    fd_host_overlap_elimination(in, n, dist, ratio, keep);
    for (size_t i = 0; i < keep.size(); ++i) keep_idx[i] = keep[i];
    *count = (int)keep.size();
    return FD_OK;
}

extern "C" int fd_block_nms(const fd_detection* in, int n, int image_w, int image_h, int sz, int masked, int32_t* maxima_xy,
                            int cap_pairs, int* count) {
    if (!count || n < 0 || (n > 0 && !in) || image_w < 1 || image_h < 1 || sz < 0) return FD_ERR_INVALID_ARGUMENT;
    std::vector<fd_detection> v(in, in + n);
    std::vector<int> xy;
    fd_host_block_nms_sparse(v, image_w, image_h, sz, masked != 0, xy);
    *count = (int)(xy.size() / 2);
    if (*count > cap_pairs) return FD_ERR_CAPACITY;
    for (size_t i = 0; i < xy.size(); ++i) maxima_xy[i] = xy[i];
    return FD_OK;
}

// detection::NonMaximumSuppression::eliminateRedundantDetections (NonMaximumSuppression.cpp:27-118): candidates sorted by
// ascending score (std::sort, unstable like the reference), then clusters are peeled off from the back: the best remaining
// detection takes every candidate whose IoU with it exceeds the threshold (std::stable_partition keeps the order of the
// rest), and each cluster (best first) is reduced to its maximum / average / score-weighted average.
extern "C" int fd_nms_iou(const fd_box* in, int n, double overlap_threshold, int maximum_type, fd_box* out, int* count) {
    if (!count || n < 0 || (n > 0 && (!in || !out)) || maximum_type < 0 || maximum_type > 2) return FD_ERR_INVALID_ARGUMENT;
    std::vector<fd_box> candidates(in, in + n);
    if (overlap_threshold == 1.0) {   // :28-29
        for (int i = 0; i < n; ++i) out[i] = in[i];
        *count = n;
        return FD_OK;
    }
    std::sort(candidates.begin(), candidates.end(), [](const fd_box& a, const fd_box& b) { return a.score < b.score; });
    auto overlap = [](const fd_box& a, const fd_box& b) {   // computeOverlap :58-62 with cv::Rect operator& and area()
        const int x = std::max(a.x, b.x), y = std::max(a.y, b.y);
        const int w = std::min(a.x + a.w, b.x + b.w) - x, h = std::min(a.y + a.h, b.y + b.h) - y;
        const double intersectionArea = (w <= 0 || h <= 0) ? 0 : w * h;
        const double unionArea = a.w * a.h + b.w * b.h - intersectionArea;
        return intersectionArea / unionArea;
    };
    int nout = 0;
    while (!candidates.empty()) {
        const fd_box detection = candidates.back();
        auto firstOverlapping = std::stable_partition(candidates.begin(), candidates.end(),
                                                      [&](const fd_box& c) { return overlap(detection, c) <= overlap_threshold; });
        std::vector<fd_box> cluster(firstOverlapping, candidates.end());
        std::reverse(cluster.begin(), cluster.end());
        candidates.erase(firstOverlapping, candidates.end());
        if (cluster.empty()) return FD_ERR_RUNTIME;   // overlap threshold > 1: nothing overlaps, not even the box itself; the reference loops forever
        fd_box r = cluster.front();
        if (maximum_type != 0) {
            double weightSum = 0, xSum = 0, ySum = 0, wSum = 0, hSum = 0;
            for (const fd_box& e : cluster) {
                const double weight = maximum_type == 2 ? (double)e.score : 1.0;
                weightSum += weight;
                xSum += weight * e.x; ySum += weight * e.y; wSum += weight * e.w; hSum += weight * e.h;
            }
            if (maximum_type == 1) weightSum = (double)cluster.size();
            r.x = (int)std::round(xSum / weightSum); r.y = (int)std::round(ySum / weightSum);
            r.w = (int)std::round(wSum / weightSum); r.h = (int)std::round(hSum / weightSum);
        }
        out[nout++] = r;
    }
    *count = nout;
    return FD_OK;
}

// Scale limits of the feature pyramid of an extraction::AggregatedFeaturesExtractor (AggregatedFeaturesExtractor.cpp:30-31,
// 47-77): computed with the incremental scale factor of the octaveLayerCount pyramid, exact or approximated.
void fd_host_aggregated_limits(int window_w, int window_h, int cell_size, int octave_layer_count, int min_window_width, int width, int height,
                               double& minScale, double& maxScale) {
    const int patchWpx = window_w * cell_size, patchHpx = window_h * cell_size;
    const double inc = std::pow(0.5, 1. / octave_layer_count);
    maxScale = 1.0;
    if (min_window_width > patchWpx) {
        const double m = (double)patchWpx / min_window_width;
        const int minLayerIndex = (int)std::ceil(std::log(m) / std::log(inc));
        maxScale = std::pow(inc, minLayerIndex);
    }
    const double aspectRatio = (double)patchHpx / (double)patchWpx, imageAspectRatio = (double)height / (double)width;
    const int maxWidth = aspectRatio > imageAspectRatio ? (int)(height / aspectRatio) : width;
    const double m = (double)patchWpx / maxWidth;
    const int maxLayerIndex = (int)(std::log(m) / std::log(inc));
    minScale = std::pow(inc, maxLayerIndex);
}

// Layers of ImagePyramid::createApproximated(octaveLayerCount, min, max) (ImagePyramid.cpp:51-63): the source pyramid has one
// layer per octave (createLayers(const Mat&), :170-198: scale 1, then pyrDown while scale *= 0.5 stays >= min), FHOG turns each
// kept one into an exact feature layer, and createLayers(const ImagePyramid&) (:200-235) emits every exact layer followed by its
// approximations.  Whether a layer exists is decided by the double rounding of these very expressions (libm pow, repeated
// *= 0.5, exact.scale * pow(inc, i)), so none of them is rewritten.
void fd_host_plan_aggregated(int cell_size, int octave_layer_count, double minScale, double maxScale, int width, int height,
                             FdAggregatedPlan& plan) {
    plan.minScale = minScale;
    plan.maxScale = maxScale;
    plan.layers.clear();
    plan.exactPx.clear();
    const int n = octave_layer_count;
    const double inc = std::pow(0.5, 1. / n);
    struct Src { int index; double scale; int w, h; };
    std::vector<Src> src;
    {
        double scaleFactor = 1.0;   // pow(incrementalScaleFactor, 0) of the one-layer pyramid
        int pw = fd_cvRound(width * scaleFactor), ph = fd_cvRound(height * scaleFactor);
        if (scaleFactor <= maxScale && scaleFactor >= minScale) src.push_back(Src{0, scaleFactor, pw, ph});
        scaleFactor *= 0.5;
        for (int j = 1; scaleFactor >= minScale && pw > 1; ++j, scaleFactor *= 0.5) {
            pw = (pw + 1) / 2;
            ph = (ph + 1) / 2;
            if (scaleFactor <= maxScale) src.push_back(Src{j, scaleFactor, pw, ph});
        }
    }
    for (const Src& s : src) {
        if (s.scale < minScale) break;
        fd_aggregated_layer e;
        std::memset(&e, 0, sizeof(e));
        e.index = s.index * n;
        e.parent = -1;
        e.rows = s.h / cell_size;
        e.cols = s.w / cell_size;
        e.scale = s.scale;
        e.scale_x = (double)s.w / (double)width;     // ImagePyramid.cpp:178-179,187-188
        e.scale_y = (double)s.h / (double)height;
        const int parent = (int)plan.layers.size();
        if (s.scale <= maxScale) {
            plan.layers.push_back(e);
            plan.exactPx.emplace_back(s.w, s.h);
        }
        for (int i = 1; i < n; ++i) {
            const double scaleFactor = std::pow(inc, i);
            const double overallScale = e.scale * scaleFactor;
            if (overallScale >= minScale && overallScale <= maxScale) {
                fd_aggregated_layer a;
                std::memset(&a, 0, sizeof(a));
                a.index = e.index + i;
                a.approximated = 1;
                a.parent = parent;
                a.cols = fd_cvRound(e.cols * scaleFactor);   // ImagePyramid::resize :278
                a.rows = fd_cvRound(e.rows * scaleFactor);
                a.scale = overallScale;
                a.scale_x = e.scale_x * scaleFactor;
                a.scale_y = e.scale_y * scaleFactor;
                plan.layers.push_back(a);
            }
        }
    }
}

extern "C" int fd_aggregated_plan_layers(int window_w, int window_h, int cell_size, int octave_layer_count, int min_window_width, int width,
                                         int height, fd_aggregated_layer* out, int cap, int* n) {
    if (!n || window_w < 1 || window_h < 1 || cell_size < 1 || octave_layer_count < 1 || width < 1 || height < 1 || cap < 0 || (cap > 0 && !out))
        return FD_ERR_INVALID_ARGUMENT;
    double minScale, maxScale;
    fd_host_aggregated_limits(window_w, window_h, cell_size, octave_layer_count, min_window_width, width, height, minScale, maxScale);
    FdAggregatedPlan plan;
    fd_host_plan_aggregated(cell_size, octave_layer_count, minScale, maxScale, width, height, plan);
    *n = (int)plan.layers.size();
    if (plan.exactPx.size() < 2) return FD_ERR_RUNTIME;   // ImagePyramid::estimateLambdas (ImagePyramid.cpp:238-239)
    if (*n > cap) return FD_ERR_CAPACITY;
    for (int i = 0; i < *n; ++i) out[i] = plan.layers[i];
    return FD_OK;
}

// ---- HaarFeatureFilter's feature table (HaarFeatureFilter.cpp:41-136), host only ---------------------------------------------------
// Everything is float arithmetic written as the reference writes it (this file is built with -ffp-contract=off): 0.5f * base.width,
// base.width / 3 (a float division), base.x + 2 * base.width / 3, 255 * 2.f / 3.
static bool haar_params_ok(const fd_haar_params* hp) {
    if (!hp || hp->num_sizes < 0 || hp->num_xs < 0 || hp->num_ys < 0 || (hp->types & ~FD_HAAR_ALL)) return false;
    return (hp->num_sizes == 0 || hp->sizes) && (hp->num_xs == 0 || hp->xs) && (hp->num_ys == 0 || hp->ys);
}

bool fd_host_haar_features(const fd_haar_params* hp, std::vector<fd_haar_feature>& features) {
    features.clear();
    if (!haar_params_ok(hp)) return false;
    const int types = hp->types;
    fd_haar_feature feature;
    std::memset(&feature, 0, sizeof(feature));
    auto rect = [&](int j, float x, float y, float w, float h, float weight) {
        feature.rects[j][0] = x; feature.rects[j][1] = y; feature.rects[j][2] = w; feature.rects[j][3] = h;
        feature.weights[j] = weight;
    };
    auto push = [&](int n, float factor) {
        feature.num_rects = n;
        feature.factor = factor;
        for (int j = n; j < 4; ++j) rect(j, 0.f, 0.f, 0.f, 0.f, 0.f);
        features.push_back(feature);
    };
    for (int si = 0; si < hp->num_sizes; ++si) {
        const float size = hp->sizes[si];
        for (int yi = 0; yi < hp->num_ys; ++yi) {
            const float y = hp->ys[yi];
            for (int xi = 0; xi < hp->num_xs; ++xi) {
                const float x = hp->xs[xi];
                struct { float x, y, width, height; } base = {x - size / 2, y - size / 2, size, size};
                if (base.x < 0.f || base.x + base.width > 1.f || base.y < 0.f || base.y + base.height > 1.f) continue;
                feature.area = base.width * base.height;
                if (types & FD_HAAR_2RECTANGLE) {
                    rect(0, base.x, base.y, 0.5f * base.width, base.height, 1.f);
                    rect(1, base.x + 0.5f * base.width, base.y, 0.5f * base.width, base.height, -1.f);
                    push(2, 255 * 1.f / 2);
                    rect(0, base.x, base.y, base.width, 0.5f * base.height, 1.f);
                    rect(1, base.x, base.y + 0.5f * base.height, base.width, 0.5f * base.height, -1.f);
                    push(2, 255 * 1.f / 2);
                }
                if (types & FD_HAAR_3RECTANGLE) {
                    rect(0, base.x, base.y, base.width / 3, base.height, 1.f);
                    rect(1, base.x + base.width / 3, base.y, base.width / 3, base.height, -2.f);
                    rect(2, base.x + 2 * base.width / 3, base.y, base.width / 3, base.height, 1.f);
                    push(3, 255 * 2.f / 3);
                    rect(0, base.x, base.y, base.width, base.height / 3, 1.f);
                    rect(1, base.x, base.y + base.height / 3, base.width, base.height / 3, -2.f);
                    rect(2, base.x, base.y + 2 * base.height / 3, base.width, base.height / 3, 1.f);
                    push(3, 255 * 2.f / 3);
                }
                if (types & FD_HAAR_4RECTANGLE) {
                    rect(0, base.x, base.y, base.width / 2, base.height / 2, 1.f);
                    rect(1, base.x + base.width / 2, base.y + base.height / 2, base.width / 2, base.height / 2, 1.f);
                    rect(2, base.x + base.width / 2, base.y, base.width / 2, base.height / 2, -1.f);
                    rect(3, base.x, base.y + base.height / 2, base.width / 2, base.height / 2, -1.f);
                    push(4, 255 * 1.f / 2);
                }
                if (types & FD_HAAR_CENTER_SURROUND) {
                    rect(0, base.x, base.y, base.width, base.height, 1.f);
                    rect(1, base.x + base.width / 4, base.y + base.height / 4, base.width / 2, base.height / 2, -4.f);
                    push(2, 255 * 3.f / 4);
                }
            }
        }
    }
    // every rectangle edge inside [0, 1] (and finite): what bounds the reads of HaarFeatureFilter::applyTo to the patch plus one row / column
    for (const fd_haar_feature& f : features)
        for (int j = 0; j < f.num_rects; ++j) {
            const float e[4] = {f.rects[j][0], f.rects[j][0] + f.rects[j][2], f.rects[j][1], f.rects[j][1] + f.rects[j][3]};
            for (float v : e)
                if (!(v >= 0.f && v <= 1.f)) return false;
        }
    return true;
}

extern "C" int fd_haar_grid(int count, float* coords) {
    if (count < 0 || (count > 0 && !coords)) return FD_ERR_INVALID_ARGUMENT;
    const float step = 1.f / (float)((unsigned int)count + 1);
    for (unsigned int i = 0; i < (unsigned int)count; ++i) coords[i] = (float)(i + 1) * step;
    return FD_OK;
}

extern "C" int fd_haar_feature_count(const fd_haar_params* hp) {
    std::vector<fd_haar_feature> features;
    return fd_host_haar_features(hp, features) ? (int)features.size() : -1;
}

extern "C" int fd_haar_features(const fd_haar_params* hp, fd_haar_feature* out, int cap, int* count) {
    std::vector<fd_haar_feature> features;
    if (!count || cap < 0 || (cap > 0 && !out) || !fd_host_haar_features(hp, features)) return FD_ERR_INVALID_ARGUMENT;
    *count = (int)features.size();
    if (*count > cap) return FD_ERR_CAPACITY;
    for (int i = 0; i < *count; ++i) out[i] = features[i];
    return FD_OK;
}

// ---- argument rules of the integral-image calls (integral.hip), host only: the length of one output, or -1 where the call is an error ----
// Written with divisions, not products, so that no argument can overflow the rule itself.
extern "C" int fd_integral_image_length(int width, int height) {
    if (width < 1 || height < 1) return -1;
    if (width > (2147483647 / 255) / height) return -1;   // 255 * width * height > 2^31 - 1 (integer: the same as width * height > 8421504)
    return (width + 1) * (height + 1);
}

extern "C" int fd_integral_gradient_length(int rows, int cols) {
    if (rows < 2 || cols < 2 || rows > FD_GRADIENT_MAX_GRID || cols > FD_GRADIENT_MAX_GRID) return -1;
    return 2 * rows * cols;
}

extern "C" int fd_gradient_sum_length(int rows, int cols, int cell_rows, int cell_cols) {
    if (rows < 1 || cols < 1 || cell_rows < 1 || cell_cols < 1 || rows > FD_GRADIENT_MAX_GRID || cols > FD_GRADIENT_MAX_GRID) return -1;
    if (rows % cell_rows != 0 || cols % cell_cols != 0) return -1;
    return 4 * cell_rows * cell_cols;
}

// LDS of one workgroup (four wavefronts) of the fused SURF kernel: per wavefront the gradient patch, G * G uchar2 padded to 16 bytes,
// and the unnormalised descriptor, 4 C C floats
size_t fd_host_surf_lds_bytes(int gradient_count, int cell_count) {
    const size_t grad = ((size_t)gradient_count * gradient_count * 2 + 15) & ~(size_t)15;
    return 4 * (grad + sizeof(float) * 4 * (size_t)cell_count * cell_count);
}

extern "C" int fd_surf_feature_length(int gradient_count, int cell_count) {
    if (gradient_count < 2 || gradient_count > FD_SURF_MAX_GRID || cell_count < 1 || gradient_count % cell_count != 0) return -1;
    if (fd_host_surf_lds_bytes(gradient_count, cell_count) > FD_SURF_LDS_BUDGET) return -1;
    return 4 * cell_count * cell_count;
}

// ---- the wrapper chain of a feature extractor: checked and copied for a call; applied to a list of samples on the host (the device
// applies it in fd_particle_sample) ----
FdSampleMaps fd_sample_maps_checked(const fd_sample_map* maps, int n_maps, unsigned allowedKindsMask, const char* who) {
    if (n_maps < 0 || (n_maps > 0 && !maps)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
    if (n_maps > FD_SAMPLE_MAPS_MAX) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %d sample maps, at most %d", who, n_maps, FD_SAMPLE_MAPS_MAX);
    FdSampleMaps chain;
    std::memset(&chain, 0, sizeof(chain));
    chain.n = n_maps;
    for (int k = 0; k < n_maps; ++k) {
        const int32_t kind = maps[k].kind;
        if (kind < 0 || kind > 31 || !((allowedKindsMask >> kind) & 1u)) {
            if (allowedKindsMask == 1u << FD_SAMPLE_MAP_RESIZE)
                FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: sample map kind %d; a pyramid chain takes FD_SAMPLE_MAP_RESIZE only", who, kind);
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown sample map kind %d", who, kind);
        }
        chain.m[k] = maps[k];
    }
    return chain;
}
extern "C" int fd_sample_maps_apply(const fd_sample_map* maps, int n_maps, int n, int32_t* xywh) {
    if (n < 0 || (n > 0 && !xywh)) return FD_ERR_INVALID_ARGUMENT;
    FdSampleMaps chain;
    try {
        chain = fd_sample_maps_checked(maps, n_maps, 1u << FD_SAMPLE_MAP_RESIZE | 1u << FD_SAMPLE_MAP_INTEGRAL, "fd_sample_maps_apply");
    } catch (const FdError& e) {
        return e.code;
    }
    for (int i = 0; i < n; ++i) {
        int32_t* s = xywh + 4 * (size_t)i;
        for (int k = 0; k < chain.n; ++k) fd_sample_map_apply(chain.m[k], s[0], s[1], s[2], s[3]);
    }
    return FD_OK;
}

// ---- the box of the additional negatives on the host: fd_negative_bounds, the function k_particles_negatives itself calls ----
extern "C" int fd_particles_negatives_bounds(const fd_particles_negatives_params* params, int32_t x, int32_t y, int32_t size, int32_t bounds[6]) {
    if (!params || !bounds) return FD_ERR_INVALID_ARGUMENT;
    const FdNegativeBounds b = fd_negative_bounds(params->offset_factor, params->down_scale, params->up_scale, x, y, size);
    bounds[0] = b.xLow; bounds[1] = b.xHigh; bounds[2] = b.yLow; bounds[3] = b.yHigh; bounds[4] = b.sizeLow; bounds[5] = b.sizeHigh;
    return FD_OK;
}

// ---- the examples of SelfLearningMeasurementModel::adapt on the host (SelfLearningMeasurementModel.cpp:89-125): the candidates in
// index order, sorted only when there are more than max_count, by fd_example_candidate / fd_example_before, the comparisons
// k_particles_examples runs ----
extern "C" int fd_particles_examples_select(int n, const double* weight, const uint8_t* valid, const fd_particles_examples_params* params, int* n_pos,
                                            int32_t* pos_index, int* n_neg, int32_t* neg_index) {
    if (n_pos) *n_pos = 0;
    if (n_neg) *n_neg = 0;
    if (n < 0 || !params || !n_pos || !pos_index || !n_neg || !neg_index || (n > 0 && !weight)) return FD_ERR_INVALID_ARGUMENT;
    if (params->max_count < 1 || params->max_count > FD_PARTICLES_EXAMPLES_MAX || !std::isfinite(params->positive_threshold) ||
        !std::isfinite(params->negative_threshold) || params->negative_threshold > params->positive_threshold || (params->require_window != 0 && params->require_window != 1) || (params->require_window && n > 0 && !valid))
        return FD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
        if (!(weight[i] >= 0.0 && weight[i] <= DBL_MAX)) return FD_ERR_RUNTIME;
    const size_t K = (size_t)params->max_count;
    auto side = [&](bool positive, double threshold, int32_t* out) {
        std::vector<int32_t> chosen;
        for (int i = 0; i < n; ++i)
            if (fd_example_candidate(positive, weight[i], threshold) && (!params->require_window || valid[i])) chosen.push_back(i);
        if (chosen.size() > K) {
            std::sort(chosen.begin(), chosen.end(), [&](int32_t a, int32_t b) { return fd_example_before(positive, weight[a], a, weight[b], b); });
            chosen.resize(K);
        }
        std::copy(chosen.begin(), chosen.end(), out);
        return (int)chosen.size();
    };
    *n_pos = side(true, params->positive_threshold, pos_index);
    *n_neg = side(false, params->negative_threshold, neg_index);
    return FD_OK;
}

extern "C" int fd_particles_examples_bounds(int family, int kind, const void* params, int channels, int max_count, int* row_length, int* row_capacity) {
    if (!params || !row_length || !row_capacity || max_count < 1 || max_count > FD_PARTICLES_EXAMPLES_MAX) return FD_ERR_INVALID_ARGUMENT;
    int len = -1;
    if (family == FD_EXAMPLES_INTEGRAL) {
        if (kind == FD_INTEGRAL_HAAR) len = fd_haar_feature_count((const fd_haar_params*)params);
        else if (kind == FD_INTEGRAL_SURF) len = fd_surf_feature_length(((const fd_surf_params*)params)->gradient_count, ((const fd_surf_params*)params)->cell_count);
        else if (kind == FD_INTEGRAL_HOG) len = fd_integral_hog_feature_length((const fd_integral_hog_params*)params);
    } else if (family == FD_EXAMPLES_PYRAMID) {
        if (kind == FD_SAMPLES_HIST) len = fd_hist_feature_length((const fd_hist_params*)params, channels);
        else if (kind == FD_SAMPLES_EHOG) len = fd_ehog_feature_length((const fd_ehog_patch_params*)params, channels);
        else if (kind == FD_SAMPLES_PATCH) len = fd_patch_feature_length((const fd_patch_samples_params*)params);
    }
    if (len < 0 || (long long)len * 2 * max_count > INT32_MAX) return FD_ERR_INVALID_ARGUMENT;
    *row_length = len;
    *row_capacity = len * 2 * max_count;
    return FD_OK;
}

// ---- part (a) of the sample -> window rule as a table for the device (k_particles_windows): fd_sample_layer_position, the function
// fd_sample_window itself calls, evaluated once per width ----
extern "C" int fd_sample_layer_table(int n_layers, int first_index, double incremental_scale, int patch_w, int cap, int16_t* layer_of_width, int* length) {
    if (n_layers < 0 || n_layers > INT16_MAX || patch_w < 1 || !(incremental_scale > 0 && incremental_scale < 1) || cap < 0 || !length ||
        (cap > 0 && !layer_of_width))
        return FD_ERR_INVALID_ARGUMENT;
    auto position = [&](int width) { return fd_sample_layer_position(first_index, incremental_scale, patch_w, width); };
    // The largest width that maps to a kept layer.  The position does not decrease with the width: patch_w / width of neighbouring
    // widths differs by 2^-31 of its value or more, log's error stays below 2^-52 of its value.  So the widths whose position lies below
    // n_layers are the ones up to some width, which a bisection with the function itself finds; that width maps to a kept layer, or none does.
    int last = 0;
    if (n_layers > 0 && position(1) < (long)n_layers) {
        int lo = 1, hi = INT32_MAX;
        while (lo < hi) {
            const int mid = lo + (int)(((int64_t)hi - lo + 1) / 2);
            if (position(mid) < (long)n_layers) lo = mid;
            else hi = mid - 1;
        }
        if (position(lo) >= 0) last = lo;
    }
    *length = last == INT32_MAX ? INT32_MAX : (last > 0 ? last + 1 : 0);
    if (*length > cap) return FD_ERR_CAPACITY;
    for (int w = 0; w < *length; ++w) {
        const long pos = w > 0 ? position(w) : -1;
        layer_of_width[w] = pos >= 0 && pos < (long)n_layers ? (int16_t)pos : (int16_t)-1;
    }
    return FD_OK;
}

// ---- OpticalFlowTransitionModel's host arithmetic; the tracking itself is optflow.hip ----

// OpticalFlowTransitionModel.cpp:63-75, operation for operation: gridPoint's first value is formed in double (0.5 * gridX is a double
// product) and stored as float, the value a row starts from afterwards in float
extern "C" int fd_flow_grid(int grid_w, int grid_h, int circle, float* out_xy, int cap, int* n) {
    if (grid_w < 1 || grid_h < 1 || grid_w > 1024 || grid_h > 1024 || cap < 0 || !n || (cap > 0 && !out_xy)) return FD_ERR_INVALID_ARGUMENT;
    const float gridY = 1.f / static_cast<float>(grid_h + 2);
    const float gridX = 1.f / static_cast<float>(grid_w + 2);
    const float r = 0.5f - 0.5f * (gridX + gridY);
    float px = (float)(-0.5f + 0.5 * gridX + gridX), py = (float)(-0.5f + 0.5 * gridY + gridY);
    int count = 0;
    for (int y = 0; y < grid_h; ++y) {
        for (int x = 0; x < grid_w; ++x) {
            if (!circle || px * px + py * py < r * r) {
                if (count < cap) { out_xy[2 * count] = px; out_xy[2 * count + 1] = py; }
                ++count;
            }
            px += gridX;
        }
        px = -0.5f + gridX / 2 + gridX;
        py += gridY;
    }
    *n = count;
    return count > cap ? FD_ERR_CAPACITY : FD_OK;
}

// OpticalFlowTransitionModel.cpp:114-170.  Not the reference's: pairs are ordered by (distance, index) -- its std::sort on the distance
// alone leaves ties to the implementation; a pair whose distance is NaN counts as not tracked; with fewer than two correct pairs there
// is no ratio to take a median of (the reference indexes an empty vector) and the result is not ok; a NaN ratio (two points that
// coincide) sorts behind every number.
extern "C" int fd_flow_median(const float* points, const float* fwd, const float* bwd, const uint8_t* fstatus, const uint8_t* bstatus, int n,
                              fd_flow_motion* out) {
    if (!out || n < 0 || (n > 0 && (!points || !fwd || !bwd || !fstatus || !bstatus))) return FD_ERR_INVALID_ARGUMENT;
    out->ok = 0;
    out->n_valid = out->n_correct = 0;
    out->median_x = out->median_y = 0.f;
    out->median_ratio = 1.f;
    struct Pair { float d; int i; };
    std::vector<Pair> pairs;
    pairs.reserve(n);
    for (int i = 0; i < n; ++i) {
        if (!fstatus[i] || !bstatus[i]) continue;
        const float dx = bwd[2 * i] - points[2 * i], dy = bwd[2 * i + 1] - points[2 * i + 1];
        const float d = dx * dx + dy * dy;
        if (d == d) pairs.push_back(Pair{d, i});
    }
    std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.d < b.d || (a.d == b.d && a.i < b.i); });
    out->n_valid = (int)pairs.size();
    if (out->order)
        for (size_t k = 0; k < pairs.size(); ++k) out->order[k] = pairs[k].i;
    const size_t half = (size_t)n / 2;
    if (pairs.size() < half) return FD_OK;
    const float maxError = 1 * 0.5f;
    size_t correct = 0;
    while (correct < pairs.size() && !(pairs[correct].d > maxError)) ++correct;
    out->n_correct = (int)correct;
    if (correct < half || correct < 2) return FD_OK;
    std::vector<float> xs(correct), ys(correct);
    for (size_t k = 0; k < correct; ++k) {
        const int i = pairs[k].i;
        xs[k] = fwd[2 * i] - points[2 * i];
        ys[k] = fwd[2 * i + 1] - points[2 * i + 1];
    }
    auto nanLast = [](float a, float b) { return a < b || (a == a && b != b); };
    std::sort(xs.begin(), xs.end(), nanLast);
    std::sort(ys.begin(), ys.end(), nanLast);
    out->median_x = xs[correct / 2];
    out->median_y = ys[correct / 2];
    std::vector<float> ratios;
    ratios.reserve(correct * (correct - 1) / 2);
    for (size_t a = 0; a < correct; ++a) {
        const int i = pairs[a].i;
        for (size_t b = a + 1; b < correct; ++b) {
            const int j = pairs[b].i;
            const float bx = points[2 * i] - points[2 * j], by = points[2 * i + 1] - points[2 * j + 1];
            const float ax = fwd[2 * i] - fwd[2 * j], ay = fwd[2 * i + 1] - fwd[2 * j + 1];
            ratios.push_back((ax * ax + ay * ay) / (bx * bx + by * by));
        }
    }
    std::nth_element(ratios.begin(), ratios.begin() + ratios.size() / 2, ratios.end(), nanLast);   // the element a full sort puts there
    out->median_ratio = std::sqrt(ratios[ratios.size() / 2]);
    out->ok = 1;
    return FD_OK;
}
