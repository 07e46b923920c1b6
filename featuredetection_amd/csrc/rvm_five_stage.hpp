// featuredetection_amd/csrc/rvm_five_stage.hpp -- detection::FiveStageSlidingWindowDetector::detect (FiveStageSlidingWindowDetector.cpp:
// 187-320, :331-380) with a ProbabilisticRvmClassifier as first stage and a ProbabilisticSvmClassifier (f32 support vectors) or a
// ProbabilisticRvmClassifier as second stage ("firstClassifier prvm" of ffpDetectApp's FaceFrontal.cfg).  Included by rvm.hip only, at
// its end.
//
// Stage 1 is fd_detect_rvm's window scan (rvm_scan_*): it leaves every window's u8 feature row in m->feats and the positive records in
// m->pos.  Stage 3 classifies the survivors' own feature vectors, float(u8) * conv_scale + conv_shift, which never leave the device:
// k_rvm_rows_f32 gathers the rows into dense f32 rows and the second classifier's kernels (k_svm_generic / the RVM cascade) run on those.
// Stage 2 (overlap elimination) and stages 4-5 (five_stage_stages.hpp) are host code on ~100 records.
//
// Two orders, same bytes:
//   two waits  cascade | wait | sort, overlap elimination | gather + second stage on the survivors | wait | verdicts, NMS
//   one wait   (SVM second stage) cascade, gather + SVM on ALL positives by record slot, the count read from the cascade's device
//              counter | wait | sort, overlap elimination, the survivors' distances looked up by slot | verdicts, NMS
// A row's distance does not depend on what else is in the launch.  FD_FS_SPEC=0 selects the two-wait order, which is also the path of a
// frame with more positives than RVM_FS_SPEC_CAP and of an RVM second stage.
#pragma once
#include "five_stage_stages.hpp"

namespace {

constexpr int RVM_FS_SPEC_CAP = 4096;   // rows the one-wait order's launches cover

// Rows of the u8 feature matrix feats[total][dim] as dense f32 rows[n][dim], converted with k_rvm_pass<true>'s expression.  One wavefront
// per row.  Row r of the output is the window recs[r] (a positive record of the cascade; the record is copied to recs_out, host memory,
// when given) or wids[r].  dcount (may be NULL): the row count lives on the device, the grid covers n.
// A row starts at byte wid * dim, in general not dword-aligned: the whole dwords inside the row are fetched as dwords (lane == dword,
// coalesced), the up to three bytes in front of the first and behind the last one as bytes; the row is put together in LDS and written
// out lane == element (256 contiguous bytes per store).  dim <= RVM_MAX_DIM^2 is rvm_scan_check's guarantee (the entry points call it before
// any launch).  recs_out and, behind this kernel, the second stage's distances are written by the device straight into pinned host memory,
// as the WVM path's tail does: the host reads them after the stream's wait.
static_assert((RVM_MAX_DIM * RVM_MAX_DIM + 8) % 4 == 0, "k_rvm_rows_f32: every wavefront's LDS slab must start dword-aligned");
__global__ __launch_bounds__(256) void k_rvm_rows_f32(const uint8_t* __restrict__ feats, int dim, float scale, float shift,
                                                      const FdPosRec* __restrict__ recs, const uint32_t* __restrict__ wids,
                                                      const unsigned int* __restrict__ dcount, unsigned int n, float* __restrict__ rows,
                                                      FdPosRec* __restrict__ recs_out) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[4][RVM_MAX_DIM * RVM_MAX_DIM + 8];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const unsigned int row = blockIdx.x * 4u + (unsigned int)wave;
    unsigned int cnt = n;
    if (dcount) cnt = min(*dcount, n);
    if (row >= cnt) return;   // (no workgroup barrier below: the wavefronts of a workgroup are independent)
    uint64_t wid;
    if (recs) {
        const FdPosRec r = recs[row];
        wid = fd_pos_wid(r);
        if (recs_out && lane == 0) recs_out[row] = r;
    } else {
        wid = wids[row];
    }
    const uint64_t b = wid * (uint64_t)dim;
    const uint8_t* base = feats + (b & ~(uint64_t)3);   // feats comes from hipMalloc: dword-aligned
    const int head = (int)(b & 3);
    const int end = head + dim;                         // the row is base[head .. end)
    const int w0 = head ? 1 : 0, w1 = end >> 2;         // its whole dwords: [w0, w1)
    unsigned char* s = stage[wave];
    for (int j = w0 + lane; j < w1; j += 64) reinterpret_cast<uint32_t*>(s)[j] = reinterpret_cast<const uint32_t*>(base)[j];
    {
        const int k = head + lane;                      // bytes in front of the first whole dword
        if (k < min(4 * w0, end)) s[k] = base[k];
        const int kt = 4 * max(w1, w0) + lane;          // bytes behind the last one
        if (lane < 4 && kt < end) s[kt] = base[kt];
    }
    wave_sync();
    float* o = rows + (size_t)row * dim;
    for (int i = lane; i < dim; i += 64) o[i] = (float)s[head + i] * scale + shift;   // cv::Mat::convertTo(CV_32F, scale, shift)
}

void rvm_rows_launch(hipStream_t st, const fd_rvm* m, const fd_rvm_detect_params* dp, const FdPosRec* recs, const uint32_t* wids,
                     const unsigned int* dcount, unsigned int n, float* rows, FdPosRec* recs_out) {
    hipLaunchKernelGGL(k_rvm_rows_f32, dim3((n + 3) / 4), dim3(256), 0, st, m->feats.as<uint8_t>(), m->dev.dim, dp->conv_scale, dp->conv_shift, recs,
                       wids, dcount, n, rows, recs_out);
    HIP_CHECK(hipGetLastError());
}

// everything the entry points refuse, before anything is launched (updated: the pyramid must hold an image already)
void rvm_fs_check(fd_ctx* ctx, const fd_pyramid* p, const fd_rvm* first, const fd_rvm_detect_params* dp, const fd_svm* second_svm,
                  const fd_rvm* second_rvm, const int* count, bool updated, const char* who) {
    if (!ctx || !p || !first || !dp || !count) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    if ((second_svm != nullptr) == (second_rvm != nullptr))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: exactly one second classifier (SVM or RVM) must be given", who);
    const int dim = first->filter_w * first->filter_h;
    if (second_svm) {
        if (fd_svm_is_u8(second_svm)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the second SVM must have f32 support vectors (it classifies the converted patch)", who);
        if (fd_svm_dim(second_svm) != dim) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the second SVM works on %d values, the first stage's patch has %d", who, fd_svm_dim(second_svm), dim);
    } else {
        if (second_rvm == first) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: first and second classifier are the same handle (they share scratch)", who);
        if (second_rvm->filter_w != first->filter_w || second_rvm->filter_h != first->filter_h)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the second RVM's filters are %d x %d, the first's %d x %d", who, second_rvm->filter_w, second_rvm->filter_h,
                     first->filter_w, first->filter_h);
        if (second_rvm->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
    }
    rvm_scan_check(ctx, p, first, dp, who, updated);
}

void rvm_five_stage(fd_ctx* ctx, fd_pyramid* p, fd_rvm* m, const fd_rvm_detect_params* dp, const fd_svm* svm, fd_rvm* second, float oe_dist,
                    float oe_ratio, const int* roi, fd_detection* out, int cap, int* count, int32_t* stage_counts) {
    *count = 0;
    if (stage_counts) stage_counts[0] = stage_counts[1] = stage_counts[2] = stage_counts[3] = 0;
    std::vector<fd_detection> pos2;
    RvmScan sc;
    if (!rvm_scan_windows(ctx, p, m, dp, roi, sc)) {
        five_stage_nms(p, roi, pos2, out, cap, count, stage_counts);
        return;
    }
    hipStream_t st = ctx->stream;
    const int dim = m->dev.dim;
    const int64_t rowBytes = (int64_t)dim * 4;
    // stage 1: the cascade of fd_detect_rvm
    rvm_scan_cascade(ctx, m, dp, sc, false);
    const unsigned int* dcnt = m->counters.as<unsigned int>();   // [0]: positives
    // pinned staging: [count (64 bytes) | records | distances | levels]
    auto layout = [&](size_t n, bool withRecs, size_t& recOff, size_t& distOff, size_t& levelOff) {
        recOff = 64;
        distOff = recOff + (withRecs ? sizeof(FdPosRec) * n : ((sizeof(uint32_t) * n + 15) & ~(size_t)15));
        levelOff = distOff + sizeof(double) * n;
        return levelOff + sizeof(int32_t) * n;
    };
    size_t recOff, distOff, levelOff;
    const bool spec = svm && fd_knob_fs_spec();
    m->h_fs.reserve(layout(spec ? RVM_FS_SPEC_CAP : 0, true, recOff, distOff, levelOff));
    char* hb = m->h_fs.as<char>();
    HIP_CHECK(hipMemcpyAsync(hb, dcnt, 4, hipMemcpyDeviceToHost, st));
    if (spec) {   // the SVM on every positive, by record slot, straight behind the cascade
        m->rows.reserve((size_t)RVM_FS_SPEC_CAP * rowBytes);
        rvm_rows_launch(st, m, dp, m->pos.as<FdPosRec>(), nullptr, dcnt, RVM_FS_SPEC_CAP, m->rows.as<float>(), reinterpret_cast<FdPosRec*>(hb + recOff));
        fd_svm_f32_launch_counted(st, svm, m->rows.p, rowBytes, RVM_FS_SPEC_CAP, dcnt, reinterpret_cast<double*>(hb + distOff));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    const unsigned int cnt = *reinterpret_cast<const unsigned int*>(hb);
    if (cnt > sc.pos_cap) FD_THROW(FD_ERR_DEVICE_CAPACITY, "five-stage (RVM): %u positives exceed the device buffer", cnt);
    const bool scored = spec && cnt <= (unsigned int)RVM_FS_SPEC_CAP;
    std::vector<FdPosRec> raw(cnt);
    if (scored) std::memcpy(raw.data(), hb + recOff, sizeof(FdPosRec) * cnt);
    else if (cnt) HIP_CHECK(hipMemcpy(raw.data(), m->pos.p, sizeof(FdPosRec) * cnt, hipMemcpyDeviceToHost));
    std::vector<uint32_t> order(cnt);   // record slots in window order, as fd_detect_rvm returns its positives
    for (unsigned int i = 0; i < cnt; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return fd_pos_before(raw[a], raw[b]); });
    std::vector<fd_detection> dets(cnt);
    for (unsigned int i = 0; i < cnt; ++i) dets[i] = rvm_detection(p, m, sc.wls, dp, raw[order[i]]);
    if (stage_counts) stage_counts[0] = (int)cnt;
    // stage 2: overlap elimination
    std::vector<int> keep;
    fd_host_overlap_elimination(dets.data(), (int)cnt, oe_dist, oe_ratio, keep);
    if (stage_counts) stage_counts[1] = (int)keep.size();
    // stage 3: the second classifier on the survivors' feature vectors
    const size_t n = keep.size();
    if (scored) {
        const double thr = (double)fd_svm_threshold(svm);
        const double* dist = reinterpret_cast<const double*>(hb + distOff);
        for (size_t i = 0; i < n; ++i) {
            const double dv = dist[order[(size_t)keep[i]]];
            if (dv >= thr) five_stage_accept(dets[(size_t)keep[i]], dv, pos2);
        }
    } else if (n) {
        if (sc.total > (int64_t)0xffffffffu) FD_THROW(FD_ERR_INVALID_ARGUMENT, "five-stage (RVM): too many windows (%lld)", (long long)sc.total);
        m->h_fs.reserve(layout(n, false, recOff, distOff, levelOff));
        hb = m->h_fs.as<char>();
        uint32_t* wids = reinterpret_cast<uint32_t*>(hb + recOff);
        for (size_t i = 0; i < n; ++i) wids[i] = (uint32_t)fd_pos_wid(raw[order[(size_t)keep[i]]]);
        m->rows.reserve(n * (size_t)rowBytes);
        rvm_rows_launch(st, m, dp, nullptr, wids, nullptr, (unsigned int)n, m->rows.as<float>(), nullptr);
        const double* dist = reinterpret_cast<const double*>(hb + distOff);
        const int32_t* level = reinterpret_cast<const int32_t*>(hb + levelOff);
        if (svm) {
            fd_svm_generic_launch_on(st, svm, m->rows.p, nullptr, rowBytes, (int64_t)n, reinterpret_cast<double*>(hb + distOff));
        } else {
            run_cascade<false>(ctx, second, m->rows.p, rowBytes, 1.f, 0.f, (int64_t)n, true, 0u);
            HIP_CHECK(hipMemcpyAsync(hb + distOff, second->dist.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(hb + levelOff, second->level.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        const int last = svm ? 0 : second->dev.numUse - 1;
        const double thr = svm ? (double)fd_svm_threshold(svm) : (double)second->h_thr[(size_t)last];
        for (size_t i = 0; i < n; ++i) {
            const bool passes = svm ? dist[i] >= thr : (level[i] == last && dist[i] >= thr);   // RvmClassifier.cpp:68-73
            if (passes) five_stage_accept(dets[(size_t)keep[i]], dist[i], pos2);
        }
    }
    // stages 4-5
    five_stage_nms(p, roi, pos2, out, cap, count, stage_counts);
}

}  // namespace

extern "C" {

int fd_detect_five_stage_rvm(fd_ctx* ctx, fd_pyramid* p, const fd_rvm* first, const fd_rvm_detect_params* dp, const fd_svm* second_svm,
                             const fd_rvm* second_rvm, float oe_dist, float oe_ratio, const int* roi, fd_detection* out, int cap, int* count,
                             int32_t* stage_counts) {
    return fd_guard(ctx, [&] {
        rvm_fs_check(ctx, p, first, dp, second_svm, second_rvm, count, true, "fd_detect_five_stage_rvm");
        rvm_five_stage(ctx, p, const_cast<fd_rvm*>(first), dp, second_svm, const_cast<fd_rvm*>(second_rvm), oe_dist, oe_ratio, roi, out, cap, count,
                       stage_counts);
    });
}

// Detector::detect(const Mat& image): the pyramid update (with the pyramid's image filter) and the detection of one frame in one call
int fd_detect_five_stage_rvm_image(fd_ctx* ctx, fd_pyramid* p, const fd_rvm* first, const fd_rvm_detect_params* dp, const fd_svm* second_svm,
                                   const fd_rvm* second_rvm, const uint8_t* image, int width, int height, int channels, int image_is_device,
                                   float oe_dist, float oe_ratio, const int* roi, fd_detection* out, int cap, int* count, int32_t* stage_counts) {
    return fd_guard(ctx, [&] {
        if (!image) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_detect_five_stage_rvm_image: NULL argument");
        rvm_fs_check(ctx, p, first, dp, second_svm, second_rvm, count, false, "fd_detect_five_stage_rvm_image");
        HIP_CHECK(hipSetDevice(ctx->device));
        fd_pyramid_update_on(p, image, width, height, channels, image_is_device, ctx->stream);
        rvm_five_stage(ctx, p, const_cast<fd_rvm*>(first), dp, second_svm, const_cast<fd_rvm*>(second_rvm), oe_dist, oe_ratio, roi, out, cap, count,
                       stage_counts);
    });
}

}  // extern "C"
