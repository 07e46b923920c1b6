// featuredetection_amd/csrc/five_stage_stages.hpp -- the stages of detection::FiveStageSlidingWindowDetector::detect that do not depend on
// the first classifier: stage 3's verdict on one survivor and stages 4-5.  Host code only; included by five_stage.hpp (WVM first stage,
// wvm.hip) and rvm_five_stage.hpp (RVM first stage, rvm.hip).
#pragma once
#include "fd_internal.hpp"
#include <algorithm>
#include <vector>

// Stages 4-5 of FiveStageSlidingWindowDetector::detect on the SVM positives of one image (FiveStageSlidingWindowDetector.cpp:
// 262-320; the roi variant :360-380 only sorts): block NMS on the probability map, one detection per maximum, sorted by probability.
static void five_stage_nms(const fd_pyramid* p, const int* roi, std::vector<fd_detection>& svmPos, fd_detection* out, int cap, int* count,
                           int32_t* stage_counts) {
    if (stage_counts) stage_counts[2] = (int)svmPos.size();
    auto byProb = [](const fd_detection& a, const fd_detection& b) { return a.probability > b.probability; };
    bool sortAtEnd = true;
    if (!roi) {
        std::vector<int> maxima;
        fd_host_block_nms_sparse(svmPos, p->img_w, p->img_h, 35, true, maxima);
        if (maxima.empty()) fd_host_block_nms_sparse(svmPos, p->img_w, p->img_h, 35, false, maxima);
        if (maxima.empty()) {
            sortAtEnd = false;  // "return svmPatchesPositive; // Should be empty." (:292-294), unsorted
        } else {
            std::sort(svmPos.begin(), svmPos.end(), byProb);
            std::vector<fd_detection> res;
            for (size_t i = 0; i + 1 < maxima.size(); i += 2) {
                const int x = maxima[i], y = maxima[i + 1];
                auto it = std::find_if(svmPos.begin(), svmPos.end(), [&](const fd_detection& a) { return a.cx == x && a.cy == y; });
                if (it != svmPos.end()) res.push_back(*it);
            }
            svmPos.swap(res);
        }
    }
    if (sortAtEnd) std::sort(svmPos.begin(), svmPos.end(), byProb);
    if (stage_counts) stage_counts[3] = (int)svmPos.size();
    *count = (int)svmPos.size();
    for (size_t i = 0; i < svmPos.size() && (int)i < cap && out; ++i) out[i] = svmPos[i];
    if (out && (int)svmPos.size() > cap) FD_THROW(FD_ERR_CAPACITY, "five-stage: %zu detections, capacity %d", svmPos.size(), cap);
}

// Stage 3's verdict on one survivor: strongClassifier->classify() gives a bool only, so a survivor at or above the SVM's threshold becomes
// an SVM positive with the distance as its score and ClassifiedPatch(patch, bool)'s default probability (ClassifiedPatch.hpp:29-30).
static inline void five_stage_accept(const fd_detection& survivor, double dist, std::vector<fd_detection>& svmPos) {
    fd_detection d = survivor;
    d.score = (float)dist;
    d.positive = 1;
    d.probability = 0.5;
    svmPos.push_back(d);
}
