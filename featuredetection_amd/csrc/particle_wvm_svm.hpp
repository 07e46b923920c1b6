// featuredetection_amd/csrc/particle_wvm_svm.hpp -- condensation::WvmSvmModel (WvmSvmModel.cpp:69-118) for a resident particle set: the
// rule "the at most 8 most probable WVM positives are re-scored by the SVM" and the model's weighting, on the device.
// Included by condensation.hip only, behind k_particles_weigh, whose logistic (particle_logistic) and reduction
// (particles_publish_best) the weigh kernel here shares.  The cascade in front is wvm.hip's (fd_wvm_list_launch_resident), the SVM
// between the two kernels svm.hip's generic launch on a fixed list of 8 rows.
#pragma once
#include "fd_internal.hpp"

namespace {

constexpr int WVM_SVM_RESCORED = 8;   // WvmSvmModel.cpp:98-99: resize(8)

// what k_particles_wvm_svm_select leaves for the SVM launch and k_particles_wvm_svm_weigh; fd_particles_get_wvm_svm_trace reads it back
struct ParticleWvmSvmSel {
    uint32_t row[WVM_SVM_RESCORED];      // patch rows of the selected positives: the SVM's gather list.  Unused entries name row 0
    double distance[WVM_SVM_RESCORED];   // the SVM's outputs for them
    int32_t index[WVM_SVM_RESCORED];     // their particles, most probable first; unused entries -1
    int32_t count, pad;
};

// the argument of ProbabilisticWvmClassifier's logistic (.cpp:52) and of the SVM's: one product, one sum, each rounded
__device__ inline double wvm_svm_logistic_argument(double a, double b, double x) { return __dadd_rn(a, __dmul_rn(b, x)); }

// ascending t as ascending integers; -0 is +0, a NaN ranks behind every number
__device__ inline unsigned long long wvm_svm_rank(double t) {
    if (t != t) return ~0ull;
    const unsigned long long u = (unsigned long long)__double_as_longlong(t + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// score[i] = (double)fout of window i: what fd_particles_get and the weigh kernel read
__global__ __launch_bounds__(256) void k_particles_fout_scores(const float* __restrict__ fout, int n, double* __restrict__ score) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) score[i] = (double)fout[i];
}

// The selection.  Candidates: the positive records whose particle is valid (the spare window of an invalid particle can be a positive).
// Key: t = logisticA + logisticB * fout; p_wvm = 1 / (1 + exp(t)) falls as t rises, so the most probable have the smallest t.  The up to
// 8 smallest (t, particle index) are found one per round: every thread walks its records for the smallest pair behind the last one
// selected, the workgroup reduces.  posCount NULL: no cascade ran (no layer holds a window), nothing is selected.
__global__ __launch_bounds__(PT) void k_particles_wvm_svm_select(const uint4* __restrict__ pos, const unsigned int* __restrict__ posCount, int n,
                                                                 const uint8_t* __restrict__ valid, double logisticA, double logisticB,
                                                                 ParticleWvmSvmSel* __restrict__ sel) {
    __shared__ unsigned long long sRank[PT];
    __shared__ uint32_t sIdx[PT], sRow[PT];
    constexpr uint32_t NONE = 0xffffffffu;
    const int tid = threadIdx.x;
    const unsigned int cnt = posCount ? min(*posCount, (unsigned int)n) : 0u;
    unsigned long long lastRank = 0ull;
    uint32_t lastIdx = 0u;
    int count = 0;
    for (int r = 0; r < WVM_SVM_RESCORED; ++r) {
        unsigned long long bestRank = ~0ull;
        uint32_t bestIdx = NONE, bestRow = 0u;
        for (unsigned int c = tid; c < cnt; c += PT) {
            const uint4 rec = pos[c];
            const uint32_t i = rec.x;
            if (rec.y != 0u || i >= (uint32_t)n || !valid[i]) continue;
            const unsigned long long rank = wvm_svm_rank(wvm_svm_logistic_argument(logisticA, logisticB, (double)__uint_as_float(rec.w)));
            if (r > 0 && (rank < lastRank || (rank == lastRank && i <= lastIdx))) continue;   // selected in an earlier round
            if (rank < bestRank || (rank == bestRank && i < bestIdx)) { bestRank = rank; bestIdx = i; bestRow = c; }
        }
        sRank[tid] = bestRank; sIdx[tid] = bestIdx; sRow[tid] = bestRow;
        __syncthreads();
        for (int s = PT / 2; s > 0; s >>= 1) {
            if (tid < s && (sRank[tid + s] < sRank[tid] || (sRank[tid + s] == sRank[tid] && sIdx[tid + s] < sIdx[tid]))) {
                sRank[tid] = sRank[tid + s]; sIdx[tid] = sIdx[tid + s]; sRow[tid] = sRow[tid + s];
            }
            __syncthreads();
        }
        lastRank = sRank[0];
        lastIdx = sIdx[0];
        const uint32_t row = sRow[0];
        __syncthreads();   // the next round overwrites the arrays
        if (lastIdx == NONE) break;   // uniform: no candidate is left
        if (tid == 0) { sel->row[r] = row; sel->index[r] = (int32_t)lastIdx; }
        count = r + 1;
    }
    if (tid == 0) {
        for (int r = count; r < WVM_SVM_RESCORED; ++r) { sel->row[r] = 0u; sel->index[r] = -1; }
        sel->count = count;
    }
}

// WvmSvmModel.cpp:73-111 for every sample: an invalid one gets target 0, weight 0, score 0; a valid one target 0 and weight 0.5 * p_wvm
// (ProbabilisticWvmClassifier.cpp:52 in double, with its float constants); a selected one target = distance >= threshold and weight
// 2 * (0.5 * p_wvm) * p_svm.  Two passes as k_particles_weigh: the first only looks for a weight that is negative or not finite.
__global__ __launch_bounds__(PT) void k_particles_wvm_svm_weigh(ParticleGen g, int n, const uint8_t* __restrict__ valid, double wvmA, double wvmB,
                                                                double svmA, double svmB, double svmThreshold,
                                                                const ParticleWvmSvmSel* __restrict__ sel, fd_particles_info* __restrict__ info) {
    __shared__ int32_t sIndex[WVM_SVM_RESCORED];
    __shared__ double sDistance[WVM_SVM_RESCORED];
    const int tid = threadIdx.x;
    if (tid < WVM_SVM_RESCORED) {
        sIndex[tid] = tid < sel->count ? sel->index[tid] : -1;
        sDistance[tid] = sel->distance[tid];
    }
    __syncthreads();
    auto place = [&](int i) {
        for (int k = 0; k < WVM_SVM_RESCORED; ++k)
            if (sIndex[k] == i) return k;
        return -1;
    };
    auto weighed = [&](int i, int k) {
        const double pWvm = 1.0f / (1.0f + exp(wvm_svm_logistic_argument(wvmA, wvmB, g.score[i])));
        const double w = 0.5 * pWvm;
        return k < 0 ? w : 2 * w * particle_logistic(wvm_svm_logistic_argument(svmA, svmB, sDistance[k]));
    };
    int bad = 0;
    for (int i = tid; i < n; i += PT)
        if (valid[i] && !particle_weight_ok(weighed(i, place(i)))) bad = 1;
    if (__syncthreads_or(bad)) {
        if (tid == 0) info->bad_weight = 1;
        return;
    }
    double best = -DBL_MAX;
    int nValid = 0;
    for (int i = tid; i < n; i += PT) {
        double score = 0.0;
        if (!valid[i]) {
            g.target[i] = 0;
            g.weight[i] = 0.0;
            g.score[i] = 0.0;
        } else {
            const int k = place(i);
            score = g.score[i];
            g.weight[i] = weighed(i, k);
            g.target[i] = k >= 0 && sDistance[k] >= svmThreshold;
            ++nValid;
        }
        if (best < score) best = score;
    }
    particles_publish_best(best, nValid, info);
}

}  // namespace
