// featuredetection_amd/csrc/particle_examples.hpp -- the examples of condensation::SelfLearningMeasurementModel::adapt
// (SelfLearningMeasurementModel.cpp:89-125) for a resident particle set: out of the generation the up to K samples above a positive
// threshold and the up to K below a negative one, chosen in one workgroup behind k_particles_state, so that a frame of the
// self-learning tracker hands its adaptation the few samples it reads, and their feature rows, in the frame's one read-back and never
// downloads the generation.  Included by condensation.hip only, behind particle_negatives.hpp, whose radix selection
// (negatives_select) it reuses.  The comparisons are fd_example_candidate / fd_example_before (fd_internal.hpp), the copy the host's
// fd_particles_examples_select uses.
//
// The reference collects a side's candidates in index order and, only when there are more than K of them, sorts them (positives by
// weight descending, negatives ascending) and keeps the first K.  Its std::sort is unstable; here equal weights keep the lower index
// first.  So a side is: at most K candidates -- all of them, in index order; more -- the K first under fd_example_before, in that order.
#pragma once
#include "fd_internal.hpp"

namespace {

// the frame's read-back block (fd_particles::examples): this head, then 2 K feature rows from examples_rows_offset() on
struct ParticleExamplesHead {
    fd_particles_info info;
    fd_flow_motion_info motion;
    int32_t nPos, nNeg;
    fd_particles_example pos[FD_PARTICLES_EXAMPLES_MAX], neg[FD_PARTICLES_EXAMPLES_MAX];
    uint8_t rowValid[2 * FD_PARTICLES_EXAMPLES_MAX];   // slot s < K: positive s; slot K + s: negative s
};
constexpr size_t examples_rows_offset() { return (sizeof(ParticleExamplesHead) + 15) & ~(size_t)15; }

struct ExamplesLds {
    unsigned int hist[PT], chosen[2];
    int waveCandidates[PT / 64], waveEqual[PT / 64], waveAbove[PT / 64];
    int32_t sIdx[FD_PARTICLES_EXAMPLES_MAX];
};

// A candidate's key, larger for the better example, never 0 (0 is "not a candidate").  The weights of a generation that
// k_particles_state let pass are not negative and finite, so the bits of weight + 0.0 (-0 becomes +0) ascend with the weight and stay
// below 0x7ff0...: + 1 for the positives, the complement for the negatives.
__device__ inline unsigned long long examples_key(bool positive, double weight) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(weight + 0.0);
    return positive ? bits + 1ull : ~bits;
}

// One side, by the whole workgroup; returns its count, the records are in rec[0 .. count).  With M candidates:
//  - M > K: T, the K-th largest key, by radix selection; the survivors are the G < K candidates above T and of those equal to T the
//    K - G with the lowest indices.  M <= K: T = 0, every candidate is above it.
//  - every wavefront walks a contiguous quarter of the samples twice, 64 at a time: first it counts its keys above and equal to T; with
//    the counts of the wavefronts in front of it, ballots then give every survivor its place in index order (sIdx).
//  - M <= K: that is the list.  M > K: survivor j goes to the slot that counts the survivors before it (fd_example_before).
// All loops are counted; the cut is made of integer counts, so it does not depend on who adds first.
__device__ inline int examples_side(const ParticleGen& g, const uint8_t* __restrict__ valid, int n, bool positive, double threshold, bool requireWindow, int K,
                                    unsigned long long* keys, ExamplesLds& L, fd_particles_example* __restrict__ rec) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();   // the side before this one has read keys and L
    int mine = 0;
    for (int i = tid; i < n; i += PT) {
        const double w = g.weight[i];
        const bool candidate = fd_example_candidate(positive, w, threshold) && (!requireWindow || valid[i] != 0);
        keys[i] = candidate ? examples_key(positive, w) : 0ull;
        mine += candidate ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (lane == 0) L.waveCandidates[wave] = mine;
    __syncthreads();
    int M = 0;
    for (int w = 0; w < PT / 64; ++w) M += L.waveCandidates[w];
    const unsigned long long T = M > K ? negatives_select(keys, n, L.hist, L.chosen, (unsigned int)(M - K)) : 0ull;

    const int count = negatives_survivors(keys, n, T, M, K, FD_PARTICLES_EXAMPLES_MAX, L.waveEqual, L.waveAbove,
                                          [&](int slot, int i, unsigned long long) { L.sIdx[slot] = i; });
    __syncthreads();
    if (tid < count) {
        const int32_t index = L.sIdx[tid];
        const double w = g.weight[index];
        int place = tid;
        if (M > K) {
            place = 0;
            for (int s = 0; s < count; ++s) {
                const int32_t other = L.sIdx[s];
                place += fd_example_before(positive, g.weight[other], other, w, index) ? 1 : 0;
            }
        }
        fd_particles_example r{};   // the padding too: the record is copied whole
        r.index = index; r.x = g.x[index]; r.y = g.y[index]; r.size = g.size[index]; r.valid = 0; r.weight = w;
        rec[place] = r;
    }
    return count;
}

// One workgroup behind k_particles_state: the info (and the flow's motion) into the read-back block, then both sides.  With
// bad_weight both counts are 0; whether a state was found does not matter.
__global__ __launch_bounds__(PT) void k_particles_examples(ParticleGen g, const uint8_t* __restrict__ valid, int n, fd_particles_examples_params prm,
                                                           const fd_particles_info* __restrict__ info, const fd_flow_motion_info* __restrict__ motion,
                                                           ParticleExamplesHead* __restrict__ out) {
    extern __shared__ __align__(16) unsigned long long exampleKeys[];   // n
    __shared__ ExamplesLds L;
    const int tid = threadIdx.x;
    const bool bad = info->bad_weight != 0;   // uniform over the workgroup
    if (tid == 0) {
        out->info = *info;
        if (motion) out->motion = *motion;
    }
    int nPos = 0, nNeg = 0;
    if (!bad) {
        nPos = examples_side(g, valid, n, true, prm.positive_threshold, prm.require_window != 0, prm.max_count, exampleKeys, L, out->pos);
        nNeg = examples_side(g, valid, n, false, prm.negative_threshold, prm.require_window != 0, prm.max_count, exampleKeys, L, out->neg);
    }
    if (tid == 0) { out->nPos = nPos; out->nNeg = nNeg; }
}

// the chosen samples as the compact list the family's kernel reads: slot s through the wrapper chain (fd_particle_sample); a slot
// without a record gets the empty window {0, 0, 0, 0}
__global__ __launch_bounds__(2 * FD_PARTICLES_EXAMPLES_MAX) void k_particles_examples_xywh(const ParticleExamplesHead* __restrict__ head, int K, double aspect,
                                                                                          FdSampleMaps maps, int4* __restrict__ xywh) {
    const int s = threadIdx.x;
    if (s >= 2 * K) return;
    const bool negative = s >= K;
    const int k = negative ? s - K : s;
    int4 out = make_int4(0, 0, 0, 0);
    if (k < (negative ? head->nNeg : head->nPos)) {
        const fd_particles_example r = negative ? head->neg[k] : head->pos[k];
        int32_t sx, sy, sw, sh;
        fd_particle_sample(r.x, r.y, r.size, aspect, maps, sx, sy, sw, sh);
        out = make_int4(sx, sy, sw, sh);
    }
    xywh[s] = out;
}

// the same for a pyramid family: k_particles_windows in list form.  Slot s resolves its record through the chain to a window {layer, bx,
// by} by the host's rule (the width -> layer table, fd_sample_place) and flags it; a slot without a record or without a window is
// flagged invalid and lists `spare`, a window that exists, so that the feature kernel reads valid memory: its row never leaves the device
__global__ __launch_bounds__(2 * FD_PARTICLES_EXAMPLES_MAX) void k_particles_examples_windows(const ParticleExamplesHead* __restrict__ head, int K, double aspect,
                                                                                             FdSampleMaps maps, ParticleLayers layers,
                                                                                             const int16_t* __restrict__ layerOf, int tableLen, int pw, int ph,
                                                                                             FdSampleWindow spare, int32_t* __restrict__ list,
                                                                                             uint8_t* __restrict__ valid) {
    const int s = threadIdx.x;
    if (s >= 2 * K) return;
    const bool negative = s >= K;
    const int k = negative ? s - K : s;
    FdSampleWindow w = spare;
    bool ok = false;
    if (k < (negative ? head->nNeg : head->nPos)) {
        const fd_particles_example r = negative ? head->neg[k] : head->pos[k];
        int32_t sx, sy, sw, sh;
        fd_particle_sample(r.x, r.y, r.size, aspect, maps, sx, sy, sw, sh);
        const int pos = sw > 0 && sw < tableLen ? (int)layerOf[sw] : -1;
        if (pos >= 0 && pos < layers.n) {
            int32_t bx, by;
            ok = fd_sample_place(layers.l[pos].scale, layers.l[pos].w, layers.l[pos].h, pw, ph, sx, sy, sw, sh, bx, by);
            if (ok) { w.layer = pos; w.bx = bx; w.by = by; }
        }
    }
    list[3 * s] = w.layer; list[3 * s + 1] = w.bx; list[3 * s + 2] = w.by;
    valid[s] = ok ? 1 : 0;
}

}  // namespace
