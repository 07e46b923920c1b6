// featuredetection_amd/csrc/particle_negatives.hpp -- the additional negatives of condensation::PositionDependentMeasurementModel::adapt
// (PositionDependentMeasurementModel.cpp:172-192) for a resident particle set: of the samples outside a box around the state
// k_particles_state has just extracted, the K with the largest weights, so that a frame of that model hands its adaptation the few
// samples it reads in the frame's one read-back and never downloads the generation.  Included by condensation.hip only,
// behind ParticleGen; the box is fd_negative_bounds (fd_internal.hpp), the copy the host's adapt uses.
//
// The reference walks the samples in index order and keeps a list ascending by weight: it inserts at lower_bound while the list is not
// full, afterwards it replaces the front when front.weight < sample.weight and bubbles the new element up while prev > next.  Both
// steps put a new element before equal ones, so the list is: the K samples largest under (weight descending, index ascending), in the
// order (weight ascending, index descending).
#pragma once
#include "fd_internal.hpp"

namespace {

// what k_particles_negatives leaves behind the info, in the same device block: one copy brings both back
struct ParticleNegativesOut {
    int32_t count, pad;
    fd_particles_negative rec[FD_PARTICLES_NEGATIVES_MAX];
};
struct ParticleReadBack {
    fd_particles_info info;
    ParticleNegativesOut negatives;
};

// a candidate's key: the weights of a generation that k_particles_state let pass are not negative and finite, so the bits of
// weight + 0.0 (-0 becomes +0) ascend with the weight; + 1 keeps 0 for "not a candidate"
__device__ inline unsigned long long negatives_key(double weight) { return (unsigned long long)__double_as_longlong(weight + 0.0) + 1ull; }

static_assert(PT == 256, "negatives_select clears and walks one histogram bin per thread");

// one more key in its bin, k_flow_motion's form: the lanes that share the bin of the first taking lane go in as one addition (equal
// weights -- the zeros of the samples without a window -- crowd into one bin).  Integer additions: the histogram does not depend on
// who adds first.
__device__ inline void negatives_hist_add(unsigned int* hist, unsigned int bin, bool take) {
    const unsigned long long takers = __ballot(take);
    if (!takers) return;
    const int leader = __ffsll((long long)takers) - 1;
    const unsigned int leaderBin = (unsigned int)__shfl((int)bin, leader);
    const unsigned long long same = __ballot(take && bin == leaderBin);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[leaderBin], (unsigned int)__popcll(same));
    else if (take && bin != leaderBin) atomicAdd(&hist[bin], 1u);
}

// The k-th smallest (from 0) of the non-zero keys[0 .. n) by radix selection: eight passes of eight bits from the top; a pass counts
// the keys that agree with the digits chosen so far by their next digit, and the first wavefront walks the 256 counts to the digit
// that holds rank k.  Every thread of the workgroup calls this; k is below the number of non-zero keys.
__device__ inline unsigned long long negatives_select(const unsigned long long* keys, int n, unsigned int* hist, unsigned int* chosen, unsigned int k) {
    const int tid = threadIdx.x;
    unsigned long long prefix = 0ull;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        const unsigned long long above = pass == 0 ? 0ull : ~0ull << (shift + 8);
        hist[tid] = 0;   // PT == 256 bins
        __syncthreads();
        for (int base = 0; base < n; base += PT) {   // whole wavefronts: negatives_hist_add ballots
            const int i = base + tid;
            const unsigned long long key = i < n ? keys[i] : 0ull;
            negatives_hist_add(hist, (unsigned int)(key >> shift) & 255u, key != 0ull && (key & above) == prefix);
        }
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
        prefix |= (unsigned long long)chosen[0] << shift;
        k = chosen[1];
    }
    return prefix;
}

// The survivors of a selection in index order, by the whole workgroup (shared with k_particles_examples, particle_examples.hpp): of the M
// non-zero keys[0 .. n) those above the cut T and, of those equal to T, the first with the lowest indices, min(M, K) in all (M <= K: T is 0
// and every candidate lies above it).  Every wavefront walks a contiguous quarter of the samples twice, 64 at a time: first it counts
// its keys above and equal to T; with the counts of the wavefronts in front of it, ballots then give every survivor its place in index
// order, and store(slot, index, key) is called for it once, slot < min(M, K) <= cap.  Returns that count; the caller synchronises
// before it reads what store wrote.  waveEqual / waveAbove: PT / 64 ints of LDS each.
template <class Store>
__device__ inline int negatives_survivors(const unsigned long long* keys, int n, unsigned long long T, int M, int K, int cap, int* waveEqual, int* waveAbove,
                                          Store store) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int segment = ((n + PT - 1) / PT) * 64, begin = wave * segment;   // a wavefront's quarter, whole steps of 64
    int equalHere = 0, aboveHere = 0;
    for (int o = 0; o < segment; o += 64) {
        const int i = begin + o + lane;
        const unsigned long long key = i < n ? keys[i] : 0ull;
        equalHere += __popcll(__ballot(i < n && key == T));
        aboveHere += __popcll(__ballot(key > T));
    }
    if (lane == 0) { waveEqual[wave] = equalHere; waveAbove[wave] = aboveHere; }
    __syncthreads();
    int G = 0, equalRun = 0, aboveRun = 0;
    for (int w = 0; w < PT / 64; ++w) {
        G += waveAbove[w];
        if (w < wave) { equalRun += waveEqual[w]; aboveRun += waveAbove[w]; }
    }
    const int need = M > K ? K - G : 0;     // of the keys equal to T (with M <= K those are no candidates)
    for (int o = 0; o < segment; o += 64) {
        const int i = begin + o + lane;
        const unsigned long long key = i < n ? keys[i] : 0ull;
        const bool above = key > T, equal = i < n && key == T;
        const unsigned long long aboveMask = __ballot(above), equalMask = __ballot(equal), below = (1ull << lane) - 1ull;
        const int aboveRank = aboveRun + __popcll(aboveMask & below), equalRank = equalRun + __popcll(equalMask & below);
        const int slot = aboveRank + min(equalRank, need);   // of a survivor: < G + need
        if ((above || (equal && equalRank < need)) && slot < cap) store(slot, i, key);
        aboveRun += __popcll(aboveMask);
        equalRun += __popcll(equalMask);
    }
    return M > K ? K : M;   // G + need
}

// One workgroup behind k_particles_state.  Without a state, or with bad_weight, the count is 0.  Otherwise, with M candidates (the
// samples outside the box; their keys in LDS, 0 for every other sample):
//  - M > K: T, the K-th largest key, by radix selection; the survivors are the G < K candidates above T and of those equal to T the
//    K - G with the lowest indices.  M <= K: T = 0, every candidate is above it.
//  - every wavefront walks a contiguous quarter of the samples twice, 64 at a time: first it counts its keys above and equal to T;
//    with the counts of the wavefronts in front of it, ballots then give every survivor its place in index order (sKey / sIdx).
//  - survivor j goes to the output slot that counts the survivors listed before it: a smaller key, or the same key and a higher index.
// All loops are counted; nothing waits on another workgroup; the additions are integer ones.
__global__ __launch_bounds__(PT) void k_particles_negatives(ParticleGen g, int n, fd_particles_negatives_params prm, const fd_particles_info* __restrict__ info,
                                                            ParticleNegativesOut* __restrict__ out) {
    extern __shared__ __align__(16) unsigned long long negKeys[];   // n
    __shared__ unsigned int hist[PT], chosen[2];
    __shared__ int waveCandidates[PT / 64], waveEqual[PT / 64], waveAbove[PT / 64];
    __shared__ unsigned long long sKey[FD_PARTICLES_NEGATIVES_MAX];
    __shared__ int32_t sIdx[FD_PARTICLES_NEGATIVES_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = prm.max_count;
    if (!info->found || info->bad_weight) {   // uniform over the workgroup
        if (tid == 0) { out->count = 0; out->pad = 0; }
        return;
    }
    const FdNegativeBounds bounds = fd_negative_bounds(prm.offset_factor, prm.down_scale, prm.up_scale, info->x, info->y, info->size);
    int mine = 0;
    for (int i = tid; i < n; i += PT) {
        const bool candidate = fd_negative_outside(bounds, g.x[i], g.y[i], g.size[i]);
        negKeys[i] = candidate ? negatives_key(g.weight[i]) : 0ull;
        mine += candidate ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (lane == 0) waveCandidates[wave] = mine;
    __syncthreads();
    int M = 0;
    for (int w = 0; w < PT / 64; ++w) M += waveCandidates[w];
    const unsigned long long T = M > K ? negatives_select(negKeys, n, hist, chosen, (unsigned int)(M - K)) : 0ull;

    const int count = negatives_survivors(negKeys, n, T, M, K, FD_PARTICLES_NEGATIVES_MAX, waveEqual, waveAbove,
                                          [&](int slot, int i, unsigned long long key) { sKey[slot] = key; sIdx[slot] = i; });
    __syncthreads();
    if (tid < count) {
        const unsigned long long key = sKey[tid];
        const int32_t index = sIdx[tid];
        int place = 0;
        for (int s = 0; s < count; ++s) place += (sKey[s] < key || (sKey[s] == key && sIdx[s] > index)) ? 1 : 0;
        fd_particles_negative r;
        r.index = index; r.x = g.x[index]; r.y = g.y[index]; r.size = g.size[index]; r.weight = g.weight[index];
        out->rec[place] = r;
    }
    if (tid == 0) { out->count = count; out->pad = 0; }
}

}  // namespace
