// featuredetection_amd/csrc/condensation.hip -- the particle set of the Condensation tracker resident on the device: two generations of
// samples as structure-of-arrays and the per-frame steps of ResamplingSampler(LowVarianceSampling, SimpleTransitionModel)
// (ResamplingSampler.cpp:50-59, LowVarianceSampling.cpp:20-46, SimpleTransitionModel.cpp:25-44), of
// ExtendedHogBasedMeasurementModel's weighting (.cpp:173-205) and of FilteringStateExtractor(WeightedMeanStateExtractor)
// (WeightedMeanStateExtractor.cpp:23-62).  The scoring of the samples is the tracker's (ehog_tracker.hpp).  A set without a tracker serves
// SingleClassifierModel on the integral family (scored by integral.hip, weighed by k_particles_weigh's classifier mode) and
// OpticalFlowTransitionModel::predict (k_particles_sample with the motion optflow.hip leaves on the device), and SingleClassifierModel
// on the pyramid families: fd_particles_evaluate_pyramid resolves the samples to windows here (particle_windows.hpp) and hands the list to
// the scoring kernels of hog.hip / rvm.hip.  condensation::WvmSvmModel takes the same window list through wvm.hip's cascade
// (fd_particles_evaluate_wvm_svm); its selection rule and its weighting are particle_wvm_svm.hpp.  The additional negatives of
// PositionDependentMeasurementModel::adapt are chosen behind the state (fd_particles_state_negatives, particle_negatives.hpp), and so are
// the examples of SelfLearningMeasurementModel::adapt, with their feature rows (fd_particles_state_examples_*, particle_examples.hpp).  DESIGN.md 4.7.
//
// Kernels: k_particles_sample, k_particles_weigh, k_particles_state -- one workgroup of 256 threads each, because every one of them
// needs the whole set: the cumulative weights and the state sums are sequential double sums in index order (the resampler compares
// against them, so another association would select other samples); they are walked by single lanes in LDS, everything around them
// is parallel.  k_particles_negatives (particle_negatives.hpp) is a fourth of this shape: its selection needs every weight; k_particles_examples (particle_examples.hpp) a fifth.  All loops are
// counted; nothing waits on another workgroup.
#include "fd_internal.hpp"
#include "particle_windows.hpp"
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>

namespace {

constexpr int PT = 256;                        // threads of the single-workgroup kernels
constexpr int32_t PARTICLE_NO_CLUSTER = INT32_MIN;   // the empty key of the cluster table
constexpr int PARTICLES_CLASSIFIER = 3;        // k_particles_weigh as SingleClassifierModel: behind the FD_PARTICLES_* modes of fd_particles_weigh

struct ParticleGen {
    int32_t *x, *y, *size, *vx, *vy;
    float* vsize;
    double *weight, *score;
    uint8_t* target;
    int32_t* cluster;
};

__host__ __device__ inline bool particle_weight_ok(double w) { return w >= 0.0 && w <= DBL_MAX; }   // not negative, not infinite, not NaN

// LowVarianceSampling::resample + SimpleTransitionModel::predict + the fresh samples of ResamplingSampler::sample.
// cum[k]: the weights added up in index order, by one lane.  The forward walk of the reference (advance while pointer > sum) ends at
// the smallest k with pointer <= cum[k] (weights are not negative, so cum does not decrease): every copy finds its k by bisection.
// Where rounding leaves the last pointers above the total the walk stops at the last sample (the reference walks off the end).
// With `motion` (OpticalFlowTransitionModel::predict, .cpp:173-190): where it is ok a copy's velocity is the median flow, moved by the
// draws of `flowDiffusion`; otherwise the copy is moved as without a motion.  The branch is uniform over the launch.
__global__ __launch_bounds__(PT) void k_particles_sample(ParticleGen src, ParticleGen dst, int nOld, int nCopies, int nFresh, double step, double start,
                                                         const double* __restrict__ diffusion, const int32_t* __restrict__ fresh, int32_t firstFreshId,
                                                         int32_t* __restrict__ source, fd_particles_info* __restrict__ info,
                                                         const fd_flow_motion_info* __restrict__ motion, const double* __restrict__ flowDiffusion) {
    extern __shared__ double cum[];
    const int tid = threadIdx.x;
    const bool byFlow = motion && motion->ok;
    if (byFlow) diffusion = flowDiffusion;
    if (nCopies > 0) {
        for (int i = tid; i < nOld; i += PT) cum[i] = src.weight[i];
        __syncthreads();
        if (tid == 0) {
            double running = 0.0;
            for (int i = 0; i < nOld; ++i) {
                running = running + cum[i];
                cum[i] = running;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < nCopies; i += PT) {
        const double weightPointer = start + (double)(unsigned int)i * step;
        int lo = 0, hi = nOld - 1;
        for (int it = 0; it < 14 && lo < hi; ++it) {   // 2^13 = FD_PARTICLES_MAX
            const int mid = (lo + hi) >> 1;
            if (weightPointer > cum[mid]) lo = mid + 1;
            else hi = mid;
        }
        const int k = lo;
        double vx = src.vx[k], vy = src.vy[k], vs = src.vsize[k];
        if (byFlow) { vx = motion->median_x; vy = motion->median_y; vs = motion->median_ratio; }
        vx = vx + diffusion[3 * i];
        vy = vy + diffusion[3 * i + 1];
        vs = vs * diffusion[3 * i + 2];
        const int nvx = static_cast<int>(round(vx)), nvy = static_cast<int>(round(vy));
        const float nvs = (float)vs;
        dst.vx[i] = nvx; dst.vy[i] = nvy; dst.vsize[i] = nvs;
        dst.x[i] = src.x[k] + nvx;
        dst.y[i] = src.y[k] + nvy;
        dst.size[i] = static_cast<int>(roundf((float)src.size[k] * nvs));   // int * float: the product and its rounding are float
        dst.weight[i] = 1.0; dst.score[i] = 0.0; dst.target[i] = 0;
        dst.cluster[i] = src.cluster[k];
        source[i] = k;
    }
    for (int j = tid; j < nFresh; j += PT) {
        const int i = nCopies + j;
        dst.x[i] = fresh[3 * j]; dst.y[i] = fresh[3 * j + 1]; dst.size[i] = fresh[3 * j + 2];
        dst.vx[i] = 0; dst.vy[i] = 0; dst.vsize[i] = 1.f;
        dst.weight[i] = 1.0; dst.score[i] = 0.0; dst.target[i] = 0;
        dst.cluster[i] = firstFreshId + j;
        source[i] = -1;
    }
    if (tid == 0) {
        info->count = nCopies + nFresh;
        info->n_valid = 0;
        info->bad_weight = 0;
        info->best_score = -DBL_MAX;
    }
}

// ProbabilisticSvmClassifier::getProbability (.cpp:54-58) on fABp = logisticA + logisticB * score, in double
__device__ inline double particle_logistic(double fABp) { return fABp >= 0 ? exp(-fABp) / (1.0 + exp(-fABp)) : 1.0 / (1.0 + exp(fABp)); }

// the end of a weighing kernel: the largest of the threads' best scores and the sum of their valid counts into the info
__device__ inline void particles_publish_best(double best, int nValid, fd_particles_info* __restrict__ info) {
    __shared__ double sBest[PT];
    __shared__ int sValid[PT];
    const int tid = threadIdx.x;
    sBest[tid] = best;
    sValid[tid] = nValid;
    __syncthreads();
    for (int s = PT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            if (sBest[tid] < sBest[tid + s]) sBest[tid] = sBest[tid + s];
            sValid[tid] += sValid[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        info->best_score = sBest[0];
        info->n_valid = sValid[0];
    }
}

// ExtendedHogBasedMeasurementModel::scored for every sample, ProbabilisticSvmClassifier::getProbability (.cpp:54-58) in double.  Two
// passes: the first only looks for a product that is negative or not finite; with one, nothing is written but the flag.
// mode PARTICLES_CLASSIFIER is SingleClassifierModel.cpp:32-42: the weight is the probability itself, target = score >= svmThreshold.
__global__ __launch_bounds__(PT) void k_particles_weigh(ParticleGen g, int n, const uint8_t* __restrict__ valid, double logisticA, double logisticB,
                                                        double svmThreshold, int mode, double rejectionThreshold, fd_particles_info* __restrict__ info) {
    const int tid = threadIdx.x;
    auto weighed = [&](int i) {
        const double p = particle_logistic(logisticA + logisticB * g.score[i]);
        return mode == PARTICLES_CLASSIFIER ? p : g.weight[i] * p;
    };
    int bad = 0;
    for (int i = tid; i < n; i += PT)
        if (valid[i] && !particle_weight_ok(weighed(i))) bad = 1;
    if (__syncthreads_or(bad)) {
        if (tid == 0) info->bad_weight = 1;
        return;
    }
    double best = -DBL_MAX;   // bestScore = lowest(); std::max(bestScore, score) never takes a NaN
    int nValid = 0;
    for (int i = tid; i < n; i += PT) {
        double score = 0.0;
        if (!valid[i]) {
            g.target[i] = 0;
            g.weight[i] = 0.0;
            g.score[i] = 0.0;
        } else {
            score = g.score[i];
            g.weight[i] = weighed(i);
            g.target[i] = mode == FD_PARTICLES_TARGET_LOST || mode == PARTICLES_CLASSIFIER ? score >= svmThreshold
                                                                                           : (mode == FD_PARTICLES_SLIDING_WINDOW ? score > rejectionThreshold : 1);
            ++nValid;
        }
        if (best < score) best = score;
    }
    particles_publish_best(best, nValid, info);
}

}  // namespace

#include "particle_wvm_svm.hpp"
#include "particle_negatives.hpp"
#include "particle_examples.hpp"

namespace {

__device__ inline unsigned int particle_hash(int32_t id) { return (unsigned int)id * 2654435761u; }

// FilteringStateExtractor + WeightedMeanStateExtractor.  The cluster sizes are counted in an LDS hash table (`slots` a power of two
// >= 2 n: linear probing, integer atomics, so the counts do not depend on the order of arrival); one 64-bit atomic max over
// (size, -index) of every target sample then names the first member of the largest cluster, of equally large clusters the one whose
// first member comes first.  The sums: per chunk of 256 samples every thread forms its sample's seven products (0 for a sample
// outside the cluster: the sums start at +0 and never become -0, so adding +0 changes no bit), and eight lanes add one column each
// in index order.  The eighth column adds up all weights of the generation.
__global__ __launch_bounds__(PT) void k_particles_state(ParticleGen g, int n, int slots, fd_particles_info* __restrict__ info) {
    extern __shared__ __align__(8) unsigned char stateLds[];
    __shared__ unsigned long long sWinner;
    __shared__ double sSums[8];
    __shared__ int sTargets[PT];
    const int tid = threadIdx.x;
    int32_t* keys = (int32_t*)stateLds;
    int* counts = (int*)(stateLds + sizeof(int32_t) * (size_t)slots);
    for (int s = tid; s < slots; s += PT) { keys[s] = PARTICLE_NO_CLUSTER; counts[s] = 0; }
    if (tid == 0) sWinner = 0ull;
    __syncthreads();
    int bad = tid == 0 && info->bad_weight, nTarget = 0;   // raised by k_particles_weigh: the generation was left unweighted
    for (int i = tid; i < n; i += PT) {
        if (!particle_weight_ok(g.weight[i])) bad = 1;
        if (!g.target[i]) continue;
        ++nTarget;
        const int32_t id = g.cluster[i];
        unsigned int slot = particle_hash(id) & (unsigned int)(slots - 1);
        for (int probe = 0; probe < slots; ++probe) {   // slots > number of distinct ids: a free slot exists
            const int32_t old = atomicCAS(&keys[slot], PARTICLE_NO_CLUSTER, id);
            if (old == PARTICLE_NO_CLUSTER || old == id) { atomicAdd(&counts[slot], 1); break; }
            slot = (slot + 1) & (unsigned int)(slots - 1);
        }
    }
    bad = __syncthreads_or(bad);
    for (int i = tid; i < n; i += PT) {
        if (!g.target[i]) continue;
        const int32_t id = g.cluster[i];
        unsigned int slot = particle_hash(id) & (unsigned int)(slots - 1);
        for (int probe = 0; probe < slots && keys[slot] != id; ++probe) slot = (slot + 1) & (unsigned int)(slots - 1);
        atomicMax(&sWinner, ((unsigned long long)(unsigned int)counts[slot] << 32) | (unsigned int)(INT32_MAX - i));
    }
    sTargets[tid] = nTarget;
    __syncthreads();
    for (int s = PT / 2; s > 0; s >>= 1) {
        if (tid < s) sTargets[tid] += sTargets[tid + s];
        __syncthreads();
    }
    const unsigned long long winner = sWinner;
    const bool any = winner != 0ull && !bad;
    const int32_t winnerId = winner != 0ull ? g.cluster[INT32_MAX - (int)(unsigned int)(winner & 0xffffffffull)] : 0;
    __syncthreads();   // the table has been read: its memory now holds the products
    double* terms = (double*)stateLds;   // [8][PT]
    double acc = 0.0;
    for (int base = 0; base < n; base += PT) {
        const int i = base + tid;
        double t[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (i < n) {
            const double w = g.weight[i];
            t[7] = w;
            if (any && g.target[i] && g.cluster[i] == winnerId) {
                t[0] = w * g.x[i]; t[1] = w * g.y[i]; t[2] = w * g.size[i]; t[3] = w * g.vx[i]; t[4] = w * g.vy[i]; t[5] = w * g.vsize[i];
                t[6] = w;
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) terms[c * PT + tid] = t[c];
        __syncthreads();
        if (tid < 8) {
            const int m = min(PT, n - base);
            const double* column = terms + tid * PT;
            for (int j = 0; j < m; ++j) acc = acc + column[j];
        }
        __syncthreads();
    }
    if (tid < 8) sSums[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        const double weightSum = sSums[6];
        info->count = n;
        info->n_target = sTargets[0];
        info->weight_sum = sSums[7];
        if (bad) info->bad_weight = 1;
        info->found = 0;
        info->x = info->y = info->size = info->vx = info->vy = 0;
        info->vsize = 0.f;
        info->cluster_id = winnerId;
        if (any && weightSum != 0) {   // if (weightSum == 0) return shared_ptr<Sample>()
            info->found = 1;
            info->x = (int)(sSums[0] / weightSum + 0.5);
            info->y = (int)(sSums[1] / weightSum + 0.5);
            info->size = (int)(sSums[2] / weightSum + 0.5);
            info->vx = (int)(sSums[3] / weightSum + 0.5);
            info->vy = (int)(sSums[4] / weightSum + 0.5);
            info->vsize = (float)(int)(sSums[5] / weightSum + 0.5);   // the reference truncates the size factor as well
        }
    }
}

int particle_state_slots(int n) {
    int slots = 2048;   // 16 KB: the eight columns of products fit
    while (slots < 2 * n) slots *= 2;
    return slots;
}

}  // namespace

struct fd_particles {
    fd_ctx* ctx = nullptr;
    fd_ehog_tracker* tracker = nullptr;   // NULL: an unbound set (fd_particles_create_unbound)
    int capacity = 0, n = 0, cur = 0;
    bool sumKnown = true, bad = false, evaluated = false;
    double sum = 0.0;   // the weights of the current generation added in index order, when sumKnown
    DevBuf arena, staging;
    DevBuf dinfo;   // a ParticleReadBack: the fd_particles_info every kernel writes, and behind it what k_particles_negatives leaves
    DevBuf examples;   // fd_particles_state_examples_*: a ParticleExamplesHead and the feature rows behind it, the frame's one read-back
    std::vector<unsigned char> examplesHost;
    DevBuf exampleList;   // fd_particles_state_examples_pyramid: the window {layer, bx, by} of every slot
    DevBuf list;   // fd_particles_evaluate_pyramid: the window {layer, bx, by} of every sample, slot i for sample i
    ParticleGen gen[2];
    int32_t* source = nullptr;
    int32_t* windows = nullptr;   // per sample {layer, bx, by, valid} of fd_particles_evaluate, or the mapped {x, y, width, height} of _evaluate_integral
    uint8_t* valid = nullptr;
    HostBuf pinned;   // the draws of one fd_particles_sample / _sample_flow on their way to the device
    // fd_particles_evaluate_wvm_svm: the model the current generation was evaluated with (NULL: none, or another kind of evaluate), what its
    // cascade left on the device (wvmCascaded: it ran at all), and the selection of fd_particles_weigh_wvm_svm
    const fd_wvm* wvm = nullptr;
    bool wvmCascaded = false, wvmWeighed = false;
    FdWvmResidentRun wvmRun{};
    DevBuf wvmSel;
    void evaluatedBy(const fd_wvm* m) { evaluated = true; wvm = m; wvmWeighed = false; }
    void notEvaluated() { evaluated = false; wvm = nullptr; wvmWeighed = false; }
    hipEvent_t uploaded = nullptr;
    ~fd_particles() { if (uploaded) (void)hipEventDestroy(uploaded); }
};

namespace {

fd_particles* particles_checked(fd_ctx* ctx, fd_particles* p, const char* what) {
    if (!ctx || !p) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (p->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "objects belong to different contexts");
    HIP_CHECK(hipSetDevice(ctx->device));
    return p;
}

// the state kernel on the current generation, into p->dinfo
void particles_queue_state(fd_ctx* ctx, fd_particles* p) {
    static uint64_t allowed = 0;
    const int slots = particle_state_slots(p->n);
    const size_t lds = sizeof(int32_t) * 2 * (size_t)slots;
    fd_allow_lds(ctx, (const void*)k_particles_state, (int)(sizeof(int32_t) * 2 * (size_t)particle_state_slots(FD_PARTICLES_MAX)), allowed);
    hipLaunchKernelGGL(k_particles_state, dim3(1), dim3(PT), lds, ctx->stream, p->gen[p->cur], p->n, slots, p->dinfo.as<fd_particles_info>());
    HIP_CHECK(hipGetLastError());
}

// state kernel + the read-back of the info; refreshes what the host knows about the generation.  With `negatives` the selection is
// queued behind the state kernel and comes back in the same copy: *count records into `records`
void particles_read_state(fd_ctx* ctx, fd_particles* p, fd_particles_info* out, const fd_flow_motion_info* dmotion = nullptr,
                          fd_flow_motion_info* motion = nullptr, const fd_particles_negatives_params* negatives = nullptr, int* count = nullptr,
                          fd_particles_negative* records = nullptr) {
    static uint64_t allowedNegatives = 0;
    particles_queue_state(ctx, p);
    ParticleReadBack back;
    if (negatives) {
        fd_allow_lds(ctx, (const void*)k_particles_negatives, (int)(sizeof(unsigned long long) * FD_PARTICLES_MAX), allowedNegatives);
        hipLaunchKernelGGL(k_particles_negatives, dim3(1), dim3(PT), sizeof(unsigned long long) * (size_t)p->n, ctx->stream, p->gen[p->cur], p->n, *negatives,
                           p->dinfo.as<fd_particles_info>(), &p->dinfo.as<ParticleReadBack>()->negatives);
        HIP_CHECK(hipGetLastError());
        const size_t bytes = offsetof(ParticleReadBack, negatives.rec) + sizeof(fd_particles_negative) * (size_t)negatives->max_count;
        HIP_CHECK(hipMemcpyAsync(&back, p->dinfo.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        HIP_CHECK(hipMemcpyAsync(out, p->dinfo.p, sizeof(*out), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (dmotion) HIP_CHECK(hipMemcpyAsync(motion, dmotion, sizeof(*motion), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (negatives) {
        *out = back.info;
        *count = std::min(std::max(back.negatives.count, 0), negatives->max_count);
        std::memcpy(records, back.negatives.rec, sizeof(fd_particles_negative) * (size_t)*count);
    }
    p->sum = out->weight_sum;
    p->sumKnown = true;
    p->bad = out->bad_weight != 0;
}

void particles_create(fd_ctx* ctx, fd_ehog_tracker* t, int capacity, fd_particles** out) {
    if (capacity < 1 || capacity > FD_PARTICLES_MAX) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_create: the capacity must be 1 .. %d", FD_PARTICLES_MAX);
    HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<fd_particles> p(new fd_particles());
    p->ctx = ctx;
    p->tracker = t;
    p->capacity = capacity;
    const size_t N = (size_t)capacity;
    // per generation: weight, score (8 N each), x, y, size, vx, vy, vsize, cluster (4 N each), target (N); then the window list (16 N), source (4 N) and valid (N)
    const size_t perGen = (16 * N + 28 * N + N + 63) & ~(size_t)63;   // the doubles of the second generation stay aligned
    p->arena.reserve(2 * perGen + 20 * N + N);
    HIP_CHECK(hipMemset(p->arena.p, 0, 2 * perGen + 20 * N + N));
    unsigned char* base = p->arena.as<unsigned char>();
    for (int gi = 0; gi < 2; ++gi) {
        unsigned char* b = base + perGen * gi;
        ParticleGen& G = p->gen[gi];
        G.weight = (double*)b; G.score = (double*)(b + 8 * N);
        int32_t* q = (int32_t*)(b + 16 * N);
        G.x = q; G.y = q + N; G.size = q + 2 * N; G.vx = q + 3 * N; G.vy = q + 4 * N; G.vsize = (float*)(q + 5 * N); G.cluster = q + 6 * N;
        G.target = (uint8_t*)(q + 7 * N);
    }
    p->windows = (int32_t*)(base + 2 * perGen);   // 16-byte elements at a 64-byte boundary
    p->source = (int32_t*)(base + 2 * perGen + 16 * N);
    p->valid = (uint8_t*)(base + 2 * perGen + 20 * N);
    p->staging.reserve(60 * N);   // two blocks of draws (24 N each) and the fresh samples (12 N)
    p->pinned.reserve(60 * N);
    p->dinfo.reserve(sizeof(ParticleReadBack));
    fd_particles_info zero;
    std::memset(&zero, 0, sizeof(zero));
    zero.best_score = -DBL_MAX;
    HIP_CHECK(hipMemcpy(p->dinfo.p, &zero, sizeof(zero), hipMemcpyHostToDevice));
    HIP_CHECK(hipEventCreateWithFlags(&p->uploaded, hipEventDisableTiming));
    *out = p.release();
}

// fd_particles_sample (flow NULL), and fd_particles_sample_flow: `diffusion` is then the fallback block
void particles_sample(fd_ctx* ctx, fd_particles* p, const char* who, fd_flow* flow, int count, int n_resampled, double u, const double* flow_diffusion,
                      const double* diffusion, const int32_t* fresh, int32_t first_fresh_cluster_id) {
    particles_checked(ctx, p, who);
    if (count < 0 || count > p->capacity) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %d samples, the capacity is %d", who, count, p->capacity);
    if (n_resampled < 0 || n_resampled > count) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %d of %d samples resampled", who, n_resampled, count);
    const int nFresh = count - n_resampled;
    if ((n_resampled > 0 && (!diffusion || (flow && !flow_diffusion))) || (nFresh > 0 && !fresh)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    if (nFresh > 0 && ((int64_t)first_fresh_cluster_id + nFresh - 1 > INT32_MAX || first_fresh_cluster_id == PARTICLE_NO_CLUSTER))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the fresh cluster ids leave the int range", who);
    const fd_flow_motion_info* dmotion = flow ? fd_flow_device_motion(ctx, flow, who) : nullptr;
    if (!p->sumKnown) {   // weighed since the last read-back: ask the device for the sum the step is made of
        fd_particles_info info;
        particles_read_state(ctx, p, &info);
    }
    if (p->bad) FD_THROW(FD_ERR_RUNTIME, "%s: the generation holds a weight that is negative or not finite", who);
    // LowVarianceSampling.cpp:22-26
    int nCopies = 0;
    double step = 0.0, start = 0.0;
    if (p->n > 0 && n_resampled > 0) {
        step = p->sum / (size_t)n_resampled;
        if (step > 0) {
            start = step * u;
            nCopies = n_resampled;
        }
    }
    // the draws: one pinned block, one copy
    HIP_CHECK(hipEventSynchronize(p->uploaded));
    unsigned char* pin = p->pinned.as<unsigned char>();
    const size_t diffBytes = sizeof(double) * 3 * (size_t)nCopies, freshBytes = sizeof(int32_t) * 3 * (size_t)nFresh;
    const size_t flowBytes = flow ? diffBytes : 0;
    if (diffBytes) std::memcpy(pin, diffusion, diffBytes);
    if (flowBytes) std::memcpy(pin + diffBytes, flow_diffusion, flowBytes);
    if (freshBytes) std::memcpy(pin + diffBytes + flowBytes, fresh, freshBytes);
    if (diffBytes + flowBytes + freshBytes) {
        HIP_CHECK(hipMemcpyAsync(p->staging.p, pin, diffBytes + flowBytes + freshBytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipEventRecord(p->uploaded, ctx->stream));
    }
    const int next = p->cur ^ 1;
    const unsigned char* staged = p->staging.as<unsigned char>();
    hipLaunchKernelGGL(k_particles_sample, dim3(1), dim3(PT), nCopies > 0 ? sizeof(double) * (size_t)p->n : 0, ctx->stream, p->gen[p->cur], p->gen[next],
                       p->n, nCopies, nFresh, step, start, (const double*)staged, (const int32_t*)(staged + diffBytes + flowBytes), first_fresh_cluster_id,
                       p->source, p->dinfo.as<fd_particles_info>(), dmotion, (const double*)(staged + diffBytes));
    HIP_CHECK(hipGetLastError());
    p->cur = next;
    p->n = nCopies + nFresh;
    p->sum = (double)p->n;   // every new sample has weight 1: n times 1 added up is exact
    p->sumKnown = true;
    p->notEvaluated();
}

// the kept layers of pyr as the window kernels take them; spare: the first kept layer that holds a pw x ph window at all (layer -1: none)
ParticleLayers particle_layers(const fd_pyramid* pyr, int pw, int ph, FdSampleWindow& spare) {
    ParticleLayers layers;
    std::memset(&layers, 0, sizeof(layers));
    layers.n = (int32_t)pyr->kept.size();
    spare = FdSampleWindow{-1, 0, 0};
    for (int l = 0; l < layers.n; ++l) {
        const HostLayer& L = pyr->all[pyr->kept[l]];
        layers.l[l].scale = L.scale; layers.l[l].w = L.w; layers.l[l].h = L.h;
        if (spare.layer < 0 && L.w >= pw && L.h >= ph) spare.layer = l;
    }
    return layers;
}

// k_particles_windows for the current generation (n > 0) and patches of pw x ph: fills p->list, the trace and the valid flags.  False:
// no kept layer holds a window at all, every sample is invalid and the list must not be scored.
bool particles_windows(fd_ctx* ctx, fd_particles* p, fd_pyramid* pyr, int pw, int ph, double aspect_ratio, const FdSampleMaps& chain) {
    const ParticleGen& G = p->gen[p->cur];
    FdSampleWindow spare;
    const ParticleLayers layers = particle_layers(pyr, pw, ph, spare);
    p->list.reserve(sizeof(int32_t) * 3 * (size_t)p->capacity);
    hipLaunchKernelGGL(k_particles_windows, dim3((p->n + 255) / 256), dim3(256), 0, ctx->stream, G.x, G.y, G.size, p->n, aspect_ratio, chain, layers,
                       pyr->sample_table.dev.as<int16_t>(), pyr->sample_table.length, pw, ph, spare, p->list.as<int32_t>(), (int4*)p->windows, p->valid);
    HIP_CHECK(hipGetLastError());
    return spare.layer >= 0;
}

void particles_weigh(fd_ctx* ctx, fd_particles* p, const char* who, double logistic_a, double logistic_b, double svm_threshold, int mode,
                     double rejection_threshold) {
    if (!p->evaluated) FD_THROW(FD_ERR_RUNTIME, "%s: the generation has not been evaluated (fd_particles_evaluate, _evaluate_integral, _evaluate_pyramid)", who);
    hipLaunchKernelGGL(k_particles_weigh, dim3(1), dim3(PT), 0, ctx->stream, p->gen[p->cur], p->n, p->valid, logistic_a, logistic_b, svm_threshold, mode,
                       rejection_threshold, p->dinfo.as<fd_particles_info>());
    HIP_CHECK(hipGetLastError());
    p->sumKnown = false;
}

}  // namespace

extern "C" {

int fd_particles_create(fd_ctx* ctx, fd_ehog_tracker* t, int capacity, fd_particles** out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !t || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_create: NULL argument");
        particles_create(ctx, t, capacity, out);
    });
}

int fd_particles_create_unbound(fd_ctx* ctx, int capacity, fd_particles** out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_create_unbound: NULL argument");
        particles_create(ctx, nullptr, capacity, out);
    });
}

void fd_particles_destroy(fd_particles* p) { delete p; }

int fd_particles_capacity(const fd_particles* p) { return p ? p->capacity : 0; }

int fd_particles_route_enabled(void) { return fd_knob_cond_device() ? 1 : 0; }

int fd_particles_set(fd_ctx* ctx, fd_particles* p, int n, const fd_particles_arrays* in) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_set");
        if (n < 0 || n > p->capacity) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_set: %d samples, the capacity is %d", n, p->capacity);
        if (n > 0 && (!in || !in->x || !in->y || !in->size || !in->vx || !in->vy || !in->vsize || !in->weight || !in->cluster_id))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_set: NULL argument");
        double sum = 0.0;
        bool bad = false;
        for (int i = 0; i < n; ++i) {
            if (in->cluster_id[i] == PARTICLE_NO_CLUSTER) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_set: cluster id %d is reserved", PARTICLE_NO_CLUSTER);
            sum = sum + in->weight[i];
            bad = bad || !particle_weight_ok(in->weight[i]);
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const ParticleGen& G = p->gen[p->cur];
        const size_t N = (size_t)n;
        if (n > 0) {
            HIP_CHECK(hipMemcpy(G.x, in->x, 4 * N, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(G.y, in->y, 4 * N, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(G.size, in->size, 4 * N, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(G.vx, in->vx, 4 * N, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(G.vy, in->vy, 4 * N, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(G.vsize, in->vsize, 4 * N, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(G.weight, in->weight, 8 * N, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(G.cluster, in->cluster_id, 4 * N, hipMemcpyHostToDevice));
            if (in->score) HIP_CHECK(hipMemcpy(G.score, in->score, 8 * N, hipMemcpyHostToDevice));
            else HIP_CHECK(hipMemset(G.score, 0, 8 * N));
            if (in->target) HIP_CHECK(hipMemcpy(G.target, in->target, N, hipMemcpyHostToDevice));
            else HIP_CHECK(hipMemset(G.target, 0, N));
            HIP_CHECK(hipMemset(p->source, 0xff, 4 * N));
            HIP_CHECK(hipMemset(p->valid, 0, N));
        }
        fd_particles_info zero;
        std::memset(&zero, 0, sizeof(zero));
        zero.count = n;
        zero.best_score = -DBL_MAX;
        zero.bad_weight = bad;
        HIP_CHECK(hipMemcpy(p->dinfo.p, &zero, sizeof(zero), hipMemcpyHostToDevice));
        p->n = n;
        p->sum = sum;
        p->sumKnown = true;
        p->bad = bad;
        p->notEvaluated();
    });
}

int fd_particles_get(fd_ctx* ctx, fd_particles* p, int cap, int* n, const fd_particles_arrays* out) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_get");
        if (!n || cap < 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_get: bad argument");
        *n = p->n;
        if (p->n > cap) FD_THROW(FD_ERR_CAPACITY, "fd_particles_get: %d samples, capacity %d", p->n, cap);
        const ParticleGen& G = p->gen[p->cur];
        const size_t N = (size_t)p->n;
        auto fetch = [&](void* dst, const void* src, size_t bytes) {
            if (dst && bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        };
        if (out) {
            fetch(out->x, G.x, 4 * N); fetch(out->y, G.y, 4 * N); fetch(out->size, G.size, 4 * N); fetch(out->vx, G.vx, 4 * N); fetch(out->vy, G.vy, 4 * N);
            fetch(out->vsize, G.vsize, 4 * N); fetch(out->weight, G.weight, 8 * N); fetch(out->score, G.score, 8 * N); fetch(out->target, G.target, N);
            fetch(out->cluster_id, G.cluster, 4 * N);
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_particles_get_trace(fd_ctx* ctx, fd_particles* p, int32_t* source, int32_t* windows, uint8_t* valid) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_get_trace");
        const size_t N = (size_t)p->n;
        if (windows && !p->evaluated) FD_THROW(FD_ERR_RUNTIME, "fd_particles_get_trace: the generation has not been evaluated");
        if (source && N) HIP_CHECK(hipMemcpyAsync(source, p->source, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
        if (valid && N) HIP_CHECK(hipMemcpyAsync(valid, p->valid, N, hipMemcpyDeviceToHost, ctx->stream));
        if (windows && N) HIP_CHECK(hipMemcpyAsync(windows, p->windows, 16 * N, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int fd_particles_sample(fd_ctx* ctx, fd_particles* p, int count, int n_resampled, double u, const double* diffusion, const int32_t* fresh,
                        int32_t first_fresh_cluster_id) {
    return fd_guard(ctx, [&] {
        particles_sample(ctx, p, "fd_particles_sample", nullptr, count, n_resampled, u, nullptr, diffusion, fresh, first_fresh_cluster_id);
    });
}

int fd_particles_sample_flow(fd_ctx* ctx, fd_particles* p, fd_flow* flow, int count, int n_resampled, double u, const double* flow_diffusion,
                             const double* fallback_diffusion, const int32_t* fresh, int32_t first_fresh_cluster_id) {
    return fd_guard(ctx, [&] {
        if (!flow) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_sample_flow: NULL argument");
        particles_sample(ctx, p, "fd_particles_sample_flow", flow, count, n_resampled, u, flow_diffusion, fallback_diffusion, fresh, first_fresh_cluster_id);
    });
}

int fd_particles_evaluate(fd_ctx* ctx, fd_particles* p, int use_patches, double aspect_ratio) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_evaluate");
        if (!p->tracker) FD_THROW(FD_ERR_RUNTIME, "fd_particles_evaluate: the set is bound to no tracker (fd_particles_create_unbound)");
        const ParticleGen& G = p->gen[p->cur];
        fd_ehog_tracker_score_particles(ctx, p->tracker, p->n, G.x, G.y, G.size, aspect_ratio, use_patches != 0, p->windows, p->valid, G.score);
        p->evaluatedBy(nullptr);
    });
}

int fd_particles_evaluate_pyramid(fd_ctx* ctx, fd_particles* p, fd_pyramid* pyr, int kind, const void* params, const fd_svm* svm, double aspect_ratio,
                                  const fd_sample_map* maps, int n_maps) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_evaluate_pyramid";
        if (!ctx || !p || !pyr || !params || !svm) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        const FdSampleMaps chain = fd_sample_maps_checked(maps, n_maps, 1u << FD_SAMPLE_MAP_RESIZE, who);
        if (kind != FD_SAMPLES_HIST && kind != FD_SAMPLES_EHOG && kind != FD_SAMPLES_PATCH) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown feature kind %d", who, kind);
        particles_checked(ctx, p, who);
        if (pyr->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: objects belong to different contexts", who);
        fd_pyramid_require_single(pyr, who);
        fd_pyramid_require_image(pyr);
        if (pyr->kept.size() > (size_t)FD_WIN_MAX_LAYERS) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: too many pyramid layers (%zu)", who, pyr->kept.size());
        const int n = p->n;
        const ParticleGen& G = p->gen[p->cur];
        auto score_list = [&](const int32_t* dlist, int* pw, int* ph) {   // dlist NULL: the argument rules alone
            if (kind == FD_SAMPLES_PATCH) fd_patch_samples_score_list(ctx, pyr, (const fd_patch_samples_params*)params, svm, who, dlist, n, G.score, pw, ph);
            else fd_hist_samples_score_list(ctx, pyr, kind, params, svm, who, dlist, n, G.score, pw, ph);
        };
        int pw = 0, ph = 0;
        score_list(nullptr, &pw, &ph);
        particle_windows_table(ctx, pyr, pw, who);
        if (n > 0 && particles_windows(ctx, p, pyr, pw, ph, aspect_ratio, chain)) score_list(p->list.as<int32_t>(), &pw, &ph);
        p->evaluatedBy(nullptr);
    });
}

int fd_particles_evaluate_wvm_svm(fd_ctx* ctx, fd_particles* p, fd_pyramid* pyr, const fd_wvm* wvm, const fd_svm* svm, double aspect_ratio,
                                  const fd_sample_map* maps, int n_maps) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_evaluate_wvm_svm";
        if (!ctx || !p || !pyr || !wvm || !svm) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        particles_checked(ctx, p, who);
        p->notEvaluated();   // a refused call leaves the generation "not evaluated"
        const FdSampleMaps chain = fd_sample_maps_checked(maps, n_maps, 1u << FD_SAMPLE_MAP_RESIZE, who);
        fd_wvm_resident_check(ctx, pyr, wvm, svm, p->n, who);
        fd_pyramid_require_single(pyr, who);
        fd_pyramid_require_image(pyr);
        int pw = 0, ph = 0;
        fd_wvm_patch_size(wvm, &pw, &ph);
        particle_windows_table(ctx, pyr, pw, who);
        const int n = p->n;
        p->wvmCascaded = false;
        if (n > 0 && particles_windows(ctx, p, pyr, pw, ph, aspect_ratio, chain)) {
            fd_wvm_list_launch_resident(ctx, pyr, const_cast<fd_wvm*>(wvm), p->list.as<int32_t>(), n, p->wvmRun);
            p->wvmCascaded = true;
            hipLaunchKernelGGL(k_particles_fout_scores, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, p->wvmRun.fout, n, p->gen[p->cur].score);
            HIP_CHECK(hipGetLastError());
        }
        p->evaluatedBy(wvm);
    });
}

int fd_particles_weigh_wvm_svm(fd_ctx* ctx, fd_particles* p, const fd_wvm* wvm, const fd_svm* svm) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_weigh_wvm_svm";
        if (!ctx || !p || !wvm || !svm) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        particles_checked(ctx, p, who);
        fd_wvm_svm_pair_check(ctx, wvm, svm, who);   // this call's SVM reads the patch rows: the evaluate's check was of its own argument
        if (!p->evaluated || p->wvm != wvm)
            FD_THROW(FD_ERR_RUNTIME, "%s: the generation has not been evaluated by fd_particles_evaluate_wvm_svm with this WVM", who);
        if (p->wvmCascaded && fd_wvm_run_serial(wvm) != p->wvmRun.serial)
            FD_THROW(FD_ERR_RUNTIME, "%s: the WVM handle has run again since fd_particles_evaluate_wvm_svm: the positives of that run are gone", who);
        if (p->n == 0) { p->wvmWeighed = true; return; }
        double wvmA, wvmB, svmA, svmB;
        fd_wvm_logistic(wvm, &wvmA, &wvmB);
        fd_svm_logistic(svm, &svmA, &svmB);
        const bool fresh = !p->wvmSel.p;
        p->wvmSel.reserve(sizeof(ParticleWvmSvmSel));
        if (fresh) HIP_CHECK(hipMemsetAsync(p->wvmSel.p, 0, sizeof(ParticleWvmSvmSel), ctx->stream));
        ParticleWvmSvmSel* sel = p->wvmSel.as<ParticleWvmSvmSel>();
        const FdWvmResidentRun& run = p->wvmRun;
        hipLaunchKernelGGL(k_particles_wvm_svm_select, dim3(1), dim3(PT), 0, ctx->stream, run.pos, p->wvmCascaded ? run.pos_count : nullptr, p->n, p->valid,
                           wvmA, wvmB, sel);
        HIP_CHECK(hipGetLastError());
        // a fixed 8 rows: the unused entries name row 0, which exists, and their distances are never read
        if (p->wvmCascaded) fd_svm_generic_launch(ctx, svm, run.patches, sel->row, (int64_t)run.dim, WVM_SVM_RESCORED, sel->distance);
        hipLaunchKernelGGL(k_particles_wvm_svm_weigh, dim3(1), dim3(PT), 0, ctx->stream, p->gen[p->cur], p->n, p->valid, wvmA, wvmB, svmA, svmB,
                           (double)fd_svm_threshold(svm), sel, p->dinfo.as<fd_particles_info>());
        HIP_CHECK(hipGetLastError());
        p->sumKnown = false;
        p->wvmWeighed = true;
    });
}

int fd_particles_get_wvm_svm_trace(fd_ctx* ctx, fd_particles* p, int* count, int32_t* index, double* distance) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_get_wvm_svm_trace";
        if (!ctx || !p || !count) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
        particles_checked(ctx, p, who);
        if (!p->evaluated || !p->wvm || !p->wvmWeighed)
            FD_THROW(FD_ERR_RUNTIME, "%s: the generation has not been evaluated and weighed by fd_particles_evaluate_wvm_svm / _weigh_wvm_svm", who);
        ParticleWvmSvmSel sel;
        std::memset(&sel, 0, sizeof(sel));
        if (p->n > 0) {
            HIP_CHECK(hipMemcpyAsync(&sel, p->wvmSel.p, sizeof(sel), hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
        *count = sel.count;
        for (int k = 0; k < WVM_SVM_RESCORED; ++k) {
            if (index) index[k] = k < sel.count ? sel.index[k] : -1;
            if (distance) distance[k] = k < sel.count ? sel.distance[k] : 0.0;
        }
    });
}

int fd_particles_weigh(fd_ctx* ctx, fd_particles* p, double logistic_a, double logistic_b, double svm_threshold, int mode, double rejection_threshold) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_weigh");
        if (mode != FD_PARTICLES_TARGET_LOST && mode != FD_PARTICLES_SLIDING_WINDOW && mode != FD_PARTICLES_ALL_TARGETS)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_weigh: unknown mode %d", mode);
        particles_weigh(ctx, p, "fd_particles_weigh", logistic_a, logistic_b, svm_threshold, mode, rejection_threshold);
    });
}

int fd_particles_weigh_classifier(fd_ctx* ctx, fd_particles* p, double logistic_a, double logistic_b, double threshold) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_weigh_classifier");
        particles_weigh(ctx, p, "fd_particles_weigh_classifier", logistic_a, logistic_b, threshold, PARTICLES_CLASSIFIER, 0.0);
    });
}

int fd_particles_state(fd_ctx* ctx, fd_particles* p, fd_particles_info* out) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_state");
        if (!out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_state: NULL argument");
        particles_read_state(ctx, p, out);
        if (out->bad_weight) FD_THROW(FD_ERR_RUNTIME, "fd_particles_state: the generation holds a weight that is negative or not finite");
    });
}

int fd_particles_state_flow(fd_ctx* ctx, fd_particles* p, fd_flow* flow, fd_particles_info* info, fd_flow_motion_info* motion) {
    return fd_guard(ctx, [&] {
        particles_checked(ctx, p, "fd_particles_state_flow");
        if (!flow || !info || !motion) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_particles_state_flow: NULL argument");
        particles_read_state(ctx, p, info, fd_flow_device_motion(ctx, flow, "fd_particles_state_flow"), motion);
        if (info->bad_weight) FD_THROW(FD_ERR_RUNTIME, "fd_particles_state_flow: the generation holds a weight that is negative or not finite");
    });
}

int fd_particles_state_negatives(fd_ctx* ctx, fd_particles* p, fd_flow* flow, const fd_particles_negatives_params* params, fd_particles_info* info,
                                 fd_flow_motion_info* motion, int* count, fd_particles_negative* out) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_state_negatives";
        if (count) *count = 0;
        if (!params || !info || !count || !out || (flow != nullptr) != (motion != nullptr)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
        if (params->max_count < 1 || params->max_count > FD_PARTICLES_NEGATIVES_MAX)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: max_count %d, it must be 1 .. %d", who, params->max_count, FD_PARTICLES_NEGATIVES_MAX);
        if (!std::isfinite(params->offset_factor) || !std::isfinite(params->down_scale) || !std::isfinite(params->up_scale))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the bounds (offset_factor %g, down_scale %g, up_scale %g) must be finite", who, (double)params->offset_factor,
                     (double)params->down_scale, (double)params->up_scale);
        particles_checked(ctx, p, who);
        particles_read_state(ctx, p, info, flow ? fd_flow_device_motion(ctx, flow, who) : nullptr, motion, params, count, out);
        if (info->bad_weight) FD_THROW(FD_ERR_RUNTIME, "%s: the generation holds a weight that is negative or not finite", who);
    });
}

}  // extern "C"

FdParticlesView fd_particles_view(fd_ctx* ctx, fd_particles* p, const char* who) {
    particles_checked(ctx, p, who);
    const ParticleGen& G = p->gen[p->cur];
    return FdParticlesView{p->n, G.x, G.y, G.size, G.score, p->valid, p->windows};
}

void fd_particles_set_evaluated(fd_particles* p) { p->evaluatedBy(nullptr); }

// ---- fd_particles_state_examples_*: the halves around the family's feature kernel (fd_internal.hpp) ----
void fd_particles_examples_check(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, const char* who) {
    if (a.n_pos) *a.n_pos = 0;
    if (a.n_neg) *a.n_neg = 0;
    if (!a.params || !a.info || !a.n_pos || !a.pos || !a.n_neg || !a.neg || !a.rows || (a.flow != nullptr) != (a.motion != nullptr))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    const fd_particles_examples_params& prm = *a.params;
    if (prm.max_count < 1 || prm.max_count > FD_PARTICLES_EXAMPLES_MAX)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: max_count %d, it must be 1 .. %d", who, prm.max_count, FD_PARTICLES_EXAMPLES_MAX);
    if (!std::isfinite(prm.positive_threshold) || !std::isfinite(prm.negative_threshold))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the thresholds (positive %g, negative %g) must be finite", who, prm.positive_threshold, prm.negative_threshold);
    if (prm.negative_threshold > prm.positive_threshold)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: negative_threshold %g lies above positive_threshold %g", who, prm.negative_threshold, prm.positive_threshold);
    if (prm.require_window != 0 && prm.require_window != 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: require_window %d, it must be 0 or 1", who, prm.require_window);
    particles_checked(ctx, p, who);
}

FdExamplesRun fd_particles_examples_begin(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, int rowLength, const char* who) {
    static uint64_t allowed = 0;
    const fd_particles_examples_params& prm = *a.params;
    const long long need = 2LL * prm.max_count * rowLength;
    if (a.row_length) *a.row_length = rowLength;
    if (a.row_capacity < 0 || (long long)a.row_capacity < need)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: row_capacity %d, 2 * max_count (%d) rows of %d floats need %lld", who, a.row_capacity, prm.max_count, rowLength, need);
    const fd_flow_motion_info* dmotion = a.flow ? fd_flow_device_motion(ctx, a.flow, who) : nullptr;
    if (prm.require_window && !p->evaluated)
        FD_THROW(FD_ERR_RUNTIME, "%s: require_window on a generation that has not been evaluated (fd_particles_evaluate*)", who);
    p->examples.reserve(examples_rows_offset() + sizeof(float) * (size_t)need);
    ParticleExamplesHead* head = p->examples.as<ParticleExamplesHead>();
    particles_queue_state(ctx, p);
    fd_allow_lds(ctx, (const void*)k_particles_examples, (int)(sizeof(unsigned long long) * FD_PARTICLES_MAX), allowed);
    hipLaunchKernelGGL(k_particles_examples, dim3(1), dim3(PT), sizeof(unsigned long long) * (size_t)p->n, ctx->stream, p->gen[p->cur], p->valid, p->n, prm,
                       p->dinfo.as<fd_particles_info>(), dmotion, head);
    HIP_CHECK(hipGetLastError());
    return FdExamplesRun{(float*)(p->examples.as<unsigned char>() + examples_rows_offset()), head->rowValid};
}

void fd_particles_examples_xywh(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, double aspect, const FdSampleMaps& chain, int32_t* dxywh) {
    hipLaunchKernelGGL(k_particles_examples_xywh, dim3(1), dim3(2 * FD_PARTICLES_EXAMPLES_MAX), 0, ctx->stream, p->examples.as<ParticleExamplesHead>(),
                       a.params->max_count, aspect, chain, (int4*)dxywh);
    HIP_CHECK(hipGetLastError());
}

void fd_particles_examples_end(fd_ctx* ctx, fd_particles* p, const FdExamplesArgs& a, int rowLength, const char* who) {
    const int K = a.params->max_count;
    const size_t rowBytes = sizeof(float) * (size_t)rowLength, bytes = examples_rows_offset() + rowBytes * 2 * (size_t)K;
    p->examplesHost.resize(bytes);
    HIP_CHECK(hipMemcpyAsync(p->examplesHost.data(), p->examples.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ParticleExamplesHead head;
    std::memcpy(&head, p->examplesHost.data(), sizeof(head));
    const unsigned char* hostRows = p->examplesHost.data() + examples_rows_offset();
    *a.info = head.info;
    if (a.motion) *a.motion = head.motion;
    p->sum = head.info.weight_sum;
    p->sumKnown = true;
    p->bad = head.info.bad_weight != 0;
    if (head.info.bad_weight) FD_THROW(FD_ERR_RUNTIME, "%s: the generation holds a weight that is negative or not finite", who);
    const int nPos = std::min(std::max(head.nPos, 0), K), nNeg = std::min(std::max(head.nNeg, 0), K);
    for (int r = 0; r < nPos + nNeg; ++r) {
        const bool negative = r >= nPos;
        const int k = negative ? r - nPos : r, slot = negative ? K + k : k;
        fd_particles_example rec = negative ? head.neg[k] : head.pos[k];
        rec.valid = head.rowValid[slot] ? 1 : 0;
        (negative ? a.neg : a.pos)[k] = rec;
        if (rec.valid && rowBytes) std::memcpy(a.rows + (size_t)r * rowLength, hostRows + (size_t)slot * rowBytes, rowBytes);
    }
    *a.n_pos = nPos;
    *a.n_neg = nNeg;
}

extern "C" int fd_particles_state_examples_pyramid(fd_ctx* ctx, fd_particles* p, fd_flow* flow, fd_pyramid* pyr, int kind, const void* params,
                                                   double aspect_ratio, const fd_sample_map* maps, int n_maps,
                                                   const fd_particles_examples_params* examples_params, fd_particles_info* info, fd_flow_motion_info* motion,
                                                   int* n_pos, fd_particles_example* pos, int* n_neg, fd_particles_example* neg, float* rows, int row_capacity,
                                                   int* row_length) {
    return fd_guard(ctx, [&] {
        static const char* const who = "fd_particles_state_examples_pyramid";
        if (!ctx || !p || !pyr || !params) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
        const FdExamplesArgs a{flow, examples_params, info, motion, n_pos, n_neg, pos, neg, rows, row_capacity, row_length};
        fd_particles_examples_check(ctx, p, a, who);
        const FdSampleMaps chain = fd_sample_maps_checked(maps, n_maps, 1u << FD_SAMPLE_MAP_RESIZE, who);
        if (kind != FD_SAMPLES_HIST && kind != FD_SAMPLES_EHOG && kind != FD_SAMPLES_PATCH) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown feature kind %d", who, kind);
        if (pyr->ctx != ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: objects belong to different contexts", who);
        fd_pyramid_require_single(pyr, who);
        fd_pyramid_require_image(pyr);
        if (pyr->kept.size() > (size_t)FD_WIN_MAX_LAYERS) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: too many pyramid layers (%zu)", who, pyr->kept.size());
        const int slots = 2 * examples_params->max_count;   // the launch size does not depend on what was chosen
        int len = 0, pw = 0, ph = 0;
        auto features = [&](const int32_t* dlist) {   // dlist NULL: the argument rules alone
            return kind == FD_SAMPLES_PATCH ? fd_patch_samples_features_list(ctx, pyr, (const fd_patch_samples_params*)params, who, dlist, slots, &len, &pw, &ph)
                                            : fd_hist_samples_features_list(ctx, pyr, kind, params, who, dlist, slots, &len, &pw, &ph);
        };
        features(nullptr);
        particle_windows_table(ctx, pyr, pw, who);
        FdSampleWindow spare;
        const ParticleLayers layers = particle_layers(pyr, pw, ph, spare);
        p->exampleList.reserve(sizeof(int32_t) * 3 * 2 * FD_PARTICLES_EXAMPLES_MAX);
        const FdExamplesRun run = fd_particles_examples_begin(ctx, p, a, len, who);
        hipLaunchKernelGGL(k_particles_examples_windows, dim3(1), dim3(2 * FD_PARTICLES_EXAMPLES_MAX), 0, ctx->stream, p->examples.as<ParticleExamplesHead>(),
                           examples_params->max_count, aspect_ratio, chain, layers, pyr->sample_table.dev.as<int16_t>(), pyr->sample_table.length, pw, ph, spare,
                           p->exampleList.as<int32_t>(), run.valid);
        HIP_CHECK(hipGetLastError());
        if (spare.layer >= 0) {   // otherwise no kept layer holds a window: every slot is invalid and the list must not be read
            const float* dfeat = features(p->exampleList.as<int32_t>());
            if (len > 0) HIP_CHECK(hipMemcpyAsync(run.rows, dfeat, sizeof(float) * (size_t)len * slots, hipMemcpyDeviceToDevice, ctx->stream));
        }
        fd_particles_examples_end(ctx, p, a, len, who);
    });
}
