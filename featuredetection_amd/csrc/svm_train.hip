// featuredetection_amd/csrc/svm_train.hip -- linear C-SVC training on the device, libsvm's model bit for bit on a given Q
// (DESIGN.md section 4.6).  What ExtendedHogBasedMeasurementModel's adaptation needs of libsvm::LibSvmClassifier::train
// (LibSvmClassifier.cpp:156-189, libSvm/src/svm.cpp Solver::Solve :551-830 without shrinking, select_working_set :833-930,
// calculate_rho :1013-1049, LibSvmUtils::extractSupportVectors LibSvmUtils.cpp:105-118).
//
//   k_svm_gram<LINEAR>   K = X X^T on the f64 MFMA pipe (f32 products are exact in f64), Q_ij = (float)(y_i y_j K_ij), QD_i = K_ii;
//                 also the start state alpha = 0, G = -1
//   k_svm_smo     one workgroup per problem: a counted loop of SMO iterations over a per-launch budget; alpha, G, the iteration
//                 count and the converged flag persist in global memory between launches (the host relaunches)
//   k_svm_smo_large   the same for up to 16384 examples: 1024 threads, G and a status byte per element
//                 in LDS, alpha in memory; the arithmetic, the block reductions and the slot layout are shared with k_svm_smo
//   k_svm_finish<Staged, false>   rho, the objective and the support-vector counts (one thread, libsvm's summation order), and
//                 the single weight vector, one thread per dimension.  Staged: alpha and G of a problem of k_svm_smo go through
//                 LDS; one of k_svm_smo_large is read from memory
//
//
// The same solver on the Q of a polynomial, RBF or histogram-intersection kernel, with the model returned as support vectors and
// coefficients (fd_kernel_svm_*; Kernel::kernel_poly / kernel_rbf / kernel_hik svm.cpp:235-273, svm_train's
// two-class model, LibSvmUtils::extractCoefficients):
//   k_svm_gram<POLY>, <RBF>   the same dot tile with an epilogue in double: powi(gamma dot + coef0, degree) or
//                       exp(-gamma ((xs_i + xs_j) - 2 dot)); xs comes from a first launch over the diagonal tiles
//                       (k_svm_gram<SVM_GRAM_XS>), so that the diagonal of the second launch subtracts the very same sum and
//                       K_ii = 1 exactly
//   k_svm_gram_hik      sum_k min(x_ik, x_jk) in double with k ascending (libsvm's order: Q and QD are libsvm's bits), the operand
//                       tiles staged through LDS
//   k_svm_finish<Staged, true>   rho, objective, counts as above, and in the same pass the support-vector indices and
//                       (float)(alpha_i y_i); no weight vector
//   k_svm_gather_sv     the support vectors' rows into a dense [n_sv][d] buffer
//
// One-class models and libsvm's sigmoid fit for a C-SVC (fd_one_class_svm_*, fd_kernel_svm_cv_sigmoid, DESIGN.md section 4.11;
// solve_one_class svm.cpp:1577-1607, svm_binary_svc_probability :1940-2024, k_function :342-420, sigmoid_train :1752-1863):
//   k_svm_one_class_start   behind the Gram of a problem of positives: libsvm's start state for nu and its gradient, summed as
//                       Solver::Solve does; the solvers and the finish follow unchanged (the linear term is in the descriptor)
//   k_svm_gather_rows   a cross-validation fold's rows into the fold's block; the five folds then train as one batch
//   k_svm_cv_decision<Kernel>   the held-out examples' decision values in double, k_function's and svm_predict_values' order
// The Newton fit on the decision values is host code (svm_sigmoid_train, libm's exp and log).
//
// A problem is n_pos positive rows followed by n_neg negative rows, so y_i = +1 for i < n_pos and libsvm's class grouping is the
// identity; the bound status is alpha compared with 0 and C as update_alpha_status does.
#include "fd_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SVM_MAX_N = 1024;
constexpr int SVM_SMO_THREADS = 256;
constexpr int SVM_SMO_WAVES = SVM_SMO_THREADS / 64;
constexpr size_t SVM_LDS_BUDGET = 160 * 1024;     // LDS of one gfx950 workgroup
constexpr int SVM_SLOT_BYTES = 512;               // the reduction slots of k_svm_smo
constexpr int SVM_DEFAULT_LAUNCH_ITERATIONS = 16384;
constexpr double SVM_TAU = 1e-12;
// the large solver (fd_linear_svm_train_large)
constexpr int SVM_LARGE_MAX_N = FD_SVM_LARGE_MAX_N;
constexpr int SVM_LARGE_THREADS = 1024;
constexpr int SVM_LARGE_WAVES = SVM_LARGE_THREADS / 64;
constexpr int SVM_LARGE_U = 4;                // elements of a thread whose loads are issued together
constexpr int SVM_LARGE_SLOT_BYTES = 1024;

struct SvmProbDev {
    const float* x;            // n x d, row-major
    float* Q;                  // n_pad x n_pad
    double* QD;                // n_pad
    double* alpha;             // n_pad
    double* G;                 // n_pad
    float* w;                  // d
    fd_svm_train_info* info;
    int32_t* state;            // [0] iterations, [1] converged
    double Cp, Cn, eps;
    int32_t n_pos, n, n_pad, d, q_in_lds, max_iter;
    // the support-vector form (fd_kernel_svm_*) only
    double* xs;                // n_pad: x_i . x_i of the RBF kernel
    int32_t* sv_index;         // n: the examples with alpha > 0, ascending
    float* coef;               // n: (float)(alpha_i y_i) of these
    float* sv;                 // n x d: their rows; NULL when not asked for
    double gamma, coef0;       // of the polynomial and RBF kernels; the host picks the kernel's instantiation of k_svm_gram
    int32_t degree;
    // the linear term p of the dual, the same for every example: -1 (C-SVC), 0 (one-class)
    double lin;
    // one-class only (solve_one_class): alpha_i = 1 for i < oc_full, alpha_oc_full = oc_frac, 0 behind
    int32_t oc_full;
    double oc_frac;
};

// The LDS slots of a solver: per wavefront what either block reduction leaves, and for k_svm_smo_large (Pub = 4) the pair's
// alpha_i, G_i, alpha_j, G_j that their owners publish.  The LDS formulas below reserve SVM_SLOT_BYTES / SVM_LARGE_SLOT_BYTES.
template <int Waves, int Pub>
struct SvmSlots {
    double av[Waves];    // Gmax of a wavefront
    double bv[Waves];    // its smallest obj_diff
    double bg[Waves];    // its Gmax2
    double pub[Pub];
    int ai[Waves], bi[Waves];
};
typedef SvmSlots<SVM_SMO_WAVES, 0> SvmSmoSlots;
typedef SvmSlots<SVM_LARGE_WAVES, 4> SvmLargeSlots;
static_assert(sizeof(SvmSmoSlots) <= SVM_SLOT_BYTES && sizeof(SvmLargeSlots) <= SVM_LARGE_SLOT_BYTES, "the slots outgrow their LDS reserve");

inline int svm_pad(int n) { return (n + 15) / 16 * 16; }
inline size_t svm_smo_lds(int n, bool withQ) {
    const size_t np = (size_t)svm_pad(n);
    return 3 * sizeof(double) * np + SVM_SLOT_BYTES + (withQ ? sizeof(float) * np * np : 0);
}
inline size_t svm_large_lds(int n) { return (sizeof(double) + 1) * (size_t)svm_pad(n) + SVM_LARGE_SLOT_BYTES; }   // G, status, slots
inline bool svm_q_in_lds(int n) { return svm_smo_lds(n, true) <= SVM_LDS_BUDGET; }

// One wavefront per 16 x 16 tile of K, the whole feature length: lane (r, kq) feeds row r of both operand tiles at feature
// k + kq.  Rows from n up to n_pad read as zero.  The result is in the C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15,
// row = (lane >> 4) + 4 * reg.
__device__ __forceinline__ f64x4 svm_dot_tile(const SvmProbDev& p, int ti, int tj) {
    const int lane = threadIdx.x, r = lane & 15, kq = lane >> 4;
    const int i = ti * 16 + r, j = tj * 16 + r;
    const bool iok = i < p.n, jok = j < p.n;
    const float* __restrict__ xi = p.x + (size_t)(iok ? i : 0) * p.d;
    const float* __restrict__ xj = p.x + (size_t)(jok ? j : 0) * p.d;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    constexpr int U = 4;   // k-steps whose loads are issued together
    for (int k = 0; k < p.d; k += 4 * U) {
        float a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = k + 4 * u + kq;
            const bool kok = kk < p.d;
            const int kc = kok ? kk : 0;   // in-range address for the masked lanes
            a[u] = xi[kc];
            b[u] = xj[kc];
            a[u] = (iok && kok) ? a[u] : 0.f;
            b[u] = (jok && kok) ? b[u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[u], (double)b[u], acc, 0, 0, 0);
    }
    return acc;
}

// Q_ij = (float)(y_i y_j K_ij) of a tile, QD and the start state on the diagonal
__device__ __forceinline__ void svm_store_tile(const SvmProbDev& p, int ti, int tj, const double (&K)[4]) {
    const int lane = threadIdx.x, col = tj * 16 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = ti * 16 + (lane >> 4) + 4 * q;
        const bool same = (row < p.n_pos) == (col < p.n_pos);
        p.Q[(size_t)row * p.n_pad + col] = (float)(same ? K[q] : -K[q]);
        if (row == col) {
            p.QD[row] = K[q];
            p.alpha[row] = 0.0;
            p.G[row] = -1.0;
        }
    }
}

// powi of svm.cpp:26
__device__ __forceinline__ double svm_powi(double base, int times) {
    double tmp = base, ret = 1.0;
    for (int t = times; t > 0; t /= 2) {
        if (t % 2 == 1) ret *= tmp;
        tmp = tmp * tmp;
    }
    return ret;
}

// Linear, polynomial and RBF kernel on the dot tile, one instantiation each (the host picks it), and the xs pass of the RBF
// kernel.  SVM_GRAM_XS: the diagonal tiles only (blockIdx.x), which write xs_i = x_i . x_i and nothing else; the launch over all
// tiles that follows accumulates its diagonal in the same order, so that (xs_i + xs_i) - 2 dot_ii = 0 and K_ii = exp(-0) = 1
// exactly, as where x_square and dot are one function.  The padding is written as zero: the zero rows make it so for the linear
// kernel, which neither loads xs nor masks; a polynomial or RBF kernel of the zero rows is not zero.
constexpr int SVM_GRAM_XS = -1;
template <int Kernel>   // FD_KERNEL_LINEAR, FD_KERNEL_POLY, FD_KERNEL_RBF or SVM_GRAM_XS
__global__ __launch_bounds__(64) void k_svm_gram(const SvmProbDev* __restrict__ P) {
    const SvmProbDev p = P[blockIdx.z];
    const int ti = Kernel == SVM_GRAM_XS ? blockIdx.x : blockIdx.y, tj = blockIdx.x;
    if (ti * 16 >= p.n_pad || tj * 16 >= p.n_pad) return;
    const f64x4 acc = svm_dot_tile(p, ti, tj);
    const int lane = threadIdx.x, col = tj * 16 + (lane & 15);
    if (Kernel == SVM_GRAM_XS) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (ti * 16 + (lane >> 4) + 4 * q == col) p.xs[col] = acc[q];
        return;
    }
    double K[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = ti * 16 + (lane >> 4) + 4 * q;
        double v = acc[q];
        if (Kernel == FD_KERNEL_POLY) v = svm_powi(p.gamma * v + p.coef0, p.degree);
        if (Kernel == FD_KERNEL_RBF) v = exp(-p.gamma * ((p.xs[row] + p.xs[col]) - 2.0 * v));
        K[q] = (Kernel == FD_KERNEL_LINEAR || (row < p.n && col < p.n)) ? v : 0.0;
    }
    svm_store_tile(p, ti, tj, K);
}

// The histogram-intersection kernel: one wavefront per 16 x 16 tile, lane (c, kq) owns the entries (kq + 4 q, c) as in the MFMA
// layout.  Chunks of SVM_HIK_KC features of the two operand tiles go through LDS (rows padded by one word: the 16 columns of a
// read fall into 16 banks); per feature a lane takes the minimum (exact), converts and adds in double, k ascending as
// kernel_hik does.  Rows from n up to n_pad read row 0 and are written as zero.
constexpr int SVM_HIK_KC = 64;
__global__ __launch_bounds__(64) void k_svm_gram_hik(const SvmProbDev* __restrict__ P) {
    __shared__ float sA[16][SVM_HIK_KC + 1], sB[16][SVM_HIK_KC + 1];
    const SvmProbDev p = P[blockIdx.z];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti * 16 >= p.n_pad || tj * 16 >= p.n_pad) return;
    const int lane = threadIdx.x, c = lane & 15, kq = lane >> 4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < p.d; k0 += SVM_HIK_KC) {
        const int kn = min(SVM_HIK_KC, p.d - k0);
        const int kc = k0 + (lane < kn ? lane : 0);   // in-range address for the masked lanes
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ti * 16 + r, j = tj * 16 + r;
            sA[r][lane] = p.x[(size_t)(i < p.n ? i : 0) * p.d + kc];
            sB[r][lane] = p.x[(size_t)(j < p.n ? j : 0) * p.d + kc];
        }
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            const float b = sB[c][k];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float a = sA[kq + 4 * q][k];
                acc[q] += (double)(b < a ? b : a);   // min<double>(x_ik, x_jk)
            }
        }
        __syncthreads();
    }
    const int col = tj * 16 + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = ti * 16 + kq + 4 * q;
        if (row >= p.n || col >= p.n) acc[q] = 0.0;
    }
    svm_store_tile(p, ti, tj, acc);
}

// The start state of a one-class problem (solve_one_class svm.cpp:1586-1593 and the gradient Solver::Solve builds from it
// :571-588), behind the Gram launch, which ran as for n_pos = n: alpha_i = 1 for i < oc_full, oc_frac at oc_full, 0 behind, and
// G_j = 0 + sum over the i with alpha_i > 0, ascending, of alpha_i * (double)Q_ij -- a product, then a sum, as G[j] += alpha_i *
// Q_i[j] is.  One thread per j: consecutive threads read consecutive floats of row i.
__global__ __launch_bounds__(256) void k_svm_one_class_start(const SvmProbDev* __restrict__ P) {
    const SvmProbDev p = P[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= p.n) return;
    const double aj = j < p.oc_full ? 1.0 : (j == p.oc_full ? p.oc_frac : 0.0);
    double g = p.lin;
    const int last = min(p.oc_full, p.n - 1);   // the last i whose alpha can be positive
    for (int i = 0; i <= last; ++i) {
        const double ai = i < p.oc_full ? 1.0 : p.oc_frac;
        if (ai > 0.0) g += ai * (double)p.Q[(size_t)i * p.n_pad + j];
    }
    p.alpha[j] = aj;
    p.G[j] = g;
}

// (value, index) of the larger value, ties to the higher index: what a scan in index order with >= leaves
__device__ __forceinline__ void svm_take_max(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi > i)) { v = ov; i = oi; }
}
// the smaller value, ties to the higher index (a scan with <=)
__device__ __forceinline__ void svm_take_min(double& v, int& i, double ov, int oi) {
    if (ov < v || (ov == v && oi > i)) { v = ov; i = oi; }
}

// The two block reductions of a solver: over the wavefront by shuffles, over the wavefronts through the LDS slots, after which
// every thread holds the result.  One barrier each.
// the larger (v, i), ties to the higher index
template <int Waves, int Pub>
__device__ __forceinline__ void svm_block_argmax(SvmSlots<Waves, Pub>& s, double& v, int& i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) svm_take_max(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
    if (lane == 0) { s.av[wave] = v; s.ai[wave] = i; }
    __syncthreads();
    v = s.av[0];
    i = s.ai[0];
#pragma unroll
    for (int w = 1; w < Waves; ++w) svm_take_max(v, i, s.av[w], s.ai[w]);
}
// the smaller (v, i), ties to the higher index, and the maximum of g
template <int Waves, int Pub>
__device__ __forceinline__ void svm_block_argmin_max(SvmSlots<Waves, Pub>& s, double& v, int& i, double& g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        svm_take_min(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
        g = fmax(g, __shfl_xor(g, o, 64));
    }
    if (lane == 0) { s.bv[wave] = v; s.bi[wave] = i; s.bg[wave] = g; }
    __syncthreads();
    v = s.bv[0];
    i = s.bi[0];
    g = s.bg[0];
#pragma unroll
    for (int w = 1; w < Waves; ++w) {
        svm_take_min(v, i, s.bv[w], s.bi[w]);
        g = fmax(g, s.bg[w]);
    }
}

// A problem that is done, converged or at max_iterations, in an earlier launch (a batch relaunches until its last problem is
// done): the solvers leave it alone, the finish reports it
__device__ __forceinline__ bool svm_done(const SvmProbDev& p) { return p.state[1] || p.state[0] >= p.max_iter; }
// what a solver leaves for the next launch and the finish, besides alpha and G
__device__ __forceinline__ void svm_store_state(const SvmProbDev& p, int iter, int converged) {
    if (threadIdx.x == 0) {
        p.state[0] = iter;
        p.state[1] = converged;
    }
}
// the stopping test of Solve: optimal (without a pair only when the Gram holds a NaN)
__device__ __forceinline__ bool svm_optimal(double gmax, double gmax2, double eps, int i, int j) { return gmax + gmax2 < eps || i < 0 || j < 0; }

// The element-wise steps of Solver::Solve, shared by k_svm_smo and k_svm_smo_large.
// i: element k in the scan that maximises -y_t G_t over I_up, the highest index among equals (:847-865); inUp: alpha_k below its
// bound (positives) / above zero (negatives)
__device__ __forceinline__ void svm_scan_i(int k, bool pos, bool inUp, double g, double& gmax, int& gi) {
    if (pos) {
        if (inUp && -g >= gmax) { gmax = -g; gi = k; }
    } else {
        if (inUp && g >= gmax) { gmax = g; gi = k; }
    }
}
// j: element k in the scan that minimises obj_diff over I_low with grad_diff > 0, the highest index among equals; Gmax2 on the
// way (:872-922).  inLow: alpha_k above zero (positives) / below its bound (negatives).  Qik is read only for the elements that
// need it.
template <typename QikF>
__device__ __forceinline__ void svm_scan_j(int k, bool pos, bool inLow, double g, double gmax, double yi, double QDi, double QDk, QikF Qik,
                                           double& gmax2, double& omin, int& gj) {
    if (pos) {
        if (inLow) {
            const double gd = gmax + g;
            if (g >= gmax2) gmax2 = g;
            if (gd > 0.0) {
                const double quad = QDi + QDk - 2.0 * yi * Qik();
                const double od = quad > 0.0 ? -(gd * gd) / quad : -(gd * gd) / SVM_TAU;
                if (od <= omin) { gj = k; omin = od; }
            }
        }
    } else {
        if (inLow) {
            const double gd = gmax - g;
            if (-g >= gmax2) gmax2 = -g;
            if (gd > 0.0) {
                const double quad = QDi + QDk + 2.0 * yi * Qik();
                const double od = quad > 0.0 ? -(gd * gd) / quad : -(gd * gd) / SVM_TAU;
                if (od <= omin) { gj = k; omin = od; }
            }
        }
    }
}
// the two-variable update with its clipping (:640-734): the new alpha_i, alpha_j in ai, aj
__device__ __forceinline__ void svm_pair_update(bool ipos, bool jpos, double Ci, double Cj, double QDi, double QDj, float Qij, double Gi, double Gj,
                                                double& ai, double& aj) {
    if (ipos != jpos) {
        double quad = QDi + QDj + (double)(2.f * Qij);
        if (quad <= 0.0) quad = SVM_TAU;
        const double delta = (-Gi - Gj) / quad;
        const double diff = ai - aj;
        ai += delta;
        aj += delta;
        if (diff > 0.0) {
            if (aj < 0.0) { aj = 0.0; ai = diff; }
        } else {
            if (ai < 0.0) { ai = 0.0; aj = -diff; }
        }
        if (diff > Ci - Cj) {
            if (ai > Ci) { ai = Ci; aj = Ci - diff; }
        } else {
            if (aj > Cj) { aj = Cj; ai = Cj + diff; }
        }
    } else {
        double quad = QDi + QDj - (double)(2.f * Qij);
        if (quad <= 0.0) quad = SVM_TAU;
        const double delta = (Gi - Gj) / quad;
        const double sum = ai + aj;
        ai -= delta;
        aj += delta;
        if (sum > Ci) {
            if (ai > Ci) { ai = Ci; aj = sum - Ci; }
        } else {
            if (aj < 0.0) { aj = 0.0; ai = sum; }
        }
        if (sum > Cj) {
            if (aj > Cj) { aj = Cj; ai = sum - Cj; }
        } else {
            if (ai < 0.0) { ai = 0.0; aj = sum; }
        }
    }
}

// Solver::Solve's loop.  Every thread owns the elements tid, tid + 256, ...; the two selections are reduced over the block
// (svm_block_argmax, svm_block_argmin_max), after which every thread holds i, j and performs the two-variable update redundantly.  Three barriers per iteration: behind either selection, and between reading alpha / G of
// (i, j) and their owners' writes.
__global__ __launch_bounds__(SVM_SMO_THREADS) void k_svm_smo(const SvmProbDev* __restrict__ P, int budget) {
    extern __shared__ double svm_lds[];
    const SvmProbDev p = P[blockIdx.x];
    if (svm_done(p)) return;
    const int tid = threadIdx.x;
    const int n = p.n, np = p.n_pad, n_pos = p.n_pos;
    double* sAlpha = svm_lds;
    double* sG = sAlpha + np;
    double* sQD = sG + np;
    SvmSmoSlots& slots = *(SvmSmoSlots*)(sQD + np);
    float* sQ = (float*)((char*)(sQD + np) + SVM_SLOT_BYTES);
    for (int k = tid; k < np; k += SVM_SMO_THREADS) {
        sAlpha[k] = p.alpha[k];
        sG[k] = p.G[k];
        sQD[k] = p.QD[k];
    }
    if (p.q_in_lds)
        for (int k = tid; k < np * np; k += SVM_SMO_THREADS) sQ[k] = p.Q[k];
    const float* __restrict__ Qbase = p.q_in_lds ? sQ : p.Q;
    __syncthreads();
    const double Cp = p.Cp, Cn = p.Cn, eps = p.eps;
    int iter = p.state[0];
    int converged = 0;
    for (int it = 0; it < budget; ++it) {
        if (iter >= p.max_iter) break;
        // i: maximises -y_t G_t over I_up, the highest index among equals (:847-865)
        double gmax = -INFINITY;
        int gi = -1;
        for (int k = tid; k < n; k += SVM_SMO_THREADS)
            svm_scan_i(k, k < n_pos, k < n_pos ? sAlpha[k] < Cp : sAlpha[k] > 0.0, sG[k], gmax, gi);
        svm_block_argmax(slots, gmax, gi);
        const int i = gi;
        // j: minimises obj_diff over I_low with grad_diff > 0, the highest index among equals; Gmax2 on the way (:872-922)
        double gmax2 = -INFINITY, omin = INFINITY;
        int gj = -1;
        if (i >= 0) {
            const double yi = i < n_pos ? 1.0 : -1.0, QDi = sQD[i];
            const float* __restrict__ Qi = Qbase + (size_t)i * np;
            for (int k = tid; k < n; k += SVM_SMO_THREADS)
                svm_scan_j(k, k < n_pos, k < n_pos ? sAlpha[k] > 0.0 : sAlpha[k] < Cn, sG[k], gmax, yi, QDi, sQD[k], [&] { return Qi[k]; }, gmax2, omin, gj);
        }
        svm_block_argmin_max(slots, omin, gj, gmax2);
        const int j = gj;
        if (svm_optimal(gmax, gmax2, eps, i, j)) {
            converged = 1;
            break;
        }
        ++iter;
        const float* __restrict__ Qi = Qbase + (size_t)i * np;
        const float* __restrict__ Qj = Qbase + (size_t)j * np;
        const bool ipos = i < n_pos, jpos = j < n_pos;
        const double Ci = ipos ? Cp : Cn, Cj = jpos ? Cp : Cn;
        const double oldAi = sAlpha[i], oldAj = sAlpha[j], Gi = sG[i], Gj = sG[j];
        double ai = oldAi, aj = oldAj;
        svm_pair_update(ipos, jpos, Ci, Cj, sQD[i], sQD[j], Qi[j], Gi, Gj, ai, aj);
        const double dai = ai - oldAi, daj = aj - oldAj;
        __syncthreads();   // every thread has read alpha and G of (i, j)
        if (tid == (i & (SVM_SMO_THREADS - 1))) sAlpha[i] = ai;
        if (tid == (j & (SVM_SMO_THREADS - 1))) sAlpha[j] = aj;
        for (int k = tid; k < n; k += SVM_SMO_THREADS) sG[k] += (double)Qi[k] * dai + (double)Qj[k] * daj;   // (:741-744)
    }
    // the loop's last writes are their owners' own elements: no barrier needed before the owners store them
    for (int k = tid; k < n; k += SVM_SMO_THREADS) {
        p.alpha[k] = sAlpha[k];
        p.G[k] = sG[k];
    }
    svm_store_state(p, iter, converged);
}

// k_svm_smo for up to SVM_LARGE_MAX_N examples: one workgroup of 1024 threads per problem, thread t owns the elements t,
// t + 1024, ... (at most 16).  G lives in LDS (8 n bytes, 128 KB at the limit) next to one status byte per element, the two set
// memberships the selections ask of alpha (libsvm's alpha_status; 16 KB).  alpha itself stays in global memory and is touched by
// the owners of i and j only; QD and the rows of Q are read through the cache.  The owners of i and j publish alpha and G of the
// pair through LDS slots, so that an iteration has three barriers as in k_svm_smo: behind either selection and behind the
// publication.  The arithmetic, the reductions and the slots are k_svm_smo's.
// The iteration loop is written out a second time on purpose: where alpha, G, QD and Q live, how the pair is fetched around the
// third barrier, and eager loads four at a time against the lazy Qik are the design; a hook for each would outweigh the lines saved.
__global__ __launch_bounds__(SVM_LARGE_THREADS) void k_svm_smo_large(const SvmProbDev* __restrict__ P, int budget) {
    extern __shared__ double svm_lds[];
    const SvmProbDev p = P[blockIdx.x];
    if (svm_done(p)) return;
    const int tid = threadIdx.x;
    const int n = p.n, np = p.n_pad, n_pos = p.n_pos;
    double* sG = svm_lds;
    SvmLargeSlots& slots = *(SvmLargeSlots*)(sG + np);
    double* pub = slots.pub;   // alpha_i, G_i, alpha_j, G_j
    uint8_t* sStatus = (uint8_t*)(sG + np) + SVM_LARGE_SLOT_BYTES;   // [np] bit 0: in I_up, bit 1: in I_low
    const float* __restrict__ Q = p.Q;
    const double* __restrict__ QD = p.QD;
    const double Cp = p.Cp, Cn = p.Cn, eps = p.eps;
    auto status_of = [&](int k, double a) { return (uint8_t)(k < n_pos ? (a < Cp ? 1 : 0) | (a > 0.0 ? 2 : 0) : (a > 0.0 ? 1 : 0) | (a < Cn ? 2 : 0)); };
    for (int k = tid; k < n; k += SVM_LARGE_THREADS) {
        sG[k] = p.G[k];
        sStatus[k] = status_of(k, p.alpha[k]);
    }
    __syncthreads();
    int iter = p.state[0];
    int converged = 0;
    for (int it = 0; it < budget; ++it) {
        if (iter >= p.max_iter) break;
        double gmax = -INFINITY;
        int gi = -1;
        for (int k = tid; k < n; k += SVM_LARGE_THREADS) svm_scan_i(k, k < n_pos, (sStatus[k] & 1) != 0, sG[k], gmax, gi);
        svm_block_argmax(slots, gmax, gi);
        const int i = gi;
        double gmax2 = -INFINITY, omin = INFINITY;
        int gj = -1;
        if (i >= 0) {
            const double yi = i < n_pos ? 1.0 : -1.0, QDi = QD[i];
            const float* __restrict__ Qi = Q + (size_t)i * np;
            if ((i & (SVM_LARGE_THREADS - 1)) == tid) { pub[0] = p.alpha[i]; pub[1] = sG[i]; }
            for (int k0 = tid; k0 < n; k0 += SVM_LARGE_U * SVM_LARGE_THREADS) {
                float qi[SVM_LARGE_U];
                double qd[SVM_LARGE_U];
#pragma unroll
                for (int u = 0; u < SVM_LARGE_U; ++u) {   // the loads of a step, in flight together (in-range address for the masked lanes)
                    const int k = k0 + u * SVM_LARGE_THREADS, kc = k < n ? k : 0;
                    qi[u] = Qi[kc];
                    qd[u] = QD[kc];
                }
#pragma unroll
                for (int u = 0; u < SVM_LARGE_U; ++u) {
                    const int k = k0 + u * SVM_LARGE_THREADS;
                    if (k < n) svm_scan_j(k, k < n_pos, (sStatus[k] & 2) != 0, sG[k], gmax, yi, QDi, qd[u], [&] { return qi[u]; }, gmax2, omin, gj);
                }
            }
        }
        svm_block_argmin_max(slots, omin, gj, gmax2);
        const int j = gj;
        if (svm_optimal(gmax, gmax2, eps, i, j)) {
            converged = 1;
            break;
        }
        ++iter;
        const float* __restrict__ Qi = Q + (size_t)i * np;
        const float* __restrict__ Qj = Q + (size_t)j * np;
        const float Qij = Qi[j];
        const double QDi = QD[i], QDj = QD[j];
        if ((j & (SVM_LARGE_THREADS - 1)) == tid) { pub[2] = p.alpha[j]; pub[3] = sG[j]; }
        __syncthreads();   // the pair's alpha and G are published; nobody writes G before everybody holds them
        const bool ipos = i < n_pos, jpos = j < n_pos;
        const double Ci = ipos ? Cp : Cn, Cj = jpos ? Cp : Cn;
        const double oldAi = pub[0], Gi = pub[1], oldAj = pub[2], Gj = pub[3];
        double ai = oldAi, aj = oldAj;
        svm_pair_update(ipos, jpos, Ci, Cj, QDi, QDj, Qij, Gi, Gj, ai, aj);
        const double dai = ai - oldAi, daj = aj - oldAj;
        if ((i & (SVM_LARGE_THREADS - 1)) == tid) { p.alpha[i] = ai; sStatus[i] = status_of(i, ai); }
        if ((j & (SVM_LARGE_THREADS - 1)) == tid) { p.alpha[j] = aj; sStatus[j] = status_of(j, aj); }
        for (int k0 = tid; k0 < n; k0 += SVM_LARGE_U * SVM_LARGE_THREADS) {
            float qi[SVM_LARGE_U], qj[SVM_LARGE_U];
#pragma unroll
            for (int u = 0; u < SVM_LARGE_U; ++u) {
                const int k = k0 + u * SVM_LARGE_THREADS, kc = k < n ? k : 0;
                qi[u] = Qi[kc];
                qj[u] = Qj[kc];
            }
#pragma unroll
            for (int u = 0; u < SVM_LARGE_U; ++u) {
                const int k = k0 + u * SVM_LARGE_THREADS;
                if (k < n) sG[k] += (double)qi[u] * dai + (double)qj[u] * daj;   // (:741-744)
            }
        }
    }
    // a thread's last writes to G are its own elements; alpha is in memory already
    for (int k = tid; k < n; k += SVM_LARGE_THREADS) p.G[k] = sG[k];
    svm_store_state(p, iter, converged);
}

// The pieces of k_svm_finish.  Only for a problem that is done (converged or at max_iterations); for one that the solver goes on
// with in the next launch the host needs the progress only.
__device__ __forceinline__ bool svm_finish_pending(const SvmProbDev& p, bool first) {
    if (svm_done(p)) return false;
    if (first) {
        fd_svm_train_info out = {};
        out.iterations = p.state[0];
        *p.info = out;
    }
    return true;
}
// w_k = sum over the support vectors, in index order, of (float)(alpha_i y_i * (double)x_ik) accumulated in float
// (extractSupportVectors, CV_32F)
__device__ __forceinline__ void svm_finish_weight(const SvmProbDev& p, int k) {
    if (k >= p.d) return;
    float w = 0.f;
    const float* __restrict__ xk = p.x + k;
    for (int i = 0; i < p.n; ++i) {
        const double a = p.alpha[i];
        if (a > 0.0) {
            const double coef = i < p.n_pos ? a : -a;
            w += (float)(coef * (double)xk[(size_t)i * p.d]);
        }
    }
    p.w[k] = w;
}
// rho, the objective and the counts by one thread; the sums run in index order as calculate_rho's and Solve's do.  EmitSv: the
// pass also lists the support vectors, ascending, with their coefficients (float)(alpha_i y_i) (svm_train's model for two classes,
// extractCoefficients)
template <bool EmitSv>
__device__ __forceinline__ void svm_finish_info(const SvmProbDev& p, const double* sA, const double* sGf) {
    const int n = p.n, n_pos = p.n_pos;
    double ub = INFINITY, lb = -INFINITY, sumFree = 0.0, obj = 0.0;
    int nFree = 0, nSv = 0, nBounded = 0;
    for (int i = 0; i < n; ++i) {
        const bool pos = i < n_pos;
        const double a = sA[i], g = sGf[i], C = pos ? p.Cp : p.Cn;
        const double yG = pos ? g : -g;
        if (a >= C) {
            if (!pos) ub = fmin(ub, yG);
            else lb = fmax(lb, yG);
        } else if (a <= 0.0) {
            if (pos) ub = fmin(ub, yG);
            else lb = fmax(lb, yG);
        } else {
            ++nFree;
            sumFree += yG;
        }
        obj += a * (g + p.lin);
        if (a > 0.0) {
            if (EmitSv) {
                p.sv_index[nSv] = i;
                p.coef[nSv] = (float)(pos ? a : -a);
            }
            ++nSv;
            if (a >= C) ++nBounded;
        }
    }
    fd_svm_train_info out;
    out.iterations = p.state[0];
    out.converged = p.state[1];
    out.n_sv = nSv;
    out.n_bounded = nBounded;
    out.launches = 0;   // the host's count
    out.rho = nFree > 0 ? sumFree / nFree : (ub + lb) / 2;
    out.objective = obj / 2;
    *p.info = out;
}

// The finish of a problem (blockIdx.y).  The weight-vector form: the single weight vector, one thread per dimension over the
// blocks along x, and rho, objective and counts by thread 0 of the first block.  SvForm: one block, no weight vector; the
// sequential pass also writes sv_index and coef.  Staged: alpha and G go through LDS for the one thread (a problem of k_svm_smo,
// at most SVM_MAX_N examples); one of k_svm_smo_large is read from memory.
template <bool Staged, bool SvForm>
__global__ __launch_bounds__(256) void k_svm_finish(const SvmProbDev* __restrict__ P) {
    __shared__ double sA[Staged ? SVM_MAX_N : 1], sGf[Staged ? SVM_MAX_N : 1];
    const SvmProbDev p = P[blockIdx.y];
    const int tid = threadIdx.x, n = p.n;
    if (svm_finish_pending(p, blockIdx.x == 0 && tid == 0)) return;
    if (!SvForm) svm_finish_weight(p, blockIdx.x * 256 + tid);
    if (blockIdx.x != 0) return;
    if (Staged) {
        for (int i = tid; i < n; i += 256) {
            sA[i] = p.alpha[i];
            sGf[i] = p.G[i];
        }
        __syncthreads();
    }
    if (tid == 0) svm_finish_info<SvForm>(p, Staged ? sA : p.alpha, Staged ? sGf : p.G);
}

// sv[q][k] = x[sv_index[q]][k] for the n_sv support vectors that k_svm_finish listed (none while the problem is pending): one
// thread per element, consecutive threads along d
__global__ __launch_bounds__(256) void k_svm_gather_sv(const SvmProbDev* __restrict__ P) {
    const SvmProbDev p = P[blockIdx.y];
    if (!p.sv) return;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)p.info->n_sv * p.d) return;
    const size_t q = e / p.d;
    p.sv[e] = p.x[(size_t)p.sv_index[q] * p.d + (e - q * p.d)];
}

// out[q][k] = x[idx[q]][k]: the rows of a cross-validation fold's training part, positives first, into the fold's block
__global__ __launch_bounds__(256) void k_svm_gather_rows(const float* __restrict__ x, const int32_t* __restrict__ idx, float* __restrict__ out,
                                                         size_t elements, int d) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elements) return;
    const size_t q = e / d;
    out[e] = x[(size_t)idx[q] * d + (e - q * d)];
}

// The decision values of the held-out examples of the (at most five) folds of fd_kernel_svm_cv_sigmoid: what svm_predict_values
// (svm.cpp:2506-2562) gives for a two-class model, sum_s (alpha_s y_s) k_function(x, sv_s) - rho in double, s in the model's
// order, k_function (:342-420) summing in feature order: x y, (x - y)^2, min.  The rows are addressed through index lists into
// the examples: sv lists a fold's support vectors in ascending fold index (positives first), held its held-out examples.
struct SvmCvFoldDev {
    const int32_t* sv;
    const double* coef;     // alpha_s y_s, double
    const int32_t* held;
    int32_t n_sv, n_held;   // n_held = 0: a fold that trained nothing
    double rho;
};
struct SvmCvDev {
    const float* x;         // n x d
    double* dec;            // n, in example order
    int32_t d, degree;
    double gamma, coef0;
    SvmCvFoldDev fold[FD_SVM_CV_FOLDS];
};
// One wavefront per 16 held-out rows (blockIdx.x) of a fold (blockIdx.y), k_svm_gram_hik's pattern: 16 support vectors at a
// time, feature chunks of both operand tiles through padded LDS, lane (c, kq) accumulating the pairs (held kq + 4 q, sv c) in
// double with k ascending.  After a tile the 16 x 16 kernel values go through LDS and lane h < 16 adds coef_s K_hs to its row's
// sum, s ascending; the tiles are walked in ascending order, - rho comes last.  Rows past the lists read the lists' first row.
constexpr int SVM_CV_KC = 64;
template <int Kernel>
__global__ __launch_bounds__(64) void k_svm_cv_decision(const SvmCvDev P) {
    __shared__ float sA[16][SVM_CV_KC + 1], sB[16][SVM_CV_KC + 1];
    __shared__ double sK[16][17];
    __shared__ int32_t sHeld[16], sSv[16];
    const SvmCvFoldDev f = P.fold[blockIdx.y];
    const int h0 = blockIdx.x * 16;
    if (h0 >= f.n_held) return;
    const int lane = threadIdx.x, c = lane & 15, kq = lane >> 4, d = P.d;
    if (lane < 16) sHeld[lane] = f.held[h0 + lane < f.n_held ? h0 + lane : 0];
    double sum = 0.0;
    for (int s0 = 0; s0 < f.n_sv; s0 += 16) {
        if (lane < 16) sSv[lane] = f.sv[s0 + lane < f.n_sv ? s0 + lane : 0];
        __syncthreads();
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < d; k0 += SVM_CV_KC) {
            const int kn = min(SVM_CV_KC, d - k0);
            const int kc = k0 + (lane < kn ? lane : 0);   // in-range address for the masked lanes
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sA[r][lane] = P.x[(size_t)sHeld[r] * d + kc];
                sB[r][lane] = P.x[(size_t)sSv[r] * d + kc];
            }
            __syncthreads();
            for (int k = 0; k < kn; ++k) {
                const float b = sB[c][k];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float a = sA[kq + 4 * q][k];
                    if (Kernel == FD_KERNEL_HIK) {
                        acc[q] += (double)(b < a ? b : a);   // min<double>(x_k, sv_k)
                    } else if (Kernel == FD_KERNEL_RBF) {
                        const double diff = (double)a - (double)b;
                        acc[q] += diff * diff;
                    } else {
                        acc[q] += (double)a * (double)b;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double v = acc[q];
            if (Kernel == FD_KERNEL_POLY) v = svm_powi(P.gamma * v + P.coef0, P.degree);
            if (Kernel == FD_KERNEL_RBF) v = exp(-P.gamma * v);
            sK[kq + 4 * q][c] = v;
        }
        __syncthreads();
        if (lane < 16) {
            const int ns = min(16, f.n_sv - s0);
            for (int s = 0; s < ns; ++s) sum += f.coef[s0 + s] * sK[lane][s];
        }
        __syncthreads();   // sK and sSv are rewritten by the next tile
    }
    if (lane < 16 && h0 + lane < f.n_held) P.dec[sHeld[lane]] = sum - f.rho;
}

struct SvmTrainScratch {
    DevBuf x, q, dbl, w, desc, info, state;
    DevBuf xs, svList, sv;   // the support-vector form: xs; sv_index and coef; the gathered rows
    DevBuf cvX, cvRows, cvIdx, cvCoef, cvDec;   // fd_kernel_svm_cv_sigmoid: a host caller's x; the folds' rows; index lists; coef; dec
};

// the run of a support-vector form (fd_kernel_svm_*) with its checked kernel; the solver follows from the number of examples
FdSvmRunSpec svm_sv_spec(const char* who, const fd_svm_kernel* k, int64_t n) {
    if (!k) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    FdSvmRunSpec f = {who, n > SVM_MAX_N};
    f.svForm = true;
    f.kernel = k->kernel;
    if (k->kernel == FD_KERNEL_POLY || k->kernel == FD_KERNEL_RBF) {
        if (!(k->p0 >= 0.0) || std::isinf(k->p0)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: gamma must be finite and not negative (%g)", who, k->p0);
        f.gamma = k->p0;
    }
    if (k->kernel == FD_KERNEL_POLY) {
        if (!std::isfinite(k->p1)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the polynomial kernel's constant must be finite (%g)", who, k->p1);
        if (!(k->p2 >= 0.0) || k->p2 > 2147483647.0 || k->p2 != std::floor(k->p2))
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the polynomial kernel's degree must be a non-negative integer (%g)", who, k->p2);
        f.coef0 = k->p1;
        f.degree = (int32_t)k->p2;
    } else if (k->kernel != FD_KERNEL_LINEAR && k->kernel != FD_KERNEL_RBF && k->kernel != FD_KERNEL_HIK) {
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown kernel %d", who, k->kernel);
    }
    return f;
}

// 0 for a shape the trainer takes, else which of svm_check_shape's messages applies
// oneClass: n_pos examples and no negative one
int svm_shape_fault(int n_pos, int n_neg, int d, int maxN, bool oneClass = false) {
    if (n_pos < 1 || (oneClass ? n_neg != 0 : n_neg < 1)) return oneClass ? 4 : 1;
    if ((int64_t)n_pos + n_neg > maxN) return 2;
    return d < 1 ? 3 : 0;
}

void svm_check_shape(const char* who, int n_pos, int n_neg, int d, int maxN, bool oneClass = false) {
    const int fault = svm_shape_fault(n_pos, n_neg, d, maxN, oneClass);
    if (fault == 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: needs at least one positive and one negative example (%d, %d)", who, n_pos, n_neg);
    if (fault == 4) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: needs at least one example (%d)", who, n_pos);
    if (fault == 2) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %lld examples, at most %d", who, (long long)n_pos + n_neg, maxN);
    if (fault == 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the feature length must be positive (%d)", who, d);
}

// max_iterations = 0: libsvm's own cap
inline int svm_default_max_iter(int n) { return std::max(10000000, 100 * n); }

fd_svm_train_params svm_checked_params(const char* who, const fd_svm_train_params* prm) {
    if (!prm) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    fd_svm_train_params p = *prm;
    if (!(p.C > 0.0) || !(p.weight_pos > 0.0) || !(p.weight_neg > 0.0))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: C and the class weights must be positive (%g, %g, %g)", who, p.C, p.weight_pos, p.weight_neg);
    if (!(p.eps >= 0.0)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: eps must not be negative (%g)", who, p.eps);
    if (p.max_iterations < 0 || p.launch_iterations < 0)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: max_iterations and launch_iterations must not be negative", who);
    if (p.eps == 0.0) p.eps = 1e-4;
    if (p.launch_iterations == 0) p.launch_iterations = SVM_DEFAULT_LAUNCH_ITERATIONS;
    return p;
}

inline size_t svm_align(size_t v) { return (v + 255) / 256 * 256; }

// The aligned byte counts of one problem's buffers, each written here and nowhere else: summed they size the reserves, one after
// the other they place the problem.  SZ_X: the rows of a host caller; SZ_AOUT: alpha in the pinned area; SZ_XS, SZ_LIST (sv_index,
// then coef, n_pad entries each) and SZ_SV (the gathered rows, where asked for): the support-vector form only.  The weights and
// the list have the same size on the device and in the pinned area.
enum { SZ_X, SZ_Q, SZ_DBL, SZ_W, SZ_AOUT, SZ_XS, SZ_LIST, SZ_SV, SZ_COUNT };
struct SvmSizes {
    size_t b[SZ_COUNT] = {};
};
SvmSizes svm_sizes(const fd_svm_train_problem& pr, const FdSvmRunSpec& spec, int c) {
    const size_t n = (size_t)pr.n_pos + pr.n_neg, np = (size_t)svm_pad((int)n);
    SvmSizes z;
    if (!pr.is_device) z.b[SZ_X] = svm_align(sizeof(float) * n * pr.d);
    z.b[SZ_Q] = svm_align(sizeof(float) * np * np);
    z.b[SZ_DBL] = svm_align(sizeof(double) * np * 3);   // QD, alpha, G
    z.b[SZ_W] = svm_align(sizeof(float) * pr.d);
    z.b[SZ_AOUT] = svm_align(sizeof(double) * np);
    if (spec.svForm) {
        z.b[SZ_XS] = svm_align(sizeof(double) * np);
        z.b[SZ_LIST] = svm_align(2 * sizeof(int32_t) * np);
        if (spec.outs && (spec.outs[c].support_vectors || spec.outs[c].sv_store)) z.b[SZ_SV] = svm_align(sizeof(float) * n * pr.d);
    }
    return z;
}

// What one call works on: the problems' descriptors, and the layout of the context's pinned staging area (pageable copies
// cost about a millisecond each on this stack): descriptors, infos, the host callers' X, and the weights / alpha to return.
struct SvmRun {
    std::vector<SvmProbDev> h;
    std::vector<size_t> outW, outA, outS;   // offsets into the pinned area (outS: sv_index, then coef, n entries each)
    char* pinned = nullptr;
    size_t infoOff = 0;
    int maxPad = 0, maxD = 0;
    size_t smoLds = 0;
};

void svm_prepare(fd_ctx* ctx, const FdSvmRunSpec& spec, int count, const fd_svm_train_problem* probs, const fd_svm_train_params& prm, SvmRun& run) {
    SvmTrainScratch& sc = fd_scratch<SvmTrainScratch>(ctx);
    const char* who = spec.who;
    std::vector<SvmSizes> sizes(count);
    SvmSizes total;
    for (int c = 0; c < count; ++c) {
        const fd_svm_train_problem& pr = probs[c];
        svm_check_shape(who, pr.n_pos, pr.n_neg, pr.d, spec.large ? SVM_LARGE_MAX_N : SVM_MAX_N, spec.nu > 0.0);
        if (!pr.x) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
        sizes[c] = svm_sizes(pr, spec, c);
        for (int k = 0; k < SZ_COUNT; ++k) total.b[k] += sizes[c].b[k];
    }
    sc.x.reserve(total.b[SZ_X]);
    try {
        sc.q.reserve(total.b[SZ_Q]);
    } catch (const FdError& e) {   // up to 1 GiB for a large problem: the caller learns what did not fit
        FD_THROW(FD_ERR_RUNTIME, "%s: no device memory for Q (%zu bytes): %s", who, total.b[SZ_Q], e.msg.c_str());
    }
    sc.dbl.reserve(total.b[SZ_DBL]);
    sc.w.reserve(total.b[SZ_W]);
    sc.desc.reserve(sizeof(SvmProbDev) * count);
    sc.info.reserve(sizeof(fd_svm_train_info) * count);
    sc.state.reserve(sizeof(int32_t) * 2 * count);
    if (spec.svForm) {
        sc.xs.reserve(total.b[SZ_XS]);
        sc.svList.reserve(total.b[SZ_LIST]);
        try {
            sc.sv.reserve(total.b[SZ_SV]);
        } catch (const FdError& e) {
            FD_THROW(FD_ERR_RUNTIME, "%s: no device memory for the support vectors (%zu bytes): %s", who, total.b[SZ_SV], e.msg.c_str());
        }
    }
    run.infoOff = svm_align(sizeof(SvmProbDev) * count);
    const size_t xOff = run.infoOff + svm_align(sizeof(fd_svm_train_info) * count);
    size_t outOff = xOff + total.b[SZ_X];
    run.pinned = (char*)fd_pinned(ctx, outOff + total.b[SZ_W] + total.b[SZ_AOUT] + total.b[SZ_LIST]);
    SvmProbDev* hd = (SvmProbDev*)run.pinned;
    run.h.resize(count);
    run.outW.resize(count);
    run.outA.resize(count);
    run.outS.resize(count);
    SvmSizes at;   // where the next problem's share of each buffer begins
    for (int c = 0; c < count; ++c) {
        const fd_svm_train_problem& pr = probs[c];
        const SvmSizes& z = sizes[c];
        const int n = pr.n_pos + pr.n_neg, np = svm_pad(n);
        auto take = [&](const DevBuf& buf, int k) {
            char* at_k = (char*)buf.p + at.b[k];
            at.b[k] += z.b[k];
            return at_k;
        };
        SvmProbDev D = {};
        if (pr.is_device) {
            D.x = pr.x;
        } else {
            std::memcpy(run.pinned + xOff + at.b[SZ_X], pr.x, sizeof(float) * (size_t)n * pr.d);
            D.x = (const float*)take(sc.x, SZ_X);
        }
        D.Q = (float*)take(sc.q, SZ_Q);
        D.QD = (double*)take(sc.dbl, SZ_DBL);
        D.alpha = D.QD + np;
        D.G = D.alpha + np;
        D.w = (float*)take(sc.w, SZ_W);
        if (c == 0 && spec.wOverride) D.w = spec.wOverride;
        run.outW[c] = outOff;
        outOff += z.b[SZ_W];
        run.outA[c] = outOff;
        outOff += z.b[SZ_AOUT];
        D.info = sc.info.as<fd_svm_train_info>() + c;
        D.state = sc.state.as<int32_t>() + 2 * c;
        D.Cp = prm.C * prm.weight_pos;
        D.Cn = prm.C * prm.weight_neg;
        D.eps = prm.eps;
        D.n_pos = pr.n_pos;
        D.n = n;
        D.n_pad = np;
        D.d = pr.d;
        D.q_in_lds = !spec.large && svm_q_in_lds(n) ? 1 : 0;
        D.max_iter = prm.max_iterations > 0 ? prm.max_iterations : svm_default_max_iter(n);
        D.lin = -1.0;
        if (spec.nu > 0.0) {   // solve_one_class: p = 0, (int)(nu l) alphas at the bound 1 and the remainder behind them
            D.lin = 0.0;
            D.oc_full = (int)(spec.nu * n);
            D.oc_frac = spec.nu * n - D.oc_full;
        }
        if (spec.svForm) {
            D.xs = (double*)take(sc.xs, SZ_XS);
            D.sv_index = (int32_t*)take(sc.svList, SZ_LIST);
            D.coef = (float*)(D.sv_index + np);
            if (z.b[SZ_SV]) D.sv = (float*)take(sc.sv, SZ_SV);
            run.outS[c] = outOff;
            outOff += z.b[SZ_LIST];
            D.gamma = spec.gamma;
            D.coef0 = spec.coef0;
            D.degree = spec.degree;
        }
        run.h[c] = D;
        hd[c] = D;
        run.maxPad = std::max(run.maxPad, np);
        run.maxD = std::max(run.maxD, pr.d);
        run.smoLds = std::max(run.smoLds, spec.large ? svm_large_lds(n) : svm_smo_lds(n, D.q_in_lds != 0));
    }
    if (total.b[SZ_X]) HIP_CHECK(hipMemcpyAsync(sc.x.p, run.pinned + xOff, total.b[SZ_X], hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(sc.desc.p, hd, sizeof(SvmProbDev) * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(sc.state.p, 0, sizeof(int32_t) * 2 * count, ctx->stream));
    const dim3 tiles(run.maxPad / 16, run.maxPad / 16, count);
    void (*gram)(const SvmProbDev*) = k_svm_gram<FD_KERNEL_LINEAR>;
    if (spec.kernel == FD_KERNEL_HIK) gram = k_svm_gram_hik;
    if (spec.kernel == FD_KERNEL_POLY) gram = k_svm_gram<FD_KERNEL_POLY>;
    if (spec.kernel == FD_KERNEL_RBF) {   // xs first, from the diagonal tiles
        gram = k_svm_gram<FD_KERNEL_RBF>;
        hipLaunchKernelGGL(k_svm_gram<SVM_GRAM_XS>, dim3(run.maxPad / 16, 1, count), dim3(64), 0, ctx->stream, sc.desc.as<SvmProbDev>());
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(gram, tiles, dim3(64), 0, ctx->stream, sc.desc.as<SvmProbDev>());
    HIP_CHECK(hipGetLastError());
    if (spec.nu > 0.0) {   // in place of alpha = 0, G = -1
        hipLaunchKernelGGL(k_svm_one_class_start, dim3((run.maxPad + 255) / 256, count), dim3(256), 0, ctx->stream, sc.desc.as<SvmProbDev>());
        HIP_CHECK(hipGetLastError());
    }
}

fd_svm_train_problem svm_single_problem(const float* x, int n_pos, int n_neg, int d, int is_device, float* weights, float* bias, double* alpha) {
    fd_svm_train_problem pr = {};
    pr.x = x;
    pr.n_pos = n_pos;
    pr.n_neg = n_neg;
    pr.d = d;
    pr.is_device = is_device;
    pr.weights = weights;
    pr.bias = bias;
    pr.alpha = alpha;
    return pr;
}

void svm_gram(fd_ctx* ctx, const FdSvmRunSpec& spec, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD,
              double* G0 = nullptr) {
    HIP_CHECK(hipSetDevice(ctx->device));
    const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, nullptr, nullptr, nullptr);
    fd_svm_train_params prm = {1.0, 1.0, 1.0, 1e-4, 0, SVM_DEFAULT_LAUNCH_ITERATIONS};
    SvmRun run;
    svm_prepare(ctx, spec, 1, &pr, prm, run);
    const SvmProbDev& D = run.h[0];
    HIP_CHECK(hipMemcpy2DAsync(Q, sizeof(float) * D.n, D.Q, sizeof(float) * D.n_pad, sizeof(float) * D.n, D.n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(QD, D.QD, sizeof(double) * D.n, hipMemcpyDeviceToHost, ctx->stream));
    if (G0) HIP_CHECK(hipMemcpyAsync(G0, D.G, sizeof(double) * D.n, hipMemcpyDeviceToHost, ctx->stream));   // the start gradient
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// the two linear Gram entry points and the two single-problem linear trainers: `spec` names the one that was called
int svm_linear_gram(fd_ctx* ctx, const FdSvmRunSpec& spec, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !Q || !QD) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", spec.who);
        svm_gram(ctx, spec, x, n_pos, n_neg, d, is_device, Q, QD);
    });
}
int svm_linear_train(fd_ctx* ctx, const FdSvmRunSpec& spec, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_train_params* params,
                     float* weights, float* bias, double* alpha, fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !weights || !bias || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", spec.who);
        const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, weights, bias, alpha);
        fd_svm_train_run(ctx, spec, 1, &pr, params, info);
    });
}

// trains one problem of a support-vector form and creates the f32 model with fd_svm_create; one-class when spec.nu > 0
void svm_train_model(fd_ctx* ctx, FdSvmRunSpec spec, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel& kernel,
                     const fd_svm_train_params* params, float threshold, double logistic_a, double logistic_b, fd_svm** out, fd_svm_train_info* info) {
    svm_check_shape(spec.who, n_pos, n_neg, d, SVM_LARGE_MAX_N, spec.nu > 0.0);   // before the lists are sized by n
    const int n = n_pos + n_neg;
    std::vector<int32_t> svIndex(n);
    std::vector<float> coef(n), rows;
    float bias = 0.f;
    const FdSvmSvOut o = {svIndex.data(), coef.data(), nullptr, &rows};
    spec.outs = &o;
    const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, nullptr, &bias, nullptr);
    fd_svm_train_run(ctx, spec, 1, &pr, params, info);
    if (info->n_sv < 1) FD_THROW(FD_ERR_RUNTIME, "%s: the trained model has no support vector", spec.who);
    if (spec.nu > 0.0 && !std::isfinite(info->rho))   // nu = 1: every alpha at its bound, rho = +inf
        FD_THROW(FD_ERR_RUNTIME, "%s: the trained model's rho is not finite (%g)", spec.who, info->rho);
    fd_svm_model md = {};
    md.kernel = kernel.kernel;
    md.p0 = kernel.p0;
    md.p1 = kernel.p1;
    md.p2 = kernel.p2;
    md.num_sv = info->n_sv;
    md.dim = d;
    md.dtype = FD_DTYPE_F32;
    md.support_vectors = rows.data();
    md.coefficients = coef.data();
    md.bias = bias;
    md.threshold = threshold;
    md.logistic_a = logistic_a;
    md.logistic_b = logistic_b;
    const int created = fd_svm_create(ctx, &md, out);
    if (created != FD_OK) throw FdError{created, ctx->error};
}

// svm_check_parameter's rule for ONE_CLASS (svm.cpp:3056-3060)
double svm_checked_nu(const char* who, double nu) {
    if (!(nu > 0.0) || nu > 1.0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: nu <= 0 or nu > 1 (%g)", who, nu);
    return nu;
}
// a one-class run: nu into the spec, and the solver's parameters with both bounds 1
fd_svm_train_params svm_one_class_params(FdSvmRunSpec& spec, const fd_svm_one_class_params& p) {
    spec.nu = svm_checked_nu(spec.who, p.nu);
    return fd_svm_train_params{1.0, 1.0, 1.0, p.eps, p.max_iterations, p.launch_iterations};
}

// sigmoid_train (svm.cpp:1752-1863), operation for operation; labels_i > 0 for i < n_pos
void svm_sigmoid_train(int l, const double* dec, int n_pos, double& A, double& B, int* iterations, int* status) {
    const double prior1 = n_pos, prior0 = l - n_pos;
    const int max_iter = 100;
    const double min_step = 1e-10, sigma = 1e-12, eps = 1e-5;
    const double hiTarget = (prior1 + 1.0) / (prior1 + 2.0), loTarget = 1 / (prior0 + 2.0);
    std::vector<double> t(l);
    A = 0.0;
    B = std::log((prior0 + 1.0) / (prior1 + 1.0));
    double fval = 0.0;
    for (int i = 0; i < l; ++i) {
        t[i] = i < n_pos ? hiTarget : loTarget;
        const double fApB = dec[i] * A + B;
        if (fApB >= 0) fval += t[i] * fApB + std::log(1 + std::exp(-fApB));
        else fval += (t[i] - 1) * fApB + std::log(1 + std::exp(fApB));
    }
    int iter, st = FD_SVM_SIGMOID_CONVERGED;
    for (iter = 0; iter < max_iter; ++iter) {
        double h11 = sigma, h22 = sigma, h21 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int i = 0; i < l; ++i) {
            const double fApB = dec[i] * A + B;
            double p, q;
            if (fApB >= 0) {
                p = std::exp(-fApB) / (1.0 + std::exp(-fApB));
                q = 1.0 / (1.0 + std::exp(-fApB));
            } else {
                p = 1.0 / (1.0 + std::exp(fApB));
                q = std::exp(fApB) / (1.0 + std::exp(fApB));
            }
            const double d2 = p * q;
            h11 += dec[i] * dec[i] * d2;
            h22 += d2;
            h21 += dec[i] * d2;
            const double d1 = t[i] - p;
            g1 += dec[i] * d1;
            g2 += d1;
        }
        if (std::fabs(g1) < eps && std::fabs(g2) < eps) break;
        const double det = h11 * h22 - h21 * h21;
        const double dA = -(h22 * g1 - h21 * g2) / det;
        const double dB = -(-h21 * g1 + h11 * g2) / det;
        const double gd = g1 * dA + g2 * dB;
        double stepsize = 1;
        while (stepsize >= min_step) {
            const double newA = A + stepsize * dA, newB = B + stepsize * dB;
            double newf = 0.0;
            for (int i = 0; i < l; ++i) {
                const double fApB = dec[i] * newA + newB;
                if (fApB >= 0) newf += t[i] * fApB + std::log(1 + std::exp(-fApB));
                else newf += (t[i] - 1) * fApB + std::log(1 + std::exp(fApB));
            }
            if (newf < fval + 0.0001 * stepsize * gd) {
                A = newA;
                B = newB;
                fval = newf;
                break;
            } else {
                stepsize = stepsize / 2.0;
            }
        }
        if (stepsize < min_step) {
            st = FD_SVM_SIGMOID_LINE_SEARCH_FAILED;
            break;
        }
    }
    if (iter >= max_iter) st = FD_SVM_SIGMOID_MAX_ITERATIONS;
    if (iterations) *iterations = iter;
    if (status) *status = st;
}

// fd_kernel_svm_cv_sigmoid: the folds' index lists on the host, their rows gathered on the device, the trainer over the
// folds (those of up to 1024 rows in one run, the larger ones in another), k_svm_cv_decision over the held-out rows, the fit.
void svm_cv_sigmoid(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                    const fd_svm_train_params* params, const int32_t* perm, double* prob_a, double* prob_b, double* dec_values,
                    fd_svm_cv_info* cv_info) {
    const char* who = "fd_kernel_svm_cv_sigmoid";
    const FdSvmRunSpec kspec = svm_sv_spec(who, kernel, 0);
    svm_check_shape(who, n_pos, n_neg, d, SVM_LARGE_MAX_N);
    const fd_svm_train_params prm = svm_checked_params(who, params);
    const int n = n_pos + n_neg;
    {
        std::vector<char> seen(n, 0);
        for (int i = 0; i < n; ++i) {
            if (perm[i] < 0 || perm[i] >= n || seen[perm[i]]) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: perm is not a permutation of 0..%d (entry %d)", who, n - 1, i);
            seen[perm[i]] = 1;
        }
    }
    // the folds train with C = 1 and the weighted bounds as class weights (svm.cpp:1998-2007)
    const fd_svm_train_params foldPrm = {1.0, prm.C * prm.weight_pos, prm.C * prm.weight_neg, prm.eps, prm.max_iterations, prm.launch_iterations};
    constexpr int F = FD_SVM_CV_FOLDS;
    fd_svm_cv_info ci = {};
    std::vector<int32_t> train[F], held[F];
    int nPosOf[F];
    size_t rowsOff[F], rowsTotal = 0, idxTotal = 0;
    for (int f = 0; f < F; ++f) {
        const int begin = (int)((int64_t)f * n / F), end = (int)((int64_t)(f + 1) * n / F);
        std::vector<int32_t> neg;
        for (int j = 0; j < n; ++j) {   // svm_group_classes: the positives in permuted order, then the negatives
            if (j >= begin && j < end) continue;
            (perm[j] < n_pos ? train[f] : neg).push_back(perm[j]);
        }
        nPosOf[f] = (int)train[f].size();
        const int nNegOf = (int)neg.size();
        train[f].insert(train[f].end(), neg.begin(), neg.end());
        held[f].assign(perm + begin, perm + end);
        ci.fold_trained[f] = nPosOf[f] > 0 && nNegOf > 0 ? 1 : 0;
        ci.fold_constant[f] = ci.fold_trained[f] ? 0.0 : (nPosOf[f] > 0 ? 1.0 : (nNegOf > 0 ? -1.0 : 0.0));
        if (!ci.fold_trained[f]) {
            train[f].clear();
            held[f].clear();   // no decision values from the device
        }
        rowsOff[f] = rowsTotal;
        rowsTotal += svm_align(sizeof(float) * train[f].size() * d);
        idxTotal += 2 * (size_t)n;   // a fold's lists: train, later its support vectors in their place; held
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    SvmTrainScratch& sc = fd_scratch<SvmTrainScratch>(ctx);
    const float* dx = x;
    if (!is_device) {
        sc.cvX.reserve(sizeof(float) * (size_t)n * d);
        HIP_CHECK(hipMemcpyAsync(sc.cvX.p, x, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice, ctx->stream));
        dx = sc.cvX.as<float>();
    }
    try {
        sc.cvRows.reserve(rowsTotal);
    } catch (const FdError& e) {
        FD_THROW(FD_ERR_RUNTIME, "%s: no device memory for the folds' rows (%zu bytes): %s", who, rowsTotal, e.msg.c_str());
    }
    sc.cvIdx.reserve(sizeof(int32_t) * idxTotal);
    sc.cvCoef.reserve(sizeof(double) * (size_t)n * F);
    sc.cvDec.reserve(sizeof(double) * n);
    std::vector<int32_t> hIdx(idxTotal, 0);
    for (int f = 0; f < F; ++f) {
        std::copy(train[f].begin(), train[f].end(), hIdx.begin() + 2 * (size_t)n * f);
        std::copy(held[f].begin(), held[f].end(), hIdx.begin() + 2 * (size_t)n * f + n);
    }
    HIP_CHECK(hipMemcpyAsync(sc.cvIdx.p, hIdx.data(), sizeof(int32_t) * idxTotal, hipMemcpyHostToDevice, ctx->stream));
    std::vector<double> alpha[F];
    std::vector<int32_t> svIndex[F];
    std::vector<float> coefF[F];
    float bias[F];
    fd_svm_train_problem prob[F];
    FdSvmSvOut outs[F];
    for (int f = 0; f < F; ++f) {
        if (!ci.fold_trained[f]) continue;
        const size_t rows = train[f].size(), elements = rows * d;
        float* block = (float*)((char*)sc.cvRows.p + rowsOff[f]);
        hipLaunchKernelGGL(k_svm_gather_rows, dim3((unsigned)((elements + 255) / 256)), dim3(256), 0, ctx->stream, dx,
                           sc.cvIdx.as<int32_t>() + 2 * (size_t)n * f, block, elements, d);
        HIP_CHECK(hipGetLastError());
        alpha[f].resize(rows);
        svIndex[f].resize(rows);
        coefF[f].resize(rows);
        prob[f] = svm_single_problem(block, nPosOf[f], (int)rows - nPosOf[f], d, 1, nullptr, &bias[f], alpha[f].data());
        outs[f] = FdSvmSvOut{svIndex[f].data(), coefF[f].data(), nullptr, nullptr};
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));   // hIdx and a pageable x are read
    for (int large = 0; large < 2; ++large) {   // the folds of either solver in one run
        std::vector<int> which;
        std::vector<fd_svm_train_problem> probs;
        std::vector<FdSvmSvOut> os;
        for (int f = 0; f < F; ++f)
            if (ci.fold_trained[f] && ((int)train[f].size() > SVM_MAX_N) == (large != 0)) {
                which.push_back(f);
                probs.push_back(prob[f]);
                os.push_back(outs[f]);
            }
        if (which.empty()) continue;
        FdSvmRunSpec spec = kspec;
        spec.large = large != 0;
        spec.outs = os.data();
        std::vector<fd_svm_train_info> infos(which.size());
        fd_svm_train_run(ctx, spec, (int)which.size(), probs.data(), &foldPrm, infos.data());
        for (size_t c = 0; c < which.size(); ++c) ci.fold[which[c]] = infos[c];
    }
    // the models' support vectors as example indices, and alpha_s y_s in double
    SvmCvDev cv = {};
    cv.x = dx;
    cv.dec = sc.cvDec.as<double>();
    cv.d = d;
    cv.degree = kspec.degree;
    cv.gamma = kspec.gamma;
    cv.coef0 = kspec.coef0;
    std::vector<double> hCoef((size_t)n * F, 0.0);
    int maxHeld = 0;
    for (int f = 0; f < F; ++f) {
        if (!ci.fold_trained[f]) continue;
        const int nsv = ci.fold[f].n_sv;
        int32_t* sv = hIdx.data() + 2 * (size_t)n * f;
        for (int s = 0; s < nsv; ++s) {
            const int q = svIndex[f][s];
            hCoef[(size_t)n * f + s] = q < nPosOf[f] ? alpha[f][q] : -alpha[f][q];
            sv[s] = train[f][q];
        }
        SvmCvFoldDev& fd = cv.fold[f];
        fd.sv = sc.cvIdx.as<int32_t>() + 2 * (size_t)n * f;
        fd.held = fd.sv + n;
        fd.coef = sc.cvCoef.as<double>() + (size_t)n * f;
        fd.n_sv = nsv;
        fd.n_held = (int)held[f].size();
        fd.rho = ci.fold[f].rho;
        maxHeld = std::max(maxHeld, fd.n_held);
    }
    std::vector<double> dec(n, 0.0);
    if (maxHeld > 0) {
        HIP_CHECK(hipMemcpyAsync(sc.cvIdx.p, hIdx.data(), sizeof(int32_t) * idxTotal, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(sc.cvCoef.p, hCoef.data(), sizeof(double) * hCoef.size(), hipMemcpyHostToDevice, ctx->stream));
        void (*decision)(const SvmCvDev) = k_svm_cv_decision<FD_KERNEL_LINEAR>;
        if (kspec.kernel == FD_KERNEL_POLY) decision = k_svm_cv_decision<FD_KERNEL_POLY>;
        if (kspec.kernel == FD_KERNEL_RBF) decision = k_svm_cv_decision<FD_KERNEL_RBF>;
        if (kspec.kernel == FD_KERNEL_HIK) decision = k_svm_cv_decision<FD_KERNEL_HIK>;
        hipLaunchKernelGGL(decision, dim3((maxHeld + 15) / 16, F), dim3(64), 0, ctx->stream, cv);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(dec.data(), sc.cvDec.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    for (int f = 0; f < F; ++f) {
        if (ci.fold_trained[f]) continue;
        const int begin = (int)((int64_t)f * n / F), end = (int)((int64_t)(f + 1) * n / F);
        for (int j = begin; j < end; ++j) dec[perm[j]] = ci.fold_constant[f];
    }
    svm_sigmoid_train(n, dec.data(), n_pos, *prob_a, *prob_b, &ci.newton_iterations, &ci.status);
    if (dec_values) std::memcpy(dec_values, dec.data(), sizeof(double) * n);
    if (cv_info) *cv_info = ci;
}
}  // namespace

// Trains `count` problems in one set of launches; infos[c] is filled for every problem.  Leaves ctx->stream synchronised.
// spec.large: problems of up to SVM_LARGE_MAX_N examples on k_svm_smo_large, one workgroup each (the public entry points pass one;
// the sigmoid fit's folds up to five).  spec.svForm: the problems' weights are NULL; spec.outs receives the model.  spec.nu > 0:
// one-class problems.
void fd_svm_train_run(fd_ctx* ctx, const FdSvmRunSpec& spec, int count, const fd_svm_train_problem* probs, const fd_svm_train_params* params,
                      fd_svm_train_info* infos) {
    const char* who = spec.who;
    const bool large = spec.large, svForm = spec.svForm;
    float* const wOverride = spec.wOverride;
    const fd_svm_train_params prm = svm_checked_params(who, params);
    if (count < 1 || !probs || !infos) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument or no problem", who);
    HIP_CHECK(hipSetDevice(ctx->device));
    SvmRun run;
    svm_prepare(ctx, spec, count, probs, prm, run);
    SvmTrainScratch& sc = fd_scratch<SvmTrainScratch>(ctx);
    size_t rowElements = 0;   // the gather's grid: the largest n x d among the problems that want their support vectors' rows
    for (int c = 0; c < count; ++c)
        if (run.h[c].sv) rowElements = std::max(rowElements, (size_t)run.h[c].n * run.h[c].d);
    static uint64_t ldsAllowed = 0, ldsAllowedLarge = 0;
    if (large) fd_allow_lds(ctx, (const void*)k_svm_smo_large, (int)SVM_LDS_BUDGET, ldsAllowedLarge);
    else fd_allow_lds(ctx, (const void*)k_svm_smo, (int)SVM_LDS_BUDGET, ldsAllowed);
    const auto finish = large ? (svForm ? k_svm_finish<false, true> : k_svm_finish<false, false>)
                              : (svForm ? k_svm_finish<true, true> : k_svm_finish<true, false>);
    const fd_svm_train_info* hinfo = (const fd_svm_train_info*)(run.pinned + run.infoOff);
    int launches = 0;
    for (;;) {
        if (large)
            hipLaunchKernelGGL(k_svm_smo_large, dim3(count), dim3(SVM_LARGE_THREADS), run.smoLds, ctx->stream, sc.desc.as<SvmProbDev>(), prm.launch_iterations);
        else
            hipLaunchKernelGGL(k_svm_smo, dim3(count), dim3(SVM_SMO_THREADS), run.smoLds, ctx->stream, sc.desc.as<SvmProbDev>(), prm.launch_iterations);
        HIP_CHECK(hipGetLastError());
        ++launches;
        hipLaunchKernelGGL(finish, dim3(svForm ? 1 : (run.maxD + 255) / 256, count), dim3(256), 0, ctx->stream, sc.desc.as<SvmProbDev>());
        if (rowElements) {
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_svm_gather_sv, dim3((unsigned)((rowElements + 255) / 256), count), dim3(256), 0, ctx->stream, sc.desc.as<SvmProbDev>());
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(run.pinned + run.infoOff, sc.info.p, sizeof(fd_svm_train_info) * count, hipMemcpyDeviceToHost, ctx->stream));
        // the results ride along: in the usual case the first launch converges and this is the only wait
        for (int c = 0; c < count; ++c) {
            const SvmProbDev& D = run.h[c];
            if (probs[c].weights && !(c == 0 && wOverride))
                HIP_CHECK(hipMemcpyAsync(run.pinned + run.outW[c], D.w, sizeof(float) * D.d, hipMemcpyDeviceToHost, ctx->stream));
            if (probs[c].alpha) HIP_CHECK(hipMemcpyAsync(run.pinned + run.outA[c], D.alpha, sizeof(double) * D.n, hipMemcpyDeviceToHost, ctx->stream));
            if (svForm) HIP_CHECK(hipMemcpyAsync(run.pinned + run.outS[c], D.sv_index, 2 * sizeof(int32_t) * D.n_pad, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        bool done = true;
        for (int c = 0; c < count; ++c) done = done && (hinfo[c].converged || hinfo[c].iterations >= run.h[c].max_iter);
        if (done) break;
    }
    for (int c = 0; c < count; ++c) {
        infos[c] = hinfo[c];
        infos[c].launches = launches;
        const fd_svm_train_problem& pr = probs[c];
        if (pr.weights && !(c == 0 && wOverride)) std::memcpy(pr.weights, run.pinned + run.outW[c], sizeof(float) * pr.d);
        if (pr.alpha) std::memcpy(pr.alpha, run.pinned + run.outA[c], sizeof(double) * run.h[c].n);
        if (pr.bias) *pr.bias = (float)infos[c].rho;
    }
    if (!svForm) return;
    bool rows = false;
    for (int c = 0; c < count; ++c) {   // the lists from the staging area; the rows, whose number is known only now, straight from the device
        const SvmProbDev& D = run.h[c];
        const FdSvmSvOut& o = spec.outs[c];
        const size_t nsv = (size_t)infos[c].n_sv;
        std::memcpy(o.sv_index, run.pinned + run.outS[c], sizeof(int32_t) * nsv);
        std::memcpy(o.coefficients, run.pinned + run.outS[c] + sizeof(int32_t) * D.n_pad, sizeof(float) * nsv);
        if (o.sv_store) o.sv_store->resize(nsv * D.d);
        float* dst = o.sv_store ? o.sv_store->data() : o.support_vectors;
        if (D.sv && nsv) {
            HIP_CHECK(hipMemcpyAsync(dst, D.sv, sizeof(float) * nsv * D.d, hipMemcpyDeviceToHost, ctx->stream));
            rows = true;
        }
    }
    if (rows) HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

extern "C" {

int fd_linear_svm_train_limits(int n_pos, int n_neg, int d, int* q_in_lds, int* max_iterations) {
    if (svm_shape_fault(n_pos, n_neg, d, SVM_MAX_N)) return FD_ERR_INVALID_ARGUMENT;
    const int n = n_pos + n_neg;
    if (q_in_lds) *q_in_lds = svm_q_in_lds(n) ? 1 : 0;
    if (max_iterations) *max_iterations = svm_default_max_iter(n);
    return FD_OK;
}

int fd_linear_svm_train_large_limits(int n_pos, int n_neg, int d, int* lds_bytes, int* max_iterations) {
    if (svm_shape_fault(n_pos, n_neg, d, SVM_LARGE_MAX_N)) return FD_ERR_INVALID_ARGUMENT;
    const int n = n_pos + n_neg;
    if (lds_bytes) *lds_bytes = (int)svm_large_lds(n);
    if (max_iterations) *max_iterations = svm_default_max_iter(n);
    return FD_OK;
}

int fd_linear_svm_gram(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD) {
    return svm_linear_gram(ctx, {"fd_linear_svm_gram", false}, x, n_pos, n_neg, d, is_device, Q, QD);
}

int fd_linear_svm_gram_large(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD) {
    return svm_linear_gram(ctx, {"fd_linear_svm_gram_large", true}, x, n_pos, n_neg, d, is_device, Q, QD);
}

int fd_linear_svm_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_train_params* params, float* weights,
                        float* bias, double* alpha, fd_svm_train_info* info) {
    return svm_linear_train(ctx, {"fd_linear_svm_train", false}, x, n_pos, n_neg, d, is_device, params, weights, bias, alpha, info);
}

int fd_linear_svm_train_large(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_train_params* params,
                              float* weights, float* bias, double* alpha, fd_svm_train_info* info) {
    return svm_linear_train(ctx, {"fd_linear_svm_train_large", true}, x, n_pos, n_neg, d, is_device, params, weights, bias, alpha, info);
}

int fd_linear_svm_train_batch(fd_ctx* ctx, int count, const fd_svm_train_problem* problems, const fd_svm_train_params* params, fd_svm_train_info* infos) {
    return fd_guard(ctx, [&] {
        if (!ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train_batch: NULL argument");
        if (count > 65535) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train_batch: %d problems, at most 65535", count);
        for (int c = 0; c < count && problems; ++c)
            if (!problems[c].weights || !problems[c].bias) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train_batch: NULL argument in problem %d", c);
        fd_svm_train_run(ctx, {"fd_linear_svm_train_batch"}, count, problems, params, infos);
    });
}

/* ---- the support-vector form: any kernel of fd_svm_model ---- */
int fd_kernel_svm_train_limits(int n_pos, int n_neg, int d, int* q_in_lds, int* large, int* max_iterations) {
    if (svm_shape_fault(n_pos, n_neg, d, SVM_LARGE_MAX_N)) return FD_ERR_INVALID_ARGUMENT;
    const int n = n_pos + n_neg;
    if (q_in_lds) *q_in_lds = n <= SVM_MAX_N && svm_q_in_lds(n) ? 1 : 0;
    if (large) *large = n > SVM_MAX_N ? 1 : 0;
    if (max_iterations) *max_iterations = svm_default_max_iter(n);
    return FD_OK;
}

int fd_kernel_svm_gram(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel, float* Q, double* QD) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !Q || !QD) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_gram: NULL argument");
        svm_gram(ctx, svm_sv_spec("fd_kernel_svm_gram", kernel, (int64_t)n_pos + n_neg), x, n_pos, n_neg, d, is_device, Q, QD);
    });
}

int fd_kernel_svm_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                        const fd_svm_train_params* params, int32_t* sv_index, float* coefficients, float* support_vectors, float* bias, double* alpha,
                        fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !sv_index || !coefficients || !bias || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train: NULL argument");
        FdSvmRunSpec spec = svm_sv_spec("fd_kernel_svm_train", kernel, (int64_t)n_pos + n_neg);
        const FdSvmSvOut out = {sv_index, coefficients, support_vectors, nullptr};
        spec.outs = &out;
        const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, nullptr, bias, alpha);
        fd_svm_train_run(ctx, spec, 1, &pr, params, info);
    });
}

int fd_kernel_svm_train_model(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                              const fd_svm_train_params* params, float threshold, double logistic_a, double logistic_b, fd_svm** out,
                              fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !out || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_model: NULL argument");
        *out = nullptr;
        const FdSvmRunSpec spec = svm_sv_spec("fd_kernel_svm_train_model", kernel, (int64_t)n_pos + n_neg);
        svm_train_model(ctx, spec, x, n_pos, n_neg, d, is_device, *kernel, params, threshold, logistic_a, logistic_b, out, info);
    });
}

int fd_kernel_svm_train_batch(fd_ctx* ctx, int count, const fd_kernel_svm_train_problem* problems, const fd_svm_kernel* kernel,
                              const fd_svm_train_params* params, fd_svm_train_info* infos) {
    return fd_guard(ctx, [&] {
        if (!ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_batch: NULL argument");
        if (count > 65535) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_batch: %d problems, at most 65535", count);
        FdSvmRunSpec spec = svm_sv_spec("fd_kernel_svm_train_batch", kernel, 0);   // the batch runs on the small solver
        std::vector<fd_svm_train_problem> probs;
        std::vector<FdSvmSvOut> outs;
        for (int c = 0; c < count && problems; ++c) {
            const fd_kernel_svm_train_problem& pr = problems[c];
            if (!pr.sv_index || !pr.coefficients || !pr.bias) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_batch: NULL argument in problem %d", c);
            probs.push_back(svm_single_problem(pr.x, pr.n_pos, pr.n_neg, pr.d, pr.is_device, nullptr, pr.bias, pr.alpha));
            outs.push_back(FdSvmSvOut{pr.sv_index, pr.coefficients, pr.support_vectors, nullptr});
        }
        spec.outs = outs.data();
        fd_svm_train_run(ctx, spec, count, problems ? probs.data() : nullptr, params, infos);
    });
}

/* ---- one-class models ---- */
int fd_one_class_svm_train_limits(int n, int d, int* q_in_lds, int* large, int* max_iterations) {
    if (svm_shape_fault(n, 0, d, SVM_LARGE_MAX_N, true)) return FD_ERR_INVALID_ARGUMENT;
    if (q_in_lds) *q_in_lds = n <= SVM_MAX_N && svm_q_in_lds(n) ? 1 : 0;
    if (large) *large = n > SVM_MAX_N ? 1 : 0;
    if (max_iterations) *max_iterations = svm_default_max_iter(n);
    return FD_OK;
}

int fd_one_class_svm_gram(fd_ctx* ctx, const float* x, int n, int d, int is_device, const fd_svm_kernel* kernel, double nu, float* Q, double* QD,
                          double* G0) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !Q || !QD) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_one_class_svm_gram: NULL argument");
        FdSvmRunSpec spec = svm_sv_spec("fd_one_class_svm_gram", kernel, n);
        spec.nu = svm_checked_nu(spec.who, nu);
        svm_gram(ctx, spec, x, n, 0, d, is_device, Q, QD, G0);
    });
}

int fd_one_class_svm_train(fd_ctx* ctx, const float* x, int n, int d, int is_device, const fd_svm_kernel* kernel,
                           const fd_svm_one_class_params* params, int32_t* sv_index, float* coefficients, float* support_vectors, float* bias,
                           double* alpha, fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !params || !sv_index || !coefficients || !bias || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_one_class_svm_train: NULL argument");
        FdSvmRunSpec spec = svm_sv_spec("fd_one_class_svm_train", kernel, n);
        const fd_svm_train_params prm = svm_one_class_params(spec, *params);
        const FdSvmSvOut out = {sv_index, coefficients, support_vectors, nullptr};
        spec.outs = &out;
        const fd_svm_train_problem pr = svm_single_problem(x, n, 0, d, is_device, nullptr, bias, alpha);
        fd_svm_train_run(ctx, spec, 1, &pr, &prm, info);
    });
}

int fd_one_class_svm_train_model(fd_ctx* ctx, const float* x, int n, int d, int is_device, const fd_svm_kernel* kernel,
                                 const fd_svm_one_class_params* params, float threshold, double logistic_a, double logistic_b, fd_svm** out,
                                 fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !params || !out || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_one_class_svm_train_model: NULL argument");
        *out = nullptr;
        FdSvmRunSpec spec = svm_sv_spec("fd_one_class_svm_train_model", kernel, n);
        const fd_svm_train_params prm = svm_one_class_params(spec, *params);
        svm_train_model(ctx, spec, x, n, 0, d, is_device, *kernel, &prm, threshold, logistic_a, logistic_b, out, info);
    });
}

/* ---- libsvm's sigmoid fit ---- */
int fd_svm_sigmoid_train(int n, const double* dec_values, int n_pos, double* prob_a, double* prob_b, int* iterations, int* status) {
    if (n < 1 || n_pos < 0 || n_pos > n || !dec_values || !prob_a || !prob_b) return FD_ERR_INVALID_ARGUMENT;
    svm_sigmoid_train(n, dec_values, n_pos, *prob_a, *prob_b, iterations, status);
    return FD_OK;
}

int fd_kernel_svm_cv_sigmoid(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                             const fd_svm_train_params* params, const int32_t* perm, double* prob_a, double* prob_b, double* dec_values,
                             fd_svm_cv_info* cv_info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !perm || !prob_a || !prob_b) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_cv_sigmoid: NULL argument");
        svm_cv_sigmoid(ctx, x, n_pos, n_neg, d, is_device, kernel, params, perm, prob_a, prob_b, dec_values, cv_info);
    });
}

}  // extern "C"
