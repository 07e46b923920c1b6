// featuredetection_amd/csrc/svm_train.hip -- linear C-SVC training on the device, libsvm's model bit for bit on a given Q
// (DESIGN.md section 4.6).  What ExtendedHogBasedMeasurementModel's adaptation needs of libsvm::LibSvmClassifier::train
// (LibSvmClassifier.cpp:156-189, libSvm/src/svm.cpp Solver::Solve :551-830 without shrinking, select_working_set :833-930,
// calculate_rho :1013-1049, LibSvmUtils::extractSupportVectors LibSvmUtils.cpp:105-118).
//
//   k_svm_gram    K = X X^T on the f64 MFMA pipe (f32 products are exact in f64), Q_ij = (float)(y_i y_j K_ij), QD_i = K_ii;
//                 also the start state alpha = 0, G = -1
//   k_svm_smo     one workgroup per problem: a counted loop of SMO iterations over a per-launch budget; alpha, G, the iteration
//                 count and the converged flag persist in global memory between launches (the host relaunches)
//   k_svm_finish  rho, the objective and the support-vector counts (one thread, libsvm's summation order), and the single
//                 weight vector, one thread per dimension
//   k_svm_smo_large, k_svm_finish_large   the same for up to 16384 examples: 1024 threads, G and a status
//                 byte per element in LDS, alpha in memory; the arithmetic is shared with the two kernels above
//
//
// The same solver on the Q of a polynomial, RBF or histogram-intersection kernel, with the model returned as support vectors and
// coefficients (fd_kernel_svm_*; Kernel::kernel_poly / kernel_rbf / kernel_hik svm.cpp:235-273, svm_train's
// two-class model, LibSvmUtils::extractCoefficients):
//   k_svm_gram_kernel   k_svm_gram's dot tile with an epilogue in double: powi(gamma dot + coef0, degree) or
//                       exp(-gamma ((xs_i + xs_j) - 2 dot)); xs comes from a first launch over the diagonal tiles, so that the
//                       diagonal of the second launch subtracts the very same sum and K_ii = 1 exactly
//   k_svm_gram_hik      sum_k min(x_ik, x_jk) in double with k ascending (libsvm's order: Q and QD are libsvm's bits), the operand
//                       tiles staged through LDS
//   k_svm_finish_sv     rho, objective, counts as above, and in the same pass the support-vector indices and (float)(alpha_i y_i)
//   k_svm_gather_sv     the support vectors' rows into a dense [n_sv][d] buffer
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
    double gamma, coef0;
    int32_t kernel, degree;    // FD_KERNEL_*
};

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

// the linear kernel: the zero rows make the padding of Q zero
__global__ __launch_bounds__(64) void k_svm_gram(const SvmProbDev* __restrict__ P) {
    const SvmProbDev p = P[blockIdx.z];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti * 16 >= p.n_pad || tj * 16 >= p.n_pad) return;
    const f64x4 acc = svm_dot_tile(p, ti, tj);
    const double K[4] = {acc[0], acc[1], acc[2], acc[3]};
    svm_store_tile(p, ti, tj, K);
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

// Linear, polynomial and RBF kernel on the dot tile.  xsPass: the diagonal tiles only (blockIdx.x), which write xs_i = x_i . x_i
// and nothing else; the launch over all tiles that follows accumulates its diagonal in the same order, so that
// (xs_i + xs_i) - 2 dot_ii = 0 and K_ii = exp(-0) = 1 exactly, as where x_square and dot are one function.  The padding is
// written as zero (a kernel of the zero rows is not).
__global__ __launch_bounds__(64) void k_svm_gram_kernel(const SvmProbDev* __restrict__ P, int xsPass) {
    const SvmProbDev p = P[blockIdx.z];
    const int ti = xsPass ? blockIdx.x : blockIdx.y, tj = blockIdx.x;
    if (ti * 16 >= p.n_pad || tj * 16 >= p.n_pad) return;
    const f64x4 acc = svm_dot_tile(p, ti, tj);
    const int lane = threadIdx.x, col = tj * 16 + (lane & 15);
    if (xsPass) {
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
        if (p.kernel == FD_KERNEL_POLY) v = svm_powi(p.gamma * v + p.coef0, p.degree);
        else if (p.kernel == FD_KERNEL_RBF) v = exp(-p.gamma * ((p.xs[row] + p.xs[col]) - 2.0 * v));
        K[q] = (row < p.n && col < p.n) ? v : 0.0;
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

// (value, index) of the larger value, ties to the higher index: what a scan in index order with >= leaves
__device__ __forceinline__ void svm_take_max(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi > i)) { v = ov; i = oi; }
}
// the smaller value, ties to the higher index (a scan with <=)
__device__ __forceinline__ void svm_take_min(double& v, int& i, double ov, int oi) {
    if (ov < v || (ov == v && oi > i)) { v = ov; i = oi; }
}

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

// Solver::Solve's loop.  Every thread owns the elements tid, tid + 256, ...; the two selections are reduced over the
// wavefront by shuffles and over the four wavefronts through LDS slots, after which every thread holds i, j and performs the
// two-variable update redundantly.  Three barriers per iteration: behind either selection, and between reading alpha / G of
// (i, j) and their owners' writes.
__global__ __launch_bounds__(SVM_SMO_THREADS) void k_svm_smo(const SvmProbDev* __restrict__ P, int budget) {
    extern __shared__ double svm_lds[];
    const SvmProbDev p = P[blockIdx.x];
    if (p.state[1] || p.state[0] >= p.max_iter) return;   // done in an earlier launch (a batch relaunches until its last problem is done)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = p.n, np = p.n_pad, n_pos = p.n_pos;
    double* sAlpha = svm_lds;
    double* sG = sAlpha + np;
    double* sQD = sG + np;
    double* slotAv = sQD + np;                        // [4] Gmax of a wavefront
    double* slotBv = slotAv + SVM_SMO_WAVES;          // [4] its smallest obj_diff
    double* slotBg = slotBv + SVM_SMO_WAVES;          // [4] its Gmax2
    int* slotAi = (int*)(slotBg + SVM_SMO_WAVES);     // [4]
    int* slotBi = slotAi + SVM_SMO_WAVES;             // [4]
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
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) svm_take_max(gmax, gi, __shfl_xor(gmax, o, 64), __shfl_xor(gi, o, 64));
        if (lane == 0) { slotAv[wave] = gmax; slotAi[wave] = gi; }
        __syncthreads();
        gmax = slotAv[0];
        gi = slotAi[0];
#pragma unroll
        for (int w = 1; w < SVM_SMO_WAVES; ++w) svm_take_max(gmax, gi, slotAv[w], slotAi[w]);
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
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            svm_take_min(omin, gj, __shfl_xor(omin, o, 64), __shfl_xor(gj, o, 64));
            gmax2 = fmax(gmax2, __shfl_xor(gmax2, o, 64));
        }
        if (lane == 0) { slotBv[wave] = omin; slotBi[wave] = gj; slotBg[wave] = gmax2; }
        __syncthreads();
        omin = slotBv[0];
        gj = slotBi[0];
        gmax2 = slotBg[0];
#pragma unroll
        for (int w = 1; w < SVM_SMO_WAVES; ++w) {
            svm_take_min(omin, gj, slotBv[w], slotBi[w]);
            gmax2 = fmax(gmax2, slotBg[w]);
        }
        const int j = gj;
        if (gmax + gmax2 < eps || i < 0 || j < 0) {   // optimal (without a pair only when the Gram holds a NaN)
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
    if (tid == 0) {
        p.state[0] = iter;
        p.state[1] = converged;
    }
}

// k_svm_smo for up to SVM_LARGE_MAX_N examples: one workgroup of 1024 threads per problem, thread t owns the elements t,
// t + 1024, ... (at most 16).  G lives in LDS (8 n bytes, 128 KB at the limit) next to one status byte per element, the two set
// memberships the selections ask of alpha (libsvm's alpha_status; 16 KB).  alpha itself stays in global memory and is touched by
// the owners of i and j only; QD and the rows of Q are read through the cache.  The owners of i and j publish alpha and G of the
// pair through LDS slots, so that an iteration has three barriers as in k_svm_smo: behind either selection and behind the
// publication.  The arithmetic is k_svm_smo's.
__global__ __launch_bounds__(SVM_LARGE_THREADS) void k_svm_smo_large(const SvmProbDev* __restrict__ P, int budget) {
    extern __shared__ double svm_lds[];
    const SvmProbDev p = P[blockIdx.x];
    if (p.state[1] || p.state[0] >= p.max_iter) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = p.n, np = p.n_pad, n_pos = p.n_pos;
    double* sG = svm_lds;
    double* slotAv = sG + np;                          // [16] Gmax of a wavefront
    double* slotBv = slotAv + SVM_LARGE_WAVES;         // [16] its smallest obj_diff
    double* slotBg = slotBv + SVM_LARGE_WAVES;         // [16] its Gmax2
    double* pub = slotBg + SVM_LARGE_WAVES;            // alpha_i, G_i, alpha_j, G_j
    int* slotAi = (int*)(pub + 4);                     // [16]
    int* slotBi = slotAi + SVM_LARGE_WAVES;            // [16]
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
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) svm_take_max(gmax, gi, __shfl_xor(gmax, o, 64), __shfl_xor(gi, o, 64));
        if (lane == 0) { slotAv[wave] = gmax; slotAi[wave] = gi; }
        __syncthreads();
        gmax = slotAv[0];
        gi = slotAi[0];
#pragma unroll
        for (int w = 1; w < SVM_LARGE_WAVES; ++w) svm_take_max(gmax, gi, slotAv[w], slotAi[w]);
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
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            svm_take_min(omin, gj, __shfl_xor(omin, o, 64), __shfl_xor(gj, o, 64));
            gmax2 = fmax(gmax2, __shfl_xor(gmax2, o, 64));
        }
        if (lane == 0) { slotBv[wave] = omin; slotBi[wave] = gj; slotBg[wave] = gmax2; }
        __syncthreads();
        omin = slotBv[0];
        gj = slotBi[0];
        gmax2 = slotBg[0];
#pragma unroll
        for (int w = 1; w < SVM_LARGE_WAVES; ++w) {
            svm_take_min(omin, gj, slotBv[w], slotBi[w]);
            gmax2 = fmax(gmax2, slotBg[w]);
        }
        const int j = gj;
        if (gmax + gmax2 < eps || i < 0 || j < 0) {
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
    if (tid == 0) {
        p.state[0] = iter;
        p.state[1] = converged;
    }
}

// The pieces of k_svm_finish and k_svm_finish_large.  Only for a problem that is done (converged or at max_iterations); for one
// that the solver goes on with in the next launch the host needs the progress only.
__device__ __forceinline__ bool svm_finish_pending(const SvmProbDev& p, bool first) {
    if (p.state[1] || p.state[0] >= p.max_iter) return false;
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
        obj += a * (g + -1.0);
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

// rho, objective and counts by thread 0 of a problem's first block (alpha and G staged in LDS), and the single weight vector,
// one thread per dimension
__global__ __launch_bounds__(256) void k_svm_finish(const SvmProbDev* __restrict__ P) {
    __shared__ double sA[SVM_MAX_N], sGf[SVM_MAX_N];
    const SvmProbDev p = P[blockIdx.y];
    const int tid = threadIdx.x, n = p.n;
    if (svm_finish_pending(p, blockIdx.x == 0 && tid == 0)) return;
    svm_finish_weight(p, blockIdx.x * 256 + tid);
    if (blockIdx.x != 0) return;
    for (int i = tid; i < n; i += 256) {
        sA[i] = p.alpha[i];
        sGf[i] = p.G[i];
    }
    __syncthreads();
    if (tid != 0) return;
    svm_finish_info<false>(p, sA, sGf);
}

// the same for a problem of k_svm_smo_large: the one thread reads alpha and G from memory
__global__ __launch_bounds__(256) void k_svm_finish_large(const SvmProbDev* __restrict__ P) {
    const SvmProbDev p = P[blockIdx.y];
    const int tid = threadIdx.x;
    if (svm_finish_pending(p, blockIdx.x == 0 && tid == 0)) return;
    svm_finish_weight(p, blockIdx.x * 256 + tid);
    if (blockIdx.x == 0 && tid == 0) svm_finish_info<false>(p, p.alpha, p.G);
}

// The finish of the support-vector form, one block per problem: no weight vector; the sequential pass also writes sv_index and
// coef.  Large: alpha and G are read from memory as in k_svm_finish_large.
template <bool Large>
__global__ __launch_bounds__(256) void k_svm_finish_sv(const SvmProbDev* __restrict__ P) {
    __shared__ double sA[Large ? 1 : SVM_MAX_N], sGf[Large ? 1 : SVM_MAX_N];
    const SvmProbDev p = P[blockIdx.x];
    const int tid = threadIdx.x, n = p.n;
    if (svm_finish_pending(p, tid == 0)) return;
    if (Large) {
        if (tid == 0) svm_finish_info<true>(p, p.alpha, p.G);
        return;
    }
    for (int i = tid; i < n; i += 256) {
        sA[i] = p.alpha[i];
        sGf[i] = p.G[i];
    }
    __syncthreads();
    if (tid == 0) svm_finish_info<true>(p, sA, sGf);
}

// sv[q][k] = x[sv_index[q]][k] for the n_sv support vectors that k_svm_finish_sv listed (none while the problem is pending): one
// thread per element, consecutive threads along d
__global__ __launch_bounds__(256) void k_svm_gather_sv(const SvmProbDev* __restrict__ P) {
    const SvmProbDev p = P[blockIdx.y];
    if (!p.sv) return;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)p.info->n_sv * p.d) return;
    const size_t q = e / p.d;
    p.sv[e] = p.x[(size_t)p.sv_index[q] * p.d + (e - q * p.d)];
}

struct SvmTrainScratch {
    DevBuf x, q, dbl, w, desc, info, state;
    DevBuf xs, svList, sv;   // the support-vector form: xs; sv_index and coef; the gathered rows
};

// The support-vector form of a run (fd_kernel_svm_*): the checked kernel and, per problem, where the model goes (host).  The
// first n_sv entries of sv_index / coefficients and the first n_sv rows of support_vectors are written.
struct SvmSvOut {
    int32_t* sv_index;
    float* coefficients;
    float* support_vectors;           // n x d, or NULL
    std::vector<float>* sv_store;     // in place of support_vectors: resized to n_sv x d
};
struct SvmSvForm {
    int32_t kernel, degree;
    double gamma, coef0;
    const SvmSvOut* outs;             // count entries, or NULL (the Gram alone)
};

SvmSvForm svm_checked_kernel(const char* who, const fd_svm_kernel* k) {
    if (!k) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    SvmSvForm f = {k->kernel, 0, 0.0, 0.0, nullptr};
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

void svm_check_shape(const char* who, int n_pos, int n_neg, int d, int maxN = SVM_MAX_N) {
    if (n_pos < 1 || n_neg < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: needs at least one positive and one negative example (%d, %d)", who, n_pos, n_neg);
    if ((int64_t)n_pos + n_neg > maxN) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %lld examples, at most %d", who, (long long)n_pos + n_neg, maxN);
    if (d < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the feature length must be positive (%d)", who, d);
}

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

// wOverride: device buffer that receives problem 0's weights in place of the scratch (the tracker's dweights)
// large: the problems of fd_linear_svm_train_large (up to SVM_LARGE_MAX_N examples, Q always in memory)
// form: the support-vector form with its kernel; NULL: the linear weight-vector form
void svm_prepare(fd_ctx* ctx, const char* who, int count, const fd_svm_train_problem* probs, const fd_svm_train_params& prm, float* wOverride,
                 SvmRun& run, bool large = false, const SvmSvForm* form = nullptr) {
    SvmTrainScratch& sc = fd_scratch<SvmTrainScratch>(ctx);
    size_t xBytes = 0, qBytes = 0, dblBytes = 0, wBytes = 0, outBytes = 0, xsBytes = 0, listBytes = 0, svBytes = 0;
    auto wantsRows = [&](int c) { return form && form->outs && (form->outs[c].support_vectors || form->outs[c].sv_store); };
    for (int c = 0; c < count; ++c) {
        const fd_svm_train_problem& pr = probs[c];
        svm_check_shape(who, pr.n_pos, pr.n_neg, pr.d, large ? SVM_LARGE_MAX_N : SVM_MAX_N);
        if (!pr.x) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
        const size_t n = (size_t)pr.n_pos + pr.n_neg, np = (size_t)svm_pad((int)n);
        if (!pr.is_device) xBytes += svm_align(sizeof(float) * n * pr.d);
        qBytes += svm_align(sizeof(float) * np * np);
        dblBytes += svm_align(sizeof(double) * np * 3);
        wBytes += svm_align(sizeof(float) * pr.d);
        outBytes += svm_align(sizeof(float) * pr.d) + svm_align(sizeof(double) * np);
        if (form) {
            xsBytes += svm_align(sizeof(double) * np);
            listBytes += svm_align(2 * sizeof(int32_t) * np);
            outBytes += svm_align(2 * sizeof(int32_t) * np);
            if (wantsRows(c)) svBytes += svm_align(sizeof(float) * n * pr.d);
        }
    }
    sc.x.reserve(xBytes);
    try {
        sc.q.reserve(qBytes);
    } catch (const FdError& e) {   // up to 1 GiB for a large problem: the caller learns what did not fit
        FD_THROW(FD_ERR_RUNTIME, "%s: no device memory for Q (%zu bytes): %s", who, qBytes, e.msg.c_str());
    }
    sc.dbl.reserve(dblBytes);
    sc.w.reserve(wBytes);
    sc.desc.reserve(sizeof(SvmProbDev) * count);
    sc.info.reserve(sizeof(fd_svm_train_info) * count);
    sc.state.reserve(sizeof(int32_t) * 2 * count);
    if (form) {
        sc.xs.reserve(xsBytes);
        sc.svList.reserve(listBytes);
        try {
            sc.sv.reserve(svBytes);
        } catch (const FdError& e) {
            FD_THROW(FD_ERR_RUNTIME, "%s: no device memory for the support vectors (%zu bytes): %s", who, svBytes, e.msg.c_str());
        }
    }
    run.infoOff = svm_align(sizeof(SvmProbDev) * count);
    const size_t xOff = run.infoOff + svm_align(sizeof(fd_svm_train_info) * count);
    size_t outOff = xOff + xBytes;
    run.pinned = (char*)fd_pinned(ctx, outOff + outBytes);
    SvmProbDev* hd = (SvmProbDev*)run.pinned;
    run.h.resize(count);
    run.outW.resize(count);
    run.outA.resize(count);
    run.outS.resize(count);
    size_t xo = 0, qo = 0, dblo = 0, wo = 0, xso = 0, listo = 0, svo = 0;
    for (int c = 0; c < count; ++c) {
        const fd_svm_train_problem& pr = probs[c];
        const int n = pr.n_pos + pr.n_neg, np = svm_pad(n);
        SvmProbDev& D = run.h[c];
        if (pr.is_device) {
            D.x = pr.x;
        } else {
            D.x = (const float*)((char*)sc.x.p + xo);
            std::memcpy(run.pinned + xOff + xo, pr.x, sizeof(float) * (size_t)n * pr.d);
            xo += svm_align(sizeof(float) * (size_t)n * pr.d);
        }
        D.Q = (float*)((char*)sc.q.p + qo);
        qo += svm_align(sizeof(float) * (size_t)np * np);
        D.QD = (double*)((char*)sc.dbl.p + dblo);
        D.alpha = D.QD + np;
        D.G = D.alpha + np;
        dblo += svm_align(sizeof(double) * (size_t)np * 3);
        D.w = (c == 0 && wOverride) ? wOverride : (float*)((char*)sc.w.p + wo);
        wo += svm_align(sizeof(float) * pr.d);
        run.outW[c] = outOff;
        outOff += svm_align(sizeof(float) * pr.d);
        run.outA[c] = outOff;
        outOff += svm_align(sizeof(double) * (size_t)np);
        D.info = sc.info.as<fd_svm_train_info>() + c;
        D.state = sc.state.as<int32_t>() + 2 * c;
        D.Cp = prm.C * prm.weight_pos;
        D.Cn = prm.C * prm.weight_neg;
        D.eps = prm.eps;
        D.n_pos = pr.n_pos;
        D.n = n;
        D.n_pad = np;
        D.d = pr.d;
        D.q_in_lds = !large && svm_q_in_lds(n) ? 1 : 0;
        D.max_iter = prm.max_iterations > 0 ? prm.max_iterations : std::max(10000000, 100 * n);
        D.xs = nullptr;
        D.sv_index = nullptr;
        D.coef = nullptr;
        D.sv = nullptr;
        D.gamma = D.coef0 = 0.0;
        D.kernel = FD_KERNEL_LINEAR;
        D.degree = 0;
        if (form) {
            D.xs = (double*)((char*)sc.xs.p + xso);
            xso += svm_align(sizeof(double) * (size_t)np);
            D.sv_index = (int32_t*)((char*)sc.svList.p + listo);
            D.coef = (float*)(D.sv_index + np);
            listo += svm_align(2 * sizeof(int32_t) * (size_t)np);
            if (wantsRows(c)) {
                D.sv = (float*)((char*)sc.sv.p + svo);
                svo += svm_align(sizeof(float) * (size_t)n * pr.d);
            }
            run.outS[c] = outOff;
            outOff += svm_align(2 * sizeof(int32_t) * (size_t)np);
            D.gamma = form->gamma;
            D.coef0 = form->coef0;
            D.kernel = form->kernel;
            D.degree = form->degree;
        }
        hd[c] = D;
        run.maxPad = std::max(run.maxPad, np);
        run.maxD = std::max(run.maxD, pr.d);
        run.smoLds = std::max(run.smoLds, large ? svm_large_lds(n) : svm_smo_lds(n, D.q_in_lds != 0));
    }
    if (xBytes) HIP_CHECK(hipMemcpyAsync(sc.x.p, run.pinned + xOff, xBytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(sc.desc.p, hd, sizeof(SvmProbDev) * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(sc.state.p, 0, sizeof(int32_t) * 2 * count, ctx->stream));
    const dim3 tiles(run.maxPad / 16, run.maxPad / 16, count);
    if (!form) {
        hipLaunchKernelGGL(k_svm_gram, tiles, dim3(64), 0, ctx->stream, sc.desc.as<SvmProbDev>());
    } else if (form->kernel == FD_KERNEL_HIK) {
        hipLaunchKernelGGL(k_svm_gram_hik, tiles, dim3(64), 0, ctx->stream, sc.desc.as<SvmProbDev>());
    } else {
        if (form->kernel == FD_KERNEL_RBF) {   // xs first, from the diagonal tiles
            hipLaunchKernelGGL(k_svm_gram_kernel, dim3(run.maxPad / 16, 1, count), dim3(64), 0, ctx->stream, sc.desc.as<SvmProbDev>(), 1);
            HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_svm_gram_kernel, tiles, dim3(64), 0, ctx->stream, sc.desc.as<SvmProbDev>(), 0);
    }
    HIP_CHECK(hipGetLastError());
}

// Trains `count` problems in one set of launches; infos[c] is filled for every problem.  Problem 0's weights go to wOverride
// (device) when given.  Leaves ctx->stream synchronised.  large: one problem of up to SVM_LARGE_MAX_N examples on k_svm_smo_large.
// form: the support-vector form (the problems' weights are NULL; form->outs receives the model).
void svm_train_run(fd_ctx* ctx, const char* who, int count, const fd_svm_train_problem* probs, const fd_svm_train_params* params, float* wOverride,
                   fd_svm_train_info* infos, bool large, const SvmSvForm* form = nullptr) {
    const fd_svm_train_params prm = svm_checked_params(who, params);
    if (count < 1 || !probs || !infos) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument or no problem", who);
    HIP_CHECK(hipSetDevice(ctx->device));
    SvmRun run;
    svm_prepare(ctx, who, count, probs, prm, wOverride, run, large, form);
    SvmTrainScratch& sc = fd_scratch<SvmTrainScratch>(ctx);
    size_t rowElements = 0;   // the gather's grid: the largest n x d among the problems that want their support vectors' rows
    for (int c = 0; c < count; ++c)
        if (run.h[c].sv) rowElements = std::max(rowElements, (size_t)run.h[c].n * run.h[c].d);
    static uint64_t ldsAllowed = 0, ldsAllowedLarge = 0;
    if (large) fd_allow_lds(ctx, (const void*)k_svm_smo_large, (int)SVM_LDS_BUDGET, ldsAllowedLarge);
    else fd_allow_lds(ctx, (const void*)k_svm_smo, (int)SVM_LDS_BUDGET, ldsAllowed);
    const fd_svm_train_info* hinfo = (const fd_svm_train_info*)(run.pinned + run.infoOff);
    int launches = 0;
    for (;;) {
        if (large)
            hipLaunchKernelGGL(k_svm_smo_large, dim3(count), dim3(SVM_LARGE_THREADS), run.smoLds, ctx->stream, sc.desc.as<SvmProbDev>(), prm.launch_iterations);
        else
            hipLaunchKernelGGL(k_svm_smo, dim3(count), dim3(SVM_SMO_THREADS), run.smoLds, ctx->stream, sc.desc.as<SvmProbDev>(), prm.launch_iterations);
        HIP_CHECK(hipGetLastError());
        ++launches;
        if (form) {
            hipLaunchKernelGGL(large ? k_svm_finish_sv<true> : k_svm_finish_sv<false>, dim3(count), dim3(large ? 64 : 256), 0, ctx->stream,
                               sc.desc.as<SvmProbDev>());
            if (rowElements) {
                HIP_CHECK(hipGetLastError());
                hipLaunchKernelGGL(k_svm_gather_sv, dim3((unsigned)((rowElements + 255) / 256), count), dim3(256), 0, ctx->stream,
                                   sc.desc.as<SvmProbDev>());
            }
        } else {
            hipLaunchKernelGGL(large ? k_svm_finish_large : k_svm_finish, dim3((run.maxD + 255) / 256, count), dim3(256), 0, ctx->stream,
                               sc.desc.as<SvmProbDev>());
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(run.pinned + run.infoOff, sc.info.p, sizeof(fd_svm_train_info) * count, hipMemcpyDeviceToHost, ctx->stream));
        // the results ride along: in the usual case the first launch converges and this is the only wait
        for (int c = 0; c < count; ++c) {
            const SvmProbDev& D = run.h[c];
            if (probs[c].weights && !(c == 0 && wOverride))
                HIP_CHECK(hipMemcpyAsync(run.pinned + run.outW[c], D.w, sizeof(float) * D.d, hipMemcpyDeviceToHost, ctx->stream));
            if (probs[c].alpha) HIP_CHECK(hipMemcpyAsync(run.pinned + run.outA[c], D.alpha, sizeof(double) * D.n, hipMemcpyDeviceToHost, ctx->stream));
            if (form) HIP_CHECK(hipMemcpyAsync(run.pinned + run.outS[c], D.sv_index, 2 * sizeof(int32_t) * D.n_pad, hipMemcpyDeviceToHost, ctx->stream));
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
    if (!form) return;
    bool rows = false;
    for (int c = 0; c < count; ++c) {   // the lists from the staging area; the rows, whose number is known only now, straight from the device
        const SvmProbDev& D = run.h[c];
        const SvmSvOut& o = form->outs[c];
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

void svm_gram(fd_ctx* ctx, const char* who, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD, bool large,
              const SvmSvForm* form = nullptr) {
    HIP_CHECK(hipSetDevice(ctx->device));
    fd_svm_train_problem pr = {};
    pr.x = x;
    pr.n_pos = n_pos;
    pr.n_neg = n_neg;
    pr.d = d;
    pr.is_device = is_device;
    fd_svm_train_params prm = {1.0, 1.0, 1.0, 1e-4, 0, SVM_DEFAULT_LAUNCH_ITERATIONS};
    SvmRun run;
    svm_prepare(ctx, who, 1, &pr, prm, nullptr, run, large, form);
    const SvmProbDev& D = run.h[0];
    HIP_CHECK(hipMemcpy2DAsync(Q, sizeof(float) * D.n, D.Q, sizeof(float) * D.n_pad, sizeof(float) * D.n, D.n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(QD, D.QD, sizeof(double) * D.n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
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
}  // namespace

void fd_svm_train_run(fd_ctx* ctx, const char* who, int count, const fd_svm_train_problem* probs, const fd_svm_train_params* params, float* wOverride,
                      fd_svm_train_info* infos) {
    svm_train_run(ctx, who, count, probs, params, wOverride, infos, false);
}

extern "C" {

int fd_linear_svm_train_limits(int n_pos, int n_neg, int d, int* q_in_lds, int* max_iterations) {
    if (n_pos < 1 || n_neg < 1 || (int64_t)n_pos + n_neg > SVM_MAX_N || d < 1) return FD_ERR_INVALID_ARGUMENT;
    const int n = n_pos + n_neg;
    if (q_in_lds) *q_in_lds = svm_q_in_lds(n) ? 1 : 0;
    if (max_iterations) *max_iterations = std::max(10000000, 100 * n);
    return FD_OK;
}

int fd_linear_svm_train_large_limits(int n_pos, int n_neg, int d, int* lds_bytes, int* max_iterations) {
    if (n_pos < 1 || n_neg < 1 || (int64_t)n_pos + n_neg > SVM_LARGE_MAX_N || d < 1) return FD_ERR_INVALID_ARGUMENT;
    const int n = n_pos + n_neg;
    if (lds_bytes) *lds_bytes = (int)svm_large_lds(n);
    if (max_iterations) *max_iterations = std::max(10000000, 100 * n);
    return FD_OK;
}

int fd_linear_svm_gram(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !Q || !QD) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_gram: NULL argument");
        svm_gram(ctx, "fd_linear_svm_gram", x, n_pos, n_neg, d, is_device, Q, QD, false);
    });
}

int fd_linear_svm_gram_large(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, float* Q, double* QD) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !Q || !QD) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_gram_large: NULL argument");
        svm_gram(ctx, "fd_linear_svm_gram_large", x, n_pos, n_neg, d, is_device, Q, QD, true);
    });
}

int fd_linear_svm_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_train_params* params, float* weights,
                        float* bias, double* alpha, fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !weights || !bias || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train: NULL argument");
        const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, weights, bias, alpha);
        svm_train_run(ctx, "fd_linear_svm_train", 1, &pr, params, nullptr, info, false);
    });
}

int fd_linear_svm_train_large(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_train_params* params,
                              float* weights, float* bias, double* alpha, fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !weights || !bias || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train_large: NULL argument");
        const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, weights, bias, alpha);
        svm_train_run(ctx, "fd_linear_svm_train_large", 1, &pr, params, nullptr, info, true);
    });
}

int fd_linear_svm_train_batch(fd_ctx* ctx, int count, const fd_svm_train_problem* problems, const fd_svm_train_params* params, fd_svm_train_info* infos) {
    return fd_guard(ctx, [&] {
        if (!ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train_batch: NULL argument");
        if (count > 65535) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train_batch: %d problems, at most 65535", count);
        for (int c = 0; c < count && problems; ++c)
            if (!problems[c].weights || !problems[c].bias) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_linear_svm_train_batch: NULL argument in problem %d", c);
        fd_svm_train_run(ctx, "fd_linear_svm_train_batch", count, problems, params, nullptr, infos);
    });
}

/* ---- the support-vector form: any kernel of fd_svm_model ---- */
int fd_kernel_svm_train_limits(int n_pos, int n_neg, int d, int* q_in_lds, int* large, int* max_iterations) {
    if (n_pos < 1 || n_neg < 1 || (int64_t)n_pos + n_neg > SVM_LARGE_MAX_N || d < 1) return FD_ERR_INVALID_ARGUMENT;
    const int n = n_pos + n_neg;
    if (q_in_lds) *q_in_lds = n <= SVM_MAX_N && svm_q_in_lds(n) ? 1 : 0;
    if (large) *large = n > SVM_MAX_N ? 1 : 0;
    if (max_iterations) *max_iterations = std::max(10000000, 100 * n);
    return FD_OK;
}

int fd_kernel_svm_gram(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel, float* Q, double* QD) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !Q || !QD) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_gram: NULL argument");
        const SvmSvForm form = svm_checked_kernel("fd_kernel_svm_gram", kernel);
        svm_gram(ctx, "fd_kernel_svm_gram", x, n_pos, n_neg, d, is_device, Q, QD, (int64_t)n_pos + n_neg > SVM_MAX_N, &form);
    });
}

int fd_kernel_svm_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                        const fd_svm_train_params* params, int32_t* sv_index, float* coefficients, float* support_vectors, float* bias, double* alpha,
                        fd_svm_train_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !sv_index || !coefficients || !bias || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train: NULL argument");
        SvmSvForm form = svm_checked_kernel("fd_kernel_svm_train", kernel);
        const SvmSvOut out = {sv_index, coefficients, support_vectors, nullptr};
        form.outs = &out;
        const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, nullptr, bias, alpha);
        svm_train_run(ctx, "fd_kernel_svm_train", 1, &pr, params, nullptr, info, (int64_t)n_pos + n_neg > SVM_MAX_N, &form);
    });
}

int fd_kernel_svm_train_model(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_svm_kernel* kernel,
                              const fd_svm_train_params* params, float threshold, double logistic_a, double logistic_b, fd_svm** out,
                              fd_svm_train_info* info) {
    int rc = fd_guard(ctx, [&] {
        if (!ctx || !x || !out || !info) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_model: NULL argument");
        *out = nullptr;
        SvmSvForm form = svm_checked_kernel("fd_kernel_svm_train_model", kernel);
        svm_check_shape("fd_kernel_svm_train_model", n_pos, n_neg, d, SVM_LARGE_MAX_N);   // before the lists are sized by n
        const int n = n_pos + n_neg;
        std::vector<int32_t> svIndex(n);
        std::vector<float> coef(n), rows;
        float bias = 0.f;
        const SvmSvOut o = {svIndex.data(), coef.data(), nullptr, &rows};
        form.outs = &o;
        const fd_svm_train_problem pr = svm_single_problem(x, n_pos, n_neg, d, is_device, nullptr, &bias, nullptr);
        svm_train_run(ctx, "fd_kernel_svm_train_model", 1, &pr, params, nullptr, info, n > SVM_MAX_N, &form);
        if (info->n_sv < 1) FD_THROW(FD_ERR_RUNTIME, "fd_kernel_svm_train_model: the trained model has no support vector");
        fd_svm_model md = {};
        md.kernel = kernel->kernel;
        md.p0 = kernel->p0;
        md.p1 = kernel->p1;
        md.p2 = kernel->p2;
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
    });
    return rc;
}

int fd_kernel_svm_train_batch(fd_ctx* ctx, int count, const fd_kernel_svm_train_problem* problems, const fd_svm_kernel* kernel,
                              const fd_svm_train_params* params, fd_svm_train_info* infos) {
    return fd_guard(ctx, [&] {
        if (!ctx) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_batch: NULL argument");
        if (count > 65535) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_batch: %d problems, at most 65535", count);
        SvmSvForm form = svm_checked_kernel("fd_kernel_svm_train_batch", kernel);
        std::vector<fd_svm_train_problem> probs;
        std::vector<SvmSvOut> outs;
        for (int c = 0; c < count && problems; ++c) {
            const fd_kernel_svm_train_problem& pr = problems[c];
            if (!pr.sv_index || !pr.coefficients || !pr.bias) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_kernel_svm_train_batch: NULL argument in problem %d", c);
            probs.push_back(svm_single_problem(pr.x, pr.n_pos, pr.n_neg, pr.d, pr.is_device, nullptr, pr.bias, pr.alpha));
            outs.push_back(SvmSvOut{pr.sv_index, pr.coefficients, pr.support_vectors, nullptr});
        }
        form.outs = outs.data();
        svm_train_run(ctx, "fd_kernel_svm_train_batch", count, problems ? probs.data() : nullptr, params, nullptr, infos, false, &form);
    });
}

}  // extern "C"
