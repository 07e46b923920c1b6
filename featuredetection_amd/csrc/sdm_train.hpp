// featuredetection_amd/csrc/sdm_train.hpp -- supervised descent TRAINING: the ridge regressors of the cascade, learnt on the device.
// Included by sdm.hip behind its kernels (k_sdm_prepare, launch_descriptors, k_sdm_regress, k_sdm_update are used as they are).
//
// One cascade step of LandmarkBasedSupervisedDescentTraining::train (.cpp:297-365) / linearRegression (.cpp:439-518):
//   A      M x D feature matrix, D = L * len + 1: the descriptors of row r's shape on row r's image, then a 1
//   AtA    = A^T A, Atb = A^T (groundtruth - shapes): f32 x f32 products are exact in f64, sums over the rows in a fixed order on the
//          f64 MFMA pipe (k_st_gram: no split over M, no atomics), lower-triangle blocks only
//   lambda Manual: as given; Automatic: factor * ||AtA||_F / M (two-stage deterministic reduction)
//   Mreg   = AtA + lambda I (the bias entry left alone when regularise_affine == 0)
//   R      solves Mreg R = Atb: blocked right-looking Cholesky (panels of ST_NB columns: diagonal block in LDS, panel solve, trailing
//          update on the f64 MFMA pipe).  Atb^T rides below the matrix as 2L extra rows, so the panel solve and the trailing
//          update ARE the blocked forward substitution; a blocked backward substitution follows.  Rounded to float once.
//   x     += A R through k_sdm_regress + k_sdm_update, the kernels fd_sdm_optimize_batch runs (dist = 1)
//
// Deviations from the reference: Cholesky in double instead of Eigen's float full-pivoting LU inverse; AtA accumulated
// in double instead of float; EigenvalueThreshold regularisation is not built; the reference draws landmarks and boxes INTO the
// training images before it takes features from them (.cpp:263-264,273): not reproduced.
//
// Memory layout.  Every leading dimension is a multiple of 64 and every row count a multiple of the slab, padded with zeros, so that
// no load of the Gram kernel is predicated.  G is (lda + ldb) x lda doubles: rows [0, lda) hold AtA (lower triangle; the 64 x 64
// diagonal blocks are complete), rows [lda, lda + N) hold Atb^T.  A pivot that is <= 0 or NaN sets flag[0] (flag[1] = its index);
// every kernel returns at once when the flag is set, every loop is counted, nothing ever waits for the flag.
#pragma once

namespace {

constexpr int ST_BLK = 64;    // a workgroup of k_st_gram / k_st_chol_trail owns ST_BLK x ST_BLK outputs (4 wavefronts x 4 MFMA tiles)
constexpr int ST_KS = 32;     // rows of A per LDS slab
constexpr int ST_LDS = 80;    // floats per slab row in LDS: the four k rows of an MFMA operand fall on different banks
constexpr int ST_NB = 32;     // Cholesky panel width
constexpr int ST_NORM_BLOCKS = 1024;

__host__ __device__ inline int st_ru(int v, int m) { return (v + m - 1) / m * m; }

// block t of the lower triangle (row-major over block rows): t = bi (bi + 1) / 2 + bj, bj <= bi
__device__ __forceinline__ void st_tri(int t, int& bi, int& bj) {
    int b = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    if ((b + 1) * (b + 2) / 2 <= t) ++b;
    if (b * (b + 1) / 2 > t) --b;
    bi = b;
    bj = t - b * (b + 1) / 2;
}

// C[bi*64 + i][bj*64 + j] = sum_k X[k][bi*64 + i] * Y[k][bj*64 + j], k = 0 .. Mpad-1 in order.  tri: blockIdx.x walks the lower
// triangle of blocks (X == Y == A: AtA); else blockIdx.x = bi, blockIdx.y = bj (X = b, Y = A: Atb^T).
// MFMA operands (v_mfma_f64_16x16x4_f64): lane supplies A[i = lane & 15][k = lane >> 4] and B[k = lane >> 4][j = lane & 15];
// C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.
__global__ __launch_bounds__(256) void k_st_gram(const float* __restrict__ X, int ldx, const float* __restrict__ Y, int ldy, int Mpad,
                                                 double* __restrict__ Cm, int ldc, int tri) {
    __shared__ __attribute__((aligned(16))) float Xs[ST_KS * ST_LDS];
    __shared__ __attribute__((aligned(16))) float Ys[ST_KS * ST_LDS];
    int bi, bj;
    if (tri) st_tri((int)blockIdx.x, bi, bj);
    else { bi = blockIdx.x; bj = blockIdx.y; }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
    // slab loads: 32 rows x 16 float4 per operand, two per thread
    const int r0 = tid >> 4, c4 = (tid & 15) * 4;
    const float* xp = X + (size_t)r0 * ldx + (size_t)bi * ST_BLK + c4;
    const float* yp = Y + (size_t)r0 * ldy + (size_t)bj * ST_BLK + c4;
    float4 xr0 = *reinterpret_cast<const float4*>(xp), xr1 = *reinterpret_cast<const float4*>(xp + (size_t)16 * ldx);
    float4 yr0 = *reinterpret_cast<const float4*>(yp), yr1 = *reinterpret_cast<const float4*>(yp + (size_t)16 * ldy);
    const int nslab = Mpad / ST_KS;
    for (int s = 0; s < nslab; ++s) {
        *reinterpret_cast<float4*>(&Xs[r0 * ST_LDS + c4]) = xr0;
        *reinterpret_cast<float4*>(&Xs[(r0 + 16) * ST_LDS + c4]) = xr1;
        *reinterpret_cast<float4*>(&Ys[r0 * ST_LDS + c4]) = yr0;
        *reinterpret_cast<float4*>(&Ys[(r0 + 16) * ST_LDS + c4]) = yr1;
        __syncthreads();
        if (s + 1 < nslab) {   // the next slab is on its way while this one is multiplied
            const size_t k1 = (size_t)(s + 1) * ST_KS;
            xr0 = *reinterpret_cast<const float4*>(xp + k1 * ldx);
            xr1 = *reinterpret_cast<const float4*>(xp + (k1 + 16) * ldx);
            yr0 = *reinterpret_cast<const float4*>(yp + k1 * ldy);
            yr1 = *reinterpret_cast<const float4*>(yp + (k1 + 16) * ldy);
        }
#pragma unroll
        for (int k = 0; k < ST_KS; k += 4) {
            const double a = (double)Xs[(k + kq) * ST_LDS + w * 16 + li];
            const float* yk = &Ys[(k + kq) * ST_LDS + li];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)yk[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)yk[16], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)yk[32], acc2, 0, 0, 0);
            acc3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)yk[48], acc3, 0, 0, 0);
        }
        __syncthreads();
    }
    double* cp = Cm + (size_t)(bi * ST_BLK + w * 16 + kq) * ldc + bj * ST_BLK + li;
    auto put = [&](int t, const f64x4& v) {
        cp[t * 16] = v.x; cp[(size_t)4 * ldc + t * 16] = v.y; cp[(size_t)8 * ldc + t * 16] = v.z; cp[(size_t)12 * ldc + t * 16] = v.w;
    };
    put(0, acc0); put(1, acc1); put(2, acc2); put(3, acc3);
}

// sum of squares of the symmetric n x n matrix from its lower triangle: stage 1, block b takes rows b, b + gridDim.x, ...
__global__ __launch_bounds__(256) void k_st_norm1(const double* __restrict__ G, int ldg, int n, double* __restrict__ parts) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const double* row = G + (size_t)i * ldg;
        for (int j = threadIdx.x; j <= i; j += 256) {
            const double v = row[j];
            s = s + (j < i ? 2.0 : 1.0) * (v * v);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) parts[blockIdx.x] = red[0];
}
// stage 2 and lambda: scal[0] = lambda, scal[1] = ||AtA||_F.  Manual (nparts == 0): lambda = value.
__global__ __launch_bounds__(256) void k_st_lambda(const double* __restrict__ parts, int nparts, int automatic, double value, int M,
                                                   double* __restrict__ scal) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s = s + parts[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double nrm = sqrt(red[0]);
        scal[1] = nrm;
        scal[0] = automatic ? value * nrm / (double)M : value;
    }
}
__global__ void k_st_add_diag(double* __restrict__ G, int ldg, int nreg, const double* __restrict__ scal) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nreg) G[(size_t)i * ldg + i] = G[(size_t)i * ldg + i] + scal[0];
}

// ---- blocked right-looking Cholesky, G = L L^T in place (lower triangle), with the right-hand-side rows below
// diagonal block [j0, j0 + nb): one workgroup, one thread per element, in LDS
__global__ __launch_bounds__(1024) void k_st_chol_diag(double* __restrict__ G, int ldg, int j0, int nb, int32_t* __restrict__ flag) {
    __shared__ double T[ST_NB][ST_NB + 1];
    if (flag[0]) return;
    const int i = threadIdx.x / ST_NB, j = threadIdx.x % ST_NB;
    const bool in = i < nb && j <= i;
    T[i][j] = in ? G[(size_t)(j0 + i) * ldg + j0 + j] : 0.0;
    for (int c = 0; c < nb; ++c) {
        __syncthreads();
        const double p = T[c][c];
        if (!(p > 0.0)) {   // <= 0 or NaN; uniform: every thread reads the same p
            if (threadIdx.x == 0) { flag[1] = j0 + c; flag[0] = 1; }
            return;
        }
        const double d = sqrt(p);
        __syncthreads();
        if (j == c && i >= c && i < nb) T[i][c] = i == c ? d : T[i][c] / d;
        __syncthreads();
        if (in && j > c) T[i][j] = T[i][j] - T[i][c] * T[j][c];
    }
    __syncthreads();
    if (in) G[(size_t)(j0 + i) * ldg + j0 + j] = T[i][j];
}
// rows below the diagonal block: X L11^T = A21, one thread per row (the right-hand-side rows included: forward substitution)
__global__ __launch_bounds__(64) void k_st_chol_panel(double* __restrict__ G, int ldg, int j0, int nb, int nrows, const int32_t* __restrict__ flag) {
    __shared__ double Ls[ST_NB][ST_NB + 1];
    __shared__ double xs[64][ST_NB + 1];
    if (flag[0]) return;
    for (int e = threadIdx.x; e < ST_NB * ST_NB; e += 64) {
        const int i = e / ST_NB, j = e % ST_NB;
        Ls[i][j] = (i < nb && j <= i) ? G[(size_t)(j0 + i) * ldg + j0 + j] : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    const int r = j0 + nb + blockIdx.x * 64 + threadIdx.x;
    if (r >= nrows) return;
    double* row = G + (size_t)r * ldg + j0;
    double* x = xs[threadIdx.x];   // the thread's row lives in LDS: counted loops, nothing unrolled into registers
    for (int c = 0; c < nb; ++c) x[c] = row[c];
    for (int c = 0; c < nb; ++c) {
        double s = x[c];
        for (int t = 0; t < c; ++t) s = s - x[t] * Ls[c][t];
        x[c] = s / Ls[c][c];
    }
    for (int c = 0; c < nb; ++c) row[c] = x[c];
}
// trailing update G[i][j] -= sum_k L[i][j0 + k] L[j][j0 + k] for c0 <= j < n, j <= i < nrows (c0 = j0 + nb): blocks of 64 x 64 from
// (c0, c0), tiles wholly above the diagonal or outside the matrix are skipped (wave-uniform tests)
__global__ __launch_bounds__(256) void k_st_chol_trail(double* __restrict__ G, int ldg, int j0, int nb, int n, int nrows, const int32_t* __restrict__ flag) {
    if (flag[0]) return;
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const int c0 = j0 + nb;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    const int rt = c0 + bi * ST_BLK + w * 16;
    if (rt >= nrows) return;
    constexpr int KS = ST_NB / 4;   // only full panels have a trailing matrix: the launch passes nb == ST_NB
    double a[KS];
    {
        const double* ar = G + (size_t)(rt + li) * ldg + j0;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = -ar[4 * s + kq];
    }
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
        const int ct = c0 + bj * ST_BLK + t * 16;
        if (ct >= n || ct > rt + 15) continue;
        const double* br = G + (size_t)(ct + li) * ldg + j0;
        double b[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) b[s] = br[4 * s + kq];
        f64x4 acc;
        double* cp = G + (size_t)(rt + kq) * ldg + ct + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = cp[(size_t)(4 * r) * ldg];
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) cp[(size_t)(4 * r) * ldg] = acc[r];
    }
}
// ---- backward substitution on the right-hand-side rows (row j of them is y_j^T, becomes r_j^T with r_j^T L = y_j^T)
__global__ __launch_bounds__(64) void k_st_back_diag(double* __restrict__ G, int ldg, int j0, int nb, int rhs0, int N, const int32_t* __restrict__ flag) {
    __shared__ double Ls[ST_NB][ST_NB + 1];
    __shared__ double xs[64][ST_NB + 1];
    if (flag[0]) return;
    for (int e = threadIdx.x; e < ST_NB * ST_NB; e += 64) {
        const int i = e / ST_NB, j = e % ST_NB;
        Ls[i][j] = (i < nb && j <= i) ? G[(size_t)(j0 + i) * ldg + j0 + j] : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= N) return;
    double* row = G + (size_t)(rhs0 + j) * ldg + j0;
    double* x = xs[threadIdx.x];
    for (int c = 0; c < nb; ++c) x[c] = row[c];
    for (int c = nb - 1; c >= 0; --c) {
        double s = x[c];
        for (int t = nb - 1; t > c; --t) s = s - x[t] * Ls[t][c];
        x[c] = s / Ls[c][c];
    }
    for (int c = 0; c < nb; ++c) row[c] = x[c];
}
// y_j[i] -= sum_c r_j[j0 + c] L[j0 + c][i] for i < j0; blockIdx.y = j
__global__ __launch_bounds__(256) void k_st_back_update(double* __restrict__ G, int ldg, int j0, int nb, int rhs0, const int32_t* __restrict__ flag) {
    if (flag[0]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= j0) return;
    double* row = G + (size_t)(rhs0 + blockIdx.y) * ldg;
    double s = row[i];
    for (int c = 0; c < nb; ++c) s = s - row[j0 + c] * G[(size_t)(j0 + c) * ldg + i];
    row[i] = s;
}
// R[d][j] = (float) r_j[d]; row biasSrc (if >= 0) goes to row biasDst instead (the trainer keeps the bias row apart, see sdm_train_run)
__global__ void k_st_round(const double* __restrict__ G, int ldg, int rhs0, int n, int N, float* __restrict__ R, int biasSrc, int biasDst,
                           const int32_t* __restrict__ flag) {
    if (flag[0]) return;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n * N) return;
    const int j = (int)(idx / n), d = (int)(idx - (int64_t)j * n);
    R[(size_t)(d == biasSrc ? biasDst : d) * N + j] = (float)G[(size_t)(rhs0 + j) * ldg + d];
}

// ---- the trainer's own small kernels
__global__ void k_st_ones(float* __restrict__ A, int lda, int col, int M) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < M) A[(size_t)r * lda + col] = 1.0f;
}
// b = groundtruth - shapes (float subtraction, as cv::Mat does)
__global__ void k_st_delta(const float* __restrict__ gt, const float* __restrict__ x, int M, int N, float* __restrict__ Bm, int ldb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * N) return;
    const int r = idx / N, j = idx - r * N;
    Bm[(size_t)r * ldb + j] = gt[idx] - x[idx];
}
// out[0] = ||gt - x||_1 / count (.cpp:293,363), out[1] = ||gt - x||_F, in double, one workgroup, fixed order
__global__ __launch_bounds__(1024) void k_st_err(const float* __restrict__ gt, const float* __restrict__ x, int64_t count, double* __restrict__ out) {
    __shared__ double r1[1024], r2[1024];
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += 1024) {
        const double d = (double)(gt[i] - x[i]);
        s1 = s1 + fabs(d);
        s2 = s2 + d * d;
    }
    r1[threadIdx.x] = s1;
    r2[threadIdx.x] = s2;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            r1[threadIdx.x] = r1[threadIdx.x] + r1[threadIdx.x + h];
            r2[threadIdx.x] = r2[threadIdx.x] + r2[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = r1[0] / (double)count; out[1] = sqrt(r2[0]); }
}

struct SdmTrainScratch {
    DevBuf A, Bm, G, parts, scal, flag, R, shapes, gt, origin, dist, status, partial, errs;
    int lastD = 0, lastN = 0, lastLda = 0;   // the last successful fd_sdm_linear_regression: its double solution still sits in G
    // fd_ctx_set_kernel_timing: events around the phases of the last timed step (fd_sdm_train_last_phase_ms, fd_hip_bench.h)
    hipEvent_t ev[7] = {};
    bool timing = false, timed = false;
    ~SdmTrainScratch() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

void st_mark(SdmTrainScratch& sc, int i, hipStream_t st) {
    if (!sc.timing) return;
    if (!sc.ev[i]) HIP_CHECK(hipEventCreate(&sc.ev[i]));
    HIP_CHECK(hipEventRecord(sc.ev[i], st));
}

// device allocation of the trainer: a failure names the byte count (as fd_linear_svm_train_large does)
void st_reserve(DevBuf& b, size_t bytes, const char* who, const char* what) {
    try {
        b.reserve(bytes);
    } catch (const FdError&) {
        (void)hipGetLastError();
        FD_THROW(FD_ERR_RUNTIME, "%s: cannot allocate %zu bytes of device memory for %s (the training set does not fit the device)", who, bytes, what);
    }
}

struct StDims {
    int M, Mpad, D, lda, N, ldb;
    size_t g_bytes() const { return sizeof(double) * (size_t)(lda + ldb) * lda; }
};
StDims st_dims(int M, int D, int N) {
    StDims d;
    d.M = M; d.Mpad = st_ru(M, ST_KS); d.D = D; d.lda = st_ru(D, ST_BLK); d.N = N; d.ldb = st_ru(N, ST_BLK);
    return d;
}

// Queues normal equations, lambda, factorisation and both substitutions for A (Mpad x lda floats, zero padded) and Bm (Mpad x ldb)
// on `st`; R (float) receives the rounded solution.  Nothing waits.  afterGram (optional) runs between the Gram launches and the
// regularisation (read-back of AtA / Atb for the callers that want them).
template <class F>
void st_solve(fd_ctx* ctx, SdmTrainScratch& sc, hipStream_t st, const StDims& d, int automatic, double lambda, int regularise_affine, float* R,
              int biasSrc, int biasDst, F&& afterGram) {
    (void)ctx;
    double* G = sc.G.as<double>();
    int32_t* flag = sc.flag.as<int32_t>();
    double* scal = sc.scal.as<double>();
    const int nbk = d.lda / ST_BLK, ldg = d.lda, n = d.D, nrows = d.lda + d.ldb, rhs0 = d.lda;
    st_mark(sc, 1, st);
    HIP_CHECK(hipMemsetAsync(flag, 0, 2 * sizeof(int32_t), st));
    HIP_CHECK(hipMemsetAsync(G, 0, d.g_bytes(), st));
    hipLaunchKernelGGL(k_st_gram, dim3(nbk * (nbk + 1) / 2), dim3(256), 0, st, sc.A.as<float>(), d.lda, sc.A.as<float>(), d.lda, d.Mpad, G, ldg, 1);
    hipLaunchKernelGGL(k_st_gram, dim3(d.ldb / ST_BLK, nbk), dim3(256), 0, st, sc.Bm.as<float>(), d.ldb, sc.A.as<float>(), d.lda, d.Mpad,
                       G + (size_t)rhs0 * ldg, ldg, 0);
    st_mark(sc, 2, st);
    int nparts = 0;
    if (automatic) {
        nparts = std::min(n, ST_NORM_BLOCKS);
        hipLaunchKernelGGL(k_st_norm1, dim3(nparts), dim3(256), 0, st, G, ldg, n, sc.parts.as<double>());
    }
    hipLaunchKernelGGL(k_st_lambda, dim3(1), dim3(256), 0, st, sc.parts.as<double>(), nparts, automatic, lambda, d.M, scal);
    afterGram();
    const int nreg = regularise_affine ? n : n - 1;
    if (nreg > 0) hipLaunchKernelGGL(k_st_add_diag, dim3((nreg + 255) / 256), dim3(256), 0, st, G, ldg, nreg, scal);
    st_mark(sc, 3, st);
    for (int j0 = 0; j0 < n; j0 += ST_NB) {
        const int nb = std::min(ST_NB, n - j0), c0 = j0 + nb;
        hipLaunchKernelGGL(k_st_chol_diag, dim3(1), dim3(ST_NB * ST_NB), 0, st, G, ldg, j0, nb, flag);
        hipLaunchKernelGGL(k_st_chol_panel, dim3((nrows - c0 + 63) / 64), dim3(64), 0, st, G, ldg, j0, nb, nrows, flag);
        if (c0 < n)
            hipLaunchKernelGGL(k_st_chol_trail, dim3((nrows - c0 + ST_BLK - 1) / ST_BLK, (n - c0 + ST_BLK - 1) / ST_BLK), dim3(256), 0, st, G, ldg, j0, nb,
                               n, nrows, flag);
    }
    st_mark(sc, 4, st);
    for (int j0 = (n - 1) / ST_NB * ST_NB; j0 >= 0; j0 -= ST_NB) {
        const int nb = std::min(ST_NB, n - j0);
        hipLaunchKernelGGL(k_st_back_diag, dim3((d.N + 63) / 64), dim3(64), 0, st, G, ldg, j0, nb, rhs0, d.N, flag);
        if (j0 > 0) hipLaunchKernelGGL(k_st_back_update, dim3((j0 + 255) / 256, d.N), dim3(256), 0, st, G, ldg, j0, nb, rhs0, flag);
    }
    const int64_t cnt = (int64_t)n * d.N;
    hipLaunchKernelGGL(k_st_round, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, G, ldg, rhs0, n, d.N, R, biasSrc, biasDst, flag);
    st_mark(sc, 5, st);
    HIP_CHECK(hipGetLastError());
}

void st_check_reg(const char* who, int type, double lambda) {
    if (type == FD_SDM_REG_EIGENVALUE_THRESHOLD)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: EigenvalueThreshold regularisation needs Eigen's FullPivLU::maxPivot() * threshold() and is not built", who);
    if (type != FD_SDM_REG_MANUAL && type != FD_SDM_REG_AUTOMATIC) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: unknown regularisation type %d", who, type);
    if (!(lambda >= 0.0)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: lambda must be >= 0", who);
}

[[noreturn]] void st_throw_pivot(int pivot) {
    FD_THROW(FD_ERR_RUNTIME, "the regularised AtA is not positive definite (pivot %d); increase lambda", pivot);
}

// per step descriptor length of a trainer configuration (validated as fd_sdm_create validates a model's desc_params)
void st_step_lengths(const fd_sdm_train_params* prm, std::vector<int>& len, std::vector<int>& half) {
    if (!prm || !prm->desc_params) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train_params: NULL desc_params");
    if (prm->num_landmarks < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train_params: no landmarks");
    if (prm->num_steps < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train_params: no cascade steps");
    if (prm->hog_variant != 0 && prm->hog_variant != 1) FD_THROW(FD_ERR_LOGIC, "descriptorType does not match 'vlhog-dt' or 'vlhog-uoctti'");
    len.clear();
    half.clear();
    for (int s = 0; s < prm->num_steps; ++s) {
        const int32_t* dp = prm->desc_params + 3 * s;
        if (dp[0] < 1 || dp[1] < 1 || dp[2] < 1) FD_THROW(FD_ERR_LOGIC, "descriptorParameters must contain numCells, cellSize and numBins.");
        if (dp[0] > 8 || dp[1] < 2 || dp[1] > 64 || dp[2] > 32)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train_params.desc_params of step %d out of range: numCells %d (1..8), cellSize %d (2..64), numBins %d (1..32)",
                     s, dp[0], dp[1], dp[2]);
        DescParams p;
        half.push_back(dp[0] * (dp[1] / 2));
        fill_desc_params(p, 64, 64, prm->num_landmarks, false, prm->hog_variant, dp[0], dp[1], dp[2], 2 * half.back());
        len.push_back(p.len);
    }
}

size_t st_train_bytes(int M, int Dmax, int N, int L) {
    const StDims d = st_dims(M, Dmax, N);
    const size_t nch = (size_t)(d.lda + RG_KCHUNK - 1) / RG_KCHUNK;
    return sizeof(float) * (size_t)d.Mpad * d.lda + sizeof(float) * (size_t)d.Mpad * d.ldb + d.g_bytes() + sizeof(double) * nch * M * N +
           sizeof(float) * (size_t)(d.lda + 1) * N + 2 * sizeof(float) * (size_t)M * N + sizeof(int32_t) * 4 * (size_t)M * L + 8 * (size_t)M;
}

}  // namespace

extern "C" {

int fd_sdm_train_limits(const fd_sdm_train_params* params, int rows, int64_t* bytes, int* max_dim) {
    return fd_guard(nullptr, [&] {
        if (rows < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train_limits: no rows");
        std::vector<int> len, half;
        st_step_lengths(params, len, half);
        int Dmax = 0;
        for (int l : len) Dmax = std::max(Dmax, params->num_landmarks * l + 1);
        if (bytes) *bytes = (int64_t)st_train_bytes(rows, Dmax, 2 * params->num_landmarks, params->num_landmarks);
        if (max_dim) *max_dim = Dmax;
    });
}

int fd_sdm_train_step_dims(const fd_sdm_train_params* params, int32_t* dims) {
    return fd_guard(nullptr, [&] {
        if (!dims) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train_step_dims: NULL dims");
        std::vector<int> len, half;
        st_step_lengths(params, len, half);
        for (size_t s = 0; s < len.size(); ++s) dims[s] = params->num_landmarks * len[s] + 1;
    });
}

int fd_sdm_linear_regression(fd_ctx* ctx, const float* A, const float* b, int M, int D, int N, int type, double lambda, int regularise_affine,
                             float* x_out, double* lambda_out, double* ata_out, double* atb_out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !A || !b || !x_out || M < 1 || D < 1 || N < 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_linear_regression: bad argument");
        st_check_reg("fd_sdm_linear_regression", type, lambda);
        if ((int64_t)D > 32768 || (int64_t)N > 4096) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_linear_regression: D <= 32768 and N <= 4096");
        HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        SdmTrainScratch& sc = fd_scratch<SdmTrainScratch>(ctx);
        const StDims d = st_dims(M, D, N);
        const char* who = "fd_sdm_linear_regression";
        st_reserve(sc.A, sizeof(float) * (size_t)d.Mpad * d.lda, who, "A");
        st_reserve(sc.Bm, sizeof(float) * (size_t)d.Mpad * d.ldb, who, "b");
        st_reserve(sc.G, d.g_bytes(), who, "AtA");
        st_reserve(sc.parts, sizeof(double) * ST_NORM_BLOCKS, who, "partial sums");
        st_reserve(sc.scal, 2 * sizeof(double), who, "lambda");
        st_reserve(sc.flag, 2 * sizeof(int32_t), who, "flag");
        st_reserve(sc.R, sizeof(float) * (size_t)D * N, who, "R");
        HIP_CHECK(hipMemsetAsync(sc.A.p, 0, sizeof(float) * (size_t)d.Mpad * d.lda, st));
        HIP_CHECK(hipMemsetAsync(sc.Bm.p, 0, sizeof(float) * (size_t)d.Mpad * d.ldb, st));
        HIP_CHECK(hipMemcpy2DAsync(sc.A.p, sizeof(float) * d.lda, A, sizeof(float) * D, sizeof(float) * D, M, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpy2DAsync(sc.Bm.p, sizeof(float) * d.ldb, b, sizeof(float) * N, sizeof(float) * N, M, hipMemcpyHostToDevice, st));
        std::vector<double> tmp;
        sc.timing = ctx->kernel_timing;
        sc.timed = false;
        st_mark(sc, 0, st);
        st_solve(ctx, sc, st, d, type == FD_SDM_REG_AUTOMATIC, lambda, regularise_affine, sc.R.as<float>(), -1, -1, [&] {
            if (ata_out) {   // the lower triangle is what the device holds: mirrored here, where a consumer wants the full matrix
                HIP_CHECK(hipMemcpy2DAsync(ata_out, sizeof(double) * D, sc.G.p, sizeof(double) * d.lda, sizeof(double) * D, D, hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                for (int i = 0; i < D; ++i)
                    for (int j = i + 1; j < D; ++j) ata_out[(size_t)i * D + j] = ata_out[(size_t)j * D + i];
            }
            if (atb_out) {
                tmp.resize((size_t)N * D);
                HIP_CHECK(hipMemcpy2DAsync(tmp.data(), sizeof(double) * D, sc.G.as<double>() + (size_t)d.lda * d.lda, sizeof(double) * d.lda, sizeof(double) * D, N,
                                           hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                for (int j = 0; j < N; ++j)
                    for (int i = 0; i < D; ++i) atb_out[(size_t)i * N + j] = tmp[(size_t)j * D + i];
            }
        });
        st_mark(sc, 6, st);
        int32_t flag[2] = {0, 0};
        double scal[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(flag, sc.flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(scal, sc.scal.p, sizeof(scal), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        sc.timed = sc.timing;
        if (lambda_out) *lambda_out = scal[0];
        sc.lastD = 0;
        if (flag[0]) st_throw_pivot(flag[1]);
        HIP_CHECK(hipMemcpy(x_out, sc.R.p, sizeof(float) * (size_t)D * N, hipMemcpyDeviceToHost));
        sc.lastD = D; sc.lastN = N; sc.lastLda = d.lda;
    });
}

int fd_sdm_train_last_phase_ms(fd_ctx* ctx, float* ms6) {
    return fd_guard(ctx, [&] {
        if (!ctx || !ms6) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train_last_phase_ms: bad argument");
        SdmTrainScratch& sc = fd_scratch<SdmTrainScratch>(ctx);
        if (!sc.timed) FD_THROW(FD_ERR_LOGIC, "fd_sdm_train_last_phase_ms: no timed step on this context (fd_ctx_set_kernel_timing)");
        for (int i = 0; i < 6; ++i) HIP_CHECK(hipEventElapsedTime(&ms6[i], sc.ev[i], sc.ev[i + 1]));
    });
}

int fd_debug_sdm_linear_regression_solution(fd_ctx* ctx, int D, int N, double* x64_out) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x64_out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_debug_sdm_linear_regression_solution: bad argument");
        SdmTrainScratch& sc = fd_scratch<SdmTrainScratch>(ctx);
        if (sc.lastD < 1 || D != sc.lastD || N != sc.lastN)
            FD_THROW(FD_ERR_LOGIC, "fd_debug_sdm_linear_regression_solution: no solved system of %d x %d on this context", D, N);
        HIP_CHECK(hipSetDevice(ctx->device));
        std::vector<double> tmp((size_t)N * D);
        HIP_CHECK(hipMemcpy2D(tmp.data(), sizeof(double) * D, sc.G.as<double>() + (size_t)sc.lastLda * sc.lastLda, sizeof(double) * sc.lastLda,
                              sizeof(double) * D, N, hipMemcpyDeviceToHost));
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < D; ++i) x64_out[(size_t)i * N + j] = tmp[(size_t)j * D + i];
    });
}

int fd_sdm_train(fd_ctx* ctx, const fd_sdm_train_params* prm, const fd_sdm_train_group* groups, int num_groups, int samples_per_image,
                 const float* initial_shapes, const float* groundtruth, float* const* R_out, float* shapes_steps_out, int32_t* row_status_out,
                 fd_sdm_train_step_info* info_out) {
    return fd_guard(ctx, [&] {
        const char* who = "fd_sdm_train";
        if (!ctx || !prm || !groups || num_groups < 1 || samples_per_image < 1 || !initial_shapes || !groundtruth || !R_out)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train: bad argument");
        st_check_reg(who, prm->regularisation, prm->lambda);
        std::vector<int> len, half;
        st_step_lengths(prm, len, half);
        const int L = prm->num_landmarks, N = 2 * L, S = prm->num_steps, K = samples_per_image;
        int64_t nimg64 = 0;
        for (int g = 0; g < num_groups; ++g) {
            if (!groups[g].images || groups[g].width < 1 || groups[g].height < 1 || groups[g].count < 1)
                FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train: group %d is empty or has no images", g);
            nimg64 += groups[g].count;
        }
        if (nimg64 * K > (1 << 24)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train: more than 2^24 rows");
        // the shape kernels index rows x 2L elements with an int
        if (nimg64 * K * 2 * prm->num_landmarks >= (int64_t)1 << 31) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train: rows x 2L must stay below 2^31");
        const int nimg = (int)nimg64, M = nimg * K;
        int Dmax = 0;
        for (int s = 0; s < S; ++s) {
            if (!R_out[s]) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_sdm_train: R_out[%d] is NULL", s);
            Dmax = std::max(Dmax, L * len[s] + 1);
        }
        HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        SdmTrainScratch& sc = fd_scratch<SdmTrainScratch>(ctx);
        sc.lastD = 0;
        const StDims dm = st_dims(M, Dmax, N);
        const int nchunksMax = (dm.lda + RG_KCHUNK - 1) / RG_KCHUNK;
        st_reserve(sc.A, sizeof(float) * (size_t)dm.Mpad * dm.lda, who, "the feature matrix");
        st_reserve(sc.Bm, sizeof(float) * (size_t)dm.Mpad * dm.ldb, who, "the shape deltas");
        st_reserve(sc.G, dm.g_bytes(), who, "AtA");
        st_reserve(sc.partial, sizeof(double) * (size_t)nchunksMax * M * N, who, "the update's partial sums");
        st_reserve(sc.parts, sizeof(double) * ST_NORM_BLOCKS, who, "partial sums");
        st_reserve(sc.scal, 2 * sizeof(double), who, "lambda");
        st_reserve(sc.flag, 2 * sizeof(int32_t), who, "flag");
        st_reserve(sc.R, sizeof(float) * (size_t)(dm.lda + 1) * N, who, "R");
        st_reserve(sc.shapes, sizeof(float) * (size_t)M * N, who, "shapes");
        st_reserve(sc.gt, sizeof(float) * (size_t)M * N, who, "ground truth");
        st_reserve(sc.origin, sizeof(int32_t) * 4 * (size_t)M * L, who, "patch origins");
        st_reserve(sc.dist, sizeof(float) * (size_t)M, who, "dist");
        st_reserve(sc.status, sizeof(int32_t) * (size_t)M, who, "row status");
        st_reserve(sc.errs, 2 * sizeof(double), who, "errors");
        // images of the groups that are host memory
        std::vector<std::unique_ptr<DevBuf>> own(num_groups);
        std::vector<const uint8_t*> dimg(num_groups);
        std::vector<int> first(num_groups);
        for (int g = 0, f = 0; g < num_groups; ++g) {
            first[g] = f;
            f += groups[g].count;
            dimg[g] = groups[g].images;
            if (!groups[g].on_device) {
                const size_t bytes = (size_t)groups[g].width * groups[g].height * groups[g].count;
                own[g].reset(new DevBuf());
                st_reserve(*own[g], bytes, who, "images");
                HIP_CHECK(hipMemcpyAsync(own[g]->p, groups[g].images, bytes, hipMemcpyHostToDevice, st));
                dimg[g] = own[g]->as<uint8_t>();
            }
        }
        // rows: the caller's are image-major (image * K + sample); the trainer's are sample-major, so that the rows of one sample
        // over the images of one group are contiguous
        auto to_internal = [&](const float* src, std::vector<float>& dst) {
            dst.resize((size_t)M * N);
            for (int i = 0; i < nimg; ++i)
                for (int k = 0; k < K; ++k) std::memcpy(&dst[((size_t)k * nimg + i) * N], src + ((size_t)i * K + k) * N, sizeof(float) * N);
        };
        auto to_caller = [&](const float* src, float* dst) {
            for (int i = 0; i < nimg; ++i)
                for (int k = 0; k < K; ++k) std::memcpy(dst + ((size_t)i * K + k) * N, src + ((size_t)k * nimg + i) * N, sizeof(float) * N);
        };
        std::vector<float> hx, hgt;
        to_internal(initial_shapes, hx);
        to_internal(groundtruth, hgt);
        HIP_CHECK(hipMemcpyAsync(sc.shapes.p, hx.data(), sizeof(float) * hx.size(), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(sc.gt.p, hgt.data(), sizeof(float) * hgt.size(), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(sc.status.p, 0, sizeof(int32_t) * (size_t)M, st));
        if (shapes_steps_out) std::memcpy(shapes_steps_out, initial_shapes, sizeof(float) * (size_t)M * N);
        std::vector<std::vector<float>> Rh(S);
        std::vector<fd_sdm_train_step_info> info(S + 1);
        std::vector<int32_t> hstatus(M);
        double errs[2];
        hipLaunchKernelGGL(k_st_err, dim3(1), dim3(1024), 0, st, sc.gt.as<float>(), sc.shapes.as<float>(), (int64_t)M * N, sc.errs.as<double>());
        HIP_CHECK(hipMemcpyAsync(errs, sc.errs.p, sizeof(errs), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        info[0] = fd_sdm_train_step_info{0.0, errs[0], errs[1], M, 0, 0};
        for (int s = 0; s < S; ++s) {
            const int F = L * len[s], D = F + 1;
            const StDims d = st_dims(M, D, N);
            sc.timing = ctx->kernel_timing && s + 1 == S;   // fd_hip_bench.h: the phases of the last step
            sc.timed = false;
            st_mark(sc, 0, st);
            HIP_CHECK(hipMemsetAsync(sc.A.p, 0, sizeof(float) * (size_t)d.Mpad * d.lda, st));
            HIP_CHECK(hipMemsetAsync(sc.Bm.p, 0, sizeof(float) * (size_t)d.Mpad * d.ldb, st));
            HIP_CHECK(hipMemsetAsync(sc.R.p, 0, sizeof(float) * (size_t)(d.lda + 1) * N, st));
            // A: (K x groups) full-size launches of the fit's own prepare + descriptor kernels into A's row blocks
            for (int g = 0; g < num_groups; ++g) {
                const int W = groups[g].width, H = groups[g].height, cnt = groups[g].count;
                const int32_t* dp = prm->desc_params + 3 * s;
                DescParams p;
                fill_desc_params(p, W, H, L, false, prm->hog_variant, dp[0], dp[1], dp[2], 2 * half[s]);
                p.image_stride = (int64_t)W * H;
                const int64_t nitems = (int64_t)cnt * L;
                const int grid = descriptor_grid(ctx, p, nitems);
                for (int k = 0; k < K; ++k) {
                    const size_t r0 = (size_t)k * nimg + first[g];
                    int32_t* org = sc.origin.as<int32_t>() + 4 * r0 * L;
                    hipLaunchKernelGGL(k_sdm_prepare, dim3((cnt * L + 255) / 256), dim3(256), 0, st, sc.shapes.as<float>() + r0 * N, cnt, L, W, H, 0, half[s],
                                       SDM_IMG, 1.0, org, sc.dist.as<float>() + r0, sc.status.as<int32_t>() + r0);
                    launch_descriptors(dim3(grid), st, dimg[g], org, p, nitems, sc.A.as<float>() + r0 * d.lda, (int64_t)d.lda);
                }
            }
            hipLaunchKernelGGL(k_st_ones, dim3((M + 255) / 256), dim3(256), 0, st, sc.A.as<float>(), d.lda, F, M);
            hipLaunchKernelGGL(k_st_delta, dim3((M * N + 255) / 256), dim3(256), 0, st, sc.gt.as<float>(), sc.shapes.as<float>(), M, N, sc.Bm.as<float>(), d.ldb);
            // R: rows [0, F) of sc.R, the bias row apart in row lda; rows [F, lda) stay zero, so that k_sdm_regress over all lda columns
            // of A (the ones column and the padding meet zero rows) adds exactly the terms fd_sdm_optimize_batch adds, in its order
            st_solve(ctx, sc, st, d, prm->regularisation == FD_SDM_REG_AUTOMATIC, prm->lambda, prm->regularise_affine, sc.R.as<float>(), F, d.lda, [] {});
            const int nchunks = (d.lda + RG_KCHUNK - 1) / RG_KCHUNK;
            hipLaunchKernelGGL(k_sdm_regress, dim3((M + 15) / 16, ((N + 15) / 16 + RG_NT - 1) / RG_NT, nchunks), dim3(64), 0, st, sc.A.as<float>(), M, d.lda,
                               sc.R.as<float>(), N, sc.partial.as<double>(), nchunks);
            hipLaunchKernelGGL(k_sdm_update, dim3((M * N + 255) / 256), dim3(256), 0, st, sc.shapes.as<float>(), sc.partial.as<double>(), nchunks,
                               sc.R.as<float>() + (size_t)d.lda * N, sc.dist.as<float>(), M, N);
            hipLaunchKernelGGL(k_st_err, dim3(1), dim3(1024), 0, st, sc.gt.as<float>(), sc.shapes.as<float>(), (int64_t)M * N, sc.errs.as<double>());
            st_mark(sc, 6, st);
            HIP_CHECK(hipGetLastError());
            // the step's one wait: flag, lambda, errors (and what the caller asked to see)
            int32_t flag[2] = {0, 0};
            double scal[2] = {0, 0};
            Rh[s].resize((size_t)D * N);
            HIP_CHECK(hipMemcpyAsync(flag, sc.flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(scal, sc.scal.p, sizeof(scal), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(errs, sc.errs.p, sizeof(errs), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(hstatus.data(), sc.status.p, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(Rh[s].data(), sc.R.p, sizeof(float) * (size_t)F * N, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(Rh[s].data() + (size_t)F * N, sc.R.as<float>() + (size_t)d.lda * N, sizeof(float) * N, hipMemcpyDeviceToHost, st));
            if (shapes_steps_out) HIP_CHECK(hipMemcpyAsync(hx.data(), sc.shapes.p, sizeof(float) * hx.size(), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            sc.timed = sc.timing;
            bool bad = false;
            for (int r = 0; r < M; ++r) bad = bad || hstatus[r] != 0;
            if (row_status_out)
                for (int i = 0; i < nimg; ++i)
                    for (int k = 0; k < K; ++k) row_status_out[(size_t)i * K + k] = hstatus[(size_t)k * nimg + i];
            if (bad)
                FD_THROW(FD_ERR_RUNTIME, "fd_sdm_train: step %d: a patch window leaves the zero-extended image (cv::Mat roi assertion in the reference); "
                                         "see row_status_out", s);
            if (info_out) { info_out[s + 1].lambda = scal[0]; info_out[s + 1].pivot_flag = flag[0] ? flag[1] + 1 : 0; }
            if (flag[0]) st_throw_pivot(flag[1]);
            info[s + 1] = fd_sdm_train_step_info{scal[0], errs[0], errs[1], M, D, 0};
            if (shapes_steps_out) to_caller(hx.data(), shapes_steps_out + (size_t)(s + 1) * M * N);
        }
        for (int s = 0; s < S; ++s) std::memcpy(R_out[s], Rh[s].data(), sizeof(float) * Rh[s].size());
        if (info_out)
            for (int s = 0; s <= S; ++s) info_out[s] = info[s];
    });
}

}  // extern "C"
