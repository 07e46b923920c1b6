// featuredetection_amd/csrc/liblinear.hip -- liblinear's primal L2-regularised L2-loss SVC (L2R_L2LOSS_SVC) trained with the
// trust-region Newton method TRON on the device.  What liblinear::LibLinearClassifier::train needs of
// liblinear (LibLinearClassifier.cpp:96-148; linear.cpp l2r_l2_svc_fun :191-340, train_one :2181-2230; tron.cpp TRON::tron :56-158,
// trcg :160-221; LibLinearUtils.cpp:70-105).
//
//   f(w) = 1/2 w.w + sum_i C_i max(0, 1 - y_i w.x_i)^2        y_i = +1 for i < n_pos, else -1;  C_i = C weight_pos / C weight_neg
//
// Everything is double; x stays float in memory and is widened on load; with bias the row has one more feature of value 1 that is
// never stored.  The state of a problem (LlState and seven vectors of m = d + bias doubles) lives in device memory.
//
//   ll_pass    a workgroup owns the rows [slab * slab_rows, ...) and reads each once from memory; what it does follows from the phase:
//                fun   z_i = y_i (x_i . v) stored; the slab's sum of C_i (1 - z_i)^2 over 1 - z_i > 0
//                grad  the active flag z_i < 1 stored; the slab's sum of C_i y_i (z_i - 1) x_i over the active rows, and their number
//                Hv    over the active rows t_i = C_i (x_i . v), then the slab's sum of t_i x_i (subXv, the scale and subXTv in one
//                      visit of the slab: the second sweep over its rows is served by the cache)
//              into part[slab][m], fpart[slab], npart[slab]
//   ll_step    one workgroup: sums the slabs' partials in ascending slab order and advances TRON's scalar state machine as tron.cpp
//              orders it; writes the vector the next pass needs, the next phase and the done word
//   k_ll_pass, k_ll_step     the two bodies as kernels of the multi-workgroup form: a phase boundary is a kernel boundary, the
//              host enqueues (pass, step) pairs in budgets and reads the done word once per budget; launches behind done return
//   k_ll_tron_small          one workgroup per problem loops over the two bodies with barriers (one slab of all rows), budgeted
//              per launch: tracker-sized problems and batches
//
// The order of every sum is fixed by (n, d, bias) and the form:
//   row dot     lane l of a wavefront adds the products k = l, l + 64, ... ascending; the 64 lanes are folded by xor 32, 16, .. 1;
//               the bias term v[d] is added last
//   block sum   (ll_block_sum) thread t adds its elements t, t + T, ... ascending; lanes folded as above; wavefronts ascending
//   column sum  of a slab: its active rows are listed ascending; thread (group q, column k) adds the listed rows q, q + G, ...
//               in list order, the G = T / min(T, ceil64(m)) groups are added ascending
//   slabs       ascending
// so that two calls give the same bits, whichever device memory x lives in and however the launches are budgeted.
//
// Where this leaves liblinear: sums in the order above, not sequential; a cap on the total of CG steps (trcg has none); a
// non-finite z_i makes f NaN, and a non-finite f or |g| ends the run (liblinear drops such a row from every sum and can loop for
// ever on a NaN, each comparison being false).
#include "fd_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr int LL_PASS_THREADS = 1024;   // k_ll_pass
constexpr int LL_STEP_THREADS = 1024;   // k_ll_step and k_ll_tron_small
constexpr int LL_SLAB_QUANTUM = 64;     // slab_rows is a multiple of it in the multi-workgroup form
constexpr int LL_MAX_SLABS = 512;       // two workgroups per compute unit; 512 (d + bias) doubles for the step to sum
constexpr int64_t LL_SMALL_MAX_ELEMS = 40960;   // n (d + bias) up to which one workgroup beats two launches per phase (measured)
constexpr int LL_RED_SLOTS = 48;        // three sums by sixteen wavefronts
constexpr int LL_DEFAULT_LAUNCH_STEPS = 32, LL_DEFAULT_LAUNCH_STEPS_SMALL = 512;

enum { LL_PH_FUN0 = 0, LL_PH_GRAD0, LL_PH_HV, LL_PH_FUN, LL_PH_GRAD };
enum { LL_MODE_TRAIN = 0, LL_MODE_OBJECTIVE };

struct LlState {
    int32_t phase, done, mode, has_s;
    int32_t iter;                 // tron's iter: 1 + accepted steps
    int32_t cg_iter, boundary;    // of the running trcg
    int32_t cg_total;
    int32_t stop, converged, n_active, trace_len;
    double f, delta, gnorm, gnorm0, gg, rTr, cgtol, gs, prered, actred, snorm;
};

struct LlProb {
    const float* x;               // n x d
    double* z;                    // n
    uint8_t* act;                 // n: the active set of the last grad
    double* part;                 // slabs x m
    double* fpart;                // slabs
    int32_t* npart;               // slabs
    double *w, *w_new, *g, *s, *r, *dv, *Hd;   // m each
    LlState* st;
    int32_t* trace;               // trace_cap triples
    double Cp, Cn, tol;
    int32_t n_pos, n, d, bias, m, slabs, slab_rows, max_iter, max_cg, trace_cap;
};

inline size_t ll_align(size_t v) { return (v + 255) / 256 * 256; }
inline size_t ll_lds_bytes(int slab_rows, int threads) {
    // the sums' slots, c, the column groups' sums; the active rows' list and their number; the flags
    return sizeof(double) * (size_t)(LL_RED_SLOTS + slab_rows + threads) + sizeof(int32_t) * (size_t)(slab_rows + 2) + (size_t)(slab_rows + 7) / 8 * 8;
}

__device__ inline double ll_wave_sum(double v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The sums of N values over the block, in every thread.  Two barriers: the first also orders what the threads wrote to LDS and
// memory before the call against what they read behind it.
template <int N>
__device__ inline void ll_block_sum(double (&v)[N], double* red) {
    const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = ll_wave_sum(v[q]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < N; ++q) red[q * 16 + wave] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double a = red[q * 16];
        for (int u = 1; u < waves; ++u) a += red[q * 16 + u];
        v[q] = a;
    }
}

// tron.cpp's min and max
__device__ inline double ll_min(double x, double y) { return x < y ? x : y; }
__device__ inline double ll_max(double x, double y) { return x > y ? x : y; }

// x_i . v: lane l adds the products k = l, l + 64, ... ascending into one sum -- the loads of eight products are issued together,
// the additions keep their order -- then the lanes are folded; the bias term comes last
__device__ inline double ll_row_dot(const float* __restrict__ xi, const double* v, int d, int bias, int lane) {
    double a = 0.0;
    int k = lane;
    for (; k + 7 * 64 < d; k += 8 * 64) {
        float xv[8];
        double vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            xv[u] = xi[k + 64 * u];
            vv[u] = v[k + 64 * u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) a += vv[u] * (double)xv[u];
    }
    for (; k < d; k += 64) a += v[k] * (double)xi[k];
    a = ll_wave_sum(a);
    if (bias) a += v[d];
    return a;
}

// sum over the listed rows j = first, first + stride, ... of c_j x_j[k] (the bias column: of c_j), one sum in list order, the
// loads of eight rows issued together
__device__ inline double ll_column_sum(const float* __restrict__ xs, const double* c, const int32_t* idx, int cnt, int first, int stride, int d,
                                       int k) {
    double a = 0.0;
    int j = first;
    if (k >= d) {
        for (; j < cnt; j += stride) a += c[j];
        return a;
    }
    for (; j + 7 * stride < cnt; j += 8 * stride) {
        float xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = xs[(size_t)idx[j + u * stride] * d + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += c[j + u * stride] * (double)xv[u];
    }
    for (; j < cnt; j += stride) a += c[j] * (double)xs[(size_t)idx[j] * d + k];
    return a;
}

__device__ void ll_pass(const LlProb& P, int phase, int slab, double* lds) {
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    double* red = lds;
    double* c = lds + LL_RED_SLOTS;             // per row (fun) or per listed row (grad, Hv)
    double* comb = c + P.slab_rows;
    int32_t* idx = (int32_t*)(comb + T);        // the slab's active rows, ascending
    int32_t* cntSlot = idx + P.slab_rows;
    uint8_t* flag = (uint8_t*)(cntSlot + 2);
    const int r0 = slab * P.slab_rows, rows = min(P.slab_rows, P.n - r0);
    const int d = P.d, m = P.m;
    const float* xs = P.x + (size_t)r0 * d;
    if (phase == LL_PH_FUN0 || phase == LL_PH_FUN) {
        const double* v = phase == LL_PH_FUN0 ? P.w : P.w_new;
        for (int q = wave; q < rows; q += waves) {   // one wavefront per row
            const int i = r0 + q;
            const double a = ll_row_dot(xs + (size_t)q * d, v, d, P.bias, lane);
            if (lane == 0) {
                const double Ci = i < P.n_pos ? P.Cp : P.Cn;
                const double z = (i < P.n_pos ? 1.0 : -1.0) * a;
                P.z[i] = z;
                const double dd = 1.0 - z;
                c[q] = dd > 0 ? Ci * dd * dd : (dd - dd == 0.0 ? 0.0 : dd - dd);   // NaN for a z that is not finite
            }
        }
        __syncthreads();
        double a[1] = {0.0};
        for (int q = tid; q < rows; q += T) a[0] += c[q];
        ll_block_sum(a, red);
        if (tid == 0) P.fpart[slab] = a[0];
        return;
    }
    // grad: the active set follows from z and is stored; Hv: it is the stored one.  Listed in ascending row order by the first
    // wavefront, 64 rows at a time.
    const bool hv = phase == LL_PH_HV;
    for (int q = tid; q < rows; q += T) {
        const bool on = hv ? P.act[r0 + q] != 0 : P.z[r0 + q] < 1;
        if (!hv) P.act[r0 + q] = on;
        flag[q] = on;
    }
    __syncthreads();
    if (wave == 0) {
        int cnt = 0;
        for (int q0 = 0; q0 < rows; q0 += 64) {
            const bool on = q0 + lane < rows && flag[q0 + lane];
            const unsigned long long mask = __ballot(on);
            if (on) idx[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = q0 + lane;
            cnt += __popcll(mask);
        }
        if (lane == 0) {
            cntSlot[0] = cnt;
            if (!hv) P.npart[slab] = cnt;
        }
    }
    __syncthreads();
    const int cnt = cntSlot[0];
    if (hv) {
        for (int j = wave; j < cnt; j += waves) {   // t_j = C_i (x_i . v), one wavefront per active row
            const int q = idx[j], i = r0 + q;
            const double a = ll_row_dot(xs + (size_t)q * d, P.dv, d, P.bias, lane);
            if (lane == 0) c[j] = (i < P.n_pos ? P.Cp : P.Cn) * a;
        }
    } else {
        for (int j = tid; j < cnt; j += T) {
            const int i = r0 + idx[j];
            const double Ci = i < P.n_pos ? P.Cp : P.Cn, yi = i < P.n_pos ? 1.0 : -1.0;
            c[j] = Ci * yi * (P.z[i] - 1);
        }
    }
    __syncthreads();
    // the slab's sum over the active rows of c_j x_j; the bias column is 1
    const int cp = min(T, (m + 63) / 64 * 64), G = T / cp;
    double* out = P.part + (size_t)slab * m;
    if (G <= 1) {
        for (int k = tid; k < m; k += T) out[k] = ll_column_sum(xs, c, idx, cnt, 0, 1, d, k);
    } else {
        const int grp = tid / cp, k = tid - grp * cp;
        comb[tid] = grp < G && k < m ? ll_column_sum(xs, c, idx, cnt, grp, G, d, k) : 0.0;
        __syncthreads();
        if (tid < m) {
            double t = comb[tid];
            for (int u = 1; u < G; ++u) t += comb[u * cp + tid];
            out[tid] = t;
        }
    }
}

__device__ inline void ll_stop(LlState& S, int why) {
    S.done = 1;
    S.stop = why;
    S.converged = why == FD_LL_STOP_GRADIENT ? 1 : 0;
}

// trcg's set-up and the head of its loop (tron.cpp:169-183) for the current g: s = 0, r = d = -g.  Returns whether a CG step
// follows; otherwise the run has stopped (the CG cap) or trcg ends at once (r within cgtol: a zero gradient only).
__device__ inline bool ll_trcg_start(const LlProb& P, LlState& S) {
    const int T = blockDim.x, m = P.m;
    for (int k = threadIdx.x; k < m; k += T) {
        const double rk = -P.g[k];
        P.s[k] = 0.0;
        P.r[k] = rk;
        P.dv[k] = rk;
    }
    S.cgtol = 0.1 * sqrt(S.gg);
    S.cg_iter = 0;
    S.boundary = 0;
    S.rTr = S.gg;   // (-g_k)(-g_k) summed as g.g was
    if (sqrt(S.rTr) <= S.cgtol) return false;
    if (S.cg_total >= P.max_cg) {
        ll_stop(S, FD_LL_STOP_CG_CAP);
        return false;
    }
    S.phase = LL_PH_HV;
    return true;
}

// behind trcg (tron.cpp:92-96): w_new = w + s, gs, prered, and |s| for the step bound
__device__ inline void ll_trcg_end(const LlProb& P, LlState& S, double* red) {
    const int T = blockDim.x, m = P.m;
    double a[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < m; k += T) {
        const double sk = P.s[k];
        P.w_new[k] = P.w[k] + sk;
        a[0] += P.g[k] * sk;
        a[1] += sk * P.r[k];
        a[2] += sk * sk;
    }
    ll_block_sum(a, red);
    S.gs = a[0];
    S.prered = -0.5 * (a[0] - a[1]);
    S.snorm = sqrt(a[2]);
    S.phase = LL_PH_FUN;
}

// the foot of tron's loop behind the accept test (tron.cpp:136-151) and its head (:88): the warnings, max_iter, the next trcg
__device__ inline void ll_next_iteration(const LlProb& P, LlState& S, double* red) {
    if (S.f < -1.0e+32) {
        ll_stop(S, FD_LL_STOP_NONFINITE);   // tron's first warning; f >= 0 here
    } else if (fabs(S.actred) <= 0 && S.prered <= 0) {
        ll_stop(S, FD_LL_STOP_ACTRED_ZERO);
    } else if (fabs(S.actred) <= 1.0e-12 * fabs(S.f) && fabs(S.prered) <= 1.0e-12 * fabs(S.f)) {
        ll_stop(S, FD_LL_STOP_ACTRED_SMALL);
    } else if (S.iter > P.max_iter) {
        ll_stop(S, FD_LL_STOP_MAX_ITER);
    } else if (!ll_trcg_start(P, S) && !S.done) {
        ll_trcg_end(P, S, red);
    }
}

__device__ void ll_step(const LlProb& P, double* lds) {
    const int T = blockDim.x, tid = threadIdx.x, m = P.m;
    double* red = lds;
    LlState S = *P.st;   // every thread advances its copy alike; thread 0 stores it
    if (S.done) return;
    const bool train = S.mode == LL_MODE_TRAIN;
    const double eta0 = 1e-4, eta1 = 0.25, eta2 = 0.75, sigma1 = 0.25, sigma2 = 0.5, sigma3 = 4;
    if (S.phase == LL_PH_FUN0 || S.phase == LL_PH_FUN) {
        const double* v = S.phase == LL_PH_FUN0 ? P.w : P.w_new;
        double a[2] = {0.0, 0.0};
        for (int k = tid; k < m; k += T) a[0] += v[k] * v[k];
        for (int u = tid; u < P.slabs; u += T) a[1] += P.fpart[u];
        ll_block_sum(a, red);
        const double fval = a[0] / 2.0 + a[1];
        if (train && !isfinite(fval)) {
            if (S.phase == LL_PH_FUN0) S.f = fval;
            ll_stop(S, FD_LL_STOP_NONFINITE);
        } else if (S.phase == LL_PH_FUN0) {
            S.f = fval;
            S.phase = LL_PH_GRAD0;
        } else {
            const double fnew = fval;
            const double actred = S.f - fnew;
            if (S.iter == 1) S.delta = ll_min(S.delta, S.snorm);
            const double curv = fnew - S.f - S.gs;
            const double alpha = curv <= 0 ? sigma3 : ll_max(sigma1, -0.5 * (S.gs / curv));
            if (actred < eta0 * S.prered) S.delta = ll_min(ll_max(alpha, sigma1) * S.snorm, sigma2 * S.delta);
            else if (actred < eta1 * S.prered) S.delta = ll_max(sigma1 * S.delta, ll_min(alpha * S.snorm, sigma2 * S.delta));
            else if (actred < eta2 * S.prered) S.delta = ll_max(sigma1 * S.delta, ll_min(alpha * S.snorm, sigma3 * S.delta));
            else S.delta = ll_max(S.delta, ll_min(alpha * S.snorm, sigma3 * S.delta));
            const bool accepted = actred > eta0 * S.prered;
            if (tid == 0 && S.trace_len < P.trace_cap) {
                P.trace[3 * S.trace_len] = S.cg_iter;
                P.trace[3 * S.trace_len + 1] = S.boundary;
                P.trace[3 * S.trace_len + 2] = accepted ? 1 : 0;
            }
            ++S.trace_len;
            S.actred = actred;
            if (accepted) {
                ++S.iter;
                for (int k = tid; k < m; k += T) P.w[k] = P.w_new[k];
                S.f = fnew;
                S.phase = LL_PH_GRAD;   // the foot of the loop follows the gradient
            } else {
                ll_next_iteration(P, S, red);
            }
        }
    } else if (S.phase == LL_PH_GRAD0 || S.phase == LL_PH_GRAD) {
        double a[2] = {0.0, 0.0};
        for (int k = tid; k < m; k += T) {
            double t = P.part[k];
            for (int u = 1; u < P.slabs; ++u) t += P.part[(size_t)u * m + k];
            const double gk = P.w[k] + 2 * t;
            P.g[k] = gk;
            a[0] += gk * gk;
        }
        for (int u = tid; u < P.slabs; u += T) a[1] += (double)P.npart[u];
        ll_block_sum(a, red);
        S.gg = a[0];
        S.gnorm = sqrt(a[0]);
        S.n_active = (int32_t)a[1];
        if (S.phase == LL_PH_GRAD0) {
            S.delta = S.gnorm;
            S.gnorm0 = S.gnorm;
        }
        if (!train) {
            if (S.has_s) S.phase = LL_PH_HV;   // the host put s into dv
            else S.done = 1;
        } else if (!isfinite(S.gnorm)) {
            ll_stop(S, FD_LL_STOP_NONFINITE);
        } else if (S.gnorm <= P.tol * S.gnorm0) {
            ll_stop(S, FD_LL_STOP_GRADIENT);
        } else if (S.phase == LL_PH_GRAD0) {
            if (!ll_trcg_start(P, S) && !S.done) ll_trcg_end(P, S, red);
        } else {
            ll_next_iteration(P, S, red);
        }
    } else {   // LL_PH_HV: one step of trcg's loop (tron.cpp:183-214)
        double a[3] = {0.0, 0.0, 0.0};
        for (int k = tid; k < m; k += T) {
            double t = P.part[k];
            for (int u = 1; u < P.slabs; ++u) t += P.part[(size_t)u * m + k];
            const double dk = P.dv[k], hk = dk + 2 * t;
            P.Hd[k] = hk;
            a[0] += dk * hk;
        }
        if (!train) {
            S.done = 1;
        } else {
            ll_block_sum(a, red);
            ++S.cg_iter;
            ++S.cg_total;
            double alpha = S.rTr / a[0];
            a[0] = 0.0;
            for (int k = tid; k < m; k += T) {
                const double sk = P.s[k] + alpha * P.dv[k];
                P.s[k] = sk;
                a[0] += sk * sk;
            }
            ll_block_sum(a, red);
            bool ended = false;
            if (sqrt(a[0]) > S.delta) {   // cg reaches the trust region boundary
                alpha = -alpha;
                a[0] = a[1] = a[2] = 0.0;
                for (int k = tid; k < m; k += T) {
                    const double dk = P.dv[k], sk = P.s[k] + alpha * dk;
                    P.s[k] = sk;
                    a[0] += sk * dk;
                    a[1] += sk * sk;
                    a[2] += dk * dk;
                }
                ll_block_sum(a, red);
                const double std_ = a[0], sts = a[1], dtd = a[2];
                const double dsq = S.delta * S.delta;
                const double rad = sqrt(std_ * std_ + dtd * (dsq - sts));
                if (std_ >= 0) alpha = (dsq - sts) / (std_ + rad);
                else alpha = (rad - std_) / dtd;
                const double nalpha = -alpha;
                for (int k = tid; k < m; k += T) {
                    P.s[k] = P.s[k] + alpha * P.dv[k];
                    P.r[k] = P.r[k] + nalpha * P.Hd[k];
                }
                S.boundary = 1;
                ended = true;
            } else {
                alpha = -alpha;
                a[0] = 0.0;
                for (int k = tid; k < m; k += T) {
                    const double rk = P.r[k] + alpha * P.Hd[k];
                    P.r[k] = rk;
                    a[0] += rk * rk;
                }
                ll_block_sum(a, red);
                const double rnew = a[0], beta = rnew / S.rTr;
                for (int k = tid; k < m; k += T) {
                    const double dk = P.dv[k] * beta;
                    P.dv[k] = dk + P.r[k];
                }
                S.rTr = rnew;
                if (sqrt(rnew) <= S.cgtol) ended = true;
                else if (S.cg_total >= P.max_cg) ll_stop(S, FD_LL_STOP_CG_CAP);
            }
            if (ended) ll_trcg_end(P, S, red);
        }
    }
    __syncthreads();   // every thread has its copy of the state
    if (tid == 0) *P.st = S;
}

extern __shared__ double ll_lds[];

__global__ __launch_bounds__(LL_PASS_THREADS) void k_ll_pass(const LlProb* __restrict__ probs) {
    const LlProb P = probs[0];
    if (P.st->done) return;
    ll_pass(P, P.st->phase, blockIdx.x, ll_lds);
}

__global__ __launch_bounds__(LL_STEP_THREADS) void k_ll_step(const LlProb* __restrict__ probs) {
    const LlProb P = probs[0];
    ll_step(P, ll_lds);
}

// One workgroup per problem, one slab of all its rows: up to `budget` (pass, step) pairs, a barrier where the multi-workgroup
// form has a kernel boundary.
__global__ __launch_bounds__(LL_STEP_THREADS) void k_ll_tron_small(const LlProb* __restrict__ probs, int budget) {
    const LlProb P = probs[blockIdx.x];
    for (int b = 0; b < budget; ++b) {
        if (P.st->done) break;
        ll_pass(P, P.st->phase, 0, ll_lds);
        __syncthreads();
        ll_step(P, ll_lds);
        __syncthreads();
    }
}

// ---- host ----

struct LlGeom {
    int single, slab_rows, slabs;
    size_t lds, scratch;
};

int ll_small_rows() {
    const char* e = std::getenv("FD_LIBLINEAR_SMALL_ROWS");
    if (!e || !*e) return FD_LIBLINEAR_SMALL_MAX_N;
    return (int)std::min<long>(std::max<long>(std::strtol(e, nullptr, 10), 0), FD_LIBLINEAR_SMALL_MAX_N);
}

// the aligned sizes of a problem's buffers in the order they lie in the scratch: the state, the seven vectors and the trace are
// cleared before a run
enum { LZ_STATE, LZ_VEC, LZ_TRACE, LZ_Z, LZ_ACT, LZ_FPART, LZ_NPART, LZ_PART, LZ_COUNT };
struct LlSizes {
    size_t b[LZ_COUNT] = {};
    size_t total() const {
        size_t t = 0;
        for (size_t v : b) t += v;
        return t;
    }
};
LlSizes ll_sizes(int n, int m, int slabs, int trace_cap) {
    LlSizes z;
    z.b[LZ_STATE] = ll_align(sizeof(LlState));
    z.b[LZ_VEC] = ll_align(sizeof(double) * 7 * (size_t)m);
    z.b[LZ_TRACE] = ll_align(sizeof(int32_t) * 3 * (size_t)trace_cap);
    z.b[LZ_Z] = ll_align(sizeof(double) * (size_t)n);
    z.b[LZ_ACT] = ll_align((size_t)n);
    z.b[LZ_FPART] = ll_align(sizeof(double) * (size_t)slabs);
    z.b[LZ_NPART] = ll_align(sizeof(int32_t) * (size_t)slabs);
    z.b[LZ_PART] = ll_align(sizeof(double) * (size_t)slabs * m);
    return z;
}

// batch: a problem of fd_liblinear_train_batch, which takes the single-workgroup form whatever its feature length
LlGeom ll_geom(int n, int m, bool batch) {
    LlGeom g = {};
    g.single = batch || (n <= ll_small_rows() && (int64_t)n * m <= LL_SMALL_MAX_ELEMS) ? 1 : 0;
    if (g.single) {
        g.slab_rows = n;
        g.slabs = 1;
        g.lds = ll_lds_bytes(n, LL_STEP_THREADS);
    } else {
        const int q = (n + LL_SLAB_QUANTUM * LL_MAX_SLABS - 1) / (LL_SLAB_QUANTUM * LL_MAX_SLABS);
        g.slab_rows = LL_SLAB_QUANTUM * q;
        g.slabs = (n + g.slab_rows - 1) / g.slab_rows;
        g.lds = ll_lds_bytes(g.slab_rows, LL_STEP_THREADS);   // the step's; the pass needs less
    }
    g.scratch = ll_sizes(n, m, g.slabs, 0).total();
    return g;
}

int ll_shape_fault(int n_pos, int n_neg, int d, int bias) {
    if (n_pos < 1 || n_neg < 1) return 1;
    if ((int64_t)n_pos + n_neg > FD_LIBLINEAR_MAX_N) return 2;
    if (d < 1) return 3;
    if (bias != 0 && bias != 1) return 4;
    return (int64_t)d + bias > FD_LIBLINEAR_MAX_D ? 5 : 0;
}

void ll_check_shape(const char* who, int n_pos, int n_neg, int d, int bias) {
    const int fault = ll_shape_fault(n_pos, n_neg, d, bias);
    if (fault == 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: needs at least one positive and one negative example (%d, %d)", who, n_pos, n_neg);
    if (fault == 2) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %lld examples, at most %d", who, (long long)n_pos + n_neg, FD_LIBLINEAR_MAX_N);
    if (fault == 3) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the feature length must be positive (%d)", who, d);
    if (fault == 4) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bias must be 0 or 1 (%d)", who, bias);
    if (fault == 5) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %d features with the bias term, at most %d", who, d + bias, FD_LIBLINEAR_MAX_D);
}

fd_liblinear_params ll_checked_params(const char* who, const fd_liblinear_params* prm) {
    if (!prm) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
    fd_liblinear_params p = *prm;
    if (!(p.C > 0.0) || !(p.weight_pos > 0.0) || !(p.weight_neg > 0.0))
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: C and the class weights must be positive (%g, %g, %g)", who, p.C, p.weight_pos, p.weight_neg);
    if (!(p.eps >= 0.0)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: eps must not be negative (%g)", who, p.eps);
    if (!(p.solver_tol >= 0.0)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: solver_tol must not be negative (%g)", who, p.solver_tol);
    if (p.bias != 0 && p.bias != 1) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: bias must be 0 or 1 (%d)", who, p.bias);
    if (p.max_iterations < 0 || p.max_cg_steps < 0 || p.launch_steps < 0)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: max_iterations, max_cg_steps and launch_steps must not be negative", who);
    if (p.eps == 0.0) p.eps = 0.01;
    if (p.max_iterations == 0) p.max_iterations = 1000;
    return p;
}

struct LlScratch {
    DevBuf x, work, desc;
};

struct LlExtra {   // fd_liblinear_objective: the point, the direction, and where the results go
    const double *w, *s;
    double *f, *g, *Hs;
};

// Runs `count` problems to their end and returns what was asked for.  batch: every problem on k_ll_tron_small in one set of
// launches; otherwise count is 1 and the size picks the form.  Leaves ctx->stream synchronised.
void ll_run(fd_ctx* ctx, const char* who, int count, const fd_liblinear_problem* probs, const fd_liblinear_params* params, bool batch,
            int32_t* trace, int trace_cap, fd_liblinear_info* infos, const LlExtra* extra) {
    const fd_liblinear_params prm = ll_checked_params(who, params);
    if (count < 1 || !probs) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument or no problem", who);
    if (trace_cap < 0) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: trace_cap must not be negative (%d)", who, trace_cap);
    if (!trace) trace_cap = 0;
    std::vector<LlGeom> geo(count);
    std::vector<LlSizes> sizes(count);
    size_t xBytes = 0, workBytes = 0, ldsMax = 0;
    for (int c = 0; c < count; ++c) {
        const fd_liblinear_problem& pr = probs[c];
        ll_check_shape(who, pr.n_pos, pr.n_neg, pr.d, prm.bias);
        if (!pr.x) FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
        const int n = pr.n_pos + pr.n_neg, m = pr.d + prm.bias;
        if (batch && n > FD_LIBLINEAR_SMALL_MAX_N)
            FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: %d examples in problem %d, at most %d", who, n, c, FD_LIBLINEAR_SMALL_MAX_N);
        geo[c] = ll_geom(n, m, batch);
        sizes[c] = ll_sizes(n, m, geo[c].slabs, trace_cap);
        if (!pr.is_device) xBytes += ll_align(sizeof(float) * (size_t)n * pr.d);
        workBytes += sizes[c].total();
        ldsMax = std::max(ldsMax, geo[c].lds);
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    LlScratch& sc = fd_scratch<LlScratch>(ctx);
    try {
        sc.x.reserve(xBytes);
        sc.work.reserve(workBytes);
        sc.desc.reserve(sizeof(LlProb) * count);
    } catch (const FdError& e) {
        FD_THROW(FD_ERR_RUNTIME, "%s: no device memory for the training scratch (%zu + %zu bytes): %s", who, xBytes, workBytes, e.msg.c_str());
    }
    // pinned: the descriptors, the states, then per problem w and the trace
    const size_t stateOff = ll_align(sizeof(LlProb) * count);
    size_t outOff = stateOff + ll_align(sizeof(LlState) * count);
    std::vector<size_t> outW(count), outT(count);
    for (int c = 0; c < count; ++c) {
        outW[c] = outOff;
        outOff += ll_align(sizeof(double) * (size_t)(probs[c].d + prm.bias));
        outT[c] = outOff;
        outOff += sizes[c].b[LZ_TRACE];
    }
    char* pinned = (char*)fd_pinned(ctx, outOff);
    LlProb* hd = (LlProb*)pinned;
    LlState* hs = (LlState*)(pinned + stateOff);
    char* xAt = (char*)sc.x.p;
    char* at = (char*)sc.work.p;
    for (int c = 0; c < count; ++c) {
        const fd_liblinear_problem& pr = probs[c];
        const int n = pr.n_pos + pr.n_neg, m = pr.d + prm.bias;
        const LlSizes& z = sizes[c];
        LlProb D = {};
        if (pr.is_device) {
            D.x = pr.x;
        } else {
            const size_t bytes = sizeof(float) * (size_t)n * pr.d;
            HIP_CHECK(hipMemcpyAsync(xAt, pr.x, bytes, hipMemcpyHostToDevice, ctx->stream));
            D.x = (const float*)xAt;
            xAt += ll_align(bytes);
        }
        char* base = at;
        auto take = [&](int k) {
            char* p = at;
            at += z.b[k];
            return p;
        };
        D.st = (LlState*)take(LZ_STATE);
        D.w = (double*)take(LZ_VEC);
        D.w_new = D.w + m;
        D.g = D.w_new + m;
        D.s = D.g + m;
        D.r = D.s + m;
        D.dv = D.r + m;
        D.Hd = D.dv + m;
        D.trace = (int32_t*)take(LZ_TRACE);
        HIP_CHECK(hipMemsetAsync(base, 0, (size_t)(at - base), ctx->stream));
        D.z = (double*)take(LZ_Z);
        D.act = (uint8_t*)take(LZ_ACT);
        D.fpart = (double*)take(LZ_FPART);
        D.npart = (int32_t*)take(LZ_NPART);
        D.part = (double*)take(LZ_PART);
        D.Cp = prm.C * prm.weight_pos;
        D.Cn = prm.C * prm.weight_neg;
        D.tol = prm.solver_tol > 0.0 ? prm.solver_tol : prm.eps * std::max(std::min(pr.n_pos, pr.n_neg), 1) / n;   // train_one
        D.n_pos = pr.n_pos;
        D.n = n;
        D.d = pr.d;
        D.bias = prm.bias;
        D.m = m;
        D.slabs = geo[c].slabs;
        D.slab_rows = geo[c].slab_rows;
        D.max_iter = prm.max_iterations;
        D.max_cg = prm.max_cg_steps > 0 ? prm.max_cg_steps : 100 * m + 1000;
        D.trace_cap = trace_cap;
        hd[c] = D;
        LlState S = {};
        S.phase = LL_PH_FUN0;
        S.iter = 1;
        if (extra) {
            S.mode = LL_MODE_OBJECTIVE;
            S.has_s = extra->s ? 1 : 0;
        }
        hs[c] = S;
        HIP_CHECK(hipMemcpyAsync(D.st, hs + c, sizeof(LlState), hipMemcpyHostToDevice, ctx->stream));
        if (extra) {
            HIP_CHECK(hipMemcpyAsync(D.w, extra->w, sizeof(double) * m, hipMemcpyHostToDevice, ctx->stream));
            if (extra->s) HIP_CHECK(hipMemcpyAsync(D.dv, extra->s, sizeof(double) * m, hipMemcpyHostToDevice, ctx->stream));
        }
    }
    HIP_CHECK(hipMemcpyAsync(sc.desc.p, hd, sizeof(LlProb) * count, hipMemcpyHostToDevice, ctx->stream));
    // the states were staged in the pinned area the read-backs reuse: they have to be on the device first
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const bool single = geo[0].single != 0;
    const int budget = prm.launch_steps > 0 ? prm.launch_steps : single ? LL_DEFAULT_LAUNCH_STEPS_SMALL : LL_DEFAULT_LAUNCH_STEPS;
    const LlProb* dd = sc.desc.as<LlProb>();
    for (;;) {
        if (single) {
            hipLaunchKernelGGL(k_ll_tron_small, dim3(count), dim3(LL_STEP_THREADS), ldsMax, ctx->stream, dd, budget);
            HIP_CHECK(hipGetLastError());
        } else {
            const size_t passLds = ll_lds_bytes(geo[0].slab_rows, LL_PASS_THREADS);
            for (int b = 0; b < budget; ++b) {
                hipLaunchKernelGGL(k_ll_pass, dim3(geo[0].slabs), dim3(LL_PASS_THREADS), passLds, ctx->stream, dd);
                hipLaunchKernelGGL(k_ll_step, dim3(1), dim3(LL_STEP_THREADS), geo[0].lds, ctx->stream, dd);
            }
            HIP_CHECK(hipGetLastError());
        }
        for (int c = 0; c < count; ++c) HIP_CHECK(hipMemcpyAsync(hs + c, hd[c].st, sizeof(LlState), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        bool done = true;
        for (int c = 0; c < count; ++c) done = done && hs[c].done;
        if (done) break;
    }
    if (extra) {
        const LlProb& D = hd[0];
        *extra->f = hs[0].f;
        HIP_CHECK(hipMemcpyAsync(extra->g, D.g, sizeof(double) * D.m, hipMemcpyDeviceToHost, ctx->stream));
        if (extra->s) HIP_CHECK(hipMemcpyAsync(extra->Hs, D.Hd, sizeof(double) * D.m, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return;
    }
    for (int c = 0; c < count; ++c) {
        HIP_CHECK(hipMemcpyAsync(pinned + outW[c], hd[c].w, sizeof(double) * hd[c].m, hipMemcpyDeviceToHost, ctx->stream));
        if (trace_cap) HIP_CHECK(hipMemcpyAsync(pinned + outT[c], hd[c].trace, sizeof(int32_t) * 3 * (size_t)trace_cap, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < count; ++c) {
        const fd_liblinear_problem& pr = probs[c];
        const LlState& S = hs[c];
        const double* w = (const double*)(pinned + outW[c]);
        for (int k = 0; k < pr.d; ++k) pr.weights[k] = (float)w[k];
        if (pr.bias) *pr.bias = prm.bias ? (float)(-w[pr.d]) : 0.f;
        if (pr.w) std::memcpy(pr.w, w, sizeof(double) * hd[c].m);
        if (trace_cap) std::memcpy(trace, pinned + outT[c], sizeof(int32_t) * 3 * (size_t)std::min(S.trace_len, trace_cap));
        if (infos) {
            fd_liblinear_info& o = infos[c];
            o.iterations = S.iter - 1;
            o.cg_steps = S.cg_total;
            o.converged = S.converged;
            o.stop = S.stop;
            o.n_active = S.n_active;
            o.trace_len = S.trace_len;
            o.objective = S.f;
            o.gnorm = S.gnorm;
            o.gnorm0 = S.gnorm0;
            o.delta = S.delta;
        }
    }
}

}  // namespace

extern "C" {

int fd_liblinear_train_limits(int n_pos, int n_neg, int d, int bias, int* single_workgroup, int* slab_rows, int64_t* scratch_bytes, int* lds_bytes) {
    if (ll_shape_fault(n_pos, n_neg, d, bias)) return FD_ERR_INVALID_ARGUMENT;
    const LlGeom g = ll_geom(n_pos + n_neg, d + bias, false);
    if (single_workgroup) *single_workgroup = g.single;
    if (slab_rows) *slab_rows = g.slab_rows;
    if (scratch_bytes) *scratch_bytes = (int64_t)g.scratch;
    if (lds_bytes) *lds_bytes = (int)g.lds;
    return FD_OK;
}

int fd_liblinear_train(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_liblinear_params* params, float* weights,
                       float* bias_out, double* w, int32_t* trace, int trace_cap, fd_liblinear_info* info) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !weights || !bias_out) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_liblinear_train: NULL argument");
        const fd_liblinear_problem pr = {x, n_pos, n_neg, d, is_device, weights, bias_out, w};
        ll_run(ctx, "fd_liblinear_train", 1, &pr, params, false, trace, trace_cap, info, nullptr);
    });
}

int fd_liblinear_train_batch(fd_ctx* ctx, int count, const fd_liblinear_problem* problems, const fd_liblinear_params* params,
                             fd_liblinear_info* infos) {
    return fd_guard(ctx, [&] {
        if (!ctx || !infos) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_liblinear_train_batch: NULL argument");
        if (count > 65535) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_liblinear_train_batch: %d problems, at most 65535", count);
        for (int c = 0; c < count && problems; ++c)
            if (!problems[c].weights || !problems[c].bias) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_liblinear_train_batch: NULL argument in problem %d", c);
        ll_run(ctx, "fd_liblinear_train_batch", count, problems, params, true, nullptr, 0, infos, nullptr);
    });
}

int fd_liblinear_objective(fd_ctx* ctx, const float* x, int n_pos, int n_neg, int d, int is_device, const fd_liblinear_params* params,
                           const double* w, const double* s, double* f, double* g, double* Hs) {
    return fd_guard(ctx, [&] {
        if (!ctx || !x || !w || !f || !g || (s && !Hs)) FD_THROW(FD_ERR_INVALID_ARGUMENT, "fd_liblinear_objective: NULL argument");
        const fd_liblinear_problem pr = {x, n_pos, n_neg, d, is_device, nullptr, nullptr, nullptr};
        const LlExtra extra = {w, s, f, g, Hs};
        ll_run(ctx, "fd_liblinear_objective", 1, &pr, params, false, nullptr, 0, nullptr, &extra);
    });
}

}  // extern "C"
