// featuredetection_amd/csrc/wvm_dense_group.hpp -- the dense pre-filter for a GROUP of detectors that scan the same windows
// (included by wvm.hip only, behind wvm_dense.hpp).
//
// ffpDetectApp.cpp:557-600 runs its detectors one after the other over the same frame; seven of the fifteen *.cfg detectors share one
// pyramid and a 24 x 24 patch, two more the 16 x 24 ear patch, two the 20 x 20 profile-face patch.  HistEq64 (HistEq64Filter.cpp:32-125)
// depends on the window only, so for such a group everything up to the equalised pixels -- histogram slide, cdf, LUT, the LUT gather:
// 86 % of k_wvm_prefilter's instructions -- is the same work done once per detector.  k_wvm_prefilter_group does it ONCE per window:
//   1. / 2. as k_wvm_prefilter (lane == window, private histogram column that slides down, register cdf chain, LUT in LDS), with
//       wvm_dense.hpp's pieces: WvdLaneLds, wvd_hist_clear, WvdWaves, wvd_layer_task, wvd_cdf_lut;
//   3a. the equalised patch of the lane's window is gathered once and kept in REGISTERS as the finished B operands of all k-steps
//       (KS x 8 dwords per lane: 144 for 24 x 24);
//   3b. per detector of the group: the exact digit contraction against that detector's table (the only per-detector memory traffic:
//       its operand fragments, 2 KB per k-step from L2), then wvd_fold and wvd_levels with that detector's constants -- the one
//       copy of the fold and the error-bound arithmetic both kernels call, so a detector's queue holds the same windows;
//   6. survivors per detector (bits in LDS while the lane walks down its column) -> that detector's stage-B queue (wvd_push_survivors).
// Round 2's k_wvm_prefilter_multi shared only the histogram / cdf / LUT (13 % less kernel time) and was dropped; this one shares the gather
// as well, which is what the time goes into.
#pragma once

constexpr int WVD_GMAX = 8;   // detectors per group launch
// patch sizes the group kernel takes: the equalised patch stays in a lane's registers, KS x 8 dwords, up to KS = 18 k-steps
// (24 x 24; the 24 k-steps of 32 x 24 do not fit)
constexpr bool wvd_group_fits(int pw, int ph) { return (pw / 4 * ph + 7) / 8 <= 18; }
#ifndef WVD_GRP_RD
#define WVD_GRP_RD 2
#endif

struct WvdMember {
    const wvd_v4i* B;          // the detector's digit table
    const WvdConst* c;         // its level constants and scalars (WvdConst::sc)
    int64_t* q;                // its stage-B queue
    unsigned int* qcount;
};
struct WvdGroup {
    int32_t n, pad;
    WvdMember m[WVD_GMAX];
};

namespace {

template <int PW_, int PH_>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_wvm_prefilter_group(const uint8_t* __restrict__ arena, WvdTable wt, WvdGroup ga) {
    static_assert(PW_ % 4 == 0 && PW_ >= 16 && PW_ <= 32, "rows are read as dwords");
    constexpr int NW = PW_ / 4;
    constexpr int D4 = NW * PH_;
    static_assert(D4 % 4 == 0, "the equalise blocks take 4 dwords");
    constexpr int KS = (D4 + 7) / 8;
    static_assert(wvd_group_fits(PW_, PH_), "the equalised patch stays in registers: KS x 8 dwords per lane");
    __shared__ __attribute__((aligned(16384))) WvdLds S;
    __shared__ unsigned int survL[4][WVD_GMAX][64];   // bit s of [wave][detector][lane]: the lane's window s goes to that detector's exact cascade
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = wt.K;
    const int ND = ga.n;
    int li = 0;
    const WvdLaneLds ld(S.hist, S.lut, lane, wave);
    const float stretch = ((const wvd_cconst*)(uintptr_t)ga.m[0].c)->sc.stretch;   // 255 / (PW_ PH_): the same for every member

    // Operand fragments (2 x 16 bytes per lane and k-step) are requested RD k-steps ahead of their MFMAs and wrap into the next detector's
    // table: with nothing but MFMAs between the requests an L2 round trip is ~4 k-steps of one wavefront; the SIMD's second wavefront
    // covers part of it.  (The equalised patch + the accumulators are 208 of the 256 registers two wavefronts per SIMD leave.)
    constexpr int RD = KS <= 13 ? 4 : WVD_GRP_RD;   // (16 x 24 and 20 x 20 patches have the registers for four k-steps: 396 against 415, 106 against 113 us per 1080p frame)
    static_assert(RD == 1 || RD == 2 || RD == 4, "the digit tables are padded with zero k-steps to a multiple of four");
    constexpr int KSR = (KS + RD - 1) / RD * RD;   // k-steps contracted per detector: whole rounds of the ring (the pad steps add 0 x anything)
    wvd_v4i frag[RD][2];
    unsigned int lane16 = (unsigned int)lane * 16u;
    asm volatile("" : "+v"(lane16));
    auto loadFrag = [&](const wvd_v4i* B, int ks, int mt) {
        return *reinterpret_cast<const wvd_v4i*>(reinterpret_cast<const char*>(B) + (size_t)(ks * 2 + mt) * 1024 + lane16);
    };
#pragma unroll
    for (int ks = 0; ks < RD; ++ks) { frag[ks][0] = loadFrag(ga.m[0].B, ks, 0); frag[ks][1] = loadFrag(ga.m[0].B, ks, 1); }

    int lastImg = -1;
    const WvdWaves W(wt, wave);
    for (int v = W.first; v < W.end; v += W.stride) {
        int img, tile;
        W.locate(wt, v, img, tile);
        if (img != lastImg) { li = 0; lastImg = img; }
        while (li + 1 < wt.n && tile >= wt.l[li + 1].sTileFirst) ++li;   // tiles ascend per wavefront inside a frame
        const WvdLayer& wl = wt.l[li];
        unsigned int ix;
        int iy0, rows;
        wvd_layer_task(tile, lane, wl, K, ix, iy0, rows);
        const int lw = wl.lw;
        const unsigned int rowStep = (unsigned int)(wt.sy * lw);
        const uint8_t* ubase = arena + (size_t)img * wt.imageStride + wl.off;
        const unsigned int lo0 = (unsigned int)((wl.by + iy0 * wt.sy) * lw + (wl.bx + (int)ix * wt.sx));
        const int64_t wid0 = (int64_t)img * wt.perImage + wl.first + (int64_t)iy0 * wl.nx + ix;

        // ---- 1. histogram of the lane's first window
        wvd_hist_clear(ld.histPtr, lane);
#pragma unroll
        for (int d = 0; d < WVD_GMAX; ++d) survL[wave][d][lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        {
            unsigned int wn[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) wn[j] = wvd_load_u32(ubase + 4 * j, lo0);
#pragma unroll 2
            for (int r = 0; r < PH_; ++r) {
                unsigned int w4[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) w4[j] = wn[j];
                const uint8_t* nsrc = ubase + (size_t)(r + 1 < PH_ ? r + 1 : r) * lw;
#pragma unroll
                for (int j = 0; j < NW; ++j) wn[j] = wvd_load_u32(nsrc + 4 * j, lo0);
                wvd_hist_row<NW, true>(w4, ld.blkH4, ld.laneOff32, ld.inc);
            }
        }
#pragma unroll 1
        for (int step = 0; step < K; ++step) {
            const bool active = step < rows;
            if (__ballot(active) == 0) break;
            if (step > 0 && active) {   // ---- 1'. slide the histogram down by one window
                const uint8_t* out0 = ubase + (size_t)(step - 1) * rowStep;
                for (int q = 0; q < wt.sy; ++q) {
                    unsigned int wo[NW], wi[NW];
#pragma unroll
                    for (int j = 0; j < NW; ++j) { wo[j] = wvd_load_u32(out0 + (size_t)q * lw + 4 * j, lo0); wi[j] = wvd_load_u32(out0 + (size_t)(q + PH_) * lw + 4 * j, lo0); }
                    wvd_hist_row<NW, false>(wo, ld.blkH4, ld.laneOff32, ld.inc);
                    wvd_hist_row<NW, true>(wi, ld.blkH4, ld.laneOff32, ld.inc);
                }
            }
            const unsigned int lo = lo0 + (unsigned int)(active ? step : (rows > 0 ? rows - 1 : 0)) * rowStep;
            wave_sync();
            // ---- 2. cdf, LUT, exact integer sums of the equalised patch
            unsigned int sumx, sumxx;
            wvd_cdf_lut<PW_ * PH_>(ld.cntLds, ld.lutLds, stretch, sumx, sumxx);
            wave_sync();
            // ---- 3a. the equalised patch as the B operands of all k-steps (k_wvm_prefilter builds them k-step by k-step in front of its
            //          MFMAs; here they stay: every detector of the group contracts the same pixels)
            unsigned int pkAll[KS][8];
            {
                unsigned int nxq[8];
                auto fetchPx = [&](int ks) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int q = 8 * ks + j;
                        if (q < D4) nxq[j] = wvd_load_u32(ubase + (size_t)(q / NW) * lw + 4 * (q % NW), lo);
                    }
                };
                fetchPx(0);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    unsigned int cur[8], pk[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) cur[j] = nxq[j];
                    if (ks + 1 < KS) fetchPx(ks + 1);
                    wvd_equalise<4>(cur, pk, ld.lutWord, ld.blkL4);
                    if (8 * ks + 4 < D4) wvd_equalise<4>(cur + 4, pk + 4, ld.lutWord, ld.blkL4);
                    else pk[4] = pk[5] = pk[6] = pk[7] = 0;
                    wvd_swap32(pk[0], pk[4]); wvd_swap32(pk[1], pk[5]); wvd_swap32(pk[2], pk[6]); wvd_swap32(pk[3], pk[7]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) pkAll[ks][j] = pk[j];
                }
            }
            // ---- 3b. per detector: contraction, fold, levels
#pragma unroll 1
            for (int d = 0; d < ND; ++d) {
                const WvdMember mb = ga.m[d];
                const wvd_v4i* Bnext = ga.m[d + 1 < ND ? d + 1 : 0].B;
                const wvd_cconst& C = *(const wvd_cconst*)(uintptr_t)mb.c;
                const WvdScal sc = {C.sc.L, C.sc.negBasis, C.sc.negBias, 0.f, C.sc.sxxSlack, 0, C.sc.scale, C.sc.nb2, C.sc.mXq};   // this detector's
                wvd_v16i acc00 = {}, acc01 = {}, acc10 = {}, acc11 = {};
                {
#pragma unroll
                    for (int ks = 0; ks < KSR; ++ks) {
                        const wvd_v4i a0 = frag[ks % RD][0], a1 = frag[ks % RD][1];
                        {   // k-step ks + RD of this detector, or the first ones of the next
                            const wvd_v4i* Bf = ks + RD < KSR ? mb.B : Bnext;
                            const int kf = ks + RD < KSR ? ks + RD : ks + RD - KSR;
                            frag[ks % RD][0] = loadFrag(Bf, kf, 0);
                            frag[ks % RD][1] = loadFrag(Bf, kf, 1);
                        }
                        const int kp = ks < KS ? ks : KS - 1;   // a pad step: zero digits against any pixels
                        const wvd_v4i b0 = {(int)pkAll[kp][0], (int)pkAll[kp][1], (int)pkAll[kp][2], (int)pkAll[kp][3]};
                        const wvd_v4i b1 = {(int)pkAll[kp][4], (int)pkAll[kp][5], (int)pkAll[kp][6], (int)pkAll[kp][7]};
                        acc00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc00, 0, 0, 0);
                        acc01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc01, 0, 0, 0);
                        acc10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc10, 0, 0, 0);
                        acc11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc11, 0, 0, 0);
                    }
                }
                // ---- 4. / 5. fold and levels (wvd_fold, wvd_levels: one copy for both pre-filter kernels)
                double xq[2][8];
                wvd_fold(acc00, acc01, acc10, acc11, xq);
                const bool undecided = wvd_levels(C, sc, xq, sumx, sumxx, active, lane);
                if (undecided) survL[wave][d][lane] |= 1u << step;   // the lane's own word
            }
        }   // windows of the column
        // ---- 6. survivors -> each detector's stage-B queue, one returning atomic per wavefront, column walk and detector
        wave_sync();
#pragma unroll 1
        for (int d = 0; d < ND; ++d) {
            wvd_push_survivors(survL[wave][d][lane], K, ga.m[d].q, ga.m[d].qcount, wid0, (unsigned int)wl.nx, lane);
        }
        wave_sync();
    }
}

}  // namespace
