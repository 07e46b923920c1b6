// featuredetection_amd/csrc/rbf_mfma.hpp -- the device side of the fragment-major layout: what the f32 RBF kernels on the matrix
// pipe share.  k_svm_rbf_mfma_svs (svm.hip: support vectors in registers, patch tiles streamed) and k_hog_svm_fused
// (hog_svm_fused.hpp: HOG vectors in registers, support-vector tiles streamed) are the same tile computation with the register
// operand on the other side of the MFMA: one LDS-DMA tile load, one K loop, one epilogue.  The A-resident k_svm_rbf_mfma and the u8
// kernel share the types and the accumulator row map only.
//
// A tile is 32 vectors of KP = 8 Q floats, fragment-major: Q groups of 256 floats, lane (h, r) of a wavefront owns the float4 at
// group q, slot h * 32 + r = elements 8q + 4h .. + 3 of vector r (frag_index in svm.hip / hog.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fd_dev {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

// row of accumulator r of this lane in the 32 x 32 C/D layout (the column is lane & 31).  lane / 32, not lane >> 5: the compiler
// simplifies this function before it inlines it and would fold the shift into the multiplication; with the division the caller's own
// lane >> 5 (the half h of hsf_hog_tile) is found and shared as before, and k_hog_svm_fused keeps its instruction stream
__device__ __forceinline__ int mfma32_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane / 32); }

// One fragment-major tile of Q groups, global -> LDS, by the eight wavefronts of a workgroup: LDS-DMA, 1 KiB per wave instruction;
// wave w moves q-groups w, w + 8, ...  Issued through inline asm so that the compiler does not see a pending LDS write (it would
// wait vmcnt(0) before every ds_read of the tile being computed); completion is awaited explicitly (vmcnt(0) + barrier) before the
// buffer is read.  Recipe: cdna_hip_programming.md section 5.7 (M0 = wave-uniform LDS destination).
template <int Q>
__device__ __forceinline__ void lds_dma_tile(const float* gTile, float* ldsDst, int lane, int wave) {
    const char* g = (const char*)gTile + (size_t)lane * 16;
    for (int q = wave; q < Q; q += 8) {
        const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_void_t*)(ldsDst + q * 256));
        const char* gsrc = g + (size_t)q * 1024;
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
    }
}

// C[i = support vector][j = patch / window] of one LDS tile against the register-resident operand: 4 Q MFMAs, the LDS read of
// step q + 1 issued ahead of the MFMAs of step q.  ldsTileAtLane: the tile's first float4 of this lane.  REG_IS_A: the register
// operand holds the support vectors (first MFMA argument) -- otherwise the patches (second)
template <int Q, bool REG_IS_A>
__device__ __forceinline__ f32x16 mfma32_tile(const f32x4* ldsTileAtLane, const f32x4 (&reg)[Q]) {
    f32x16 acc = {0};
    f32x4 p = ldsTileAtLane[0];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const f32x4 pn = ldsTileAtLane[(size_t)(q + 1 < Q ? q + 1 : q) * 64];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if constexpr (REG_IS_A) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(reg[q][t], p[t], acc, 0, 0, 0);
            else acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p[t], reg[q][t], acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        p = pn;
    }
    return acc;
}

// RBF values of a tile's 32 support vectors for this lane's patch (|x|^2 = xx), added to s in accumulator order:
// d^2 = (|x|^2 + |s|^2) - 2 x.s.  svc64: |s|^2 of the 32 support vectors, then their coefficients.  The lane holds the 16 support
// vectors mfma32_row(0 .. 15, lane); the caller adds lane ^ 32's half where its own order of fp64 additions wants it
__device__ __forceinline__ void rbf_accumulate(double& s, const f32x16& acc, float xx, const float* svc64, float negGamma, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = mfma32_row(r, lane);
        const float d2 = (xx + svc64[row]) - 2.f * acc[r];
        s += (double)svc64[32 + row] * (double)__expf(negGamma * fmaxf(d2, 0.f));
    }
}

// sum over the `rows` partial rows of window i (rows `stride` doubles apart), in row order; eight loads in flight
__device__ __forceinline__ double sum_rows(const double* __restrict__ part, int rows, int64_t stride, int64_t i) {
    double s = 0.0;
    int g = 0;
    for (; g + 8 <= rows; g += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = part[(size_t)(g + k) * stride + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; g < rows; ++g) s += part[(size_t)g * stride + i];
    return s;
}

}  // namespace fd_dev
