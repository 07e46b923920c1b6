// featuredetection_amd/csrc/particle_windows.hpp -- the samples of a resident particle set resolved to windows of a pyramid on the
// device, for the pyramid families of SingleClassifierModel (fd_particles_evaluate_pyramid).  Included by condensation.hip
// only.  The rule is fd_sample_window's (fd_internal.hpp): its part (a), width -> layer, is read from the host's table
// (fd_sample_layer_table, kept in the pyramid handle), its part (b), the placement, is fd_sample_place, the function the host calls.
#pragma once
#include "fd_internal.hpp"
#include "win_table.hpp"

namespace {

struct ParticleLayers {   // the kept layers as part (b) needs them, by value
    int32_t n;
    struct { double scale; int32_t w, h; } l[FD_WIN_MAX_LAYERS];
};

// One thread per particle: its sample (fd_particle_sample), the layer from the table (layerOf[w], widths from tableLen on have none), the
// window by fd_sample_place.  Every particle keeps slot i of the list: one without a
// window gets `spare`, a window that exists, so that the scoring kernels read valid memory; its row's score is never used
// (k_particles_weigh).  trace[i] = {layer, bx, by, valid} as fd_pyramid_sample_windows reports it.
__global__ __launch_bounds__(256) void k_particles_windows(const int32_t* __restrict__ x, const int32_t* __restrict__ y, const int32_t* __restrict__ size,
                                                           int n, double aspect, FdSampleMaps maps, ParticleLayers layers,
                                                           const int16_t* __restrict__ layerOf, int tableLen, int pw, int ph, FdSampleWindow spare,
                                                           int32_t* __restrict__ list, int4* __restrict__ trace, uint8_t* __restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t sx, sy, sw, sh;
    fd_particle_sample(x[i], y[i], size[i], aspect, maps, sx, sy, sw, sh);
    const int pos = sw > 0 && sw < tableLen ? (int)layerOf[sw] : -1;
    FdSampleWindow w = spare;
    bool ok = false;
    if (pos >= 0 && pos < layers.n) {
        int32_t bx, by;
        ok = fd_sample_place(layers.l[pos].scale, layers.l[pos].w, layers.l[pos].h, pw, ph, sx, sy, sw, sh, bx, by);
        if (ok) { w.layer = pos; w.bx = bx; w.by = by; }
    }
    list[3 * i] = w.layer; list[3 * i + 1] = w.bx; list[3 * i + 2] = w.by;
    trace[i] = ok ? make_int4(w.layer, w.bx, w.by, 1) : make_int4(-1, 0, 0, 0);
    valid[i] = ok ? 1 : 0;
}

// the pyramid's table for this patch width: built and uploaded (queued on ctx->stream) when the width or the kept layers have changed
void particle_windows_table(fd_ctx* ctx, fd_pyramid* pyr, int pw, const char* who) {
    fd_pyramid::SampleTable& T = pyr->sample_table;
    const int nLayers = (int)pyr->kept.size(), first = nLayers ? pyr->all[pyr->kept[0]].index : 0;
    if (T.length >= 0 && T.patch_w == pw && T.n_layers == nLayers && T.first_index == first && T.inc == pyr->inc) return;
    int length = 0;
    int rc = fd_sample_layer_table(nLayers, first, pyr->inc, pw, 0, nullptr, &length);
    if (rc == FD_OK || (rc == FD_ERR_CAPACITY && length <= FD_SAMPLE_TABLE_MAX)) {
        std::vector<int16_t> host((size_t)length);
        rc = fd_sample_layer_table(nLayers, first, pyr->inc, pw, length, host.data(), &length);
        if (rc == FD_OK) {
            if (T.length >= 0) HIP_CHECK(hipStreamSynchronize(ctx->stream));   // a launch still in flight may read the table this one replaces
            T.length = -1;
            T.host.swap(host);
            T.dev.reserve(sizeof(int16_t) * (size_t)std::max(length, 1));
            if (length) HIP_CHECK(hipMemcpyAsync(T.dev.p, T.host.data(), sizeof(int16_t) * (size_t)length, hipMemcpyHostToDevice, ctx->stream));
            T.length = length; T.patch_w = pw; T.n_layers = nLayers; T.first_index = first; T.inc = pyr->inc;
            return;
        }
    }
    if (rc == FD_ERR_CAPACITY)
        FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: the width -> layer table of this pyramid needs %d entries, at most %d", who, length, (int)FD_SAMPLE_TABLE_MAX);
    FD_THROW(FD_ERR_INVALID_ARGUMENT, "%s: no width -> layer table for %d layers from index %d, scale step %g, patch width %d", who, nLayers, first, pyr->inc, pw);
}

}  // namespace
