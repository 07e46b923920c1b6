/* include/fd_hip_bench.h -- measurement hooks of libfd_hip.so.  NOT part of the drop-in boundary (include/fd_hip.h): nothing a
 * maintainer of the reference would bind.  bench.py and tools/ use them to time the dominant kernel of a product call with HIP
 * events on the stream the kernel is launched on.
 */
#ifndef FD_HIP_BENCH_H_
#define FD_HIP_BENCH_H_
#include "fd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* enable != 0: the detect entry points (fd_detect_five_stage, fd_detect_wvm, fd_detect_hog_svm[_begin/_end], fd_sdm_fit_batch)
 * bracket their dominant kernel(s) with two hipEvents on the context's stream. */
int fd_ctx_set_kernel_timing(fd_ctx* ctx, int enable);   /* enable == 2: WVM cascades bracket the dense pre-filter kernel only;
                                                          * enable == 3: every k_wvb_chain2 launch of stage B (one per phase), summed */
/* duration (ms) between those events for the last timed call on this context and the name of the bracketed kernel(s) */
int fd_last_kernel_ms(fd_ctx* ctx, const char** kernel_name, float* ms);
/* With fd_ctx_set_kernel_timing(ctx, 2): duration (ms) of the last k_wvm_prefilter_group launch of a batch entry point on this context
 * (HIP events on the stream it was launched on) and the number of detectors it served; members = 0: no group launch was timed.  Meant
 * for a batch that holds ONE group (several groups of a batch are queued by different host threads: the last writer wins). */
int fd_last_group_prefilter_ms(fd_ctx* ctx, float* ms, int* members);
/* With kernel timing on: the phases (ms, HIP events on the context's stream) of the last cascade step of the last fd_sdm_train, or of the
 * last fd_sdm_linear_regression, on this context: {descriptors and deltas, Gram, norm + lambda + diagonal, Cholesky (with the forward
 * substitution it carries), backward substitution + rounding, update + errors}.  fd_sdm_linear_regression: entries 0 and 5 are empty. */
int fd_sdm_train_last_phase_ms(fd_ctx* ctx, float* ms6);
/* the unrounded (double) D x N solution of the last successful fd_sdm_linear_regression on this context, of which x_out is the rounding to
 * float: what the backward-error bound of a Cholesky solve is stated for (FD_ERR_LOGIC when there is none of that size) */
int fd_debug_sdm_linear_regression_solution(fd_ctx* ctx, int D, int N, double* x64_out);

/* Windows the last finished cascade run of this handle handed to stage B (the pre-filter's queue; all frames of a multi-frame call
 * together); -1 before the first run.  bench.py reports the spread over the calls of a run. */
int64_t fd_wvm_last_queue_length(const fd_wvm* wvm);
/* The stage-B plan of the last finished run: out[0] = phases, then per phase {first generation, end generation, windows alive at its
 * start} (13 int64 at most: 1 + 3 * 4, the most phases a plan has); -1 where unknown.  bench.py derives the chain kernel's algorithmic work from it. */
int fd_wvm_last_stage_b_plan(const fd_wvm* wvm, int64_t* out);
/* How the last finished five-stage run of this handle did its overlap elimination: -1 on the host (no device tail was queued), 0 on
 * the device (csrc/fs_tail.hpp), > 0: the device kernel gave up and the host redid it -- 1 the order of the positives could not be
 * proven to be the reference's (tied or saturated probabilities), 2 more positives in a frame than the kernel holds, 4 window ids
 * beyond 32 bits, 0x100 stage-B queue / positive buffer overflow. */
int fd_wvm_last_tail_state(const fd_wvm* wvm);
/* How the last fd_detect_five_stage / fd_detect_five_stage_image call of this handle got its SVM scores: -1 the survivors of the host
 * overlap elimination were scored in a launch of their own (two host round trips: FD_FS_SPEC=0, the device tail, models without the
 * dense stage B or the u8 MFMA SVM), 0 the scores of all WVM positives were queued behind the cascade and used (one wait), 1 they were
 * queued but the frame had more positives than the launch covered (or stage B was rerun): the call fell back to the two round trips. */
int fd_wvm_last_spec_state(const fd_wvm* wvm);

/* Test hook, needs no GPU: the rect sums (WvmClassifier.cpp:277-306) of every used level of `md` for n equalised patches, computed
 * from the tables of the dense stage B with the operand addressing of its MFMA kernel.  out[i * ncols + c]: c runs over the levels
 * 0 .. numUsed - 1, grey values 1 .. cntval - 1 inside a level.  Returns ncols (out may be NULL), -1 when the model has no dense
 * stage B.  phase_gen (5 ints, may be NULL) receives the generation boundaries of the phases, -1 padded. */
int64_t fd_debug_wvb_rect_sums(const fd_wvm_model* md, const uint8_t* patches, int64_t n, int32_t* out, int32_t* phase_gen);

/* Test hook, needs no GPU: the work plan of the dense pre-filter (k_wvm_prefilter) for n_layers layers of nx[i] x ny[i] windows,
 * `frames` frames per launch, vertical window step sy, patch height ph, on a device with `slots` resident wavefronts.  A lane walks
 * down a column through K windows; lane task t of layer i is column t % nx[i], row group t / nx[i] (rows g K .. min(ny, (g + 1) K) - 1),
 * 64 tasks per tile.  Returns K (FD_WVD_K pins it); tile_first[i] = first tile of layer i inside a frame, tile_first[n_layers] = tiles
 * per frame. */
int fd_debug_wvd_plan(const int32_t* nx, const int32_t* ny, int n_layers, int frames, int sy, int ph, int slots, int32_t* tile_first);

/* Test hook, needs no GPU: the packed plan k_wvm_prefilter runs by default (FD_WVD_PACK=0 selects the plan above) for the same
 * arguments.  The (column, row group) tasks of all layers of a frame form ONE flat list -- layer-major, group-major, column-minor --
 * cut into tiles of 64; the ny rows of a column are dealt evenly over G = ceil(ny / K) groups (the first ny % G walk ny / G + 1
 * windows, the others ny / G).  Returns K (FD_WVD_K pins it; 1 when 2 sy > ph); *tiles_per_frame = ceil(*tasks_per_frame / 64).
 * decoded[4 i ..] = {layer, column, first window row, windows} of task tasks[i] (0 <= tasks[i] < *tasks_per_frame), from the function
 * the kernel decodes its lanes with.  The outputs may be NULL (tasks / decoded with n_tasks = 0). */
int fd_debug_wvd_packed_plan(const int32_t* nx, const int32_t* ny, int n_layers, int frames, int sy, int ph, int slots, int32_t* tiles_per_frame,
                             int32_t* tasks_per_frame, const int32_t* tasks, int64_t n_tasks, int32_t* decoded);

/* Test hook, needs no GPU: tile `tile` (row-major over the 62 x 16 output tiles) of cv::pyrDown of the sw x sh 8-bit image as
 * k_pyrdown_tiled stages it in LDS, made by the kernel's own tile-entry builder and per-lane staging function.  staged[r * 128 + c],
 * 35 x 128 bytes: source pixel (2 dy0 - 2 + r, 2 dx0 - 2 + c), BORDER_REFLECT_101, wherever a stored output of the tile reads it.
 * entry[8] = {src_off, dst_off, sw, sh, dx0, dy0, nx, ny} with the layer offsets 0 (dst_off: the tile's first output inside its
 * layer); nx x ny outputs are stored.  Returns the number of tiles of the layer (image, staged, entry all NULL: only that), or -1 when
 * there is no such tile. */
int fd_debug_pyrdown_stage(const uint8_t* image, int sw, int sh, int tile, uint8_t* staged, int32_t* entry);

/* Test hook, needs no GPU: tile `tile` (row-major over the 62 x 16 tiles of the pyrDown layer) of the fused cv::resize of the sw x sh
 * 8-bit image to a dw0 x dh0 first-octave layer and its cv::pyrDown, as k_resize_down stages it in LDS, made by the launch plan's own
 * column table and tile columns and the kernel's own row, fetch, interleave and addressing functions.  staged: 36 pair slots of 512
 * bytes, one per resized row of the tile (slot 35 repeats row 34): byte 2 x = source column X0 + x of the row's upper source row y0,
 * byte 2 x + 1 = the same column of its lower source row y1.  read_off[r * 127 + c], 35 x 127: the byte of the stage where the thread
 * of tile column c reads the 16-bit pair {y0, y1} of its left source column for tile row r (resized pixel (gy0 + r, gx0 + c),
 * BORDER_REFLECT_101); the right neighbour's pair is the next 16-bit word.  entry[8] = {X0, ncol, tx, ty, gx0, gy0, dw1, dh1}.
 * Returns the number of tiles of the layer (image, staged, read_off, entry all NULL: only that), or -1 when there is no such tile or
 * k_resize_down does not take such a layer. */
int fd_debug_resize_stage(const uint8_t* image, int sw, int sh, int dw0, int dh0, int tile, uint8_t* staged, int32_t* read_off, int32_t* entry);

/* Test hook: hyperplane distances of n u8 vectors through both instantiations of the u8 RBF MFMA kernel (8 and 16 wavefronts per
 * workgroup).  fd_detect_five_stage scores one frame's positives with either, depending on how many the previous frame had, and
 * relies on bit-identical sums; tests/test_gpu_cascade_hardening.py compares them.  (fd_detect_five_stage keeps per-call state in
 * the fd_wvm handle: one handle must not be used from two threads at a time.) */
int fd_debug_svm_u8_both(fd_ctx* ctx, const fd_svm* svm, const uint8_t* features, int64_t n, double* out8, double* out16);

/* Test hook: hyperplane distances through ONE named kernel body of svm.hip, launched with the geometry and the checks the library's
 * launchers use (tests/test_gpu_svm_score.py).  `features`: n host rows (u8 or f32, as the model), row_stride_bytes apart (f32: a
 * multiple of 4), staged on the device at that stride.  `idx` (may be NULL): n_idx slots into the rows; the launch then scores the
 * n_idx gathered rows, otherwise the n rows in order.  dcount < 0: no device-side count; otherwise the value is written to a device word
 * the kernel reads, and min(dcount, launch size) entries are scored.  `out` (one double per scored entry) is filled on the device with
 * a sentinel of all-one bits (a NaN) before the launch, so entries the kernel did not write can be told apart.
 * FD_ERR_INVALID_ARGUMENT, before anything is launched, for a variant the model cannot run (wrong dtype or kernel type, no tables,
 * padded length other than 328 / 336 for _SVS, LDS over budget) or that has no such argument: only the u8 MFMA kernels and
 * k_svm_generic read a count, the f32 MFMA kernels take no slot list. */
enum {
    FD_SVM_VARIANT_PRODUCTION = 0,         /* fd_svm_generic_launch_on; with a count fd_svm_u8_mfma_launch_counted (u8) / fd_svm_f32_launch_counted (f32) */
    FD_SVM_VARIANT_U8_MFMA_8 = 1,          /* k_svm_u8_rbf_mfma<8> */
    FD_SVM_VARIANT_U8_MFMA_16 = 2,         /* k_svm_u8_rbf_mfma<16> */
    FD_SVM_VARIANT_U8_LANES_2 = 3,         /* k_svm_u8_lanes<*, 2>: HIK or not as the model says */
    FD_SVM_VARIANT_U8_LANES_4 = 4,
    FD_SVM_VARIANT_U8_LANES_8 = 5,
    FD_SVM_VARIANT_GENERIC = 6,            /* k_svm_generic (f32 rows) */
    FD_SVM_VARIANT_RBF_MFMA = 7,           /* k_svm_rbf_mfma (A-resident); rows packed fragment-major, padded to 64, |x|^2 summed in float on the host */
    FD_SVM_VARIANT_RBF_MFMA_SVS = 8,       /* k_svm_rbf_mfma_svs<41 | 42> + k_sum_partials, same packing */
    FD_SVM_VARIANT_RBF_MFMA_PRODUCTION = 9 /* fd_svm_rbf_mfma_launch (what fd_detect_hog_svm calls; FD_SVM_KERNEL is read there), same packing */
};
int fd_debug_svm_launch(fd_ctx* ctx, const fd_svm* svm, const void* features, int64_t n, int64_t row_stride_bytes, const uint32_t* idx,
                        int64_t n_idx, int64_t dcount, int variant, double* out);

#ifdef __cplusplus
}
#endif
#endif /* FD_HIP_BENCH_H_ */
