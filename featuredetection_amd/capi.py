"""ctypes binding of the C ABI in include/fd_hip.h (libfd_hip.so).

This is plumbing for tests/bench only: the product is the shared library.  There is NO CPU
fallback -- loading fails loudly when the HIP extension has not been built, and every compute call
raises FdError when no gfx950 device is usable.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FD_HIP_LIB", os.path.join(_HERE, "libfd_hip.so"))   # FD_HIP_LIB: a differently built libfd_hip.so (A/B runs of kernel variants)

FD_OK, FD_ERR_INVALID_ARGUMENT, FD_ERR_RUNTIME, FD_ERR_LOGIC, FD_ERR_HIP, FD_ERR_CAPACITY, FD_ERR_DEVICE_CAPACITY = range(7)
FD_LAYER_NONE, FD_LAYER_GRADBIN, FD_LAYER_LBP, FD_LAYER_GRADMAG_LBP = 0, 1, 2, 3
FD_SAMPLES_HIST, FD_SAMPLES_EHOG, FD_SAMPLES_PATCH = 0, 1, 2
FD_SAMPLE_TABLE_MAX = 65536
FD_HIST_SAMPLES_MAX = 1 << 20
IMAGE_GRAY, IMAGE_GREYWORLD_GRAY = 0, 1   # fd_pyramid_set_image_filter
FD_KERNEL_LINEAR, FD_KERNEL_POLY, FD_KERNEL_RBF, FD_KERNEL_HIK = 0, 1, 2, 3
FD_DTYPE_U8, FD_DTYPE_F32 = 0, 1


class FdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fd_hip error %d: %s" % (code, msg))
        self.code = code


class fd_wvm_model(C.Structure):
    _fields_ = [("filter_w", C.c_int32), ("filter_h", C.c_int32), ("num_filters", C.c_int32), ("num_used", C.c_int32),
                ("num_per_level", C.c_int32), ("basis_param", C.c_float), ("bias", C.c_float),
                ("thresholds", C.POINTER(C.c_float)), ("hk_weights", C.POINTER(C.c_float)), ("pp", C.POINTER(C.c_double)),
                ("val_off", C.POINTER(C.c_int32)), ("val", C.POINTER(C.c_double)), ("rec_off", C.POINTER(C.c_int32)),
                ("rects", C.POINTER(C.c_uint8)), ("logistic_a", C.c_double), ("logistic_b", C.c_double),
                ("num_vals", C.c_int32), ("num_rects", C.c_int32)]


class fd_svm_model(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("p0", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("num_sv", C.c_int32),
                ("dim", C.c_int32), ("dtype", C.c_int32), ("support_vectors", C.c_void_p), ("coefficients", C.POINTER(C.c_float)),
                ("bias", C.c_float), ("threshold", C.c_float), ("logistic_a", C.c_double), ("logistic_b", C.c_double)]


class fd_detection(C.Structure):
    _fields_ = [("cx", C.c_int32), ("cy", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("layer", C.c_int32),
                ("lx", C.c_int32), ("ly", C.c_int32), ("level", C.c_int32), ("positive", C.c_int32), ("score", C.c_float),
                ("probability", C.c_double)]


class fd_hog_params(C.Structure):
    _fields_ = [("patch_w", C.c_int32), ("patch_h", C.c_int32), ("step_x", C.c_int32), ("step_y", C.c_int32),
                ("bins", C.c_int32), ("cell_size", C.c_int32), ("block_size", C.c_int32), ("signed_and_unsigned", C.c_int32)]


class fd_sdm_model(C.Structure):
    _fields_ = [("num_landmarks", C.c_int32), ("num_steps", C.c_int32), ("mean", C.POINTER(C.c_float)),
                ("R", C.POINTER(C.POINTER(C.c_float))), ("R_rows", C.POINTER(C.c_int32)), ("hog_variant", C.c_int32),
                ("desc_params", C.POINTER(C.c_int32))]


class fd_sdm_train_params(C.Structure):
    _fields_ = [("num_landmarks", C.c_int32), ("num_steps", C.c_int32), ("hog_variant", C.c_int32), ("desc_params", C.POINTER(C.c_int32)),
                ("regularisation", C.c_int32), ("lambda_", C.c_double), ("regularise_affine", C.c_int32)]


class fd_sdm_train_group(C.Structure):
    _fields_ = [("images", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("count", C.c_int32), ("on_device", C.c_int32)]


class fd_sdm_train_step_info(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("err_l1", C.c_double), ("err_fro", C.c_double), ("rows", C.c_int32), ("dim", C.c_int32),
                ("pivot_flag", C.c_int32)]


SDM_REG_MANUAL, SDM_REG_AUTOMATIC, SDM_REG_EIGENVALUE_THRESHOLD = 0, 1, 2

DET_DTYPE = np.dtype([("cx", "<i4"), ("cy", "<i4"), ("w", "<i4"), ("h", "<i4"), ("layer", "<i4"), ("lx", "<i4"),
                      ("ly", "<i4"), ("level", "<i4"), ("positive", "<i4"), ("score", "<f4"), ("probability", "<f8")],
                     align=True)
assert DET_DTYPE.itemsize == C.sizeof(fd_detection)

_lib = None

# every symbol include/fd_hip.h declares (checked by tests/test_capi_symbols.py against the header)
class fd_hist_params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("patch_w", "patch_h", "step_x", "step_y", "kind", "bins", "cell_size", "block_size",
                                         "levels", "interpolate", "signed_and_unsigned", "concatenate", "normalization", "cell_h",
                                         "block_h")]


class fd_whi_params(C.Structure):
    _fields_ = [("patch_w", C.c_int32), ("patch_h", C.c_int32), ("step_x", C.c_int32), ("step_y", C.c_int32), ("alpha", C.c_float),
                ("cutoff", C.c_float)]


BOX_DTYPE = np.dtype([("score", np.float32), ("x", np.int32), ("y", np.int32), ("w", np.int32), ("h", np.int32)])


class fd_fhog_params(C.Structure):
    _fields_ = [("cell_size", C.c_int32), ("unsigned_bins", C.c_int32), ("interpolate_bins", C.c_int32), ("interpolate_cells", C.c_int32),
                ("alpha", C.c_float)]


class fd_cehog_params(C.Structure):
    _fields_ = [("cell_size", C.c_int32), ("bin_count", C.c_int32), ("signed_gradients", C.c_int32), ("unsigned_gradients", C.c_int32),
                ("interpolate_bins", C.c_int32), ("interpolate_cells", C.c_int32), ("alpha", C.c_float)]


class fd_ehog_tracker_params(C.Structure):
    _fields_ = [("filter", fd_cehog_params), ("cell_cols", C.c_int32), ("cell_rows", C.c_int32), ("octave_layer_count", C.c_int32),
                ("min_width", C.c_int32), ("max_width", C.c_int32)]


class fd_svm_train_params(C.Structure):
    _fields_ = [("C", C.c_double), ("weight_pos", C.c_double), ("weight_neg", C.c_double), ("eps", C.c_double),
                ("max_iterations", C.c_int32), ("launch_iterations", C.c_int32)]


class fd_svm_train_info(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("n_sv", C.c_int32), ("n_bounded", C.c_int32), ("launches", C.c_int32),
                ("rho", C.c_double), ("objective", C.c_double)]


class fd_liblinear_params(C.Structure):
    _fields_ = [("C", C.c_double), ("weight_pos", C.c_double), ("weight_neg", C.c_double), ("eps", C.c_double), ("solver_tol", C.c_double),
                ("bias", C.c_int32), ("max_iterations", C.c_int32), ("max_cg_steps", C.c_int32), ("launch_steps", C.c_int32)]


class fd_liblinear_info(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("cg_steps", C.c_int32), ("converged", C.c_int32), ("stop", C.c_int32), ("n_active", C.c_int32),
                ("trace_len", C.c_int32), ("objective", C.c_double), ("gnorm", C.c_double), ("gnorm0", C.c_double), ("delta", C.c_double)]


class fd_liblinear_problem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("n_pos", C.c_int32), ("n_neg", C.c_int32), ("d", C.c_int32), ("is_device", C.c_int32),
                ("weights", C.c_void_p), ("bias", C.c_void_p), ("w", C.c_void_p)]


class fd_particles_arrays(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("x", "y", "size", "vx", "vy", "vsize", "weight", "score", "target", "cluster_id")]


class fd_particles_info(C.Structure):
    _fields_ = [("found", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("size", C.c_int32), ("vx", C.c_int32), ("vy", C.c_int32),
                ("vsize", C.c_float), ("cluster_id", C.c_int32), ("count", C.c_int32), ("n_valid", C.c_int32), ("n_target", C.c_int32),
                ("bad_weight", C.c_int32), ("best_score", C.c_double), ("weight_sum", C.c_double)]


class fd_particles_negatives_params(C.Structure):
    _fields_ = [("max_count", C.c_int32), ("offset_factor", C.c_float), ("down_scale", C.c_float), ("up_scale", C.c_float)]


class fd_particles_negative(C.Structure):
    _fields_ = [("index", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("size", C.c_int32), ("weight", C.c_double)]


class fd_particles_examples_params(C.Structure):
    _fields_ = [("positive_threshold", C.c_double), ("negative_threshold", C.c_double), ("max_count", C.c_int32), ("require_window", C.c_int32)]


class fd_particles_example(C.Structure):
    _fields_ = [("index", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("size", C.c_int32), ("valid", C.c_int32), ("weight", C.c_double)]


class fd_flow_params(C.Structure):
    _fields_ = [("win_w", C.c_int32), ("win_h", C.c_int32), ("max_level", C.c_int32), ("max_count", C.c_int32), ("epsilon", C.c_double),
                ("min_eig_threshold", C.c_double)]


class fd_flow_motion(C.Structure):
    _fields_ = [("ok", C.c_int32), ("n_valid", C.c_int32), ("n_correct", C.c_int32), ("median_x", C.c_float), ("median_y", C.c_float),
                ("median_ratio", C.c_float), ("order", C.c_void_p)]


class fd_flow_motion_info(C.Structure):
    _fields_ = [("ok", C.c_int32), ("n_valid", C.c_int32), ("n_correct", C.c_int32), ("median_x", C.c_float), ("median_y", C.c_float),
                ("median_ratio", C.c_float)]


class fd_sample_map(C.Structure):
    _fields_ = [("kind", C.c_int32), ("factor", C.c_double), ("x_offset", C.c_double), ("y_offset", C.c_double)]


class fd_svm_train_problem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("n_pos", C.c_int32), ("n_neg", C.c_int32), ("d", C.c_int32), ("is_device", C.c_int32),
                ("weights", C.c_void_p), ("bias", C.c_void_p), ("alpha", C.c_void_p)]


class fd_ehog_patch_params(C.Structure):
    _fields_ = [("patch_w", C.c_int32), ("patch_h", C.c_int32), ("bins", C.c_int32), ("cell_w", C.c_int32), ("cell_h", C.c_int32),
                ("interpolate", C.c_int32), ("signed_and_unsigned", C.c_int32), ("alpha", C.c_float)]


class fd_fpdw_params(C.Structure):
    _fields_ = [("cell_size", C.c_int32), ("fast_gradient", C.c_int32), ("interpolate", C.c_int32), ("normalization_radius", C.c_int32),
                ("normalization_constant", C.c_float)]


class fd_svm_kernel(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("p0", C.c_double), ("p1", C.c_double), ("p2", C.c_double)]


class fd_kernel_svm_train_problem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("n_pos", C.c_int32), ("n_neg", C.c_int32), ("d", C.c_int32), ("is_device", C.c_int32),
                ("sv_index", C.c_void_p), ("coefficients", C.c_void_p), ("support_vectors", C.c_void_p), ("bias", C.c_void_p),
                ("alpha", C.c_void_p)]


class fd_svm_one_class_params(C.Structure):
    _fields_ = [("nu", C.c_double), ("eps", C.c_double), ("max_iterations", C.c_int32), ("launch_iterations", C.c_int32)]


FD_SVM_CV_FOLDS = 5
FD_SVM_SIGMOID_CONVERGED, FD_SVM_SIGMOID_MAX_ITERATIONS, FD_SVM_SIGMOID_LINE_SEARCH_FAILED = 0, 1, 2


class fd_svm_cv_info(C.Structure):
    _fields_ = [("fold", fd_svm_train_info * FD_SVM_CV_FOLDS), ("fold_trained", C.c_int32 * FD_SVM_CV_FOLDS),
                ("fold_constant", C.c_double * FD_SVM_CV_FOLDS), ("newton_iterations", C.c_int32), ("status", C.c_int32)]


class fd_aggregated_params(C.Structure):
    _fields_ = [("fhog", fd_fhog_params), ("window_w", C.c_int32), ("window_h", C.c_int32), ("octave_layer_count", C.c_int32),
                ("min_window_width", C.c_int32), ("width_scale", C.c_float), ("height_scale", C.c_float), ("svm_weights", C.c_void_p),
                ("svm_bias", C.c_float), ("score_threshold", C.c_float), ("nms_overlap_threshold", C.c_double), ("nms_maximum_type", C.c_int32)]


class fd_five_stage_job(C.Structure):
    _fields_ = [("pyramid", C.c_void_p), ("wvm", C.c_void_p), ("svm", C.c_void_p), ("oe_dist", C.c_float), ("oe_ratio", C.c_float),
                ("step_x", C.c_int32), ("step_y", C.c_int32), ("roi", C.c_void_p), ("out", C.c_void_p), ("cap", C.c_int32),
                ("count", C.c_int32), ("stage_counts", C.c_int32 * 4), ("status", C.c_int32), ("image", C.c_void_p), ("image_w", C.c_int32),
                ("image_h", C.c_int32), ("image_channels", C.c_int32), ("image_is_device", C.c_int32)]


class fd_rvm_model(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("p0", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("num_filters", C.c_int32),
                ("num_used", C.c_int32), ("filter_w", C.c_int32), ("filter_h", C.c_int32), ("support_vectors", C.c_void_p),
                ("coefficients", C.c_void_p), ("thresholds", C.c_void_p), ("bias", C.c_float), ("logistic_a", C.c_double),
                ("logistic_b", C.c_double)]


class fd_rvm_detect_params(C.Structure):
    _fields_ = [("feature_space", C.c_int32), ("conv_scale", C.c_float), ("conv_shift", C.c_float), ("step_x", C.c_int32),
                ("step_y", C.c_int32)]


class fd_haar_params(C.Structure):
    _fields_ = [("sizes", C.POINTER(C.c_float)), ("num_sizes", C.c_int32), ("xs", C.POINTER(C.c_float)), ("num_xs", C.c_int32),
                ("ys", C.POINTER(C.c_float)), ("num_ys", C.c_int32), ("types", C.c_int32)]


class fd_surf_params(C.Structure):
    _fields_ = [("gradient_count", C.c_int32), ("cell_count", C.c_int32)]


class fd_integral_hog_params(C.Structure):
    _fields_ = [("grad_rows", C.c_int32), ("grad_cols", C.c_int32), ("bins", C.c_int32), ("signed_gradients", C.c_int32),
                ("interpolate_bins", C.c_int32), ("kind", C.c_int32), ("hist", fd_hist_params), ("ehog", fd_ehog_patch_params)]


HAAR_FEATURE_DTYPE = np.dtype([("rects", np.float32, (4, 4)), ("weights", np.float32, (4,)), ("num_rects", np.int32), ("factor", np.float32),
                               ("area", np.float32)])
HAAR_2RECTANGLE, HAAR_3RECTANGLE, HAAR_4RECTANGLE, HAAR_CENTER_SURROUND, HAAR_ALL = 1, 2, 4, 8, 15
INTEGRAL_HAAR, INTEGRAL_SURF, INTEGRAL_HOG = 0, 1, 2

FEATURE_GRAY, FEATURE_HQ64, FEATURE_HISTEQ = 0, 1, 2
FD_FEATURE_GRAY, FD_FEATURE_HQ64, FD_FEATURE_HISTEQ, FD_FEATURE_WHI = 0, 1, 2, 3   # WHI: the sampled gray-patch calls only


class fd_patch_samples_params(C.Structure):
    _fields_ = [("patch_w", C.c_int32), ("patch_h", C.c_int32), ("feature_space", C.c_int32), ("conv_scale", C.c_float),
                ("conv_shift", C.c_float), ("whi_alpha", C.c_float), ("whi_cutoff", C.c_float)]

HIST_HOG, HIST_SPATIAL, HIST_PYRAMID_HOG, HIST_SPATIAL_PYRAMID = 0, 1, 2, 3

_SIGS = {
    "fd_ctx_warm_streams": (C.c_int, [C.c_void_p]),
    "fd_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "fd_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "fd_ctx_destroy": (None, [C.c_void_p]),
    "fd_last_error": (C.c_char_p, [C.c_void_p]),
    "fd_ctx_synchronize": (C.c_int, [C.c_void_p]),
    "fd_version": (C.c_char_p, []),
    "fd_pyramid_create": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "fd_pyramid_create_inc": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "fd_pyramid_destroy": (None, [C.c_void_p]),
    "fd_pyramid_set_layer_filter": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fd_pyramid_set_image_filter": (C.c_int, [C.c_void_p, C.c_int]),
    "fd_pyramid_image_filter": (C.c_int, [C.c_void_p]),
    "fd_pyramid_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fd_pyramid_octave_layer_count": (C.c_int, [C.c_void_p]),
    "fd_pyramid_incremental_scale": (C.c_double, [C.c_void_p]),
    "fd_pyramid_layer_count": (C.c_int, [C.c_void_p]),
    "fd_pyramid_layer_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_pyramid_layer_download": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "fd_pyramid_set_frames": (C.c_int, [C.c_void_p, C.c_int]),
    "fd_pyramid_update_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fd_pyramid_frame_layer_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fd_detect_five_stage_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_detect_five_stage_frames_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                                    C.c_void_p, C.POINTER(C.c_void_p)]),
    "fd_detect_five_stage_frames_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_pyramid_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fd_pyramid_select_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "fd_dist_owner": (C.c_int, [C.c_int64, C.c_int]),
    "fd_dist_unique_id": (C.c_int, [C.c_void_p]),
    "fd_dist_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "fd_dist_destroy": (None, [C.c_void_p]),
    "fd_dist_rank": (C.c_int, [C.c_void_p]),
    "fd_dist_world": (C.c_int, [C.c_void_p]),
    "fd_pack_records": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]),
    "fd_dist_gather_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "fd_dist_gather_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "fd_dist_gather_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "fd_dist_gather_discard": (None, [C.c_void_p]),
    "fd_dist_gather_pending": (C.c_int, [C.c_void_p]),
    "fd_pyramid_set_gradient_blur": (C.c_int, [C.c_void_p, C.c_int]),
    "fd_pyramid_window_count": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]),
    "fd_pyramid_windows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int64)]),
    "fd_greyworld": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "fd_histeq64_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "fd_wvm_create": (C.c_int, [C.c_void_p, C.POINTER(fd_wvm_model), C.POINTER(C.c_void_p)]),
    "fd_wvm_destroy": (None, [C.c_void_p]),
    "fd_wvm_eval_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "fd_svm_create": (C.c_int, [C.c_void_p, C.POINTER(fd_svm_model), C.POINTER(C.c_void_p)]),
    "fd_svm_destroy": (None, [C.c_void_p]),
    "fd_svm_distance_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "fd_detect_wvm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]),
    "fd_detect_five_stage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "fd_detect_five_stage_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "fd_overlap_elimination": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int)]),
    "fd_block_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_hog_feature_length": (C.c_int, [C.POINTER(fd_hog_params)]),
    "fd_detect_hog_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_hog_params), C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]),
    "fd_hist_feature_length": (C.c_int, [C.POINTER(fd_hist_params), C.c_int]),
    "fd_extract_hist": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_hist_params), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "fd_detect_hist_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_hist_params), C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int64), C.c_void_p]),
    "fd_whi_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "fd_equalize_hist_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "fd_extract_whi": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_whi_params), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "fd_detect_whi_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_whi_params), C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]),
    "fd_fhog_size": (C.c_int, [C.POINTER(fd_fhog_params), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_fhog_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(fd_fhog_params), C.c_void_p]),
    "fd_fhog_image_channels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(fd_fhog_params), C.c_void_p]),
    "fd_pyramid_fhog_layer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(fd_fhog_params), C.c_void_p]),
    "fd_cehog_size": (C.c_int, [C.POINTER(fd_cehog_params), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_cehog_gradient_lut": (C.c_int, [C.POINTER(fd_cehog_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_cehog_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(fd_cehog_params), C.c_void_p]),
    "fd_pyramid_cehog_layer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(fd_cehog_params), C.c_void_p]),
    "fd_ehog_feature_length": (C.c_int, [C.POINTER(fd_ehog_patch_params), C.c_int]),
    "fd_ehog_patch_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(fd_ehog_patch_params), C.c_void_p]),
    "fd_ehog_tracker_plan_layers": (C.c_int, [C.POINTER(fd_ehog_tracker_params), C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_ehog_tracker_create": (C.c_int, [C.c_void_p, C.POINTER(fd_ehog_tracker_params), C.POINTER(C.c_void_p)]),
    "fd_ehog_tracker_destroy": (None, [C.c_void_p]),
    "fd_ehog_tracker_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fd_ehog_tracker_set_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]),
    "fd_ehog_tracker_evaluate_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_ehog_tracker_extract_cells": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_ehog_tracker_extract_patches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_ehog_tracker_patch_lds_bytes": (C.c_int, [C.POINTER(fd_ehog_tracker_params)]),
    "fd_ehog_tracker_heat_peak": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "fd_ehog_tracker_heat_maxima": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_ehog_tracker_get_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_ehog_tracker_feature_layer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fd_ehog_tracker_heat_layer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fd_linear_svm_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_linear_svm_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_train_params), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.POINTER(fd_svm_train_info)]),
    "fd_linear_svm_train_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(fd_svm_train_params), C.c_void_p]),
    "fd_ehog_tracker_train_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(fd_svm_train_params),
                                            C.POINTER(fd_svm_train_info)]),
    "fd_ehog_tracker_get_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "fd_linear_svm_train_limits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_linear_svm_gram_large": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_linear_svm_train_large": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_train_params), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(fd_svm_train_info)]),
    "fd_linear_svm_train_large_limits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_liblinear_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_liblinear_params), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(fd_liblinear_info)]),
    "fd_liblinear_train_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(fd_liblinear_params), C.c_void_p]),
    "fd_liblinear_objective": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_liblinear_params), C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "fd_liblinear_train_limits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int)]),
    "fd_kernel_svm_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_kernel), C.c_void_p, C.c_void_p]),
    "fd_kernel_svm_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_kernel),
                                      C.POINTER(fd_svm_train_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(fd_svm_train_info)]),
    "fd_kernel_svm_train_model": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_kernel),
                                            C.POINTER(fd_svm_train_params), C.c_float, C.c_double, C.c_double, C.POINTER(C.c_void_p),
                                            C.POINTER(fd_svm_train_info)]),
    "fd_kernel_svm_train_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(fd_svm_kernel), C.POINTER(fd_svm_train_params), C.c_void_p]),
    "fd_kernel_svm_train_limits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_one_class_svm_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_kernel), C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "fd_one_class_svm_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_kernel),
                                         C.POINTER(fd_svm_one_class_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(fd_svm_train_info)]),
    "fd_one_class_svm_train_model": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_kernel),
                                               C.POINTER(fd_svm_one_class_params), C.c_float, C.c_double, C.c_double, C.POINTER(C.c_void_p),
                                               C.POINTER(fd_svm_train_info)]),
    "fd_one_class_svm_train_limits": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_kernel_svm_cv_sigmoid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fd_svm_kernel),
                                           C.POINTER(fd_svm_train_params), C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.c_void_p, C.POINTER(fd_svm_cv_info)]),
    "fd_svm_sigmoid_train": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]),
    "fd_aggregated_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fd_aggregated_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_aggregated_set_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]),
    "fd_particles_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fd_particles_destroy": (None, [C.c_void_p]),
    "fd_particles_capacity": (C.c_int, [C.c_void_p]),
    "fd_particles_route_enabled": (C.c_int, []),
    "fd_particles_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(fd_particles_arrays)]),
    "fd_particles_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(fd_particles_arrays)]),
    "fd_particles_get_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_particles_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int32]),
    "fd_particles_evaluate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double]),
    "fd_particles_weigh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double]),
    "fd_particles_state": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_particles_info)]),
    "fd_flow_default_params": (C.c_int, [C.POINTER(fd_flow_params)]),
    "fd_flow_limits": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_flow_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(fd_flow_params), C.POINTER(C.c_void_p)]),
    "fd_flow_destroy": (None, [C.c_void_p]),
    "fd_flow_levels": (C.c_int, [C.c_void_p]),
    "fd_flow_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fd_flow_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_flow_track_fb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_debug_flow_level": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_flow_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_flow_median": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(fd_flow_motion)]),
    "fd_particles_create_unbound": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fd_sample_maps_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fd_particles_evaluate_integral": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int]),
    "fd_particles_weigh_classifier": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "fd_particles_evaluate_pyramid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int]),
    "fd_particles_evaluate_wvm_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int]),
    "fd_particles_weigh_wvm_svm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_particles_get_wvm_svm_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "fd_sample_layer_table": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_flow_track_fb_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fd_flow_get_tracks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_debug_flow_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.POINTER(fd_flow_motion_info)]),
    "fd_particles_sample_flow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "fd_particles_state_flow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_particles_info), C.POINTER(fd_flow_motion_info)]),
    "fd_particles_negatives_bounds": (C.c_int, [C.POINTER(fd_particles_negatives_params), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "fd_particles_state_negatives": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_particles_negatives_params), C.POINTER(fd_particles_info),
                                               C.POINTER(fd_flow_motion_info), C.POINTER(C.c_int), C.POINTER(fd_particles_negative)]),
    "fd_particles_examples_select": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(fd_particles_examples_params), C.POINTER(C.c_int), C.c_void_p,
                                               C.POINTER(C.c_int), C.c_void_p]),
    "fd_particles_examples_bounds": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_particles_state_examples_pyramid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_int,
                                                      C.POINTER(fd_particles_examples_params), C.POINTER(fd_particles_info), C.POINTER(fd_flow_motion_info),
                                                      C.POINTER(C.c_int), C.POINTER(fd_particles_example), C.POINTER(C.c_int),
                                                      C.POINTER(fd_particles_example), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_particles_state_examples_integral": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_int,
                                                       C.POINTER(fd_particles_examples_params), C.POINTER(fd_particles_info), C.POINTER(fd_flow_motion_info),
                                                       C.POINTER(C.c_int), C.POINTER(fd_particles_example), C.POINTER(C.c_int),
                                                       C.POINTER(fd_particles_example), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_aggregated_create": (C.c_int, [C.c_void_p, C.POINTER(fd_aggregated_params), C.POINTER(C.c_void_p)]),
    "fd_aggregated_destroy": (None, [C.c_void_p]),
    "fd_aggregated_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_int), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_aggregated_create_approximated": (C.c_int, [C.c_void_p, C.POINTER(fd_aggregated_params), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fd_aggregated_get_lambdas": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_aggregated_get_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_aggregated_feature_layer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fd_aggregated_plan_layers": (C.c_int, [C.c_int] * 7 + [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_fpdw_size": (C.c_int, [C.POINTER(fd_fpdw_params), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_fpdw_gradient_lut": (C.c_int, [C.POINTER(fd_fpdw_params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_fpdw_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(fd_fpdw_params), C.c_void_p]),
    "fd_fpdw_cells_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(fd_fpdw_params), C.c_void_p]),
    "fd_aggregated_create_fpdw": (C.c_int, [C.c_void_p, C.POINTER(fd_aggregated_params), C.POINTER(fd_fpdw_params), C.c_int, C.c_void_p, C.c_int,
                                            C.POINTER(C.c_void_p)]),
    "fd_nms_iou": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "fd_wvm_svm_evaluate_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_five_stage_batch_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fd_five_stage_batch_end": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fd_detect_five_stage_batch": (C.c_int, [C.c_void_p, C.POINTER(fd_five_stage_job), C.c_int]),
    "fd_rvm_create": (C.c_int, [C.c_void_p, C.POINTER(fd_rvm_model), C.POINTER(C.c_void_p)]),
    "fd_rvm_destroy": (None, [C.c_void_p]),
    "fd_rvm_eval_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "fd_detect_rvm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_rvm_detect_params), C.c_void_p, C.c_void_p, C.c_int64,
                                C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]),
    "fd_detect_five_stage_rvm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_rvm_detect_params), C.c_void_p, C.c_void_p, C.c_float,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "fd_detect_five_stage_rvm_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_rvm_detect_params), C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "fd_extract_hog": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_hog_params), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "fd_gradient_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fd_gradient_filter_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fd_gradient_binning_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fd_lbp_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fd_hist_patch_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(fd_hist_params), C.c_void_p]),
    "fd_whitening_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "fd_convert_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_int]),
    "fd_unit_norm_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "fd_detect_hog_svm_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fd_hog_params), C.POINTER(C.c_void_p)]),
    "fd_detect_hog_svm_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "fd_sdm_create": (C.c_int, [C.c_void_p, C.POINTER(fd_sdm_model), C.POINTER(C.c_void_p)]),
    "fd_sdm_destroy": (None, [C.c_void_p]),
    "fd_sdm_descriptors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "fd_sdm_fit_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "fd_sdm_fit_batch_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fd_sdm_fit_batch_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_sdm_optimize_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_sdm_train": (C.c_int, [C.c_void_p, C.POINTER(fd_sdm_train_params), C.POINTER(fd_sdm_train_group), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(fd_sdm_train_step_info)]),
    "fd_sdm_linear_regression": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                           C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "fd_sdm_train_step_dims": (C.c_int, [C.POINTER(fd_sdm_train_params), C.c_void_p]),
    "fd_sdm_train_limits": (C.c_int, [C.POINTER(fd_sdm_train_params), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "fd_integral_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "fd_integral_destroy": (None, [C.c_void_p]),
    "fd_integral_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fd_integral_set_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "fd_integral_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fd_integral_download": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fd_integral_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fd_haar_grid": (C.c_int, [C.c_int, C.c_void_p]),
    "fd_haar_feature_count": (C.c_int, [C.POINTER(fd_haar_params)]),
    "fd_haar_features": (C.c_int, [C.POINTER(fd_haar_params), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "fd_integral_extract_haar": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_haar_params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_integral_gradient_patches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_gradient_sum_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fd_integral_extract_surf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_integral_svm_evaluate_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
    "fd_integral_hog_feature_length": (C.c_int, [C.POINTER(fd_integral_hog_params)]),
    "fd_integral_gradient_samples_valid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_integral_extract_hog": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_integral_hog_params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_integral_image_length": (C.c_int, [C.c_int, C.c_int]),
    "fd_integral_gradient_length": (C.c_int, [C.c_int, C.c_int]),
    "fd_gradient_sum_length": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "fd_surf_feature_length": (C.c_int, [C.c_int, C.c_int]),
    "fd_gradient_magnitude_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fd_sample_windows": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "fd_pyramid_sample_windows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_hist_samples_limits": (C.c_int, [C.POINTER(C.c_int)]),
    "fd_hist_extract_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_hist_params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_ehog_extract_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_ehog_patch_params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_hist_svm_evaluate_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "fd_hist_svm_evaluate_samples_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p]),
    "fd_patch_feature_length": (C.c_int, [C.POINTER(fd_patch_samples_params)]),
    "fd_patch_extract_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_patch_samples_params), C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "fd_patch_svm_evaluate_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_patch_samples_params), C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "fd_patch_rvm_evaluate_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(fd_patch_samples_params), C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/fd_hip_bench.h: measurement hooks (not part of the drop-in boundary)
_BENCH_SIGS = {
    "fd_debug_svm_u8_both": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "fd_debug_svm_launch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    "fd_ctx_set_kernel_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "fd_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float)]),
    "fd_sdm_train_last_phase_ms": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fd_debug_sdm_linear_regression_solution": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fd_last_group_prefilter_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "fd_debug_wvb_rect_sums": (C.c_int64, [C.POINTER(fd_wvm_model), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "fd_wvm_last_queue_length": (C.c_int64, [C.c_void_p]),
    "fd_wvm_last_tail_state": (C.c_int, [C.c_void_p]),
    "fd_wvm_last_spec_state": (C.c_int, [C.c_void_p]),
    "fd_wvm_last_stage_b_plan": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fd_debug_wvd_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fd_debug_wvd_packed_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_void_p]),
    "fd_debug_pyrdown_stage": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fd_debug_resize_stage": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def lib():
    """Loads libfd_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in list(_SIGS.items()) + list(_BENCH_SIGS.items()):
            f = getattr(l, name)  # AttributeError if the ABI lost a symbol
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _c(arr, dtype):
    return np.ascontiguousarray(arr, dtype=dtype)


class Context:
    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        rc = lib().fd_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h))
        if rc != FD_OK:
            raise FdError(rc, "fd_ctx_create failed (no usable gfx950 device?)")

    def check(self, rc):
        if rc != FD_OK:
            raise FdError(rc, lib().fd_last_error(self.h).decode())

    def synchronize(self):
        self.check(lib().fd_ctx_synchronize(self.h))

    def close(self):
        if self.h:
            lib().fd_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def set_kernel_timing(self, enable=True):
        self.check(lib().fd_ctx_set_kernel_timing(self.h, int(enable)))

    def last_kernel_ms(self):
        name = C.c_char_p()
        ms = C.c_float()
        lib().fd_last_kernel_ms(self.h, C.byref(name), C.byref(ms))
        return (name.value or b"").decode(), float(ms.value)

    def warm_streams(self):
        self.check(lib().fd_ctx_warm_streams(self.h))

    def last_group_prefilter_ms(self):
        """(ms, members) of the last k_wvm_prefilter_group launch timed with set_kernel_timing(2); members == 0: none"""
        ms, n = C.c_float(), C.c_int()
        self.check(lib().fd_last_group_prefilter_ms(self.h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    # ---- stand-alone filters
    def histeq64(self, patches):
        patches = _c(patches, np.uint8)
        n, h, w = patches.shape
        out = np.empty_like(patches)
        self.check(lib().fd_histeq64_batch(self.h, _ptr(patches), n, w, h, _ptr(out)))
        return out

    def greyworld(self, bgr):
        bgr = _c(bgr, np.uint8)
        out = np.empty_like(bgr)
        self.check(lib().fd_greyworld(self.h, _ptr(bgr), bgr.shape[1], bgr.shape[0], _ptr(out), 0))
        return out


class Pyramid:
    def __init__(self, ctx, octave_layers=None, min_scale=0.09, max_scale=0.25, inc=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        if inc is not None:
            ctx.check(lib().fd_pyramid_create_inc(ctx.h, inc, min_scale, max_scale, C.byref(self.h)))
        else:
            ctx.check(lib().fd_pyramid_create(ctx.h, octave_layers, min_scale, max_scale, C.byref(self.h)))

    def set_layer_filter(self, kind, bins=9, signed_gradients=False, interpolate=False, grad_kernel=1, lbp_type=0, blur_kernel=0):
        self.ctx.check(lib().fd_pyramid_set_layer_filter(self.h, kind, bins, int(signed_gradients), int(interpolate), grad_kernel,
                                                         lbp_type))
        self.ctx.check(lib().fd_pyramid_set_gradient_blur(self.h, blur_kernel))

    def set_image_filter(self, kind):
        """IMAGE_GRAY (default) or IMAGE_GREYWORLD_GRAY: GreyWorldNormalizationFilter in front of the gray conversion, for every later update"""
        self.ctx.check(lib().fd_pyramid_set_image_filter(self.h, kind))

    @property
    def image_filter(self):
        return lib().fd_pyramid_image_filter(self.h)

    def update(self, image):
        image = _c(image, np.uint8)
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        self.ctx.check(lib().fd_pyramid_update(self.h, _ptr(image), w, h, ch, 0))

    def update_device(self, dev_ptr, w, h, ch):
        self.ctx.check(lib().fd_pyramid_update(self.h, C.c_void_p(dev_ptr), w, h, ch, 1))

    @property
    def octave_layers(self):
        return lib().fd_pyramid_octave_layer_count(self.h)

    @property
    def inc(self):
        return lib().fd_pyramid_incremental_scale(self.h)

    def layers(self):
        out = []
        for i in range(lib().fd_pyramid_layer_count(self.h)):
            idx, w, h, ch = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            sc = C.c_double()
            lib().fd_pyramid_layer_info(self.h, i, C.byref(idx), C.byref(sc), C.byref(w), C.byref(h), C.byref(ch))
            out.append(dict(index=idx.value, scale=sc.value, w=w.value, h=h.value, ch=ch.value))
        return out

    def layer(self, i):
        info = self.layers()[i]
        shape = (info["h"], info["w"]) if info["ch"] == 1 else (info["h"], info["w"], info["ch"])
        a = np.empty(shape, np.uint8)
        self.ctx.check(lib().fd_pyramid_layer_download(self.h, i, _ptr(a)))
        return a

    def set_frames(self, n):
        """the pyramid holds n frames of identical size (one launch per pyramid stage, one cascade run for all of them)"""
        self.ctx.check(lib().fd_pyramid_set_frames(self.h, n))
        self.nframes = n

    def update_frames(self, images=None, device_ptrs=None, w=0, h=0, ch=0):
        """images: list of equally sized host arrays, or device_ptrs + (w, h, ch) for frames resident in HBM"""
        if images is not None:
            imgs = [np.ascontiguousarray(i, np.uint8) for i in images]
            h, w = imgs[0].shape[:2]
            ch = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
            ptrs = (C.c_void_p * len(imgs))(*[i.ctypes.data for i in imgs])
            self.ctx.check(lib().fd_pyramid_update_frames(self.h, ptrs, len(imgs), w, h, ch, 0))
        else:
            ptrs = (C.c_void_p * len(device_ptrs))(*device_ptrs)
            self.ctx.check(lib().fd_pyramid_update_frames(self.h, ptrs, len(device_ptrs), w, h, ch, 1))

    def frame_layer(self, frame, i):
        info = self.layers()[i]
        shape = (info["h"], info["w"]) if info["ch"] == 1 else (info["h"], info["w"], info["ch"])
        out = np.empty(shape, np.uint8)
        self.ctx.check(lib().fd_pyramid_frame_layer_download(self.h, frame, i, _ptr(out)))
        return out

    def select(self, first_layer=-1, last_layer=-1, step_layer=1, roi=None):
        """layer sub-range / default roi of every enumeration that follows; select() resets"""
        r = _c(roi, np.int32) if roi is not None else None
        self.ctx.check(lib().fd_pyramid_select(self.h, first_layer, last_layer, step_layer, _ptr(r)))

    def window_count(self, pw, ph, sx, sy, roi=None):
        n = C.c_int64()
        r = _c(roi, np.int32) if roi is not None else None
        self.ctx.check(lib().fd_pyramid_window_count(self.h, pw, ph, sx, sy, _ptr(r), C.byref(n)))
        return n.value

    def sample_windows(self, pw, ph, samples):
        """samples (n, 4) {x, y, width, height} -> (n, 4) int32 {layer position, bx, by, valid} by the sample -> window rule"""
        s = _c(samples, np.int32).reshape(-1, 4)
        out = np.zeros((len(s), 4), np.int32)
        self.ctx.check(lib().fd_pyramid_sample_windows(self.h, pw, ph, len(s), _ptr(s), _ptr(out)))
        return out

    def windows(self, pw, ph, sx, sy, roi=None):
        n = self.window_count(pw, ph, sx, sy, roi)
        out = np.empty((n, 7), np.int32)
        r = _c(roi, np.int32) if roi is not None else None
        cnt = C.c_int64()
        self.ctx.check(lib().fd_pyramid_windows(self.h, pw, ph, sx, sy, _ptr(r), _ptr(out), n, C.byref(cnt)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().fd_pyramid_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):   # a handle nobody holds any more gives its device memory back (hipFree waits for the device)
        try:
            self.close()
        except Exception:
            pass


def _wvm_struct(m, cls):
    """m: dict of numpy arrays (featuredetection_amd.synth.make_wvm); cls: the ctypes struct type."""
    keep = dict(thresholds=_c(m["thresholds"], np.float32), hk_weights=_c(m["hk_weights"], np.float32),
                pp=_c(m["pp"], np.float64), val_off=_c(m["val_off"], np.int32), val=_c(m["val"], np.float64),
                rec_off=_c(m["rec_off"], np.int32), rects=_c(m["rects"], np.uint8))
    s = cls()
    s.filter_w, s.filter_h = int(m["filter_w"]), int(m["filter_h"])
    s.num_filters, s.num_used, s.num_per_level = int(m["num_filters"]), int(m["num_used"]), int(m["num_per_level"])
    s.basis_param, s.bias = float(m["basis_param"]), float(m["bias"])
    s.thresholds = keep["thresholds"].ctypes.data_as(C.POINTER(C.c_float))
    s.hk_weights = keep["hk_weights"].ctypes.data_as(C.POINTER(C.c_float))
    s.pp = keep["pp"].ctypes.data_as(C.POINTER(C.c_double))
    s.val_off = keep["val_off"].ctypes.data_as(C.POINTER(C.c_int32))
    s.val = keep["val"].ctypes.data_as(C.POINTER(C.c_double))
    s.rec_off = keep["rec_off"].ctypes.data_as(C.POINTER(C.c_int32))
    s.rects = keep["rects"].ctypes.data_as(C.POINTER(C.c_uint8))
    s.logistic_a, s.logistic_b = float(m["logistic_a"]), float(m["logistic_b"])
    if hasattr(s, "num_vals"):   # fd_wvm_model: array lengths, so that the library can reject truncated models
        s.num_vals, s.num_rects = len(keep["val"]), len(keep["rects"].reshape(-1, 4))
    return s, keep


class Wvm:
    def __init__(self, ctx, model):
        self.ctx = ctx
        self.model = model
        s, keep = _wvm_struct(model, fd_wvm_model)
        self.h = C.c_void_p()
        ctx.check(lib().fd_wvm_create(ctx.h, C.byref(s), C.byref(self.h)))

    def last_queue_length(self):
        """measurement hook: windows the last finished run queued for stage B (-1 before the first run)"""
        return int(lib().fd_wvm_last_queue_length(self.h))

    def last_stage_b_plan(self):
        """measurement hook: [(first generation, end generation, windows alive at its start)] per stage-B phase of the last finished run"""
        out = np.full(13, -1, np.int64)   # 1 + 3 * WVB_MAXPHASE
        lib().fd_wvm_last_stage_b_plan(self.h, _ptr(out))
        return [(int(out[1 + 3 * i]), int(out[2 + 3 * i]), int(out[3 + 3 * i])) for i in range(max(0, int(out[0])))]

    def last_spec_state(self):
        """test hook: -1 the survivors' SVM launch of its own, 0 the scores of all positives queued behind the cascade were used, 1 queued
        but not usable: fell back (fd_hip_bench.h)"""
        return int(lib().fd_wvm_last_spec_state(self.h))

    def last_tail_state(self):
        """test hook: -1 overlap elimination on the host, 0 on the device, > 0 the device kernel gave up (fd_hip_bench.h)"""
        return int(lib().fd_wvm_last_tail_state(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().fd_wvm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):   # a handle nobody holds any more gives its device memory back (hipFree waits for the device)
        try:
            self.close()
        except Exception:
            pass


def pack_records(image_id, detector_id, dets):
    """fd_pack_records: fd_detection array -> float64 [n, 8] {image, detector, cx, cy, w, h, score, probability} (host only)"""
    dets = np.ascontiguousarray(dets, DET_DTYPE)
    out = np.zeros((len(dets), 8), np.float64)
    rc = lib().fd_pack_records(int(image_id), int(detector_id), _ptr(dets), len(dets), _ptr(out))
    if rc != FD_OK:
        raise FdError(rc, "fd_pack_records")
    return out


class Dist:
    """fd_dist_*: image-shard data parallelism, one process per GPU; gather() = one ncclAllGather of the detection records"""

    def __init__(self, ctx, rank=0, world=1, unique_id=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        idb = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id)) if unique_id is not None else None
        ctx.check(lib().fd_dist_init(ctx.h, rank, world, idb, C.byref(self.h)))

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        rc = lib().fd_dist_unique_id(buf)
        if rc != FD_OK:
            raise FdError(rc, "fd_dist_unique_id (librccl)")
        return bytes(buf)

    def gather(self, local, cap):
        local = np.ascontiguousarray(local, np.float64).reshape(-1, 8)
        world = lib().fd_dist_world(self.h)
        out = np.zeros((world * cap, 8), np.float64)
        n, tr = C.c_int64(), C.c_int()
        self.ctx.check(lib().fd_dist_gather_records(self.h, _ptr(local), len(local), cap, _ptr(out), len(out), C.byref(n), C.byref(tr)))
        return out[:n.value], bool(tr.value)

    def gather_begin(self, local, cap):
        """fd_dist_gather_begin: header exchange + the payload collective queued on the handle's own stream"""
        local = np.ascontiguousarray(local, np.float64).reshape(-1, 8)
        self._cap = cap
        self.ctx.check(lib().fd_dist_gather_begin(self.h, _ptr(local), len(local), cap))

    def gather_end(self):
        """fd_dist_gather_end -> (records of all ranks, truncated)"""
        world = lib().fd_dist_world(self.h)
        n, tr = C.c_int64(), C.c_int()
        self.ctx.check(lib().fd_dist_gather_end(self.h, None, 0, C.byref(n), C.byref(tr)))   # count first: the buffer follows the records
        out = np.zeros((max(int(n.value), 1), 8), np.float64)
        self.ctx.check(lib().fd_dist_gather_end(self.h, _ptr(out), len(out), C.byref(n), C.byref(tr)))
        return out[:n.value], bool(tr.value)

    def discard(self):
        """fd_dist_gather_discard: drop the gathered set a count-only call / FD_ERR_CAPACITY left in the handle"""
        lib().fd_dist_gather_discard(self.h)

    def pending(self):
        return bool(lib().fd_dist_gather_pending(self.h))

    def close(self):
        if self.h:
            lib().fd_dist_destroy(self.h)
            self.h = C.c_void_p()


def dist_gather_count(dist, local, cap):
    """fd_dist_gather_records with all == NULL: runs the collective and returns the number of records waiting in the handle"""
    local = np.ascontiguousarray(local, np.float64).reshape(-1, 8)
    n, tr = C.c_int64(), C.c_int()
    dist.ctx.check(lib().fd_dist_gather_records(dist.h, _ptr(local), len(local), cap, None, 0, C.byref(n), C.byref(tr)))
    return int(n.value)


def svm_u8_both(ctx, svm, feats):
    """Test hook: distances of u8 vectors through k_svm_u8_rbf_mfma<8> and <16> -> (out8, out16)"""
    feats = _c(feats, np.uint8).reshape(-1, svm.dim)
    o8, o16 = np.empty(len(feats), np.float64), np.empty(len(feats), np.float64)
    ctx.check(lib().fd_debug_svm_u8_both(ctx.h, svm.h, _ptr(feats), len(feats), _ptr(o8), _ptr(o16)))
    return o8, o16


# fd_debug_svm_launch: the kernel bodies of svm.hip by name (include/fd_hip_bench.h)
(SVM_PRODUCTION, SVM_U8_MFMA_8, SVM_U8_MFMA_16, SVM_U8_LANES_2, SVM_U8_LANES_4, SVM_U8_LANES_8, SVM_GENERIC, SVM_RBF_MFMA, SVM_RBF_MFMA_SVS,
 SVM_RBF_MFMA_PRODUCTION) = range(10)


def svm_launch(ctx, svm, feats, variant, idx=None, dcount=-1, n=None):
    """Test hook: distances through one named kernel body.  feats: 2-D array of the model's dtype whose rows may be longer than svm.dim
    (the row stride is feats.strides[0]; only the first svm.dim elements of a row belong to the vector); n: score only the first n
    rows; idx: slots into those rows (the launch scores len(idx) gathered rows); dcount >= 0: a device-side count.  Returns float64
    [len(idx) or n]; entries the kernel did not write are NaN with all bits set (SVM_SENTINEL_BITS)."""
    assert feats.ndim == 2 and feats.dtype == svm.np_dtype and feats.shape[1] >= svm.dim and feats.strides[1] == feats.itemsize
    n = feats.shape[0] if n is None else n
    assert 1 <= n <= feats.shape[0]
    if idx is not None:
        idx = _c(idx, np.uint32)
    out = np.zeros(len(idx) if idx is not None else n, np.float64)
    ctx.check(lib().fd_debug_svm_launch(ctx.h, svm.h, C.c_void_p(feats.ctypes.data), n, feats.strides[0], _ptr(idx), len(idx) if idx is not None else 0,
                                        int(dcount), int(variant), _ptr(out)))
    return out


SVM_SENTINEL_BITS = 0xFFFFFFFFFFFFFFFF


def wvd_plan(nx, ny, frames, sy, ph, slots):
    """Test hook (no GPU): the dense pre-filter's plan for layers of nx[i] x ny[i] windows -> (K, first tile of every layer + tiles per frame)"""
    nx, ny = _c(nx, np.int32), _c(ny, np.int32)
    first = np.zeros(len(nx) + 1, np.int32)
    k = lib().fd_debug_wvd_plan(_ptr(nx), _ptr(ny), len(nx), frames, sy, ph, slots, _ptr(first))
    if k < 1:
        raise FdError(k, "fd_debug_wvd_plan")
    return k, first


def wvd_packed_plan(nx, ny, frames, sy, ph, slots, tasks=None):
    """Test hook (no GPU): the pre-filter's packed plan -> (K, tiles per frame, tasks per frame, decoded), decoded[i] = (layer, column,
    first window row, windows) of tasks[i]; tasks=None decodes every task of a frame"""
    nx, ny = _c(nx, np.int32), _c(ny, np.int32)
    tiles, ntask = C.c_int32(), C.c_int32()
    k = lib().fd_debug_wvd_packed_plan(_ptr(nx), _ptr(ny), len(nx), frames, sy, ph, slots, C.byref(tiles), C.byref(ntask), None, 0, None)
    if k < 1:
        raise FdError(k, "fd_debug_wvd_packed_plan")
    tasks = np.arange(ntask.value, dtype=np.int32) if tasks is None else _c(tasks, np.int32)
    dec = np.zeros((len(tasks), 4), np.int32)
    if len(tasks):
        k = lib().fd_debug_wvd_packed_plan(_ptr(nx), _ptr(ny), len(nx), frames, sy, ph, slots, None, None, _ptr(tasks), len(tasks), _ptr(dec))
        if k < 1:
            raise FdError(k, "fd_debug_wvd_packed_plan")
    return k, tiles.value, ntask.value, dec


def pyrdown_stage(image, tile):
    """Test hook (no GPU): tile `tile` of the pyrDown of a 2-D uint8 image as k_pyrdown_tiled stages it -> (tiles of the layer,
    staged [35, 128] uint8, entry dict); tile=None only counts the tiles"""
    image = _c(image, np.uint8)
    sh, sw = image.shape
    if tile is None:
        nt = lib().fd_debug_pyrdown_stage(None, sw, sh, 0, None, None)
        if nt < 1:
            raise FdError(1, "fd_debug_pyrdown_stage: no such tile")
        return nt
    staged, entry = np.zeros((35, 128), np.uint8), np.zeros(8, np.int32)
    nt = lib().fd_debug_pyrdown_stage(_ptr(image), sw, sh, tile, _ptr(staged), _ptr(entry))
    if nt < 1:
        raise FdError(1, "fd_debug_pyrdown_stage: no such tile")
    return nt, staged, dict(zip(("src_off", "dst_off", "sw", "sh", "dx0", "dy0", "nx", "ny"), entry.tolist()))


def resize_stage(image, dw0, dh0, tile):
    """Test hook (no GPU): tile `tile` of the fused resize (2-D uint8 image -> dw0 x dh0) + pyrDown as k_resize_down stages it ->
    (tiles of the layer, staged [36, 512] uint8, read offsets [35, 127] int32, entry dict); tile=None only counts the tiles"""
    image = _c(image, np.uint8)
    sh, sw = image.shape
    if tile is None:
        nt = lib().fd_debug_resize_stage(None, sw, sh, dw0, dh0, 0, None, None, None)
        if nt < 1:
            raise FdError(1, "fd_debug_resize_stage: not a layer of k_resize_down")
        return nt
    staged, off, entry = np.zeros((36, 512), np.uint8), np.zeros((35, 127), np.int32), np.zeros(8, np.int32)
    nt = lib().fd_debug_resize_stage(_ptr(image), sw, sh, dw0, dh0, tile, _ptr(staged), _ptr(off), _ptr(entry))
    if nt < 1:
        raise FdError(1, "fd_debug_resize_stage: no such tile")
    return nt, staged, off, dict(zip(("X0", "ncol", "tx", "ty", "gx0", "gy0", "dw1", "dh1"), entry.tolist()))


def wvb_rect_sums(model, patches_eq):
    """Test hook (no GPU): rect sums of every used level from the dense stage-B tables -> ([n, ncols] int32, phase boundaries),
    or None when the model has no dense stage B."""
    s, keep = _wvm_struct(model, fd_wvm_model)
    patches_eq = _c(patches_eq, np.uint8)
    n = patches_eq.shape[0]
    gen = np.zeros(5, np.int32)
    ncols = lib().fd_debug_wvb_rect_sums(C.byref(s), None, 0, None, _ptr(gen))
    if ncols < 0:
        return None
    out = np.empty((n, ncols), np.int32)
    lib().fd_debug_wvb_rect_sums(C.byref(s), _ptr(patches_eq), n, _ptr(out), None)
    return out, [int(g) for g in gen if g >= 0]


def wvm_eval(ctx, wvm, patches_eq):
    """WvmClassifier::computeHyperplaneDistance on already equalised patches [n, h, w] u8"""
    patches_eq = _c(patches_eq, np.uint8)
    n = patches_eq.shape[0]
    lv = np.empty(n, np.int32)
    sc = np.empty(n, np.float32)
    ctx.check(lib().fd_wvm_eval_batch(ctx.h, wvm.h, _ptr(patches_eq), n, _ptr(lv), _ptr(sc)))
    return lv, sc


class Svm:
    def __init__(self, ctx, model):
        self.ctx = ctx
        self.model = model
        dtype = np.uint8 if model["dtype"] == FD_DTYPE_U8 else np.float32
        sv = _c(model["sv"], dtype)
        coeff = _c(model["coeff"], np.float32)
        s = fd_svm_model()
        s.kernel = int(model["kernel"])
        s.p0, s.p1, s.p2 = float(model.get("p0", 0)), float(model.get("p1", 0)), float(model.get("p2", 0))
        s.num_sv, s.dim = sv.shape
        s.dtype = int(model["dtype"])
        s.support_vectors = sv.ctypes.data
        s.coefficients = coeff.ctypes.data_as(C.POINTER(C.c_float))
        s.bias, s.threshold = float(model["bias"]), float(model.get("threshold", 0.0))
        s.logistic_a, s.logistic_b = float(model.get("logistic_a", 0.00556)), float(model.get("logistic_b", -2.95))
        self.h = C.c_void_p()
        ctx.check(lib().fd_svm_create(ctx.h, C.byref(s), C.byref(self.h)))
        self.dim = s.dim
        self.np_dtype = dtype

    @classmethod
    def from_handle(cls, ctx, handle, dim):
        """an f32 model the library created itself (fd_kernel_svm_train_model); the object owns the handle"""
        self = cls.__new__(cls)
        self.ctx, self.model, self.h, self.dim, self.np_dtype = ctx, None, handle, dim, np.float32
        return self

    def distance(self, feats):
        feats = _c(feats, self.np_dtype).reshape(-1, self.dim)
        out = np.empty(feats.shape[0], np.float64)
        self.ctx.check(lib().fd_svm_distance_batch(self.ctx.h, self.h, _ptr(feats), feats.shape[0], _ptr(out)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().fd_svm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):   # a handle nobody holds any more gives its device memory back (hipFree waits for the device)
        try:
            self.close()
        except Exception:
            pass


def hog_params(pw=20, ph=20, sx=2, sy=2, bins=9, cell=5, block=2, signed_and_unsigned=False):
    return fd_hog_params(pw, ph, sx, sy, bins, cell, block, int(signed_and_unsigned))


def detect_wvm(ctx, pyr, wvm, sx=1, sy=1, roi=None, want_all=False, cap=1 << 20):
    n = pyr.window_count(wvm.model["filter_w"], wvm.model["filter_h"], sx, sy, roi)
    out = np.zeros(min(cap, max(n, 1)), DET_DTYPE)
    lv = np.empty(n, np.int32) if want_all else None
    sc = np.empty(n, np.float32) if want_all else None
    cnt = C.c_int64()
    r = _c(roi, np.int32) if roi is not None else None
    ctx.check(lib().fd_detect_wvm(ctx.h, pyr.h, wvm.h, sx, sy, _ptr(r), _ptr(out), out.shape[0], C.byref(cnt), _ptr(lv), _ptr(sc)))
    return out[:cnt.value], lv, sc


def detect_five_stage(ctx, pyr, wvm, svm, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1, roi=None, cap=4096):
    out = np.zeros(cap, DET_DTYPE)
    cnt = C.c_int()
    stages = np.zeros(4, np.int32)
    r = _c(roi, np.int32) if roi is not None else None
    ctx.check(lib().fd_detect_five_stage(ctx.h, pyr.h, wvm.h, svm.h, oe_dist, oe_ratio, sx, sy, _ptr(r), _ptr(out), cap,
                                         C.byref(cnt), _ptr(stages)))
    return out[:cnt.value], stages


class FiveStageImage:
    """fd_detect_five_stage_image with preallocated result buffers: Detector::detect(image) for one frame after the other (the output
    arrays are reused: copy what must outlive the next call)"""

    def __init__(self, ctx, pyr, wvm, svm, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1, cap=4096):
        self.ctx, self.pyr, self.wvm, self.svm = ctx, pyr, wvm, svm
        self.args = (oe_dist, oe_ratio, sx, sy)
        self.cap = cap
        self.out = np.zeros(cap, DET_DTYPE)
        self.cnt = C.c_int()
        self.stages = np.zeros(4, np.int32)
        self._fn = lib().fd_detect_five_stage_image
        self._outp, self._stp, self._cntp = _ptr(self.out), _ptr(self.stages), C.byref(self.cnt)

    def detect_device(self, dev_ptr, w, h, ch):
        a = self.args
        self.ctx.check(self._fn(self.ctx.h, self.pyr.h, self.wvm.h, self.svm.h, C.c_void_p(dev_ptr), w, h, ch, 1, a[0], a[1], a[2], a[3], None,
                                self._outp, self.cap, self._cntp, self._stp))
        return self.out[:self.cnt.value], self.stages

    def detect(self, image):
        image = np.ascontiguousarray(image, np.uint8)
        ch = 1 if image.ndim == 2 else image.shape[2]
        a = self.args
        self.ctx.check(self._fn(self.ctx.h, self.pyr.h, self.wvm.h, self.svm.h, _ptr(image), image.shape[1], image.shape[0], ch, 0, a[0], a[1], a[2], a[3],
                                None, self._outp, self.cap, self._cntp, self._stp))
        return self.out[:self.cnt.value], self.stages


def detect_five_stage_frames(ctx, pyr, wvm, svm, nframes, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1, roi=None, cap=256):
    """fd_detect_five_stage_frames on a multi-frame pyramid: [(detections, stage_counts)] per frame"""
    held = int(getattr(pyr, "nframes", 1) or 1)   # the C side writes one entry per frame OF THE PYRAMID (see FiveStageFrames)
    if nframes != held:
        raise ValueError("detect_five_stage_frames: nframes=%d but the pyramid holds %d frames" % (nframes, held))
    out = np.empty((nframes, cap), DET_DTYPE)
    counts = np.zeros(nframes, np.int32)
    stages = np.zeros((nframes, 4), np.int32)
    r = _c(roi, np.int32) if roi is not None else None
    ctx.check(lib().fd_detect_five_stage_frames(ctx.h, pyr.h, wvm.h, svm.h, oe_dist, oe_ratio, sx, sy, _ptr(r), _ptr(out), cap, _ptr(counts), _ptr(stages)))
    return [(out[f, :counts[f]].copy(), stages[f].copy()) for f in range(nframes)]


class FiveStageFrames:
    """fd_detect_five_stage_frames_begin / _end: the cascade run of all frames of a multi-frame pyramid is queued by the constructor,
    end() runs the host stages + the SVM launch and returns [(detections, stage_counts)] per frame"""

    def __init__(self, ctx, pyr, wvm, svm, nframes, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1, roi=None, cap=256):
        # _end writes one entry per frame OF THE PYRAMID into counts / stages / out: the buffers are sized from the pyramid, and a
        # caller who states another number is told so instead of getting a heap overflow
        held = int(getattr(pyr, "nframes", 1) or 1)
        if nframes != held:
            raise ValueError("FiveStageFrames: nframes=%d but the pyramid holds %d frames" % (nframes, held))
        self.ctx, self.nframes, self.cap = ctx, held, cap
        self._keep = (pyr, wvm, svm)
        self.ticket = C.c_void_p()
        r = _c(roi, np.int32) if roi is not None else None
        ctx.check(lib().fd_detect_five_stage_frames_begin(ctx.h, pyr.h, wvm.h, svm.h, oe_dist, oe_ratio, sx, sy, _ptr(r), C.byref(self.ticket)))

    def end(self):
        out = np.empty((self.nframes, self.cap), DET_DTYPE)
        counts = np.zeros(self.nframes, np.int32)
        stages = np.zeros((self.nframes, 4), np.int32)
        t, self.ticket = self.ticket, C.c_void_p()
        self.ctx.check(lib().fd_detect_five_stage_frames_end(self.ctx.h, t, _ptr(out), self.cap, _ptr(counts), _ptr(stages)))
        return [(out[f, :counts[f]].copy(), stages[f].copy()) for f in range(self.nframes)]

    def close(self):
        """drops a ticket that was never ended (its host task is waited for, results are discarded)"""
        if getattr(self, "ticket", None):
            t, self.ticket = self.ticket, C.c_void_p()
            lib().fd_detect_five_stage_frames_end(self.ctx.h, t, None, 0, None, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def end_flat(self):
        """as end(), but one array for the call: (detections of all frames in frame order, frame index of each, stage_counts[frames, 4])"""
        out = np.empty((self.nframes, self.cap), DET_DTYPE)
        counts = np.zeros(self.nframes, np.int32)
        stages = np.zeros((self.nframes, 4), np.int32)
        t, self.ticket = self.ticket, C.c_void_p()
        self.ctx.check(lib().fd_detect_five_stage_frames_end(self.ctx.h, t, _ptr(out), self.cap, _ptr(counts), _ptr(stages)))
        mask = np.arange(self.cap)[None, :] < counts[:, None]
        return out[mask], np.repeat(np.arange(self.nframes), counts), stages


def _five_stage_jobs(detectors, oe_dist, oe_ratio, sx, sy, cap, device_frames, host_frames=None):
    n = len(detectors)
    jobs = (fd_five_stage_job * n)()
    outs = [np.empty(cap, DET_DTYPE) for _ in range(n)]   # the library fills the first `count` records
    for j, (pyr, wvm, svm), o in zip(jobs, detectors, outs):
        j.pyramid, j.wvm, j.svm = pyr.h, wvm.h, svm.h
        j.oe_dist, j.oe_ratio, j.step_x, j.step_y, j.roi = oe_dist, oe_ratio, sx, sy, None
        j.out, j.cap = o.ctypes.data, cap
    if device_frames is not None:
        for j, (ptr, w, h, ch) in zip(jobs, device_frames):
            j.image, j.image_w, j.image_h, j.image_channels, j.image_is_device = ptr, w, h, ch, 1
    if host_frames is not None:
        imgs = [np.ascontiguousarray(im, np.uint8) for im in host_frames]
        jobs._images = imgs   # the library reads them until the batch has ended: they live as long as the jobs
        for j, im in zip(jobs, imgs):
            j.image, j.image_w, j.image_h, j.image_channels, j.image_is_device = im.ctypes.data, im.shape[1], im.shape[0], 1 if im.ndim == 2 else im.shape[2], 0
    return jobs, outs


def _five_stage_results(jobs, outs):
    return [(o[:j.count].copy(), np.array(list(j.stage_counts), np.int32)) for j, o in zip(jobs, outs)]


def detect_five_stage_batch(ctx, detectors, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1, cap=4096, device_frames=None, host_frames=None):
    """detectors: list of (pyramid, wvm, svm); returns [(detections, stage_counts)] in the same order.
    device_frames: optional list of (device pointer, w, h, channels) per detector: the pyramid is updated inside the call;
    host_frames: the same with host images (numpy arrays)"""
    jobs, outs = _five_stage_jobs(detectors, oe_dist, oe_ratio, sx, sy, cap, device_frames, host_frames)
    ctx.check(lib().fd_detect_five_stage_batch(ctx.h, jobs, len(detectors)))
    return _five_stage_results(jobs, outs)


class FiveStageBatch:
    """fd_five_stage_batch_begin / _end: begin queues the pyramid updates and cascades of all detectors and returns;
    end() runs the host stages and returns [(detections, stage_counts)].  Batches in flight must use different handles."""
    def __init__(self, ctx, detectors, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1, cap=4096, device_frames=None, host_frames=None):
        self.ctx = ctx
        self._keep = list(detectors)   # the handles in the jobs stay alive while the batch is in flight
        self.jobs, self.outs = _five_stage_jobs(detectors, oe_dist, oe_ratio, sx, sy, cap, device_frames, host_frames)
        self.ticket = C.c_void_p()
        ctx.check(lib().fd_five_stage_batch_begin(ctx.h, self.jobs, len(detectors), C.byref(self.ticket)))

    def end(self):
        t, self.ticket = self.ticket, None
        self.ctx.check(lib().fd_five_stage_batch_end(self.ctx.h, t))
        return _five_stage_results(self.jobs, self.outs)

    def __del__(self):   # the library's threads write to self.jobs / self.outs until the batch has been ended
        t, self.ticket = getattr(self, "ticket", None), None
        if t:
            try:
                lib().fd_five_stage_batch_end(self.ctx.h, t)
            except Exception:
                pass


def fhog(ctx, gray=None, pyramid=None, layer=0, cell_size=8, unsigned_bins=9, interpolate_bins=False, interpolate_cells=True, alpha=0.2):
    """FhogFilter::applyTo on a host gray (h, w) / BGR (h, w, 3) image or on a layer of a gray pyramid:
    (rows, cols, 3 * unsigned_bins + 4) float32"""
    fp = fd_fhog_params(cell_size, unsigned_bins, int(interpolate_bins), int(interpolate_cells), alpha)
    if gray is not None:
        gray = _c(gray, np.uint8)
        h, w = gray.shape[:2]
    else:
        info = pyramid.layers()[layer]
        h, w = info["h"], info["w"]
    cs = max(cell_size, 1)   # invalid parameters are reported by the library
    out = np.zeros((h // cs, w // cs, max(3 * unsigned_bins + 4, 0)), np.float32)
    if gray is not None:
        ch = 1 if gray.ndim == 2 else gray.shape[2]
        if ch == 1:
            ctx.check(lib().fd_fhog_image(ctx.h, _ptr(gray), w, h, C.byref(fp), _ptr(out)))
        else:
            ctx.check(lib().fd_fhog_image_channels(ctx.h, _ptr(gray), w, h, ch, C.byref(fp), _ptr(out)))
    else:
        ctx.check(lib().fd_pyramid_fhog_layer(ctx.h, pyramid.h, layer, C.byref(fp), _ptr(out)))
    return out


def cehog_params(cell_size=8, bin_count=18, signed_gradients=True, unsigned_gradients=True, interpolate_bins=False, interpolate_cells=True,
                 alpha=0.2):
    """fd_cehog_params with CompleteExtendedHogFilter's defaults"""
    return fd_cehog_params(cell_size, bin_count, int(signed_gradients), int(unsigned_gradients), int(interpolate_bins), int(interpolate_cells),
                           alpha)


def cehog_size(fp, width, height):
    """fd_cehog_size (host only): (rows, cols, channels); FdError for invalid parameters"""
    r, c, d = C.c_int(), C.c_int(), C.c_int()
    rc = lib().fd_cehog_size(C.byref(fp), width, height, C.byref(r), C.byref(c), C.byref(d))
    if rc != FD_OK:
        raise FdError(rc, "fd_cehog_size: invalid CompleteExtendedHogFilter parameters or image size")
    return r.value, c.value, d.value


def cehog_gradient_lut(fp):
    """fd_cehog_gradient_lut (host only): index1, index2 (int32), weight1, weight2 (float32), each (512, 512) indexed [dx + 256, dy + 256]"""
    i1, i2 = np.zeros((512, 512), np.int32), np.zeros((512, 512), np.int32)
    w1, w2 = np.zeros((512, 512), np.float32), np.zeros((512, 512), np.float32)
    rc = lib().fd_cehog_gradient_lut(C.byref(fp), _ptr(i1), _ptr(i2), _ptr(w1), _ptr(w2))
    if rc != FD_OK:
        raise FdError(rc, "fd_cehog_gradient_lut: invalid CompleteExtendedHogFilter parameters")
    return i1, i2, w1, w2


def cehog_image(ctx, fp, gray=None, pyramid=None, layer=0):
    """CompleteExtendedHogFilter::applyTo on a host gray (h, w) image or on a layer of a gray pyramid: (rows, cols, channels) float32"""
    if gray is not None:
        gray = _c(gray, np.uint8)
        h, w = gray.shape[:2]
    else:
        info = pyramid.layers()[layer]
        h, w = info["h"], info["w"]
    cs = max(fp.cell_size, 1)   # invalid parameters are reported by the library
    both = fp.signed_gradients and fp.unsigned_gradients
    out = np.zeros((h // cs, w // cs, max(fp.bin_count + (fp.bin_count // 2 if both else 0) + 4, 0)), np.float32)
    if gray is not None:
        ctx.check(lib().fd_cehog_image(ctx.h, _ptr(gray), w, h, C.byref(fp), _ptr(out)))
    else:
        ctx.check(lib().fd_pyramid_cehog_layer(ctx.h, pyramid.h, layer, C.byref(fp), _ptr(out)))
    return out


def ehog_patch_params(pw, ph, bins=9, cell_w=5, cell_h=0, interpolate=False, signed_and_unsigned=False, alpha=0.2):
    return fd_ehog_patch_params(pw, ph, bins, cell_w, cell_h, int(interpolate), int(signed_and_unsigned), alpha)


def ehog_feature_length(ep, channels):
    return lib().fd_ehog_feature_length(C.byref(ep), channels)


def ehog_patch_batch(ctx, bin_patches, ep):
    """ExtendedHogFilter on bin_patches [n, ph, pw, channels] u8 (or [n, ph, pw]): [n, rows, cols, bins (+ bins / 2) + 4] f32"""
    b = _c(bin_patches, np.uint8)
    ch = b.shape[3] if b.ndim == 4 else 1
    F = lib().fd_ehog_feature_length(C.byref(ep), ch)
    if F < 0:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "invalid extended HOG parameters")
    D = ep.bins + (ep.bins // 2 if ep.signed_and_unsigned else 0) + 4
    cells = F // D
    out = np.zeros((b.shape[0], F), np.float32)
    ctx.check(lib().fd_ehog_patch_batch(ctx.h, _ptr(b), b.shape[0], ch, C.byref(ep), _ptr(out)))
    return out.reshape(b.shape[0], cells, D)


# fd_ehog_layer: one layer of an extended-HOG tracker
EHOG_LAYER_DTYPE = np.dtype([("index", "<i4"), ("width", "<i4"), ("height", "<i4"), ("rows", "<i4"), ("cols", "<i4"), ("reserved", "<i4"),
                             ("scale", "<f8")], align=True)


def ehog_tracker_params(fp, cell_cols, cell_rows, octave_layers, min_width, max_width):
    return fd_ehog_tracker_params(fp, cell_cols, cell_rows, octave_layers, min_width, max_width)


def ehog_tracker_plan_layers(prm, width, height):
    """fd_ehog_tracker_plan_layers (host only): the layers of a tracker on a width x height image as an EHOG_LAYER_DTYPE array;
    FdError (FD_ERR_RUNTIME) when fewer than two layers remain"""
    out = np.zeros(256, EHOG_LAYER_DTYPE)
    n = C.c_int()
    rc = lib().fd_ehog_tracker_plan_layers(C.byref(prm), width, height, _ptr(out), len(out), C.byref(n))
    if rc != FD_OK:
        raise FdError(rc, "fd_ehog_tracker_plan_layers: %d layers" % n.value)
    return out[:n.value].copy()


def ehog_tracker_patch_lds_bytes(prm):
    return lib().fd_ehog_tracker_patch_lds_bytes(C.byref(prm))


class EhogTracker:
    """fd_ehog_tracker: feature pyramid, heat pyramid, samples, patches, peak and maxima of ExtendedHogBasedMeasurementModel"""

    def __init__(self, ctx, prm):
        self.ctx = ctx
        self.prm = prm
        both = prm.filter.signed_gradients and prm.filter.unsigned_gradients
        self.channels = prm.filter.bin_count + (prm.filter.bin_count // 2 if both else 0) + 4
        self.h = C.c_void_p()
        ctx.check(lib().fd_ehog_tracker_create(ctx.h, C.byref(prm), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().fd_ehog_tracker_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, image):
        image = _c(image, np.uint8)
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        self.ctx.check(lib().fd_ehog_tracker_update(self.ctx.h, self.h, _ptr(image), w, h, ch, 0))

    def update_device(self, dev_ptr, w, h, ch):
        self.ctx.check(lib().fd_ehog_tracker_update(self.ctx.h, self.h, C.c_void_p(dev_ptr), w, h, ch, 1))

    def set_svm(self, weights, bias):
        weights = _c(weights, np.float32)
        if weights.size != self.prm.cell_rows * self.prm.cell_cols * self.channels:
            raise ValueError("weights must be [cell_rows][cell_cols][channels]")
        self.ctx.check(lib().fd_ehog_tracker_set_svm(self.ctx.h, self.h, _ptr(weights), bias))

    def train_svm(self, x, n_pos, **kw):
        """fd_ehog_tracker_train_svm on n_pos positive rows followed by the negative rows of x; keywords as svm_train_params.
        Returns the training info (a dict)."""
        x = _c(x, np.float32).reshape(len(x), -1)
        if x.shape[1] != self.prm.cell_rows * self.prm.cell_cols * self.channels:
            raise ValueError("examples must be [cell_rows][cell_cols][channels]")
        prm, info = svm_train_params(**kw), fd_svm_train_info()
        self.ctx.check(lib().fd_ehog_tracker_train_svm(self.ctx.h, self.h, _ptr(x), n_pos, len(x) - n_pos, C.byref(prm), C.byref(info)))
        return _svm_info(info)

    def get_svm(self):
        """(weights float32 (cell_rows, cell_cols, channels), bias) of the installed model"""
        w, bias = np.zeros((self.prm.cell_rows, self.prm.cell_cols, self.channels), np.float32), C.c_float()
        self.ctx.check(lib().fd_ehog_tracker_get_svm(self.ctx.h, self.h, _ptr(w), C.byref(bias)))
        return w, bias.value

    def layers(self):
        out = np.zeros(256, EHOG_LAYER_DTYPE)
        n = C.c_int()
        self.ctx.check(lib().fd_ehog_tracker_get_layers(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def feature_layer(self, layer):
        ls = self.layers()   # a layer that does not exist is reported by the library
        shape = (ls[layer]["rows"], ls[layer]["cols"], self.channels) if 0 <= layer < len(ls) else (1, 1, self.channels)
        out = np.zeros(shape, np.float32)
        self.ctx.check(lib().fd_ehog_tracker_feature_layer(self.ctx.h, self.h, layer, _ptr(out)))
        return out

    def heat_layer(self, layer):
        n = len(self.layers())
        shape = (self.layers()[layer]["rows"], self.layers()[layer]["cols"]) if 0 <= layer < n else (1, 1)
        out = np.zeros(shape, np.float32)
        self.ctx.check(lib().fd_ehog_tracker_heat_layer(self.ctx.h, self.h, layer, _ptr(out)))
        return out

    def _samples(self, xywh):
        xywh = _c(np.asarray(xywh, np.int32).reshape(-1, 4), np.int32)
        return xywh, np.zeros(len(xywh), np.uint8)

    def evaluate_samples(self, xywh):
        """(valid uint8 (n,), score float32 (n,)) of samples {x, y, width, height}"""
        xywh, valid = self._samples(xywh)
        score = np.zeros(len(xywh), np.float32)
        self.ctx.check(lib().fd_ehog_tracker_evaluate_samples(self.ctx.h, self.h, len(xywh), _ptr(xywh), _ptr(valid), _ptr(score)))
        return valid, score

    def extract_cells(self, xywh):
        """(valid, features float32 (n, cell_rows, cell_cols, channels))"""
        xywh, valid = self._samples(xywh)
        feat = np.zeros((len(xywh), self.prm.cell_rows, self.prm.cell_cols, self.channels), np.float32)
        self.ctx.check(lib().fd_ehog_tracker_extract_cells(self.ctx.h, self.h, len(xywh), _ptr(xywh), _ptr(valid), _ptr(feat)))
        return valid, feat

    def extract_patches(self, xywh, want_score=False):
        """(valid, features) or (valid, features, score float64 (n,))"""
        xywh, valid = self._samples(xywh)
        feat = np.zeros((len(xywh), self.prm.cell_rows, self.prm.cell_cols, self.channels), np.float32)
        score = np.zeros(len(xywh), np.float64) if want_score else None
        self.ctx.check(lib().fd_ehog_tracker_extract_patches(self.ctx.h, self.h, len(xywh), _ptr(xywh), _ptr(valid), _ptr(feat), _ptr(score)))
        return (valid, feat, score) if want_score else (valid, feat)

    def heat_peak(self):
        """(found, BOX_DTYPE record): getHeatPeak"""
        box = np.zeros(1, BOX_DTYPE)
        found = C.c_int()
        self.ctx.check(lib().fd_ehog_tracker_heat_peak(self.ctx.h, self.h, _ptr(box), C.byref(found)))
        return bool(found.value), box[0]

    def heat_maxima(self, threshold, cap=4096):
        """BOX_DTYPE array of the local maxima above threshold, scan order; FdError FD_ERR_CAPACITY (with .count) when cap is too small"""
        out = np.zeros(max(cap, 1), BOX_DTYPE)
        n = C.c_int()
        rc = lib().fd_ehog_tracker_heat_maxima(self.ctx.h, self.h, threshold, _ptr(out), cap, C.byref(n))
        if rc != FD_OK:
            e = FdError(rc, lib().fd_last_error(self.ctx.h).decode())
            e.count = n.value
            raise e
        return out[:n.value].copy()


FD_PARTICLES_MAX = 8192
FD_PARTICLES_TARGET_LOST, FD_PARTICLES_SLIDING_WINDOW, FD_PARTICLES_ALL_TARGETS = 0, 1, 2
# the fields of a generation of particles, in the order of fd_particles_arrays
PARTICLE_FIELDS = (("x", np.int32), ("y", np.int32), ("size", np.int32), ("vx", np.int32), ("vy", np.int32), ("vsize", np.float32),
                   ("weight", np.float64), ("score", np.float64), ("target", np.uint8), ("cluster_id", np.int32))


class Particles:
    """fd_particles: the particle set of the Condensation tracker resident on the device, bound to one EhogTracker.  A generation is a
    dict of arrays keyed like PARTICLE_FIELDS."""

    def __init__(self, ctx, tracker, capacity):
        self.ctx = ctx
        self.tracker = tracker   # must outlive the set; None: an unbound set (Particles.unbound)
        self.h = C.c_void_p()
        if tracker is None:
            ctx.check(lib().fd_particles_create_unbound(ctx.h, capacity, C.byref(self.h)))
        else:
            ctx.check(lib().fd_particles_create(ctx.h, tracker.h, capacity, C.byref(self.h)))

    @classmethod
    def unbound(cls, ctx, capacity):
        """fd_particles_create_unbound: a set without a tracker, for evaluate_integral / weigh_classifier"""
        return cls(ctx, None, capacity)

    def close(self):
        if self.h:
            lib().fd_particles_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def capacity(self):
        return lib().fd_particles_capacity(self.h)

    def set(self, x, y, size, vx=None, vy=None, vsize=None, weight=None, score=None, target=None, cluster_id=None):
        """fills the current generation; defaults: velocity 0, size factor 1, weight 1, score 0, no target flag, cluster ids 0"""
        n = len(x)
        given = dict(x=x, y=y, size=size, vx=vx, vy=vy, vsize=vsize, weight=weight, score=score, target=target, cluster_id=cluster_id)
        default = dict(vx=0, vy=0, vsize=1, weight=1, score=0, target=0, cluster_id=0)
        keep = [_c(np.full(n, default[name]) if given[name] is None else given[name], dtype) for name, dtype in PARTICLE_FIELDS]
        if any(len(a) != n for a in keep):
            raise ValueError("the fields of a generation have one length")
        arrays = fd_particles_arrays(*[_ptr(a) for a in keep])
        self.ctx.check(lib().fd_particles_set(self.ctx.h, self.h, n, C.byref(arrays)))

    def get(self):
        """the current generation as a dict of arrays"""
        keep = {name: np.zeros(self.capacity, dtype) for name, dtype in PARTICLE_FIELDS}
        arrays = fd_particles_arrays(*[_ptr(keep[name]) for name, _ in PARTICLE_FIELDS])
        n = C.c_int()
        self.ctx.check(lib().fd_particles_get(self.ctx.h, self.h, self.capacity, C.byref(n), C.byref(arrays)))
        return {name: a[:n.value].copy() for name, a in keep.items()}

    def trace(self, windows=True):
        """(source int32 (n,), windows int32 (n, 4) {layer, bx, by, valid} or None, valid uint8 (n,)) of the last sample / evaluate"""
        source, valid = np.zeros(self.capacity, np.int32), np.zeros(self.capacity, np.uint8)
        win = np.zeros((self.capacity, 4), np.int32) if windows else None
        self.ctx.check(lib().fd_particles_get_trace(self.ctx.h, self.h, _ptr(source), _ptr(win), _ptr(valid)))
        n = len(self)
        return source[:n].copy(), (win[:n].copy() if windows else None), valid[:n].copy()

    def __len__(self):
        n = C.c_int()
        rc = lib().fd_particles_get(self.ctx.h, self.h, FD_PARTICLES_MAX, C.byref(n), None)
        self.ctx.check(rc)
        return n.value

    def sample(self, count, n_resampled, u, diffusion, fresh, first_fresh_cluster_id):
        """fd_particles_sample: diffusion float64 (n_resampled, 3) {dx, dy, size factor}, fresh int32 (count - n_resampled, 3) {x, y, size}"""
        diffusion = _c(np.asarray(diffusion, np.float64).reshape(-1, 3), np.float64)
        fresh = _c(np.asarray(fresh, np.int32).reshape(-1, 3), np.int32)
        if len(diffusion) < n_resampled or len(fresh) < count - n_resampled:
            raise ValueError("too few draws")
        self.ctx.check(lib().fd_particles_sample(self.ctx.h, self.h, count, n_resampled, u, _ptr(diffusion), _ptr(fresh), first_fresh_cluster_id))

    def evaluate(self, use_patches, aspect_ratio):
        self.ctx.check(lib().fd_particles_evaluate(self.ctx.h, self.h, int(use_patches), aspect_ratio))

    def weigh(self, logistic_a, logistic_b, svm_threshold, mode, rejection_threshold):
        self.ctx.check(lib().fd_particles_weigh(self.ctx.h, self.h, logistic_a, logistic_b, svm_threshold, mode, rejection_threshold))

    def _state(self, rc, info):
        out = {name: getattr(info, name) for name, _ in fd_particles_info._fields_}
        if rc != FD_OK:
            e = FdError(rc, lib().fd_last_error(self.ctx.h).decode())
            e.info = out
            raise e
        return out

    def state(self):
        """fd_particles_state: the info as a dict; FdError (with .info) when a weight is negative or not finite"""
        info = fd_particles_info()
        return self._state(lib().fd_particles_state(self.ctx.h, self.h, C.byref(info)), info)

    def evaluate_integral(self, integral, svm, aspect_ratio, maps=(), haar=None, surf=None, hog=None):
        """fd_particles_evaluate_integral on an updated Integral: haar / surf / hog as Integral.svm_evaluate_samples takes them, maps a
        sequence of ("resize", factor, x_offset, y_offset) and ("integral",) from the outermost wrapper in"""
        kind, prm, _keep = _integral_kind(haar, surf, hog)
        chain = sample_maps(maps)
        self.ctx.check(lib().fd_particles_evaluate_integral(self.ctx.h, self.h, integral.h, kind, prm, svm.h, aspect_ratio, chain, len(chain)))

    def evaluate_pyramid(self, pyr, svm, aspect_ratio, maps=(), hist=None, ehog=None, patch=None):
        """fd_particles_evaluate_pyramid on an updated Pyramid: exactly one of hist (fd_hist_params), ehog (fd_ehog_patch_params) and patch
        (fd_patch_samples_params), as hist_svm_evaluate_samples / patch_svm_evaluate_samples take them; maps a sequence of ("resize",
        factor, x_offset, y_offset) from the outermost wrapper in"""
        given = [(FD_SAMPLES_HIST, hist), (FD_SAMPLES_EHOG, ehog), (FD_SAMPLES_PATCH, patch)]
        given = [(kind, prm) for kind, prm in given if prm is not None]
        if len(given) != 1:
            raise ValueError("exactly one of hist, ehog and patch")
        kind, prm = given[0]
        chain = sample_maps(maps)
        self.ctx.check(lib().fd_particles_evaluate_pyramid(self.ctx.h, self.h, pyr.h, kind, C.byref(prm), svm.h, aspect_ratio, chain, len(chain)))

    def weigh_classifier(self, logistic_a, logistic_b, threshold):
        self.ctx.check(lib().fd_particles_weigh_classifier(self.ctx.h, self.h, logistic_a, logistic_b, threshold))

    def evaluate_wvm_svm(self, pyr, wvm, svm, aspect_ratio, maps=()):
        """fd_particles_evaluate_wvm_svm on an updated gray Pyramid: the WVM cascade on every particle's window; maps as evaluate_pyramid"""
        chain = sample_maps(maps)
        self.ctx.check(lib().fd_particles_evaluate_wvm_svm(self.ctx.h, self.h, pyr.h, wvm.h, svm.h, aspect_ratio, chain, len(chain)))

    def weigh_wvm_svm(self, wvm, svm):
        """fd_particles_weigh_wvm_svm: the SVM on the up to 8 most probable WVM positives, then WvmSvmModel's targets and weights"""
        self.ctx.check(lib().fd_particles_weigh_wvm_svm(self.ctx.h, self.h, wvm.h, svm.h))

    def wvm_svm_trace(self):
        """fd_particles_get_wvm_svm_trace: (selected particle indices int32 (count,), most probable first, their SVM distances float64)"""
        count, index, distance = C.c_int(), np.zeros(8, np.int32), np.zeros(8, np.float64)
        self.ctx.check(lib().fd_particles_get_wvm_svm_trace(self.ctx.h, self.h, C.byref(count), _ptr(index), _ptr(distance)))
        return index[:count.value].copy(), distance[:count.value].copy()

    def sample_flow(self, flow, count, n_resampled, u, flow_diffusion, fallback_diffusion, fresh, first_fresh_cluster_id):
        """fd_particles_sample_flow: sample() with the motion `flow` holds on the device and a block of draws for either transition"""
        flow_diffusion = _c(np.asarray(flow_diffusion, np.float64).reshape(-1, 3), np.float64)
        fallback_diffusion = _c(np.asarray(fallback_diffusion, np.float64).reshape(-1, 3), np.float64)
        fresh = _c(np.asarray(fresh, np.int32).reshape(-1, 3), np.int32)
        if len(flow_diffusion) < n_resampled or len(fallback_diffusion) < n_resampled or len(fresh) < count - n_resampled:
            raise ValueError("too few draws")
        self.ctx.check(lib().fd_particles_sample_flow(self.ctx.h, self.h, flow.h, count, n_resampled, u, _ptr(flow_diffusion), _ptr(fallback_diffusion),
                                                      _ptr(fresh), first_fresh_cluster_id))

    def state_flow(self, flow):
        """fd_particles_state_flow: (info as state() gives it, the flow handle's motion as a dict) in one read-back"""
        info, motion = fd_particles_info(), fd_flow_motion_info()
        out = self._state(lib().fd_particles_state_flow(self.ctx.h, self.h, flow.h, C.byref(info), C.byref(motion)), info)
        return out, _motion_dict(motion)

    def state_negatives(self, params, flow=None):
        """fd_particles_state_negatives: (info as state() gives it, the flow handle's motion as a dict or None without a flow, the chosen
        negatives as a dict of arrays index, x, y, size (int32) and weight (float64) in the list order of
        PositionDependentMeasurementModel::adapt) in one read-back; params from negatives_params().  FdError carries .info."""
        info, motion, count = fd_particles_info(), fd_flow_motion_info(), C.c_int()
        records = (fd_particles_negative * FD_PARTICLES_NEGATIVES_MAX)()
        rc = lib().fd_particles_state_negatives(self.ctx.h, self.h, flow.h if flow is not None else None, C.byref(params), C.byref(info),
                                                C.byref(motion) if flow is not None else None, C.byref(count), records)
        try:
            out = self._state(rc, info)
        except FdError as e:
            e.count = count.value
            raise
        chosen = {name: np.array([getattr(records[k], name) for k in range(count.value)], np.float64 if name == "weight" else np.int32)
                  for name, _ in fd_particles_negative._fields_}
        return out, (_motion_dict(motion) if flow is not None else None), chosen

    def state_examples(self, params, source, aspect_ratio, maps=(), haar=None, surf=None, hog=None, hist=None, ehog=None, patch=None, flow=None,
                       row_capacity=None, channels=1):
        """fd_particles_state_examples_integral (source an updated Integral; haar / surf / hog as evaluate_integral takes them) or
        fd_particles_state_examples_pyramid (source an updated Pyramid; hist / ehog / patch as evaluate_pyramid takes them): (info as
        state() gives it, the flow handle's motion as a dict or None without a flow, the positive examples, the negative examples, rows)
        in one read-back.  params from examples_params(); maps the adaptive extractor's chain.  Each list is a dict of arrays index, x, y,
        size, valid (int32) and weight (float64) in SelfLearningMeasurementModel::adapt's order; rows is float32 (n_pos + n_neg, row
        length), the positives' rows first, zero where the record is not valid.  row_capacity (floats) defaults to what
        particles_examples_bounds reports for `channels`, the channel count of the pyramid's bin image (hist / ehog only: 2 with bin
        interpolation).  FdError carries .info and .counts."""
        family, kind, prm, _keep = _examples_kind(haar, surf, hog, hist, ehog, patch)
        chain = sample_maps(maps)
        info, motion, n_pos, n_neg, row_length = fd_particles_info(), fd_flow_motion_info(), C.c_int(), C.c_int(), C.c_int()
        pos, neg = (fd_particles_example * FD_PARTICLES_EXAMPLES_MAX)(), (fd_particles_example * FD_PARTICLES_EXAMPLES_MAX)()
        if row_capacity is None:
            row_capacity = 0
            length, capacity = C.c_int(), C.c_int()
            if lib().fd_particles_examples_bounds(family, kind, prm, int(channels), params.max_count, C.byref(length), C.byref(capacity)) == FD_OK:
                row_capacity = capacity.value   # otherwise the call itself refuses the parameters, with its message
        rows = np.zeros(max(int(row_capacity), 1), np.float32)
        call = lib().fd_particles_state_examples_integral if family == FD_EXAMPLES_INTEGRAL else lib().fd_particles_state_examples_pyramid
        rc = call(self.ctx.h, self.h, flow.h if flow is not None else None, source.h, kind, prm, aspect_ratio, chain, len(chain), C.byref(params),
                  C.byref(info), C.byref(motion) if flow is not None else None, C.byref(n_pos), pos, C.byref(n_neg), neg, _ptr(rows), int(row_capacity),
                  C.byref(row_length))
        try:
            out = self._state(rc, info)
        except FdError as e:
            e.counts = (n_pos.value, n_neg.value)
            raise

        def records(rec, count):
            return {name: np.array([getattr(rec[k], name) for k in range(count)], np.float64 if name == "weight" else np.int32)
                    for name, _ in fd_particles_example._fields_}
        total = n_pos.value + n_neg.value
        return (out, (_motion_dict(motion) if flow is not None else None), records(pos, n_pos.value), records(neg, n_neg.value),
                rows[:total * row_length.value].reshape(total, row_length.value).copy())


FD_PARTICLES_EXAMPLES_MAX = 32


def examples_params(positive_threshold, negative_threshold, max_count=10, require_window=False):
    """fd_particles_examples_params: SelfLearningMeasurementModel's thresholds, its 10 examples per side, and whether a candidate needs
    the valid flag of the generation's evaluate (the usable branch) or not (the bootstrap branch)"""
    return fd_particles_examples_params(float(positive_threshold), float(negative_threshold), int(max_count), int(require_window))


def particles_examples_select(weight, params, valid=None):
    """fd_particles_examples_select (host only): (positive indices, negative indices), int32, in list order"""
    weight = _c(np.asarray(weight, np.float64), np.float64)
    valid = None if valid is None else _c(np.asarray(valid, np.uint8), np.uint8)
    n_pos, n_neg = C.c_int(), C.c_int()
    pos, neg = np.zeros(FD_PARTICLES_EXAMPLES_MAX, np.int32), np.zeros(FD_PARTICLES_EXAMPLES_MAX, np.int32)
    rc = lib().fd_particles_examples_select(len(weight), _ptr(weight), _ptr(valid), C.byref(params), C.byref(n_pos), _ptr(pos), C.byref(n_neg), _ptr(neg))
    if rc != FD_OK:
        raise FdError(rc, "fd_particles_examples_select")
    return pos[:n_pos.value].copy(), neg[:n_neg.value].copy()


FD_EXAMPLES_INTEGRAL, FD_EXAMPLES_PYRAMID = 0, 1


def _examples_kind(haar=None, surf=None, hog=None, hist=None, ehog=None, patch=None):
    """(family, kind, pointer to the parameters, the object the pointer needs alive) of exactly one feature extractor"""
    pyramid = [(kind, prm) for kind, prm in ((FD_SAMPLES_HIST, hist), (FD_SAMPLES_EHOG, ehog), (FD_SAMPLES_PATCH, patch)) if prm is not None]
    if pyramid:
        if len(pyramid) != 1 or haar is not None or surf is not None or hog is not None:
            raise ValueError("exactly one of haar, surf, hog, hist, ehog and patch")
        return FD_EXAMPLES_PYRAMID, pyramid[0][0], C.byref(pyramid[0][1]), pyramid[0][1]
    return (FD_EXAMPLES_INTEGRAL,) + _integral_kind(haar, surf, hog)


def particles_examples_bounds(max_count, channels=1, **extractor):
    """fd_particles_examples_bounds (host only): (row length, row capacity) in floats; the extractor as state_examples takes it"""
    family, kind, prm, _keep = _examples_kind(**extractor)
    length, capacity = C.c_int(), C.c_int()
    rc = lib().fd_particles_examples_bounds(family, kind, prm, int(channels), int(max_count), C.byref(length), C.byref(capacity))
    if rc != FD_OK:
        raise FdError(rc, "fd_particles_examples_bounds")
    return length.value, capacity.value


FD_PARTICLES_NEGATIVES_MAX = 64


def negatives_params(max_count, offset_factor):
    """fd_particles_negatives_params as the host layer forms them from sampleAdditionalNegatives and negativeOffsetFactor: down_scale =
    1 - offset_factor and up_scale = 1 / down_scale in float"""
    with np.errstate(divide="ignore"):
        f = np.float32(offset_factor)
        down = np.float32(1) - f
        up = np.float32(1) / down
    return fd_particles_negatives_params(int(max_count), float(f), float(down), float(up))


def particles_negatives_bounds(params, x, y, size):
    """fd_particles_negatives_bounds (host only): int32 (6,) {xLow, xHigh, yLow, yHigh, sizeLow, sizeHigh} of the state {x, y, size}"""
    bounds = np.zeros(6, np.int32)
    rc = lib().fd_particles_negatives_bounds(C.byref(params), int(x), int(y), int(size), _ptr(bounds))
    if rc != FD_OK:
        raise FdError(rc, "fd_particles_negatives_bounds")
    return bounds


FD_SAMPLE_MAP_RESIZE, FD_SAMPLE_MAP_INTEGRAL, FD_SAMPLE_MAPS_MAX = 0, 1, 4
FD_FLOW_RESIDENT_MAX_POINTS = 1024


def sample_maps(maps):
    """an array of fd_sample_map from ("resize", factor[, x_offset[, y_offset]]) and ("integral",) entries, outer to inner"""
    chain = (fd_sample_map * len(maps))()
    for k, entry in enumerate(maps):
        if entry[0] == "resize":
            values = list(entry[1:]) + [0.0] * (4 - len(entry))
            chain[k] = fd_sample_map(FD_SAMPLE_MAP_RESIZE, float(values[0]), float(values[1]), float(values[2]))
        elif entry[0] == "integral":
            chain[k] = fd_sample_map(FD_SAMPLE_MAP_INTEGRAL, 0.0, 0.0, 0.0)
        else:
            chain[k] = fd_sample_map(int(entry[0]), 0.0, 0.0, 0.0)   # an unknown kind, for the library to refuse
    return chain


def sample_maps_apply(maps, samples):
    """fd_sample_maps_apply (host only): the mapped copy of samples int32 (n, 4) {x, y, width, height}"""
    s = _c(samples, np.int32).reshape(-1, 4).copy()
    chain = sample_maps(maps)
    rc = lib().fd_sample_maps_apply(chain, len(chain), len(s), _ptr(s))
    if rc != FD_OK:
        raise FdError(rc, "fd_sample_maps_apply")
    return s


def _motion_dict(m):
    return dict(ok=bool(m.ok), n_valid=m.n_valid, n_correct=m.n_correct, median_x=np.float32(m.median_x), median_y=np.float32(m.median_y),
                median_ratio=np.float32(m.median_ratio))


FD_FLOW_MAX_POINTS, FD_FLOW_MAX_LEVELS = 16384, 8
(FD_FLOW_EXIT_NONE, FD_FLOW_EXIT_SKIP_RANGE, FD_FLOW_EXIT_SKIP_EIGEN, FD_FLOW_EXIT_EPS, FD_FLOW_EXIT_OSCILLATION, FD_FLOW_EXIT_COUNT,
 FD_FLOW_EXIT_LEFT_RANGE) = range(7)


def flow_params(**kw):
    """fd_flow_params: fd_flow_default_params (15 x 15 window, max_level 2, 30 iterations, epsilon 0.01, min_eig_threshold 1e-4) with overrides"""
    p = fd_flow_params()
    lib().fd_flow_default_params(C.byref(p))
    for name, value in kw.items():
        if name not in dict(fd_flow_params._fields_):
            raise TypeError("fd_flow_params has no field %r" % name)
        setattr(p, name, value)
    return p


def flow_limits():
    """fd_flow_limits: (max points per call, smallest window side, largest window side)"""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    lib().fd_flow_limits(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def flow_grid(grid_w, grid_h, circle=True):
    """fd_flow_grid: OpticalFlowTransitionModel's template points, float32 (n, 2)"""
    n = C.c_int()
    out = np.zeros((max(grid_w, 0) * max(grid_h, 0), 2), np.float32)
    rc = lib().fd_flow_grid(grid_w, grid_h, int(bool(circle)), _ptr(out), len(out), C.byref(n))
    if rc != FD_OK:
        raise FdError(rc, "fd_flow_grid(%d, %d)" % (grid_w, grid_h))
    return out[:n.value].copy()


def flow_median(points, fwd, bwd, fstatus, bstatus):
    """fd_flow_median: dict(ok, n_valid, n_correct, median_x, median_y, median_ratio (np.float32 each), order int32 (n_valid,))"""
    points, fwd, bwd = (_c(np.asarray(a, np.float32).reshape(-1, 2), np.float32) for a in (points, fwd, bwd))
    fstatus, bstatus = _c(fstatus, np.uint8).ravel(), _c(bstatus, np.uint8).ravel()
    n = len(points)
    if not (len(fwd) == len(bwd) == len(fstatus) == len(bstatus) == n):
        raise ValueError("the arrays of the tracked points have one length")
    order = np.zeros(max(n, 1), np.int32)
    m = fd_flow_motion()
    m.order = order.ctypes.data
    rc = lib().fd_flow_median(_ptr(points), _ptr(fwd), _ptr(bwd), _ptr(fstatus), _ptr(bstatus), n, C.byref(m))
    if rc != FD_OK:
        raise FdError(rc, "fd_flow_median")
    return dict(ok=bool(m.ok), n_valid=m.n_valid, n_correct=m.n_correct, median_x=np.float32(m.median_x), median_y=np.float32(m.median_y),
                median_ratio=np.float32(m.median_ratio), order=order[:m.n_valid].copy())


class Flow:
    """fd_flow: the flow pyramids of the current and the previous frame (width x height) and pyramidal Lucas-Kanade between them"""

    def __init__(self, ctx, width, height, params=None, **kw):
        self.ctx = ctx
        self.width, self.height = width, height
        self.params = params if params is not None else flow_params(**kw)
        self.h = C.c_void_p()
        ctx.check(lib().fd_flow_create(ctx.h, width, height, C.byref(self.params), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().fd_flow_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def levels(self):
        return lib().fd_flow_levels(self.h)

    def update(self, image):
        """the next frame: a uint8 array (h, w) or (h, w, 3) BGR on the host, or a torch uint8 tensor of that shape on the device"""
        if hasattr(image, "data_ptr"):
            if str(image.dtype) != "torch.uint8" or image.stride(-1) != 1 or (image.dim() == 3 and image.stride(1) != image.shape[2]):
                raise ValueError("a device image is a uint8 tensor with dense rows")
            shape, ptr, stride, dev = tuple(image.shape), C.c_void_p(image.data_ptr()), int(image.stride(0)), 1
        else:
            image = _c(image, np.uint8)
            shape, ptr, stride, dev = image.shape, _ptr(image), int(image.strides[0]), 0
        ch = 1 if len(shape) == 2 else shape[2]
        if shape[:2] != (self.height, self.width):
            raise ValueError("the image is %s, the flow was created for %d x %d" % (shape, self.width, self.height))
        self.ctx.check(lib().fd_flow_update(self.ctx.h, self.h, ptr, ch, stride, dev))

    def track(self, points, backward=False, trace=False):
        """fd_flow_track: (out float32 (n, 2), status uint8 (n,)[, trace uint8 (n, FD_FLOW_MAX_LEVELS, 2) {steps, exit reason}])"""
        points = _c(np.asarray(points, np.float32).reshape(-1, 2), np.float32)
        n = len(points)
        out, status = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        tr = np.zeros((n, FD_FLOW_MAX_LEVELS, 2), np.uint8) if trace else None
        self.ctx.check(lib().fd_flow_track(self.ctx.h, self.h, int(bool(backward)), _ptr(points), n, _ptr(out), _ptr(status), _ptr(tr)))
        return (out, status, tr) if trace else (out, status)

    def track_fb(self, points):
        """fd_flow_track_fb: (fwd, bwd float32 (n, 2), fstatus, bstatus uint8 (n,))"""
        points = _c(np.asarray(points, np.float32).reshape(-1, 2), np.float32)
        n = len(points)
        fwd, bwd = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        fst, bst = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.ctx.check(lib().fd_flow_track_fb(self.ctx.h, self.h, _ptr(points), n, _ptr(fwd), _ptr(bwd), _ptr(fst), _ptr(bst)))
        return fwd, bwd, fst, bst

    def track_fb_resident(self, points):
        """fd_flow_track_fb_resident: queues both trackings and the median flow of the tracks; nothing comes back"""
        points = _c(np.asarray(points, np.float32).reshape(-1, 2), np.float32)
        self.ctx.check(lib().fd_flow_track_fb_resident(self.ctx.h, self.h, _ptr(points), len(points)))

    def get_tracks(self):
        """fd_flow_get_tracks: dict(fwd, bwd float32 (n, 2), fstatus, bstatus uint8 (n,), order int32 (n_valid,), n_valid, n_correct) of the
        last resident track"""
        cap = FD_FLOW_RESIDENT_MAX_POINTS
        fwd, bwd = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        fst, bst, order = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
        n, nv, nc = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(lib().fd_flow_get_tracks(self.ctx.h, self.h, cap, C.byref(n), _ptr(fwd), _ptr(bwd), _ptr(fst), _ptr(bst), _ptr(order), C.byref(nv),
                                                C.byref(nc)))
        k = n.value
        return dict(fwd=fwd[:k].copy(), bwd=bwd[:k].copy(), fstatus=fst[:k].copy(), bstatus=bst[:k].copy(), order=order[:nv.value].copy(),
                    n_valid=nv.value, n_correct=nc.value)

    def debug_motion(self, points, fwd, bwd, fstatus, bstatus):
        """fd_debug_flow_motion: the median-flow kernel on the caller's arrays -> dict(ok, n_valid, n_correct, median_x, median_y,
        median_ratio); the motion stays in the handle for Particles.sample_flow"""
        points, fwd, bwd = (_c(np.asarray(a, np.float32).reshape(-1, 2), np.float32) for a in (points, fwd, bwd))
        fstatus, bstatus = _c(fstatus, np.uint8).ravel(), _c(bstatus, np.uint8).ravel()
        n = len(points)
        if not (len(fwd) == len(bwd) == len(fstatus) == len(bstatus) == n):
            raise ValueError("the arrays of the tracked points have one length")
        m = fd_flow_motion_info()
        self.ctx.check(lib().fd_debug_flow_motion(self.ctx.h, self.h, _ptr(points), _ptr(fwd), _ptr(bwd), _ptr(fstatus), _ptr(bstatus), n, C.byref(m)))
        return _motion_dict(m)

    def level(self, level, previous=False):
        """fd_debug_flow_level: (image uint8 (ph, pw), derivatives int16 (ph, pw, 2)) of a stored level, border included"""
        w, h = C.c_int(), C.c_int()
        self.ctx.check(lib().fd_debug_flow_level(self.ctx.h, self.h, int(bool(previous)), level, None, None, C.byref(w), C.byref(h)))
        img, der = np.zeros((h.value, w.value), np.uint8), np.zeros((h.value, w.value, 2), np.int16)
        self.ctx.check(lib().fd_debug_flow_level(self.ctx.h, self.h, int(bool(previous)), level, _ptr(img), _ptr(der), C.byref(w), C.byref(h)))
        return img, der


def svm_train_params(C_=1.0, weight_pos=1.0, weight_neg=1.0, eps=0.0, max_iterations=0, launch_iterations=0, **kw):
    """fd_svm_train_params; the bound may be given as C_ or C"""
    return fd_svm_train_params(kw.pop("C", C_), weight_pos, weight_neg, eps, max_iterations, launch_iterations, **kw)


def _svm_info(info):
    return {name: getattr(info, name) for name, _ in fd_svm_train_info._fields_}


def _linear_svm_limits(name, n_pos, n_neg, d):
    """the two results of the host-only fd_linear_svm_train_limits / _large_limits (`name`)"""
    a, m = C.c_int(), C.c_int()
    rc = getattr(lib(), name)(n_pos, n_neg, d, C.byref(a), C.byref(m))
    if rc != FD_OK:
        raise FdError(rc, "%s: invalid sizes (%d, %d, %d)" % (name, n_pos, n_neg, d))
    return a.value, m.value


def _linear_svm_gram(fn, ctx, x, n_pos):
    x = _c(x, np.float32)
    n, d = x.shape
    q, qd = np.zeros((n, n), np.float32), np.zeros(n, np.float64)
    ctx.check(fn(ctx.h, _ptr(x), n_pos, n - n_pos, d, 0, _ptr(q), _ptr(qd)))
    return q, qd


def _linear_svm_train(fn, ctx, x, n_pos, kw):
    x = _c(x, np.float32)
    n, d = x.shape
    w, bias, alpha = np.zeros(d, np.float32), C.c_float(), np.zeros(n, np.float64)
    prm, info = svm_train_params(**kw), fd_svm_train_info()
    ctx.check(fn(ctx.h, _ptr(x), n_pos, n - n_pos, d, 0, C.byref(prm), _ptr(w), C.byref(bias), _ptr(alpha), C.byref(info)))
    return w, bias.value, alpha, _svm_info(info)


def linear_svm_train_limits(n_pos, n_neg, d):
    """fd_linear_svm_train_limits (host only): (q_in_lds, max_iterations); FdError for sizes the trainer refuses"""
    q, m = _linear_svm_limits("fd_linear_svm_train_limits", n_pos, n_neg, d)
    return bool(q), m


def linear_svm_gram(ctx, x, n_pos):
    """(Q float32 (n, n), QD float64 (n,)) of n_pos positive rows followed by the negative rows of x"""
    return _linear_svm_gram(lib().fd_linear_svm_gram, ctx, x, n_pos)


def linear_svm_train(ctx, x, n_pos, **kw):
    """fd_linear_svm_train: (weights float32 (d,), bias, alpha float64 (n,), info dict); keywords as svm_train_params"""
    return _linear_svm_train(lib().fd_linear_svm_train, ctx, x, n_pos, kw)


SVM_LARGE_MAX_N = 16384   # FD_SVM_LARGE_MAX_N


def linear_svm_train_large_limits(n_pos, n_neg, d):
    """fd_linear_svm_train_large_limits (host only): (lds_bytes, max_iterations); FdError for sizes the large trainer refuses"""
    return _linear_svm_limits("fd_linear_svm_train_large_limits", n_pos, n_neg, d)


def linear_svm_gram_large(ctx, x, n_pos):
    """linear_svm_gram for up to SVM_LARGE_MAX_N rows (fd_linear_svm_gram_large)"""
    return _linear_svm_gram(lib().fd_linear_svm_gram_large, ctx, x, n_pos)


def linear_svm_train_large(ctx, x, n_pos, **kw):
    """linear_svm_train for up to SVM_LARGE_MAX_N rows (fd_linear_svm_train_large)"""
    return _linear_svm_train(lib().fd_linear_svm_train_large, ctx, x, n_pos, kw)


def linear_svm_train_batch(ctx, problems, **kw):
    """fd_linear_svm_train_batch over [(x, n_pos), ...]: a list of (weights, bias, alpha, info) like linear_svm_train's"""
    count = len(problems)
    xs = [_c(x, np.float32) for x, _ in problems]
    ws = [np.zeros(x.shape[1], np.float32) for x in xs]
    alphas = [np.zeros(x.shape[0], np.float64) for x in xs]
    biases = np.zeros(max(count, 1), np.float32)
    arr = (fd_svm_train_problem * max(count, 1))()
    for c, (x, (_, n_pos)) in enumerate(zip(xs, problems)):
        arr[c] = fd_svm_train_problem(x.ctypes.data, n_pos, x.shape[0] - n_pos, x.shape[1], 0, ws[c].ctypes.data,
                                      biases.ctypes.data + 4 * c, alphas[c].ctypes.data)
    infos = (fd_svm_train_info * max(count, 1))()
    prm = svm_train_params(**kw)
    ctx.check(lib().fd_linear_svm_train_batch(ctx.h, count, arr, C.byref(prm), infos))
    return [(ws[c], float(biases[c]), alphas[c], _svm_info(infos[c])) for c in range(count)]


LIBLINEAR_MAX_N, LIBLINEAR_MAX_D, LIBLINEAR_SMALL_MAX_N = 1048576, 8192, 2048   # FD_LIBLINEAR_*
FD_LL_STOP_GRADIENT, FD_LL_STOP_MAX_ITER, FD_LL_STOP_ACTRED_ZERO, FD_LL_STOP_ACTRED_SMALL, FD_LL_STOP_CG_CAP, FD_LL_STOP_NONFINITE = 1, 2, 3, 4, 5, 6


def liblinear_params(C_=1.0, weight_pos=1.0, weight_neg=1.0, eps=0.0, solver_tol=0.0, bias=False, max_iterations=0, max_cg_steps=0,
                     launch_steps=0, **kw):
    """fd_liblinear_params; the bound may be given as C_ or C"""
    return fd_liblinear_params(kw.pop("C", C_), weight_pos, weight_neg, eps, solver_tol, int(bias), max_iterations, max_cg_steps, launch_steps, **kw)


def _liblinear_info(info):
    return {name: getattr(info, name) for name, _ in fd_liblinear_info._fields_}


def liblinear_train_limits(n_pos, n_neg, d, bias=False):
    """fd_liblinear_train_limits (host only): (single_workgroup, slab_rows, scratch_bytes, lds_bytes); FdError for sizes the trainer
    refuses.  FD_LIBLINEAR_SMALL_ROWS in the environment moves the rule (0: the multi-workgroup form for every size)."""
    single, rows, scratch, lds = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
    rc = lib().fd_liblinear_train_limits(n_pos, n_neg, d, int(bias), C.byref(single), C.byref(rows), C.byref(scratch), C.byref(lds))
    if rc != FD_OK:
        raise FdError(rc, "fd_liblinear_train_limits: invalid sizes (%d, %d, %d, %d)" % (n_pos, n_neg, d, int(bias)))
    return bool(single.value), rows.value, scratch.value, lds.value


def liblinear_train(ctx, x, n_pos, trace_cap=1024, **kw):
    """fd_liblinear_train: (weights float32 (d,), bias, w float64 (d + bias,), trace int32 (k, 3), info dict); x: host array or
    device tensor; keywords as liblinear_params"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    prm, info = liblinear_params(**kw), fd_liblinear_info()
    weights, bias, w = np.zeros(d, np.float32), C.c_float(), np.zeros(d + prm.bias, np.float64)
    trace = np.zeros((max(trace_cap, 1), 3), np.int32)
    ctx.check(lib().fd_liblinear_train(ctx.h, xp, n_pos, n - n_pos, d, dev, C.byref(prm), _ptr(weights), C.byref(bias), _ptr(w), _ptr(trace),
                                       trace_cap, C.byref(info)))
    return weights, bias.value, w, trace[:min(info.trace_len, trace_cap)], _liblinear_info(info)


def liblinear_train_batch(ctx, problems, **kw):
    """fd_liblinear_train_batch over [(x, n_pos), ...] (host arrays): a list of (weights, bias, w, info)"""
    count = len(problems)
    prm = liblinear_params(**kw)
    xs = [_c(x, np.float32) for x, _ in problems]
    ws = [np.zeros(x.shape[1], np.float32) for x in xs]
    wds = [np.zeros(x.shape[1] + prm.bias, np.float64) for x in xs]
    biases = np.zeros(max(count, 1), np.float32)
    arr = (fd_liblinear_problem * max(count, 1))()
    for c, (x, (_, n_pos)) in enumerate(zip(xs, problems)):
        arr[c] = fd_liblinear_problem(x.ctypes.data, n_pos, x.shape[0] - n_pos, x.shape[1], 0, ws[c].ctypes.data, biases.ctypes.data + 4 * c,
                                      wds[c].ctypes.data)
    infos = (fd_liblinear_info * max(count, 1))()
    ctx.check(lib().fd_liblinear_train_batch(ctx.h, count, arr, C.byref(prm), infos))
    return [(ws[c], float(biases[c]), wds[c], _liblinear_info(infos[c])) for c in range(count)]


def liblinear_objective(ctx, x, n_pos, w, s=None, **kw):
    """fd_liblinear_objective: (f, g float64 (d + bias,), Hs or None) at the float64 point w; keywords as liblinear_params"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    prm = liblinear_params(**kw)
    w = _c(w, np.float64)
    if w.shape != (d + prm.bias,):
        raise ValueError("w has d + bias entries")
    f, g = C.c_double(), np.zeros(d + prm.bias, np.float64)
    hs = None
    if s is not None:
        s = _c(s, np.float64)
        if s.shape != w.shape:
            raise ValueError("s has d + bias entries")
        hs = np.zeros_like(g)
    ctx.check(lib().fd_liblinear_objective(ctx.h, xp, n_pos, n - n_pos, d, dev, C.byref(prm), _ptr(w), _ptr(s) if s is not None else None,
                                           C.byref(f), _ptr(g), _ptr(hs) if hs is not None else None))
    return f.value, g, hs


def svm_kernel(kernel, p0=0.0, p1=0.0, p2=0.0):
    """fd_svm_kernel: FD_KERNEL_* and its parameters as in fd_svm_model (rbf: gamma; poly: alpha, constant, degree)"""
    return fd_svm_kernel(int(kernel), float(p0), float(p1), float(p2))


def _svm_kernel(kernel):
    return kernel if isinstance(kernel, fd_svm_kernel) else svm_kernel(*kernel)


def _x_and_pointer(x):
    """(keep-alive, pointer, n, d, is_device) of a host array or a torch tensor on the device (float32, contiguous)"""
    if hasattr(x, "data_ptr"):
        if str(x.dtype) != "torch.float32" or not x.is_contiguous() or x.dim() != 2 or not x.is_cuda:
            raise ValueError("a device input is a contiguous float32 n x d tensor on the GPU")
        return x, C.c_void_p(x.data_ptr()), int(x.shape[0]), int(x.shape[1]), 1
    x = _c(x, np.float32)
    if x.ndim != 2:
        raise ValueError("x is n x d")
    return x, _ptr(x), x.shape[0], x.shape[1], 0


def kernel_svm_train_limits(n_pos, n_neg, d):
    """fd_kernel_svm_train_limits (host only): (q_in_lds, large, max_iterations); FdError for sizes the trainer refuses"""
    q, l, m = C.c_int(), C.c_int(), C.c_int()
    rc = lib().fd_kernel_svm_train_limits(n_pos, n_neg, d, C.byref(q), C.byref(l), C.byref(m))
    if rc != FD_OK:
        raise FdError(rc, "fd_kernel_svm_train_limits: invalid sizes (%d, %d, %d)" % (n_pos, n_neg, d))
    return bool(q.value), bool(l.value), m.value


def kernel_svm_gram(ctx, x, n_pos, kernel):
    """fd_kernel_svm_gram: (Q float32 (n, n), QD float64 (n,)); kernel: svm_kernel(...) or its argument tuple"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    k = _svm_kernel(kernel)
    q, qd = np.zeros((n, n), np.float32), np.zeros(n, np.float64)
    ctx.check(lib().fd_kernel_svm_gram(ctx.h, xp, n_pos, n - n_pos, d, dev, C.byref(k), _ptr(q), _ptr(qd)))
    return q, qd


def kernel_svm_train(ctx, x, n_pos, kernel, want_support_vectors=True, **kw):
    """fd_kernel_svm_train: (sv_index int32 (n_sv,), coefficients float32 (n_sv,), support_vectors float32 (n_sv, d) or None, bias,
    alpha float64 (n,), info dict); x: host array or device tensor; keywords as svm_train_params"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    k = _svm_kernel(kernel)
    svi, coef, alpha, bias = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float64), C.c_float()
    sv = np.zeros((n, d), np.float32) if want_support_vectors else None
    prm, info = svm_train_params(**kw), fd_svm_train_info()
    ctx.check(lib().fd_kernel_svm_train(ctx.h, xp, n_pos, n - n_pos, d, dev, C.byref(k), C.byref(prm), _ptr(svi), _ptr(coef), _ptr(sv),
                                        C.byref(bias), _ptr(alpha), C.byref(info)))
    m = info.n_sv
    return svi[:m].copy(), coef[:m].copy(), (sv[:m].copy() if sv is not None else None), bias.value, alpha, _svm_info(info)


def kernel_svm_train_model(ctx, x, n_pos, kernel, threshold=0.0, logistic_a=0.00556, logistic_b=-2.95, **kw):
    """fd_kernel_svm_train_model: (Svm, info dict) -- the trained f32 model, ready for Svm.distance"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    k = _svm_kernel(kernel)
    prm, info, h = svm_train_params(**kw), fd_svm_train_info(), C.c_void_p()
    ctx.check(lib().fd_kernel_svm_train_model(ctx.h, xp, n_pos, n - n_pos, d, dev, C.byref(k), C.byref(prm), threshold, logistic_a, logistic_b,
                                              C.byref(h), C.byref(info)))
    return Svm.from_handle(ctx, h, d), _svm_info(info)


def kernel_svm_train_batch(ctx, problems, kernel, **kw):
    """fd_kernel_svm_train_batch over [(x, n_pos), ...] (host arrays): a list of tuples like kernel_svm_train's"""
    count = len(problems)
    xs = [_c(x, np.float32) for x, _ in problems]
    svis = [np.zeros(x.shape[0], np.int32) for x in xs]
    coefs = [np.zeros(x.shape[0], np.float32) for x in xs]
    svs = [np.zeros(x.shape, np.float32) for x in xs]
    alphas = [np.zeros(x.shape[0], np.float64) for x in xs]
    biases = np.zeros(max(count, 1), np.float32)
    arr = (fd_kernel_svm_train_problem * max(count, 1))()
    for c, (x, (_, n_pos)) in enumerate(zip(xs, problems)):
        arr[c] = fd_kernel_svm_train_problem(x.ctypes.data, n_pos, x.shape[0] - n_pos, x.shape[1], 0, svis[c].ctypes.data, coefs[c].ctypes.data,
                                             svs[c].ctypes.data, biases.ctypes.data + 4 * c, alphas[c].ctypes.data)
    infos = (fd_svm_train_info * max(count, 1))()
    k, prm = _svm_kernel(kernel), svm_train_params(**kw)
    ctx.check(lib().fd_kernel_svm_train_batch(ctx.h, count, arr, C.byref(k), C.byref(prm), infos))
    out = []
    for c in range(count):
        m = infos[c].n_sv
        out.append((svis[c][:m].copy(), coefs[c][:m].copy(), svs[c][:m].copy(), float(biases[c]), alphas[c], _svm_info(infos[c])))
    return out


def svm_one_class_params(nu=0.5, eps=0.0, max_iterations=0, launch_iterations=0):
    """fd_svm_one_class_params"""
    return fd_svm_one_class_params(float(nu), float(eps), int(max_iterations), int(launch_iterations))


def one_class_svm_train_limits(n, d):
    """fd_one_class_svm_train_limits (host only): (q_in_lds, large, max_iterations); FdError for sizes the trainer refuses"""
    q, l, m = C.c_int(), C.c_int(), C.c_int()
    rc = lib().fd_one_class_svm_train_limits(n, d, C.byref(q), C.byref(l), C.byref(m))
    if rc != FD_OK:
        raise FdError(rc, "fd_one_class_svm_train_limits: invalid sizes (%d, %d)" % (n, d))
    return bool(q.value), bool(l.value), m.value


def one_class_svm_gram(ctx, x, kernel, nu):
    """fd_one_class_svm_gram: (Q float32 (n, n), QD float64 (n,), G0 float64 (n,) -- the start gradient of this nu)"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    k = _svm_kernel(kernel)
    q, qd, g0 = np.zeros((n, n), np.float32), np.zeros(n, np.float64), np.zeros(n, np.float64)
    ctx.check(lib().fd_one_class_svm_gram(ctx.h, xp, n, d, dev, C.byref(k), nu, _ptr(q), _ptr(qd), _ptr(g0)))
    return q, qd, g0


def one_class_svm_train(ctx, x, kernel, want_support_vectors=True, **kw):
    """fd_one_class_svm_train: (sv_index, coefficients, support_vectors or None, bias, alpha, info dict) like kernel_svm_train's;
    keywords as svm_one_class_params"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    k = _svm_kernel(kernel)
    svi, coef, alpha, bias = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float64), C.c_float()
    sv = np.zeros((n, d), np.float32) if want_support_vectors else None
    prm, info = svm_one_class_params(**kw), fd_svm_train_info()
    ctx.check(lib().fd_one_class_svm_train(ctx.h, xp, n, d, dev, C.byref(k), C.byref(prm), _ptr(svi), _ptr(coef), _ptr(sv), C.byref(bias),
                                           _ptr(alpha), C.byref(info)))
    m = info.n_sv
    return svi[:m].copy(), coef[:m].copy(), (sv[:m].copy() if sv is not None else None), bias.value, alpha, _svm_info(info)


def one_class_svm_train_model(ctx, x, kernel, threshold=0.0, logistic_a=0.00556, logistic_b=-2.95, **kw):
    """fd_one_class_svm_train_model: (Svm, info dict); FdError (FD_ERR_RUNTIME) when rho is not finite (nu = 1)"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    k = _svm_kernel(kernel)
    prm, info, h = svm_one_class_params(**kw), fd_svm_train_info(), C.c_void_p()
    ctx.check(lib().fd_one_class_svm_train_model(ctx.h, xp, n, d, dev, C.byref(k), C.byref(prm), threshold, logistic_a, logistic_b, C.byref(h),
                                                 C.byref(info)))
    return Svm.from_handle(ctx, h, d), _svm_info(info)


def svm_sigmoid_train(dec_values, n_pos):
    """fd_svm_sigmoid_train (host only): (probA, probB, iterations, status) of libsvm's sigmoid_train on decision values whose
    first n_pos belong to positive examples"""
    dec = _c(dec_values, np.float64).reshape(-1)
    a, b, it, st = C.c_double(), C.c_double(), C.c_int(), C.c_int()
    rc = lib().fd_svm_sigmoid_train(len(dec), _ptr(dec) if len(dec) else None, n_pos, C.byref(a), C.byref(b), C.byref(it), C.byref(st))
    if rc != FD_OK:
        raise FdError(rc, "fd_svm_sigmoid_train: invalid arguments (%d, %d)" % (len(dec), n_pos))
    return a.value, b.value, it.value, st.value


def kernel_svm_cv_sigmoid(ctx, x, n_pos, kernel, perm, **kw):
    """fd_kernel_svm_cv_sigmoid: (probA, probB, dec_values float64 (n,), info) -- info: folds (a list of five dicts: the fold's
    train info, trained, constant), newton_iterations, status; perm: n ints; keywords as svm_train_params"""
    keep, xp, n, d, dev = _x_and_pointer(x)
    k = _svm_kernel(kernel)
    perm = _c(perm, np.int32).reshape(-1)
    if len(perm) != n:
        raise ValueError("perm has n entries")
    dec, a, b = np.zeros(n, np.float64), C.c_double(), C.c_double()
    prm, ci = svm_train_params(**kw), fd_svm_cv_info()
    ctx.check(lib().fd_kernel_svm_cv_sigmoid(ctx.h, xp, n_pos, n - n_pos, d, dev, C.byref(k), C.byref(prm), _ptr(perm), C.byref(a), C.byref(b),
                                             _ptr(dec), C.byref(ci)))
    folds = [dict(_svm_info(ci.fold[f]), trained=bool(ci.fold_trained[f]), constant=ci.fold_constant[f]) for f in range(FD_SVM_CV_FOLDS)]
    return a.value, b.value, dec, dict(folds=folds, newton_iterations=ci.newton_iterations, status=ci.status)


# fd_aggregated_layer: one feature layer of an aggregated-features detector
AGG_LAYER_DTYPE = np.dtype([("index", "<i4"), ("approximated", "<i4"), ("parent", "<i4"), ("rows", "<i4"), ("cols", "<i4"),
                            ("reserved", "<i4"), ("scale", "<f8"), ("scale_x", "<f8"), ("scale_y", "<f8")], align=True)


def aggregated_plan_layers(window_w, window_h, cell_size, octave_layers, min_window_width, width, height):
    """fd_aggregated_plan_layers (host only): the feature layers of an approximated detector on a width x height image as an
    AGG_LAYER_DTYPE array; FdError (FD_ERR_RUNTIME) when fewer than two exact layers remain"""
    out = np.zeros(1024, AGG_LAYER_DTYPE)
    n = C.c_int()
    rc = lib().fd_aggregated_plan_layers(window_w, window_h, cell_size, octave_layers, min_window_width, width, height, _ptr(out), len(out),
                                         C.byref(n))
    if rc != 0:
        raise FdError(rc, "fd_aggregated_plan_layers: status %d (%d layers)" % (rc, n.value))
    return out[:n.value].copy()


def _fpdw_params(cell_size, fast_gradient, interpolate_bins, normalization_radius, normalization_constant):
    radius = cell_size if normalization_radius is None else normalization_radius   # DetectorTrainingApp passes the cell size
    return fd_fpdw_params(cell_size, int(fast_gradient), int(interpolate_bins), radius, normalization_constant)


def fpdw_size(width, height, cell_size=8, **kw):
    """fd_fpdw_size (host only): (rows, cols, channels) of the FPDW cells of a width x height image"""
    fp = _fpdw_params(cell_size, kw.get("fast_gradient", True), kw.get("interpolate_bins", False), kw.get("normalization_radius"),
                      kw.get("normalization_constant", 0.01))
    r, c, d = C.c_int(), C.c_int(), C.c_int()
    rc = lib().fd_fpdw_size(C.byref(fp), width, height, C.byref(r), C.byref(c), C.byref(d))
    if rc != FD_OK:
        raise FdError(rc, "fd_fpdw_size: invalid parameters")
    return r.value, c.value, d.value


def fpdw_gradient_lut(interpolate_bins=False):
    """fd_fpdw_gradient_lut (host only): dict of the 65536-entry arrays bin1, bin2 (int32), w1, w2, magnitude (float32), index
    gx | gy << 8"""
    fp = _fpdw_params(8, True, interpolate_bins, None, 0.01)
    out = dict(bin1=np.zeros(65536, np.int32), bin2=np.zeros(65536, np.int32), w1=np.zeros(65536, np.float32),
               w2=np.zeros(65536, np.float32), magnitude=np.zeros(65536, np.float32))
    rc = lib().fd_fpdw_gradient_lut(C.byref(fp), _ptr(out["bin1"]), _ptr(out["bin2"]), _ptr(out["w1"]), _ptr(out["w2"]), _ptr(out["magnitude"]))
    if rc != FD_OK:
        raise FdError(rc, "fd_fpdw_gradient_lut failed")
    return out


def _fpdw_call(ctx, fn, bgr, out_shape, fp):
    bgr = _c(bgr, np.uint8)
    if bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError("FPDW features need a BGR image (h, w, 3)")
    h, w = bgr.shape[:2]
    out = np.zeros(out_shape(h, w), np.float32)
    ctx.check(fn(ctx.h, _ptr(bgr), w, h, C.byref(fp), _ptr(out)))
    return out


def fpdw_image(ctx, bgr, cell_size=8, fast_gradient=True, interpolate_bins=False, normalization_radius=None, normalization_constant=0.01):
    """FpdwFeaturesFilter::applyTo on a host BGR image: (h, w, 10) float32"""
    fp = _fpdw_params(cell_size, fast_gradient, interpolate_bins, normalization_radius, normalization_constant)
    return _fpdw_call(ctx, lib().fd_fpdw_image, bgr, lambda h, w: (h, w, 10), fp)


def fpdw_cells_image(ctx, bgr, cell_size=8, fast_gradient=True, interpolate_bins=False, normalization_radius=None, normalization_constant=0.01):
    """ChainedFilter(FpdwFeaturesFilter, AggregationFilter(cell_size, true, false)) on a host BGR image: (h / cell, w / cell, 10) float32"""
    fp = _fpdw_params(cell_size, fast_gradient, interpolate_bins, normalization_radius, normalization_constant)
    cs = max(cell_size, 1)   # invalid parameters are reported by the library
    return _fpdw_call(ctx, lib().fd_fpdw_cells_image, bgr, lambda h, w: (h // cs, w // cs, 10), fp)


class Aggregated:
    """fd_aggregated handle: AggregatedFeaturesDetector with GrayscaleFilter + FhogFilter; weights (window_h, window_w, 3B+4).
    approximate=True: the approximated feature pyramid (ImagePyramid::createApproximated) with the given per-channel lambdas,
    or lambdas estimated per image when lambdas is None.
    features="fpdw": no image filter and FpdwFeaturesFilter + AggregationFilter as layer filter instead (BGR images only; weights
    (window_h, window_w, 10); normalization_radius None: the cell size)."""
    def __init__(self, ctx, weights, bias, threshold, cell_size=8, unsigned_bins=9, interpolate_bins=False, interpolate_cells=True, alpha=0.2,
                 octave_layers=5, min_window_width=0, width_scale=1.0, height_scale=1.0, nms_overlap=0.3, nms_type=0, approximate=False,
                 lambdas=None, features="fhog", fast_gradient=True, normalization_radius=None, normalization_constant=0.01):
        if features not in ("fhog", "fpdw"):
            raise ValueError("features must be 'fhog' or 'fpdw'")
        self.ctx = ctx
        self._w = _c(weights, np.float32)
        wh, ww, d = self._w.shape
        assert d == (10 if features == "fpdw" else 3 * unsigned_bins + 4)
        prm = fd_aggregated_params(fd_fhog_params(cell_size, unsigned_bins, int(interpolate_bins), int(interpolate_cells), alpha), ww, wh,
                                   octave_layers, min_window_width, width_scale, height_scale, self._w.ctypes.data, bias, threshold,
                                   nms_overlap, nms_type)
        self.h = C.c_void_p()
        self.channels = d
        if features == "fpdw":
            if lambdas is not None and not approximate:
                raise ValueError("lambdas belong to the approximated feature pyramid (approximate=True)")
            fp = _fpdw_params(cell_size, fast_gradient, interpolate_bins, normalization_radius, normalization_constant)
            lam = _c(lambdas, np.float64) if lambdas is not None else None
            ctx.check(lib().fd_aggregated_create_fpdw(ctx.h, C.byref(prm), C.byref(fp), int(approximate), _ptr(lam) if lam is not None else None,
                                                      len(lam) if lam is not None else 0, C.byref(self.h)))
        elif approximate:
            lam = _c(lambdas, np.float64) if lambdas is not None else None
            ctx.check(lib().fd_aggregated_create_approximated(ctx.h, C.byref(prm), _ptr(lam) if lam is not None else None,
                                                              len(lam) if lam is not None else 0, C.byref(self.h)))
        else:
            if lambdas is not None:
                raise ValueError("lambdas belong to the approximated feature pyramid (approximate=True)")
            ctx.check(lib().fd_aggregated_create(ctx.h, C.byref(prm), C.byref(self.h)))

    def lambdas(self):
        """the lambdas the last detect used (approximated handles)"""
        out = np.zeros(self.channels, np.float64)
        n = C.c_int()
        self.ctx.check(lib().fd_aggregated_get_lambdas(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def layers(self):
        """feature layers of the last detect, in layer order (AGG_LAYER_DTYPE)"""
        out = np.zeros(1024, AGG_LAYER_DTYPE)
        n = C.c_int()
        self.ctx.check(lib().fd_aggregated_get_layers(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def feature_layer(self, i):
        """feature layer i (position in layers()) of the last detect: (rows, cols, 3B+4) float32"""
        L = self.layers()[i]
        out = np.empty((int(L["rows"]), int(L["cols"]), self.channels), np.float32)
        self.ctx.check(lib().fd_aggregated_feature_layer(self.ctx.h, self.h, int(i), _ptr(out)))
        return out

    def update(self, image):
        """AggregatedFeaturesExtractor::update: the feature layers of the image, no scores (layers(), feature_layer(), extract())"""
        image = _c(image, np.uint8)
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        self.ctx.check(lib().fd_aggregated_update(self.ctx.h, self.h, _ptr(image), w, h, ch, 0))

    def extract(self, boxes, out=None):
        """AggregatedFeaturesExtractor::extract(Rect) for n boxes (x, y, w, h) in image pixels: (features float32 (n, window_h *
        window_w * channels), bounds BOX_DTYPE (n,), valid bool (n,)).  Rows and bounds of invalid boxes keep what `out` (or
        zeros) held."""
        boxes = _c(np.asarray(boxes, np.int32).reshape(-1, 4), np.int32)
        n = len(boxes)
        d = self._w.size
        feats = np.zeros((n, d), np.float32) if out is None else out
        assert feats.dtype == np.float32 and feats.shape == (n, d) and feats.flags.c_contiguous
        bounds, valid = np.zeros(n, BOX_DTYPE), np.zeros(n, np.uint8)
        self.ctx.check(lib().fd_aggregated_extract(self.ctx.h, self.h, n, _ptr(boxes), _ptr(feats), 0, _ptr(bounds), _ptr(valid)))
        return feats, bounds, valid.astype(bool)

    def set_svm(self, weights, bias, threshold):
        """replaces the linear SVM and the threshold of the handle (fd_aggregated_set_svm)"""
        w = _c(weights, np.float32)
        if w.shape != self._w.shape:
            raise ValueError("weights must have shape %r" % (self._w.shape,))
        self.ctx.check(lib().fd_aggregated_set_svm(self.ctx.h, self.h, _ptr(w), bias, threshold))
        self._w = w

    def detect(self, image, cap=1 << 16, candidates=True):
        """(final detections, candidates) as BOX_DTYPE arrays (candidates None when not asked for)"""
        image = _c(image, np.uint8)
        h, w = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        return self._detect(_ptr(image), w, h, ch, 0, cap, candidates)

    def detect_device(self, ptr, w, h, ch, cap=1 << 16, candidates=False):
        """same on a frame that already lives in HBM (ptr: device address of h x w x ch bytes)"""
        return self._detect(C.c_void_p(ptr), w, h, ch, 1, cap, candidates)

    def _detect(self, iptr, w, h, ch, is_device, cap, candidates):
        out = np.zeros(cap, BOX_DTYPE)
        cand = np.zeros(1 << 20, BOX_DTYPE) if candidates else None
        n, nc = C.c_int(), C.c_int()
        self.ctx.check(lib().fd_aggregated_detect(self.ctx.h, self.h, iptr, w, h, ch, is_device, _ptr(out), cap, C.byref(n),
                                                  _ptr(cand) if candidates else None, len(cand) if candidates else 0, C.byref(nc)))
        return out[:n.value], (cand[:nc.value] if candidates else None)

    def close(self):
        if getattr(self, "h", None):
            lib().fd_aggregated_destroy(self.h)
            self.h = None

    def __del__(self):   # a handle nobody holds any more gives its device memory back (hipFree waits for the device)
        try:
            self.close()
        except Exception:
            pass


def nms_iou(boxes, overlap_threshold, maximum_type=0):
    """NonMaximumSuppression::eliminateRedundantDetections on a BOX_DTYPE array (host only)"""
    boxes = _c(boxes, BOX_DTYPE)
    out = np.zeros(max(len(boxes), 1), BOX_DTYPE)
    cnt = C.c_int()
    rc = lib().fd_nms_iou(_ptr(boxes), len(boxes), overlap_threshold, maximum_type, _ptr(out), C.byref(cnt))
    if rc != 0:
        raise FdError(rc, "fd_nms_iou: invalid arguments (overlap threshold %g, maximum type %d)" % (overlap_threshold, maximum_type))
    return out[:cnt.value]


def wvm_svm_evaluate(ctx, pyr, wvm, svm, samples):
    """condensation::WvmSvmModel::evaluate: samples (n, 4) {x, y, width, height} -> (target bool[n], weight f64[n])"""
    samples = _c(samples, np.int32).reshape(-1, 4)
    target = np.zeros(len(samples), np.uint8)
    weight = np.zeros(len(samples), np.float64)
    ctx.check(lib().fd_wvm_svm_evaluate_samples(ctx.h, pyr.h, wvm.h, svm.h, len(samples), _ptr(samples), _ptr(target), _ptr(weight)))
    return target.astype(bool), weight


def overlap_elimination(dets, dist, ratio):
    dets = _c(dets, DET_DTYPE)
    keep = np.empty(max(len(dets), 1), np.int32)
    cnt = C.c_int()
    rc = lib().fd_overlap_elimination(_ptr(dets), len(dets), dist, ratio, _ptr(keep), C.byref(cnt))
    if rc != FD_OK:
        raise FdError(rc, "fd_overlap_elimination")
    return keep[:cnt.value]


def block_nms(dets, img_w, img_h, sz=35, masked=True):
    dets = _c(dets, DET_DTYPE)
    xy = np.empty((max(len(dets), 1), 2), np.int32)
    cnt = C.c_int()
    rc = lib().fd_block_nms(_ptr(dets), len(dets), img_w, img_h, sz, int(masked), _ptr(xy), len(xy), C.byref(cnt))
    if rc != FD_OK:
        raise FdError(rc, "fd_block_nms")
    return xy[:cnt.value]


def extract_hog(ctx, pyr, hp):
    n = C.c_int64()
    ctx.check(lib().fd_extract_hog(ctx.h, pyr.h, C.byref(hp), None, 0, C.byref(n)))
    F = lib().fd_hog_feature_length(C.byref(hp))
    out = np.empty((n.value, F), np.float32)
    ctx.check(lib().fd_extract_hog(ctx.h, pyr.h, C.byref(hp), _ptr(out), n.value, C.byref(n)))
    return out


def hist_params(kind, pw=20, ph=20, sx=2, sy=2, bins=9, cell=5, block=1, levels=2, interpolate=False, signed_and_unsigned=False,
                concatenate=False, normalization=1, cell_h=0, block_h=0):
    return fd_hist_params(pw, ph, sx, sy, kind, bins, cell, block, levels, int(interpolate), int(signed_and_unsigned),
                          int(concatenate), int(normalization), cell_h, block_h)


def extract_hist(ctx, pyr, hp):
    """features of every window: (n_windows, feature_length) float32"""
    n = C.c_int64()
    ctx.check(lib().fd_extract_hist(ctx.h, pyr.h, C.byref(hp), None, 0, C.byref(n)))
    layers = pyr.layers()
    if not layers:   # no pyramid layer inside [min scale, max scale]: no windows
        return np.empty((0, 0), np.float32)
    ch = layers[0]["ch"]
    F = lib().fd_hist_feature_length(C.byref(hp), ch)
    if F < 0:
        raise ValueError("invalid histogram parameters")
    out = np.empty((n.value, F), np.float32)
    ctx.check(lib().fd_extract_hist(ctx.h, pyr.h, C.byref(hp), _ptr(out), n.value, C.byref(n)))
    return out


def detect_hist_svm(ctx, pyr, svm, hp, want_all=True, cap=1 << 20):
    n = pyr.window_count(hp.patch_w, hp.patch_h, hp.step_x, hp.step_y)
    out = np.zeros(min(cap, max(n, 1)), DET_DTYPE)
    alld = np.empty(n, np.float64) if want_all else None
    cnt = C.c_int64()
    ctx.check(lib().fd_detect_hist_svm(ctx.h, pyr.h, svm.h, C.byref(hp), _ptr(out), out.shape[0], C.byref(cnt), _ptr(alld)))
    return out[:cnt.value], alld


class Rvm:
    """fd_rvm handle; m: dict as synth.make_rvm"""
    def __init__(self, ctx, m):
        self.ctx, self.model = ctx, m
        self._sv = _c(m["sv"], np.float32)
        self._coeff = _c(m["coeff"], np.float32)
        self._thr = _c(m["thresholds"], np.float32)
        s = fd_rvm_model()
        s.kernel = int(m["kernel"]); s.p0 = float(m.get("p0", 0)); s.p1 = float(m.get("p1", 0)); s.p2 = float(m.get("p2", 0))
        s.num_filters = self._sv.shape[0]; s.num_used = int(m.get("num_used", 0))
        s.filter_w, s.filter_h = int(m["filter_w"]), int(m["filter_h"])
        s.support_vectors = self._sv.ctypes.data; s.coefficients = self._coeff.ctypes.data; s.thresholds = self._thr.ctypes.data
        s.bias = float(m["bias"]); s.logistic_a = float(m.get("logistic_a", 0.0)); s.logistic_b = float(m.get("logistic_b", -1.0))
        self.h = C.c_void_p()
        ctx.check(lib().fd_rvm_create(ctx.h, C.byref(s), C.byref(self.h)))

    def eval(self, feats):
        feats = _c(feats, np.float32).reshape(len(feats), -1)
        lv = np.empty(len(feats), np.int32)
        d = np.empty(len(feats), np.float64)
        self.ctx.check(lib().fd_rvm_eval_batch(self.ctx.h, self.h, _ptr(feats), len(feats), _ptr(lv), _ptr(d)))
        return lv, d

    def close(self):
        if getattr(self, "h", None):
            lib().fd_rvm_destroy(self.h)
            self.h = None

    def __del__(self):   # a handle nobody holds any more gives its device memory back (hipFree waits for the device)
        try:
            self.close()
        except Exception:
            pass


def detect_rvm(ctx, pyr, rvm, feature_space=FEATURE_HQ64, conv_scale=1.0, conv_shift=0.0, sx=1, sy=1, roi=None, want_all=True, cap=1 << 20):
    n = pyr.window_count(rvm.model["filter_w"], rvm.model["filter_h"], sx, sy, roi)
    out = np.zeros(min(cap, max(n, 1)), DET_DTYPE)
    lv = np.empty(n, np.int32) if want_all else None
    dd = np.empty(n, np.float64) if want_all else None
    cnt = C.c_int64()
    dp = fd_rvm_detect_params(feature_space, conv_scale, conv_shift, sx, sy)
    r = _c(roi, np.int32) if roi is not None else None
    ctx.check(lib().fd_detect_rvm(ctx.h, pyr.h, rvm.h, C.byref(dp), _ptr(r), _ptr(out), out.shape[0], C.byref(cnt), _ptr(lv), _ptr(dd)))
    return out[:cnt.value], lv, dd


def _second_handles(second):
    """(svm handle, rvm handle) of a five-stage second classifier: a capi.Svm or a capi.Rvm"""
    if isinstance(second, Svm):
        return second.h, None
    if isinstance(second, Rvm):
        return None, second.h
    raise TypeError("second classifier must be a capi.Svm or a capi.Rvm")


def detect_five_stage_rvm(ctx, pyr, rvm, second, feature_space=FEATURE_HQ64, conv_scale=1.0, conv_shift=0.0, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1,
                          roi=None, cap=4096):
    """fd_detect_five_stage_rvm: the five-stage detector with an RVM first stage; second: capi.Svm (f32) or capi.Rvm.  (dets, stage_counts)"""
    out = np.zeros(cap, DET_DTYPE)
    cnt = C.c_int()
    stages = np.zeros(4, np.int32)
    dp = fd_rvm_detect_params(feature_space, conv_scale, conv_shift, sx, sy)
    r = _c(roi, np.int32) if roi is not None else None
    hs, hr = _second_handles(second)
    ctx.check(lib().fd_detect_five_stage_rvm(ctx.h, pyr.h, rvm.h, C.byref(dp), hs, hr, oe_dist, oe_ratio, _ptr(r), _ptr(out), cap, C.byref(cnt),
                                             _ptr(stages)))
    return out[:cnt.value], stages


class FiveStageRvmImage:
    """fd_detect_five_stage_rvm_image with preallocated result buffers, the twin of FiveStageImage (the output arrays are reused: copy what
    must outlive the next call)"""

    def __init__(self, ctx, pyr, rvm, second, feature_space=FEATURE_HQ64, conv_scale=1.0, conv_shift=0.0, oe_dist=5.0, oe_ratio=0.0, sx=1, sy=1,
                 cap=4096):
        self.ctx, self.pyr, self.rvm, self.second = ctx, pyr, rvm, second
        self.dp = fd_rvm_detect_params(feature_space, conv_scale, conv_shift, sx, sy)
        self.args = (oe_dist, oe_ratio)
        self.cap = cap
        self.out = np.zeros(cap, DET_DTYPE)
        self.cnt = C.c_int()
        self.stages = np.zeros(4, np.int32)
        self._fn = lib().fd_detect_five_stage_rvm_image
        self._hs, self._hr = _second_handles(second)
        self._outp, self._stp, self._cntp = _ptr(self.out), _ptr(self.stages), C.byref(self.cnt)

    def _run(self, iptr, w, h, ch, is_device):
        a = self.args
        self.ctx.check(self._fn(self.ctx.h, self.pyr.h, self.rvm.h, C.byref(self.dp), self._hs, self._hr, iptr, w, h, ch, is_device, a[0], a[1], None,
                                self._outp, self.cap, self._cntp, self._stp))
        return self.out[:self.cnt.value], self.stages

    def detect_device(self, dev_ptr, w, h, ch):
        return self._run(C.c_void_p(dev_ptr), w, h, ch, 1)

    def detect(self, image):
        image = np.ascontiguousarray(image, np.uint8)
        ch = 1 if image.ndim == 2 else image.shape[2]
        return self._run(_ptr(image), image.shape[1], image.shape[0], ch, 0)


def whi_batch(ctx, patches, alpha=1.0, cutoff=0.390625):
    patches = _c(patches, np.uint8)
    n, h, w = patches.shape
    out = np.empty((n, h, w), np.float32)
    ctx.check(lib().fd_whi_batch(ctx.h, _ptr(patches), n, w, h, alpha, cutoff, _ptr(out)))
    return out


def equalize_hist_batch(ctx, patches):
    patches = _c(patches, np.uint8)
    n, h, w = patches.shape
    out = np.empty_like(patches)
    ctx.check(lib().fd_equalize_hist_batch(ctx.h, _ptr(patches), n, w, h, _ptr(out)))
    return out


def whi_params(pw=20, ph=20, sx=2, sy=2, alpha=1.0, cutoff=0.390625):
    return fd_whi_params(pw, ph, sx, sy, alpha, cutoff)


def extract_whi(ctx, pyr, wp):
    n = C.c_int64()
    ctx.check(lib().fd_extract_whi(ctx.h, pyr.h, C.byref(wp), None, 0, C.byref(n)))
    out = np.empty((n.value, wp.patch_w * wp.patch_h), np.float32)
    ctx.check(lib().fd_extract_whi(ctx.h, pyr.h, C.byref(wp), _ptr(out), n.value, C.byref(n)))
    return out


def detect_whi_svm(ctx, pyr, svm, wp, want_all=True, cap=1 << 20):
    n = pyr.window_count(wp.patch_w, wp.patch_h, wp.step_x, wp.step_y)
    out = np.zeros(min(cap, max(n, 1)), DET_DTYPE)
    alld = np.empty(n, np.float64) if want_all else None
    cnt = C.c_int64()
    ctx.check(lib().fd_detect_whi_svm(ctx.h, pyr.h, svm.h, C.byref(wp), _ptr(out), out.shape[0], C.byref(cnt), _ptr(alld)))
    return out[:cnt.value], alld


def detect_hog_svm(ctx, pyr, svm, hp, want_all=True, cap=1 << 20):
    n = pyr.window_count(hp.patch_w, hp.patch_h, hp.step_x, hp.step_y)
    out = np.zeros(min(cap, max(n, 1)), DET_DTYPE)
    alld = np.empty(n, np.float64) if want_all else None
    cnt = C.c_int64()
    ctx.check(lib().fd_detect_hog_svm(ctx.h, pyr.h, svm.h, C.byref(hp), _ptr(out), out.shape[0], C.byref(cnt), _ptr(alld)))
    return out[:cnt.value], alld


# ---- stand-alone ImageFilter::applyTo forms
def gradient_image(ctx, gray, ksize=1, blur=0):
    g = _c(gray, np.uint8)
    out = np.empty(g.shape + (2,), np.uint8)
    if blur:
        ctx.check(lib().fd_gradient_filter_image(ctx.h, _ptr(g), g.shape[1], g.shape[0], ksize, blur, _ptr(out)))
    else:
        ctx.check(lib().fd_gradient_image(ctx.h, _ptr(g), g.shape[1], g.shape[0], ksize, _ptr(out)))
    return out


def gradient_binning_image(ctx, grad2ch, bins, signed_gradients=False, interpolate=False):
    g = _c(grad2ch, np.uint8)
    out = np.empty(g.shape[:2] + (4 if interpolate else 2,), np.uint8)
    ctx.check(lib().fd_gradient_binning_image(ctx.h, _ptr(g), g.shape[1], g.shape[0], bins, int(signed_gradients), int(interpolate), _ptr(out)))
    return out


def lbp_image(ctx, gray, lbp_type=0):
    g = _c(gray, np.uint8)
    out = np.empty(g.shape, np.uint8)
    ctx.check(lib().fd_lbp_image(ctx.h, _ptr(g), g.shape[1], g.shape[0], lbp_type, _ptr(out)))
    return out


def gradient_magnitude_image(ctx, grad2ch):
    """imageprocessing::GradientMagnitudeFilter on a CV_8UC2 gradient image [h, w, 2] -> [h, w] u8"""
    g = _c(grad2ch, np.uint8)
    if g.ndim != 3 or g.shape[2] != 2:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "GradientMagnitudeFilter: the image must have two channels")
    out = np.empty(g.shape[:2], np.uint8)
    ctx.check(lib().fd_gradient_magnitude_image(ctx.h, _ptr(g), g.shape[1], g.shape[0], _ptr(out)))
    return out


def sample_windows(layers, inc, pw, ph, samples):
    """host only: layers as Pyramid.layers() (dicts with index, scale, w, h); samples (n, 4) {x, y, width, height} ->
    (n, 4) int32 {layer position, bx, by, valid}"""
    s = _c(samples, np.int32).reshape(-1, 4)
    idx = _c([l["index"] for l in layers], np.int32)
    sc = _c([l["scale"] for l in layers], np.float64)
    lw = _c([l["w"] for l in layers], np.int32)
    lh = _c([l["h"] for l in layers], np.int32)
    out = np.zeros((len(s), 4), np.int32)
    rc = lib().fd_sample_windows(len(layers), _ptr(idx), _ptr(sc), _ptr(lw), _ptr(lh), inc, pw, ph, len(s), _ptr(s), _ptr(out))
    if rc != FD_OK:
        raise FdError(rc, "fd_sample_windows: invalid arguments")
    return out


def sample_layer_table(n_layers, first_index, inc, patch_w, cap=FD_SAMPLE_TABLE_MAX):
    """fd_sample_layer_table (host only): int16[length], entry w the position in the kept-layer list of a sample of width w, -1 for
    none.  FdError FD_ERR_CAPACITY (with .length, the entries it needs) when the table is longer than cap"""
    length = C.c_int(0)
    table = np.zeros(0, np.int16)
    rc = lib().fd_sample_layer_table(n_layers, first_index, inc, patch_w, 0, None, C.byref(length))
    if rc in (FD_OK, FD_ERR_CAPACITY) and length.value <= cap:
        table = np.zeros(length.value, np.int16)
        rc = lib().fd_sample_layer_table(n_layers, first_index, inc, patch_w, len(table), _ptr(table), C.byref(length))
    if rc != FD_OK:
        e = FdError(rc, "fd_sample_layer_table: %s" % ("a table of %d entries" % length.value if rc == FD_ERR_CAPACITY else "invalid arguments"))
        e.length = length.value
        raise e
    return table


def hist_samples_limits():
    n = C.c_int()
    if lib().fd_hist_samples_limits(C.byref(n)) != FD_OK:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "fd_hist_samples_limits")
    return n.value


def hist_extract_samples(ctx, pyr, hp, samples):
    """the FD_HIST_* patch filter hp on the sampled windows of pyr: (features (n, F) f32, valid bool[n]); rows without a window are zero"""
    s = _c(samples, np.int32).reshape(-1, 4)
    layers = pyr.layers()
    F = lib().fd_hist_feature_length(C.byref(hp), layers[0]["ch"] if layers else 1)
    if F < 0:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "invalid histogram parameters")
    feats = np.zeros((len(s), F), np.float32)
    valid = np.zeros(len(s), np.uint8)
    ctx.check(lib().fd_hist_extract_samples(ctx.h, pyr.h, C.byref(hp), len(s), _ptr(s), _ptr(valid), _ptr(feats)))
    return feats, valid.astype(bool)


def ehog_extract_samples(ctx, pyr, ep, samples):
    """ExtendedHogFilter on the sampled windows of a FD_LAYER_GRADBIN pyramid: (features (n, F) f32, valid bool[n])"""
    s = _c(samples, np.int32).reshape(-1, 4)
    layers = pyr.layers()
    F = lib().fd_ehog_feature_length(C.byref(ep), layers[0]["ch"] if layers else 2)
    if F < 0:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "invalid extended HOG parameters")
    feats = np.zeros((len(s), F), np.float32)
    valid = np.zeros(len(s), np.uint8)
    ctx.check(lib().fd_ehog_extract_samples(ctx.h, pyr.h, C.byref(ep), len(s), _ptr(s), _ptr(valid), _ptr(feats)))
    return feats, valid.astype(bool)


def hist_svm_evaluate_samples(ctx, pyr, params, svm, samples, want_distance=False):
    """condensation::SingleClassifierModel::evaluate on sampled pyramid windows: params is a fd_hist_params or a fd_ehog_patch_params;
    -> (target bool[n], weight f64[n]) and, with want_distance, the hyperplane distances f64[n]"""
    kind = FD_SAMPLES_EHOG if isinstance(params, fd_ehog_patch_params) else FD_SAMPLES_HIST
    s = _c(samples, np.int32).reshape(-1, 4)
    target = np.zeros(len(s), np.uint8)
    weight = np.zeros(len(s), np.float64)
    if want_distance:
        dist = np.zeros(len(s), np.float64)
        ctx.check(lib().fd_hist_svm_evaluate_samples_distance(ctx.h, pyr.h, kind, C.byref(params), svm.h, len(s), _ptr(s), _ptr(target), _ptr(weight),
                                                              _ptr(dist)))
        return target.astype(bool), weight, dist
    ctx.check(lib().fd_hist_svm_evaluate_samples(ctx.h, pyr.h, kind, C.byref(params), svm.h, len(s), _ptr(s), _ptr(target), _ptr(weight)))
    return target.astype(bool), weight


def patch_samples_params(pw=20, ph=20, feature_space=FD_FEATURE_GRAY, conv_scale=1.0, conv_shift=0.0, whi_alpha=1.0, whi_cutoff=0.390625):
    return fd_patch_samples_params(pw, ph, feature_space, conv_scale, conv_shift, whi_alpha, whi_cutoff)


def patch_extract_samples(ctx, pyr, pp, samples):
    """the gray-patch feature space pp on the sampled windows of a gray pyramid: (features (n, pw * ph) f32, valid bool[n]); rows without a
    window are zero"""
    s = _c(samples, np.int32).reshape(-1, 4)
    F = lib().fd_patch_feature_length(C.byref(pp))
    feats = np.zeros((len(s), max(F, 0)), np.float32)   # F < 0: the call refuses the parameters, with its message, before it writes
    valid = np.zeros(len(s), np.uint8)
    ctx.check(lib().fd_patch_extract_samples(ctx.h, pyr.h, C.byref(pp), len(s), _ptr(s), _ptr(valid), _ptr(feats)))
    return feats, valid.astype(bool)


def patch_svm_evaluate_samples(ctx, pyr, pp, svm, samples, want_distance=False):
    """condensation::SingleClassifierModel::evaluate on sampled gray patches with an f32 SVM: (target bool[n], weight f64[n]) and, with
    want_distance, the hyperplane distances f64[n]"""
    s = _c(samples, np.int32).reshape(-1, 4)
    target = np.zeros(len(s), np.uint8)
    weight = np.zeros(len(s), np.float64)
    dist = np.zeros(len(s), np.float64) if want_distance else None
    ctx.check(lib().fd_patch_svm_evaluate_samples(ctx.h, pyr.h, C.byref(pp), svm.h, len(s), _ptr(s), _ptr(target), _ptr(weight), _ptr(dist)))
    return (target.astype(bool), weight, dist) if want_distance else (target.astype(bool), weight)


def patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, samples):
    """the RVM cascade on sampled gray patches: (valid bool[n], level i32[n], distance f64[n], target bool[n]); a sample without a window
    has valid False, level -1, distance 0, target False"""
    s = _c(samples, np.int32).reshape(-1, 4)
    valid = np.zeros(len(s), np.uint8)
    level = np.full(len(s), -1, np.int32)
    dist = np.zeros(len(s), np.float64)
    target = np.zeros(len(s), np.uint8)
    ctx.check(lib().fd_patch_rvm_evaluate_samples(ctx.h, pyr.h, C.byref(pp), rvm.h, len(s), _ptr(s), _ptr(valid), _ptr(level), _ptr(dist),
                                                  _ptr(target)))
    return valid.astype(bool), level, dist, target.astype(bool)


def hist_patch_batch(ctx, bin_patches, hp):
    """bin_patches: [n, ph, pw, channels] u8 (or [n, ph, pw]); hp from hist_params(...)"""
    b = _c(bin_patches, np.uint8)
    ch = b.shape[3] if b.ndim == 4 else 1
    F = lib().fd_hist_feature_length(C.byref(hp), ch)
    if F < 0:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "invalid histogram parameters")
    out = np.empty((b.shape[0], F), np.float32)
    ctx.check(lib().fd_hist_patch_batch(ctx.h, _ptr(b), b.shape[0], ch, C.byref(hp), _ptr(out)))
    return out


def whitening_batch(ctx, patches, alpha=1.0, cutoff=0.390625):
    p = _c(patches, np.uint8)
    out = np.empty(p.shape, np.uint8)
    ctx.check(lib().fd_whitening_batch(ctx.h, _ptr(p), p.shape[0], p.shape[2], p.shape[1], alpha, cutoff, _ptr(out)))
    return out


def convert_batch(ctx, src, alpha=1.0, beta=0.0, to_f32=True):
    s = np.ascontiguousarray(src)
    if s.dtype not in (np.uint8, np.float32):
        raise ValueError("u8 or f32")
    out = np.empty(s.shape, np.float32 if to_f32 else np.uint8)
    ctx.check(lib().fd_convert_batch(ctx.h, _ptr(s), FD_DTYPE_F32 if s.dtype == np.float32 else FD_DTYPE_U8, s.size, alpha, beta, _ptr(out),
                                     FD_DTYPE_F32 if to_f32 else FD_DTYPE_U8))
    return out


def unit_norm_batch(ctx, vecs, norm_type=4):
    v = _c(vecs, np.float32)
    out = np.empty(v.shape, np.float32)
    ctx.check(lib().fd_unit_norm_batch(ctx.h, _ptr(v), v.shape[0], int(np.prod(v.shape[1:])), norm_type, _ptr(out)))
    return out


# ---- integral-image features on sampled windows (HaarFeatureFilter, IntegralGradientFilter, GradientSumFilter, the SURF-like chain)
class _HaarParams:
    """fd_haar_params with the arrays it points to; grid: the (sizes, xCount, yCount, types) constructors' equidistant grid"""

    def __init__(self, sizes=(0.2, 0.4), xs=None, ys=None, types=HAAR_ALL, grid=(5, 5)):
        self.sizes = _c(sizes, np.float32).ravel()
        self.xs = haar_grid(grid[0]) if xs is None else _c(xs, np.float32).ravel()
        self.ys = (haar_grid(grid[1]) if xs is None else self.xs) if ys is None else _c(ys, np.float32).ravel()
        fp = C.POINTER(C.c_float)
        self.c = fd_haar_params(self.sizes.ctypes.data_as(fp), len(self.sizes), self.xs.ctypes.data_as(fp), len(self.xs),
                                self.ys.ctypes.data_as(fp), len(self.ys), int(types))


def haar_params(sizes=(0.2, 0.4), xs=None, ys=None, types=HAAR_ALL, grid=(5, 5)):
    """HaarFeatureFilter's constructors: explicit centre coordinates xs (ys defaults to xs), or an equidistant grid of grid = (xCount,
    yCount) points; the defaults are the default constructor's"""
    return _HaarParams(sizes, xs, ys, types, grid)


def haar_grid(count):
    out = np.empty(max(count, 0), np.float32)
    if lib().fd_haar_grid(count, _ptr(out)) != FD_OK:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "fd_haar_grid: invalid count %d" % count)
    return out


def haar_feature_count(hp):
    n = lib().fd_haar_feature_count(C.byref(hp.c) if hp is not None else None)
    if n < 0:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "HaarFeatureFilter: invalid parameters")
    return n


def haar_features(hp):
    """the feature table of HaarFeatureFilter::buildFeatures as a HAAR_FEATURE_DTYPE array"""
    out = np.zeros(haar_feature_count(hp), HAAR_FEATURE_DTYPE)
    cnt = C.c_int()
    rc = lib().fd_haar_features(C.byref(hp.c), _ptr(out), len(out), C.byref(cnt))
    if rc != FD_OK:
        raise FdError(rc, "fd_haar_features")
    return out[:cnt.value]


def surf_feature_length(gradient_count, cell_count):
    """length of the fused SURF descriptor, 4 * cell_count^2 (host only); FdError where fd_integral_extract_surf rejects the pair"""
    n = lib().fd_surf_feature_length(gradient_count, cell_count)
    if n < 0:
        raise FdError(FD_ERR_INVALID_ARGUMENT, "fd_integral_extract_surf: invalid gradient count %d / cell count %d" % (gradient_count, cell_count))
    return n


def integral_hog_params(rows, cols=None, bins=9, signed_gradients=False, interpolate_bins=False, hist=None, ehog=None):
    """fd_integral_hog_params: IntegralGradientFilter(rows, cols) -> GradientBinningFilter(bins, signed_gradients, interpolate_bins) ->
    hist (a fd_hist_params: one of the four HIST_* patch filters) or ehog (a fd_ehog_patch_params: ExtendedHogFilter)"""
    if (hist is None) == (ehog is None):
        raise ValueError("exactly one of hist and ehog")
    p = fd_integral_hog_params()
    p.grad_rows, p.grad_cols = int(rows), int(rows if cols is None else cols)
    p.bins, p.signed_gradients, p.interpolate_bins = int(bins), int(signed_gradients), int(interpolate_bins)
    if hist is not None:
        p.kind, p.hist = FD_SAMPLES_HIST, hist
    else:
        p.kind, p.ehog = FD_SAMPLES_EHOG, ehog
    return p


def integral_hog_feature_length(hp):
    """floats per sample of Integral.extract_hog (host only); -1 where the call is refused"""
    return lib().fd_integral_hog_feature_length(C.byref(hp) if hp is not None else None)


def integral_gradient_samples_valid(width, height, rows, cols, samples):
    """which samples of a width x height image IntegralGradientFilter(rows, cols) can serve (host only) -> bool[n]"""
    s = _c(samples, np.int32).reshape(-1, 4)
    valid = np.zeros(len(s), np.uint8)
    rc = lib().fd_integral_gradient_samples_valid(width, height, rows, cols, len(s), _ptr(s), _ptr(valid))
    if rc != FD_OK:
        raise FdError(rc, "fd_integral_gradient_samples_valid: invalid image size %d x %d or grid %d x %d" % (width, height, rows, cols))
    return valid.astype(bool)


def integral_image(ctx, gray):
    g = _c(gray, np.uint8)
    out = np.empty((g.shape[0] + 1, g.shape[1] + 1), np.int32)
    ctx.check(lib().fd_integral_image(ctx.h, _ptr(g), g.shape[1], g.shape[0], _ptr(out)))
    return out


def gradient_sum_batch(ctx, grad2ch, cell_rows, cell_cols=None):
    """GradientSumFilter on [n, rows, cols, 2] u8 gradient patches -> [n, cell_rows * cell_cols * 4] f32"""
    g = _c(grad2ch, np.uint8)
    cell_cols = cell_rows if cell_cols is None else cell_cols
    n, rows, cols = g.shape[:3]
    out = np.empty((n, max(cell_rows, 0) * max(cell_cols, 0) * 4), np.float32)
    ctx.check(lib().fd_gradient_sum_batch(ctx.h, _ptr(g), n, rows, cols, cell_rows, cell_cols, _ptr(out)))
    return out


def _integral_kind(haar=None, surf=None, hog=None, kind=None):
    """(FD_INTEGRAL_* kind, pointer to its parameters, the object the pointer needs alive) of exactly one of haar, surf and hog"""
    given = [k for k, v in (("haar", haar), ("surf", surf), ("hog", hog)) if v is not None]
    if len(given) != 1 or (kind is not None and kind != given[0]):
        raise ValueError("exactly one of haar, surf and hog (and kind, when given, names it)")
    if haar is not None:
        return INTEGRAL_HAAR, C.byref(haar.c), haar
    if hog is not None:
        return INTEGRAL_HOG, C.byref(hog), hog
    sp = fd_surf_params(int(surf[0]), int(surf[1]))
    return INTEGRAL_SURF, C.byref(sp), sp


class Integral:
    """fd_integral: the integral image of a frame and the patch filters of a DirectImageFeatureExtractor on sampled windows.
    samples: (n, 4) {x, y, width, height}; every extraction returns (rows, valid bool[n])."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx.check(lib().fd_integral_create(ctx.h, C.byref(self.h)))

    def _check(self, rc):   # fd_integral_update / _download report through the handle's context
        self.ctx.check(rc)

    def update(self, image):
        img = _c(image, np.uint8)
        ch = 1 if img.ndim == 2 else img.shape[2]
        self._check(lib().fd_integral_update(self.h, _ptr(img), img.shape[1], img.shape[0], ch, 0))

    def update_device(self, dev_ptr, w, h, ch):
        self._check(lib().fd_integral_update(self.h, C.c_void_p(dev_ptr), w, h, ch, 1))

    def set_image(self, integral):
        """an integral image made elsewhere ((h + 1) x (w + 1) int32) instead of an update"""
        I = _c(integral, np.int32)
        self._check(lib().fd_integral_set_image(self.h, _ptr(I), I.shape[1], I.shape[0]))

    def size(self):
        w, h = C.c_int(), C.c_int()
        lib().fd_integral_size(self.h, C.byref(w), C.byref(h))
        return w.value, h.value

    def download(self):
        w, h = self.size()
        out = np.empty((h, w), np.int32)
        self._check(lib().fd_integral_download(self.h, _ptr(out)))
        return out

    @staticmethod
    def _samples(samples):
        return _c(samples, np.int32).reshape(-1, 4)

    def extract_haar(self, hp, samples, download=True):
        s = self._samples(samples)
        feats = np.empty((len(s), haar_feature_count(hp)), np.float32) if download else None
        valid = np.zeros(len(s), np.uint8) if download else None
        self.ctx.check(lib().fd_integral_extract_haar(self.ctx.h, self.h, C.byref(hp.c), len(s), _ptr(s), _ptr(feats), _ptr(valid)))
        return (feats, valid.astype(bool)) if download else None

    def gradient_patches(self, rows, cols, samples):
        s = self._samples(samples)
        out = np.empty((len(s), max(rows, 0), max(cols, 0), 2), np.uint8)
        valid = np.zeros(len(s), np.uint8)
        self.ctx.check(lib().fd_integral_gradient_patches(self.ctx.h, self.h, rows, cols, len(s), _ptr(s), _ptr(out), _ptr(valid)))
        return out, valid.astype(bool)

    def extract_surf(self, gradient_count, cell_count, samples, download=True):
        s = self._samples(samples)
        feats = np.empty((len(s), 4 * max(cell_count, 0) ** 2), np.float32) if download else None
        valid = np.zeros(len(s), np.uint8) if download else None
        self.ctx.check(lib().fd_integral_extract_surf(self.ctx.h, self.h, gradient_count, cell_count, len(s), _ptr(s), _ptr(feats), _ptr(valid)))
        return (feats, valid.astype(bool)) if download else None

    def extract_hog(self, hp, samples, download=True):
        """the integral HOG family (integral_hog_params) in one launch"""
        s = self._samples(samples)
        feats = np.empty((len(s), max(integral_hog_feature_length(hp), 0)), np.float32) if download else None
        valid = np.zeros(len(s), np.uint8) if download else None
        self.ctx.check(lib().fd_integral_extract_hog(self.ctx.h, self.h, C.byref(hp), len(s), _ptr(s), _ptr(feats), _ptr(valid)))
        return (feats, valid.astype(bool)) if download else None

    def svm_evaluate_samples(self, svm, samples, haar=None, surf=None, hog=None, kind=None):
        """condensation::SingleClassifierModel::evaluate: haar = haar_params(...), surf = (gradient_count, cell_count) or
        hog = integral_hog_params(...) -> (target bool[n], weight f64[n]).  kind ("haar" | "surf" | "hog"), when given, must name
        the argument that is set."""
        s = self._samples(samples)
        target = np.zeros(len(s), np.uint8)
        weight = np.zeros(len(s), np.float64)
        kind, prm, _keep = _integral_kind(haar, surf, hog, kind)
        self.ctx.check(lib().fd_integral_svm_evaluate_samples(self.ctx.h, self.h, kind, prm, svm.h, len(s), _ptr(s), _ptr(target), _ptr(weight)))
        return target.astype(bool), weight

    def close(self):
        if getattr(self, "h", None):
            lib().fd_integral_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):   # a handle nobody holds any more gives its device memory back (hipFree waits for the device)
        try:
            self.close()
        except Exception:
            pass


class HogSvmRun:
    """fd_detect_hog_svm_begin / _end: the frame's kernels and read-back are queued by the constructor, end() collects the detections."""

    def __init__(self, ctx, pyr, svm, hp, cap=1 << 14):
        self.ctx, self.cap = ctx, cap
        self._keep = (pyr, svm)
        self.ticket = C.c_void_p()
        ctx.check(lib().fd_detect_hog_svm_begin(ctx.h, pyr.h, svm.h, C.byref(hp), C.byref(self.ticket)))

    def end(self):
        out = np.empty(self.cap, DET_DTYPE)
        cnt = C.c_int64()
        t, self.ticket = self.ticket, C.c_void_p()
        self.ctx.check(lib().fd_detect_hog_svm_end(self.ctx.h, t, _ptr(out), out.shape[0], C.byref(cnt)))
        return out[:cnt.value].copy()


class Sdm:
    def __init__(self, ctx, model):
        self.ctx = ctx
        self.model = model
        L, S = int(model["L"]), int(model["S"])
        self._mean = _c(model["mean"], np.float32)
        self._R = [_c(r, np.float32) for r in model["R"]]
        ptrs = (C.POINTER(C.c_float) * S)(*[r.ctypes.data_as(C.POINTER(C.c_float)) for r in self._R])
        rows = _c([r.shape[0] for r in self._R], np.int32)
        s = fd_sdm_model()
        s.num_landmarks, s.num_steps = L, S
        s.mean = self._mean.ctypes.data_as(C.POINTER(C.c_float))
        s.R = C.cast(ptrs, C.POINTER(C.POINTER(C.c_float)))
        s.R_rows = rows.ctypes.data_as(C.POINTER(C.c_int32))
        s.hog_variant = int(model["variant"])
        # per step {numCells, cellSize, numBins}: the non-adaptive branch of optimize() (SdmLandmarkModel.hpp:236-238,246-248)
        self._dp = _c(model["desc_params"], np.int32) if model.get("desc_params") is not None else None
        if self._dp is not None:
            assert self._dp.size == 3 * S
            s.desc_params = self._dp.ctypes.data_as(C.POINTER(C.c_int32))
        self.h = C.c_void_p()
        ctx.check(lib().fd_sdm_create(ctx.h, C.byref(s), C.byref(self.h)))
        self.L, self.S = L, S

    def fit(self, gray_images, face_boxes):
        """gray_images: [B,H,W] u8; face_boxes: [B,4] (x,y,w,h).  Returns (shapes [B,2L], status [B])."""
        imgs = _c(gray_images, np.uint8)
        B, H, W = imgs.shape
        fb = _c(face_boxes, np.int32).reshape(B, 4)
        out = np.empty((B, 2 * self.L), np.float32)
        st = np.zeros(B, np.int32)
        self.ctx.check(lib().fd_sdm_fit_batch(self.ctx.h, self.h, _ptr(imgs), W, H, B, _ptr(fb), 0, _ptr(out), _ptr(st)))
        return out, st

    def fit_device(self, dev_ptr, W, H, B, face_boxes):
        fb = _c(face_boxes, np.int32).reshape(B, 4)
        out = np.empty((B, 2 * self.L), np.float32)
        st = np.zeros(B, np.int32)
        self.ctx.check(lib().fd_sdm_fit_batch(self.ctx.h, self.h, C.c_void_p(dev_ptr), W, H, B, _ptr(fb), 1, _ptr(out), _ptr(st)))
        return out, st

    def fit_device_begin(self, dev_ptr, W, H, B, face_boxes):
        """fd_sdm_fit_batch_begin on images resident in HBM: returns a ticket for fit_end; several can be in flight"""
        fb = _c(face_boxes, np.int32).reshape(B, 4)
        t = C.c_void_p()
        self.ctx.check(lib().fd_sdm_fit_batch_begin(self.ctx.h, self.h, C.c_void_p(dev_ptr), W, H, B, _ptr(fb), 1, C.byref(t)))
        return (t, B, fb)

    def fit_begin(self, gray_images, face_boxes):
        imgs = _c(gray_images, np.uint8)
        B, H, W = imgs.shape
        fb = _c(face_boxes, np.int32).reshape(B, 4)
        t = C.c_void_p()
        self.ctx.check(lib().fd_sdm_fit_batch_begin(self.ctx.h, self.h, _ptr(imgs), W, H, B, _ptr(fb), 0, C.byref(t)))
        return (t, B, (fb, imgs))   # host images stay alive with the ticket

    def fit_end(self, ticket):
        t, B, _keep = ticket
        out = np.empty((B, 2 * self.L), np.float32)
        st = np.zeros(B, np.int32)
        self.ctx.check(lib().fd_sdm_fit_batch_end(self.ctx.h, t, _ptr(out), _ptr(st)))
        return out, st

    def optimize(self, gray_images, shapes):
        """fd_sdm_optimize_batch: gray_images [B,H,W] u8, shapes [B,2L] start shapes.  Returns (shapes [B,2L], status [B])."""
        imgs = _c(gray_images, np.uint8)
        B, H, W = imgs.shape
        out = _c(shapes, np.float32).reshape(B, 2 * self.L).copy()
        st = np.zeros(B, np.int32)
        self.ctx.check(lib().fd_sdm_optimize_batch(self.ctx.h, self.h, _ptr(imgs), W, H, B, 0, _ptr(out), _ptr(st)))
        return out, st

    def close(self):
        if getattr(self, "h", None):
            lib().fd_sdm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):   # a handle nobody holds any more gives its device memory back (hipFree waits for the device)
        try:
            self.close()
        except Exception:
            pass


def sdm_descriptors(ctx, gray, px, py, wsh, variant=1, num_cells=3, cell_size=10, num_bins=9):
    gray = _c(gray, np.uint8)
    px, py = _c(px, np.float32), _c(py, np.float32)
    n = len(px)
    ln = C.c_int()
    ctx.check(lib().fd_sdm_descriptors(ctx.h, _ptr(gray), gray.shape[1], gray.shape[0], _ptr(px), _ptr(py), n, wsh, variant, num_cells,
                                       cell_size, num_bins, None, C.byref(ln)))
    out = np.empty((n, ln.value), np.float32)
    ctx.check(lib().fd_sdm_descriptors(ctx.h, _ptr(gray), gray.shape[1], gray.shape[0], _ptr(px), _ptr(py), n, wsh, variant, num_cells,
                                       cell_size, num_bins, _ptr(out), C.byref(ln)))
    return out


def _sdm_train_params(L, desc_params, variant, regularisation, lam, regularise_affine):
    dp = _c(desc_params, np.int32).reshape(-1)
    assert dp.size % 3 == 0 and dp.size > 0
    p = fd_sdm_train_params()
    p.num_landmarks, p.num_steps, p.hog_variant = int(L), dp.size // 3, int(variant)
    p.desc_params = dp.ctypes.data_as(C.POINTER(C.c_int32))
    p.regularisation, p.lambda_, p.regularise_affine = int(regularisation), float(lam), int(bool(regularise_affine))
    return p, dp


def sdm_train_limits(L, desc_params, rows, variant=1):
    """fd_sdm_train_limits (host only): (device bytes the trainer keeps resident, largest D of the steps)"""
    p, _keep = _sdm_train_params(L, desc_params, variant, SDM_REG_AUTOMATIC, 0.5, True)
    b, m = C.c_int64(), C.c_int()
    rc = lib().fd_sdm_train_limits(C.byref(p), int(rows), C.byref(b), C.byref(m))
    if rc != FD_OK:
        raise FdError(rc, "fd_sdm_train_limits: invalid parameters")
    return b.value, m.value


def sdm_linear_regression(ctx, A, b, regularisation=SDM_REG_AUTOMATIC, lam=0.5, regularise_affine=True, want_normal_equations=False):
    """fd_sdm_linear_regression: x [D,N] float32 and lambda; with want_normal_equations also AtA [D,D] and Atb [D,N] (float64)"""
    A, b = _c(A, np.float32), _c(b, np.float32)
    M, D = A.shape
    N = b.shape[1]
    assert b.shape[0] == M
    x, lo = np.zeros((D, N), np.float32), C.c_double()
    ata = np.zeros((D, D), np.float64) if want_normal_equations else None
    atb = np.zeros((D, N), np.float64) if want_normal_equations else None
    ctx.check(lib().fd_sdm_linear_regression(ctx.h, _ptr(A), _ptr(b), M, D, N, int(regularisation), float(lam), int(bool(regularise_affine)),
                                             _ptr(x), C.byref(lo), _ptr(ata), _ptr(atb)))
    return (x, lo.value, ata, atb) if want_normal_equations else (x, lo.value)


def sdm_linear_regression_solution(ctx, D, N):
    """the double solution the last sdm_linear_regression on this context rounded to float"""
    x = np.zeros((D, N), np.float64)
    ctx.check(lib().fd_debug_sdm_linear_regression_solution(ctx.h, int(D), int(N), _ptr(x)))
    return x


def sdm_train_last_phase_ms(ctx):
    """fd_sdm_train_last_phase_ms: dict of the six phase times (ms) of the last timed step"""
    ms = np.zeros(6, np.float32)
    ctx.check(lib().fd_sdm_train_last_phase_ms(ctx.h, _ptr(ms)))
    return dict(zip(("descriptors", "gram", "norm", "cholesky", "substitution", "update"), ms.tolist()))


def sdm_train(ctx, groups, samples_per_image, initial_shapes, groundtruth, desc_params, variant=1, regularisation=SDM_REG_AUTOMATIC,
              lam=0.5, regularise_affine=True):
    """fd_sdm_train.  groups: list of [count,H,W] u8 arrays (images numbered through the groups in order); both shape arrays
    [images * samples_per_image, 2L], image-major.  Returns a dict: R (list of [D_s,2L]), shapes_steps [S+1,M,2L], row_status [M],
    info (list of S+1 dicts).  On FdError the exception carries row_status as .row_status."""
    x0, gt = _c(initial_shapes, np.float32), _c(groundtruth, np.float32)
    M, N = x0.shape
    L = N // 2
    assert gt.shape == x0.shape
    p, dp = _sdm_train_params(L, desc_params, variant, regularisation, lam, regularise_affine)
    S = p.num_steps
    # a group is a [count,H,W] u8 array, or (device pointer, count, H, W) for images resident in HBM
    imgs = [g if isinstance(g, tuple) else _c(g, np.uint8) for g in groups]
    arr = (fd_sdm_train_group * len(imgs))()
    for a, g in zip(arr, imgs):
        if isinstance(g, tuple):
            a.images, a.count, a.height, a.width, a.on_device = int(g[0]), int(g[1]), int(g[2]), int(g[3]), 1
        else:
            a.images, a.count, a.height, a.width, a.on_device = g.ctypes.data, g.shape[0], g.shape[1], g.shape[2], 0
    assert sum(a.count for a in arr) * samples_per_image == M
    dims = np.zeros(S, np.int32)
    rc = lib().fd_sdm_train_step_dims(C.byref(p), _ptr(dims))
    if rc != FD_OK:
        raise FdError(rc, "fd_sdm_train_step_dims: invalid parameters")
    R = [np.zeros((d, N), np.float32) for d in dims]
    ptrs = (C.c_void_p * S)(*[r.ctypes.data for r in R])
    steps = np.zeros((S + 1, M, N), np.float32)
    status = np.zeros(M, np.int32)
    info = (fd_sdm_train_step_info * (S + 1))()
    rc = lib().fd_sdm_train(ctx.h, C.byref(p), arr, len(imgs), int(samples_per_image), _ptr(x0), _ptr(gt), ptrs, _ptr(steps), _ptr(status), info)
    if rc != FD_OK:
        e = FdError(rc, lib().fd_last_error(ctx.h).decode())
        e.row_status, e.R = status, R
        raise e
    return dict(R=R, shapes_steps=steps, row_status=status,
                info=[dict(lam=i.lambda_, err_l1=i.err_l1, err_fro=i.err_fro, rows=i.rows, dim=i.dim, pivot_flag=i.pivot_flag) for i in info])
