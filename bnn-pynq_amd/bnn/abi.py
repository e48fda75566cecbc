"""ctypes binding of the runtime's C ABI (``include/bnn_mi355x.h``): the reference's six symbols
(``bnn/bnn.py:69-77`` binds the same ones through cffi) plus the ``bnn_mi355x_*`` extensions.
Used by ``bnn.py``, ``multigpu.py``, ``bench.py`` and the tests."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.realpath(__file__))
PLATFORM = os.environ.get("BNN_PLATFORM", "mi355x")
# BNN_MI355X_LIBDIR: kernel-tuning experiments point this at an alternative build of the same ABI
LIB_DIR = os.environ.get("BNN_MI355X_LIBDIR") or os.path.join(ROOT, "libraries", PLATFORM)
PARAM_ROOT = os.path.join(ROOT, "params")

LEGACY = ["load_parameters", "inference", "inference_multiple", "inference_multiple_with_faults",
          "free_results", "deinit"]
EXT = ["bnn_mi355x_network", "bnn_mi355x_image_bytes", "bnn_mi355x_last_error", "bnn_mi355x_set_device",
       "bnn_mi355x_pack_params", "bnn_mi355x_export_params", "bnn_mi355x_import_params",
       "bnn_mi355x_inference_buffer", "bnn_mi355x_inference_raw", "bnn_mi355x_inference_device",
       "bnn_mi355x_reserve", "bnn_mi355x_set_fault_seed", "bnn_mi355x_last_faults", "bnn_mi355x_plan_faults",
       "bnn_mi355x_pack_params_faulty", "bnn_mi355x_debug_stage_output", "bnn_mi355x_profile",
       "bnn_mi355x_profile_read", "bnn_mi355x_stage_name", "bnn_mi355x_thumbnail_size", "bnn_mi355x_images_to_cifar",
       "bnn_mi355x_params_bytes", "bnn_mi355x_import_params_device", "bnn_mi355x_params_crc", "bnn_mi355x_chunk_plan",
       "bnn_mi355x_binarize_pack", "bnn_mi355x_fault_campaigns", "bnn_mi355x_last_campaign_faults",
       "bnn_mi355x_enumerate_faults", "bnn_mi355x_fault_sweep", "bnn_mi355x_last_sweep_stages",
       "bnn_mi355x_enumerate_act_faults", "bnn_mi355x_act_fault_sweep", "bnn_mi355x_last_act_sweep_stages",
       "bnn_mi355x_matrix_stages", "bnn_mi355x_act_noise_campaigns", "bnn_mi355x_last_act_noise_counts",
       "bnn_mi355x_last_act_noise_seeds", "bnn_mi355x_act_noise_mask", "bnn_mi355x_enumerate_input_faults",
       "bnn_mi355x_input_fault_sweep", "bnn_mi355x_last_input_sweep_stages", "bnn_mi355x_input_noise_campaigns",
       "bnn_mi355x_last_input_noise_counts", "bnn_mi355x_last_input_noise_seeds", "bnn_mi355x_input_noise_mask",
       "bnn_mi355x_sweep_profile", "bnn_mi355x_last_sweep_profile", "bnn_mi355x_mem_noise_campaigns",
       "bnn_mi355x_last_mem_noise_counts", "bnn_mi355x_last_mem_noise_seeds", "bnn_mi355x_mem_noise_mask",
       "bnn_mi355x_mem_noise_params", "bnn_mi355x_hardening_scheme", "bnn_mi355x_hardening_layout", "bnn_mi355x_hardened_site",
       "bnn_mi355x_hardened_mem_noise_mask", "bnn_mi355x_pack_params_hardened", "bnn_mi355x_hardened_mem_noise_campaigns",
       "bnn_mi355x_hardened_mem_noise_params", "bnn_mi355x_last_hardened_mem_noise_counts",
       "bnn_mi355x_last_hardened_mem_noise_seeds", "bnn_mi355x_exposure_mask", "bnn_mi355x_exposure_campaigns",
       "bnn_mi355x_exposure_params", "bnn_mi355x_last_exposure_counts", "bnn_mi355x_last_exposure_seeds", "bnn_mi355x_ecc_encode",
       "bnn_mi355x_ecc_decode", "bnn_mi355x_ecc_layout", "bnn_mi355x_ecc_check_site", "bnn_mi355x_ecc_exposure_mask",
       "bnn_mi355x_pack_params_ecc", "bnn_mi355x_ecc_exposure_campaigns", "bnn_mi355x_ecc_exposure_params",
       "bnn_mi355x_last_ecc_exposure_counts", "bnn_mi355x_last_ecc_exposure_seeds", "bnn_mi355x_ecc_repair",
       "bnn_mi355x_pack_params_repair", "bnn_mi355x_repair_exposure_campaigns", "bnn_mi355x_repair_exposure_params",
       "bnn_mi355x_last_repair_exposure_counts", "bnn_mi355x_last_repair_exposure_seeds", "bnn_mi355x_wecc_encode",
       "bnn_mi355x_wecc_decode", "bnn_mi355x_wecc_repair", "bnn_mi355x_wecc_layout", "bnn_mi355x_wecc_exposure_mask",
       "bnn_mi355x_pack_params_wecc", "bnn_mi355x_wecc_exposure_campaigns", "bnn_mi355x_wecc_exposure_params",
       "bnn_mi355x_last_wecc_exposure_counts", "bnn_mi355x_last_wecc_exposure_seeds", "bnn_mi355x_iwecc_layout",
       "bnn_mi355x_iwecc_site", "bnn_mi355x_pack_params_iwecc", "bnn_mi355x_iwecc_exposure_campaigns",
       "bnn_mi355x_iwecc_exposure_params", "bnn_mi355x_last_iwecc_exposure_counts", "bnn_mi355x_last_iwecc_exposure_seeds",
       "bnn_mi355x_tile_boxes", "bnn_mi355x_windows_to_cifar", "bnn_mi355x_classify_windows", "bnn_mi355x_glyph_fit",
       "bnn_mi355x_resample_coeffs", "bnn_mi355x_enhance_picture", "bnn_mi355x_glyphs_to_mnist", "bnn_mi355x_classify_glyphs",
       "bnn_mi355x_find_glyphs_host", "bnn_mi355x_find_glyphs", "bnn_mi355x_read_glyphs", "bnn_mi355x_last_find_usec",
       "bnn_mi355x_order_lines", "bnn_mi355x_page_to_mnist", "bnn_mi355x_read_page", "bnn_mi355x_scan_grid",
       "bnn_mi355x_scan_boxes", "bnn_mi355x_scan_planes", "bnn_mi355x_scan_device", "bnn_mi355x_scan_scene",
       "bnn_mi355x_debug_scan_stage", "bnn_mi355x_scan_resize", "bnn_mi355x_scan_clip", "bnn_mi355x_scan_clip_capacity",
       "bnn_mi355x_scan_clip_layout", "bnn_mi355x_debug_scan_clip_stage", "bnn_mi355x_detect_windows_host",
       "bnn_mi355x_detect_windows", "bnn_mi355x_detect_clip", "bnn_mi355x_unpack_frames_host", "bnn_mi355x_unpack_frames",
       "bnn_mi355x_scan_clip_frames", "bnn_mi355x_detect_clip_frames", "bnn_mi355x_scan_clip_device", "bnn_mi355x_detect_clip_device"]

# bnn_mi355x_frames.format by name (include/bnn_mi355x.h, BNN_MI355X_FORMAT_*)
PIXEL_FORMATS = {"rgb": 0, "l": 1, "bgr": 2, "nv12": 3, "i420": 4, "yuyv": 5}


class Frames(C.Structure):
    """``bnn_mi355x_frames``"""
    _fields_ = [("format", C.c_int), ("range", C.c_int), ("width", C.c_int), ("height", C.c_int), ("n_frames", C.c_int),
                ("row_stride", C.c_long), ("frame_stride", C.c_long)]


class GlyphOpts(C.Structure):
    """``bnn_mi355x_glyph_opts``"""
    _fields_ = [("contrast", C.c_float), ("brightness", C.c_float), ("threshold", C.c_int), ("filter", C.c_int),
                ("square_blank", C.c_int)]


class FindOpts(C.Structure):
    """``bnn_mi355x_find_opts``"""
    _fields_ = [("ink_level", C.c_int), ("reach_x", C.c_int), ("reach_y", C.c_int), ("min_pixels", C.c_int), ("order", C.c_int)]


class PageOpts(C.Structure):
    """``bnn_mi355x_page_opts``"""
    _fields_ = [("mask", C.c_int), ("line_order", C.c_int), ("word_gap", C.c_int)]


class DetectOpts(C.Structure):
    """``bnn_mi355x_detect_opts``"""
    _fields_ = [("class_mask", C.c_uint64), ("by_score", C.c_int), ("min_score", C.c_int), ("iou_num", C.c_int), ("iou_den", C.c_int),
                ("max_candidates", C.c_int), ("max_det", C.c_int)]


def lib_path(network, runtime="python_sw", lib_dir=None):
    return os.path.join(lib_dir or LIB_DIR, "%s-%s-%s.so" % (runtime, network, PLATFORM))


def declare_legacy(L):
    """argument / return types of the reference's cdef"""
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.load_parameters.argtypes = [C.c_char_p]
    L.load_parameters.restype = None
    L.inference.argtypes = [C.c_char_p, ip, C.c_int, fp]
    L.inference.restype = C.c_int
    L.inference_multiple.argtypes = [C.c_char_p, C.c_int, ip, fp, C.c_int]
    L.inference_multiple.restype = ip
    L.inference_multiple_with_faults.argtypes = [C.c_char_p, C.c_int, ip, fp, C.c_uint, C.c_int, C.c_int, ip, C.c_uint]
    L.inference_multiple_with_faults.restype = ip
    L.free_results.argtypes = [ip]
    L.free_results.restype = None
    L.deinit.argtypes = []
    L.deinit.restype = None


def declare_extensions(L):
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.bnn_mi355x_network.restype = C.c_char_p
    L.bnn_mi355x_image_bytes.restype = C.c_int
    L.bnn_mi355x_last_error.restype = C.c_char_p
    L.bnn_mi355x_set_device.argtypes = [C.c_int]
    L.bnn_mi355x_pack_params.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    L.bnn_mi355x_pack_params.restype = C.c_size_t
    L.bnn_mi355x_export_params.argtypes = [C.c_void_p, C.c_size_t]
    L.bnn_mi355x_export_params.restype = C.c_size_t
    L.bnn_mi355x_import_params.argtypes = [C.c_void_p, C.c_size_t]
    L.bnn_mi355x_params_bytes.argtypes = []
    L.bnn_mi355x_params_bytes.restype = C.c_size_t
    L.bnn_mi355x_import_params_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.bnn_mi355x_params_crc.argtypes = []
    L.bnn_mi355x_params_crc.restype = C.c_uint
    L.bnn_mi355x_inference_buffer.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, C.c_int]
    L.bnn_mi355x_inference_buffer.restype = ip
    L.bnn_mi355x_inference_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, fp]
    L.bnn_mi355x_inference_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    L.bnn_mi355x_reserve.argtypes = [C.c_int]
    L.bnn_mi355x_chunk_plan.argtypes = [C.c_int, C.c_int, ip, C.c_int]
    if hasattr(L, "bnn_mi355x_matrix_stages"):  # (an older build of the same ABI under BNN_MI355X_LIBDIR lacks it)
        L.bnn_mi355x_matrix_stages.argtypes = [C.c_int]
        L.bnn_mi355x_matrix_stages.restype = C.c_int
    L.bnn_mi355x_binarize_pack.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.bnn_mi355x_set_fault_seed.argtypes = [C.c_ulonglong]
    L.bnn_mi355x_last_faults.argtypes = [ip, C.c_int]
    L.bnn_mi355x_plan_faults.argtypes = [C.c_ulonglong, C.c_int, C.c_uint, C.c_int, C.c_int, ip, C.c_uint, ip, C.c_int]
    L.bnn_mi355x_fault_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_ulonglong, C.c_uint, C.c_int, C.c_int, ip, C.c_uint,
                                             ip, fp]
    L.bnn_mi355x_fault_campaigns.restype = ip
    L.bnn_mi355x_last_campaign_faults.argtypes = [ip, C.c_int]
    L.bnn_mi355x_enumerate_faults.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, ip, C.c_int]
    L.bnn_mi355x_enumerate_faults.restype = C.c_long
    L.bnn_mi355x_fault_sweep.argtypes = [C.c_char_p, C.c_int, ip, C.c_int, ip, ip, C.c_long, ip, fp]
    L.bnn_mi355x_fault_sweep.restype = C.c_long
    L.bnn_mi355x_last_sweep_stages.argtypes = [C.POINTER(C.c_long), C.c_int]
    L.bnn_mi355x_enumerate_act_faults.argtypes = [C.c_int, C.c_long, ip, C.c_int]
    L.bnn_mi355x_enumerate_act_faults.restype = C.c_long
    L.bnn_mi355x_act_fault_sweep.argtypes = [C.c_char_p, C.c_int, ip, C.c_int, ip, ip, C.c_long, ip, fp]
    L.bnn_mi355x_act_fault_sweep.restype = C.c_long
    L.bnn_mi355x_last_act_sweep_stages.argtypes = [C.POINTER(C.c_long), C.c_int]
    if hasattr(L, "bnn_mi355x_act_noise_campaigns"):  # (an older build of the same ABI under BNN_MI355X_LIBDIR lacks them)
        L.bnn_mi355x_act_noise_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_ulonglong, C.POINTER(C.c_uint), C.c_int, ip, fp]
        L.bnn_mi355x_act_noise_campaigns.restype = ip
        L.bnn_mi355x_last_act_noise_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_act_noise_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
        L.bnn_mi355x_act_noise_mask.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_uint, C.c_long, ip, C.c_int]
        L.bnn_mi355x_act_noise_mask.restype = C.c_long
    if hasattr(L, "bnn_mi355x_input_noise_campaigns"):  # (likewise)
        L.bnn_mi355x_enumerate_input_faults.argtypes = [C.c_long, ip, C.c_int]
        L.bnn_mi355x_enumerate_input_faults.restype = C.c_long
        L.bnn_mi355x_input_fault_sweep.argtypes = [C.c_char_p, C.c_int, ip, C.c_int, ip, ip, C.c_long, ip, fp]
        L.bnn_mi355x_input_fault_sweep.restype = C.c_long
        L.bnn_mi355x_last_input_sweep_stages.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_input_noise_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_ulonglong, C.c_uint, ip, fp]
        L.bnn_mi355x_input_noise_campaigns.restype = ip
        L.bnn_mi355x_last_input_noise_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_input_noise_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
        L.bnn_mi355x_input_noise_mask.argtypes = [C.c_ulonglong, C.c_int, C.c_uint, C.c_long, ip, C.c_int]
        L.bnn_mi355x_input_noise_mask.restype = C.c_long
    if hasattr(L, "bnn_mi355x_sweep_profile"):  # (likewise)
        L.bnn_mi355x_sweep_profile.argtypes = [C.c_int]
        L.bnn_mi355x_last_sweep_profile.argtypes = [C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_long, ip]
        L.bnn_mi355x_last_sweep_profile.restype = C.c_long
    if hasattr(L, "bnn_mi355x_mem_noise_campaigns"):  # (likewise)
        up = C.POINTER(C.c_uint)
        L.bnn_mi355x_mem_noise_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, ip, fp]
        L.bnn_mi355x_mem_noise_campaigns.restype = ip
        L.bnn_mi355x_last_mem_noise_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_mem_noise_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
        L.bnn_mi355x_mem_noise_mask.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_uint, C.c_long, ip, C.c_int]
        L.bnn_mi355x_mem_noise_mask.restype = C.c_long
        L.bnn_mi355x_mem_noise_params.argtypes = [C.c_ulonglong, up, up, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_mem_noise_params.restype = C.c_size_t
    if hasattr(L, "bnn_mi355x_hardened_mem_noise_campaigns"):  # (likewise)
        up = C.POINTER(C.c_uint)
        L.bnn_mi355x_hardening_layout.argtypes = [C.c_int, C.c_int, ip]
        L.bnn_mi355x_hardened_site.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
        L.bnn_mi355x_hardened_mem_noise_mask.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_long, ip,
                                                         C.c_int]
        L.bnn_mi355x_hardened_mem_noise_mask.restype = C.c_long
        L.bnn_mi355x_pack_params_hardened.argtypes = [C.c_char_p, C.c_int, ip, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_pack_params_hardened.restype = C.c_size_t
        L.bnn_mi355x_hardened_mem_noise_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int,
                                                              ip, fp]
        L.bnn_mi355x_hardened_mem_noise_campaigns.restype = ip
        L.bnn_mi355x_hardened_mem_noise_params.argtypes = [C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_hardened_mem_noise_params.restype = C.c_size_t
        L.bnn_mi355x_last_hardened_mem_noise_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_hardened_mem_noise_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    if hasattr(L, "bnn_mi355x_exposure_campaigns"):  # (likewise)
        up = C.POINTER(C.c_uint)
        L.bnn_mi355x_exposure_mask.argtypes = [C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_long, ip,
                                               C.c_int]
        L.bnn_mi355x_exposure_mask.restype = C.c_long
        L.bnn_mi355x_exposure_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, C.c_int,
                                                    C.c_int, ip, fp]
        L.bnn_mi355x_exposure_campaigns.restype = ip
        L.bnn_mi355x_exposure_params.argtypes = [C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_exposure_params.restype = C.c_size_t
        L.bnn_mi355x_last_exposure_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_exposure_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    if hasattr(L, "bnn_mi355x_ecc_exposure_campaigns"):  # (likewise)
        up = C.POINTER(C.c_uint)
        L.bnn_mi355x_ecc_encode.argtypes = [C.c_uint]
        L.bnn_mi355x_ecc_encode.restype = C.c_uint
        L.bnn_mi355x_ecc_decode.argtypes = [C.c_uint, C.c_uint, up]
        L.bnn_mi355x_ecc_layout.argtypes = [C.c_int, C.c_int, C.c_int, ip]
        L.bnn_mi355x_ecc_check_site.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
        L.bnn_mi355x_ecc_exposure_mask.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                                                   C.c_long, ip, C.c_int]
        L.bnn_mi355x_ecc_exposure_mask.restype = C.c_long
        L.bnn_mi355x_pack_params_ecc.argtypes = [C.c_char_p, C.c_int, C.c_int, ip, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_pack_params_ecc.restype = C.c_size_t
        L.bnn_mi355x_ecc_exposure_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int,
                                                        C.c_int, C.c_int, ip, fp]
        L.bnn_mi355x_ecc_exposure_campaigns.restype = ip
        L.bnn_mi355x_ecc_exposure_params.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_size_t]
        L.bnn_mi355x_ecc_exposure_params.restype = C.c_size_t
        L.bnn_mi355x_last_ecc_exposure_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_ecc_exposure_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    if hasattr(L, "bnn_mi355x_repair_exposure_campaigns"):  # (likewise)
        up = C.POINTER(C.c_uint)
        L.bnn_mi355x_ecc_repair.argtypes = [C.c_uint, C.c_uint, up, up]
        L.bnn_mi355x_pack_params_repair.argtypes = [C.c_char_p, C.c_int, C.c_int, ip, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_pack_params_repair.restype = C.c_size_t
        L.bnn_mi355x_repair_exposure_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up,
                                                           C.c_int, C.c_int, C.c_int, C.c_int, ip, fp]
        L.bnn_mi355x_repair_exposure_campaigns.restype = ip
        L.bnn_mi355x_repair_exposure_params.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, C.c_int, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_size_t]
        L.bnn_mi355x_repair_exposure_params.restype = C.c_size_t
        L.bnn_mi355x_last_repair_exposure_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_repair_exposure_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    if hasattr(L, "bnn_mi355x_wecc_exposure_campaigns"):  # (likewise)
        up = C.POINTER(C.c_uint)
        ullp = C.POINTER(C.c_ulonglong)
        L.bnn_mi355x_wecc_encode.argtypes = [C.c_ulonglong]
        L.bnn_mi355x_wecc_encode.restype = C.c_uint
        L.bnn_mi355x_wecc_decode.argtypes = [C.c_ulonglong, C.c_uint, ullp]
        L.bnn_mi355x_wecc_repair.argtypes = [C.c_ulonglong, C.c_uint, ullp, up]
        L.bnn_mi355x_wecc_layout.argtypes = [C.c_int, C.c_int, ip]
        L.bnn_mi355x_wecc_exposure_mask.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_uint, C.c_long, ip, C.c_int]
        L.bnn_mi355x_wecc_exposure_mask.restype = C.c_long
        L.bnn_mi355x_pack_params_wecc.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_pack_params_wecc.restype = C.c_size_t
        L.bnn_mi355x_wecc_exposure_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, up,
                                                         up, C.c_int, C.c_int, C.c_int, C.c_int, ip, fp]
        L.bnn_mi355x_wecc_exposure_campaigns.restype = ip
        L.bnn_mi355x_wecc_exposure_params.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_wecc_exposure_params.restype = C.c_size_t
        L.bnn_mi355x_last_wecc_exposure_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_wecc_exposure_seeds.argtypes = [ullp, C.c_int]
    if hasattr(L, "bnn_mi355x_iwecc_exposure_campaigns"):  # (likewise)
        up = C.POINTER(C.c_uint)
        L.bnn_mi355x_iwecc_layout.argtypes = [C.c_int, C.c_int, C.c_int, ip]
        L.bnn_mi355x_iwecc_site.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.POINTER(C.c_long)]
        L.bnn_mi355x_pack_params_iwecc.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_pack_params_iwecc.restype = C.c_size_t
        L.bnn_mi355x_iwecc_exposure_campaigns.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong,
                                                          up, up, C.c_int, C.c_int, C.c_int, C.c_int, ip, fp]
        L.bnn_mi355x_iwecc_exposure_campaigns.restype = ip
        L.bnn_mi355x_iwecc_exposure_params.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, up, up, C.c_int, C.c_int,
                                                       C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_iwecc_exposure_params.restype = C.c_size_t
        L.bnn_mi355x_last_iwecc_exposure_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bnn_mi355x_last_iwecc_exposure_seeds.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    L.bnn_mi355x_pack_params_faulty.argtypes = [C.c_char_p, ip, C.c_int, C.c_void_p, C.c_size_t]
    L.bnn_mi355x_pack_params_faulty.restype = C.c_size_t
    L.bnn_mi355x_debug_stage_output.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.bnn_mi355x_debug_stage_output.restype = C.c_long
    L.bnn_mi355x_profile.argtypes = [C.c_int]
    L.bnn_mi355x_profile_read.argtypes = [fp, C.c_int, ip]
    L.bnn_mi355x_stage_name.argtypes = [C.c_int]
    L.bnn_mi355x_stage_name.restype = C.c_char_p
    L.bnn_mi355x_thumbnail_size.argtypes = [C.c_int, C.c_int, ip, ip]
    L.bnn_mi355x_images_to_cifar.argtypes = [C.POINTER(C.c_void_p), ip, ip, ip, C.POINTER(C.c_long), C.c_int, C.c_void_p]
    if hasattr(L, "bnn_mi355x_classify_windows"):  # (an older build of the same ABI under BNN_MI355X_LIBDIR lacks them)
        L.bnn_mi355x_tile_boxes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
        L.bnn_mi355x_tile_boxes.restype = C.c_long
        L.bnn_mi355x_windows_to_cifar.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
        L.bnn_mi355x_classify_windows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_int, fp, fp,
                                                  C.c_int]
        L.bnn_mi355x_classify_windows.restype = ip
    if hasattr(L, "bnn_mi355x_classify_glyphs"):  # (likewise)
        op = C.POINTER(GlyphOpts)
        L.bnn_mi355x_glyph_fit.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.bnn_mi355x_resample_coeffs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.bnn_mi355x_enhance_picture.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, op, C.c_void_p, ip]
        L.bnn_mi355x_glyphs_to_mnist.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, op, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        L.bnn_mi355x_classify_glyphs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, op, C.c_int, fp, fp,
                                                 C.c_void_p]
        L.bnn_mi355x_classify_glyphs.restype = ip
    if hasattr(L, "bnn_mi355x_read_glyphs"):  # (likewise)
        op, fo = C.POINTER(GlyphOpts), C.POINTER(FindOpts)
        L.bnn_mi355x_find_glyphs_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, fo, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.bnn_mi355x_find_glyphs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, op, fo, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int]
        L.bnn_mi355x_read_glyphs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, op, fo, C.c_int, C.c_int, ip, C.c_void_p, fp, fp,
                                             C.c_void_p]
        L.bnn_mi355x_read_glyphs.restype = ip
        L.bnn_mi355x_last_find_usec.argtypes = []
        L.bnn_mi355x_last_find_usec.restype = C.c_float
    if hasattr(L, "bnn_mi355x_read_page"):  # (likewise)
        op, fo, po = C.POINTER(GlyphOpts), C.POINTER(FindOpts), C.POINTER(PageOpts)
        L.bnn_mi355x_order_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bnn_mi355x_page_to_mnist.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, op, fo, po, C.c_int, ip, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
        L.bnn_mi355x_read_page.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, op, fo, po, C.c_int, C.c_int, ip, C.c_void_p,
                                           C.c_void_p, C.c_void_p, fp, fp, C.c_void_p]
        L.bnn_mi355x_read_page.restype = ip
    if hasattr(L, "bnn_mi355x_scan_scene"):  # (likewise)
        L.bnn_mi355x_scan_grid.argtypes = [C.c_int, C.c_int, ip, ip]
        L.bnn_mi355x_scan_boxes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, ip, ip]
        L.bnn_mi355x_scan_boxes.restype = C.c_long
        L.bnn_mi355x_scan_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, ip, fp, C.c_int]
        L.bnn_mi355x_scan_planes.restype = ip
        L.bnn_mi355x_scan_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bnn_mi355x_scan_scene.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_void_p, fp, fp,
                                            C.c_int]
        L.bnn_mi355x_scan_scene.restype = ip
        L.bnn_mi355x_debug_scan_stage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, ip, ip]
        L.bnn_mi355x_debug_scan_stage.restype = C.c_long
        L.bnn_mi355x_scan_resize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "bnn_mi355x_scan_clip"):  # (likewise)
        L.bnn_mi355x_scan_clip.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, fp, fp, C.c_int]
        L.bnn_mi355x_scan_clip.restype = ip
        L.bnn_mi355x_scan_clip_capacity.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.bnn_mi355x_scan_clip_layout.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        L.bnn_mi355x_debug_scan_clip_stage.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int,
                                                       C.c_int, C.c_void_p, C.c_size_t]
        L.bnn_mi355x_debug_scan_clip_stage.restype = C.c_long
    if hasattr(L, "bnn_mi355x_detect_clip"):  # (likewise)
        do = C.POINTER(DetectOpts)
        L.bnn_mi355x_detect_windows_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, do, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bnn_mi355x_detect_windows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, do, C.c_void_p, C.c_void_p, C.c_void_p, fp]
        L.bnn_mi355x_detect_clip.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_int, do,
                                             C.c_void_p, C.c_void_p, C.c_void_p, fp, fp, fp]
    if hasattr(L, "bnn_mi355x_detect_clip_frames"):  # (likewise)
        do, fr = C.POINTER(DetectOpts), C.POINTER(Frames)
        L.bnn_mi355x_unpack_frames_host.argtypes = [fr, C.c_void_p, C.c_void_p]
        L.bnn_mi355x_unpack_frames.argtypes = [fr, C.c_void_p, C.c_void_p, fp]
        L.bnn_mi355x_scan_clip_frames.argtypes = [fr, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, fp, fp, C.c_int]
        L.bnn_mi355x_scan_clip_frames.restype = ip
        L.bnn_mi355x_detect_clip_frames.argtypes = [fr, C.c_void_p, C.c_void_p, C.c_int, C.c_int, do, C.c_void_p, C.c_void_p, C.c_void_p, fp, fp, fp]
        L.bnn_mi355x_scan_clip_device.argtypes = [fr, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, fp, fp, C.c_int, C.c_void_p]
        L.bnn_mi355x_scan_clip_device.restype = ip
        L.bnn_mi355x_detect_clip_device.argtypes = [fr, C.c_void_p, C.c_void_p, C.c_int, C.c_int, do, C.c_void_p, C.c_void_p, C.c_void_p, fp, fp, fp,
                                                    C.c_void_p]


_cache = {}


def load(network, runtime="python_sw", lib_dir=None):
    return load_path(lib_path(network, runtime, lib_dir))


def load_path(path):
    """dlopen once per process and path (like the reference's _libraries cache) and declare the ABI"""
    if path in _cache:
        return _cache[path]
    if not os.path.exists(path):
        raise RuntimeError("runtime library %s not found: build it with `make -C bnn-pynq_amd` "
                           "(the MI355X runtime has no CPU fallback)" % path)
    L = C.CDLL(path)
    declare_legacy(L)
    L.has_extensions = hasattr(L, "bnn_mi355x_inference_buffer")
    if L.has_extensions:
        declare_extensions(L)
    _cache[path] = L
    return L
