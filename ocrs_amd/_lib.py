"""ctypes binding of libocrs_amd.so (include/ocrs_amd.h).

The library is the product: there is NO Python/CPU fallback.  If the shared
object is missing or no GPU is visible, calls fail loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OCRS_AMD_LIB: an ablation build of the same library (ocrs_amd.build --variant), for A/B timing only
LIB_PATH = os.environ.get("OCRS_AMD_LIB") or os.path.join(_HERE, "libocrs_amd.so")

OCRS_OK = 0
STATUS_NAMES = {
    0: "OK", 1: "INVALID_ARGUMENT", 2: "MODEL_NOT_LOADED", 3: "MODEL_DIMS", 4: "RUN_FAILED", 5: "WRONG_OUTPUT",
    6: "IMAGE_SOURCE", 7: "DEVICE", 8: "IO", 9: "CAPACITY",
}

RUN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.POINTER(C.c_float)),
                     C.POINTER(C.c_int64), C.POINTER(C.c_int))


class EngineParams(C.Structure):
    _fields_ = [("detection_model", C.c_void_p), ("recognition_model", C.c_void_p), ("debug", C.c_int),
                ("decode_method", C.c_int), ("beam_width", C.c_uint32), ("alphabet", C.c_char_p),
                ("allowed_chars", C.c_char_p), ("numerics", C.c_int), ("coalesce", C.c_int), ("coalesce_pages", C.c_int),
                ("coalesce_window_us", C.c_int), ("layout_threads", C.c_int), ("rec_max_pixels", C.c_int64)]


class GroupParams(C.Structure):
    _fields_ = [("detection_model", C.c_void_p), ("detection_model_len", C.c_size_t), ("recognition_model", C.c_void_p),
                ("recognition_model_len", C.c_size_t), ("devices", C.POINTER(C.c_int)), ("n_devices", C.c_size_t),
                ("debug", C.c_int), ("decode_method", C.c_int), ("beam_width", C.c_uint32), ("alphabet", C.c_char_p),
                ("allowed_chars", C.c_char_p), ("gather", C.c_int), ("numerics", C.c_int), ("coalesce", C.c_int),
                ("coalesce_pages", C.c_int), ("coalesce_window_us", C.c_int), ("layout_threads", C.c_int), ("rec_max_pixels", C.c_int64),
                ("min_block", C.c_int), ("shared_block", C.c_int)]


class RunOptions(C.Structure):
    _fields_ = [("timing", C.c_int)]


class TextCharC(C.Structure):
    _fields_ = [("ch", C.c_uint32), ("top", C.c_int32), ("left", C.c_int32), ("bottom", C.c_int32),
                ("right", C.c_int32)]


class OcrsError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status
        self.status_name = STATUS_NAMES.get(status, str(status))


# Every symbol include/ocrs_amd.h declares (tests check they are all exported).
DECLARED_SYMBOLS = [
    "ocrs_last_error", "ocrs_buffer_free", "ocrs_device_count", "ocrs_set_device", "ocrs_set_option", "ocrs_ctc_beam_search", "ocrs_model_load_file",
    "ocrs_model_load_bytes", "ocrs_model_from_callback", "ocrs_model_input_shape", "ocrs_model_run",
    "ocrs_model_flops", "ocrs_model_free", "ocrs_engine_new", "ocrs_engine_free", "ocrs_image_source_check_bytes",
    "ocrs_engine_prepare_input", "ocrs_engine_prepare_input_device", "ocrs_page_free", "ocrs_page_dims",
    "ocrs_page_image", "ocrs_engine_detect_words", "ocrs_engine_detect_words_batch",
    "ocrs_engine_detect_text_pixels", "ocrs_engine_detection_threshold", "ocrs_engine_find_text_lines",
    "ocrs_engine_find_text_lines_batch",
    "ocrs_engine_recognize_text", "ocrs_engine_recognize_text_batch", "ocrs_engine_recognize_tokens",
    "ocrs_engine_prepare_recognition_input", "ocrs_text_item_rotated_rect", "ocrs_rotated_rect_corners", "ocrs_engine_get_text", "ocrs_device_malloc", "ocrs_device_free",
    "ocrs_device_upload", "ocrs_device_synchronize", "ocrs_device_measure_peaks", "ocrs_engine_enable_timing", "ocrs_stage_count",
    "ocrs_stage_name", "ocrs_engine_stage_times", "ocrs_kernel_class_count", "ocrs_kernel_class_name",
    "ocrs_engine_kernel_stats", "ocrs_engine_set_kernel_timing_mask", "ocrs_gru_tile_plan", "ocrs_host_malloc", "ocrs_host_free", "ocrs_engine_prepare_input_batch",
    "ocrs_get_device", "ocrs_model_load_file_on_device", "ocrs_model_load_bytes_on_device", "ocrs_model_device", "ocrs_engine_device",
    "ocrs_engine_group_new", "ocrs_engine_group_free", "ocrs_engine_group_size", "ocrs_engine_group_member", "ocrs_group_deal",
    "ocrs_group_prepare_input_batch", "ocrs_group_prepare_input_device_batch", "ocrs_group_detect_words_batch",
    "ocrs_group_recognize_text_batch", "ocrs_group_gather", "ocrs_group_final_gather", "ocrs_group_worker_threads", "ocrs_group_last_gather", "ocrs_device_malloc_on", "ocrs_engine_coalesce_stats", "ocrs_coalescer_selftest", "ocrs_stream_plan_selftest", "ocrs_conv_rows_selftest", "ocrs_engine_kernel_mfma_flops", "ocrs_engine_prepare_input_jpeg", "ocrs_jpeg_decode_rgb", "ocrs_jpeg_info", "ocrs_jpeg_coefficients",
    "ocrs_group_member_stats", "ocrs_numa_parse_cpulist", "ocrs_numa_bind_selftest", "ocrs_engine_recognize_logits", "ocrs_engine_set_option", "ocrs_engine_get_option", "ocrs_option_name", "ocrs_device_pool_stats", "ocrs_device_pool_configure", "ocrs_device_pool_trim",
    "ocrs_device_set_isolation", "ocrs_device_isolation", "ocrs_group_set_replay", "ocrs_abi_version",
    "ocrs_engine_recognize_text_scored", "ocrs_engine_recognize_text_batch_scored", "ocrs_ctc_beam_search_scored",
    "ocrs_engine_run_recognition_ops", "ocrs_ctc_decode_packed", "ocrs_mask_component_rects",
    "ocrs_engine_detect_words_scored", "ocrs_engine_detect_words_batch_scored", "ocrs_group_detect_words_batch_scored",
    "ocrs_engine_find_text_lines_indexed", "ocrs_engine_find_text_lines_batch_indexed",
    "ocrs_detection_tile_plan", "ocrs_engine_detect_words_tiled", "ocrs_engine_detect_words_batch_tiled",
    "ocrs_engine_detect_text_pixels_tiled", "ocrs_group_detect_words_batch_tiled",
    "ocrs_line_frame", "ocrs_line_char_boxes", "ocrs_engine_prepare_recognition_input_rectified",
    "ocrs_engine_recognize_text_rectified", "ocrs_engine_recognize_text_batch_rectified",
    "ocrs_group_recognize_text_batch_rectified", "ocrs_engine_recognize_tokens_rectified",
    "ocrs_engine_rotate_page", "ocrs_engine_rotate_pages", "ocrs_unrotate_rects", "ocrs_unrotate_chars",
    "ocrs_orientation_vote", "ocrs_engine_detect_orientation", "ocrs_engine_page_from_grey",
    "ocrs_engine_resize_page", "ocrs_engine_resize_pages", "ocrs_work_size", "ocrs_rescale_rects",
    "ocrs_engine_detect_words_at", "ocrs_engine_detect_words_batch_at",
    "ocrs_normalize_params_default", "ocrs_normalize_params_check", "ocrs_engine_normalize_page", "ocrs_engine_normalize_pages",
    "ocrs_skew_params_default", "ocrs_skew_params_check", "ocrs_skew_table", "ocrs_engine_skew_scores", "ocrs_engine_estimate_skew",
    "ocrs_engine_warp_page", "ocrs_engine_warp_pages", "ocrs_deskew_map", "ocrs_unwarp_rects", "ocrs_unwarp_chars",
    "ocrs_outline_params_default", "ocrs_outline_params_check", "ocrs_engine_edge_peaks", "ocrs_outline_choose", "ocrs_engine_find_outline",
    "ocrs_quad_map", "ocrs_engine_project_page", "ocrs_engine_project_pages", "ocrs_unproject_rects", "ocrs_unproject_chars",
    "ocrs_rules_params_default", "ocrs_rules_params_check", "ocrs_engine_remove_rules_page", "ocrs_engine_remove_rules_pages",
    "ocrs_speckle_params_default", "ocrs_speckle_params_check", "ocrs_engine_despeckle_page", "ocrs_engine_despeckle_pages",
    "ocrs_binarize_params_default", "ocrs_binarize_params_check", "ocrs_engine_binarize_page", "ocrs_engine_binarize_pages",
    "ocrs_morph_params_default", "ocrs_morph_params_check", "ocrs_engine_morph_page", "ocrs_engine_morph_pages",
    "ocrs_rank_params_default", "ocrs_rank_params_check", "ocrs_engine_rank_page", "ocrs_engine_rank_pages",
    "ocrs_frame_params_default", "ocrs_frame_params_check", "ocrs_engine_clean_frame_page", "ocrs_engine_clean_frame_pages",
    "ocrs_engine_ink_profiles", "ocrs_frame_choice_params_default", "ocrs_frame_choice_params_check", "ocrs_frame_choose",
    "ocrs_engine_crop_page", "ocrs_engine_crop_pages", "ocrs_uncrop_rects", "ocrs_uncrop_chars",
    "ocrs_measure_params_default", "ocrs_measure_params_check", "ocrs_engine_measure_page", "ocrs_engine_measure_pages",
    "ocrs_measure_choice_params_default", "ocrs_measure_choice_params_check", "ocrs_measure_choose", "ocrs_work_scale_for_text",
    "ocrs_reverse_params_default", "ocrs_reverse_params_check", "ocrs_engine_unreverse_page", "ocrs_engine_unreverse_pages",
]

ABI_VERSION = 6   # include/ocrs_amd.h OCRS_ABI_VERSION
TILE_OVERLAP_DEFAULT = 100   # include/ocrs_amd.h OCRS_TILE_OVERLAP_DEFAULT
RESAMPLE_FILTERS = {"auto": 0, "bilinear": 1, "area": 2}   # include/ocrs_amd.h ocrs_resample_filter
POLARITIES = {"auto": 0, "keep": 1, "invert": 2}   # include/ocrs_amd.h ocrs_polarity
MEASURE_BINS = 256   # include/ocrs_amd.h OCRS_MEASURE_BINS
WORK_TEXT_HEIGHT_DEFAULT = 14   # include/ocrs_amd.h OCRS_WORK_TEXT_HEIGHT_DEFAULT


class NormalizeParams(C.Structure):   # include/ocrs_amd.h ocrs_normalize_params
    _fields_ = [("tile", C.c_int32), ("polarity", C.c_int32), ("flatten", C.c_int32), ("levels", C.c_int32)]


class NormalizeInfo(C.Structure):   # include/ocrs_amd.h ocrs_normalize_info
    _fields_ = [("dark", C.c_int32), ("white", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("vote", C.c_int64),
                ("counted", C.c_uint64)]

    def as_dict(self):
        return {"dark": int(self.dark), "vote": int(self.vote), "white": int(self.white), "lo": int(self.lo), "hi": int(self.hi),
                "counted": int(self.counted)}


class RulesParams(C.Structure):   # include/ocrs_amd.h ocrs_rules_params
    _fields_ = [("threshold", C.c_float), ("min_length", C.c_int32), ("max_thickness", C.c_int32), ("margin", C.c_int32), ("paper", C.c_float)]


class RulesInfo(C.Structure):   # include/ocrs_amd.h ocrs_rules_info
    _fields_ = [("paper_bin", C.c_int32), ("fill", C.c_float), ("ink", C.c_uint64), ("counted", C.c_uint64), ("h_removed", C.c_uint64),
                ("v_removed", C.c_uint64), ("overwritten", C.c_uint64), ("kept", C.c_uint64)]

    def as_dict(self):
        return {"paper_bin": int(self.paper_bin), "fill": float(self.fill), "ink": int(self.ink), "counted": int(self.counted),
                "h_removed": int(self.h_removed), "v_removed": int(self.v_removed), "overwritten": int(self.overwritten),
                "kept": int(self.kept)}


class SpeckleParams(C.Structure):   # include/ocrs_amd.h ocrs_speckle_params
    _fields_ = [("threshold", C.c_float), ("max_area", C.c_int32), ("max_hole", C.c_int32), ("keep_near", C.c_int32), ("paper", C.c_float),
                ("ink_level", C.c_float)]


class SpeckleInfo(C.Structure):   # include/ocrs_amd.h ocrs_speckle_info
    _fields_ = [("paper_bin", C.c_int32), ("ink_bin", C.c_int32), ("paper_fill", C.c_float), ("ink_fill", C.c_float), ("ink", C.c_uint64),
                ("counted", C.c_uint64), ("specks", C.c_uint64), ("kept", C.c_uint64), ("speck_pixels", C.c_uint64),
                ("kept_pixels", C.c_uint64), ("holes", C.c_uint64), ("hole_pixels", C.c_uint64)]

    def as_dict(self):
        return {name: (float if name.endswith("_fill") else int)(getattr(self, name)) for name, _ in self._fields_}


class BinarizeParams(C.Structure):   # include/ocrs_amd.h ocrs_binarize_params
    _fields_ = [("radius", C.c_int32), ("k_q8", C.c_int32), ("keep_ink", C.c_int32), ("ink_level", C.c_float), ("paper", C.c_float)]


class BinarizeInfo(C.Structure):   # include/ocrs_amd.h ocrs_binarize_info
    _fields_ = [("counted", C.c_uint64), ("ink", C.c_uint64), ("ink_fill", C.c_float), ("paper_fill", C.c_float)]

    def as_dict(self):
        return {name: (float if name.endswith("_fill") else int)(getattr(self, name)) for name, _ in self._fields_}


class MorphParams(C.Structure):   # include/ocrs_amd.h ocrs_morph_params
    _fields_ = [("op", C.c_int32), ("rx", C.c_int32), ("ry", C.c_int32)]


class MorphInfo(C.Structure):   # include/ocrs_amd.h ocrs_morph_info
    _fields_ = [("counted", C.c_uint64), ("changed", C.c_uint64), ("ink_before", C.c_uint64), ("ink_after", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class RankParams(C.Structure):   # include/ocrs_amd.h ocrs_rank_params
    _fields_ = [("rx", C.c_int32), ("ry", C.c_int32), ("percent", C.c_int32), ("tail", C.c_int32)]


class RankInfo(C.Structure):   # include/ocrs_amd.h ocrs_rank_info
    _fields_ = [("counted", C.c_uint64), ("changed", C.c_uint64), ("ink_before", C.c_uint64), ("ink_after", C.c_uint64), ("spared", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class FrameParams(C.Structure):   # include/ocrs_amd.h ocrs_frame_params
    _fields_ = [("threshold", C.c_float), ("depth", C.c_int32), ("sides", C.c_int32), ("min_area", C.c_int32), ("paper", C.c_float)]


class FrameInfo(C.Structure):   # include/ocrs_amd.h ocrs_frame_info
    _fields_ = [("paper_bin", C.c_int32), ("paper_fill", C.c_float), ("ink", C.c_uint64), ("counted", C.c_uint64), ("ring_ink", C.c_uint64),
                ("removed", C.c_uint64), ("removed_pixels", C.c_uint64), ("kept", C.c_uint64), ("kept_pixels", C.c_uint64)]

    def as_dict(self):
        return {name: (float if name.endswith("_fill") else int)(getattr(self, name)) for name, _ in self._fields_}


class FrameChoiceParams(C.Structure):   # include/ocrs_amd.h ocrs_frame_choice_params
    _fields_ = [("min_count", C.c_int32), ("pad", C.c_int32), ("gutter_min_width", C.c_int32), ("gutter_max_ink", C.c_int32)]


class FrameChoice(C.Structure):   # include/ocrs_amd.h ocrs_frame_choice
    _fields_ = [("found", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("gutter_x", C.c_int32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class MeasureParams(C.Structure):   # include/ocrs_amd.h ocrs_measure_params
    _fields_ = [("threshold", C.c_float), ("min_area", C.c_int32)]


class MeasureInfo(C.Structure):   # include/ocrs_amd.h ocrs_measure_info
    _fields_ = [("ink", C.c_uint64), ("components", C.c_uint32), ("counted", C.c_uint32), ("run_h", C.c_uint32 * MEASURE_BINS),
                ("run_v", C.c_uint32 * MEASURE_BINS), ("comp_h", C.c_uint32 * MEASURE_BINS), ("comp_w", C.c_uint32 * MEASURE_BINS),
                ("area_by_h", C.c_uint64 * MEASURE_BINS)]

    def as_dict(self):
        import numpy as np
        out = {}
        for name, _ in self._fields_:   # exact integers: Python ints and uint32 / uint64 [256] arrays
            v = getattr(self, name)
            out[name] = int(v) if isinstance(v, int) else np.array(v[:], np.uint64 if name == "area_by_h" else np.uint32)
        return out

    @classmethod
    def from_dict(cls, info):
        import numpy as np
        out = cls()
        for name, _ in cls._fields_:
            if name in ("ink", "components", "counted"):
                setattr(out, name, int(info[name]))
            else:
                a = np.asarray(info[name])
                if a.shape != (MEASURE_BINS,):
                    raise ValueError("measure info: %s holds %d bins" % (name, MEASURE_BINS))
                getattr(out, name)[:] = [int(v) for v in a.tolist()]
        return out


class MeasureChoiceParams(C.Structure):   # include/ocrs_amd.h ocrs_measure_choice_params
    _fields_ = [("min_height_strokes", C.c_double)]


class TextScaleC(C.Structure):   # include/ocrs_amd.h ocrs_text_scale
    _fields_ = [("stroke", C.c_int32), ("text_height", C.c_int32), ("support", C.c_uint32), ("blank", C.c_int32)]


class ReverseParams(C.Structure):   # include/ocrs_amd.h ocrs_reverse_params
    _fields_ = [("threshold", C.c_float), ("min_height", C.c_int32), ("min_width", C.c_int32), ("min_fill", C.c_float), ("min_holes", C.c_int32),
                ("max_hole", C.c_int32)]


class ReverseInfo(C.Structure):   # include/ocrs_amd.h ocrs_reverse_info
    _fields_ = [("ink", C.c_uint64), ("components", C.c_uint64), ("candidates", C.c_uint64), ("panels", C.c_uint64), ("panel_pixels", C.c_uint64),
                ("holes", C.c_uint64), ("hole_pixels", C.c_uint64), ("skipped_holes", C.c_uint64), ("inverted", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class CropRect(C.Structure):   # include/ocrs_amd.h ocrs_crop_rect
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32)]


class SkewParams(C.Structure):   # include/ocrs_amd.h ocrs_skew_params
    _fields_ = [("max_deg", C.c_double), ("coarse_step_deg", C.c_double), ("fine_step_deg", C.c_double), ("work_max_side", C.c_int32),
                ("reserved", C.c_int32)]


class SkewInfo(C.Structure):   # include/ocrs_amd.h ocrs_skew_info
    _fields_ = [("angle_deg", C.c_double), ("best_score", C.c_uint64), ("second_score", C.c_uint64), ("fine_score", C.c_uint64),
                ("work_h", C.c_int32), ("work_w", C.c_int32), ("coarse_index", C.c_int32), ("fine_index", C.c_int32)]


class OutlineParams(C.Structure):   # include/ocrs_amd.h ocrs_outline_params
    _fields_ = [("max_deg", C.c_double), ("step_deg", C.c_double), ("min_cover", C.c_double), ("min_span", C.c_double), ("min_area", C.c_double),
                ("work_max_side", C.c_int32), ("min_step", C.c_int32)]


class OutlineInfo(C.Structure):   # include/ocrs_amd.h ocrs_outline_info
    _fields_ = [("found", C.c_int32), ("polarity", C.c_int32), ("corners", C.c_float * 8), ("counts", C.c_uint32 * 4), ("angles", C.c_int32 * 4),
                ("work_h", C.c_int32), ("work_w", C.c_int32)]


_lib = None


def lib():
    """Load the shared object (building it is __graft_entry__.build()'s job)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OcrsError(7, "libocrs_amd.so is not built: run `python -m ocrs_amd.build` "
                               "(there is no CPU fallback for the HIP engine)")
        L = C.CDLL(LIB_PATH)
        L.ocrs_abi_version.restype = C.c_uint32
        if L.ocrs_abi_version() != ABI_VERSION:   # EngineParams / GroupParams below mirror the structs of THIS version
            raise OcrsError(7, "libocrs_amd.so has ABI version %d, this binding was written for %d: rebuild (python -m ocrs_amd.build)"
                            % (L.ocrs_abi_version(), ABI_VERSION))
        L.ocrs_last_error.restype = C.c_char_p
        L.ocrs_engine_detection_threshold.restype = C.c_float
        L.ocrs_engine_detection_threshold.argtypes = [C.c_void_p]
        L.ocrs_stage_name.restype = C.c_char_p
        L.ocrs_kernel_class_name.restype = C.c_char_p
        L.ocrs_buffer_free.argtypes = [C.c_void_p]
        for name in ("ocrs_model_free", "ocrs_engine_free", "ocrs_page_free", "ocrs_engine_group_free"):
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = None
        _lib = L
    return _lib


def check(status):
    if status != OCRS_OK:
        msg = lib().ocrs_last_error()
        raise OcrsError(status, msg.decode("utf-8", "replace") if msg else STATUS_NAMES.get(status, "error"))


def device_count():
    n = C.c_int(0)
    check(lib().ocrs_device_count(C.byref(n)))
    return n.value


def measure_peaks():
    """(fp32 MFMA TFLOP/s, HBM copy GB/s) this device sustains (micro-benchmarks in kernels_peaks.hip)."""
    a, b = C.c_double(0), C.c_double(0)
    check(lib().ocrs_device_measure_peaks(C.byref(a), C.byref(b)))
    return a.value, b.value


def set_option(name, value):
    """ocrs_set_option: the process DEFAULT of a tuning option — what engines created afterwards start with, and what a
    bare Model.run uses.  An existing engine keeps its own copy: OcrEngine.set_option."""
    check(lib().ocrs_set_option(name.encode(), C.c_long(int(value))))


def option_names():
    out, i = [], 0
    while True:
        n = C.c_char_p()
        check(lib().ocrs_option_name(i, C.byref(n)))
        if not n.value:
            return out
        out.append(n.value.decode())
        i += 1


POOL_FIELDS = ("device_live", "device_cached", "device_cap", "device_peak_live", "device_driver_allocs", "device_driver_frees",
               "pinned_live", "pinned_cached", "pinned_cap", "pinned_peak_live", "pinned_driver_allocs", "pinned_driver_frees")


def pool_stats(device=-1):
    """ocrs_device_pool_stats as a dict (bytes / counts)."""
    v = (C.c_uint64 * 12)()
    check(lib().ocrs_device_pool_stats(int(device), v))
    return dict(zip(POOL_FIELDS, (int(x) for x in v)))


def pool_trim(device=-1):
    check(lib().ocrs_device_pool_trim(int(device)))


def pool_configure(device=-1, device_cached_cap=0, pinned_cached_cap=0):
    check(lib().ocrs_device_pool_configure(int(device), C.c_uint64(int(device_cached_cap)), C.c_uint64(int(pinned_cached_cap))))


ISOLATION = {"auto": 0, "none": 1}


def set_isolation(policy="auto", device=-1):
    """ocrs_device_set_isolation: how kernels of engines with numerics != exact are kept away from other requests' kernels."""
    check(lib().ocrs_device_set_isolation(int(device), int(ISOLATION[policy])))


def isolation(device=-1):
    v = (C.c_int * 3)()
    check(lib().ocrs_device_isolation(int(device), v))
    return {"mode": ("free", "serial")[v[0]], "relaxed_engines": int(v[1]), "cus": int(v[2])}


def ctc_beam_search(logp, width, impl=0):
    """ocrs_ctc_beam_search on a [T, C] float32 matrix -> [(label, pos)]."""
    import numpy as np
    a = np.ascontiguousarray(logp, np.float32)
    t, c = a.shape
    lab, pos, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_size_t(0)
    check(lib().ocrs_ctc_beam_search(a.ctypes.data_as(C.POINTER(C.c_float)), t, c, C.c_uint32(width), int(impl),
                                     C.byref(lab), C.byref(pos), C.byref(n)))
    out = [(int(lab[i]), int(pos[i])) for i in range(n.value)]
    lib().ocrs_buffer_free(lab)
    lib().ocrs_buffer_free(pos)
    return out


def ctc_beam_search_scored(logp, width, impl=0):
    """ocrs_ctc_beam_search_scored on a [T, C] float32 matrix -> ([(label, pos)], score, step log-probs float32)."""
    import numpy as np
    a = np.ascontiguousarray(logp, np.float32)
    t, c = a.shape
    lab, pos, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_size_t(0)
    score, slp = C.c_double(0.0), C.POINTER(C.c_float)()
    check(lib().ocrs_ctc_beam_search_scored(a.ctypes.data_as(C.POINTER(C.c_float)), t, c, C.c_uint32(width), int(impl),
                                            C.byref(lab), C.byref(pos), C.byref(n), C.byref(score), C.byref(slp)))
    out = [(int(lab[i]), int(pos[i])) for i in range(n.value)]
    lp = np.array([slp[i] for i in range(n.value)], np.float32)
    for p in (lab, pos, slp):
        lib().ocrs_buffer_free(p)
    return out, score.value, lp


DECODE_METHODS = {"greedy": 0, "greedy_scored": 1, "beam": 2, "beam_scored": 3}   # include/ocrs_amd.h ocrs_ctc_decode_packed


def ctc_decode_packed(mats, excluded=None, method="greedy", width=1, want_logp=True):
    """ocrs_ctc_decode_packed on a list of head outputs [T_i, C] float32 (T_i may be 0) as one packed batch -> per line, in
    the caller's order, a dict: steps [(label, pos)], logp (the unmasked log-probs [T_i, C]; None unless want_logp) and,
    with a scored method, step_logp (float32) and score (float64).  excluded: labels to mask, or None."""
    import numpy as np
    mats = [np.ascontiguousarray(m, np.float32) for m in mats]
    n = len(mats)
    c = int(mats[0].shape[1]) if n else 1
    assert all(m.ndim == 2 and m.shape[1] == c for m in mats)
    lengths = np.array([m.shape[0] for m in mats], np.int32)
    flat = np.concatenate([m.reshape(-1) for m in mats]) if n else np.zeros(0, np.float32)
    flat = np.ascontiguousarray(flat if flat.size else np.zeros(1, np.float32), np.float32)
    excl = None
    if excluded is not None:
        flags = np.zeros(c, np.uint8)
        flags[list(excluded)] = 1
        excl = flags.ctypes.data_as(C.POINTER(C.c_uint8))
    m = DECODE_METHODS[method] if isinstance(method, str) else int(method)
    scored = m in (1, 3)
    lab, pos, slp, lp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
    offs = (C.c_size_t * (n + 1))()
    scores = (C.c_double * max(n, 1))()
    check(lib().ocrs_ctc_decode_packed(flat.ctypes.data_as(C.POINTER(C.c_float)), lengths.ctypes.data_as(C.POINTER(C.c_int32)),
                                       C.c_size_t(n), c, excl, m, C.c_uint32(width), C.byref(lab), C.byref(pos), offs,
                                       C.byref(slp) if scored else None, scores if scored else None,
                                       C.byref(lp) if want_logp else None))
    total = int(offs[n])
    labels = np.ctypeslib.as_array(lab, shape=(max(total, 1),))[:total].copy()
    positions = np.ctypeslib.as_array(pos, shape=(max(total, 1),))[:total].copy()
    step_lp = np.ctypeslib.as_array(slp, shape=(max(total, 1),))[:total].copy() if scored else None
    rows = int(lengths.sum())
    logp = np.ctypeslib.as_array(lp, shape=(max(rows * c, 1),))[:rows * c].copy() if want_logp else None
    for p in (lab, pos) + ((slp,) if scored else ()) + ((lp,) if want_logp else ()):
        lib().ocrs_buffer_free(p)
    out, row = [], 0
    for i in range(n):
        a, b, t = int(offs[i]), int(offs[i + 1]), int(lengths[i])
        r = {"steps": [(int(labels[q]), int(positions[q])) for q in range(a, b)],
             "logp": logp[row * c:(row + t) * c].reshape(t, c) if want_logp else None}
        if scored:
            r["step_logp"] = step_lp[a:b]
            r["score"] = float(scores[i])
        out.append(r)
        row += t
    return out


def mask_component_rects(masks, expand=3.0, min_area=100.0, max_comp=None, arena=None):
    """ocrs_mask_component_rects on masks [n, h, w] (or one [h, w]) of 0 / 1 bytes -> per page a dict: n_roots, overflow
    (bool), rects [k, 6] float32 and valid [k] uint8 for the k = min(n_roots, max_comp) slots of the page.  max_comp and
    arena default to what a detection request takes for the page size."""
    import numpy as np
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.ndim == 2:
        masks = masks[None]
    n, h, w = masks.shape
    if max_comp is None:
        max_comp = min(65536, h * w // 2 + 16)
    if arena is None:
        arena = 2 * h * w + 64
    slots = max(int(max_comp), 1)
    n_roots, overflow = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rects, valid = np.zeros((n, slots, 6), np.float32), np.zeros((n, slots), np.uint8)
    check(lib().ocrs_mask_component_rects(masks.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(n), C.c_int(h), C.c_int(w),
                                          C.c_float(expand), C.c_float(min_area), C.c_int(int(max_comp)), C.c_int64(int(arena)),
                                          n_roots.ctypes.data_as(C.POINTER(C.c_int32)), overflow.ctypes.data_as(C.POINTER(C.c_int32)),
                                          rects.ctypes.data_as(C.POINTER(C.c_float)), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
    out = []
    for i in range(n):
        k = min(int(n_roots[i]), slots)
        out.append({"n_roots": int(n_roots[i]), "overflow": bool(overflow[i]), "rects": rects[i, :k].copy(), "valid": valid[i, :k].copy()})
    return out


def require_gpu():
    n = device_count()
    if n < 1:
        raise OcrsError(7, "no HIP device visible: the ocrs_amd engine has no CPU fallback")
    return n


def jpeg_coefficients(data):
    """ocrs_jpeg_coefficients (host only): (geom int32[28], quant uint16[256], coef int16[n_blocks, 64])."""
    import numpy as np
    geom = (C.c_int32 * 28)()
    quant = (C.c_uint16 * 256)()
    coef = C.POINTER(C.c_int16)()
    nb = C.c_size_t(0)
    buf = C.create_string_buffer(bytes(data), len(data))
    check(lib().ocrs_jpeg_coefficients(buf, C.c_size_t(len(data)), geom, quant, C.byref(coef), C.byref(nb)))
    a = np.ctypeslib.as_array(coef, shape=(max(nb.value, 1) * 64,))[: nb.value * 64].reshape(-1, 64).copy()
    lib().ocrs_buffer_free(coef)
    return np.array(geom[:], np.int32), np.array(quant[:], np.uint16), a


def jpeg_info(data):
    h, w, n, prog, nz = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    buf = C.create_string_buffer(bytes(data), len(data))
    check(lib().ocrs_jpeg_info(buf, C.c_size_t(len(data)), C.byref(h), C.byref(w), C.byref(n), C.byref(prog), C.byref(nz)))
    return {"height": h.value, "width": w.value, "components": n.value, "progressive": bool(prog.value), "nonzero": nz.value}


def jpeg_decode_rgb(data, device=-1):
    """ocrs_jpeg_decode_rgb: host entropy decode + GPU IDCT / upsampling / colour -> (RGB8 [H, W, 3], bytes that crossed PCIe)."""
    import numpy as np
    rgb = C.POINTER(C.c_uint8)()
    h, w, cb = C.c_int(0), C.c_int(0), C.c_size_t(0)
    buf = C.create_string_buffer(bytes(data), len(data))
    check(lib().ocrs_jpeg_decode_rgb(C.c_int(device), buf, C.c_size_t(len(data)), C.byref(rgb), C.byref(h), C.byref(w), C.byref(cb)))
    a = np.ctypeslib.as_array(rgb, shape=(h.value * w.value * 3,)).reshape(h.value, w.value, 3).copy()
    lib().ocrs_buffer_free(rgb)
    return a, cb.value
