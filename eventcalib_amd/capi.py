"""ctypes binding of libecal.so (include/ecal.h).  No torch objects cross this layer: device pointers are
passed as integers (``tensor.data_ptr()``), streams as ``torch.cuda.current_stream().cuda_stream``."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# every symbol include/ecal.h declares (tests check that the built library exports them all)
EXPORTED_SYMBOLS = [
    "ecal_abi_version", "ecal_init", "ecal_destroy", "ecal_strerror", "ecal_last_error", "ecal_sync",
    "ecal_dbscan_batch", "ecal_dbscan_batch_dev",
    "ecal_window_bounds_dev", "ecal_check_sorted_dev", "ecal_sort_events_dev", "ecal_slice_events_dev",
    "ecal_set_point_order", "ecal_get_point_order", "ecal_ref_bucket_step", "ecal_ref_pixel_hash",
    "ecal_comm_unique_id", "ecal_comm_init", "ecal_comm_destroy", "ecal_comm_size", "ecal_comm_rank", "ecal_comm_allreduce_sum_dev", "ecal_comm_allreduce",
    "ecal_circle_radius_threshold", "ecal_extract_batch_dev", "ecal_extract_batch_ordered_dev", "ecal_extract_batch_exact_dev", "ecal_cluster_order_list_dev", "ecal_set_median_ties", "ecal_set_tail_mode", "ecal_get_tail_mode", "ecal_calibrate_fisheye_views", "ecal_set_profile_ranges",
    "ecal_get_median_ties", "ecal_detect_fused_dev", "ecal_cluster_order_dev", "ecal_cluster_order",
    "ecal_stream_create", "ecal_stream_destroy", "ecal_stream_size", "ecal_stream_data", "ecal_stream_to_bin_file", "ecal_detect_batch", "ecal_copy_dev",
    "ecal_grid_order_dev", "ecal_grid_order", "ecal_associate_dev", "ecal_associate", "ecal_pin_host", "ecal_unpin_host",
    "ecal_detect_stream_tiled", "ecal_gather_features_dev", "ecal_detect_pass", "ecal_detect_keyframes", "ecal_detect_keyframes_sharded", "ecal_detect_keyframes_cap_hint", "ecal_detect_keyframes_cap_hint_dev", "ecal_stream_create_from_file", "ecal_stream_times", "ecal_rectify_batch_dev", "ecal_rectify_batch",
    "ecal_solver_create", "ecal_solver_destroy", "ecal_solver_param_size", "ecal_solver_normal_size",
    "ecal_solver_num_chunks", "ecal_solver_evaluate_dev", "ecal_solver_evaluate", "ecal_residuals_dev", "ecal_residuals", "ecal_lm_default_options",
    "ecal_solver_solve", "ecal_inverse_radial_distortion", "ecal_solver_create_dev", "ecal_solver_num_residuals",
    "ecal_associate_ranges_dev", "ecal_ref_nth_element_f64", "ecal_solver_create_from_stream", "ecal_rectify_keyframes", "ecal_solver_time_shard_cuts",
    "ecal_slice_events_packed_dev", "ecal_dbscan_batch_packed_dev", "ecal_extract_batch_packed_dev", "ecal_unpack_points_dev",
    "ecal_report_default_options", "ecal_solver_report_dev", "ecal_solver_report", "ecal_solver_num_landmarks",
    "ecal_report_px_default_options", "ecal_solver_report_px_dev", "ecal_solver_report_px", "ecal_residuals_px_dev", "ecal_residuals_px",
    "ecal_board_image_default_options", "ecal_solver_board_image_dev", "ecal_solver_board_image", "ecal_solver_board_points_dev", "ecal_solver_board_points",
    "ecal_solver_reassociate_dev", "ecal_solver_reassociate", "ecal_solver_create_reassociated",
    "ecal_text_default_options", "ecal_events_from_text_dev", "ecal_text_count_lines_dev", "ecal_stream_create_from_text_file", "ecal_text_to_bin_file",
    "ecal_raw_default_options", "ecal_raw_block_words", "ecal_raw_count_events_dev", "ecal_events_from_raw_dev", "ecal_stream_create_from_raw_file", "ecal_raw_to_bin_file",
    "ecal_aedat_default_options", "ecal_aedat_block_events", "ecal_aedat_parse_header", "ecal_aedat_index_packets", "ecal_aedat_count_events_dev", "ecal_events_from_aedat_dev", "ecal_stream_create_from_aedat_file", "ecal_aedat_to_bin_file",
    "ecal_aedat4_default_options", "ecal_aedat4_block_events", "ecal_aedat4_parse_header", "ecal_aedat4_index_packets", "ecal_aedat4_count_events_dev", "ecal_events_from_aedat4_dev", "ecal_stream_create_from_aedat4_file", "ecal_aedat4_to_bin_file",
    "ecal_bag_default_options", "ecal_bag_block_events", "ecal_bag_index_messages", "ecal_bag_count_events_dev", "ecal_events_from_bag_dev", "ecal_stream_create_from_bag_file", "ecal_bag_to_bin_file",
    "ecal_fields_default_options", "ecal_to_fields_default_options", "ecal_npy_default_options", "ecal_fields_block_events", "ecal_events_from_fields_host", "ecal_events_from_fields_dev", "ecal_stream_create_from_fields", "ecal_events_to_fields_host", "ecal_events_to_fields_dev", "ecal_npy_parse_header", "ecal_stream_create_from_npy_file", "ecal_npy_to_bin_file", "ecal_stream_to_npy_file",
    "ecal_hot_pixel_default_options", "ecal_pixel_activity_dev", "ecal_hot_pixel_mask", "ecal_filter_events_dev", "ecal_stream_remove_hot_pixels",
    "ecal_noise_default_options", "ecal_noise_verdict_host", "ecal_noise_verdict_dev", "ecal_denoise_events_dev", "ecal_stream_remove_noise",
    "ecal_undistort_camera_from_params", "ecal_undistort_reference_canvas", "ecal_undistort_camera_error", "ecal_undistort_options_error", "ecal_undistort_round_half_away", "ecal_undistort_points_host", "ecal_undistort_points_dev", "ecal_undistort_events_dev", "ecal_stream_undistort", "ecal_undistorted_frames_dev", "ecal_stream_undistorted_frames",
    "ecal_image_reference_options", "ecal_image_options_error", "ecal_camera_monotone_radius", "ecal_distort_points_host", "ecal_distort_points_dev", "ecal_undistort_image_host", "ecal_image_table_host", "ecal_image_maps_host", "ecal_image_plan_create", "ecal_image_plan_destroy", "ecal_image_plan_info", "ecal_image_plan_maps_dev", "ecal_image_plan_maps", "ecal_image_plan_table", "ecal_undistort_images_dev", "ecal_undistort_images",
    "ecal_calib_default_options", "ecal_calib_view_blocks_dev", "ecal_pnp_batch_dev", "ecal_pnp_batch", "ecal_pose_gates", "ecal_calibrate_views", "ecal_spline_fit", "ecal_spline_eval", "ecal_spline_so3_refine",
]


# ---- the mirror of include/ecal.h: its structs, callback types, record layouts (numpy dtypes) and constants, then PROTOTYPES ----
class PackedPoints(ctypes.Structure):
    """ecal_packed_points: d_xy16 [cap_points] u32 (x | y << 16), d_seg_fmt [2S] u32 (0 doubles, 1 packed, 3 both)."""
    _fields_ = [("d_xy16", ctypes.c_void_p), ("d_seg_fmt", ctypes.c_void_p)]


class RectifyParams(ctypes.Structure):
    """ecal_rectify_params (include/ecal.h)."""
    _fields_ = [("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
                ("dist", ctypes.c_double * 5), ("width", ctypes.c_double), ("height", ctypes.c_double),
                ("rows", ctypes.c_uint32), ("cols", ctypes.c_uint32), ("asymmetric", ctypes.c_int),
                ("circle_radius", ctypes.c_double), ("fit_circle", ctypes.c_int), ("model", ctypes.c_int)]


class TextOptions(ctypes.Structure):
    """ecal_text_options (include/ecal.h, text ingest)."""
    _fields_ = [("time_magnitude", ctypes.c_double), ("has_time_base", ctypes.c_int), ("time_base", ctypes.c_int64),
                ("has_end_stamp", ctypes.c_int), ("end_stamp", ctypes.c_int64), ("start_time", ctypes.c_double),
                ("has_end_time", ctypes.c_int), ("end_time", ctypes.c_double), ("duplicate_last", ctypes.c_int)]


class TextInfo(ctypes.Structure):
    """ecal_text_info (include/ecal.h, text ingest)."""
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_blank", ctypes.c_uint64), ("n_events", ctypes.c_uint64),
                ("n_negative", ctypes.c_uint64), ("n_after_end", ctypes.c_uint64), ("n_before_start", ctypes.c_uint64),
                ("n_host_lines", ctypes.c_uint64), ("first_bad_line", ctypes.c_uint64), ("time_base", ctypes.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


RAW_AUTO, RAW_EVT2, RAW_EVT3 = 0, 2, 3   # ECAL_RAW_AUTO / _EVT2 / _EVT3
_RAW_FORMATS = {None: RAW_AUTO, "auto": RAW_AUTO, "evt2": RAW_EVT2, "evt3": RAW_EVT3}


def raw_format(fmt):
    """"EVT2" / "EVT3" / None (from the file header), or the ECAL_RAW_* number, as the number"""
    if isinstance(fmt, str) or fmt is None:
        return _RAW_FORMATS[fmt.lower() if fmt else None]
    return int(fmt)


class RawOptions(ctypes.Structure):
    """ecal_raw_options (include/ecal.h, raw ingest)."""
    _fields_ = [("format", ctypes.c_int), ("time_base", ctypes.c_int64), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("start_time", ctypes.c_double), ("has_end_time", ctypes.c_int), ("end_time", ctypes.c_double)]


class RawInfo(ctypes.Structure):
    """ecal_raw_info (include/ecal.h, raw ingest)."""
    _fields_ = [("n_words", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("n_no_state", ctypes.c_uint64),
                ("n_outside", ctypes.c_uint64), ("n_negative", ctypes.c_uint64), ("n_before_start", ctypes.c_uint64),
                ("n_after_end", ctypes.c_uint64), ("n_other_words", ctypes.c_uint64), ("n_trailing_bytes", ctypes.c_uint64),
                ("n_time_wraps", ctypes.c_uint64), ("format", ctypes.c_int), ("header_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


AEDAT_AUTO, AEDAT_2_0, AEDAT_3_1 = 0, 20, 31   # ECAL_AEDAT_AUTO / _2_0 / _3_1
_AEDAT_FORMATS = {None: AEDAT_AUTO, "auto": AEDAT_AUTO, "2.0": AEDAT_2_0, "3.1": AEDAT_3_1}


def aedat_format(fmt):
    """"3.1" / "2.0" / None (from the file's version line), or the ECAL_AEDAT_* number, as the number"""
    if isinstance(fmt, str) or fmt is None:
        return _AEDAT_FORMATS[fmt.lower() if fmt else None]
    return int(fmt)


class AedatOptions(ctypes.Structure):
    """ecal_aedat_options (include/ecal.h, aedat ingest)."""
    _fields_ = [("format", ctypes.c_int), ("source", ctypes.c_int), ("time_base", ctypes.c_int64), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("flip_x", ctypes.c_int), ("flip_y", ctypes.c_int), ("start_time", ctypes.c_double),
                ("has_end_time", ctypes.c_int), ("end_time", ctypes.c_double)]


class AedatInfo(ctypes.Structure):
    """ecal_aedat_info (include/ecal.h, aedat ingest)."""
    _fields_ = [("n_raw_events", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("n_invalid", ctypes.c_uint64),
                ("n_outside", ctypes.c_uint64), ("n_negative", ctypes.c_uint64), ("n_before_start", ctypes.c_uint64),
                ("n_after_end", ctypes.c_uint64), ("n_packets", ctypes.c_uint64), ("n_other_packets", ctypes.c_uint64),
                ("n_records", ctypes.c_uint64), ("n_other_records", ctypes.c_uint64), ("n_trailing_bytes", ctypes.c_uint64),
                ("n_time_wraps", ctypes.c_uint64), ("header_bytes", ctypes.c_uint64), ("format", ctypes.c_int)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class AedatPacket(ctypes.Structure):
    """ecal_aedat_packet (include/ecal.h, aedat ingest): 16 bytes."""
    _fields_ = [("offset_of_first_event", ctypes.c_uint64), ("n_events", ctypes.c_uint32), ("ts_overflow", ctypes.c_int32)]


AEDAT_PACKET_DTYPE = np.dtype([("offset_of_first_event", "<u8"), ("n_events", "<u4"), ("ts_overflow", "<i4")])


AEDAT4_NONE, AEDAT4_LZ4, AEDAT4_LZ4_HIGH, AEDAT4_ZSTD, AEDAT4_ZSTD_HIGH = 0, 1, 2, 3, 4   # ECAL_AEDAT4_*
_AEDAT4_COMPRESSIONS = {None: AEDAT4_LZ4, "none": AEDAT4_NONE, "lz4": AEDAT4_LZ4, "lz4_high": AEDAT4_LZ4_HIGH, "zstd": AEDAT4_ZSTD,
                        "zstd_high": AEDAT4_ZSTD_HIGH}


def aedat4_compression(c):
    """"none" / "lz4" / None (lz4), or the ECAL_AEDAT4_* number, as the number"""
    if isinstance(c, str) or c is None:
        return _AEDAT4_COMPRESSIONS[c.lower() if c else None]
    return int(c)


class Aedat4Options(ctypes.Structure):
    """ecal_aedat4_options (include/ecal.h, aedat4 ingest)."""
    _fields_ = [("compression", ctypes.c_int), ("stream_id", ctypes.c_int), ("auto_time_base", ctypes.c_int), ("flip_x", ctypes.c_int),
                ("flip_y", ctypes.c_int), ("has_end_time", ctypes.c_int), ("time_base", ctypes.c_int64), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("start_time", ctypes.c_double), ("end_time", ctypes.c_double),
                ("max_inflated_bytes", ctypes.c_uint64)]


class Aedat4Info(ctypes.Structure):
    """ecal_aedat4_info (include/ecal.h, aedat4 ingest)."""
    _fields_ = [("n_raw_events", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("n_outside", ctypes.c_uint64),
                ("n_negative", ctypes.c_uint64), ("n_before_start", ctypes.c_uint64), ("n_after_end", ctypes.c_uint64),
                ("n_packets", ctypes.c_uint64), ("n_other_packets", ctypes.c_uint64), ("n_trailing_bytes", ctypes.c_uint64),
                ("n_compressed_bytes", ctypes.c_uint64), ("n_inflated_bytes", ctypes.c_uint64), ("first_stamp_us", ctypes.c_int64),
                ("time_base", ctypes.c_int64), ("compression", ctypes.c_int), ("stream_id", ctypes.c_int)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class Aedat4Packet(ctypes.Structure):
    """ecal_aedat4_packet (include/ecal.h, aedat4 ingest): 16 bytes."""
    _fields_ = [("offset_of_data", ctypes.c_uint64), ("n_bytes", ctypes.c_uint32), ("zero", ctypes.c_uint32)]


AEDAT4_PACKET_DTYPE = np.dtype([("offset_of_data", "<u8"), ("n_bytes", "<u4"), ("zero", "<u4")])


class BagOptions(ctypes.Structure):
    """ecal_bag_options (include/ecal.h, bag ingest).  topic / type are byte strings that must outlive the call (Context.bag_options
    keeps them on the object)."""
    _fields_ = [("topic", ctypes.c_char_p), ("type", ctypes.c_char_p), ("auto_time_base", ctypes.c_int), ("time_base", ctypes.c_int64),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("flip_x", ctypes.c_int), ("flip_y", ctypes.c_int),
                ("start_time", ctypes.c_double), ("has_end_time", ctypes.c_int), ("end_time", ctypes.c_double)]


class BagInfo(ctypes.Structure):
    """ecal_bag_info (include/ecal.h, bag ingest)."""
    _fields_ = [("n_raw_events", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("n_outside", ctypes.c_uint64),
                ("n_negative", ctypes.c_uint64), ("n_before_start", ctypes.c_uint64), ("n_after_end", ctypes.c_uint64),
                ("n_messages", ctypes.c_uint64), ("n_other_messages", ctypes.c_uint64), ("n_chunks", ctypes.c_uint64),
                ("n_connections", ctypes.c_uint64), ("n_trailing_bytes", ctypes.c_uint64), ("first_stamp_ns", ctypes.c_int64),
                ("time_base", ctypes.c_int64), ("msg_width", ctypes.c_uint32), ("msg_height", ctypes.c_uint32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class BagMessage(ctypes.Structure):
    """ecal_bag_message (include/ecal.h, bag ingest): 16 bytes."""
    _fields_ = [("offset_of_first_event", ctypes.c_uint64), ("n_events", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


BAG_MESSAGE_DTYPE = np.dtype([("offset_of_first_event", "<u8"), ("n_events", "<u4"), ("reserved", "<u4")])


class Field(ctypes.Structure):
    """ecal_field (include/ecal.h, array ingest): element i at ptr + i * stride."""
    _fields_ = [("ptr", ctypes.c_void_p), ("stride", ctypes.c_int64), ("type", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class FieldsOptions(ctypes.Structure):
    """ecal_fields_options (include/ecal.h, array ingest)."""
    _fields_ = [("time_magnitude", ctypes.c_double), ("time_base", ctypes.c_int64), ("auto_time_base", ctypes.c_int),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("flip_x", ctypes.c_int), ("flip_y", ctypes.c_int),
                ("start_time", ctypes.c_double), ("has_end_time", ctypes.c_int), ("end_time", ctypes.c_double)]


class FieldsInfo(ctypes.Structure):
    """ecal_fields_info (include/ecal.h, array ingest)."""
    _fields_ = [("n_raw_events", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("n_outside", ctypes.c_uint64),
                ("n_negative", ctypes.c_uint64), ("n_before_start", ctypes.c_uint64), ("n_after_end", ctypes.c_uint64),
                ("time_base", ctypes.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class ToFieldsOptions(ctypes.Structure):
    """ecal_to_fields_options (include/ecal.h, array ingest)."""
    _fields_ = [("ticks_per_second", ctypes.c_double), ("time_base", ctypes.c_int64), ("polarity_signed", ctypes.c_int)]


class ToFieldsInfo(ctypes.Structure):
    """ecal_to_fields_info (include/ecal.h, array ingest)."""
    _fields_ = [("n_events", ctypes.c_uint64), ("n_unrepresentable", ctypes.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class NpyField(ctypes.Structure):
    """ecal_npy_field (include/ecal.h, array ingest)."""
    _fields_ = [("offset", ctypes.c_uint64), ("type", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class NpyLayout(ctypes.Structure):
    """ecal_npy_layout (include/ecal.h, array ingest)."""
    _fields_ = [("data_offset", ctypes.c_uint64), ("n_events", ctypes.c_uint64), ("item_stride", ctypes.c_uint64), ("field", NpyField * 4),
                ("version_major", ctypes.c_uint32), ("version_minor", ctypes.c_uint32)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("data_offset", "n_events", "item_stride", "version_major", "version_minor")}
        d["fields"] = {name: (int(self.field[k].offset), FIELD_TYPE_NAMES[self.field[k].type] if self.field[k].type < 9 else None)
                       for k, name in enumerate("txyp")}
        return d


class NpyOptions(ctypes.Structure):
    """ecal_npy_options (include/ecal.h, array ingest).  The names are byte strings that must outlive the call (npy_options keeps them
    on the object)."""
    _fields_ = [("fields", FieldsOptions), ("t_name", ctypes.c_char_p), ("x_name", ctypes.c_char_p), ("y_name", ctypes.c_char_p),
                ("p_name", ctypes.c_char_p), ("columns", ctypes.c_char_p)]


# ECAL_FIELD_*: the code of a numpy dtype (bool is U8), and the numpy dtype of a code
FIELD_TYPE_NAMES = ("U8", "I8", "U16", "I16", "U32", "I32", "I64", "F32", "F64")
FIELD_DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.int64, np.float32, np.float64)


def field_type(dtype):
    """the ECAL_FIELD_* code of a numpy dtype (or of a torch dtype); ValueError for one that is not a column type"""
    if not isinstance(dtype, (np.dtype, type, str)):   # a torch dtype
        name = str(dtype).replace("torch.", "")
        dtype = {"bool": "bool", "float": "float32", "double": "float64", "half": "float16", "long": "int64", "int": "int32", "short": "int16"}.get(name, name)
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise ValueError("dtype %s is not a column type of the array ingest" % (dtype,))
    if dt == np.bool_:
        return 0
    if dt.byteorder == ">":
        raise ValueError("big-endian dtype %s: the array ingest reads little-endian columns" % dt)
    for code, d in enumerate(FIELD_DTYPES):
        if dt == np.dtype(d):
            return code
    raise ValueError("dtype %s is not a column type of the array ingest (U8, I8, U16, I16, U32, I32, I64, F32, F64 are)" % dt)


class HotPixelOptions(ctypes.Structure):
    """ecal_hot_pixel_options (include/ecal.h, pixel activity / hot pixels)."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("quantile_permille", ctypes.c_uint32),
                ("min_count", ctypes.c_uint32), ("factor", ctypes.c_double)]


class HotPixelInfo(ctypes.Structure):
    """ecal_hot_pixel_info (include/ecal.h, pixel activity / hot pixels)."""
    _fields_ = [("n_events", ctypes.c_uint64), ("n_off_grid", ctypes.c_uint64), ("n_removed", ctypes.c_uint64), ("n_kept", ctypes.c_uint64),
                ("n_active_pixels", ctypes.c_uint32), ("n_hot_pixels", ctypes.c_uint32), ("n_masked_pixels", ctypes.c_uint32),
                ("quantile_count", ctypes.c_uint32), ("max_count", ctypes.c_uint32), ("max_kept_count", ctypes.c_uint32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


# ecal_activity_totals / ecal_filter_totals as numpy records
ACTIVITY_TOTALS = np.dtype([("n_events", np.uint64), ("n_on_grid", np.uint64), ("n_off_grid", np.uint64)])
FILTER_TOTALS = np.dtype([("n_events", np.uint64), ("n_off_grid", np.uint64), ("n_removed", np.uint64), ("n_kept", np.uint64)])


class NoiseOptions(ctypes.Structure):
    """ecal_noise_options (include/ecal.h, noise filter)."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("radius", ctypes.c_uint32), ("min_support", ctypes.c_uint32),
                ("include_self", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("dt", ctypes.c_double)]


CAMERA_RADIAL, CAMERA_FISHEYE = 0, 1          # ECAL_CAMERA_RADIAL / _FISHEYE
UNDISTORT_SUBPIXEL, UNDISTORT_PIXEL = 0, 1    # ECAL_UNDISTORT_SUBPIXEL / _PIXEL
UNDISTORT_TOTALS = np.dtype([("n_events", np.uint64), ("n_invalid", np.uint64), ("n_outside", np.uint64), ("n_kept", np.uint64)])
UNDISTORT_FRAME_TOTALS = np.dtype([("n_pos", np.uint32), ("n_neg", np.uint32), ("n_invalid", np.uint32), ("n_outside", np.uint32)])


class UndistortCamera(ctypes.Structure):
    """ecal_undistort_camera (include/ecal.h, undistortion)."""
    _fields_ = [("model", ctypes.c_int), ("reserved", ctypes.c_int), ("intr", ctypes.c_double * 9), ("out_k", ctypes.c_double * 4)]


class UndistortOptions(ctypes.Structure):
    """ecal_undistort_options (include/ecal.h, undistortion)."""
    _fields_ = [("mode", ctypes.c_uint32), ("out_width", ctypes.c_uint32), ("out_height", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("off_x", ctypes.c_double), ("off_y", ctypes.c_double)]

    def as_dict(self):
        return {"mode": int(self.mode), "out_width": int(self.out_width), "out_height": int(self.out_height),
                "off_x": float(self.off_x), "off_y": float(self.off_y)}


IMAGE_REFERENCE, IMAGE_BILINEAR = 0, 1              # ECAL_IMAGE_REFERENCE / _BILINEAR
DISTORT_INVALID, DISTORT_NOT_CONVERGED = 1, 2       # ECAL_DISTORT_INVALID / _NOT_CONVERGED


class ImageOptions(ctypes.Structure):
    """ecal_image_options (include/ecal.h, image undistortion)."""
    _fields_ = [("method", ctypes.c_uint32), ("channels", ctypes.c_uint32), ("out_width", ctypes.c_uint32), ("out_height", ctypes.c_uint32),
                ("normalize", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("off_x", ctypes.c_double), ("off_y", ctypes.c_double)]

    def as_dict(self):
        return {"method": int(self.method), "channels": int(self.channels), "out_width": int(self.out_width), "out_height": int(self.out_height),
                "normalize": int(self.normalize), "off_x": float(self.off_x), "off_y": float(self.off_y)}


class ImageInfo(ctypes.Structure):
    """ecal_image_info (include/ecal.h, image undistortion)."""
    _fields_ = [("opt", ImageOptions), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("n_invalid_sources", ctypes.c_uint64),
                ("n_empty", ctypes.c_uint64), ("n_entries", ctypes.c_uint64), ("max_neighbours", ctypes.c_uint32), ("truncated", ctypes.c_uint32),
                ("bytes", ctypes.c_uint64), ("r_lim", ctypes.c_double), ("n_invalid", ctypes.c_uint64), ("n_not_converged", ctypes.c_uint64)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_[1:]}
        d["options"] = self.opt.as_dict()
        return d


class _SplineProblem(ctypes.Structure):
    _fields_ = [("n_segments", ctypes.c_uint32), ("seg_cp_off", ctypes.c_void_p), ("knots", ctypes.c_void_p),
                ("n_res", ctypes.c_uint64), ("obs", ctypes.c_void_p), ("time", ctypes.c_void_p),
                ("lm_id", ctypes.c_void_p), ("seg_id", ctypes.c_void_p), ("n_landmarks", ctypes.c_uint32),
                ("landmarks", ctypes.c_void_p), ("circle_radius", ctypes.c_double), ("huber_a", ctypes.c_double),
                ("use_so3", ctypes.c_int), ("camera_model", ctypes.c_int)]


ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class LmOptions(ctypes.Structure):
    _fields_ = [("max_num_iterations", ctypes.c_int), ("function_tolerance", ctypes.c_double),
                ("gradient_tolerance", ctypes.c_double), ("parameter_tolerance", ctypes.c_double),
                ("initial_trust_region_radius", ctypes.c_double), ("max_trust_region_radius", ctypes.c_double),
                ("min_relative_decrease", ctypes.c_double), ("min_lm_diagonal", ctypes.c_double),
                ("max_lm_diagonal", ctypes.c_double), ("jacobi_scaling", ctypes.c_int),
                ("allreduce", ALLREDUCE_FN), ("allreduce_user", ctypes.c_void_p),
                ("distributed", ctypes.c_int), ("rank", ctypes.c_int), ("world_size", ctypes.c_int)]


class LmSummary(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int), ("successful_steps", ctypes.c_int), ("unsuccessful_steps", ctypes.c_int),
                ("jacobian_evaluations", ctypes.c_int), ("cost_evaluations", ctypes.c_int),
                ("termination", ctypes.c_int), ("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                ("seconds", ctypes.c_double), ("seconds_evaluate", ctypes.c_double),
                ("seconds_linear_solve", ctypes.c_double)]


class ReportOptions(ctypes.Structure):
    """ecal_report_options (include/ecal.h)."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("cell_px", ctypes.c_uint32), ("hist_bins", ctypes.c_uint32),
                ("hist_range", ctypes.c_double), ("outlier_thresh", ctypes.c_double)]


# ecal_bin_stats / ecal_report_totals as numpy records
BIN_STATS = np.dtype([("n", np.uint64), ("n_out", np.uint64), ("sum_r", np.float64), ("sum_r2", np.float64), ("sum_abs", np.float64),
                      ("max_abs", np.float64)])
REPORT_TOTALS = np.dtype([("all", BIN_STATS), ("cost", np.float64)])
# ecal_report_px_totals (the report in pixels)
REPORT_PX_TOTALS = np.dtype([("all", BIN_STATS), ("n_degenerate", np.uint64), ("sum_px_per_unit", np.float64)])


class BoardImageOptions(ctypes.Structure):
    """ecal_board_image_options (include/ecal.h)."""
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("bin", ctypes.c_double), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("ring_bins", ctypes.c_uint32), ("ring_range", ctypes.c_double)]


# ecal_board_image_totals / ecal_ring_stats as numpy records; the kernel's block and staging sizes (ECAL_BOARD_IMAGE_*)
BOARD_IMAGE_TOTALS = np.dtype([("n_events", np.uint64), ("n_outside_time", np.uint64), ("n_behind", np.uint64),
                               ("n_outside_image", np.uint64), ("n_image", np.uint64, (2,)), ("n_ring", np.uint64)])
RING_STATS = np.dtype([("n", np.uint64), ("sum_d", np.float64), ("sum_d2", np.float64)])
BOARD_IMAGE_BLOCK, BOARD_IMAGE_CP_LDS = 4096, 16
# ecal_reassociate_totals
REASSOCIATE_TOTALS = np.dtype([("n_events", np.uint64), ("n_outside_time", np.uint64), ("n_behind", np.uint64),
                               ("n_off_ring", np.uint64), ("n_kept", np.uint64)])


CALIB_FIX_ASPECT_RATIO, CALIB_FIX_PRINCIPAL_POINT, CALIB_ZERO_TANGENT_DIST = 1 << 0, 1 << 1, 1 << 2
CALIB_FIX_K1, CALIB_FIX_K2, CALIB_FIX_K3, CALIB_FIX_K4, CALIB_FIX_K5, CALIB_FIX_K6 = (1 << 3, 1 << 4, 1 << 5, 1 << 6,
                                                                                      1 << 7, 1 << 8)
CALIB_FIX_SKEW, CALIB_RECOMPUTE_EXTRINSIC = 1 << 9, 1 << 10
CALIB_USE_INTRINSIC_GUESS = 1 << 11
CALIB_BLOCK_DOUBLES = 272


class CalibOptions(ctypes.Structure):
    """ecal_calib_options (include/ecal.h)."""
    _fields_ = [("model", ctypes.c_int), ("flags", ctypes.c_uint32), ("aspect_ratio", ctypes.c_double),
                ("max_iter", ctypes.c_int), ("eps", ctypes.c_double), ("allreduce", ALLREDUCE_FN),
                ("allreduce_user", ctypes.c_void_p)]


class CalibResult(ctypes.Structure):
    _fields_ = [("intr", ctypes.c_double * 12), ("rms", ctypes.c_double), ("iterations", ctypes.c_int),
                ("jacobian_evaluations", ctypes.c_int), ("error_evaluations", ctypes.c_int), ("seconds", ctypes.c_double)]


class DetectParams(ctypes.Structure):
    """ecal_detect_params (include/ecal.h)."""
    _fields_ = [("dbscan_eps", ctypes.c_double), ("dbscan_min_samples", ctypes.c_uint32), ("cluster_min_sample", ctypes.c_uint32),
                ("need_clusters", ctypes.c_uint32), ("circle_radius_threshold", ctypes.c_double), ("fit_circle", ctypes.c_int),
                ("knn_num", ctypes.c_uint32), ("rows", ctypes.c_uint32), ("cols", ctypes.c_uint32)]


class IngestStats(ctypes.Structure):
    _fields_ = [("chunks", ctypes.c_uint32), ("max_chunk_events", ctypes.c_uint64), ("bytes_uploaded", ctypes.c_uint64),
                ("seconds", ctypes.c_double)]


class AdaptiveParams(ctypes.Structure):
    _fields_ = [("motion_time_step", ctypes.c_double), ("frame_event_num_threshold", ctypes.c_uint32), ("piece_num", ctypes.c_uint32),
                ("start_time", ctypes.c_double), ("end_time", ctypes.c_double), ("max_passes", ctypes.c_uint32),
                ("check_every", ctypes.c_uint32), ("gate_mode", ctypes.c_int), ("piece_first", ctypes.c_uint32),
                ("piece_count", ctypes.c_uint32)]
GATE_OWN_PIECE, GATE_SHARED_MAP = 0, 1


class KeyframeFrame(ctypes.Structure):   # ecal_keyframe_frame
    _fields_ = [("has", ctypes.c_int), ("time", ctypes.c_double), ("dir", ctypes.c_double * 64)]


_FRAME_RECV = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(KeyframeFrame), ctypes.c_int)
_FRAME_SEND = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(KeyframeFrame))


class AdaptiveHandover(ctypes.Structure):   # ecal_adaptive_handover
    _fields_ = [("recv", _FRAME_RECV), ("send", _FRAME_SEND), ("user", ctypes.c_void_p)]


def _prototypes():
    """name -> (restype, argtypes) of every symbol include/ecal.h declares, in the header's order of arguments: POINTER(Struct)
    where the callers pass byref(struct), c_void_p for handles and for device and host buffers, c_char_p for paths and text.
    tests/test_capi_prototypes.py holds the table against the header."""
    vp, cp, i32, u32, u64, sz, f64 = (ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t,
                                      ctypes.c_double)
    P = ctypes.POINTER
    u8 = ctypes.c_uint8
    keyframes = [vp, vp, u64, P(AdaptiveParams), P(DetectParams), u32, u32, vp, vp, vp, vp, P(u32), P(u32), P(u64)]
    return {
        "ecal_abi_version": (i32, []),
        "ecal_init": (i32, [i32, P(vp)]),
        "ecal_destroy": (None, [vp]),
        "ecal_strerror": (cp, [i32]),
        "ecal_last_error": (cp, [vp]),
        "ecal_sync": (i32, [vp]),
        "ecal_dbscan_batch": (i32, [vp, vp, vp, u32, f64, u32, vp, vp]),
        "ecal_dbscan_batch_dev": (i32, [vp, vp, vp, vp, u32, u32, u32, f64, u32, vp, vp, vp]),
        "ecal_window_bounds_dev": (i32, [vp, vp, u64, vp, vp, u32, vp, vp, vp, vp]),
        "ecal_check_sorted_dev": (i32, [vp, vp, u64, vp, vp]),
        "ecal_sort_events_dev": (i32, [vp, vp, u64, vp, vp]),
        "ecal_slice_events_dev": (i32, [vp, vp, u64, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp]),
        "ecal_set_point_order": (i32, [vp, i32]),
        "ecal_get_point_order": (i32, [vp]),
        "ecal_ref_bucket_step": (u64, [i32]),
        "ecal_ref_pixel_hash": (u64, [f64, f64]),
        "ecal_comm_unique_id": (i32, [vp]),
        "ecal_comm_init": (i32, [vp, vp, i32, i32]),
        "ecal_comm_destroy": (i32, [vp]),
        "ecal_comm_size": (i32, [vp]),
        "ecal_comm_rank": (i32, [vp]),
        "ecal_comm_allreduce_sum_dev": (i32, [vp, vp, sz, vp]),
        "ecal_comm_allreduce": (i32, [vp, vp, sz, vp]),
        "ecal_circle_radius_threshold": (f64, [f64, f64, i32, i32, i32, f64, f64]),
        "ecal_extract_batch_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, f64, i32, u32, vp, vp, vp, vp, vp, vp]),
        "ecal_extract_batch_ordered_dev": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, f64, i32, u32, vp, vp, vp, vp, vp, vp]),
        "ecal_extract_batch_exact_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, f64, u32, u32, f64, i32, u32, vp, vp, vp, vp, vp, vp]),
        "ecal_cluster_order_list_dev": (i32, [vp, vp, vp, vp, u32, f64, vp, vp, vp, vp, i32, vp, vp, vp]),
        "ecal_set_median_ties": (i32, [vp, i32]),
        "ecal_set_tail_mode": (i32, [vp, i32]),
        "ecal_get_tail_mode": (i32, [vp]),
        "ecal_calibrate_fisheye_views": (i32, [vp, vp, u32, vp, u32, f64, f64, P(CalibOptions), P(CalibResult), vp, vp, vp, P(i32)]),
        "ecal_set_profile_ranges": (i32, [vp, i32]),
        "ecal_get_median_ties": (i32, [vp]),
        "ecal_detect_fused_dev": (i32, [vp, vp, u64, vp, vp, vp, u32, u32, u32, u32, f64, u32, u32, u32, f64, i32, u32,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "ecal_cluster_order_dev": (i32, [vp, vp, vp, vp, u32, f64, vp, vp, vp, vp, i32, vp]),
        "ecal_cluster_order": (i32, [vp, vp, vp, u32, f64, vp, vp, vp, vp]),
        "ecal_stream_create": (i32, [vp, vp, u64, P(vp)]),
        "ecal_stream_destroy": (None, [vp]),
        "ecal_stream_size": (u64, [vp]),
        "ecal_stream_data": (vp, [vp]),
        "ecal_stream_to_bin_file": (i32, [vp, vp, cp]),
        "ecal_detect_batch": (i32, [vp, vp, vp, vp, u32, P(DetectParams), u32, vp]),
        "ecal_copy_dev": (i32, [vp, vp, vp, sz, vp, i32]),
        "ecal_grid_order_dev": (i32, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp]),
        "ecal_grid_order": (i32, [vp, vp, u32, u32, u32, vp, vp]),
        "ecal_associate_dev": (i32, [vp, vp, u64, vp, vp, u32, u32, f64, f64, f64, f64, vp, vp, vp, vp, vp]),
        "ecal_associate": (i32, [vp, vp, vp, vp, u32, u32, f64, f64, f64, f64, u64, vp, vp, vp, P(u64)]),
        "ecal_pin_host": (i32, [vp, vp, sz]),
        "ecal_unpin_host": (i32, [vp, vp]),
        "ecal_detect_stream_tiled": (i32, [vp, vp, u64, f64, f64, u32, P(DetectParams), u32, vp, vp, vp, P(u32), P(IngestStats)]),
        "ecal_gather_features_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, vp, vp]),
        "ecal_detect_pass": (i32, [vp, vp, u64, vp, vp, u32, P(DetectParams), u32, vp]),
        "ecal_detect_keyframes": (i32, keyframes),
        "ecal_detect_keyframes_sharded": (i32, keyframes + [P(AdaptiveHandover)]),
        "ecal_detect_keyframes_cap_hint": (u64, [P(AdaptiveParams), u64]),
        "ecal_detect_keyframes_cap_hint_dev": (u64, [vp, vp, u64, P(AdaptiveParams)]),
        "ecal_stream_create_from_file": (i32, [vp, cp, f64, i32, f64, P(vp)]),
        "ecal_stream_times": (i32, [vp, P(f64), P(f64)]),
        "ecal_rectify_batch_dev": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, P(RectifyParams), vp, vp, vp, vp]),
        "ecal_rectify_batch": (i32, [vp, vp, vp, vp, vp, u32, vp, u32, vp, P(RectifyParams), vp, vp, vp]),
        "ecal_solver_create": (i32, [vp, P(_SplineProblem), P(vp)]),
        "ecal_solver_destroy": (None, [vp]),
        "ecal_solver_param_size": (sz, [vp]),
        "ecal_solver_normal_size": (sz, [vp]),
        "ecal_solver_num_chunks": (u32, [vp]),
        "ecal_solver_evaluate_dev": (i32, [vp, vp, i32, vp, vp]),
        "ecal_solver_evaluate": (i32, [vp, vp, i32, vp]),
        "ecal_residuals_dev": (i32, [vp, vp, vp, vp, vp, vp]),
        "ecal_residuals": (i32, [vp, vp, vp, vp, vp]),
        "ecal_lm_default_options": (None, [P(LmOptions)]),
        "ecal_solver_solve": (i32, [vp, vp, P(LmOptions), P(LmSummary)]),
        "ecal_inverse_radial_distortion": (None, [vp, vp]),
        "ecal_solver_create_dev": (i32, [vp, P(_SplineProblem), vp, vp, P(vp)]),
        "ecal_solver_num_residuals": (u64, [vp]),
        "ecal_associate_ranges_dev": (i32, [vp, vp, u64, vp, vp, u32, u32, vp, u32, f64, f64, vp, vp, vp, vp, vp, vp]),
        "ecal_ref_nth_element_f64": (None, [vp, u32, u32]),
        "ecal_solver_create_from_stream": (i32, [vp, vp, vp, vp, u32, u32, vp, u32, f64, f64, P(_SplineProblem), P(vp)]),
        "ecal_rectify_keyframes": (i32, [vp, vp, vp, u32, P(DetectParams), vp, vp, P(RectifyParams), vp, vp, vp]),
        "ecal_solver_time_shard_cuts": (i32, [vp, u32, i32, vp]),
        "ecal_slice_events_packed_dev": (i32, [vp, vp, u64, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, P(PackedPoints), vp]),
        "ecal_dbscan_batch_packed_dev": (i32, [vp, vp, vp, vp, u32, u32, u32, f64, u32, vp, vp, P(PackedPoints), vp]),
        "ecal_extract_batch_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, f64, u32, u32, f64, i32, u32, vp, vp, vp, vp, vp,
                                                P(PackedPoints), vp]),
        "ecal_unpack_points_dev": (i32, [vp, P(PackedPoints), vp, vp, u32, vp, vp]),
        "ecal_report_default_options": (None, [P(ReportOptions)]),
        "ecal_solver_report_dev": (i32, [vp, vp, vp, u32, P(ReportOptions), vp, vp, vp, vp, vp, vp, vp]),
        "ecal_solver_report": (i32, [vp, vp, vp, u32, P(ReportOptions), vp, vp, vp, vp, vp, vp]),
        "ecal_solver_num_landmarks": (u32, [vp]),
        "ecal_report_px_default_options": (None, [P(ReportOptions)]),
        "ecal_solver_report_px_dev": (i32, [vp, vp, vp, u32, P(ReportOptions), vp, vp, vp, vp, vp, vp, vp]),
        "ecal_solver_report_px": (i32, [vp, vp, vp, u32, P(ReportOptions), vp, vp, vp, vp, vp, vp]),
        "ecal_residuals_px_dev": (i32, [vp, vp, vp, vp, vp, vp]),
        "ecal_residuals_px": (i32, [vp, vp, vp, vp, vp]),
        "ecal_board_image_default_options": (i32, [vp, P(BoardImageOptions)]),
        "ecal_solver_board_image_dev": (i32, [vp, vp, vp, u64, P(BoardImageOptions), vp, vp, vp, vp, vp]),
        "ecal_solver_board_image": (i32, [vp, vp, vp, P(BoardImageOptions), vp, vp, vp, vp]),
        "ecal_solver_board_points_dev": (i32, [vp, vp, vp, u64, vp, vp, vp]),
        "ecal_solver_board_points": (i32, [vp, vp, vp, vp, vp]),
        "ecal_solver_reassociate_dev": (i32, [vp, vp, vp, u64, f64, vp, vp, vp, vp, vp, vp, vp]),
        "ecal_solver_reassociate": (i32, [vp, vp, vp, f64, u64, vp, vp, vp, vp, P(u64), vp]),
        "ecal_solver_create_reassociated": (i32, [vp, vp, vp, f64, P(vp), vp]),
        "ecal_text_default_options": (None, [P(TextOptions)]),
        "ecal_events_from_text_dev": (i32, [vp, vp, u64, P(TextOptions), vp, u64, P(TextInfo), vp]),
        "ecal_text_count_lines_dev": (i32, [vp, vp, u64, P(u64), vp]),
        "ecal_stream_create_from_text_file": (i32, [vp, cp, P(TextOptions), P(vp), P(TextInfo)]),
        "ecal_text_to_bin_file": (i32, [vp, cp, cp, P(TextOptions), P(TextInfo)]),
        "ecal_raw_default_options": (None, [P(RawOptions)]),
        "ecal_raw_block_words": (u32, [i32]),
        "ecal_raw_count_events_dev": (i32, [vp, vp, u64, i32, P(u64), vp]),
        "ecal_events_from_raw_dev": (i32, [vp, vp, u64, P(RawOptions), vp, u64, P(RawInfo), vp]),
        "ecal_stream_create_from_raw_file": (i32, [vp, cp, P(RawOptions), P(vp), P(RawInfo)]),
        "ecal_raw_to_bin_file": (i32, [vp, cp, cp, P(RawOptions), P(RawInfo)]),
        "ecal_aedat_default_options": (None, [P(AedatOptions)]),
        "ecal_aedat_block_events": (u32, [i32]),
        "ecal_aedat_parse_header": (i32, [vp, cp, u64, P(i32), P(u64)]),
        "ecal_aedat_index_packets": (i32, [vp, vp, u64, i32, vp, u64, P(u64), P(AedatInfo)]),
        "ecal_aedat_count_events_dev": (i32, [vp, vp, u64, vp, u64, i32, P(u64), vp]),
        "ecal_events_from_aedat_dev": (i32, [vp, vp, u64, vp, u64, P(AedatOptions), vp, u64, P(AedatInfo), vp]),
        "ecal_stream_create_from_aedat_file": (i32, [vp, cp, P(AedatOptions), P(vp), P(AedatInfo)]),
        "ecal_aedat_to_bin_file": (i32, [vp, cp, cp, P(AedatOptions), P(AedatInfo)]),
        "ecal_aedat4_default_options": (None, [P(Aedat4Options)]),
        "ecal_aedat4_block_events": (u32, []),
        "ecal_aedat4_parse_header": (i32, [vp, cp, u64, u64, P(i32), P(u64), P(u64)]),
        "ecal_aedat4_index_packets": (i32, [vp, vp, u64, i32, vp, u64, P(u64), P(Aedat4Info)]),
        "ecal_aedat4_count_events_dev": (i32, [vp, vp, u64, vp, u64, P(Aedat4Options), P(u64), vp]),
        "ecal_events_from_aedat4_dev": (i32, [vp, vp, u64, vp, u64, P(Aedat4Options), vp, u64, P(Aedat4Info), vp]),
        "ecal_stream_create_from_aedat4_file": (i32, [vp, cp, P(Aedat4Options), P(vp), P(Aedat4Info)]),
        "ecal_aedat4_to_bin_file": (i32, [vp, cp, cp, P(Aedat4Options), P(Aedat4Info)]),
        "ecal_bag_default_options": (None, [P(BagOptions)]),
        "ecal_bag_block_events": (u32, []),
        "ecal_bag_index_messages": (i32, [vp, vp, u64, P(BagOptions), vp, u64, P(u64), P(BagInfo)]),
        "ecal_bag_count_events_dev": (i32, [vp, vp, u64, vp, u64, P(u64), vp]),
        "ecal_events_from_bag_dev": (i32, [vp, vp, u64, vp, u64, P(BagOptions), vp, u64, P(BagInfo), vp]),
        "ecal_stream_create_from_bag_file": (i32, [vp, cp, P(BagOptions), P(vp), P(BagInfo)]),
        "ecal_bag_to_bin_file": (i32, [vp, cp, cp, P(BagOptions), P(BagInfo)]),
        "ecal_fields_default_options": (None, [P(FieldsOptions)]),
        "ecal_to_fields_default_options": (None, [P(ToFieldsOptions)]),
        "ecal_npy_default_options": (None, [P(NpyOptions)]),
        "ecal_fields_block_events": (u32, []),
        "ecal_events_from_fields_host": (i32, [P(Field), u64, P(FieldsOptions), vp, u64, P(FieldsInfo), cp, u64]),
        "ecal_events_from_fields_dev": (i32, [vp, P(Field), u64, P(FieldsOptions), vp, u64, P(FieldsInfo), vp]),
        "ecal_stream_create_from_fields": (i32, [vp, P(Field), u64, P(FieldsOptions), P(vp), P(FieldsInfo)]),
        "ecal_events_to_fields_host": (i32, [vp, u64, P(Field), P(ToFieldsOptions), P(ToFieldsInfo), cp, u64]),
        "ecal_events_to_fields_dev": (i32, [vp, vp, u64, P(Field), P(ToFieldsOptions), P(ToFieldsInfo), vp]),
        "ecal_npy_parse_header": (i32, [vp, vp, u64, u64, P(NpyOptions), P(NpyLayout), cp, u64]),
        "ecal_stream_create_from_npy_file": (i32, [vp, cp, P(NpyOptions), P(vp), P(FieldsInfo)]),
        "ecal_npy_to_bin_file": (i32, [vp, cp, cp, P(NpyOptions), P(FieldsInfo)]),
        "ecal_stream_to_npy_file": (i32, [vp, vp, cp]),
        "ecal_hot_pixel_default_options": (None, [P(HotPixelOptions)]),
        "ecal_pixel_activity_dev": (i32, [vp, vp, u64, u32, u32, vp, vp, vp]),
        "ecal_hot_pixel_mask": (i32, [vp, P(HotPixelOptions), vp, vp, P(HotPixelInfo)]),
        "ecal_filter_events_dev": (i32, [vp, vp, u64, vp, u32, u32, vp, vp, vp, vp]),
        "ecal_stream_remove_hot_pixels": (i32, [vp, vp, P(HotPixelOptions), vp, P(vp), vp, vp, P(HotPixelInfo)]),
        "ecal_noise_default_options": (None, [P(NoiseOptions)]),
        "ecal_noise_verdict_host": (i32, [vp, u64, P(NoiseOptions), vp, vp]),
        "ecal_noise_verdict_dev": (i32, [vp, vp, u64, P(NoiseOptions), vp, vp, vp]),
        "ecal_denoise_events_dev": (i32, [vp, vp, u64, P(NoiseOptions), vp, vp, vp, vp]),
        "ecal_stream_remove_noise": (i32, [vp, vp, P(NoiseOptions), P(vp), vp]),
        "ecal_undistort_camera_from_params": (None, [i32, vp, P(UndistortCamera)]),
        "ecal_undistort_reference_canvas": (None, [u32, u32, P(UndistortOptions)]),
        "ecal_undistort_camera_error": (cp, [P(UndistortCamera)]),
        "ecal_undistort_options_error": (cp, [P(UndistortOptions)]),
        "ecal_undistort_round_half_away": (f64, [f64]),
        "ecal_undistort_points_host": (i32, [P(UndistortCamera), vp, u64, vp, vp]),
        "ecal_undistort_points_dev": (i32, [vp, P(UndistortCamera), vp, u64, vp, vp, vp]),
        "ecal_undistort_events_dev": (i32, [vp, P(UndistortCamera), P(UndistortOptions), vp, u64, vp, vp, vp, vp]),
        "ecal_stream_undistort": (i32, [vp, vp, P(UndistortCamera), P(UndistortOptions), P(vp), vp]),
        "ecal_undistorted_frames_dev": (i32, [vp, P(UndistortCamera), P(UndistortOptions), vp, P(PackedPoints), vp, vp, u32, vp, vp, vp]),
        "ecal_stream_undistorted_frames": (i32, [vp, vp, P(UndistortCamera), P(UndistortOptions), vp, vp, u32, vp, vp]),
        "ecal_image_reference_options": (None, [u32, u32, P(ImageOptions)]),
        "ecal_image_options_error": (cp, [P(ImageOptions)]),
        "ecal_camera_monotone_radius": (i32, [P(UndistortCamera), u32, u32, P(f64), P(u32)]),
        "ecal_distort_points_host": (i32, [P(UndistortCamera), u32, u32, vp, u64, vp, vp]),
        "ecal_distort_points_dev": (i32, [vp, P(UndistortCamera), u32, u32, vp, u64, vp, vp, vp]),
        "ecal_undistort_image_host": (i32, [P(UndistortCamera), u32, u32, P(ImageOptions), vp, vp, vp, P(ImageInfo)]),
        "ecal_image_table_host": (i32, [P(UndistortCamera), u32, u32, P(ImageOptions), vp, vp, vp, u64, P(ImageInfo)]),
        "ecal_image_maps_host": (i32, [P(UndistortCamera), u32, u32, P(ImageOptions), vp, vp, vp, P(ImageInfo)]),
        "ecal_image_plan_create": (i32, [vp, P(UndistortCamera), u32, u32, P(ImageOptions), P(vp)]),
        "ecal_image_plan_destroy": (None, [vp]),
        "ecal_image_plan_info": (i32, [vp, P(ImageInfo)]),
        "ecal_image_plan_maps_dev": (i32, [vp, vp, vp, vp, vp]),
        "ecal_image_plan_maps": (i32, [vp, vp, vp, vp]),
        "ecal_image_plan_table": (i32, [vp, vp, vp, vp]),
        "ecal_undistort_images_dev": (i32, [vp, vp, vp, u32, vp, vp, vp]),
        "ecal_undistort_images": (i32, [vp, vp, vp, u32, vp, vp]),
        "ecal_calib_default_options": (None, [P(CalibOptions)]),
        "ecal_calib_view_blocks_dev": (i32, [vp, vp, u32, vp, u32, i32, u32, f64, vp, vp, i32, vp, vp]),
        "ecal_pnp_batch_dev": (i32, [vp, vp, u32, vp, vp, u32, i32, vp, f64, i32, i32, vp, vp, vp, vp, vp]),
        "ecal_pnp_batch": (i32, [vp, vp, u32, vp, vp, u32, i32, vp, f64, i32, i32, vp, vp, vp, vp]),
        "ecal_pose_gates": (i32, [u32, P(f64), P(f64), P(f64), P(u8), P(u8), f64, P(u32), P(u32), P(u32), P(u32)]),
        "ecal_calibrate_views": (i32, [vp, vp, u32, vp, u32, f64, f64, P(CalibOptions), P(CalibResult), vp, vp, vp]),
        "ecal_spline_fit": (i32, [vp, vp, u32, u32, u32, vp, vp]),
        "ecal_spline_eval": (i32, [vp, vp, u32, u32, vp, u32, vp]),
        "ecal_spline_so3_refine": (i32, [vp, u32, vp, vp, vp, u32, i32, P(f64), P(f64), P(i32)]),
    }


PROTOTYPES = _prototypes()
# the ecal_debug_* symbols the package calls (not in the public header: set where the library exports them)
DEBUG_PROTOTYPES = {
    "ecal_debug_reload_env": (ctypes.c_int, [ctypes.c_void_p]),
    "ecal_debug_px_todo_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]),
    "ecal_debug_tail_seen": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]),
}


import weakref

_live_contexts = weakref.WeakSet()


def sync_env():
    """Tests: the library reads its debug switches (ECAL_* environment variables) once per context, at ecal_init; after changing
    one under a live context, call this — every live Context re-reads them (ecal_debug_reload_env)."""
    for c in list(_live_contexts):
        c.reload_env()


class EcalError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("ecal status %d: %s" % (status, msg))
        self.status = status


def lib_path():
    return os.path.join(_HERE, "libecal.so")


def load_library():
    """Load libecal.so; raises (never falls back) if the HIP library has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C eventcalib_amd/csrc`). There is no CPU fallback." % p)
    # torch wheels bundle their own libamdhip64 under the same soname: whichever HIP runtime is mapped first serves
    # the whole process, and torch cannot find a GPU through the system one.  Let torch (when present) map its
    # runtime first; libecal.so then binds to that already-loaded library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(p)
    _apply_prototypes(L)
    _LIB = L
    return L


def _apply_prototypes(L):
    """the one place a prototype is set on the library handle: every public symbol (a missing one raises AttributeError), and
    the debug symbols this build exports"""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    for name, (restype, argtypes) in DEBUG_PROTOTYPES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes


def hot_pixel_options(width=None, height=None, quantile_permille=None, min_count=None, factor=None):
    """ecal_hot_pixel_options from ecal_hot_pixel_default_options (346 x 260, the 99 % quantile, 64 events, factor 8); None keeps
    the default."""
    L = load_library()
    o = HotPixelOptions()
    L.ecal_hot_pixel_default_options(ctypes.byref(o))
    if width is not None:
        o.width = int(width)
    if height is not None:
        o.height = int(height)
    if quantile_permille is not None:
        o.quantile_permille = int(quantile_permille)
    if min_count is not None:
        o.min_count = int(min_count)
    if factor is not None:
        o.factor = float(factor)
    return o


def hot_pixel_mask(counts, extra_mask=None, **options):
    """ecal_hot_pixel_mask (host arrays; no context, no device): counts [2, H, W] (any integer type whose values fit uint32) and
    an optional extra_mask [H, W] (non-zero: remove whatever it counts) -> (mask [H, W] bool, info dict).  options:
    quantile_permille, min_count, factor; width and height come from the shape of counts."""
    L = load_library()
    c = np.asarray(counts)
    if c.ndim != 3 or c.shape[0] != 2:
        raise ValueError("counts must be [2, H, W]")
    if c.size and (int(c.min()) < 0 or int(c.max()) > 0xFFFFFFFF):
        raise ValueError("counts must fit uint32")
    c = np.ascontiguousarray(c, np.uint32)
    H, W = c.shape[1:]
    o = hot_pixel_options(width=W, height=H, **options)
    extra = None
    if extra_mask is not None:
        extra = np.ascontiguousarray(np.asarray(extra_mask) != 0, np.uint8)
        if extra.shape != (H, W):
            raise ValueError("extra_mask must be [H, W]")
    mask = np.zeros((H, W), np.uint8)
    info = HotPixelInfo()
    st = L.ecal_hot_pixel_mask(c.ctypes.data if c.size else None, ctypes.byref(o), extra.ctypes.data if extra is not None and extra.size else None,
                               mask.ctypes.data if mask.size else None, ctypes.byref(info))
    if st != 0:
        raise EcalError(st, L.ecal_strerror(st).decode() + ": ecal_hot_pixel_mask (width and height from 1 to 4096, quantile_permille <= 1000, "
                        "a finite factor >= 0)")
    return mask.astype(bool), info.as_dict()


def noise_options(width=None, height=None, radius=None, min_support=None, include_self=None, dt=None, reserved=None):
    """ecal_noise_options from ecal_noise_default_options (346 x 260, radius 1, min_support 1, include_self 0, dt 0.005 in the stream's
    time unit); None keeps the default."""
    L = load_library()
    o = NoiseOptions()
    L.ecal_noise_default_options(ctypes.byref(o))
    for name, value in (("width", width), ("height", height), ("radius", radius), ("min_support", min_support),
                        ("include_self", include_self), ("reserved", reserved)):
        if value is not None:
            setattr(o, name, int(value))
    if dt is not None:
        o.dt = float(dt)
    return o


NOISE_OPTIONS_RULE = "width and height from 1 to 4096, radius from 1 to 3, min_support at least 1, include_self 0 or 1, reserved 0, dt at least 0 and not NaN"


def noise_verdict_host(events, **options):
    """ecal_noise_verdict_host (host arrays; no context, no device): the sequential walk of the noise filter over packed 25-byte
    records -> (verdict uint8 [n]: 1 keep, 0 remove; totals: one FILTER_TOTALS record).  options: width, height, radius,
    min_support, include_self, dt."""
    L = load_library()
    ev = np.frombuffer(events, np.uint8) if isinstance(events, (bytes, bytearray, memoryview)) else np.asarray(events, np.uint8).ravel()
    ev = np.ascontiguousarray(ev)
    assert ev.size % 25 == 0, "packed 25-byte event records"
    n = ev.size // 25
    o = noise_options(**options)
    verdict = np.zeros(n, np.uint8)
    tot = np.zeros(1, FILTER_TOTALS)
    st = L.ecal_noise_verdict_host(ev.ctypes.data if n else None, n, ctypes.byref(o), verdict.ctypes.data if n else None, tot.ctypes.data)
    if st != 0:
        raise EcalError(st, L.ecal_strerror(st).decode() + ": ecal_noise_verdict_host (" + NOISE_OPTIONS_RULE + ")")
    return verdict, tot[0]


def undistort_camera(params, model=CAMERA_RADIAL, out_k=None, reserved=0):
    """ecal_undistort_camera from the head of the solver's parameter vector (fx fy cx cy k1..k5; ecal_undistort_camera_from_params:
    out_k = fx fy cx cy, as the reference's K_ * Xc) or with another ideal camera out_k = (fx', fy', cx', cy').  An UndistortCamera
    is handed through."""
    if isinstance(params, UndistortCamera):
        return params
    L = load_library()
    p = np.ascontiguousarray(np.asarray(params, np.float64).ravel()[:9])
    if p.size != 9:
        raise ValueError("fx fy cx cy k1..k5: nine numbers")
    cam = UndistortCamera()
    L.ecal_undistort_camera_from_params(int(model), p.ctypes.data, ctypes.byref(cam))
    if out_k is not None:
        cam.out_k[:] = [float(v) for v in out_k]
    cam.reserved = int(reserved)
    return cam


def undistort_reference_canvas(width, height):
    """ecal_undistort_reference_canvas: PIXEL options with the reference's canvas, round(1.2 * size), and offsets, size * 0.1"""
    L = load_library()
    o = UndistortOptions()
    L.ecal_undistort_reference_canvas(int(width), int(height), ctypes.byref(o))
    return o


def undistort_options(mode=None, out_width=None, out_height=None, off_x=None, off_y=None, reserved=None, sensor=None):
    """ecal_undistort_options: SUBPIXEL by default; sensor=(width, height) starts from the reference canvas (PIXEL); "pixel" /
    "subpixel" or the number for mode.  An UndistortOptions is handed through."""
    if isinstance(mode, UndistortOptions):
        return mode
    o = undistort_reference_canvas(*sensor) if sensor is not None else UndistortOptions()
    if mode is not None:
        o.mode = {"subpixel": UNDISTORT_SUBPIXEL, "pixel": UNDISTORT_PIXEL}[mode.lower()] if isinstance(mode, str) else int(mode)
    for name, value in (("out_width", out_width), ("out_height", out_height), ("reserved", reserved)):
        if value is not None:
            setattr(o, name, int(value))
    if off_x is not None:
        o.off_x = float(off_x)
    if off_y is not None:
        o.off_y = float(off_y)
    return o


def undistort_camera_error(cam):
    """ecal_undistort_camera_error: None, or the text that names the refused field"""
    L = load_library()
    r = L.ecal_undistort_camera_error(ctypes.byref(cam))
    return r.decode() if r else None


def undistort_options_error(opt):
    """ecal_undistort_options_error: None, or the text that names the refused field"""
    L = load_library()
    r = L.ecal_undistort_options_error(ctypes.byref(opt))
    return r.decode() if r else None


def undistort_round_half_away(a):
    """ecal_undistort_round_half_away: std::round as the library spells it"""
    L = load_library()
    return float(L.ecal_undistort_round_half_away(float(a)))


def undistort_points_host(cam, uv):
    """ecal_undistort_points_host (host arrays; no context, no device): uv [n, 2] -> (out [n, 2] float64 with 0, 0 where invalid,
    flag uint8 [n]: 0 valid, 1 invalid).  cam: an UndistortCamera (undistort_camera)."""
    L = load_library()
    uv = np.ascontiguousarray(np.asarray(uv, np.float64).reshape(-1, 2))
    n = uv.shape[0]
    out = np.zeros((n, 2), np.float64)
    flag = np.zeros(n, np.uint8)
    st = L.ecal_undistort_points_host(ctypes.byref(cam), uv.ctypes.data if n else None, n, out.ctypes.data if n else None,
                                      flag.ctypes.data if n else None)
    if st != 0:
        raise EcalError(st, L.ecal_strerror(st).decode() + ": ecal_undistort_points_host: " + (undistort_camera_error(cam) or "null pointer"))
    return out, flag


def image_reference_options(width, height):
    """ecal_image_reference_options: the reference's canvas, round(1.2 * size) with offsets round(size * 0.1), 3 channels, normalize 1,
    REFERENCE"""
    L = load_library()
    o = ImageOptions()
    L.ecal_image_reference_options(int(width), int(height), ctypes.byref(o))
    return o


def image_options(method=None, channels=None, out_width=None, out_height=None, normalize=None, off_x=None, off_y=None, reserved=None,
                  sensor=None, reference_canvas=False):
    """ecal_image_options.  sensor=(width, height): the canvas is the sensor's own (BILINEAR, normalize 0, no offsets), or with
    reference_canvas=True the reference's (REFERENCE, 3 channels, normalize 1); "reference" / "bilinear" or the number for method.
    An ImageOptions is handed through."""
    if isinstance(method, ImageOptions):
        return method
    if sensor is not None and reference_canvas:
        o = image_reference_options(*sensor)
    else:
        o = ImageOptions(IMAGE_BILINEAR, 1, 0, 0, 0, 0, 0.0, 0.0)
        if sensor is not None:
            o.out_width, o.out_height = int(sensor[0]), int(sensor[1])
    if method is not None:
        o.method = {"reference": IMAGE_REFERENCE, "bilinear": IMAGE_BILINEAR}[method.lower()] if isinstance(method, str) else int(method)
    for name, value in (("channels", channels), ("out_width", out_width), ("out_height", out_height), ("normalize", normalize), ("reserved", reserved)):
        if value is not None:
            setattr(o, name, int(value))
    if off_x is not None:
        o.off_x = float(off_x)
    if off_y is not None:
        o.off_y = float(off_y)
    return o


def image_options_error(opt):
    """ecal_image_options_error: None, or the text that names the refused field"""
    L = load_library()
    r = L.ecal_image_options_error(ctypes.byref(opt) if opt is not None else None)
    return r.decode() if r else None


def _image_sensor_error(width, height):
    if not 1 <= int(width) <= 8192:
        return "width from 1 to 8192"
    if not 1 <= int(height) <= 8192:
        return "height from 1 to 8192"
    return None


def _image_host_fail(L, st, who, cam, width, height, opt):
    why = undistort_camera_error(cam) or _image_sensor_error(width, height) or (image_options_error(opt) if opt is not None else None)
    raise EcalError(st, L.ecal_strerror(st).decode() + ": " + who + ": " + (why or "null pointer or the wrong method"))


def camera_monotone_radius(cam, width, height):
    """ecal_camera_monotone_radius -> (r_lim, truncated): the normalised sensor radius up to which the forward projection inverts"""
    L = load_library()
    r, t = ctypes.c_double(0.0), ctypes.c_uint32(0)
    st = L.ecal_camera_monotone_radius(ctypes.byref(cam), max(0, int(width)), max(0, int(height)), ctypes.byref(r), ctypes.byref(t))
    if st != 0:
        _image_host_fail(L, st, "ecal_camera_monotone_radius", cam, width, height, None)
    return float(r.value), int(t.value)


def distort_points_host(cam, width, height, uv):
    """ecal_distort_points_host (host arrays; no context, no device): uv [n, 2] of the ideal camera -> (out [n, 2] float64 sensor
    pixels with 0, 0 where invalid, flag uint8 [n]: 0, DISTORT_INVALID or DISTORT_NOT_CONVERGED)."""
    L = load_library()
    uv = np.ascontiguousarray(np.asarray(uv, np.float64).reshape(-1, 2))
    n = uv.shape[0]
    out = np.zeros((n, 2), np.float64)
    flag = np.zeros(n, np.uint8)
    st = L.ecal_distort_points_host(ctypes.byref(cam), max(0, int(width)), max(0, int(height)), uv.ctypes.data if n else None, n,
                                    out.ctypes.data if n else None, flag.ctypes.data if n else None)
    if st != 0:
        _image_host_fail(L, st, "ecal_distort_points_host", cam, width, height, None)
    return out, flag


def _frames_arg(images, width, height, channels):
    """uint8 [H, W], [H, W, C] or [N, H, W, C] -> ([N, H, W, C] contiguous, the rank it came with)"""
    a = np.asarray(images)
    if a.dtype != np.uint8:
        raise ValueError("images must be uint8")
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    elif rank != 4:
        raise ValueError("images: (H, W), (H, W, C) or (N, H, W, C)")
    if a.shape[1:] != (int(height), int(width), int(channels)):
        raise ValueError("images of %s do not match the sensor %d x %d with %d channel(s)" % (a.shape[1:], int(width), int(height), int(channels)))
    return np.ascontiguousarray(a), rank


def _frames_result(out, rank):
    return out[0, :, :, 0] if rank == 2 else (out[0] if rank == 3 else out)


def undistort_image_host(cam, width, height, image, opt=None, **options):
    """ecal_undistort_image_host (host arrays; no context, no device): ONE frame uint8 [H, W] or [H, W, C] -> (picture uint8 of the same
    rank on the canvas, minmax float32 [2], info dict).  opt an ImageOptions, or options for image_options."""
    L = load_library()
    o = opt if opt is not None else image_options(**options)
    if image_options_error(o) or _image_sensor_error(width, height):
        _image_host_fail(L, -1, "ecal_undistort_image_host", cam, width, height, o)
    a, rank = _frames_arg(image, width, height, o.channels)
    if rank == 4 or a.shape[0] != 1:
        raise ValueError("one frame")
    out = np.zeros((1, int(o.out_height), int(o.out_width), int(o.channels)), np.uint8)
    mm = np.zeros(2, np.float32)
    info = ImageInfo()
    st = L.ecal_undistort_image_host(ctypes.byref(cam), int(width), int(height), ctypes.byref(o), a.ctypes.data, out.ctypes.data, mm.ctypes.data,
                                     ctypes.byref(info))
    if st != 0:
        _image_host_fail(L, st, "ecal_undistort_image_host", cam, width, height, o)
    return _frames_result(out, rank), mm, info.as_dict()


def image_table_host(cam, width, height, opt=None, **options):
    """ecal_image_table_host: the REFERENCE table of the host walk -> (off uint32 [canvas pixels + 1], idx uint32 [n], w float64 [n],
    info dict)"""
    L = load_library()
    o = opt if opt is not None else image_options(**options)
    if image_options_error(o) or _image_sensor_error(width, height):
        _image_host_fail(L, -1, "ecal_image_table_host", cam, width, height, o)
    off = np.zeros(int(o.out_width) * int(o.out_height) + 1, np.uint32)
    cap = 13 * int(width) * int(height)   # a source neighbours at most 13 canvas pixels
    idx, w = np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
    info = ImageInfo()
    st = L.ecal_image_table_host(ctypes.byref(cam), int(width), int(height), ctypes.byref(o), off.ctypes.data, idx.ctypes.data, w.ctypes.data, cap,
                                 ctypes.byref(info))
    if st != 0:
        _image_host_fail(L, st, "ecal_image_table_host", cam, width, height, o)
    n = int(info.n_entries)
    return off, idx[:n].copy(), w[:n].copy(), info.as_dict()


def image_maps_host(cam, width, height, opt=None, **options):
    """ecal_image_maps_host: the BILINEAR maps of the host walk -> (map_x, map_y float32 [out_height, out_width], valid uint8, info dict)"""
    L = load_library()
    o = opt if opt is not None else image_options(**options)
    if image_options_error(o) or _image_sensor_error(width, height):
        _image_host_fail(L, -1, "ecal_image_maps_host", cam, width, height, o)
    shape = (int(o.out_height), int(o.out_width))
    mx, my, valid = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape, np.uint8)
    info = ImageInfo()
    st = L.ecal_image_maps_host(ctypes.byref(cam), int(width), int(height), ctypes.byref(o), mx.ctypes.data, my.ctypes.data, valid.ctypes.data,
                                ctypes.byref(info))
    if st != 0:
        _image_host_fail(L, st, "ecal_image_maps_host", cam, width, height, o)
    return mx, my, valid, info.as_dict()


class ImagePlan:
    """An ecal_image_plan of a Context (Context.image_plan): the method's tables on the device for one camera, sensor and canvas."""

    def __init__(self, ctx, cam, width, height, opt):
        L = ctx._L
        vp = ctypes.c_void_p
        self._ctx, self._L, self._h = ctx, L, None
        self.width, self.height = int(width), int(height)
        h = vp()
        ctx._check(L.ecal_image_plan_create(ctx._h, ctypes.byref(cam), max(0, int(width)), max(0, int(height)), ctypes.byref(opt), ctypes.byref(h)))
        self._h = h
        info = ImageInfo()
        ctx._check(L.ecal_image_plan_info(h, ctypes.byref(info)))
        self._info = info
        self.options = info.opt

    @property
    def info(self):
        return self._info.as_dict()

    def close(self):
        if self._h is not None and self._ctx._h is not None:
            self._L.ecal_image_plan_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _shape(self):
        return int(self.options.out_height), int(self.options.out_width)

    def maps(self):
        """ecal_image_plan_maps -> (map_x, map_y float32 [out_height, out_width], valid uint8): cv::remap's CV_32FC1 maps (BILINEAR)"""
        mx, my, valid = np.zeros(self._shape(), np.float32), np.zeros(self._shape(), np.float32), np.zeros(self._shape(), np.uint8)
        self._ctx._check(self._L.ecal_image_plan_maps(self._h, mx.ctypes.data, my.ctypes.data, valid.ctypes.data))
        return mx, my, valid

    def maps_dev(self):
        """ecal_image_plan_maps_dev -> (map_x, map_y float32 CUDA tensors [out_height, out_width], valid uint8 CUDA tensor)"""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        mx, my = torch.empty(self._shape(), dtype=torch.float32, device=dev), torch.empty(self._shape(), dtype=torch.float32, device=dev)
        valid = torch.empty(self._shape(), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            self._ctx._check(self._L.ecal_image_plan_maps_dev(self._h, mx.data_ptr(), my.data_ptr(), valid.data_ptr(),
                                                              torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
        return mx, my, valid

    def table(self):
        """ecal_image_plan_table -> (off uint32 [canvas pixels + 1], idx uint32 [n_entries], w float64 [n_entries]) (REFERENCE)"""
        n = int(self._info.n_entries)
        off = np.zeros(self._shape()[0] * self._shape()[1] + 1, np.uint32)
        idx, w = np.zeros(n, np.uint32), np.zeros(n, np.float64)
        self._ctx._check(self._L.ecal_image_plan_table(self._h, off.ctypes.data, idx.ctypes.data if n else None, w.ctypes.data if n else None))
        return off, idx, w

    def apply(self, images, minmax=False):
        """ecal_undistort_images: uint8 host frames [H, W], [H, W, C] or [N, H, W, C] -> the pictures, the same rank, on the canvas
        (with minmax=True: also float32 [N, 2], every frame's min and max before the rounding)"""
        a, rank = _frames_arg(images, self.width, self.height, self.options.channels)
        n = a.shape[0]
        out = np.zeros((n,) + self._shape() + (int(self.options.channels),), np.uint8)
        mm = np.zeros((n, 2), np.float32)
        self._ctx._check(self._L.ecal_undistort_images(self._ctx._h, self._h, a.ctypes.data if n else None, n, out.ctypes.data if n else None,
                                                       mm.ctypes.data if minmax and n else None))
        return (_frames_result(out, rank), mm) if minmax else _frames_result(out, rank)

    def apply_dev(self, tensor, minmax=False):
        """ecal_undistort_images_dev on a uint8 CUDA tensor [N, H, W, C] already on the device -> a uint8 CUDA tensor
        [N, out_height, out_width, C] (with minmax=True: also a float32 CUDA tensor [N, 2]); waits for the result."""
        import torch
        C = int(self.options.channels)
        if tensor.dtype != torch.uint8 or tensor.dim() != 4 or tuple(tensor.shape[1:]) != (self.height, self.width, C):
            raise ValueError("a uint8 CUDA tensor [N, %d, %d, %d]" % (self.height, self.width, C))
        t = tensor.contiguous()
        n = t.shape[0]
        out = torch.empty((n,) + self._shape() + (C,), dtype=torch.uint8, device=t.device)
        mm = torch.empty((n, 2), dtype=torch.float32, device=t.device)
        with torch.cuda.device(t.device):
            self._ctx._check(self._L.ecal_undistort_images_dev(self._ctx._h, self._h, t.data_ptr() if n else None, n, out.data_ptr() if n else None,
                                                               mm.data_ptr() if minmax and n else None, torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
        return (out, mm) if minmax else out


def fields_options(time_magnitude=None, time_base=None, auto_time_base=False, width=0, height=0, flip_x=False, flip_y=False, start_time=None,
                   end_time=None):
    """ecal_fields_options from ecal_fields_default_options (time_magnitude 1e-6, time_base 0, no size, no flips, start_time 0, no end
    time); None leaves a default."""
    L = load_library()
    o = FieldsOptions()
    L.ecal_fields_default_options(ctypes.byref(o))
    if time_magnitude is not None:
        o.time_magnitude = float(time_magnitude)
    if time_base is not None:
        o.time_base = int(time_base)
    o.auto_time_base = 1 if auto_time_base else 0
    o.width, o.height, o.flip_x, o.flip_y = int(width), int(height), 1 if flip_x else 0, 1 if flip_y else 0
    if start_time is not None:
        o.start_time = float(start_time)
    if end_time is not None:
        o.has_end_time, o.end_time = 1, float(end_time)
    return o


def to_fields_options(ticks_per_second=None, time_base=None, polarity_signed=False):
    """ecal_to_fields_options from ecal_to_fields_default_options (1e6 ticks a second, base 0, polarity 0 / 1)."""
    L = load_library()
    o = ToFieldsOptions()
    L.ecal_to_fields_default_options(ctypes.byref(o))
    if ticks_per_second is not None:
        o.ticks_per_second = float(ticks_per_second)
    if time_base is not None:
        o.time_base = int(time_base)
    o.polarity_signed = 1 if polarity_signed else 0
    return o


def npy_options(fields=None, columns=None, **options):
    """ecal_npy_options: fields = {"t": name, "x": ..., "y": ..., "p": ...} overrides the aliases of a structured file, columns the
    order of an (N, 4) array ("txyp"); the other options are fields_options'."""
    o = NpyOptions()
    o.fields = fields_options(**options)
    keep = []
    for k in "txyp":
        name = (fields or {}).get(k)
        if name:
            keep.append(name.encode())
            setattr(o, k + "_name", keep[-1])
    if columns:
        keep.append(columns.encode())
        o.columns = keep[-1]
    o._keep = keep
    return o


def _host_column(a):
    """a 1-D numpy array as it lies in memory (any stride) -> (array kept alive, Field)"""
    a = np.asarray(a)
    if a.ndim != 1:
        raise ValueError("a column is a 1-D array")
    if a.dtype == np.uint64:
        if a.size and int(a.max()) >= 1 << 63:
            raise ValueError("uint64 stamps beyond 2^63-1 are not taken")
        a = a.view(np.int64)
    if a.size > 1 and a.strides[0] < a.dtype.itemsize:   # (a reversed or a broadcast view)
        a = np.ascontiguousarray(a)
    return a, Field(a.ctypes.data if a.size else None, a.strides[0] if a.size > 1 else a.dtype.itemsize, field_type(a.dtype), 0)


def _default_magnitude(options, stamp_dtype_code):
    if options.get("time_magnitude") is None:
        options = dict(options, time_magnitude=1.0 if stamp_dtype_code >= 7 else 1e-6)
    return options


def events_from_fields_host(t, x, y, p, capacity=None, **options):
    """ecal_events_from_fields_host: the walk of the array ingest in plain C over numpy columns (any strides: a structured array's
    fields are taken where they lie) -> (packed records as a uint8 array [n_events * 25], info dict).  No context, no device.
    time_magnitude None: 1e-6 for integer stamps, 1.0 for float stamps.  A refusal raises EcalError with the library's text."""
    L = load_library()
    cols = [_host_column(a) for a in (t, x, y, p)]
    n = cols[0][0].size
    if any(c[0].size != n for c in cols):
        raise ValueError("the four columns must have one length")
    f = (Field * 4)(*[c[1] for c in cols])
    o = fields_options(**_default_magnitude(options, f[0].type))
    cap = n if capacity is None else int(capacity)
    out = np.zeros(cap * 25, np.uint8)
    info = FieldsInfo()
    err = ctypes.create_string_buffer(512)
    st = L.ecal_events_from_fields_host(f, n, ctypes.byref(o), out.ctypes.data if cap else None, cap, ctypes.byref(info), err, 512)
    if st != 0:
        e = EcalError(st, err.value.decode())
        e.info = info.as_dict()
        raise e
    return out[: int(info.n_events) * 25], info.as_dict()


def events_to_fields_host(events, t=np.float64, xy=np.float64, p=np.uint8, **options):
    """ecal_events_to_fields_host: packed records (bytes or a numpy uint8 array) -> ({"t", "x", "y", "p"} numpy arrays of the asked
    dtypes, info dict).  Not representable events raise EcalError (status -6) with .info["n_unrepresentable"]."""
    L = load_library()
    rec = _u8_array(events)
    n = rec.size // 25
    out = {"t": np.zeros(n, t), "x": np.zeros(n, xy), "y": np.zeros(n, xy), "p": np.zeros(n, p)}
    f = (Field * 4)(*[_host_column(out[k])[1] for k in "txyp"])
    o = to_fields_options(**options)
    info = ToFieldsInfo()
    err = ctypes.create_string_buffer(512)
    st = L.ecal_events_to_fields_host(rec.ctypes.data if n else None, n, f, ctypes.byref(o), ctypes.byref(info), err, 512)
    if st != 0:
        e = EcalError(st, err.value.decode())
        e.info = info.as_dict()
        raise e
    return out, info.as_dict()


def npy_parse_header(data, file_bytes=None, fields=None, columns=None):
    """ecal_npy_parse_header over the front of a .npy file (bytes or a numpy uint8 array; file_bytes None: `data` is the whole file)
    -> layout dict: data_offset, n_events, item_stride, version_major / _minor, fields {"t": (offset, type name), ...}.  A refusal
    raises EcalError with the library's text."""
    L = load_library()
    a = _u8_array(data)
    o = npy_options(fields=fields, columns=columns)
    lay = NpyLayout()
    err = ctypes.create_string_buffer(512)
    st = L.ecal_npy_parse_header(None, a.ctypes.data if a.size else None, a.size, 0 if file_bytes is None else int(file_bytes), ctypes.byref(o),
                                 ctypes.byref(lay), err, 512)
    if st != 0:
        raise EcalError(st, err.value.decode())
    return lay.as_dict()


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _u8_array(data):
    """bytes, bytearray, memoryview (viewed in place) or anything numpy takes as uint8 -> a flat contiguous uint8 array"""
    return np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).ravel()


class Context:
    """One ecal_ctx (one per host thread, like one DBSCAN instance per reference worker)."""

    def __init__(self, device=0):
        self._L = load_library()
        h = ctypes.c_void_p()
        st = self._L.ecal_init(int(device), ctypes.byref(h))
        if st != 0:
            raise EcalError(st, self._L.ecal_strerror(st).decode())
        self._h = h
        self.device = int(device)
        _live_contexts.add(self)

    def reload_env(self):
        """ecal_debug_reload_env: read the ECAL_* debug switches again (they are read once, at ecal_init)."""
        if getattr(self, "_h", None):
            self._check(self._L.ecal_debug_reload_env(self._h))

    def close(self):
        self._calibrate_pipe = None   # (calibrate.calibrate_stream keeps its detection pipeline's arrays with the context)
        for plan in list(getattr(self, "_image_plans", ())):   # (a plan belongs to its context and goes before it)
            plan.close()
        if getattr(self, "_h", None):
            _live_contexts.discard(self)
            self._L.ecal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st):
        if st != 0:
            msg = self._L.ecal_strerror(st).decode()
            extra = self._L.ecal_last_error(self._h).decode()
            raise EcalError(st, msg + (": " + extra if extra else ""))

    def sync(self):
        self._check(self._L.ecal_sync(self._h))

    # ---- DBSCAN (host buffers) ----
    def dbscan_batch(self, xy, slice_off, eps, minpts):
        """DBSCAN::Run per slice.  xy [N,2] float64, slice_off [S+1] uint32 -> (labels int32 [N], n_clusters uint32 [S])."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        slice_off = np.ascontiguousarray(slice_off, dtype=np.uint32)
        S = slice_off.shape[0] - 1
        if S < 0:
            raise ValueError("slice_off needs at least one entry")
        labels = np.full(xy.shape[0], -1, dtype=np.int32)
        ncl = np.zeros(max(S, 0), dtype=np.uint32)
        self._check(self._L.ecal_dbscan_batch(self._h, _ptr(xy), _ptr(slice_off), S, float(eps), int(minpts),
                                              _ptr(labels), _ptr(ncl)))
        return labels, ncl

    def debug_px_todo_counts(self, stream=None):
        """ecal_debug_px_todo_counts (tests): how many segments the first and the second pixel pass of the last dbscan_batch* call
        on this context left on their to-do lists -> (first, second); second is None when no second pass ran (no segment of the
        call could need it, or the lean tail).  stream: the stream that call ran on (None: the context's own, dbscan_batch's)."""
        L = self._L
        if stream is None:
            self.sync()
            stream = 0
        out = (ctypes.c_uint32 * 2)(0xFFFFFFFF, 0xFFFFFFFF)
        self._check(L.ecal_debug_px_todo_counts(self._h, out, stream))
        return int(out[0]), (None if out[1] == 0xFFFFFFFF else int(out[1]))

    def debug_tail_plans(self):
        """ecal_debug_tail_seen (tests), read as ecal_tail_plan (ecal_ctx.hpp) reads it under tail mode "auto": the plan the NEXT call
        of the slicing and of the DBSCAN stage takes, by what the stage's last call saw on its two lists -> {"slice": p, "dbscan": p},
        p = "lean" (both lists were empty), "semi" (the second was) or "tiered".  The caller has drained the stream of those calls."""
        L = self._L
        seen = (ctypes.c_uint32 * 16)()
        self._check(L.ecal_debug_tail_seen(self._h, seen))

        def plan(first):
            a, b = int(seen[first]), int(seen[first + 1])
            return "lean" if a == 0 and b == 0 else ("semi" if a != 0xFFFFFFFF and b == 0 else "tiered")
        return {"slice": plan(0), "dbscan": plan(2)}

    # ---- DBSCAN (device buffers, raw pointers) ----
    def dbscan_batch_dev(self, d_xy, d_seg_off, d_seg_cnt, S, n_points, max_seg_points, eps, minpts, d_labels,
                         d_n_clusters, stream=0):
        self._check(self._L.ecal_dbscan_batch_dev(self._h, d_xy, d_seg_off, d_seg_cnt, int(S), int(n_points),
                                                  int(max_seg_points), float(eps), int(minpts), d_labels,
                                                  d_n_clusters, stream))

    # ---- in-library RCCL communicator (one rank per GPU) ----
    @staticmethod
    def comm_unique_id():
        """Rank 0: the 128 bytes every rank passes to comm_init (hand them over with any transport)."""
        buf = ctypes.create_string_buffer(128)
        rc = load_library().ecal_comm_unique_id(buf)
        if rc:
            raise EcalError(rc, "ecal_comm_unique_id")
        return buf.raw

    def comm_init(self, unique_id, rank, world_size):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._check(self._L.ecal_comm_init(self._h, buf, int(rank), int(world_size)))

    def comm_destroy(self):
        self._check(self._L.ecal_comm_destroy(self._h))

    def comm_size(self):
        return self._L.ecal_comm_size(self._h)

    def comm_rank(self):
        return self._L.ecal_comm_rank(self._h)

    def comm_allreduce_fn(self):
        """(ALLREDUCE_FN, user pointer) that make a solve / calibration all-reduce through this context's communicator
        (options.allreduce = ecal_comm_allreduce, options.allreduce_user = the context) — collectives are explicit."""
        fn = ctypes.cast(self._L.ecal_comm_allreduce, ALLREDUCE_FN)
        return fn, ctypes.cast(self._h, ctypes.c_void_p)

    def comm_allreduce_sum_dev(self, d_buf, n_doubles, stream=0):
        self._check(self._L.ecal_comm_allreduce_sum_dev(self._h, d_buf, int(n_doubles), stream))

    # ---- ingest + slicing (device buffers, raw pointers) ----
    ORDER_REFERENCE, ORDER_FIRST_OCCURRENCE = 0, 1

    TIES_REFERENCE, TIES_SMALLER_PID = 0, 1

    def set_median_ties(self, mode):
        """What the composite entry points do at tied medians: "reference" (default) or "smaller_pid"."""
        code = {"reference": 0, "smaller_pid": 1, 0: 0, 1: 1}[mode]
        self._check(self._L.ecal_set_median_ties(self._h, code))

    TAIL_AUTO, TAIL_TIERED, TAIL_LEAN = 0, 1, 2

    def set_tail_mode(self, mode):
        """How the stage calls schedule their later size tiers (ecal_set_tail_mode): "auto" (default: one general tail launch per
        stage while the stage's to-do lists were empty at its previous call), "tiered" (every tier, every call), "lean"."""
        code = {"auto": 0, "tiered": 1, "lean": 2, 0: 0, 1: 1, 2: 2}[mode]
        self._check(self._L.ecal_set_tail_mode(self._h, code))

    def get_tail_mode(self):
        """The mode in force as its number (TAIL_AUTO / TAIL_TIERED / TAIL_LEAN): set_tail_mode takes it back."""
        mode = self._L.ecal_get_tail_mode(self._h)
        if mode < 0:
            self._check(mode)
        return mode

    def set_profile_ranges(self, on=True):
        """roctx ranges around the stage entry points (ecal_set_profile_ranges) for `rocprofv3 --marker-trace --kernel-trace`."""
        self._check(self._L.ecal_set_profile_ranges(self._h, 1 if on else 0))

    def set_point_order(self, order):
        """Element order of the pixel sets: "reference" (EventFrame.cpp:34-35 on libstdc++; default) or "first"."""
        code = {"reference": 0, "first": 1, 0: 0, 1: 1}[order]
        self._check(self._L.ecal_set_point_order(self._h, code))

    def point_order(self):
        return {0: "reference", 1: "first"}[self._L.ecal_get_point_order(self._h)]

    def window_bounds_dev(self, d_events, n_events, d_t0, d_t1, S, d_win_lo, d_win_hi, d_win_base, stream=0):
        self._check(self._L.ecal_window_bounds_dev(self._h, d_events, int(n_events), d_t0, d_t1, int(S), d_win_lo,
                                                   d_win_hi, d_win_base, stream))

    def sort_events_dev(self, d_events, n_events, d_sorted, stream=0):
        self._check(self._L.ecal_sort_events_dev(self._h, d_events, int(n_events), d_sorted, stream))

    def check_sorted_dev(self, d_events, n_events, d_flag, stream=0):
        self._check(self._L.ecal_check_sorted_dev(self._h, d_events, int(n_events), d_flag, stream))

    # ---- what the ingest families (text, raw, aedat, aedat4, bag, npy) share: each passes its symbol, options, info and table ----
    def _fail_with_info(self, st, info):
        """EcalError of an entry point, with the info struct it filled (first_bad_line, the needed n_events, ...) as .info"""
        try:
            self._check(st)
        except EcalError as e:
            e.info = info.as_dict()
            raise

    @staticmethod
    def _bytes_tensor(data):
        """bytes / numpy uint8 / torch uint8 (any device) as a CUDA uint8 tensor whose storage starts 16-byte aligned"""
        import torch
        if isinstance(data, torch.Tensor):
            t = data.contiguous().view(torch.uint8).reshape(-1)
        else:
            a = _u8_array(data)
            t = torch.from_numpy(a.copy()) if a.size else torch.zeros(0, dtype=torch.uint8)
        t = t.cuda()
        if t.numel() and t.data_ptr() % 16:    # (a view into a larger tensor: the kernels load 16 bytes at a time)
            t = t.clone()
        return t

    @staticmethod
    def _table_tensor(table, dtype, device):
        """a packet / message table (a numpy array of `dtype`, or a CUDA uint8 tensor of 16-byte entries) as (CUDA uint8 tensor, entries)"""
        import torch
        if table is None:
            return torch.zeros(0, dtype=torch.uint8, device=device), 0
        if isinstance(table, torch.Tensor):
            t = table.contiguous().view(torch.uint8).reshape(-1).to(device)
        else:
            a = np.ascontiguousarray(table, dtype)
            t = torch.from_numpy(a.view(np.uint8).copy()).to(device) if a.size else torch.zeros(0, dtype=torch.uint8, device=device)
        return t, t.numel() // 16

    def _payload_args(self, data, table):
        """the leading arguments of a _dev decoder: (payload tensor, table tensor or None, [d_payload, bytes] + [d_table, entries] when the
        family has a table = (table, dtype))"""
        t = self._bytes_tensor(data)
        args = [t.data_ptr() if t.numel() else None, t.numel()]
        if table is None:
            return t, None, args
        pk, n_pk = self._table_tensor(table[0], table[1], t.device)
        return t, pk, args + [pk.data_ptr() if n_pk else None, n_pk]

    def _count_dev(self, symbol, data, table, *extra):
        """an ecal_X_count_*_dev call: the payload, the table when the family has one, the family's own arguments -> the count"""
        import torch
        t, pk, args = self._payload_args(data, table)     # (t and pk hold the device memory over the call)
        n = ctypes.c_uint64()
        self._check(getattr(self._L, symbol)(self._h, *args, *extra, ctypes.byref(n), torch.cuda.current_stream().cuda_stream))
        return int(n.value)

    def _events_from(self, symbol, data, table, options, info, capacity, count):
        """an ecal_events_from_X_dev call -> (records as a uint8 CUDA tensor [n_events * 25], info dict).  capacity None: count(payload
        tensor, table tensor or None); a refusal raises with .info"""
        import torch
        t, pk, args = self._payload_args(data, table)
        cap = count(t, pk) if capacity is None else int(capacity)
        out = torch.empty(cap * 25 + 16, dtype=torch.uint8, device=t.device)
        st = getattr(self._L, symbol)(self._h, *args, ctypes.byref(options), out.data_ptr(), cap, ctypes.byref(info),
                                      torch.cuda.current_stream().cuda_stream)
        if st != 0:
            self._fail_with_info(st, info)
        return out[: int(info.n_events) * 25], info.as_dict()

    def _index_table(self, symbol, data, selector, dtype, info, capacity):
        """an ecal_X_index_* call over host bytes -> (table as a numpy array of `dtype`, info dict).  selector: the family's own
        argument (source, stream_id, byref(options)).  capacity None: counted first, where -6 only says that the table is needed"""
        fn = getattr(self._L, symbol)
        a = _u8_array(data)
        ptr = a.ctypes.data if a.size else None
        n = ctypes.c_uint64()
        if capacity is None:
            st = fn(self._h, ptr, a.size, selector, None, 0, ctypes.byref(n), ctypes.byref(info))
            if st not in (0, -6):
                self._fail_with_info(st, info)
            capacity = int(n.value)
        table = np.zeros(int(capacity), dtype)
        st = fn(self._h, ptr, a.size, selector, table.ctypes.data if table.size else None, table.size, ctypes.byref(n), ctypes.byref(info))
        if st != 0:
            self._fail_with_info(st, info)
        return table[: int(n.value)], info.as_dict()

    def _to_bin(self, symbol, src, dst, options, info):
        """an ecal_X_to_bin_file call -> info dict; a refusal raises with .info"""
        st = getattr(self._L, symbol)(self._h, os.fsencode(src), os.fsencode(dst), ctypes.byref(options), ctypes.byref(info))
        if st != 0:
            self._fail_with_info(st, info)
        return info.as_dict()

    def _stream_from_file(self, symbol, path, options, info):
        """an ecal_stream_create_from_X_file call, the stream's records copied out -> (events, info dict, t_first, t_last)"""
        h = ctypes.c_void_p()
        st = getattr(self._L, symbol)(self._h, os.fsencode(path), ctypes.byref(options), ctypes.byref(h), ctypes.byref(info))
        if st != 0:
            self._fail_with_info(st, info)
        events, t_first, t_last = self._stream_records(h)
        return events, info.as_dict(), t_first, t_last

    # ---- text ingest: "stamp x y polarity" lines parsed in HBM (ecal_events_from_text_dev and the file forms) ----
    def text_options(self, time_magnitude=1e-6, time_base=None, end_stamp=None, start_time=None, end_time=None, duplicate_last=True):
        """ecal_text_options from ecal_text_default_options: time_base None = the first record line's stamp, end_stamp None = no
        break, start_time None = -inf, end_time None = to the end, duplicate_last = the reference's repeated last record."""
        L = self._L
        o = TextOptions()
        L.ecal_text_default_options(ctypes.byref(o))
        o.time_magnitude = float(time_magnitude)
        if time_base is not None:
            o.has_time_base, o.time_base = 1, int(time_base)
        if end_stamp is not None:
            o.has_end_stamp, o.end_stamp = 1, int(end_stamp)
        if start_time is not None:
            o.start_time = float(start_time)
        if end_time is not None:
            o.has_end_time, o.end_time = 1, float(end_time)
        o.duplicate_last = 1 if duplicate_last else 0
        return o

    def text_count_lines(self, text):
        """ecal_text_count_lines_dev: the lines of the text (lines + 1 bounds the records)."""
        return self._count_dev("ecal_text_count_lines_dev", text, None)

    def events_from_text(self, text, capacity=None, **options):
        """ecal_events_from_text_dev: text (bytes, a numpy uint8 array or a torch uint8 tensor; a CUDA tensor is parsed where it is)
        -> (packed 25-byte records in file order as a uint8 CUDA tensor [n_events * 25], info dict).  options: text_options'.
        capacity None: lines + 1 records (always enough); a smaller one raises EcalError with status -6 and .info["n_events"] =
        the count needed.  A malformed line raises EcalError with status -1 and .info["first_bad_line"]."""
        return self._events_from("ecal_events_from_text_dev", text, None, self.text_options(**options), TextInfo(), capacity,
                                 lambda t, _: self.text_count_lines(t) + 1)

    def text_to_bin(self, txt_path, bin_path, **options):
        """ecal_text_to_bin_file: the .bin the reference's txt2bin tool writes from txt_path (file order, no sort) -> info dict."""
        return self._to_bin("ecal_text_to_bin_file", txt_path, bin_path, self.text_options(**options), TextInfo())

    def stream_from_text_file(self, path, **options):
        """ecal_stream_create_from_text_file, its records copied into a uint8 CUDA tensor (time order: the stream sorts when the
        file is not) -> (events, info dict, t_first, t_last)."""
        return self._stream_from_file("ecal_stream_create_from_text_file", path, self.text_options(**options), TextInfo())

    def _stream_records(self, h):
        """the records of the ecal_stream h copied into a uint8 CUDA tensor, its first and last time; destroys the stream"""
        import torch
        L = self._L
        try:
            n = int(L.ecal_stream_size(h))
            events = torch.empty(n * 25, dtype=torch.uint8, device="cuda:%d" % self.device)
            t0, t1 = ctypes.c_double(), ctypes.c_double()
            self._check(L.ecal_stream_times(h, ctypes.byref(t0), ctypes.byref(t1)))
            if n:
                self._check(L.ecal_copy_dev(self._h, events.data_ptr(), L.ecal_stream_data(h), n * 25,
                                            torch.cuda.current_stream(events.device).cuda_stream, 1))
        finally:
            L.ecal_stream_destroy(h)
        return events, t0.value, t1.value

    # ---- raw ingest: Prophesee EVT3 / EVT2 payloads decoded in HBM (ecal_events_from_raw_dev and the file forms) ----
    def raw_options(self, format=None, time_base=0, width=0, height=0, start_time=None, end_time=None):
        """ecal_raw_options from ecal_raw_default_options: format "EVT2" / "EVT3" / None (from the file header), time_base in
        microseconds of the camera's clock, width / height 0 = no bound, start_time None = -inf, end_time None = to the end."""
        L = self._L
        o = RawOptions()
        L.ecal_raw_default_options(ctypes.byref(o))
        o.format, o.time_base, o.width, o.height = raw_format(format), int(time_base), int(width), int(height)
        if start_time is not None:
            o.start_time = float(start_time)
        if end_time is not None:
            o.has_end_time, o.end_time = 1, float(end_time)
        return o

    def raw_block_words(self, format):
        """ecal_raw_block_words: words per decode block of this build."""
        return int(self._L.ecal_raw_block_words(raw_format(format)))

    def raw_count_events(self, payload, format):
        """ecal_raw_count_events_dev: the events the payload's words emit before any drop (always a sufficient capacity)."""
        return self._count_dev("ecal_raw_count_events_dev", payload, None, raw_format(format))

    def events_from_raw(self, payload, format, capacity=None, **options):
        """ecal_events_from_raw_dev: payload (bytes, a numpy uint8 array or a torch uint8 tensor; a CUDA tensor is decoded where it
        is; no file header) -> (packed 25-byte records in file order as a uint8 CUDA tensor [n_events * 25], info dict).  options:
        raw_options'.  capacity None: raw_count_events (always enough); a smaller one raises EcalError with status -6 and
        .info["n_events"] = the count needed."""
        return self._events_from("ecal_events_from_raw_dev", payload, None, self.raw_options(format=format, **options), RawInfo(), capacity,
                                 lambda t, _: self.raw_count_events(t, format))

    def raw_to_bin(self, raw_path, bin_path, **options):
        """ecal_raw_to_bin_file: the records of the .raw file (file order, no sort) as a .bin of the reference's layout -> info dict."""
        return self._to_bin("ecal_raw_to_bin_file", raw_path, bin_path, self.raw_options(**options), RawInfo())

    def stream_from_raw_file(self, path, **options):
        """ecal_stream_create_from_raw_file, its records copied into a uint8 CUDA tensor (time order: the stream sorts when the
        file is not) -> (events, info dict, t_first, t_last)."""
        return self._stream_from_file("ecal_stream_create_from_raw_file", path, self.raw_options(**options), RawInfo())

    # ---- aedat ingest: iniVation AEDAT 3.1 / 2.0 payloads decoded in HBM (ecal_events_from_aedat_dev and the file forms) ----
    def aedat_options(self, format=None, source=-1, time_base=0, width=0, height=0, flip_x=False, flip_y=False, start_time=None,
                      end_time=None):
        """ecal_aedat_options from ecal_aedat_default_options: format "3.1" / "2.0" / None (from the file's version line), source >= 0
        = only polarity packets of that eventSource (3.1 file forms and the indexer), time_base in microseconds of the camera's clock,
        width / height 0 = no bound, flip_x / flip_y need them, start_time None = -inf, end_time None = to the end."""
        L = self._L
        o = AedatOptions()
        L.ecal_aedat_default_options(ctypes.byref(o))
        o.format, o.source, o.time_base, o.width, o.height = aedat_format(format), int(source), int(time_base), int(width), int(height)
        o.flip_x, o.flip_y = int(bool(flip_x)), int(bool(flip_y))
        if start_time is not None:
            o.start_time = float(start_time)
        if end_time is not None:
            o.has_end_time, o.end_time = 1, float(end_time)
        return o

    def aedat_block_events(self, format):
        """ecal_aedat_block_events: event slots / records per decode block of this build."""
        return int(self._L.ecal_aedat_block_events(aedat_format(format)))

    def aedat_parse_header(self, data, format=None):
        """ecal_aedat_parse_header: the first bytes of a file -> (format number in force, header_bytes)."""
        L = self._L
        data = bytes(data)
        fmt, hb = ctypes.c_int(aedat_format(format)), ctypes.c_uint64()
        self._check(L.ecal_aedat_parse_header(self._h, data, len(data), ctypes.byref(fmt), ctypes.byref(hb)))
        return int(fmt.value), int(hb.value)

    def aedat_index_packets(self, payload, source=-1, capacity=None):
        """ecal_aedat_index_packets over a 3.1 payload in host memory (bytes or a numpy uint8 array) -> (table as a numpy array of
        AEDAT_PACKET_DTYPE, info dict).  capacity None: counted first; a smaller one raises EcalError with status -6 and
        .info["n_packets"] = the count needed."""
        return self._index_table("ecal_aedat_index_packets", payload, int(source), AEDAT_PACKET_DTYPE, AedatInfo(), capacity)

    def aedat_count_events(self, payload, format, packets=None):
        """ecal_aedat_count_events_dev: the events before any drop (always a sufficient capacity)."""
        return self._count_dev("ecal_aedat_count_events_dev", payload, (packets, AEDAT_PACKET_DTYPE), aedat_format(format))

    def events_from_aedat(self, payload, format, packets=None, capacity=None, **options):
        """ecal_events_from_aedat_dev: payload (bytes, a numpy uint8 array or a torch uint8 tensor; a CUDA tensor is decoded where it
        is; no file header) and, for "3.1", the packet table of aedat_index_packets -> (packed 25-byte records in file order as a
        uint8 CUDA tensor [n_events * 25], info dict).  options: aedat_options'.  capacity None: aedat_count_events (always enough); a
        smaller one raises EcalError with status -6 and .info["n_events"] = the count needed."""
        return self._events_from("ecal_events_from_aedat_dev", payload, (packets, AEDAT_PACKET_DTYPE), self.aedat_options(format=format, **options),
                                 AedatInfo(), capacity, lambda t, pk: self.aedat_count_events(t, format, pk))

    def aedat_to_bin(self, aedat_path, bin_path, **options):
        """ecal_aedat_to_bin_file: the records of the .aedat file (file order, no sort) as a .bin of the reference's layout -> info dict."""
        return self._to_bin("ecal_aedat_to_bin_file", aedat_path, bin_path, self.aedat_options(**options), AedatInfo())

    def stream_from_aedat_file(self, path, **options):
        """ecal_stream_create_from_aedat_file, its records copied into a uint8 CUDA tensor (time order: the stream sorts when the
        file is not) -> (events, info dict, t_first, t_last)."""
        return self._stream_from_file("ecal_stream_create_from_aedat_file", path, self.aedat_options(**options), AedatInfo())

    # ---- aedat4 ingest: iniVation AEDAT 4 files (LZ4 packets) inflated and decoded in HBM (ecal_events_from_aedat4_dev and the file forms) ----
    def aedat4_options(self, compression=None, stream_id=-1, time_base=None, width=0, height=0, flip_x=False, flip_y=False,
                       start_time=None, end_time=None, max_inflated_bytes=None):
        """ecal_aedat4_options from ecal_aedat4_default_options: compression "none" / "lz4" (the _dev forms; the file forms take the
        header's), stream_id -1 = found by its identifier, time_base None = automatic (the first event's whole second; file forms
        only), else int64 microseconds of epoch time, width / height 0 = no upper bound, flip_x / flip_y need them, start_time None =
        -inf, end_time None = to the end, max_inflated_bytes None = the default."""
        L = self._L
        o = Aedat4Options()
        L.ecal_aedat4_default_options(ctypes.byref(o))
        o.compression, o.stream_id, o.width, o.height = aedat4_compression(compression), int(stream_id), int(width), int(height)
        if time_base is not None:
            o.auto_time_base, o.time_base = 0, int(time_base)
        o.flip_x, o.flip_y = int(bool(flip_x)), int(bool(flip_y))
        if start_time is not None:
            o.start_time = float(start_time)
        if end_time is not None:
            o.has_end_time, o.end_time = 1, float(end_time)
        if max_inflated_bytes is not None:
            o.max_inflated_bytes = int(max_inflated_bytes)
        return o

    def aedat4_block_events(self):
        """ecal_aedat4_block_events: event slots per decode block of this build."""
        return int(self._L.ecal_aedat4_block_events())

    def aedat4_parse_header(self, data, file_bytes=None):
        """ecal_aedat4_parse_header: the first bytes of a file of file_bytes bytes (None: these are all of it) -> (compression,
        packets_begin, packets_end)."""
        L = self._L
        data = bytes(data)
        c, b, e = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(L.ecal_aedat4_parse_header(self._h, data, len(data), len(data) if file_bytes is None else int(file_bytes), ctypes.byref(c),
                                               ctypes.byref(b), ctypes.byref(e)))
        return int(c.value), int(b.value), int(e.value)

    def aedat4_index_packets(self, file_bytes, stream_id=-1, capacity=None):
        """ecal_aedat4_index_packets over a whole file in host memory (bytes or a numpy uint8 array) -> (table as a numpy array of
        AEDAT4_PACKET_DTYPE, info dict).  capacity None: counted first; a smaller one raises EcalError with status -6."""
        return self._index_table("ecal_aedat4_index_packets", file_bytes, int(stream_id), AEDAT4_PACKET_DTYPE, Aedat4Info(), capacity)

    def aedat4_count_events(self, file_bytes, compression, packets, max_inflated_bytes=None):
        """ecal_aedat4_count_events_dev: the events before any drop (always a sufficient capacity)."""
        o = self.aedat4_options(compression=compression, max_inflated_bytes=max_inflated_bytes)
        return self._count_dev("ecal_aedat4_count_events_dev", file_bytes, (packets, AEDAT4_PACKET_DTYPE), ctypes.byref(o))

    def events_from_aedat4(self, file_bytes, compression, packets, capacity=None, time_base=0, **options):
        """ecal_events_from_aedat4_dev: the whole file (bytes, a numpy uint8 array or a torch uint8 tensor; a CUDA tensor is decoded
        where it is) and the packet table of aedat4_index_packets -> (packed 25-byte records in file order as a uint8 CUDA tensor
        [n_events * 25], info dict).  compression "none" / "lz4" is explicit, time_base too (microseconds, default 0).  options:
        aedat4_options'.  capacity None: aedat4_count_events (always enough); a smaller one raises EcalError with status -6 and
        .info["n_events"] = the count needed."""
        return self._events_from("ecal_events_from_aedat4_dev", file_bytes, (packets, AEDAT4_PACKET_DTYPE),
                                 self.aedat4_options(compression=compression, time_base=time_base, **options), Aedat4Info(), capacity,
                                 lambda t, pk: self.aedat4_count_events(t, compression, pk, options.get("max_inflated_bytes")))

    def aedat4_to_bin(self, aedat4_path, bin_path, **options):
        """ecal_aedat4_to_bin_file: the records of the .aedat4 file (file order, no sort) as a .bin of the reference's layout -> info dict."""
        return self._to_bin("ecal_aedat4_to_bin_file", aedat4_path, bin_path, self.aedat4_options(**options), Aedat4Info())

    def stream_from_aedat4_file(self, path, **options):
        """ecal_stream_create_from_aedat4_file, its records copied into a uint8 CUDA tensor (time order: the stream sorts when the
        file is not) -> (events, info dict, t_first, t_last)."""
        return self._stream_from_file("ecal_stream_create_from_aedat4_file", path, self.aedat4_options(**options), Aedat4Info())

    # ---- bag ingest: ROS 1 bags of dvs_msgs/EventArray messages decoded in HBM (ecal_events_from_bag_dev and the file forms) ----
    def bag_options(self, topic=None, type=None, time_base=None, width=0, height=0, flip_x=False, flip_y=False, start_time=None,
                    end_time=None):
        """ecal_bag_options from ecal_bag_default_options: topic / type None = every connection of an event type (one topic),
        time_base None = automatic (the first event's whole seconds), else int64 nanoseconds of epoch time, width / height 0 = no
        bound, flip_x / flip_y need them, start_time None = -inf, end_time None = to the end."""
        L = self._L
        o = BagOptions()
        L.ecal_bag_default_options(ctypes.byref(o))
        o.topic = os.fsencode(topic) if topic else None
        o.type = os.fsencode(type) if type else None
        if time_base is not None:
            o.auto_time_base, o.time_base = 0, int(time_base)
        o.width, o.height = int(width), int(height)
        o.flip_x, o.flip_y = int(bool(flip_x)), int(bool(flip_y))
        if start_time is not None:
            o.start_time = float(start_time)
        if end_time is not None:
            o.has_end_time, o.end_time = 1, float(end_time)
        return o

    def bag_block_events(self):
        """ecal_bag_block_events: event slots per decode block of this build."""
        return int(self._L.ecal_bag_block_events())

    def bag_index_messages(self, data, topic=None, type=None, capacity=None):
        """ecal_bag_index_messages over a bag's bytes in host memory (bytes or a numpy uint8 array) -> (table as a numpy array of
        BAG_MESSAGE_DTYPE, info dict; info["first_stamp_ns"] is the automatic time base).  capacity None: counted first; a smaller
        one raises EcalError with status -6 and .info["n_messages"] = the count needed."""
        o = self.bag_options(topic=topic, type=type)
        return self._index_table("ecal_bag_index_messages", data, ctypes.byref(o), BAG_MESSAGE_DTYPE, BagInfo(), capacity)

    def bag_count_events(self, data, messages):
        """ecal_bag_count_events_dev: the events before any drop (always a sufficient capacity)."""
        return self._count_dev("ecal_bag_count_events_dev", data, (messages, BAG_MESSAGE_DTYPE))

    def events_from_bag(self, data, messages, capacity=None, **options):
        """ecal_events_from_bag_dev: the whole bag (bytes, a numpy uint8 array or a torch uint8 tensor; a CUDA tensor is decoded where
        it is) and the message table of bag_index_messages -> (packed 25-byte records in file order as a uint8 CUDA tensor
        [n_events * 25], info dict).  options: bag_options' — the device form needs an explicit time_base (the indexer's
        first_stamp_ns is the automatic one); without one the library refuses the call.  capacity None: bag_count_events (always
        enough); a smaller one raises EcalError with status -6 and .info["n_events"] = the count needed."""
        return self._events_from("ecal_events_from_bag_dev", data, (messages, BAG_MESSAGE_DTYPE), self.bag_options(**options), BagInfo(), capacity,
                                 self.bag_count_events)

    def bag_to_bin(self, bag_path, bin_path, **options):
        """ecal_bag_to_bin_file: the records of the .bag file (file order, no sort) as a .bin of the reference's layout -> info dict."""
        return self._to_bin("ecal_bag_to_bin_file", bag_path, bin_path, self.bag_options(**options), BagInfo())

    def stream_from_bag_file(self, path, **options):
        """ecal_stream_create_from_bag_file, its records copied into a uint8 CUDA tensor (time order: the stream sorts when the file
        is not) -> (events, info dict, t_first, t_last).  info["time_base"] is the base in force (nanoseconds)."""
        return self._stream_from_file("ecal_stream_create_from_bag_file", path, self.bag_options(**options), BagInfo())

    # ---- array ingest: columns packed into records in HBM, records unpacked into columns, .npy files (ecal_events_from_fields_dev, ...) ----
    def fields_block_events(self):
        """ecal_fields_block_events: events per block of the array ingest's kernels."""
        return int(self._L.ecal_fields_block_events())

    def _device_column(self, a):
        """a column (a numpy array, or a torch tensor on any device; a CUDA tensor is taken where it is, a 1-D strided view included)
        -> (tensor kept alive, Field over device memory, length)"""
        import torch
        if isinstance(a, torch.Tensor):
            if a.dim() != 1:
                raise ValueError("a column is a 1-D array")
            if a.is_cuda and (a.numel() < 2 or a.stride(0) >= 1):
                n = a.numel()
                return a, Field(a.data_ptr() if n else None, (a.stride(0) if n > 1 else 1) * a.element_size(), field_type(a.dtype), 0), n
            a = a.cpu().contiguous().numpy()
        h, f = _host_column(a)
        h = np.ascontiguousarray(h)      # (a strided host column goes up as a copy of its own: events_from_structured keeps the items)
        t = torch.from_numpy(h.view(np.uint8).copy()).to("cuda:%d" % self.device) if h.size else torch.zeros(0, dtype=torch.uint8, device="cuda:%d" % self.device)
        return t, Field(t.data_ptr() if h.size else None, h.dtype.itemsize, f.type, 0), h.size

    def events_from_fields_dev(self, fields, n, options, d_events, capacity, stream=0):
        """ecal_events_from_fields_dev, raw: fields = (Field * 4) over device memory -> info dict; raises with .info on a refusal"""
        L = self._L
        info = FieldsInfo()
        st = L.ecal_events_from_fields_dev(self._h, fields, n, ctypes.byref(options), d_events, capacity, ctypes.byref(info), stream)
        if st != 0:
            self._fail_with_info(st, info)
        return info.as_dict()

    def events_from_arrays(self, t, x, y, p, capacity=None, **options):
        """ecal_events_from_fields_dev: four columns (numpy arrays or torch tensors of one length; a CUDA tensor is taken where it
        is, 1-D strided views included; a numpy uint64 stamp array is checked below 2^63 and viewed as int64) -> (packed 25-byte
        records in input order as a uint8 CUDA tensor [n_events * 25], info dict).  options: fields_options'; time_magnitude None:
        1e-6 for integer stamps, 1.0 for float stamps.  capacity None: the input's length (always enough); a smaller one raises
        EcalError with status -6 and .info["n_events"] = the count needed."""
        import torch
        cols = [self._device_column(a) for a in (t, x, y, p)]
        n = cols[0][2]
        if any(c[2] != n for c in cols):
            raise ValueError("the four columns must have one length")
        f = (Field * 4)(*[c[1] for c in cols])
        o = fields_options(**_default_magnitude(options, f[0].type))
        cap = n if capacity is None else int(capacity)
        out = torch.empty(cap * 25 + 16, dtype=torch.uint8, device="cuda:%d" % self.device)
        info = self.events_from_fields_dev(f, n, o, out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
        return out[: info["n_events"] * 25], info

    @staticmethod
    def _structured_roles(dtype, fields=None):
        alias = {"t": ("t", "ts", "time", "timestamp"), "x": ("x",), "y": ("y",), "p": ("p", "pol", "polarity")}
        roles = {}
        for k in "txyp":
            want = (fields or {}).get(k)
            hits = [name for name in dtype.names if (name == want if want else name.lower() in alias[k])]
            if len(hits) != 1:
                raise ValueError("structured array: %s field for %s (names: %s)" % ("no" if not hits else "more than one", k, ", ".join(dtype.names)))
            roles[k] = hits[0]
        return roles

    def events_from_structured(self, arr, fields=None, capacity=None, **options):
        """a 1-D structured numpy array (packed or aligned, 13-, 14-, 16-byte items alike) uploaded once, as it lies, and packed on the
        device with the fields pointing into the items.  Names are matched without case — t|ts|time|timestamp, x, y, p|pol|polarity
        — or given as fields = {"t": name, ...}.  -> (records as a uint8 CUDA tensor, info dict)"""
        import torch
        arr = np.ascontiguousarray(arr)
        if arr.ndim != 1 or arr.dtype.names is None:
            raise ValueError("a 1-D structured array")
        roles = self._structured_roles(arr.dtype, fields)
        n = arr.size
        d = torch.from_numpy(arr.view(np.uint8).copy()).to("cuda:%d" % self.device) if n else torch.zeros(0, dtype=torch.uint8, device="cuda:%d" % self.device)
        f = (Field * 4)()
        for k, role in enumerate("txyp"):
            dt, off = arr.dtype.fields[roles[role]][:2]
            if dt == np.uint64:
                if n and int(arr[roles[role]].max()) >= 1 << 63:
                    raise ValueError("uint64 stamps beyond 2^63-1 are not taken")
                dt = np.dtype(np.int64)
            f[k] = Field(d.data_ptr() + off if n else None, arr.dtype.itemsize, field_type(dt), 0)
        o = fields_options(**_default_magnitude(options, f[0].type))
        cap = n if capacity is None else int(capacity)
        out = torch.empty(cap * 25 + 16, dtype=torch.uint8, device="cuda:%d" % self.device)
        info = self.events_from_fields_dev(f, n, o, out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
        return out[: info["n_events"] * 25], info

    def stream_from_arrays(self, t, x, y, p, **options):
        """ecal_stream_create_from_fields: HOST columns (numpy arrays, any strides) uploaded as they lie and packed on the device, the
        records copied into a uint8 CUDA tensor (time order: the stream sorts when the input is not)
        -> (events, info dict, t_first, t_last).  auto_time_base=True: the base is element 0's stamp."""
        L = self._L
        vp = ctypes.c_void_p
        cols = [_host_column(a) for a in (t, x, y, p)]
        n = cols[0][0].size
        if any(c[0].size != n for c in cols):
            raise ValueError("the four columns must have one length")
        f = (Field * 4)(*[c[1] for c in cols])
        o = fields_options(**_default_magnitude(options, f[0].type))
        info = FieldsInfo()
        h = vp()
        st = L.ecal_stream_create_from_fields(self._h, f, n, ctypes.byref(o), ctypes.byref(h), ctypes.byref(info))
        if st != 0:
            self._fail_with_info(st, info)
        events, t_first, t_last = self._stream_records(h)
        return events, info.as_dict(), t_first, t_last

    def events_to_fields_dev(self, d_events, n, fields, options, stream=0):
        """ecal_events_to_fields_dev, raw: fields = (Field * 4) over device memory -> info dict; raises with .info on a refusal"""
        L = self._L
        info = ToFieldsInfo()
        st = L.ecal_events_to_fields_dev(self._h, d_events, n, fields, ctypes.byref(options), ctypes.byref(info), stream)
        if st != 0:
            self._fail_with_info(st, info)
        return info.as_dict()

    def events_to_arrays(self, events, t=np.float64, xy=np.float64, p=np.uint8, **options):
        """ecal_events_to_fields_dev: packed records (a torch uint8 tensor on any device, a numpy array, bytes) -> a dict of CUDA
        tensors "t", "x", "y", "p" of the asked numpy dtypes (bool for p: a torch.bool tensor).  options: ticks_per_second (1e6),
        time_base, polarity_signed.  Events that are not representable raise EcalError with status -6 and
        .info["n_unrepresentable"]."""
        import torch
        rec, n = self._records_arg(events)
        out, f = {}, (Field * 4)()
        for k, (name, dt) in enumerate((("t", t), ("x", xy), ("y", xy), ("p", p))):
            dt = np.dtype(dt)
            raw = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device=rec.device)
            out[name] = raw.view(getattr(torch, "bool" if dt == np.bool_ else dt.name))
            f[k] = Field(raw.data_ptr() if n else None, dt.itemsize, field_type(dt), 0)
        self.events_to_fields_dev(rec.data_ptr() if n else None, n, f, to_fields_options(**options), torch.cuda.current_stream(rec.device).cuda_stream)
        return out

    @staticmethod
    def _npy_magnitude(path, fields, columns, options):
        """time_magnitude None: by the stamp's type in the file's header, as events_from_arrays does (a file the parser refuses is
        left to the library call, which says why)"""
        if options.get("time_magnitude") is None:
            try:
                with open(path, "rb") as f:
                    head = f.read(1 << 20)
                lay = npy_parse_header(head, file_bytes=os.path.getsize(path), fields=fields, columns=columns)
                options = dict(options, time_magnitude=1.0 if lay["fields"]["t"][1] in ("F32", "F64") else 1e-6)
            except (OSError, EcalError):
                pass
        return options

    def npy_to_bin(self, npy_path, bin_path, fields=None, columns=None, **options):
        """ecal_npy_to_bin_file: the records of the .npy file (file order, no sort) as a .bin of the reference's layout -> info dict.
        options: fields_options'; time_magnitude None: 1e-6 for integer stamps, 1.0 for float stamps."""
        options = self._npy_magnitude(npy_path, fields, columns, options)
        return self._to_bin("ecal_npy_to_bin_file", npy_path, bin_path, npy_options(fields=fields, columns=columns, **options), FieldsInfo())

    def stream_from_npy_file(self, path, fields=None, columns=None, **options):
        """ecal_stream_create_from_npy_file, its records copied into a uint8 CUDA tensor (time order: the stream sorts when the file
        is not) -> (events, info dict, t_first, t_last).  options as npy_to_bin."""
        options = self._npy_magnitude(path, fields, columns, options)
        return self._stream_from_file("ecal_stream_create_from_npy_file", path, npy_options(fields=fields, columns=columns, **options),
                                      FieldsInfo())

    def stream_to_npy(self, events, npy_path):
        """ecal_stream_to_npy_file: packed records (time-sorted by the stream when they are not) as a .npy of the packed dtype
        [('t','<f8'),('x','<f8'),('y','<f8'),('p','u1')] — numpy's header and the records' bytes as they are."""
        import torch
        L = self._L
        h = self._host_stream(events.cpu().numpy() if isinstance(events, torch.Tensor) else
                              np.frombuffer(events, np.uint8) if isinstance(events, (bytes, bytearray, memoryview)) else events)
        try:
            self._check(L.ecal_stream_to_npy_file(self._h, h, os.fsencode(npy_path)))
        finally:
            L.ecal_stream_destroy(h)

    # ---- pixel activity / hot pixels (ecal_pixel_activity_dev, ecal_filter_events_dev and the chain) ----
    def _records_arg(self, events):
        """packed 25-byte records (a torch uint8 tensor on any device, a numpy array, bytes) -> (contiguous uint8 CUDA tensor, count);
        a contiguous CUDA tensor is taken where it is, whatever its alignment"""
        import torch
        if isinstance(events, torch.Tensor):
            t = events if events.is_cuda else events.to("cuda:%d" % self.device)
        else:
            a = np.frombuffer(events, np.uint8) if isinstance(events, (bytes, bytearray, memoryview)) else np.asarray(events, np.uint8).ravel()
            t = torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:%d" % self.device)
        t = t.contiguous().view(torch.uint8).reshape(-1)
        assert t.numel() % 25 == 0, "packed 25-byte event records"
        return t, t.numel() // 25

    def pixel_activity_dev(self, d_events, n_events, width, height, d_counts, d_totals=None, stream=0):
        """ecal_pixel_activity_dev: raw device pointers; d_counts [2][height][width] u32 and d_totals (ACTIVITY_TOTALS, or None) are
        zeroed by the call; no host synchronisation."""
        L = self._L
        self._check(L.ecal_pixel_activity_dev(self._h, d_events, int(n_events), int(width), int(height), d_counts, d_totals, stream))

    def filter_events_dev(self, d_events, n_events, d_mask, width, height, d_out, d_count, d_totals=None, stream=0):
        """ecal_filter_events_dev: raw device pointers; d_mask [height * width] u8 (non-zero: remove), d_out room for n_events
        records, d_count one u32, d_totals FILTER_TOTALS or None; no host synchronisation."""
        L = self._L
        self._check(L.ecal_filter_events_dev(self._h, d_events, int(n_events), d_mask, int(width), int(height), d_out, d_count, d_totals, stream))

    def pixel_activity(self, events, width, height):
        """How many events every pixel fired: (counts [2, H, W] int64 CUDA tensor whose values are the call's uint32 counts — plane 0
        the events with polarity byte 0, plane 1 the others —, totals: one ACTIVITY_TOTALS record).  Events whose x or y is not a
        whole number inside the sensor are counted in totals["n_off_grid"] and nowhere in the map."""
        import torch
        t, n = self._records_arg(events)
        W, H = int(width), int(height)
        if not (1 <= W <= 4096 and 1 <= H <= 4096):   # (sizes that the call itself refuses must not be allocated first)
            raise EcalError(-1, "invalid argument: ecal_pixel_activity: width and height from 1 to 4096")
        counts = torch.empty((2, H, W), dtype=torch.int32, device=t.device)
        tot = torch.empty(3, dtype=torch.int64, device=t.device)
        with torch.cuda.device(t.device):
            self.pixel_activity_dev(t.data_ptr() if n else None, n, W, H, counts.data_ptr(), tot.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        return counts.to(torch.int64) & 0xFFFFFFFF, tot.cpu().numpy().view(ACTIVITY_TOTALS)[0]

    def filter_events(self, events, mask):
        """The events whose pixel is not masked, byte for byte and in input order: (events: uint8 CUDA tensor [n_kept * 25], totals: one
        FILTER_TOTALS record).  mask: [H, W], non-zero / True = remove (a numpy array or a torch tensor).  Off-grid events stay."""
        import torch
        t, n = self._records_arg(events)
        if isinstance(mask, torch.Tensor):
            m = (mask != 0).to(torch.uint8).to(t.device).contiguous()
        else:
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)).to(t.device)
        if m.dim() != 2:
            raise ValueError("mask must be [H, W]")
        H, W = int(m.shape[0]), int(m.shape[1])
        out = torch.empty(n * 25, dtype=torch.uint8, device=t.device)
        cnt = torch.empty(1, dtype=torch.int32, device=t.device)
        tot = torch.empty(4, dtype=torch.int64, device=t.device)
        with torch.cuda.device(t.device):
            self.filter_events_dev(t.data_ptr() if n else None, n, m.data_ptr() if m.numel() else None, W, H, out.data_ptr() if n else None,
                                   cnt.data_ptr(), tot.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        kept = int(cnt.item()) & 0xFFFFFFFF
        return out[: kept * 25], tot.cpu().numpy().view(FILTER_TOTALS)[0]

    def remove_hot_pixels(self, events, width=346, height=260, extra_mask=None, **options):
        """The chain of ecal_stream_remove_hot_pixels on a tensor of records: pixel_activity -> the counts to the host ->
        hot_pixel_mask (options: quantile_permille, min_count, factor) -> filter_events.  Returns (events, info): info is
        ecal_hot_pixel_info as a dict whose event fields are the filter's totals, with `mask` [H, W] bool and `counts` [2, H, W]
        uint32 (numpy)."""
        t, n = self._records_arg(events)
        counts, _ = self.pixel_activity(t, width, height)
        counts = counts.cpu().numpy().astype(np.uint32)
        mask, info = hot_pixel_mask(counts, extra_mask=extra_mask, **options)
        out, tot = self.filter_events(t, mask)
        for k in ("n_events", "n_off_grid", "n_removed", "n_kept"):
            info[k] = int(tot[k])
        info["mask"], info["counts"] = mask, counts
        return out, info

    def stream_remove_hot_pixels(self, events, width=346, height=260, extra_mask=None, **options):
        """ecal_stream_remove_hot_pixels over an ecal_stream made of the host records `events` (the C++ shim's way) -> (events as a
        uint8 CUDA tensor, info dict with `mask` and `counts`)."""
        L = self._L
        vp = ctypes.c_void_p
        ev = np.ascontiguousarray(np.asarray(events, np.uint8).ravel())
        assert ev.size % 25 == 0, "packed 25-byte event records"
        o = hot_pixel_options(width=width, height=height, **options)
        H, W = int(o.height), int(o.width)
        ok = 1 <= W <= 4096 and 1 <= H <= 4096
        extra = np.ascontiguousarray(np.asarray(extra_mask) != 0, np.uint8) if extra_mask is not None else None
        mask = np.zeros((H, W) if ok else (0, 0), np.uint8)
        counts = np.zeros((2, H, W) if ok else (2, 0, 0), np.uint32)
        info = HotPixelInfo()
        h_in, h_out = vp(), vp()
        self._check(L.ecal_stream_create(self._h, _ptr(ev) if ev.size else None, ev.size // 25, ctypes.byref(h_in)))
        try:
            self._check(L.ecal_stream_remove_hot_pixels(self._h, h_in, ctypes.byref(o), extra.ctypes.data if extra is not None and extra.size else None,
                                                        ctypes.byref(h_out), mask.ctypes.data if mask.size else None,
                                                        counts.ctypes.data if counts.size else None, ctypes.byref(info)))
        finally:
            L.ecal_stream_destroy(h_in)
        out, _, _ = self._stream_records(h_out)
        d = info.as_dict()
        d["mask"], d["counts"] = mask.astype(bool), counts
        return out, d

    # ---- noise filter (ecal_noise_verdict_dev, ecal_denoise_events_dev and the stream call) ----
    def noise_verdict_dev(self, d_events, n_events, opt, d_verdict, d_totals=None, stream=0):
        """ecal_noise_verdict_dev: raw device pointers; opt a NoiseOptions or None (the defaults), d_verdict [n_events] u8, d_totals
        FILTER_TOTALS or None; no host synchronisation."""
        L = self._L
        self._check(L.ecal_noise_verdict_dev(self._h, d_events, int(n_events), ctypes.byref(opt) if opt is not None else None, d_verdict, d_totals, stream))

    def denoise_events_dev(self, d_events, n_events, opt, d_out, d_count, d_totals=None, stream=0):
        """ecal_denoise_events_dev: raw device pointers; d_out room for n_events records (not overlapping the events), d_count one
        u32, d_totals FILTER_TOTALS or None; no host synchronisation."""
        L = self._L
        self._check(L.ecal_denoise_events_dev(self._h, d_events, int(n_events), ctypes.byref(opt) if opt is not None else None, d_out, d_count,
                                              d_totals, stream))

    def noise_verdict(self, events, **options):
        """The noise filter's keep / remove byte per event: (verdict: uint8 CUDA tensor [n], 1 keep; totals: one FILTER_TOTALS
        record).  options: width, height, radius, min_support, include_self, dt (noise_options).  Byte for byte what
        noise_verdict_host gives."""
        import torch
        t, n = self._records_arg(events)
        o = noise_options(**options)
        verdict = torch.empty(n, dtype=torch.uint8, device=t.device)
        tot = torch.empty(4, dtype=torch.int64, device=t.device)
        with torch.cuda.device(t.device):
            self.noise_verdict_dev(t.data_ptr() if n else None, n, o, verdict.data_ptr() if n else None, tot.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        return verdict, tot.cpu().numpy().view(FILTER_TOTALS)[0]

    def denoise_events(self, events, **options):
        """The events the noise filter keeps, byte for byte and in input order: (events: uint8 CUDA tensor [n_kept * 25], totals: one
        FILTER_TOTALS record).  options as noise_verdict's.  Off-grid events stay."""
        import torch
        t, n = self._records_arg(events)
        o = noise_options(**options)
        out = torch.empty(n * 25, dtype=torch.uint8, device=t.device)
        cnt = torch.empty(1, dtype=torch.int32, device=t.device)
        tot = torch.empty(4, dtype=torch.int64, device=t.device)
        with torch.cuda.device(t.device):
            self.denoise_events_dev(t.data_ptr() if n else None, n, o, out.data_ptr() if n else None, cnt.data_ptr(), tot.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        kept = int(cnt.item()) & 0xFFFFFFFF
        return out[: kept * 25], tot.cpu().numpy().view(FILTER_TOTALS)[0]

    def remove_noise(self, events, width=346, height=260, **options):
        """ecal_stream_remove_noise's work on a tensor of records: (events, info) — info: the options in force (width, height,
        radius, min_support, include_self, dt) and the filter's totals (n_events, n_off_grid, n_removed, n_kept) as a dict."""
        o = noise_options(width=width, height=height, **options)
        out, tot = self.denoise_events(events, width=width, height=height, **options)
        info = {name: getattr(o, name) for name, _ in NoiseOptions._fields_ if name != "reserved"}
        info.update({k: int(tot[k]) for k in FILTER_TOTALS.names})
        return out, info

    def stream_remove_noise(self, events, width=346, height=260, **options):
        """ecal_stream_remove_noise over an ecal_stream made of the host records `events` (the C++ shim's way) -> (events as a uint8
        CUDA tensor, totals dict)."""
        L = self._L
        vp = ctypes.c_void_p
        ev = np.ascontiguousarray(np.asarray(events, np.uint8).ravel())
        assert ev.size % 25 == 0, "packed 25-byte event records"
        o = noise_options(width=width, height=height, **options)
        tot = np.zeros(1, FILTER_TOTALS)
        h_in, h_out = vp(), vp()
        self._check(L.ecal_stream_create(self._h, _ptr(ev) if ev.size else None, ev.size // 25, ctypes.byref(h_in)))
        try:
            self._check(L.ecal_stream_remove_noise(self._h, h_in, ctypes.byref(o), ctypes.byref(h_out), tot.ctypes.data))
        finally:
            L.ecal_stream_destroy(h_in)
        out, _, _ = self._stream_records(h_out)
        return out, {k: int(tot[0][k]) for k in FILTER_TOTALS.names}

    # ---- undistortion (ecal_undistort_points_dev, ecal_undistort_events_dev, the frames and the stream calls) ----
    def undistort_points_dev(self, cam, d_events, n_events, d_uv, d_flag, stream=0):
        """ecal_undistort_points_dev: raw device pointers; d_uv [n_events][2] f64, d_flag [n_events] u8; no host synchronisation."""
        L = self._L
        self._check(L.ecal_undistort_points_dev(self._h, ctypes.byref(cam), d_events, int(n_events), d_uv, d_flag, stream))

    def undistort_events_dev(self, cam, opt, d_events, n_events, d_out, d_count, d_totals=None, stream=0):
        """ecal_undistort_events_dev: raw device pointers; opt an UndistortOptions or None (SUBPIXEL), d_out room for n_events records
        (not overlapping the events), d_count one u32, d_totals UNDISTORT_TOTALS or None; no host synchronisation."""
        L = self._L
        self._check(L.ecal_undistort_events_dev(self._h, ctypes.byref(cam), ctypes.byref(opt) if opt is not None else None, d_events,
                                                int(n_events), d_out, d_count, d_totals, stream))

    def undistorted_frames_dev(self, cam, opt, d_xy, pk, d_seg_off, d_seg_cnt, S, d_rgb, d_frame_totals=None, stream=0):
        """ecal_undistorted_frames_dev: raw device pointers; pk a PackedPoints or None (doubles), d_rgb [S][out_height][out_width][3]
        u8, d_frame_totals [S] UNDISTORT_FRAME_TOTALS or None; no host synchronisation."""
        L = self._L
        self._check(L.ecal_undistorted_frames_dev(self._h, ctypes.byref(cam), ctypes.byref(opt) if opt is not None else None, d_xy,
                                                  ctypes.byref(pk) if pk is not None else None, d_seg_off, d_seg_cnt, int(S), d_rgb,
                                                  d_frame_totals, stream))

    def undistort_points(self, cam, events):
        """The rule per record of a packed stream: (uv: float64 CUDA tensor [n, 2] with 0, 0 where invalid, flag: uint8 CUDA tensor
        [n], 1 invalid).  RADIAL: bit for bit undistort_points_host."""
        import torch
        t, n = self._records_arg(events)
        uv = torch.empty((n, 2), dtype=torch.float64, device=t.device)
        flag = torch.empty(n, dtype=torch.uint8, device=t.device)
        with torch.cuda.device(t.device):
            self.undistort_points_dev(cam, t.data_ptr() if n else None, n, uv.data_ptr() if n else None, flag.data_ptr() if n else None,
                                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        return uv, flag

    def undistort_events(self, cam, events, opt=None, **options):
        """The stream as the ideal pinhole camera would have seen it: (events: uint8 CUDA tensor [n_kept * 25] — stamps and polarity
        bytes as they were, x and y replaced, the order kept —, totals: one UNDISTORT_TOTALS record).  opt an UndistortOptions, or
        options for undistort_options (mode, out_width, out_height, off_x, off_y, sensor)."""
        import torch
        t, n = self._records_arg(events)
        o = opt if opt is not None else undistort_options(**options)
        out = torch.empty(n * 25, dtype=torch.uint8, device=t.device)
        cnt = torch.empty(1, dtype=torch.int32, device=t.device)
        tot = torch.empty(4, dtype=torch.int64, device=t.device)
        with torch.cuda.device(t.device):
            self.undistort_events_dev(cam, o, t.data_ptr() if n else None, n, out.data_ptr() if n else None, cnt.data_ptr(), tot.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        kept = int(cnt.item()) & 0xFFFFFFFF
        return out[: kept * 25], tot.cpu().numpy().view(UNDISTORT_TOTALS)[0]

    def _host_stream(self, events):
        """an ecal_stream of the host records `events` (the C++ shim's way); the caller destroys it"""
        L = self._L
        vp = ctypes.c_void_p
        ev = np.ascontiguousarray(np.asarray(events, np.uint8).ravel())
        assert ev.size % 25 == 0, "packed 25-byte event records"
        h = vp()
        self._check(L.ecal_stream_create(self._h, _ptr(ev) if ev.size else None, ev.size // 25, ctypes.byref(h)))
        return h

    def undistort_stream(self, cam, events, opt=None, **options):
        """ecal_stream_undistort over an ecal_stream made of the host records `events` -> (events as a uint8 CUDA tensor, totals dict)."""
        L = self._L
        vp = ctypes.c_void_p
        o = opt if opt is not None else undistort_options(**options)
        tot = np.zeros(1, UNDISTORT_TOTALS)
        h_in, h_out = self._host_stream(events), vp()
        try:
            self._check(L.ecal_stream_undistort(self._h, h_in, ctypes.byref(cam), ctypes.byref(o), ctypes.byref(h_out), tot.ctypes.data))
        finally:
            L.ecal_stream_destroy(h_in)
        out, _, _ = self._stream_records(h_out)
        return out, {k: int(tot[0][k]) for k in UNDISTORT_TOTALS.names}

    def undistorted_frames(self, cam, events, t0, t1, opt=None, **options):
        """ecal_stream_undistorted_frames over an ecal_stream made of the host records `events`: EventFrame::undistortedImage for the
        windows [t0[s], t1[s]] -> (rgb uint8 [S, out_height, out_width, 3], totals: UNDISTORT_FRAME_TOTALS [S]).  Options as
        undistort_events'; the mode must be PIXEL (sensor=(width, height): the reference canvas)."""
        L = self._L
        o = opt if opt is not None else undistort_options(**options)
        t0 = np.ascontiguousarray(np.asarray(t0, np.float64).ravel())
        t1 = np.ascontiguousarray(np.asarray(t1, np.float64).ravel())
        S = t0.size
        assert t1.size == S
        ok = undistort_options_error(o) is None and o.mode == UNDISTORT_PIXEL
        rgb = np.zeros((S, int(o.out_height), int(o.out_width), 3) if ok else (S, 1, 1, 3), np.uint8)
        tot = np.zeros(S, UNDISTORT_FRAME_TOTALS)
        h_in = self._host_stream(events)
        try:
            self._check(L.ecal_stream_undistorted_frames(self._h, h_in, ctypes.byref(cam), ctypes.byref(o), _ptr(t0) if S else None,
                                                         _ptr(t1) if S else None, S, _ptr(rgb) if S else None, _ptr(tot) if S else None))
        finally:
            L.ecal_stream_destroy(h_in)
        return rgb, tot

    # ---- image undistortion (ecal_image_plan_*, ecal_undistort_images*, ecal_distort_points_dev) ----
    def image_plan(self, cam, width, height, opt=None, **options):
        """ecal_image_plan_create -> an ImagePlan with .info, .maps(), .table(), .apply(images), .apply_dev(tensor), .close().  opt an
        ImageOptions, or options for image_options (method, channels, out_width, out_height, normalize, off_x, off_y,
        reference_canvas); without a canvas the sensor's own size is taken."""
        import weakref
        if opt is None:
            options.setdefault("sensor", (width, height))
            opt = image_options(**options)
        plan = ImagePlan(self, cam, width, height, opt)
        if not hasattr(self, "_image_plans"):
            self._image_plans = weakref.WeakSet()
        self._image_plans.add(plan)
        return plan

    def distort_points_dev(self, cam, width, height, d_uv, n, d_out, d_flag, stream=0):
        """ecal_distort_points_dev: raw device pointers; d_uv and d_out [n][2] f64, d_flag [n] u8; no host synchronisation."""
        L = self._L
        self._check(L.ecal_distort_points_dev(self._h, ctypes.byref(cam), max(0, int(width)), max(0, int(height)), d_uv, int(n), d_out, d_flag, stream))

    def distort_points(self, cam, width, height, uv):
        """The forward projection on the device: uv [n, 2] of the ideal camera (a host array or a float64 CUDA tensor) -> (out: float64
        CUDA tensor [n, 2] of sensor pixels with 0, 0 where invalid, flag: uint8 CUDA tensor [n]).  RADIAL: bit for bit
        distort_points_host."""
        import torch
        dev = torch.device("cuda", self.device)
        t = uv if isinstance(uv, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(uv, np.float64).reshape(-1, 2)))
        t = t.to(device=dev, dtype=torch.float64).reshape(-1, 2).contiguous()
        n = t.shape[0]
        out = torch.empty((n, 2), dtype=torch.float64, device=dev)
        flag = torch.empty(n, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            self.distort_points_dev(cam, width, height, t.data_ptr() if n else None, n, out.data_ptr() if n else None,
                                    flag.data_ptr() if n else None, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        return out, flag

    def slice_events_dev(self, d_events, n_events, d_win_lo, d_win_hi, d_win_base, S, max_win_events, cap_points,
                         d_xy, d_seg_off, d_seg_cnt, d_event_point, d_overflow, stream=0):
        self._check(self._L.ecal_slice_events_dev(self._h, d_events, int(n_events), d_win_lo, d_win_hi, d_win_base,
                                                  int(S), int(max_win_events), int(cap_points), d_xy, d_seg_off,
                                                  d_seg_cnt, d_event_point, d_overflow, stream))

    # ---- the three stages on packed points (ecal_packed_points) ----
    def slice_events_packed_dev(self, d_events, n_events, d_win_lo, d_win_hi, d_win_base, S, max_win_events, cap_points,
                                d_xy, d_seg_off, d_seg_cnt, d_event_point, d_overflow, pk, stream=0):
        L = self._L
        self._check(L.ecal_slice_events_packed_dev(self._h, d_events, int(n_events), d_win_lo, d_win_hi, d_win_base, int(S),
                                                   int(max_win_events), int(cap_points), d_xy, d_seg_off, d_seg_cnt, d_event_point,
                                                   d_overflow, ctypes.byref(pk) if pk is not None else None, stream))

    def dbscan_batch_packed_dev(self, d_xy, d_seg_off, d_seg_cnt, S, n_points, max_seg_points, eps, minpts, d_labels, d_n_clusters,
                                pk, stream=0):
        L = self._L
        self._check(L.ecal_dbscan_batch_packed_dev(self._h, d_xy, d_seg_off, d_seg_cnt, int(S), int(n_points), int(max_seg_points),
                                                   float(eps), int(minpts), d_labels, d_n_clusters,
                                                   ctypes.byref(pk) if pk is not None else None, stream))

    def extract_batch_packed_dev(self, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters, S, n_points, eps, cluster_min, need_clusters,
                                 radius_threshold, d_win_info, d_cand_pair, d_cand_xyr, d_kept_labels, d_rep, pk, stream=0,
                                 fit_circle=False, knn_num=3):
        """The extraction the context's median-ties setting asks for (exact by default), on packed points."""
        L = self._L
        self._check(L.ecal_extract_batch_packed_dev(self._h, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters, int(S), int(n_points),
                                                    float(eps), int(cluster_min), int(need_clusters), float(radius_threshold),
                                                    int(bool(fit_circle)), int(knn_num), d_win_info, d_cand_pair, d_cand_xyr,
                                                    d_kept_labels, d_rep, ctypes.byref(pk) if pk is not None else None, stream))

    def unpack_points_dev(self, pk, d_seg_off, d_seg_cnt, n_segments, d_xy, stream=0):
        L = self._L
        self._check(L.ecal_unpack_points_dev(self._h, ctypes.byref(pk), d_seg_off, d_seg_cnt, int(n_segments), d_xy, stream))

    def get_median_ties(self):
        return int(self._L.ecal_get_median_ties(self._h))

    # ---- grid ordering ----
    def grid_order_dev(self, d_win_info, d_seg_off, d_cand_xyr, S, rows, cols, d_order, d_found, stream=0):
        self._check(self._L.ecal_grid_order_dev(self._h, d_win_info, d_seg_off, d_cand_xyr, int(S), int(rows), int(cols),
                                                d_order, d_found, stream))

    def grid_order(self, cand_xyr, rows, cols):
        """ecal_grid_order, the host-buffer form for one candidate list: cand_xyr [n, 3] -> (order int32 [rows*cols], found)."""
        cand = np.ascontiguousarray(cand_xyr, np.float64).reshape(-1, 3)
        order = np.full(max(int(rows) * int(cols), 1), -1, np.int32)
        found = np.zeros(1, np.uint32)
        self._check(self._L.ecal_grid_order(self._h, _ptr(cand) if len(cand) else None, len(cand), int(rows), int(cols), _ptr(order), _ptr(found)))
        return order[: int(rows) * int(cols)], int(found[0])

    # ---- re-detection around predicted projections ----
    def rectify_batch_dev(self, d_xy, d_seg_off, d_seg_cnt, d_kept_labels, d_win_info, d_frame_window, d_pose, F,
                          d_landmarks, params, d_feat_xyr, d_feat_valid, d_frame_info, stream=0):
        self._check(self._L.ecal_rectify_batch_dev(self._h, d_xy, d_seg_off, d_seg_cnt, d_kept_labels, d_win_info,
                                                   d_frame_window, d_pose, int(F), d_landmarks, ctypes.byref(params),
                                                   d_feat_xyr, d_feat_valid, d_frame_info, stream))

    def rectify_batch(self, xy, seg_off, seg_cnt, kept_labels, pose, landmarks, params):
        """ecal_rectify_batch, the host-buffer form: keyframe f owns segments 2f and 2f + 1 of xy [n_points, 2] / kept_labels.
        Returns (feat_xyr [F, n, 3], feat_valid [F, n] u32, frame_info [F, 2] u32); no points at all go down as NULL arrays."""
        L = self._L
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        kept = np.ascontiguousarray(kept_labels, np.int32)
        off, cnt = np.ascontiguousarray(seg_off, np.uint32), np.ascontiguousarray(seg_cnt, np.uint32)
        pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 12)
        lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3)
        F, n = pose.shape[0], int(params.rows) * int(params.cols)
        assert len(off) == 2 * F and len(cnt) == 2 * F and len(kept) == len(xy)
        feat = np.zeros((F, n, 3))
        valid, info = np.zeros((F, n), np.uint32), np.zeros((F, 2), np.uint32)
        self._check(L.ecal_rectify_batch(self._h, _ptr(xy) if len(xy) else None, _ptr(off), _ptr(cnt), _ptr(kept) if len(xy) else None,
                                         len(xy), _ptr(pose), F, _ptr(lm), ctypes.byref(params), _ptr(feat), _ptr(valid), _ptr(info)))
        return feat, valid, info

    # ---- event -> residual association ----
    def associate_dev(self, d_events, n_events, d_kf_time, d_kf_circles, n_keyframes, n_circles, t_min, t_max,
                      max_dt, edge_tol, d_obs, d_time, d_lm_id, d_count, stream=0):
        self._check(self._L.ecal_associate_dev(self._h, d_events, int(n_events), d_kf_time, d_kf_circles,
                                               int(n_keyframes), int(n_circles), float(t_min), float(t_max),
                                               float(max_dt), float(edge_tol), d_obs, d_time, d_lm_id, d_count, stream))

    def associate_ranges_dev(self, d_events, n_events, d_kf_time, d_kf_circles, n_keyframes, n_circles, d_ranges, n_ranges,
                             max_dt, edge_tol, d_obs, d_time, d_lm_id, d_seg_id, d_count, stream=0):
        """ecal_associate_ranges_dev: all spline segments in one pass; the count stays on the device."""
        self._check(self._L.ecal_associate_ranges_dev(self._h, d_events, int(n_events), d_kf_time, d_kf_circles, int(n_keyframes),
                                                      int(n_circles), d_ranges, int(n_ranges), float(max_dt), float(edge_tol),
                                                      d_obs, d_time, d_lm_id, d_seg_id, d_count, stream))

    # ---- circle-candidate extraction ----
    def circle_radius_threshold(self, width, height, rows, cols, asymmetric, square_size, circle_radius):
        return self._L.ecal_circle_radius_threshold(float(width), float(height), int(rows), int(cols),
                                                    int(bool(asymmetric)), float(square_size), float(circle_radius))

    def extract_batch_dev(self, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters, S, n_points, cluster_min,
                          need_clusters, radius_threshold, d_win_info, d_cand_pair, d_cand_xyr, d_kept_labels, d_rep,
                          stream=0, fit_circle=False, knn_num=3):
        self._check(self._L.ecal_extract_batch_dev(self._h, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters,
                                                   int(S), int(n_points), int(cluster_min), int(need_clusters),
                                                   float(radius_threshold), int(bool(fit_circle)), int(knn_num),
                                                   d_win_info, d_cand_pair, d_cand_xyr, d_kept_labels, d_rep, stream))

    def extract_batch_ordered_dev(self, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters, d_cluster_order, S, n_points, cluster_min,
                                  need_clusters, radius_threshold, d_win_info, d_cand_pair, d_cand_xyr, d_kept_labels, d_rep,
                                  stream=0, fit_circle=False, knn_num=3):
        """extract_batch_dev with the reference's own pick at tied medians (d_cluster_order from cluster_order_dev)."""
        L = self._L
        self._check(L.ecal_extract_batch_ordered_dev(self._h, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters, d_cluster_order, int(S),
                                                     int(n_points), int(cluster_min), int(need_clusters), float(radius_threshold),
                                                     int(bool(fit_circle)), int(knn_num), d_win_info, d_cand_pair, d_cand_xyr,
                                                     d_kept_labels, d_rep, stream))

    def extract_batch_exact_dev(self, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters, S, n_points, eps, cluster_min, need_clusters,
                                radius_threshold, d_win_info, d_cand_pair, d_cand_xyr, d_kept_labels, d_rep, stream=0, fit_circle=False,
                                knn_num=3):
        """The exact extraction in one call: plain pass + member order of the tied clusters + re-extraction of their windows."""
        L = self._L
        self._check(L.ecal_extract_batch_exact_dev(self._h, d_xy, d_seg_off, d_seg_cnt, d_labels, d_n_clusters, int(S), int(n_points),
                                                   float(eps), int(cluster_min), int(need_clusters), float(radius_threshold),
                                                   int(bool(fit_circle)), int(knn_num), d_win_info, d_cand_pair, d_cand_xyr,
                                                   d_kept_labels, d_rep, stream))

    def cluster_order_dev(self, d_xy, d_seg_off, d_seg_cnt, S, eps, d_labels, d_n_clusters, d_order, d_status, stream=0,
                          only_tied_medians=False):
        """Position of every core point inside the reference's Clusters[label] (expandCluster's pop order); -1 for noise.
        only_tied_medians: False / True, or 2 = only the clusters the caller marked with -3 in d_order (ecal.h)."""
        L = self._L
        self._check(L.ecal_cluster_order_dev(self._h, d_xy, d_seg_off, d_seg_cnt, int(S), float(eps), d_labels, d_n_clusters, d_order,
                                             d_status, int(only_tied_medians), stream))

    def cluster_order(self, xy, slice_off, eps, labels, n_clusters):
        """Host-buffer form of cluster_order_dev: returns (order [N] int32, status [S] uint32)."""
        L = self._L
        xy = np.ascontiguousarray(xy, np.float64)
        slice_off = np.ascontiguousarray(slice_off, np.uint32)
        labels = np.ascontiguousarray(labels, np.int32)
        n_clusters = np.ascontiguousarray(n_clusters, np.uint32)
        S = len(slice_off) - 1
        order = np.full(max(len(labels), 1), -9, np.int32)
        status = np.full(max(S, 1), 9, np.uint32)
        self._check(L.ecal_cluster_order(self._h, _ptr(xy), _ptr(slice_off), S, float(eps), _ptr(labels), _ptr(n_clusters), _ptr(order),
                                         _ptr(status)))
        return order[:len(labels)], status[:S]

    def detect_fused_dev(self, d_events, n_events, d_win_lo, d_win_hi, d_win_base, S, max_win_events, max_seg_points, cap_points,
                         eps, minpts, cluster_min, need_clusters, radius_threshold, d_xy, d_seg_off, d_seg_cnt, d_event_point,
                         d_overflow, d_labels, d_n_clusters, d_win_info, d_cand_pair, d_cand_xyr, d_kept_labels, d_rep, stream=0,
                         fit_circle=False, knn_num=3):
        """slice + DBSCAN + extraction of every window in one call (one kernel in the shipped configuration)."""
        self._check(self._L.ecal_detect_fused_dev(self._h, d_events, int(n_events), d_win_lo, d_win_hi, d_win_base, int(S),
                                                  int(max_win_events), int(max_seg_points), int(cap_points), float(eps),
                                                  int(minpts), int(cluster_min), int(need_clusters), float(radius_threshold),
                                                  int(bool(fit_circle)), int(knn_num), d_xy, d_seg_off, d_seg_cnt, d_event_point,
                                                  d_overflow, d_labels, d_n_clusters, d_win_info, d_cand_pair, d_cand_xyr,
                                                  d_kept_labels, d_rep, stream))


# ---- continuous-time calibration solve ----


def time_shard_cuts(knots, n_cp, world_size):
    """ecal_solver_time_shard_cuts: the world_size - 1 cut times of a spline's time shards (LmOptions.distributed = 2)."""
    L = load_library()
    kn = np.ascontiguousarray(knots, np.float64)
    out = np.zeros(max(world_size - 1, 1))
    rc = L.ecal_solver_time_shard_cuts(kn.ctypes.data, int(n_cp), int(world_size), out.ctypes.data)
    if rc:
        raise EcalError(rc, "ecal_solver_time_shard_cuts")
    return out[:world_size - 1]


def pose_gates(Rsw, twb, time, pnp_ok, rect_ok, motion_time_step):
    """ecal_pose_gates: the sequential keyframe gates of EventCalibIni::cvCalibration (EventCalibIni.cpp:281-302) on per-frame
    results known for all frames.  Returns (accepted indices int64, discarded by checkPose, discarded by rectify)."""
    L = load_library()
    u8p, u32p, f64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    R = np.ascontiguousarray(Rsw, np.float64).reshape(-1, 9)
    K = R.shape[0]
    tw = np.ascontiguousarray(twb, np.float64).reshape(K, 3)
    tt = np.ascontiguousarray(time, np.float64).reshape(K)
    a = np.ascontiguousarray(pnp_ok, np.uint8).reshape(K)
    b = np.ascontiguousarray(rect_ok, np.uint8).reshape(K)
    acc = np.zeros(max(K, 1), np.uint32)
    n = (ctypes.c_uint32 * 3)()
    rc = L.ecal_pose_gates(K, R.ctypes.data_as(f64p), tw.ctypes.data_as(f64p), tt.ctypes.data_as(f64p), a.ctypes.data_as(u8p),
                           b.ctypes.data_as(u8p), float(motion_time_step), acc.ctypes.data_as(u32p),
                           ctypes.cast(ctypes.byref(n, 0), u32p), ctypes.cast(ctypes.byref(n, 4), u32p), ctypes.cast(ctypes.byref(n, 8), u32p))
    if rc:
        raise EcalError(rc, "ecal_pose_gates: invalid arguments")
    return acc[:n[0]].astype(np.int64), int(n[1]), int(n[2])


def inverse_radial_distortion(k4):
    L = load_library()
    k = np.ascontiguousarray(k4, np.float64)
    b = np.zeros(5)
    L.ecal_inverse_radial_distortion(_ptr(k), _ptr(b))
    return b


def _set_members(o, options, what):
    """the options struct o with its members set from keyword arguments; a name it does not have is a TypeError"""
    for k, v in options.items():
        if not hasattr(o, k):
            raise TypeError("no %s option %r" % (what, k))
        setattr(o, k, v)
    return o


class Solver:
    """ecal_solver: residual records + spline layout resident on the GPU.

    problem: dict with seg_cp_off [G+1] u32, knots f64, obs [M,2], time [M], lm_id [M] u32,
    seg_id [M] u32 or None, landmarks [L,3], circle_radius, huber_a, use_so3 / fisheye (optional, default False).
    Parameter vector layout: [intr 9 | q n_cp x 4 (xyzw) | t n_cp x 3]."""

    def __init__(self, ctx: Context, problem, device_arrays=None, stream=0):
        """device_arrays = (d_obs, d_time, d_lm_id, d_seg_id or None, capacity, d_count or None): raw DEVICE pointers of the
        residual arrays (ecal_associate_ranges_dev's outputs) — ecal_solver_create_dev builds the problem in place; the
        dict then carries only seg_cp_off, knots, landmarks and the scalars."""
        self.ctx = ctx
        L = ctx._L
        keep = {}

        def arr(name, dt):
            a = np.ascontiguousarray(problem[name], dtype=dt)
            keep[name] = a
            return ctypes.c_void_p(a.ctypes.data)

        P = _SplineProblem()
        P.seg_cp_off = arr("seg_cp_off", np.uint32)
        P.n_segments = keep["seg_cp_off"].shape[0] - 1
        P.knots = arr("knots", np.float64)
        if device_arrays is None:
            P.obs = arr("obs", np.float64)
            P.time = arr("time", np.float64)
            P.lm_id = arr("lm_id", np.uint32)
            P.n_res = keep["time"].shape[0]
            P.seg_id = arr("seg_id", np.uint32) if problem.get("seg_id") is not None else None
        else:
            d_obs, d_time, d_lm, d_seg, cap, d_count = device_arrays
            P.obs, P.time, P.lm_id, P.seg_id, P.n_res = d_obs, d_time, d_lm, d_seg, int(cap)
        P.landmarks = arr("landmarks", np.float64)
        P.n_landmarks = keep["landmarks"].reshape(-1, 3).shape[0]
        P.circle_radius = float(problem["circle_radius"])
        P.huber_a = float(problem["huber_a"])
        self.huber_a = P.huber_a
        P.use_so3 = int(bool(problem.get("use_so3", False)))
        P.camera_model = CAMERA_FISHEYE if problem.get("fisheye", False) else CAMERA_RADIAL
        # the problem without its residual arrays: what Solver.reassociated builds the next solver from
        self._layout = dict(seg_cp_off=keep["seg_cp_off"], knots=keep["knots"], landmarks=keep["landmarks"], circle_radius=P.circle_radius,
                            huber_a=P.huber_a, use_so3=bool(P.use_so3), fisheye=P.camera_model == CAMERA_FISHEYE)
        h = ctypes.c_void_p()
        if device_arrays is None:
            ctx._check(L.ecal_solver_create(ctx._h, ctypes.byref(P), ctypes.byref(h)))
        else:
            ctx._check(L.ecal_solver_create_dev(ctx._h, ctypes.byref(P), device_arrays[5], stream, ctypes.byref(h)))
        self._adopt(h)

    def _adopt(self, h):
        """take over the ecal_solver handle h (the constructor; Solver.reassociated)"""
        L = self.ctx._L
        self._h = h
        self.n_params = int(L.ecal_solver_param_size(h))
        self.n_normal = int(L.ecal_solver_normal_size(h))
        self.n_cp = (self.n_params - 9) // 7
        self.n_chunks = int(L.ecal_solver_num_chunks(h))
        self.n_res = int(L.ecal_solver_num_residuals(h))
        self.n_landmarks = int(L.ecal_solver_num_landmarks(h))

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._L.ecal_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, params, with_jacobian=True):
        p = np.ascontiguousarray(params, np.float64)
        assert p.shape[0] == self.n_params
        acc = np.zeros(self.n_normal if with_jacobian else 1)
        self.ctx._check(self.ctx._L.ecal_solver_evaluate(self._h, _ptr(p), int(with_jacobian), _ptr(acc)))
        return acc

    def residuals(self, params, with_jacobian=True):
        """ecal_residuals: (r [n_res], J [n_res, 33] or None, cp0 [n_res]) — the per-residual CostFunction::Evaluate seam."""
        p = np.ascontiguousarray(params, np.float64)
        assert p.shape[0] == self.n_params
        L = self.ctx._L
        n = int(self.n_res)
        r = np.zeros(max(n, 1))
        J = np.zeros((max(n, 1), 33)) if with_jacobian else None
        c = np.zeros(max(n, 1), np.uint32)
        self.ctx._check(L.ecal_residuals(self._h, _ptr(p), _ptr(r), _ptr(J) if with_jacobian else None, _ptr(c)))
        return r[:n], (J[:n] if with_jacobian else None), c[:n]

    def evaluate_dev(self, d_params, with_jacobian, d_accum, stream=0):
        self.ctx._check(self.ctx._L.ecal_solver_evaluate_dev(self._h, d_params, int(with_jacobian), d_accum, stream))

    def report_options(self, **options):
        """ecal_report_default_options with the given members (width, height, cell_px, hist_bins, hist_range, outlier_thresh) set."""
        o = ReportOptions()
        self.ctx._L.ecal_report_default_options(ctypes.byref(o))
        return _set_members(o, options, "report")

    def report_dev(self, d_params, d_kf_time, n_keyframes, options, d_total, d_kf=None, d_lm=None, d_cell_n=None, d_cell_sum_r2=None,
                   d_hist=None, stream=0):
        """ecal_solver_report_dev: raw device pointers (None: that family is skipped), records laid out as BIN_STATS /
        REPORT_TOTALS; no host synchronisation."""
        self._report_dev("ecal_solver_report_dev", d_params, d_kf_time, n_keyframes, options, d_total, d_kf, d_lm, d_cell_n, d_cell_sum_r2,
                         d_hist, stream)

    def _report_dev(self, symbol, d_params, d_kf_time, n_keyframes, options, *outputs_and_stream):
        """report_dev and report_px_dev: the two calls take the same arguments"""
        self.ctx._check(getattr(self.ctx._L, symbol)(self._h, d_params, d_kf_time, int(n_keyframes),
                                                     ctypes.byref(options) if options is not None else None, *outputs_and_stream))

    def _report(self, totals_dtype, symbol, options_factory, default_range, params, kf_time, families, options):
        """report and report_px: the families' arrays, the call, the derived figures -> the dict without the keys that only one of the two
        has.  default_range: the histogram's half width where hist_range is not positive."""
        p = np.ascontiguousarray(params, np.float64)
        assert p.shape[0] == self.n_params
        o = options_factory(**options)
        want = set(families)
        if kf_time is None:
            want.discard("kf")
        kt = np.ascontiguousarray(kf_time, np.float64) if "kf" in want else None
        total = np.zeros(1, totals_dtype)
        kf = np.zeros(kt.shape[0], BIN_STATS) if "kf" in want else None
        lm = np.zeros(self.n_landmarks, BIN_STATS) if "lm" in want else None
        cn = cs = hist = None
        if "cells" in want and o.cell_px:
            cy, cx = -(-o.height // o.cell_px), -(-o.width // o.cell_px)
            cn, cs = np.zeros((cy, cx), np.uint64), np.zeros((cy, cx))
        elif "cells" in want:
            cn, cs = np.zeros((1, 1), np.uint64), np.zeros((1, 1))    # (the call refuses cell_px == 0)
        if "hist" in want:
            hist = np.zeros(max(int(o.hist_bins), 1), np.uint64)

        def ptr(a):
            return _ptr(a) if a is not None else None
        self.ctx._check(getattr(self.ctx._L, symbol)(self._h, _ptr(p), ptr(kt), 0 if kt is None else kt.shape[0], ctypes.byref(o),
                                                     _ptr(total), ptr(kf), ptr(lm), ptr(cn), ptr(cs), ptr(hist)))

        def derived(out, name, b):
            n = b["n"].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[name + "rms"] = np.sqrt(b["sum_r2"] / n)
                out[name + "mean"] = b["sum_r"] / n
                out[name + "outlier_frac"] = b["n_out"] / n
        out = {"totals": total[0], "options": o}
        derived(out, "", total["all"][0])
        if kf is not None:
            out["kf"] = kf
            derived(out, "kf_", kf)
        if lm is not None:
            out["lm"] = lm
            derived(out, "lm_", lm)
        if cn is not None:
            out["cell_n"], out["cell_sum_r2"] = cn, cs
            out["empty_cell_frac"] = float((cn == 0).mean())
        if hist is not None:
            out["hist"] = hist
            rng = o.hist_range if o.hist_range > 0 else default_range
            out["hist_edges"] = np.linspace(-rng, rng, hist.shape[0] + 1)
        return out

    def report(self, params, kf_time=None, families=("kf", "lm", "cells", "hist"), **options):
        """ecal_solver_report: the raw residuals at `params` binned on the GPU, in board units (the unit of circle_radius).
        kf_time: ascending keyframe times (all segments); options: ReportOptions members.  Returns a dict: `totals` (one
        REPORT_TOTALS record), `kf` [K] / `lm` [n_landmarks] (BIN_STATS), `cell_n` / `cell_sum_r2` [cells_y, cells_x], `hist`
        [hist_bins] with `hist_edges`, and per family `<family>_rms`, `_mean`, `_outlier_frac` (NaN where a bin is empty);
        `rms`, `mean`, `outlier_frac` of the totals, `cost` (= evaluate(params, False)[0]) and `empty_cell_frac`."""
        out = self._report(REPORT_TOTALS, "ecal_solver_report", self.report_options, 4.0 * self.huber_a, params, kf_time, families, options)
        out["cost"] = float(out["totals"]["cost"])
        return out

    def residuals_px(self, params, with_gradient=False):
        """ecal_residuals_px: the residuals in PIXELS, per record the first-order (Sampson) distance r / |d r / d (u, v)| from the
        event to the projected rim (include/ecal.h, "report in pixels").  Returns (r_px [n_res], 0.0 where the record is
        degenerate; grad [n_res, 2] = (d r / d u, d r / d v) or None; flag [n_res] uint8, 1 = degenerate)."""
        p = np.ascontiguousarray(params, np.float64)
        assert p.shape[0] == self.n_params
        n = int(self.n_res)
        r = np.zeros(max(n, 1))
        g = np.zeros((max(n, 1), 2)) if with_gradient else None
        f = np.zeros(max(n, 1), np.uint8)
        self.ctx._check(self.ctx._L.ecal_residuals_px(self._h, _ptr(p), _ptr(r), _ptr(g) if with_gradient else None, _ptr(f)))
        return r[:n], (g[:n] if with_gradient else None), f[:n]

    def report_px_options(self, **options):
        """ecal_report_px_default_options (346 x 260, 16 px cells, 64 bins, hist_range 4 px, outlier_thresh 1 px) with the given
        ReportOptions members set."""
        o = ReportOptions()
        self.ctx._L.ecal_report_px_default_options(ctypes.byref(o))
        return _set_members(o, options, "report")

    def report_px_dev(self, d_params, d_kf_time, n_keyframes, options, d_total, d_kf=None, d_lm=None, d_cell_n=None, d_cell_sum_r2=None,
                      d_hist=None, stream=0):
        """ecal_solver_report_px_dev: raw device pointers (None: that family is skipped), records laid out as BIN_STATS /
        REPORT_PX_TOTALS; no host synchronisation."""
        self._report_dev("ecal_solver_report_px_dev", d_params, d_kf_time, n_keyframes, options, d_total, d_kf, d_lm, d_cell_n, d_cell_sum_r2,
                         d_hist, stream)

    def report_px(self, params, kf_time=None, families=("kf", "lm", "cells", "hist"), **options):
        """ecal_solver_report_px: the residuals at `params` in PIXELS (residuals_px above) binned on the GPU.  Arguments and the
        returned dict as report's — `totals` is one REPORT_PX_TOTALS record and there is no `cost` — plus `n_degenerate` (records
        without a distance: in no bin), `px_per_unit` (the mean of 1 / |d r / d (u, v)|: how many pixels a board unit is in this
        data; NaN without records) and `rms_px` (= `rms`)."""
        out = self._report(REPORT_PX_TOTALS, "ecal_solver_report_px", self.report_px_options, 4.0, params, kf_time, families, options)
        total = out["totals"]
        out["n_degenerate"] = int(total["n_degenerate"])
        out["rms_px"] = out["rms"]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["px_per_unit"] = float(total["sum_px_per_unit"] / np.float64(total["all"]["n"]))
        return out

    def board_image_options(self, **options):
        """ecal_board_image_default_options (the landmarks' bounding box padded by 3 radii, bin = radius / 8, 64 ring bins over
        +- radius) with the given members (x0, y0, bin, width, height, ring_bins, ring_range) set."""
        o = BoardImageOptions()
        self.ctx._check(self.ctx._L.ecal_board_image_default_options(self._h, ctypes.byref(o)))
        return _set_members(o, options, "board image")

    def _events_arg(self, events):
        """events of the board-image calls -> (device pointer, count, object to keep alive): an EventStream-like object with an
        ecal_stream handle is not taken here; a torch uint8 tensor on the GPU (packed 25-byte records, time-sorted) or a host
        array / bytes of such records, which is uploaded."""
        import torch
        if isinstance(events, torch.Tensor):
            t = events if events.is_cuda else events.cuda()
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.frombuffer(events, np.uint8) if isinstance(events, (bytes, bytearray))
                                                      else np.asarray(events, np.uint8).ravel())).cuda()
        t = t.contiguous().view(torch.uint8).reshape(-1)
        assert t.numel() % 25 == 0, "packed 25-byte event records"
        return t.data_ptr() if t.numel() else None, t.numel() // 25, t

    def board_image_dev(self, d_params, d_events, n_events, options, d_img, d_totals, d_ring_stats=None, d_ring_hist=None, stream=0):
        """ecal_solver_board_image_dev: raw device pointers (None: that output is skipped), records laid out as
        BOARD_IMAGE_TOTALS / RING_STATS; no host synchronisation."""
        self.ctx._check(self.ctx._L.ecal_solver_board_image_dev(self._h, d_params, d_events, int(n_events),
                                                                ctypes.byref(options) if options is not None else None, d_img, d_totals,
                                                                d_ring_stats, d_ring_hist, stream))

    def board_points_dev(self, d_params, d_events, n_events, d_xw, d_flag, stream=0):
        """ecal_solver_board_points_dev: d_xw [n, 2] f64, d_flag [n] u8 (0 ok, 1 outside time, 2 behind)."""
        self.ctx._check(self.ctx._L.ecal_solver_board_points_dev(self._h, d_params, d_events, int(n_events), d_xw, d_flag, stream))

    def board_points(self, x, events):
        """The board point of every event at the parameters x: (xw [n, 2] float64, flag [n] uint8: 0 ok, 1 outside every
        segment's time range, 2 behind the camera; xw is zero where the flag is not 0)."""
        import torch
        p = torch.as_tensor(np.ascontiguousarray(x, np.float64), device="cuda")
        assert p.shape[0] == self.n_params
        d_ev, n, keep = self._events_arg(events)
        xw = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        flag = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.board_points_dev(p.data_ptr(), d_ev, n, xw.data_ptr(), flag.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        del keep
        return xw.cpu().numpy(), flag.cpu().numpy()

    def board_image(self, x, events, outputs=("image", "ring_stats", "ring_hist"), **options):
        """ecal_solver_board_image_dev: every event of the packed, time-sorted stream `events` carried through the intrinsics
        and the spline pose of the parameters x onto the board plane (board units, the unit of circle_radius).  Returns a dict:
        `image` [2, H, W] uint32 (0: negative, 1: positive events), `totals` (one BOARD_IMAGE_TOTALS record), `ring_stats`
        [n_landmarks, 2] (RING_STATS per landmark and polarity), `ring_n` / `ring_mean` / `ring_std` [n_landmarks] of d = |Xw -
        lm| - radius over both polarities (NaN where a circle drew no event), `ring_hist` [n_landmarks, ring_bins] with
        `ring_edges`, `options` and `extent` = (x0, x0 + W bin, y0, y0 + H bin), the image's frame in board units."""
        import torch
        p = torch.as_tensor(np.ascontiguousarray(x, np.float64), device="cuda")
        assert p.shape[0] == self.n_params
        o = self.board_image_options(**options)
        d_ev, n, keep = self._events_arg(events)
        H, W, B, L = int(o.height), int(o.width), int(o.ring_bins), self.n_landmarks
        want = set(outputs)
        # (sizes that the call itself refuses must not be allocated first)
        big = H * W > (1 << 24) or B > 256
        img = torch.zeros((2, H, W), dtype=torch.int32, device="cuda") if "image" in want and not big else None
        tot = torch.zeros(7, dtype=torch.int64, device="cuda")
        rs = torch.zeros((L, 2, 3), dtype=torch.float64, device="cuda") if "ring_stats" in want and B else None
        rh = torch.zeros((L, max(B, 1)), dtype=torch.int64, device="cuda") if "ring_hist" in want and B and not big else None

        def ptr(t):
            return t.data_ptr() if t is not None else None
        self.board_image_dev(p.data_ptr(), d_ev, n, o, ptr(img), tot.data_ptr(), ptr(rs), ptr(rh), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        del keep
        out = {"totals": tot.cpu().numpy().view(BOARD_IMAGE_TOTALS)[0], "options": o,
               "extent": (o.x0, o.x0 + W * o.bin, o.y0, o.y0 + H * o.bin)}
        if img is not None:
            out["image"] = img.cpu().numpy().view(np.uint32)
        if rs is not None:
            st = rs.cpu().numpy().reshape(L, 2 * 3).view(RING_STATS).reshape(L, 2)
            out["ring_stats"] = st
            nn = st["n"].sum(axis=1).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                mean = st["sum_d"].sum(axis=1) / nn
                out["ring_n"], out["ring_mean"] = st["n"].sum(axis=1), mean
                out["ring_std"] = np.sqrt(np.maximum(st["sum_d2"].sum(axis=1) / nn - mean * mean, 0.0))
        if rh is not None:
            out["ring_hist"] = rh.cpu().numpy().view(np.uint64)
            out["ring_edges"] = np.linspace(-o.ring_range, o.ring_range, B + 1)
        return out

    def _with_stream(self, events, call):
        """call(ecal_stream handle) on an ecal_stream made of the host records `events` (any order: the stream sorts)"""
        L = self.ctx._L
        ev = np.ascontiguousarray(np.asarray(events, np.uint8).ravel())
        assert ev.size % 25 == 0, "packed 25-byte event records"
        h = ctypes.c_void_p()
        self.ctx._check(L.ecal_stream_create(self.ctx._h, _ptr(ev) if ev.size else None, ev.size // 25, ctypes.byref(h)))
        try:
            return call(h, ev.size // 25)
        finally:
            L.ecal_stream_destroy(h)

    def board_image_host(self, x, events, outputs=("image", "ring_stats", "ring_hist"), **options):
        """ecal_solver_board_image, the host-buffer form over an ecal_stream made of the host records `events`: (image [2, H, W]
        or None, totals record, ring_stats [n_landmarks, 2] or None, ring_hist [n_landmarks, ring_bins] or None)."""
        p = np.ascontiguousarray(x, np.float64)
        assert p.shape[0] == self.n_params
        o = self.board_image_options(**options)
        H, W, B, L = int(o.height), int(o.width), int(o.ring_bins), self.n_landmarks
        ok = H * W <= (1 << 24) and B <= 256
        img = np.zeros((2, H, W), np.uint32) if "image" in outputs and ok else None
        tot = np.zeros(1, BOARD_IMAGE_TOTALS)
        rs = np.zeros((L, 2), RING_STATS) if "ring_stats" in outputs and B else None
        rh = np.zeros((L, B), np.uint64) if "ring_hist" in outputs and B and ok else None

        def ptr(a):
            return _ptr(a) if a is not None and a.size else None
        self._with_stream(events, lambda h, n: self.ctx._check(self.ctx._L.ecal_solver_board_image(
            self._h, _ptr(p), h, ctypes.byref(o), ptr(img), _ptr(tot), ptr(rs), ptr(rh))))
        return img, tot[0], rs, rh

    def board_points_host(self, x, events):
        """ecal_solver_board_points, the host-buffer form: (xw [n, 2], flag [n])."""
        p = np.ascontiguousarray(x, np.float64)
        assert p.shape[0] == self.n_params
        n = np.asarray(events, np.uint8).size // 25
        xw, flag = np.zeros((n, 2)), np.zeros(n, np.uint8)
        self._with_stream(events, lambda h, m: self.ctx._check(self.ctx._L.ecal_solver_board_points(
            self._h, _ptr(p), h, _ptr(xw) if n else None, _ptr(flag) if n else None)))
        return xw, flag

    # ---- re-association through the solved spline (ecal_solver_reassociate*) ----
    def reassociate_dev(self, d_params, d_events, n_events, ring_tol, d_obs, d_time, d_lm_id, d_seg_id, d_count, d_totals=None, stream=0):
        """ecal_solver_reassociate_dev: raw device pointers; the record arrays need room for n_events entries, d_count is one
        uint32, d_totals (or None) one REASSOCIATE_TOTALS record; ring_tol None or <= 0: the solver's huber_a.  No host
        synchronisation."""
        self.ctx._check(self.ctx._L.ecal_solver_reassociate_dev(self._h, d_params, d_events, int(n_events),
                                                                0.0 if ring_tol is None else float(ring_tol), d_obs, d_time, d_lm_id,
                                                                d_seg_id, d_count, d_totals, stream))

    def reassociate(self, x, events, ring_tol=None):
        """Every event of the packed, time-sorted stream `events` whose board point at the parameters x lies within ring_tol
        (board units; None: the solver's huber_a) of a circle's rim, as residual records in event order.  Returns a dict: `obs`
        [m, 2], `time` [m], `lm_id` [m], `seg_id` [m], `count` = m and `totals` (one REASSOCIATE_TOTALS record: n_events =
        n_outside_time + n_behind + n_off_ring + n_kept, n_kept = m)."""
        import torch
        p = torch.as_tensor(np.ascontiguousarray(x, np.float64), device="cuda")
        assert p.shape[0] == self.n_params
        d_ev, n, keep = self._events_arg(events)
        obs = torch.empty((max(n, 1), 2), dtype=torch.float64, device="cuda")
        tm = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
        lm = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        sg = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        tot = torch.zeros(5, dtype=torch.int64, device="cuda")
        self.reassociate_dev(p.data_ptr(), d_ev, n, ring_tol, obs.data_ptr(), tm.data_ptr(), lm.data_ptr(), sg.data_ptr(), cnt.data_ptr(),
                             tot.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        del keep
        m = int(cnt.cpu().numpy().view(np.uint32)[0])
        return {"obs": obs[:m].cpu().numpy(), "time": tm[:m].cpu().numpy(), "lm_id": lm[:m].cpu().numpy().view(np.uint32),
                "seg_id": sg[:m].cpu().numpy().view(np.uint32), "count": m, "totals": tot.cpu().numpy().view(REASSOCIATE_TOTALS)[0]}

    def reassociate_host(self, x, events, capacity, ring_tol=None, buffers=None):
        """ecal_solver_reassociate, the host-buffer form over an ecal_stream made of the host records `events`: (obs, time, lm_id,
        seg_id, count, totals record); the arrays (or `buffers`, four arrays of at least `capacity` records) are written up to
        `count` — and not at all when count > capacity (EcalError, ECAL_ERR_RANGE)."""
        p = np.ascontiguousarray(x, np.float64)
        assert p.shape[0] == self.n_params
        c = max(int(capacity), 1)
        obs, tm, lm, sg = buffers if buffers is not None else (np.zeros((c, 2)), np.zeros(c), np.zeros(c, np.uint32), np.zeros(c, np.uint32))
        cnt = ctypes.c_uint64(0)
        tot = np.zeros(1, REASSOCIATE_TOTALS)
        self._with_stream(events, lambda h, n: self.ctx._check(self.ctx._L.ecal_solver_reassociate(
            self._h, _ptr(p), h, 0.0 if ring_tol is None else float(ring_tol), int(capacity), _ptr(obs), _ptr(tm), _ptr(lm), _ptr(sg),
            ctypes.byref(cnt), _ptr(tot))))
        m = int(cnt.value)
        return obs[:m], tm[:m], lm[:m], sg[:m], m, tot[0]

    def reassociated(self, x, events, ring_tol=None, stream=None):
        """A NEW Solver with this one's layout (segments, knots, landmarks, radius, Huber width, rotation variant, camera model)
        on the records of reassociate(x, events, ring_tol), built in place on the GPU: nothing proportional to the events crosses
        PCIe.  events: a torch uint8 CUDA tensor (ecal_solver_reassociate_dev into device arrays, ecal_solver_create_dev on
        them — the chain's way, calibrate_stream), or host records / bytes (uploaded into an ecal_stream, then
        ecal_solver_create_reassociated, the C++ shim's way).  Returns (solver, totals record); this solver is left untouched and
        both are closed independently."""
        import torch
        p = np.ascontiguousarray(x, np.float64)
        assert p.shape[0] == self.n_params
        if not (isinstance(events, torch.Tensor) and events.is_cuda):
            tot = np.zeros(1, REASSOCIATE_TOTALS)
            h = ctypes.c_void_p()
            ev = events.numpy() if isinstance(events, torch.Tensor) else (
                np.frombuffer(events, np.uint8) if isinstance(events, (bytes, bytearray)) else events)
            self._with_stream(ev, lambda es, n: self.ctx._check(self.ctx._L.ecal_solver_create_reassociated(
                self._h, _ptr(p), es, 0.0 if ring_tol is None else float(ring_tol), ctypes.byref(h), _ptr(tot))))
            new = Solver.__new__(Solver)
            new.ctx, new.huber_a, new._layout = self.ctx, self.huber_a, self._layout
            new._adopt(h)
            return new, tot[0]
        dev = events.device
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        d_p = torch.as_tensor(p, device=dev)
        d_ev, n, keep = self._events_arg(events)
        obs = torch.empty((max(n, 1), 2), dtype=torch.float64, device=dev)
        tm = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        lm = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        sg = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        tot = torch.zeros(5, dtype=torch.int64, device=dev)
        self.reassociate_dev(d_p.data_ptr(), d_ev, n, ring_tol, obs.data_ptr(), tm.data_ptr(), lm.data_ptr(), sg.data_ptr(), cnt.data_ptr(),
                             tot.data_ptr(), st)
        new = Solver(self.ctx, self._layout, device_arrays=(obs.data_ptr(), tm.data_ptr(), lm.data_ptr(), sg.data_ptr(), n, cnt.data_ptr()),
                     stream=st)      # (synchronises: the records are consumed when it returns)
        del keep
        return new, tot.cpu().numpy().view(REASSOCIATE_TOTALS)[0]

    def default_options(self):
        o = LmOptions()
        self.ctx._L.ecal_lm_default_options(ctypes.byref(o))
        return o

    def solve(self, params, options=None):
        p = np.array(params, dtype=np.float64, copy=True)
        s = LmSummary()
        o = options if options is not None else self.default_options()
        self.ctx._check(self.ctx._L.ecal_solver_solve(self._h, _ptr(p), ctypes.byref(o), ctypes.byref(s)))
        return p, s


def unpack_normal(acc, n_cp):
    """Normal-equation buffer -> (cost, g [9+6 n_cp], H dense symmetric) in the order [intr | cp0 (rot3, trans3) | ...]."""
    n = 9 + 6 * n_cp
    g = np.zeros(n)
    H = np.zeros((n, n))
    g[:9] = acc[1:10]
    Hi = acc[10:91].reshape(9, 9)
    H[:9, :9] = np.triu(Hi) + np.triu(Hi, 1).T
    for c in range(n_cp):
        b = acc[91 + 204 * c: 91 + 204 * (c + 1)]
        r0 = 9 + 6 * c
        g[r0:r0 + 6] = b[:6]
        H[r0:r0 + 6, :9] = b[6:60].reshape(6, 9)
        H[:9, r0:r0 + 6] = H[r0:r0 + 6, :9].T
        for d in range(4):
            if c + d >= n_cp:
                break
            blk = b[60 + 36 * d: 96 + 36 * d].reshape(6, 6)
            c1 = 9 + 6 * (c + d)
            if d == 0:
                H[r0:r0 + 6, r0:r0 + 6] = np.triu(blk) + np.triu(blk, 1).T
            else:
                H[r0:r0 + 6, c1:c1 + 6] = blk
                H[c1:c1 + 6, r0:r0 + 6] = blk.T
    return acc[0], g, H


def make_allreduce_hook(ctx: Context, world_size):
    """ALLREDUCE_FN for LmOptions.allreduce: sums the solver's device buffer over ranks with
    torch.distributed (backend "nccl" = RCCL over xGMI on ROCm; "gloo" works for CPU-side tests of the
    plumbing).  The buffer is staged through a torch tensor; full synchronisation on both sides keeps the
    solver's private stream and torch's collective stream ordered."""
    import torch
    import torch.distributed as dist
    state = {}

    def hook(user, d_buf, n, stream):
        try:
            if world_size <= 1:
                return 0
            t = state.get(n)
            if t is None:
                t = state[n] = torch.empty(n, dtype=torch.float64, device=torch.device("cuda", ctx.device))
            ctx._check(ctx._L.ecal_copy_dev(ctx._h, t.data_ptr(), d_buf, n * 8, stream, 1))
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            torch.cuda.synchronize(t.device)
            ctx._check(ctx._L.ecal_copy_dev(ctx._h, d_buf, t.data_ptr(), n * 8, stream, 1))
            return 0
        except Exception as e:  # never let an exception cross the C boundary
            print("allreduce hook failed:", e)
            return 1

    return ALLREDUCE_FN(hook)


# ---- init calibration on calibration views ----


def calibrate_views(ctx: Context, obj, img, width, height, model=0, flags=0, aspect_ratio=1.0, max_iter=0, eps=0.0,
                    allreduce=None, intr_guess=None):
    """ecal_calibrate_views: obj [n][3], img [V][n][2] (this rank's views).  Returns a dict.  intr_guess [12] goes with
    CALIB_USE_INTRINSIC_GUESS in flags."""
    L = ctx._L
    obj = np.ascontiguousarray(obj, np.float64)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, obj.shape[0], 2)
    V = img.shape[0]
    opt = CalibOptions()
    L.ecal_calib_default_options(ctypes.byref(opt))
    opt.model, opt.flags, opt.aspect_ratio, opt.max_iter, opt.eps = int(model), int(flags), float(aspect_ratio), int(max_iter), float(eps)
    if allreduce is not None:
        if isinstance(allreduce, tuple):   # Context.comm_allreduce_fn(): (function, user pointer)
            opt.allreduce, opt.allreduce_user = allreduce
        else:
            opt.allreduce = allreduce
    res = CalibResult()
    if intr_guess is not None:
        for j, v in enumerate(np.asarray(intr_guess, np.float64)[:12]):
            res.intr[j] = float(v)
    rv, tv, pe = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    ctx._check(L.ecal_calibrate_views(ctx._h, _ptr(obj), obj.shape[0], _ptr(img) if V else None, V, float(width), float(height),
                                      ctypes.byref(opt), ctypes.byref(res), _ptr(rv) if V else None, _ptr(tv) if V else None,
                                      _ptr(pe) if V else None))
    return {"intr": np.array(res.intr[:]), "rms": res.rms, "iterations": res.iterations, "rvecs": rv, "tvecs": tv,
            "per_view_err": pe, "jacobian_evaluations": res.jacobian_evaluations,
            "error_evaluations": res.error_evaluations, "seconds": res.seconds}


def calibrate_fisheye_views(ctx: Context, obj, img, width, height, flags=0, aspect_ratio=1.0, allreduce=None, intr_guess=None):
    """ecal_calibrate_fisheye_views: the fisheye init calibration with the library's start procedure (the reference's own start
    first, the radial model's focal lengths as a guess when that fails).  Returns calibrate_views' dict + "start_used".
    intr_guess [12] goes with CALIB_USE_INTRINSIC_GUESS in flags (one run, start_used 2)."""
    L = ctx._L
    obj = np.ascontiguousarray(obj, np.float64)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, obj.shape[0], 2)
    V = img.shape[0]
    opt = CalibOptions()
    L.ecal_calib_default_options(ctypes.byref(opt))
    opt.model, opt.flags, opt.aspect_ratio = 1, int(flags), float(aspect_ratio)
    if allreduce is not None:
        if isinstance(allreduce, tuple):
            opt.allreduce, opt.allreduce_user = allreduce
        else:
            opt.allreduce = allreduce
    res = CalibResult()
    if intr_guess is not None:
        for j, v in enumerate(np.asarray(intr_guess, np.float64)[:12]):
            res.intr[j] = float(v)
    rv, tv, pe = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    used = ctypes.c_int(-1)
    ctx._check(L.ecal_calibrate_fisheye_views(ctx._h, _ptr(obj), obj.shape[0], _ptr(img) if V else None, V, float(width), float(height),
                                              ctypes.byref(opt), ctypes.byref(res), _ptr(rv) if V else None, _ptr(tv) if V else None,
                                              _ptr(pe) if V else None, ctypes.byref(used)))
    return {"intr": np.array(res.intr[:]), "rms": res.rms, "iterations": res.iterations, "rvecs": rv, "tvecs": tv,
            "per_view_err": pe, "jacobian_evaluations": res.jacobian_evaluations, "error_evaluations": res.error_evaluations,
            "seconds": res.seconds, "start_used": int(used.value)}


def calib_view_blocks_dev(ctx: Context, d_obj, n_pts, d_img, n_views, model, flags, aspect_ratio, d_intr, d_view_params,
                          with_jacobian, d_blocks, stream=0):
    ctx._check(ctx._L.ecal_calib_view_blocks_dev(ctx._h, d_obj, n_pts, d_img, n_views, model, flags, aspect_ratio, d_intr,
                                                 d_view_params, int(with_jacobian), d_blocks, stream))


def pnp_batch_dev(ctx: Context, d_obj, n_pts, d_img, d_valid, n_frames, model, d_intr, reproj_thresh, rounds, refine_iters,
                  d_pose, d_inlier=None, d_err=None, d_ok=None, stream=0):
    ctx._check(ctx._L.ecal_pnp_batch_dev(ctx._h, d_obj, n_pts, d_img, d_valid, n_frames, model, d_intr, float(reproj_thresh),
                                         int(rounds), int(refine_iters), d_pose, d_inlier, d_err, d_ok, stream))


def pnp_batch(ctx: Context, obj, img, valid, model, intr, reproj_thresh, rounds, refine_iters):
    """ecal_pnp_batch, the host-buffer form of pnp_batch_dev: obj [n][3], img [F][n][2], valid [F][n] uint32 or None, intr [12].
    Returns {"pose" [F][6], "inlier" [F][n] uint32, "err" [F], "ok" [F] uint32}."""
    L = ctx._L
    obj = np.ascontiguousarray(obj, np.float64)
    n = obj.shape[0]
    img = np.ascontiguousarray(img, np.float64).reshape(-1, n, 2)
    F = img.shape[0]
    intr = np.ascontiguousarray(np.asarray(intr, np.float64)[:12])
    if valid is not None:
        valid = np.ascontiguousarray(valid, np.uint32).reshape(F, n)
    pose, inl, err, ok = np.zeros((F, 6)), np.zeros((F, n), np.uint32), np.zeros(F), np.zeros(F, np.uint32)
    ctx._check(L.ecal_pnp_batch(ctx._h, _ptr(obj), n, _ptr(img), _ptr(valid) if valid is not None else None, F, int(model),
                                _ptr(intr), float(reproj_thresh), int(rounds), int(refine_iters), _ptr(pose), _ptr(inl), _ptr(err),
                                _ptr(ok)))
    return {"pose": pose, "inlier": inl, "err": err, "ok": ok}


def spline_fit(u, data, n_cp):
    """ecal_spline_fit: returns (knots [n_cp + 4], control points [n_cp][dim])."""
    L = load_library()
    u = np.ascontiguousarray(u, np.float64)
    data = np.ascontiguousarray(data, np.float64).reshape(len(u), -1)
    knots, cp = np.zeros(n_cp + 4), np.zeros((n_cp, data.shape[1]))
    st = L.ecal_spline_fit(_ptr(u), _ptr(data), len(u), data.shape[1], n_cp, _ptr(knots), _ptr(cp))
    if st != 0:
        raise EcalError(st, L.ecal_strerror(st).decode())
    return knots, cp


def spline_eval(knots, cp, u):
    L = load_library()
    knots, cp, u = (np.ascontiguousarray(a, np.float64) for a in (knots, cp, u))
    out = np.zeros((len(u), cp.shape[1]))
    st = L.ecal_spline_eval(_ptr(knots), _ptr(cp), cp.shape[0], cp.shape[1], _ptr(u), len(u), _ptr(out))
    if st != 0:
        raise EcalError(st, L.ecal_strerror(st).decode())
    return out


def spline_so3_refine(knots, cp_quat, sample_quat, u, max_iterations=0):
    """ecal_spline_so3_refine (BsplineSO3::optimizeCP): returns (refined control points [n_cp][4], summary dict)."""
    L = load_library()
    knots, u = np.ascontiguousarray(knots, np.float64), np.ascontiguousarray(u, np.float64)
    cp = np.ascontiguousarray(cp_quat, np.float64).copy()
    sq = np.ascontiguousarray(sample_quat, np.float64)
    c0, c1, it = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
    st = L.ecal_spline_so3_refine(_ptr(knots), cp.shape[0], _ptr(cp), _ptr(sq), _ptr(u), len(u), int(max_iterations),
                                  ctypes.byref(c0), ctypes.byref(c1), ctypes.byref(it))
    if st != 0:
        raise EcalError(st, L.ecal_strerror(st).decode())
    return cp, {"initial_cost": c0.value, "final_cost": c1.value, "iterations": it.value}


# ---- double-buffered ingest ----


def detect_stream_tiled(ctx: Context, host_ptr, n_events, t_start, window_len, windows_per_chunk, max_windows, eps=4.0, minpts=2,
                        cluster_min=5, rows=9, cols=4, radius_threshold=15.511363636363637, want_features=True):
    """ecal_detect_stream_tiled over packed records at host address `host_ptr` (pinned for overlap).  Returns
    (win_info [S,4], grid_found [S], features [S, rows*cols, 3] or None, stats dict)."""
    L = ctx._L
    u32 = ctypes.c_uint32
    prm = DetectParams(float(eps), int(minpts), int(cluster_min), int(rows * cols), float(radius_threshold), 0, 3, int(rows), int(cols))
    info = np.zeros((max_windows, 4), np.uint32)
    found = np.zeros(max_windows, np.uint32)
    feat = np.zeros((max_windows, rows * cols, 3)) if want_features else None
    nw = u32(0)
    st = IngestStats()
    ctx._check(L.ecal_detect_stream_tiled(ctx._h, host_ptr, int(n_events), float(t_start), float(window_len), int(windows_per_chunk),
                                          ctypes.byref(prm), int(max_windows), _ptr(info), _ptr(found),
                                          _ptr(feat) if want_features else None, ctypes.byref(nw), ctypes.byref(st)))
    S = nw.value
    return info[:S], found[:S], (feat[:S] if want_features else None), {"chunks": st.chunks, "max_chunk_events": st.max_chunk_events,
                                                                      "bytes_uploaded": st.bytes_uploaded, "seconds": st.seconds}


def detect_keyframes_cap_hint(ctx: Context, n_events, motion_time_step, frame_event_num_threshold, piece_num, start_time, end_time,
                              piece_first=0, piece_count=0):
    """ecal_detect_keyframes_cap_hint: a cap_points that detect_keyframes_dev will usually find sufficient."""
    L = ctx._L
    ap = AdaptiveParams(float(motion_time_step), int(frame_event_num_threshold), int(piece_num), float(start_time), float(end_time), 0, 0, 0,
                        int(piece_first), int(piece_count))
    return int(L.ecal_detect_keyframes_cap_hint(ctypes.byref(ap), int(n_events)))


def detect_keyframes_cap_hint_dev(ctx: Context, d_events, n_events, motion_time_step, frame_event_num_threshold, piece_num, start_time,
                                  end_time, piece_first=0, piece_count=0):
    """ecal_detect_keyframes_cap_hint_dev: the hint from the events of the resident stream inside [start_time, end_time]."""
    L = ctx._L
    ap = AdaptiveParams(float(motion_time_step), int(frame_event_num_threshold), int(piece_num), float(start_time), float(end_time), 0, 0, 0,
                        int(piece_first), int(piece_count))
    return int(L.ecal_detect_keyframes_cap_hint_dev(ctx._h, d_events, int(n_events), ctypes.byref(ap)))


def detect_keyframes_dev(ctx: Context, d_events, n_events, motion_time_step, frame_event_num_threshold, piece_num, start_time,
                         end_time, cap_points, max_keyframes, eps=4.0, minpts=2, cluster_min=5, rows=9, cols=4,
                         radius_threshold=15.511363636363637, max_passes=0, check_every=0, gate_mode=0, piece_first=0, piece_count=0,
                         handover=None):
    """ecal_detect_keyframes (policy on the device; gate_mode: GATE_OWN_PIECE / GATE_SHARED_MAP; piece_count != 0: only the pieces
    piece_first .. piece_first + piece_count - 1 of the piece_num).  Returns (time [K], duration [K,2], events_num [K], features [K, rows cols, 3],
    passes, windows); raises EcalError(-6) when cap_points or max_keyframes is too small.
    handover (ecal_detect_keyframes_sharded: a subset of the pieces under GATE_SHARED_MAP): an object with recv(wait) -> None (not there
    yet; only when wait is false) or (has, time, dir [2 rows]) = the frame behind the pieces before this subset, and send(has, time,
    dir) for the frame behind this subset's pieces."""
    L = ctx._L
    u32 = ctypes.c_uint32
    ap = AdaptiveParams(float(motion_time_step), int(frame_event_num_threshold), int(piece_num), float(start_time), float(end_time),
                        int(max_passes), int(check_every), int(gate_mode), int(piece_first), int(piece_count))
    prm = DetectParams(float(eps), int(minpts), int(cluster_min), int(rows * cols), float(radius_threshold), 0, 3, int(rows), int(cols))
    M = rows * cols
    t = np.empty(max_keyframes)
    d = np.empty((max_keyframes, 2))
    e = np.empty(max_keyframes, np.int32)
    f = np.empty((max_keyframes, M, 3))
    nk, ps, nw = u32(0), u32(0), ctypes.c_uint64(0)
    try:
        if handover is None:
            ctx._check(L.ecal_detect_keyframes(ctx._h, d_events, int(n_events), ctypes.byref(ap), ctypes.byref(prm), int(cap_points),
                                               int(max_keyframes), _ptr(t), _ptr(d), _ptr(e), _ptr(f), ctypes.byref(nk), ctypes.byref(ps),
                                               ctypes.byref(nw)))
        else:
            errs = []

            def recv(user, frame, wait):
                try:
                    got = handover.recv(bool(wait))
                    if got is None:
                        return 0
                    frame[0].has, frame[0].time = int(bool(got[0])), float(got[1])
                    for i, v in enumerate(got[2][: 2 * rows]):
                        frame[0].dir[i] = float(v)
                    return 1
                except BaseException as ex:   # noqa: BLE001 — never let an exception cross the C frame
                    errs.append(ex)
                    return -1

            def send(user, frame):
                try:
                    handover.send(int(frame[0].has), float(frame[0].time), [float(frame[0].dir[i]) for i in range(2 * rows)])
                    return 0
                except BaseException as ex:   # noqa: BLE001
                    errs.append(ex)
                    return -1
            ho = AdaptiveHandover(_FRAME_RECV(recv), _FRAME_SEND(send), None)
            st = L.ecal_detect_keyframes_sharded(ctx._h, d_events, int(n_events), ctypes.byref(ap), ctypes.byref(prm), int(cap_points),
                                                 int(max_keyframes), _ptr(t), _ptr(d), _ptr(e), _ptr(f), ctypes.byref(nk), ctypes.byref(ps),
                                                 ctypes.byref(nw), ctypes.byref(ho))
            if errs:
                raise errs[0]
            ctx._check(st)
    except EcalError as err:
        err.n_keyframes = int(nk.value)     # ECAL_ERR_RANGE with a count beyond max_keyframes: the keyframe capacity was short
        raise
    K = nk.value
    return t[:K].copy(), d[:K].copy(), e[:K].astype(np.int64), f[:K].copy(), ps.value, nw.value


def detect_pass(ctx: Context, d_events, n_events, t0, t1, cap_points, eps=4.0, minpts=2, cluster_min=5, rows=9, cols=4,
                radius_threshold=15.511363636363637):
    """ecal_detect_pass: packed [S, 3 + 3 rows cols] = status, ok, unique pixels, ordered circles of every window."""
    L = ctx._L
    t0 = np.ascontiguousarray(t0, np.float64)
    t1 = np.ascontiguousarray(t1, np.float64)
    S = t0.shape[0]
    prm = DetectParams(float(eps), int(minpts), int(cluster_min), int(rows * cols), float(radius_threshold), 0, 3, int(rows), int(cols))
    out = np.empty((S, 3 + 3 * rows * cols))
    ctx._check(L.ecal_detect_pass(ctx._h, d_events, int(n_events), _ptr(t0), _ptr(t1), S, ctypes.byref(prm), int(cap_points), _ptr(out)))
    return out
