"""rfd_hip -- ctypes binding of librfd_hip.so (include/rfd.h) and a thin host mirror of the
reference's `RetinaFaceDetection` (src/pipeline/module/face_detection.rs:19-513).

All compute happens in the HIP library; this module only marshals numpy buffers.  There is no CPU
fallback: if the shared library is missing, or no MI355X is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "librfd_hip.so"))

RFD_OK = 0
RFD_ERR_INVALID_ARG = -1
RFD_ERR_NO_DEVICE = -2
PRECISION_BF16, PRECISION_F32 = 0, 1
SCHEDULE_THROUGHPUT, SCHEDULE_LATENCY = 0, 1
LATENCY_MAX_BATCH = 2   # RFD_LATENCY_MAX_BATCH: the largest pass a latency context runs with the split-K kernels
RFD_ERR_HIP = -3
RFD_ERR_CAPACITY = -4
RFD_ERR_STATE = -5
RFD_ERR_IO = -6
RFD_ERR_COMM = -7
RFD_ERR_UNSUPPORTED = -8
JPEG_GRAY, JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2, 3   # rfd_jpeg_sampling
JPEG_ENTROPY_HOST, JPEG_ENTROPY_DEVICE = 0, 1           # rfd_jpeg_entropy
JPEG_PATH_HOST, JPEG_PATH_DEVICE, JPEG_PATH_REFUSED = 0, 1, 2   # rfd_jpeg_last_paths
JPEG_ORIENTATION_IGNORE, JPEG_ORIENTATION_APPLY = 0, 1  # rfd_jpeg_orientation_mode
COMM_ID_BYTES = 128
MAX_FACE_TENSORS = 4   # RFD_MAX_FACE_TENSORS
GALLERY_MAX_K = 32     # RFD_GALLERY_MAX_K
NO_IDENTITY = -1       # RFD_GALLERY_NO_IDENTITY: an unlabelled gallery row, an identity of its own
NEAREST_OTHER_ROW, NEAREST_OTHER_IDENTITY = 0, 1   # RFD_GALLERY_NEAREST_*: the modes of Gallery.nearest

# debug_set_conv_tile / op_kernels_static: the forced tiles, enum ConvTile of csrc/kernels.h (each value's meaning is there)
(TILE_HEURISTIC, TILE_128, TILE_256x128, TILE_256x64, TILE_NO_128, TILE_NO_PW_STREAM, TILE_PERSISTENT, TILE_GENERIC, TILE_PW_STREAM,
 TILE_C64, TILE_PW_STREAM_K128, TILE_PW_STREAM_K256, TILE_PW_WIDE, TILE_HALO_SMALL, TILE_HALO_LARGE, TILE_PW_GEMM, TILE_PAIR, TILE_RING,
 TILE_128_EIGHT_WAVES, TILE_KX_FOUR_WAVES) = range(20)
BACKBONE_R50 = 0
BACKBONE_MNET025 = 1

STRIDES = (32, 16, 8)       # _feat_stride_fpn, face_detection.rs:52
NUM_ANCHORS = 2             # anchors per position


class RfdError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("rfd status %d: %s" % (status, message))
        self.status = status
        self.message = message   # the library's text alone


class rfd_config(C.Structure):
    _fields_ = [("image_w", C.c_int), ("image_h", C.c_int), ("max_batch_size", C.c_int),
                ("confidence_threshold", C.c_float), ("iou_threshold", C.c_float),
                ("device_id", C.c_int), ("max_det", C.c_int), ("max_src_w", C.c_int),
                ("max_src_h", C.c_int), ("backbone", C.c_int), ("precision", C.c_int), ("schedule", C.c_int),
                ("reserved", C.c_int * 4)]


class rfd_image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("height", C.c_int), ("width", C.c_int),
                ("stride", C.c_ssize_t)]


class rfd_dets(C.Structure):
    _fields_ = [("boxes", C.c_void_p), ("landmarks", C.c_void_p), ("count", C.c_void_p),
                ("total", C.c_void_p)]


class rfd_stats(C.Structure):
    _fields_ = [("ms_h2d", C.c_float), ("ms_preprocess", C.c_float), ("ms_network", C.c_float),
                ("ms_decode", C.c_float), ("ms_sort", C.c_float), ("ms_nms", C.c_float),
                ("ms_d2h", C.c_float), ("ms_total", C.c_float), ("candidates", C.c_int64),
                ("detections", C.c_int64), ("reserved", C.c_int64 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class rfd_layer_desc(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("cin", C.c_int), ("cout", C.c_int), ("kh", C.c_int),
                ("kw", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("has_affine", C.c_int),
                ("kind", C.c_int), ("reserved", C.c_int * 3)]


class rfd_op_desc(C.Structure):
    _fields_ = [("kind", C.c_int), ("layer", C.c_int), ("in_", C.c_int), ("out", C.c_int),
                ("out2", C.c_int), ("outf", C.c_int), ("res", C.c_int), ("relu", C.c_int),
                ("res_up2", C.c_int), ("res_post", C.c_int), ("head_softmax", C.c_int),
                ("y_coff", C.c_int), ("macs", C.c_double), ("in2", C.c_int), ("layer2", C.c_int),
                ("in_affine", C.c_int), ("layer_n2", C.c_int), ("x_coff", C.c_int), ("y_split", C.c_int),
                ("y_split_add", C.c_int), ("n_valid", C.c_int), ("branch", C.c_int), ("layer_b", C.c_int),
                ("out_b", C.c_int)]


class rfd_alignment_config(C.Structure):
    _fields_ = [("out_w", C.c_int32), ("out_h", C.c_int32), ("standard_landmarks", C.c_float * 10),
                ("reserved", C.c_int32 * 4)]


class rfd_face_tensor_config(C.Structure):
    _fields_ = [("out_w", C.c_int32), ("out_h", C.c_int32), ("mean", C.c_float * 3), ("scale", C.c_float * 3),
                ("reserved", C.c_int32 * 4)]


class rfd_faces(C.Structure):
    _fields_ = [("box", C.c_void_p), ("kps", C.c_void_p), ("found", C.c_void_p), ("crops", C.c_void_p),
                ("status", C.c_void_p), ("tensors", C.c_void_p * MAX_FACE_TENSORS)]


class rfd_face_list_config(C.Structure):
    _fields_ = [("max_faces", C.c_int32), ("min_face_px", C.c_float), ("min_score", C.c_float), ("reserved", C.c_int32 * 4)]


class rfd_face_list(C.Structure):
    _fields_ = [("total", C.c_void_p), ("first", C.c_void_p), ("frame", C.c_void_p), ("row", C.c_void_p), ("box", C.c_void_p),
                ("kps", C.c_void_p), ("status", C.c_void_p), ("crops", C.c_void_p), ("tensors", C.c_void_p * MAX_FACE_TENSORS)]


class rfd_liveness_config(C.Structure):
    _fields_ = [("k", C.c_int32), ("scale", C.c_float * MAX_FACE_TENSORS), ("out_w", C.c_int32 * MAX_FACE_TENSORS),
                ("out_h", C.c_int32 * MAX_FACE_TENSORS), ("reserved", C.c_int32 * 4)]


class rfd_gallery_nearest_config(C.Structure):
    _fields_ = [("mode", C.c_int32), ("min_score", C.c_float), ("tag_mask", C.c_uint32), ("reserved", C.c_int32 * 5)]


class rfd_gallery_nearest_plan(C.Structure):
    _fields_ = [("form", C.c_int32), ("tile_rows", C.c_int32), ("tiles", C.c_int32), ("splits", C.c_int32), ("blocks", C.c_int32),
                ("blocks_per_split", C.c_int32), ("grid", C.c_int64), ("ws_bytes", C.c_int64)]


class rfd_view(C.Structure):
    _fields_ = [("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("inner", C.c_uint32)]


class rfd_view_config(C.Structure):
    _fields_ = [("tile_w", C.c_int32), ("tile_h", C.c_int32), ("overlap", C.c_int32), ("full_view", C.c_int32), ("edge_margin", C.c_float)]


class rfd_tracker_config(C.Structure):
    _fields_ = [("streams", C.c_int32), ("max_tracks", C.c_int32), ("iou_min", C.c_float), ("max_missed", C.c_int32),
                ("min_score", C.c_float), ("new_score", C.c_float), ("min_hits", C.c_int32), ("improve", C.c_float),
                ("reserved", C.c_int32 * 4)]


class rfd_track_out(C.Structure):
    _fields_ = [("track", C.c_void_p), ("flags", C.c_void_p), ("stats", C.c_void_p), ("ended", C.c_void_p), ("due", rfd_dets),
                ("due_track", C.c_void_p)]


class rfd_track(C.Structure):
    _fields_ = [("slot", C.c_int32), ("serial", C.c_int32), ("box", C.c_float * 4), ("missed", C.c_int32), ("hits", C.c_int32),
                ("shot_q", C.c_float)]


class rfd_track_identity_config(C.Structure):
    _fields_ = [("dim", C.c_int32), ("accept", C.c_float), ("release", C.c_float), ("margin", C.c_float), ("reserved", C.c_int32 * 4)]


class rfd_track_obs(C.Structure):
    _fields_ = [("total", C.c_void_p), ("first", C.c_void_p), ("row", C.c_void_p), ("serial", C.c_void_p)]


class rfd_track_identity(C.Structure):
    _fields_ = [("slot", C.c_int32), ("serial", C.c_int32), ("identity", C.c_int32), ("row", C.c_int32), ("score", C.c_float),
                ("named", C.c_int32), ("shots", C.c_int32), ("weight", C.c_float)]


class rfd_track_shot_config(C.Structure):
    _fields_ = [("crop_w", C.c_int32), ("crop_h", C.c_int32), ("reserved", C.c_int32 * 6)]


class rfd_track_shot(C.Structure):
    _fields_ = [("slot", C.c_int32), ("serial", C.c_int32), ("shots", C.c_int32), ("kept", C.c_int32), ("q", C.c_float),
                ("reserved", C.c_int32), ("first_stamp", C.c_int64), ("best_stamp", C.c_int64)]


class rfd_track_record(C.Structure):
    _fields_ = [("stream", C.c_int32), ("serial", C.c_int32), ("frame", C.c_int32), ("shots", C.c_int32), ("kept", C.c_int32),
                ("q", C.c_float), ("first_stamp", C.c_int64), ("best_stamp", C.c_int64), ("end_stamp", C.c_int64),
                ("identity", C.c_int32), ("row", C.c_int32), ("id_score", C.c_float), ("named", C.c_int32), ("id_shots", C.c_int32),
                ("id_weight", C.c_float), ("reserved", C.c_int32 * 2)]


class rfd_track_records(C.Structure):
    _fields_ = [("total", C.c_void_p), ("first", C.c_void_p), ("rec", C.c_void_p), ("crops", C.c_void_p)]


class rfd_shot_quality_config(C.Structure):
    _fields_ = [("dark", C.c_int32), ("bright", C.c_int32), ("pitch0", C.c_float), ("w_yaw", C.c_float), ("w_roll", C.c_float),
                ("w_pitch", C.c_float), ("sharp_ref", C.c_float), ("size_ref", C.c_float), ("times_score", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class rfd_redact_config(C.Structure):
    _fields_ = [("mode", C.c_int32), ("shape", C.c_int32), ("cell", C.c_int32), ("fill", C.c_uint8 * 4), ("margin_x", C.c_float),
                ("margin_top", C.c_float), ("margin_bottom", C.c_float), ("sel_mask", C.c_uint32), ("sel_value", C.c_uint32),
                ("reserved", C.c_int32 * 6)]


class rfd_annotate_style(C.Structure):
    _fields_ = [("sel_mask", C.c_uint32), ("sel_value", C.c_uint32), ("colour", C.c_uint8 * 4)]


class rfd_annotate_config(C.Structure):
    _fields_ = [("n_styles", C.c_int32), ("style", rfd_annotate_style * 4), ("thickness", C.c_int32), ("mark_radius", C.c_int32),
                ("label_source", C.c_int32), ("value_source", C.c_int32), ("text_scale", C.c_int32), ("text_colour", C.c_uint8 * 4),
                ("alpha", C.c_int32), ("margin_x", C.c_float), ("margin_top", C.c_float), ("margin_bottom", C.c_float),
                ("reserved", C.c_int32 * 4)]


class rfd_frame(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_ssize_t * 3), ("width", C.c_int32), ("height", C.c_int32),
                ("format", C.c_int32), ("color", C.c_int32), ("reserved", C.c_int32 * 4)]


class rfd_frame_layout(C.Structure):
    _fields_ = [("planes", C.c_int32), ("row_bytes", C.c_int32 * 3), ("rows", C.c_int32 * 3), ("reserved", C.c_int32)]


class rfd_jpeg_info(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("sampling", C.c_int32),
                ("restart_interval", C.c_int32), ("reserved", C.c_int32 * 3)]


class rfd_jpeg_orientation(C.Structure):
    _fields_ = [("orientation", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("stored_width", C.c_int32),
                ("stored_height", C.c_int32), ("reserved", C.c_int32 * 3)]


class rfd_jpeg_scaled_size(C.Structure):
    _fields_ = [("denom", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("stored_width", C.c_int32),
                ("stored_height", C.c_int32), ("orientation", C.c_int32), ("reserved", C.c_int32 * 2)]


class rfd_jpeg_encode_config(C.Structure):
    _fields_ = [("quality", C.c_int32), ("sampling", C.c_int32), ("restart_rows", C.c_int32), ("reserved", C.c_int32 * 5)]


class rfd_tensor_desc(C.Structure):
    _fields_ = [("channels", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("is_f32", C.c_int), ("buffer", C.c_int), ("is_input", C.c_int),
                ("head_level", C.c_int), ("channels_logical", C.c_int), ("reserved", C.c_int * 3)]


# every symbol include/rfd.h declares (tests check that the library exports them all)
API_SYMBOLS = [
    "rfd_config_default", "rfd_create", "rfd_destroy", "rfd_last_error", "rfd_version",
    "rfd_graph_create", "rfd_graph_destroy", "rfd_graph_counts", "rfd_graph_layer", "rfd_graph_op",
    "rfd_graph_tensor", "rfd_graph_macs", "rfd_graph_workspace_bytes",
    "rfd_init_synthetic_weights", "rfd_num_layers", "rfd_get_layer_weights",
    "rfd_set_layer_weights", "rfd_get_layer_affine", "rfd_set_layer_affine", "rfd_detect_batch",
    "rfd_detect_batch_device", "rfd_sync", "rfd_set_stream", "rfd_preprocess", "rfd_forward", "rfd_decode_nms",
    "rfd_nms_sorted", "_nms", "rfd_get_stats", "rfd_get_config", "rfd_set_thresholds", "rfd_set_profiling",
    "rfd_get_conv_profile", "rfd_get_op_profile", "rfd_debug_tensor_io", "rfd_debug_run_ops", "rfd_debug_run_chain", "rfd_debug_pass_chains", "rfd_debug_buffer_io",
    "rfd_debug_set_conv_tile", "rfd_debug_op_kernels", "rfd_debug_op_kernels_static", "rfd_debug_set_concurrency", "rfd_debug_persistent_kernel", "rfd_debug_poke_nms_flag", "rfd_selection_config_default",
    "rfd_select_faces", "rfd_detect_select_batch", "rfd_save_weights", "rfd_load_weights",
    "rfd_alignment_config_default", "rfd_align_faces", "rfd_detect_select_align_batch", "rfd_debug_align_setup",
    "rfd_host_alloc", "rfd_host_free", "rfd_submit_batch", "rfd_collect_batch",
    "rfd_comm_get_unique_id", "rfd_comm_init", "rfd_comm_info", "rfd_gather_detections", "rfd_comm_destroy",
    "rfd_face_tensor_config_quality", "rfd_face_tensor_config_extraction", "rfd_face_tensors",
    "rfd_align_faces_tensors", "rfd_detect_select_align_tensors_batch", "rfd_detect_faces_device", "rfd_quality_decide", "rfd_normalize_embeddings",
    "rfd_quality_decide_device", "rfd_normalize_embeddings_device",
    "rfd_face_tensor_config_quality_assessment", "rfd_liveness_config_default", "rfd_liveness_tensors",
    "rfd_liveness_tensors_device", "rfd_liveness_decide", "rfd_liveness_decide_device",
    "rfd_gallery_create", "rfd_gallery_destroy", "rfd_gallery_size", "rfd_gallery_clear", "rfd_gallery_add", "rfd_gallery_add_device",
    "rfd_gallery_get_rows", "rfd_gallery_search", "rfd_gallery_search_device", "rfd_debug_gallery_offset",
    "rfd_gallery_remove", "rfd_gallery_replace", "rfd_gallery_replace_device", "rfd_gallery_live", "rfd_gallery_removed",
    "rfd_gallery_save", "rfd_gallery_load", "rfd_gallery_file_info",
    "rfd_gallery_set_identities", "rfd_gallery_get_identities", "rfd_gallery_identities", "rfd_gallery_search_identities",
    "rfd_gallery_search_identities_device",
    "rfd_gallery_set_tags", "rfd_gallery_get_tags", "rfd_gallery_search_filtered", "rfd_gallery_search_filtered_device",
    "rfd_gallery_nearest_config_default", "rfd_gallery_nearest", "rfd_gallery_nearest_device", "rfd_debug_gallery_nearest_plan",
    "rfd_jpeg_info", "rfd_decode_jpeg_batch_device", "rfd_decode_jpeg_batch", "rfd_set_decode_threads", "rfd_debug_jpeg_coefficients",
    "rfd_set_jpeg_entropy", "rfd_jpeg_last_paths", "rfd_debug_jpeg_intervals", "rfd_debug_jpeg_coefficients_device",
    "rfd_jpeg_orientation", "rfd_set_jpeg_orientation", "rfd_jpeg_last_orientations",
    "rfd_set_jpeg_scale", "rfd_jpeg_scaled_size", "rfd_debug_jpeg_block_counts",
    "rfd_face_list_config_default", "rfd_align_detections", "rfd_detect_align_all_batch", "rfd_detect_all_faces_device",
    "rfd_view_config_default", "rfd_view_plan", "rfd_detect_views_batch_device", "rfd_detect_views_batch", "rfd_decode_nms_views",
    "rfd_tracker_config_default", "rfd_tracker_create", "rfd_tracker_destroy", "rfd_tracker_update_device", "rfd_tracker_update",
    "rfd_tracker_reset", "rfd_tracker_get_tracks", "rfd_align_detections_device",
    "rfd_track_identity_config_default", "rfd_tracker_identity_enable", "rfd_tracker_fuse_device", "rfd_tracker_label_device",
    "rfd_tracker_who_device", "rfd_tracker_fuse", "rfd_tracker_label", "rfd_tracker_who", "rfd_tracker_get_identities",
    "rfd_tracker_get_template",
    "rfd_track_shot_config_default", "rfd_tracker_shots_enable", "rfd_tracker_keep_shots_device", "rfd_tracker_collect_ended_device",
    "rfd_tracker_keep_shots", "rfd_tracker_collect_ended", "rfd_tracker_get_shots", "rfd_tracker_get_shot_crop",
    "rfd_shot_quality_config_default", "rfd_shot_quality_device", "rfd_shot_quality",
    "rfd_frame_layout_of", "rfd_convert_frames_device", "rfd_upload_frames_device", "rfd_convert_frames",
    "rfd_jpeg_encode_config_default", "rfd_jpeg_encode_bound", "rfd_jpeg_encode_header", "rfd_encode_jpeg_batch_device", "rfd_encode_jpeg_batch",
    "rfd_debug_jpeg_encode_blocks", "rfd_debug_jpeg_encode_coefficients",
    "rfd_redact_config_default", "rfd_redact_faces_device", "rfd_redact_faces",
    "rfd_annotate_config_default", "rfd_annotate_faces_device", "rfd_annotate_faces", "rfd_debug_annotate_glyph",
]

_lib = None


def load_library(path=None):
    """Load librfd_hip.so.  Raises (never falls back) when the HIP extension is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RFD_HIP_LIB") or LIB_PATH  # RFD_HIP_LIB: A/B runs of two builds on one box
    if not os.path.exists(p):
        raise ImportError("librfd_hip.so not found at %s -- build it with "
                          "rs-face-detection_amd/build.sh (there is no CPU fallback)" % p)
    L = C.CDLL(p)
    vp, ci = C.c_void_p, C.c_int
    L.rfd_last_error.restype = C.c_char_p
    L.rfd_config_default.argtypes = [C.POINTER(rfd_config)]
    L.rfd_config_default.restype = None
    L.rfd_create.argtypes = [C.POINTER(rfd_config), C.POINTER(vp)]
    L.rfd_destroy.argtypes = [vp]
    L.rfd_destroy.restype = None
    L.rfd_graph_create.argtypes = [ci, ci, ci, C.POINTER(vp)]
    L.rfd_graph_destroy.argtypes = [vp]
    L.rfd_graph_destroy.restype = None
    L.rfd_graph_counts.argtypes = [vp] + [C.POINTER(ci)] * 4
    L.rfd_graph_layer.argtypes = [vp, ci, C.POINTER(rfd_layer_desc)]
    L.rfd_graph_op.argtypes = [vp, ci, C.POINTER(rfd_op_desc)]
    L.rfd_graph_tensor.argtypes = [vp, ci, C.POINTER(rfd_tensor_desc)]
    L.rfd_graph_macs.argtypes = [vp]
    L.rfd_graph_macs.restype = C.c_double
    L.rfd_graph_workspace_bytes.argtypes = [vp]
    L.rfd_graph_workspace_bytes.restype = C.c_double
    L.rfd_init_synthetic_weights.argtypes = [vp, C.c_uint64]
    L.rfd_num_layers.argtypes = [vp]
    L.rfd_get_layer_weights.argtypes = [vp, ci, vp, vp]
    L.rfd_set_layer_weights.argtypes = [vp, ci, vp, vp]
    L.rfd_get_layer_affine.argtypes = [vp, ci, vp, vp]
    L.rfd_set_layer_affine.argtypes = [vp, ci, vp, vp]
    L.rfd_detect_batch.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_dets)]
    L.rfd_detect_batch_device.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), ci]
    L.rfd_sync.argtypes = [vp]
    L.rfd_set_stream.argtypes = [vp, vp]
    L.rfd_preprocess.argtypes = [vp, C.POINTER(rfd_image), ci, vp, vp, vp]
    L.rfd_forward.argtypes = [vp, vp, ci, C.POINTER(vp)]
    L.rfd_decode_nms.argtypes = [vp, C.POINTER(vp), ci, vp, C.POINTER(rfd_dets), vp]
    L.rfd_nms_sorted.argtypes = [vp, vp, C.POINTER(ci), vp, ci, ci, C.c_float]
    L._nms.argtypes = [vp, C.POINTER(ci), vp, ci, ci, C.c_float, ci]
    L._nms.restype = None
    L.rfd_get_stats.argtypes = [vp, C.POINTER(rfd_stats)]
    L.rfd_get_config.argtypes = [vp, C.POINTER(rfd_config)]
    L.rfd_set_thresholds.argtypes = [vp, C.c_float, C.c_float]
    L.rfd_set_profiling.argtypes = [vp, ci]
    L.rfd_get_conv_profile.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(ci)]
    L.rfd_get_op_profile.argtypes = [vp, vp, ci]
    L.rfd_debug_tensor_io.argtypes = [vp, ci, ci, vp, ci]
    L.rfd_debug_run_ops.argtypes = [vp, ci, ci, ci]
    L.rfd_debug_run_chain.argtypes = [vp, ci, ci, ci, ci, ci]
    L.rfd_debug_pass_chains.argtypes = [vp, ci, C.POINTER(ci), ci]
    L.rfd_debug_buffer_io.argtypes = [vp, ci, vp, C.c_size_t, ci, C.POINTER(C.c_size_t)]
    L.rfd_debug_set_conv_tile.argtypes = [vp, ci]
    L.rfd_debug_set_concurrency.argtypes = [vp, ci, ci, ci, ci]
    L.rfd_debug_op_kernels.argtypes = [vp, ci, ci, ci, C.c_char_p, ci]
    L.rfd_debug_op_kernels_static.argtypes = [ci] * 9 + [C.c_char_p, ci]
    L.rfd_debug_poke_nms_flag.argtypes = [vp, ci]
    L.rfd_debug_persistent_kernel.argtypes = [ci, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
    L.rfd_save_weights.argtypes = [vp, C.c_char_p]
    L.rfd_load_weights.argtypes = [vp, C.c_char_p]
    L.rfd_selection_config_default.argtypes = [vp]
    L.rfd_selection_config_default.restype = None
    L.rfd_select_faces.argtypes = [vp, C.POINTER(rfd_dets), vp, vp, ci, vp, ci, vp, vp, vp]
    L.rfd_detect_select_batch.argtypes = [vp, C.POINTER(rfd_image), ci, vp, ci, vp, vp, vp]
    L.rfd_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.rfd_host_free.argtypes = [vp]
    L.rfd_submit_batch.argtypes = [vp, C.POINTER(rfd_image), ci]
    L.rfd_collect_batch.argtypes = [vp, C.POINTER(rfd_dets), C.POINTER(ci)]
    L.rfd_comm_get_unique_id.argtypes = [vp]
    L.rfd_comm_init.argtypes = [vp, vp, ci, ci]
    L.rfd_comm_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.rfd_gather_detections.argtypes = [vp, C.POINTER(rfd_dets), ci, C.POINTER(rfd_dets)]
    L.rfd_comm_destroy.argtypes = [vp]
    L.rfd_alignment_config_default.argtypes = [C.POINTER(rfd_alignment_config)]
    L.rfd_alignment_config_default.restype = None
    L.rfd_align_faces.argtypes = [vp, C.POINTER(rfd_image), ci, vp, vp, vp, vp, vp, vp]
    L.rfd_detect_select_align_batch.argtypes = [vp, C.POINTER(rfd_image), ci, vp, ci, vp, vp, vp, vp, vp, vp]
    L.rfd_debug_align_setup.argtypes = [vp, ci] + [vp] * 11
    for f in (L.rfd_face_tensor_config_quality, L.rfd_face_tensor_config_extraction):
        f.argtypes = [C.POINTER(rfd_face_tensor_config)]
        f.restype = None
    L.rfd_face_tensors.argtypes = [vp, vp, ci, ci, ci, vp, ci, C.POINTER(vp)]
    L.rfd_detect_select_align_tensors_batch.argtypes = [vp, C.POINTER(rfd_image), ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, C.POINTER(vp)]
    L.rfd_align_faces_tensors.argtypes = [vp, C.POINTER(rfd_image), ci, vp, vp, vp, vp, vp, vp, vp, ci, C.POINTER(vp)]
    L.rfd_detect_faces_device.argtypes = [vp, C.POINTER(rfd_image), ci, vp, ci, vp, vp, ci, C.POINTER(rfd_faces), ci]
    L.rfd_face_list_config_default.argtypes = [C.POINTER(rfd_face_list_config)]
    L.rfd_face_list_config_default.restype = None
    L.rfd_align_detections.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), vp, vp, vp, ci, ci, C.POINTER(rfd_face_list)]
    L.rfd_detect_align_all_batch.argtypes = [vp, C.POINTER(rfd_image), ci, vp, vp, vp, ci, ci, C.POINTER(rfd_face_list)]
    L.rfd_detect_all_faces_device.argtypes = [vp, C.POINTER(rfd_image), ci, vp, vp, vp, ci, ci, C.POINTER(rfd_face_list), ci]
    L.rfd_quality_decide.argtypes = [vp, vp, ci, ci, C.c_float, vp, vp]
    L.rfd_quality_decide_device.argtypes = [vp, vp, ci, ci, C.c_float, vp, vp]
    L.rfd_normalize_embeddings.argtypes = [vp, vp, ci, ci, vp]
    L.rfd_normalize_embeddings_device.argtypes = [vp, vp, ci, ci, vp]
    L.rfd_face_tensor_config_quality_assessment.argtypes = [C.POINTER(rfd_face_tensor_config), ci, ci]
    L.rfd_face_tensor_config_quality_assessment.restype = None
    L.rfd_liveness_config_default.argtypes = [C.POINTER(rfd_liveness_config)]
    L.rfd_liveness_config_default.restype = None
    L.rfd_liveness_tensors.argtypes = [vp, C.POINTER(rfd_image), ci, vp, vp, vp, C.POINTER(vp), vp, vp, vp]
    L.rfd_liveness_tensors_device.argtypes = [vp, C.POINTER(rfd_image), ci, vp, vp, vp, C.POINTER(vp), vp, vp, vp, ci]
    L.rfd_liveness_decide.argtypes = [vp, C.POINTER(vp), ci, ci, ci, vp, C.c_float, vp, vp]
    L.rfd_liveness_decide_device.argtypes = [vp, C.POINTER(vp), ci, ci, ci, vp, C.c_float, vp, vp]
    L.rfd_gallery_create.argtypes = [vp, ci, ci, C.POINTER(vp)]
    L.rfd_gallery_destroy.argtypes = [vp]
    L.rfd_gallery_destroy.restype = None
    L.rfd_gallery_size.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.rfd_gallery_clear.argtypes = [vp]
    L.rfd_gallery_add.argtypes = [vp, vp, ci, C.POINTER(ci)]
    L.rfd_gallery_add_device.argtypes = [vp, vp, ci, C.POINTER(ci)]
    L.rfd_gallery_get_rows.argtypes = [vp, ci, ci, vp]
    L.rfd_gallery_search.argtypes = [vp, vp, ci, ci, vp, vp]
    L.rfd_gallery_search_device.argtypes = [vp, vp, ci, ci, vp, vp, ci]
    L.rfd_debug_gallery_offset.argtypes = [ci, ci, ci]
    L.rfd_debug_gallery_offset.restype = C.c_int64
    L.rfd_gallery_remove.argtypes = [vp, vp, ci]
    L.rfd_gallery_replace.argtypes = [vp, vp, vp, ci]
    L.rfd_gallery_replace_device.argtypes = [vp, vp, vp, ci]
    L.rfd_gallery_live.argtypes = [vp, C.POINTER(ci)]
    L.rfd_gallery_removed.argtypes = [vp, vp, ci, C.POINTER(ci)]
    L.rfd_gallery_set_identities.argtypes = [vp, vp, vp, ci]
    L.rfd_gallery_get_identities.argtypes = [vp, ci, ci, vp]
    L.rfd_gallery_identities.argtypes = [vp, C.POINTER(ci)]
    L.rfd_gallery_search_identities.argtypes = [vp, vp, ci, ci, C.c_float, vp, vp, vp]
    L.rfd_gallery_search_identities_device.argtypes = [vp, vp, ci, ci, C.c_float, vp, vp, vp, ci]
    L.rfd_gallery_set_tags.argtypes = [vp, vp, vp, ci]
    L.rfd_gallery_get_tags.argtypes = [vp, ci, ci, vp]
    L.rfd_gallery_search_filtered.argtypes = [vp, vp, ci, ci, C.c_float, vp, vp, vp, vp, vp]
    L.rfd_gallery_search_filtered_device.argtypes = [vp, vp, ci, ci, C.c_float, vp, vp, vp, vp, vp, ci]
    L.rfd_gallery_nearest_config_default.argtypes = [C.POINTER(rfd_gallery_nearest_config)]
    L.rfd_gallery_nearest_config_default.restype = None
    L.rfd_gallery_nearest.argtypes = [vp, ci, ci, C.POINTER(rfd_gallery_nearest_config), vp, vp, vp]
    L.rfd_gallery_nearest_device.argtypes = [vp, ci, ci, C.POINTER(rfd_gallery_nearest_config), vp, vp, vp, ci]
    L.rfd_debug_gallery_nearest_plan.argtypes = [ci, ci, ci, ci, ci, C.POINTER(rfd_gallery_nearest_plan)]
    L.rfd_gallery_save.argtypes = [vp, C.c_char_p]
    L.rfd_gallery_load.argtypes = [vp, C.c_char_p, ci, C.POINTER(vp)]
    L.rfd_gallery_file_info.argtypes = [C.c_char_p, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.rfd_jpeg_info.argtypes = [vp, C.c_size_t, C.POINTER(rfd_jpeg_info)]
    L.rfd_decode_jpeg_batch_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), ci, C.POINTER(rfd_image), ci]
    L.rfd_decode_jpeg_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), ci, C.POINTER(rfd_image)]
    L.rfd_set_decode_threads.argtypes = [vp, ci]
    L.rfd_debug_jpeg_coefficients.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rfd_set_jpeg_entropy.argtypes = [vp, ci]
    L.rfd_jpeg_last_paths.argtypes = [vp, vp, ci, C.POINTER(ci)]
    L.rfd_debug_jpeg_intervals.argtypes = [vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rfd_debug_jpeg_coefficients_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rfd_jpeg_orientation.argtypes = [vp, C.c_size_t, C.POINTER(rfd_jpeg_orientation)]
    L.rfd_set_jpeg_orientation.argtypes = [vp, ci]
    L.rfd_jpeg_last_orientations.argtypes = [vp, vp, ci, C.POINTER(ci)]
    L.rfd_set_jpeg_scale.argtypes = [vp, ci]
    L.rfd_jpeg_scaled_size.argtypes = [vp, C.c_size_t, ci, ci, C.POINTER(rfd_jpeg_scaled_size)]
    L.rfd_debug_jpeg_block_counts.argtypes = [vp, C.c_size_t, ci, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rfd_view_config_default.argtypes = [C.POINTER(rfd_view_config), ci, ci]
    L.rfd_view_config_default.restype = None
    L.rfd_view_plan.argtypes = [ci, ci, ci, C.POINTER(rfd_view_config), C.POINTER(rfd_view), ci, C.POINTER(ci)]
    L.rfd_detect_views_batch_device.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_view), ci, C.c_float, C.POINTER(rfd_dets), ci]
    L.rfd_detect_views_batch.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_view), ci, C.c_float, C.POINTER(rfd_dets)]
    L.rfd_decode_nms_views.argtypes = [vp, C.POINTER(vp), C.POINTER(rfd_view), ci, ci, C.c_float, C.POINTER(rfd_dets), vp]
    L.rfd_tracker_config_default.argtypes = [vp, C.POINTER(rfd_tracker_config)]
    L.rfd_tracker_create.argtypes = [vp, C.POINTER(rfd_tracker_config), C.POINTER(vp)]
    L.rfd_tracker_destroy.argtypes = [vp]
    L.rfd_tracker_destroy.restype = None
    L.rfd_tracker_update_device.argtypes = [vp, vp, C.POINTER(rfd_dets), vp, ci, C.POINTER(rfd_track_out), ci]
    L.rfd_tracker_update.argtypes = [vp, vp, C.POINTER(rfd_dets), vp, ci, C.POINTER(rfd_track_out)]
    L.rfd_tracker_reset.argtypes = [vp, ci]
    L.rfd_tracker_get_tracks.argtypes = [vp, ci, C.POINTER(rfd_track), ci, C.POINTER(ci)]
    L.rfd_track_identity_config_default.argtypes = [C.POINTER(rfd_track_identity_config)]
    L.rfd_tracker_identity_enable.argtypes = [vp, C.POINTER(rfd_track_identity_config)]
    L.rfd_tracker_fuse_device.argtypes = [vp, vp, ci, C.POINTER(rfd_track_obs), ci, vp, vp, vp, vp, ci]
    L.rfd_tracker_label_device.argtypes = [vp, vp, ci, C.POINTER(rfd_track_obs), ci, ci, vp, vp, vp, vp, ci]
    L.rfd_tracker_who_device.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, ci]
    L.rfd_tracker_fuse.argtypes = [vp, vp, ci, C.POINTER(rfd_track_obs), ci, vp, vp, vp, vp]
    L.rfd_tracker_label.argtypes = [vp, vp, ci, C.POINTER(rfd_track_obs), ci, ci, vp, vp, vp, vp]
    L.rfd_tracker_who.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.rfd_tracker_get_identities.argtypes = [vp, ci, C.POINTER(rfd_track_identity), ci, C.POINTER(ci)]
    L.rfd_tracker_get_template.argtypes = [vp, ci, C.c_int32, vp]
    L.rfd_track_shot_config_default.argtypes = [C.POINTER(rfd_track_shot_config)]
    L.rfd_tracker_shots_enable.argtypes = [vp, C.POINTER(rfd_track_shot_config)]
    L.rfd_tracker_keep_shots_device.argtypes = [vp, vp, vp, ci, C.POINTER(rfd_track_obs), ci, vp, vp, vp, vp, ci]
    L.rfd_tracker_collect_ended_device.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.POINTER(rfd_track_records), ci]
    L.rfd_tracker_keep_shots.argtypes = [vp, vp, vp, ci, C.POINTER(rfd_track_obs), ci, vp, vp, vp, vp]
    L.rfd_tracker_collect_ended.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.POINTER(rfd_track_records)]
    L.rfd_tracker_get_shots.argtypes = [vp, ci, C.POINTER(rfd_track_shot), ci, C.POINTER(ci)]
    L.rfd_tracker_get_shot_crop.argtypes = [vp, ci, C.c_int32, vp]
    L.rfd_align_detections_device.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), vp, vp, vp, ci, ci, C.POINTER(rfd_face_list), ci]
    L.rfd_shot_quality_config_default.argtypes = [C.POINTER(rfd_shot_quality_config)]
    L.rfd_shot_quality_device.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), C.POINTER(rfd_shot_quality_config), vp, vp, vp, ci]
    L.rfd_shot_quality.argtypes = [vp, C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), C.POINTER(rfd_shot_quality_config), vp, vp, vp]
    L.rfd_frame_layout_of.argtypes = [ci, ci, ci, C.POINTER(rfd_frame_layout)]
    L.rfd_convert_frames_device.argtypes = [vp, C.POINTER(rfd_frame), ci, C.POINTER(rfd_image), ci]
    L.rfd_upload_frames_device.argtypes = [vp, C.POINTER(rfd_frame), ci, C.POINTER(rfd_image), ci]
    L.rfd_convert_frames.argtypes = [vp, C.POINTER(rfd_frame), ci, C.POINTER(rfd_image)]
    ecfg = C.POINTER(rfd_jpeg_encode_config)
    L.rfd_jpeg_encode_config_default.argtypes = [ecfg]
    L.rfd_jpeg_encode_bound.argtypes = [ci, ci, ecfg, C.POINTER(C.c_size_t)]
    L.rfd_jpeg_encode_header.argtypes = [ci, ci, ecfg, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rfd_encode_jpeg_batch_device.argtypes = [vp, C.POINTER(rfd_image), ci, vp, ecfg, vp, C.c_size_t, vp, ci]
    L.rfd_encode_jpeg_batch.argtypes = [vp, C.POINTER(rfd_image), ci, ecfg, vp, C.c_size_t, vp]
    L.rfd_debug_jpeg_encode_blocks.argtypes = [vp, C.POINTER(rfd_image), ecfg, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rfd_debug_jpeg_encode_coefficients.argtypes = [vp, vp, C.c_size_t, ci, ci, ecfg, vp, C.c_size_t, C.POINTER(C.c_int32)]
    rcfg = C.POINTER(rfd_redact_config)
    L.rfd_redact_config_default.argtypes = [rcfg]
    L.rfd_redact_faces_device.argtypes = [vp, C.POINTER(rfd_image), C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), vp, rcfg, vp, ci]
    L.rfd_redact_faces.argtypes = [vp, C.POINTER(rfd_image), C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), vp, rcfg, vp]
    acfg = C.POINTER(rfd_annotate_config)
    L.rfd_annotate_config_default.argtypes = [acfg]
    L.rfd_annotate_faces_device.argtypes = [vp, C.POINTER(rfd_image), C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), vp, vp, vp, acfg, vp, ci]
    L.rfd_annotate_faces.argtypes = [vp, C.POINTER(rfd_image), C.POINTER(rfd_image), ci, C.POINTER(rfd_dets), vp, vp, vp, acfg, vp]
    L.rfd_debug_annotate_glyph.argtypes = [ci, C.POINTER(C.c_uint8 * 7)]
    if path is None:
        _lib = L
    return L


def _check(status):
    if status < 0:
        raise RfdError(status, load_library().rfd_last_error().decode("utf-8", "replace"))
    return status


def face_tensor_config(image_size, mean, scale):
    """rfd_face_tensor_config of a model: image_size (w, h); mean, scale per output channel R, G, B"""
    c = rfd_face_tensor_config()
    c.out_w, c.out_h = int(image_size[0]), int(image_size[1])
    for i in range(3):
        c.mean[i], c.scale[i] = mean[i], scale[i]
    return c


def face_tensor_config_quality():
    """the input of the quality model (face_quality.rs:43-44): 112 x 112, ImageNet mean / reciprocal std"""
    c = rfd_face_tensor_config()
    load_library().rfd_face_tensor_config_quality(C.byref(c))
    return c


def face_tensor_config_extraction():
    """the input of the ID model (face_extraction.rs:38-39): 112 x 112, (p - 127.5) / 128"""
    c = rfd_face_tensor_config()
    load_library().rfd_face_tensor_config_extraction(C.byref(c))
    return c


def face_tensor_config_quality_assessment(image_size):
    """the input of the quality-assessment model (face_quality_assessment.rs:50-76): image_size (w, h), (p - 127.5) * 0.00784313725;
    its decision is logit[0] > threshold on the model's one logit"""
    c = rfd_face_tensor_config()
    load_library().rfd_face_tensor_config_quality_assessment(C.byref(c), int(image_size[0]), int(image_size[1]))
    return c


def liveness_config(scales=None, image_sizes=None):
    """rfd_liveness_config: the four miniFAS models the reference names (face_antispoofing.rs:448-485), or one model per
    entry of scales / image_sizes [(w, h)] (more than MAX_FACE_TENSORS: the library refuses the call)"""
    c = rfd_liveness_config()
    load_library().rfd_liveness_config_default(C.byref(c))
    if scales is not None:
        c.k = len(scales)
        for j in range(min(c.k, MAX_FACE_TENSORS)):
            c.scale[j] = scales[j]
            c.out_w[j], c.out_h[j] = int(image_sizes[j][0]), int(image_sizes[j][1])
    return c


def face_list_config(max_faces=None, min_face_px=None, min_score=None):
    """rfd_face_list_config: the default (32 faces per frame, no size or score floor) with the given fields replaced"""
    c = rfd_face_list_config()
    load_library().rfd_face_list_config_default(C.byref(c))
    if max_faces is not None:
        c.max_faces = int(max_faces)
    if min_face_px is not None:
        c.min_face_px = min_face_px
    if min_score is not None:
        c.min_score = min_score
    return c


class FaceList:
    """The host arrays of an rfd_face_list for n frames and cap faces: total [1], first [n + 1], frame / row / status [cap],
    box [cap, 5], kps [cap, 5, 2], crops [cap, h, w, 3] or None, tensors [k] of [cap, 3, out_h, out_w].  The library writes
    rows below `valid` = min(total, cap) only; whatever the arrays held beyond them stays (fill: the byte they start with)."""

    def __init__(self, n, cap, cfgs, crop_size=(112, 112), want_crops=True, fill=0):
        cap = max(int(cap), 1)
        new = lambda shape, dt: np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()
        self.cap = cap
        self.total, self.first = new((1,), np.int32), new((n + 1,), np.int32)
        self.frame, self.row, self.status = new((cap,), np.int32), new((cap,), np.int32), new((cap,), np.int32)
        self.box, self.kps = new((cap, 5), np.float32), new((cap, 5, 2), np.float32)
        self.crops = new((cap, crop_size[1], crop_size[0], 3), np.uint8) if want_crops else None
        self.tensors = [new((cap, 3, max(c.out_h, 1), max(c.out_w, 1)), np.float32) for c in cfgs[:MAX_FACE_TENSORS]]

    @property
    def valid(self):
        return min(int(self.total[0]), self.cap)

    def struct(self):
        s = rfd_face_list(self.total.ctypes.data, self.first.ctypes.data, self.frame.ctypes.data, self.row.ctypes.data,
                          self.box.ctypes.data, self.kps.ctypes.data, self.status.ctypes.data,
                          None if self.crops is None else self.crops.ctypes.data)
        for j, t in enumerate(self.tensors):
            s.tensors[j] = t.ctypes.data
        return s


def _face_tensor_args(cfgs, n):
    """(config array, output arrays, pointer array) of n faces; sizes the library would refuse get a 1-element stand-in"""
    k = len(cfgs)
    arr = (rfd_face_tensor_config * max(k, 1))(*cfgs)
    outs = [np.zeros((n, 3, max(c.out_h, 1), max(c.out_w, 1)), np.float32) for c in cfgs]
    ptrs = (C.c_void_p * max(k, 1))(*[o.ctypes.data for o in outs])
    return arr, outs, ptrs


def gallery_offset(dim, row, d):
    """element offset of (row, d) in a gallery's private storage layout (rfd_debug_gallery_offset; host only, -1: out of range)"""
    return int(load_library().rfd_debug_gallery_offset(int(dim), int(row), int(d)))


GALLERY_FILE_MAGIC, GALLERY_FILE_VERSION = b"RFDG", 1


def _bf16_bits(values):
    """f32 array of values that are exact in bf16 -> their 16 bits (the upper half of the f32 bits)"""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    assert not np.any(bits & 0xffff), "values are not exact in bf16"
    return (bits >> 16).astype("<u2")


def gallery_nearest_plan(rows, row0, n, dim, cus):
    """how Gallery.nearest(row0, n) decomposes on a gallery of `rows` rows and a device of `cus` compute units
    (rfd_debug_gallery_nearest_plan; host only) -> dict of form, tile_rows, tiles, splits, blocks, blocks_per_split, grid, ws_bytes"""
    p = rfd_gallery_nearest_plan()
    _check(load_library().rfd_debug_gallery_nearest_plan(int(rows), int(row0), int(n), int(dim), int(cus), C.byref(p)))
    return {k: int(getattr(p, k)) for k, _ in p._fields_}


def view_config(net_size=(640, 640), tile=None, overlap=None, full_view=None, edge_margin=None):
    """rfd_view_config (rfd.h, "views"): the defaults for a network of net_size (w, h) -- tile = the network size, overlap =
    net_w / 5, the full view, a margin of 4 network pixels -- with the fields given replaced; tile is (w, h)"""
    c = rfd_view_config()
    load_library().rfd_view_config_default(C.byref(c), int(net_size[0]), int(net_size[1]))
    if tile is not None:
        c.tile_w, c.tile_h = int(tile[0]), int(tile[1])
    if overlap is not None:
        c.overlap = int(overlap)
    if full_view is not None:
        c.full_view = int(bool(full_view))
    if edge_margin is not None:
        c.edge_margin = float(edge_margin)
    return c


def view_plan(frame_w, frame_h, cfg, frame=0):
    """the views of one frame (rfd_view_plan), as a list of rfd_view; needs no context and no device"""
    L, n = load_library(), C.c_int(0)
    status = L.rfd_view_plan(int(frame), int(frame_w), int(frame_h), C.byref(cfg), None, 0, C.byref(n))
    if status != RFD_ERR_CAPACITY:
        _check(status)
    out = (rfd_view * max(n.value, 1))()
    _check(L.rfd_view_plan(int(frame), int(frame_w), int(frame_h), C.byref(cfg), out, n.value, C.byref(n)))
    return [rfd_view(v.frame, v.x, v.y, v.w, v.h, v.inner) for v in out[:n.value]]


def _view_array(views):
    """views: rfd_view structures or (frame, x, y, w, h, inner) tuples"""
    arr = (rfd_view * max(len(views), 1))()
    for i, v in enumerate(views):
        arr[i] = v if isinstance(v, rfd_view) else rfd_view(*[int(a) for a in v])
    return arr


def gallery_file_write(path, values_bf16_as_f32, live):
    """Writes a gallery file (rfd.h, "gallery file") from values [rows, dim] that are exact in bf16 (what Gallery.rows returns)
    and a boolean mask [rows] of the live rows.  Pure numpy: the format stated a second time, apart from the library's code."""
    v = np.ascontiguousarray(values_bf16_as_f32, np.float32)
    live = np.asarray(live, bool).reshape(-1)
    assert v.ndim == 2 and live.shape[0] == v.shape[0]
    with open(path, "wb") as f:
        f.write(GALLERY_FILE_MAGIC + np.array([GALLERY_FILE_VERSION, v.shape[1], v.shape[0], 0], "<u4").tobytes())
        f.write(np.packbits(live, bitorder="little").tobytes())
        f.write(_bf16_bits(v).tobytes())


def gallery_file_read(path):
    """-> (values [rows, dim] f32, live [rows] bool) of a gallery file; pure numpy, checks nothing but the magic and the length"""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:4] == GALLERY_FILE_MAGIC, "not a gallery file"
    version, dim, rows, _ = (int(x) for x in np.frombuffer(data, "<u4", 4, 4))
    nbits = (rows + 7) // 8
    assert version == GALLERY_FILE_VERSION and len(data) == 20 + nbits + rows * dim * 2
    live = np.unpackbits(np.frombuffer(data, np.uint8, nbits, 20), bitorder="little")[:rows].astype(bool)
    bits = np.frombuffer(data, "<u2", rows * dim, 20 + nbits).astype(np.uint32) << 16
    return bits.view(np.float32).reshape(rows, dim), live


def gallery_file_info(path):
    """(dim, rows, live rows) of a gallery file after the library's whole validation (rfd_gallery_file_info; host only, no GPU)"""
    dim, rows, live = C.c_int(), C.c_int(), C.c_int()
    _check(load_library().rfd_gallery_file_info(os.fsencode(path), C.byref(dim), C.byref(rows), C.byref(live)))
    return dim.value, rows.value, live.value


def _byte_buffer(data):
    """bytes-like -> (object that keeps the memory alive, address, length)"""
    b = np.frombuffer(bytes(data) if not isinstance(data, (bytes, bytearray, np.ndarray)) else data, np.uint8)
    return b, (b.ctypes.data if b.size else None), int(b.size)


def jpeg_info(data):
    """the header of a JPEG file (bytes) after the library's whole marker validation (rfd_jpeg_info; host only, no GPU) ->
    dict(width, height, components, sampling = JPEG_GRAY / _444 / _422 / _420, restart_interval).  A file the decoder would
    refuse raises RfdError with RFD_ERR_UNSUPPORTED or RFD_ERR_INVALID_ARG and the cause."""
    keep, addr, n = _byte_buffer(data)
    info = rfd_jpeg_info()
    _check(load_library().rfd_jpeg_info(addr, n, C.byref(info)))
    return dict(width=info.width, height=info.height, components=info.components, sampling=info.sampling,
                restart_interval=info.restart_interval)


def jpeg_orientation(data):
    """the EXIF orientation of a JPEG file (bytes) after the same validation as jpeg_info (rfd_jpeg_orientation; host only, no
    GPU) -> dict(orientation = 1..8, width, height = the size of the frame a decode in "apply" mode writes (swapped for 5..8),
    stored_width, stored_height).  A file without a usable tag has orientation 1; EXIF damage never refuses a file."""
    keep, addr, n = _byte_buffer(data)
    o = rfd_jpeg_orientation()
    _check(load_library().rfd_jpeg_orientation(addr, n, C.byref(o)))
    return dict(orientation=o.orientation, width=o.width, height=o.height, stored_width=o.stored_width,
                stored_height=o.stored_height)


def jpeg_scaled_size(data, denom, orientation="ignore"):
    """the size of the frame a decode at 1 / denom (1, 2, 4, 8) in this orientation mode ("ignore" / "apply") writes, after the
    same validation as jpeg_info (rfd_jpeg_scaled_size; host only, no GPU) -> dict(denom, width, height = ceil(stored / denom),
    swapped for orientations 5..8 in "apply" mode, stored_width, stored_height, orientation = the one that will be applied)"""
    keep, addr, n = _byte_buffer(data)
    modes = {"ignore": JPEG_ORIENTATION_IGNORE, "apply": JPEG_ORIENTATION_APPLY}
    z = rfd_jpeg_scaled_size()
    _check(load_library().rfd_jpeg_scaled_size(addr, n, int(denom), modes[orientation] if orientation in modes else int(orientation), C.byref(z)))
    return dict(denom=z.denom, width=z.width, height=z.height, stored_width=z.stored_width, stored_height=z.stored_height,
                orientation=z.orientation)


def jpeg_block_counts(data, denom):
    """the count of every block's record as the host entropy decoder writes it at 1 / denom, [blocks] u8 in the block order of
    jpeg_coefficients (rfd_debug_jpeg_block_counts; host only, no GPU)"""
    keep, addr, n = _byte_buffer(data)
    L, blocks = load_library(), C.c_size_t(0)
    st = L.rfd_debug_jpeg_block_counts(addr, n, int(denom), None, 0, C.byref(blocks))
    if st != RFD_ERR_CAPACITY:
        _check(st)
    out = np.zeros(blocks.value, np.uint8)
    _check(L.rfd_debug_jpeg_block_counts(addr, n, int(denom), out.ctypes.data, blocks.value, C.byref(blocks)))
    return out


def jpeg_coefficients(data):
    """the dequantised coefficients of every block of a JPEG file, [blocks, 64] i16 in natural order, blocks component-major
    over planes padded to whole MCUs (rfd_debug_jpeg_coefficients; host only, no GPU): the input of the inverse DCT"""
    keep, addr, n = _byte_buffer(data)
    L, blocks = load_library(), C.c_size_t(0)
    st = L.rfd_debug_jpeg_coefficients(addr, n, None, 0, C.byref(blocks))
    if st != RFD_ERR_CAPACITY:
        _check(st)
    out = np.zeros((blocks.value, 64), np.int16)
    _check(L.rfd_debug_jpeg_coefficients(addr, n, out.ctypes.data, blocks.value, C.byref(blocks)))
    return out


def jpeg_intervals(data):
    """the restart intervals of a JPEG file as the marker pre-scan finds them (rfd_debug_jpeg_intervals; host only, no GPU) ->
    [(begin, end)] byte positions in the file.  A file that is not eligible for device entropy decoding raises RfdError with
    RFD_ERR_UNSUPPORTED and the reason."""
    keep, addr, n = _byte_buffer(data)
    L, count = load_library(), C.c_size_t(0)
    st = L.rfd_debug_jpeg_intervals(addr, n, None, None, 0, C.byref(count))
    if st != RFD_ERR_CAPACITY:
        _check(st)
    begin, end = np.zeros(count.value, np.uint32), np.zeros(count.value, np.uint32)
    _check(L.rfd_debug_jpeg_intervals(addr, n, begin.ctypes.data, end.ctypes.data, count.value, C.byref(count)))
    return list(zip(begin.tolist(), end.tolist()))


def jpeg_encode_config(quality=None, sampling=None, restart_rows=None):
    """rfd_jpeg_encode_config: the library's default (90, 4:2:0, 1) with the given fields replaced; sampling a JPEG_* value"""
    c = rfd_jpeg_encode_config()
    _check(load_library().rfd_jpeg_encode_config_default(C.byref(c)))
    for k, v in (("quality", quality), ("sampling", sampling), ("restart_rows", restart_rows)):
        if v is not None:
            setattr(c, k, int(v))
    return c


def jpeg_encode_bound(width, height, cfg=None):
    """a size no file of this geometry can exceed (rfd_jpeg_encode_bound; host only, no GPU)"""
    cfg = cfg or jpeg_encode_config()
    n = C.c_size_t(0)
    _check(load_library().rfd_jpeg_encode_bound(int(width), int(height), C.byref(cfg), C.byref(n)))
    return n.value


def jpeg_encode_header(width, height, cfg=None):
    """the bytes of the file up to and including SOS (rfd_jpeg_encode_header; host only, no GPU)"""
    cfg = cfg or jpeg_encode_config()
    buf, n = (C.c_uint8 * 1024)(), C.c_size_t(0)
    _check(load_library().rfd_jpeg_encode_header(int(width), int(height), C.byref(cfg), buf, 1024, C.byref(n)))
    return bytes(buf[:n.value])


def op_kernels_static(backbone, image_w, image_h, n, op, co_running=True, tile=0, schedule=SCHEDULE_THROUGHPUT, cus=256):
    """debug_op_kernels without a context or a GPU: the kernel(s) a context of this backbone and image size would run op `op` of a
    chain of n images with, under forced tile `tile`, on a GPU of `cus` compute units"""
    buf = C.create_string_buffer(512)
    _check(load_library().rfd_debug_op_kernels_static(backbone, image_w, image_h, n, op, 1 if co_running else 0, tile, schedule, cus, buf, 512))
    return buf.value.decode().split(" + ")


def head_shapes(n, net_h, net_w):
    """Shapes of the 9 head tensors (the reference's Triton output contract,
    face_detection.rs:286-312): per level 32,16,8: cls [n,2A,h,w], bbox [n,4A,h,w], lmk [n,10A,h,w]."""
    out = []
    for s in STRIDES:
        h, w = net_h // s, net_w // s
        out += [(n, 2 * NUM_ANCHORS, h, w), (n, 4 * NUM_ANCHORS, h, w), (n, 10 * NUM_ANCHORS, h, w)]
    return out


class Graph:
    """Host-only description of the build-defined network graph (no GPU needed)."""

    def __init__(self, backbone=BACKBONE_R50, image_w=640, image_h=640):
        self._L = load_library()
        self._g = C.c_void_p()
        _check(self._L.rfd_graph_create(backbone, image_w, image_h, C.byref(self._g)))
        n = [C.c_int() for _ in range(4)]
        _check(self._L.rfd_graph_counts(self._g, *[C.byref(x) for x in n]))
        self.num_layers, self.num_ops, self.num_tensors, self.num_buffers = [x.value for x in n]
        self.layers, self.ops, self.tensors = [], [], []
        for i in range(self.num_layers):
            d = rfd_layer_desc()
            _check(self._L.rfd_graph_layer(self._g, i, C.byref(d)))
            self.layers.append(d)
        for i in range(self.num_ops):
            d = rfd_op_desc()
            _check(self._L.rfd_graph_op(self._g, i, C.byref(d)))
            self.ops.append(d)
        for i in range(self.num_tensors):
            d = rfd_tensor_desc()
            _check(self._L.rfd_graph_tensor(self._g, i, C.byref(d)))
            self.tensors.append(d)
        self.macs = self._L.rfd_graph_macs(self._g)
        self.workspace_bytes = self._L.rfd_graph_workspace_bytes(self._g)

    def __del__(self):
        if getattr(self, "_g", None):
            self._L.rfd_graph_destroy(self._g)
            self._g = None


class FaceDetectionConfig:
    """Mirror of FaceDetectionConfig::new (src/pipeline/face_pipeline/config.rs:23-32)."""

    def __init__(self):
        self.model_name = "face_detection_retina"
        self.image_size = (640, 640)     # (w, h)
        self.max_batch_size = 1
        self.confidence_threshold = 0.7
        self.iou_threshold = 0.45
        self.timeout = 20


class Gallery:
    """The enrolled embeddings of one detector in HBM (rfd.h, "gallery"): rows of `dim` values stored as bf16, searched by one
    pass per 32 queries.  Obtained from RetinaFaceDetection.gallery(); close it before the detector."""

    def __init__(self, det, dim, capacity, _load=None):
        self._L, self._det, self._g = det._L, det, C.c_void_p()
        if _load is None:
            _check(self._L.rfd_gallery_create(det._ctx, int(dim), int(capacity), C.byref(self._g)))
        else:   # RetinaFaceDetection.load_gallery
            _check(self._L.rfd_gallery_load(det._ctx, os.fsencode(_load), int(capacity), C.byref(self._g)))
            cap, d = C.c_int(), C.c_int()
            _check(self._L.rfd_gallery_size(self._g, None, C.byref(cap), C.byref(d)))
            dim, capacity = d.value, cap.value
        self.dim, self.capacity = int(dim), int(capacity)

    def close(self):
        if getattr(self, "_g", None) and getattr(self._det, "_ctx", None):
            self._L.rfd_gallery_destroy(self._g)
        self._g = None

    def __del__(self):
        self.close()

    def size(self):
        """rows enrolled so far"""
        rows = C.c_int()
        _check(self._L.rfd_gallery_size(self._g, C.byref(rows), None, None))
        return rows.value

    def clear(self):
        _check(self._L.rfd_gallery_clear(self._g))

    def _rows2d(self, x):
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2 and x.shape[1] == self.dim, "expected [n, %d], got %s" % (self.dim, x.shape)
        return x

    def add(self, emb):
        """emb [n, dim] f32 (unit vectors) -> the row the first one got; the others follow it"""
        x, first = self._rows2d(emb), C.c_int()
        _check(self._L.rfd_gallery_add(self._g, x.ctypes.data, x.shape[0], C.byref(first)))
        return first.value

    def add_device(self, emb_ptr, n):
        """the same from a raw device address ([n, dim] f32, 16-byte aligned); enqueued on the detector's stream, no synchronisation"""
        first = C.c_int()
        _check(self._L.rfd_gallery_add_device(self._g, emb_ptr, int(n), C.byref(first)))
        return first.value

    @staticmethod
    def _row_list(rows):
        return np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1), np.int32)

    def remove(self, rows):
        """rows (a list, duplicates allowed) are erased and never found again; their numbers are not reused by add"""
        r = self._row_list(rows)
        _check(self._L.rfd_gallery_remove(self._g, r.ctypes.data, r.shape[0]))

    def replace(self, rows, emb):
        """row rows[i] takes emb[i] ([n, dim] f32) and is live afterwards, whether it was live or removed; rows must be distinct"""
        r, x = self._row_list(rows), self._rows2d(emb)
        assert r.shape[0] == x.shape[0], "one row number per embedding"
        _check(self._L.rfd_gallery_replace(self._g, r.ctypes.data, x.ctypes.data, r.shape[0]))

    def replace_device(self, rows, emb_ptr):
        """the same with emb at a raw device address ([len(rows), dim] f32, 16-byte aligned); the row list stays on the host;
        enqueued on the detector's stream, no synchronisation"""
        r = self._row_list(rows)
        _check(self._L.rfd_gallery_replace_device(self._g, r.ctypes.data, emb_ptr, r.shape[0]))

    def live(self):
        """rows enrolled and not removed"""
        n = C.c_int()
        _check(self._L.rfd_gallery_live(self._g, C.byref(n)))
        return n.value

    def removed(self):
        """the removed rows, ascending (i32 array)"""
        n = C.c_int()
        _check(self._L.rfd_gallery_removed(self._g, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        _check(self._L.rfd_gallery_removed(self._g, out.ctypes.data, n.value, C.byref(n)))
        return out

    def save(self, path):
        """writes the gallery to `path` (rfd_gallery_save: synchronises, writes path + ".tmp", renames)"""
        _check(self._L.rfd_gallery_save(self._g, os.fsencode(path)))

    def rows(self, row0, n):
        """the stored (bf16) values of rows [row0, row0 + n) as f32 [n, dim]; a removed row reads as zeros"""
        out = np.zeros((int(n), self.dim), np.float32)
        _check(self._L.rfd_gallery_get_rows(self._g, int(row0), int(n), out.ctypes.data))
        return out

    def search(self, queries, k):
        """queries [n, dim] f32 -> (scores [n, k] f32, rows [n, k] i32): the k best rows of every query, score descending, equal
        scores by ascending row; (-inf, -1) where the gallery has fewer than k rows"""
        x = self._rows2d(queries)
        shape = (x.shape[0], max(int(k), 0))
        scores, rows = np.zeros(shape, np.float32), np.zeros(shape, np.int32)
        _check(self._L.rfd_gallery_search(self._g, x.ctypes.data, x.shape[0], int(k), scores.ctypes.data, rows.ctypes.data))
        return scores, rows

    def search_device(self, queries_ptr, n, k, scores_ptr, rows_ptr, async_=False):
        """the same on raw device addresses (torch tensors' data_ptr()); enqueued on the detector's stream, with no host
        synchronisation when async_ is set (then det.sync() before reading)"""
        _check(self._L.rfd_gallery_search_device(self._g, queries_ptr, int(n), int(k), scores_ptr, rows_ptr, int(async_)))

    def set_identities(self, rows, ids):
        """row rows[i] (live, distinct) gets the identity ids[i] (>= 0, or NO_IDENTITY to unlabel it); enqueued on the detector's
        stream, no synchronisation (rfd.h, "identities")"""
        r, i = self._row_list(rows), self._row_list(ids)
        assert r.shape[0] == i.shape[0], "one identity per row"
        _check(self._L.rfd_gallery_set_identities(self._g, r.ctypes.data, i.ctypes.data, r.shape[0]))

    def identities(self, row0, n):
        """the identities of rows [row0, row0 + n) (i32 array; NO_IDENTITY for unlabelled and removed rows)"""
        out = np.zeros(int(n), np.int32)
        _check(self._L.rfd_gallery_get_identities(self._g, int(row0), int(n), out.ctypes.data))
        return out

    def labelled(self):
        """live rows that carry an identity >= 0"""
        n = C.c_int()
        _check(self._L.rfd_gallery_identities(self._g, C.byref(n)))
        return n.value

    def search_identities(self, queries, k, min_score=-np.inf):
        """queries [n, dim] f32 -> (scores [n, k] f32, rows [n, k] i32, ids [n, k] i32): the k best identities of every query,
        each under its best live row (an unlabelled row is an identity of its own); entries with not score >= min_score and the
        tail beyond the gallery's identities are (-inf, -1, -1)"""
        x = self._rows2d(queries)
        shape = (x.shape[0], max(int(k), 0))
        scores, rows, ids = np.zeros(shape, np.float32), np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        _check(self._L.rfd_gallery_search_identities(self._g, x.ctypes.data, x.shape[0], int(k), float(min_score), scores.ctypes.data, rows.ctypes.data,
                                                     ids.ctypes.data))
        return scores, rows, ids

    def search_identities_device(self, queries_ptr, n, k, min_score, scores_ptr, rows_ptr, ids_ptr, async_=False):
        """the same on raw device addresses, by the conventions of search_device"""
        _check(self._L.rfd_gallery_search_identities_device(self._g, queries_ptr, int(n), int(k), float(min_score), scores_ptr, rows_ptr, ids_ptr,
                                                            int(async_)))

    @staticmethod
    def _tag_list(x):
        return np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1) & 0xFFFFFFFF, np.uint32)

    def set_tags(self, rows, tags):
        """row rows[i] (live, distinct) gets the tag tags[i], any 32-bit value; enqueued on the detector's stream, no
        synchronisation (rfd.h, "tags")"""
        r, t = self._row_list(rows), self._tag_list(tags)
        assert r.shape[0] == t.shape[0], "one tag per row"
        _check(self._L.rfd_gallery_set_tags(self._g, r.ctypes.data, t.ctypes.data, r.shape[0]))

    def tags(self, row0, n):
        """the tags of rows [row0, row0 + n) (u32 array; 0 for a row that never got one and for a removed row)"""
        out = np.zeros(int(n), np.uint32)
        _check(self._L.rfd_gallery_get_tags(self._g, int(row0), int(n), out.ctypes.data))
        return out

    def search_filtered(self, queries, k, mask, value, min_score=-np.inf):
        """search_identities among the rows r with (tag[r] & mask[q]) == value[q] for query q (mask, value: one u32 per query) ->
        (scores [n, k] f32, rows [n, k] i32, ids [n, k] i32); ids is -1 throughout on a gallery without identities"""
        x, m, v = self._rows2d(queries), self._tag_list(mask), self._tag_list(value)
        assert m.shape[0] == v.shape[0] == x.shape[0], "one mask and one value per query"
        shape = (x.shape[0], max(int(k), 0))
        scores, rows, ids = np.zeros(shape, np.float32), np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        _check(self._L.rfd_gallery_search_filtered(self._g, x.ctypes.data, x.shape[0], int(k), float(min_score), m.ctypes.data, v.ctypes.data,
                                                   scores.ctypes.data, rows.ctypes.data, ids.ctypes.data))
        return scores, rows, ids

    def search_filtered_device(self, queries_ptr, n, k, min_score, mask_ptr, value_ptr, scores_ptr, rows_ptr, ids_ptr, async_=False):
        """the same on raw device addresses (mask, value: u32 [n] each), by the conventions of search_device"""
        _check(self._L.rfd_gallery_search_filtered_device(self._g, queries_ptr, int(n), int(k), float(min_score), mask_ptr, value_ptr, scores_ptr, rows_ptr,
                                                          ids_ptr, int(async_)))

    def _nearest_config(self, mode, min_score, tag_mask):
        cfg = rfd_gallery_nearest_config()
        self._L.rfd_gallery_nearest_config_default(C.byref(cfg))
        cfg.mode, cfg.min_score, cfg.tag_mask = int(mode), float(min_score), int(tag_mask) & 0xFFFFFFFF
        return cfg

    def nearest(self, row0, n, mode=NEAREST_OTHER_ROW, min_score=-np.inf, tag_mask=0):
        """for every row a of [row0, row0 + n): the best live row b != a (mode NEAREST_OTHER_IDENTITY: of another identity) with
        (tag[a] & tag_mask) == (tag[b] & tag_mask) -> (scores [n] f32, rows [n] i32, ids [n] i32); (-inf, -1, -1) where a is
        removed or nothing reaches min_score (rfd.h, "nearest")"""
        n = int(n)
        scores, rows, ids = np.zeros(max(n, 0), np.float32), np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int32)
        cfg = self._nearest_config(mode, min_score, tag_mask)
        _check(self._L.rfd_gallery_nearest(self._g, int(row0), n, C.byref(cfg), scores.ctypes.data, rows.ctypes.data, ids.ctypes.data))
        return scores, rows, ids

    def nearest_device(self, row0, n, scores_ptr, rows_ptr, ids_ptr, mode=NEAREST_OTHER_ROW, min_score=-np.inf, tag_mask=0, async_=False):
        """the same into raw device addresses ([n] each, 4-byte aligned; ids_ptr may be None), by the conventions of search_device"""
        cfg = self._nearest_config(mode, min_score, tag_mask)
        _check(self._L.rfd_gallery_nearest_device(self._g, int(row0), int(n), C.byref(cfg), scores_ptr, rows_ptr, ids_ptr, int(async_)))


TRACK_NEW, TRACK_CONFIRMED, TRACK_DUE = 1, 2, 4   # RFD_TRACK_*: the flags of a tracked row
TRACKER_MAX_DET = 8192                            # RFD_TRACKER_MAX_DET


def tracker_config(det, **fields):
    """rfd_tracker_config: the default of a detector (1 stream, 64 slots, iou_min 0.3, max_missed 5, both scores = its confidence
    threshold, min_hits 2, improve 1.1 -- chosen values, not tuned on data) with the given fields replaced"""
    c = rfd_tracker_config()
    _check(load_library().rfd_tracker_config_default(det._ctx, C.byref(c)))
    for k, v in fields.items():
        if k not in dict(rfd_tracker_config._fields_) or k == "reserved":
            raise TypeError("rfd_tracker_config has no field %r" % k)
        setattr(c, k, v)
    return c


class TrackOut:
    """The host arrays of an rfd_track_out for n frames: track / flags [n, max_det], stats [n, 4] (matched, born, ended,
    dropped), ended [n, max_tracks], the due slab (boxes [n, max_det, 5], landmarks [n, max_det, 5, 2], count / total [n]) and
    due_track [n, max_det].  The library writes the rows below each frame's counts only; whatever the arrays held beyond them
    stays (fill: the byte they start with)."""

    def __init__(self, n, max_det, max_tracks, fill=0, want_due=True):
        new = lambda shape, dt: np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()
        self.track, self.flags = new((n, max_det), np.int32), new((n, max_det), np.uint32)
        self.stats, self.ended = new((n, 4), np.int32), new((n, max_tracks), np.int32)
        self.due_boxes = new((n, max_det, 5), np.float32) if want_due else None
        self.due_landmarks = new((n, max_det, 5, 2), np.float32) if want_due else None
        self.due_count = new((n,), np.int32) if want_due else None
        self.due_total = new((n,), np.int32) if want_due else None
        self.due_track = new((n, max_det), np.int32)

    def arrays(self):
        return [(k, v) for k, v in sorted(vars(self).items()) if v is not None]

    def struct(self):
        p = lambda a: None if a is None else a.ctypes.data
        return rfd_track_out(p(self.track), p(self.flags), p(self.stats), p(self.ended),
                             rfd_dets(p(self.due_boxes), p(self.due_landmarks), p(self.due_count), p(self.due_total)), p(self.due_track))


class Tracker:
    """Faces followed over the frames of video streams, in HBM (rfd.h, "tracker").  Obtained from RetinaFaceDetection.tracker();
    close it before the detector."""

    def __init__(self, det, cfg=None):
        self._L, self._det, self._t = det._L, det, C.c_void_p()
        self.cfg = cfg if cfg is not None else tracker_config(det)
        _check(self._L.rfd_tracker_create(det._ctx, C.byref(self.cfg), C.byref(self._t)))

    def close(self):
        if getattr(self, "_t", None) and getattr(self._det, "_ctx", None):
            self._L.rfd_tracker_destroy(self._t)
        self._t = None

    def __del__(self):
        self.close()

    @staticmethod
    def _streams(streams):
        return np.ascontiguousarray(np.asarray(streams, np.int64).reshape(-1), np.int32)

    def update(self, streams, boxes, landmarks, count, quality=None, out=None):
        """the host form: streams [n]; boxes [n, max_det, 5], landmarks [n, max_det, 5, 2], count [n] as the detect calls fill
        them; quality [n, max_det] or None -> TrackOut (out: a caller-made one to write into)"""
        s = self._streams(streams)
        n, md = len(s), self._det.max_det
        b = np.ascontiguousarray(boxes, np.float32).reshape(n, md, 5)
        l = np.ascontiguousarray(landmarks, np.float32).reshape(n, md, 10)
        c = np.ascontiguousarray(count, np.int32).reshape(n)
        q = None if quality is None else np.ascontiguousarray(quality, np.float32).reshape(n, md)
        if out is None:
            out = TrackOut(n, md, self.cfg.max_tracks)
        d = rfd_dets(b.ctypes.data, l.ctypes.data, c.ctypes.data, None)
        st = out.struct()
        _check(self._L.rfd_tracker_update(self._t, s.ctypes.data, C.byref(d), None if q is None else q.ctypes.data, n, C.byref(st)))
        return out

    def update_device(self, streams, boxes_ptr, landmarks_ptr, count_ptr, out, quality_ptr=None, async_=False):
        """the same from raw device addresses; out: an rfd_track_out of device addresses.  Enqueued on the detector's stream,
        with no host synchronisation when async_ is set"""
        s = self._streams(streams)
        d = rfd_dets(boxes_ptr, landmarks_ptr, count_ptr, None)
        _check(self._L.rfd_tracker_update_device(self._t, s.ctypes.data, C.byref(d), quality_ptr, len(s), C.byref(out), int(async_)))

    def reset(self, stream=-1):
        """the tracks of a stream (-1: of all) vanish without an ended entry; serials go on from where they were"""
        _check(self._L.rfd_tracker_reset(self._t, int(stream)))

    def tracks(self, stream):
        """the live slots of a stream in ascending slot order, as rfd_track structures (waits for the stream)"""
        n = C.c_int(0)
        _check(self._L.rfd_tracker_get_tracks(self._t, int(stream), None, 0, C.byref(n)))
        arr = (rfd_track * max(n.value, 1))()
        _check(self._L.rfd_tracker_get_tracks(self._t, int(stream), arr, n.value, C.byref(n)))
        return list(arr[:n.value])

    # ---- track identities (rfd.h, "track identities") ----
    def enable_identities(self, cfg=None, **fields):
        """rfd_tracker_identity_enable, once per tracker: cfg, or the default (dim 512, accept 0.5, release 0.4, margin 0.05 --
        chosen values, not tuned on data) with `fields` replaced"""
        self.identity_cfg = cfg if cfg is not None else track_identity_config(**fields)
        _check(self._L.rfd_tracker_identity_enable(self._t, C.byref(self.identity_cfg)))
        return self.identity_cfg

    def _obs(self, n, first, row, serial, total):
        """the host arrays of an rfd_track_obs (kept alive by the caller of this) and the struct over them"""
        f = np.ascontiguousarray(first, np.int32).reshape(n + 1)
        r = np.ascontiguousarray(row, np.int32).reshape(-1)
        s = np.ascontiguousarray(serial, np.int32).reshape(n, self._det.max_det)
        t = None if total is None else np.ascontiguousarray(total, np.int32).reshape(1)
        return (f, r, s, t), rfd_track_obs(None if t is None else t.ctypes.data, f.ctypes.data, r.ctypes.data, s.ctypes.data), len(r)

    def fuse(self, streams, first, row, serial, emb, weight=None, total=None, query=None, status=None):
        """the host form of rfd_tracker_fuse: streams [n]; first [n + 1], row [m], total (an int or None) as a FaceList holds them,
        serial [n, max_det] as TrackOut.due_track; emb [m, dim]; weight [m] or None -> (query [m, dim] f32, status [m] int32).
        query / status: caller-made arrays to write into (rows at or past the count keep what they hold)"""
        s = self._streams(streams)
        keep, obs, m = self._obs(len(s), first, row, serial, total)
        dim = self.identity_cfg.dim
        e = np.ascontiguousarray(emb, np.float32).reshape(m, dim)
        w = None if weight is None else np.ascontiguousarray(weight, np.float32).reshape(m)
        query = np.zeros((m, dim), np.float32) if query is None else query
        status = np.zeros(m, np.int32) if status is None else status
        assert query.dtype == np.float32 and query.shape == (m, dim) and query.flags.c_contiguous
        assert status.dtype == np.int32 and status.shape == (m,) and status.flags.c_contiguous
        _check(self._L.rfd_tracker_fuse(self._t, s.ctypes.data, len(s), C.byref(obs), m, e.ctypes.data, None if w is None else w.ctypes.data,
                                        query.ctypes.data, status.ctypes.data))
        return query, status

    def fuse_device(self, streams, obs, m, emb_ptr, query_ptr, status_ptr, weight_ptr=None, async_=False):
        """the same from raw device addresses; obs: an rfd_track_obs of device addresses.  Enqueued on the detector's stream, with
        no host synchronisation when async_ is set"""
        s = self._streams(streams)
        _check(self._L.rfd_tracker_fuse_device(self._t, s.ctypes.data, len(s), C.byref(obs), int(m), emb_ptr, weight_ptr, query_ptr, status_ptr,
                                               int(async_)))

    def label(self, streams, first, row, serial, scores, rows, ids, status, total=None):
        """the host form of rfd_tracker_label: the observations as in fuse; scores / rows / ids [m, k] as the gallery's identity
        search wrote them for fuse's query (ids may be None); status: fuse's"""
        s = self._streams(streams)
        keep, obs, m = self._obs(len(s), first, row, serial, total)
        sc = np.ascontiguousarray(scores, np.float32)
        assert sc.ndim == 2 and sc.shape[0] == m, "scores is [m, k]"
        k = sc.shape[1]
        rw = np.ascontiguousarray(rows, np.int32).reshape(m, k)
        idn = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(m, k)
        st = np.ascontiguousarray(status, np.int32).reshape(m)
        _check(self._L.rfd_tracker_label(self._t, s.ctypes.data, len(s), C.byref(obs), m, k, sc.ctypes.data, rw.ctypes.data,
                                         None if idn is None else idn.ctypes.data, st.ctypes.data))

    def label_device(self, streams, obs, m, k, scores_ptr, rows_ptr, ids_ptr, status_ptr, async_=False):
        """the same from raw device addresses, by the conventions of fuse_device"""
        s = self._streams(streams)
        _check(self._L.rfd_tracker_label_device(self._t, s.ctypes.data, len(s), C.byref(obs), int(m), int(k), scores_ptr, rows_ptr, ids_ptr,
                                                status_ptr, int(async_)))

    def who(self, streams, track, count, flags=None, who=None, identity=None, id_score=None):
        """the host form of rfd_tracker_who: track [n, max_det] and count [n] as TrackOut holds them; flags [n, max_det] uint32 or
        None -> (who, identity, id_score), each [n, max_det].  who / identity / id_score: caller-made arrays to write into (rows at
        or past a frame's count keep what they hold); who may be `flags` itself"""
        s = self._streams(streams)
        n, md = len(s), self._det.max_det
        tr = np.ascontiguousarray(track, np.int32).reshape(n, md)
        c = np.ascontiguousarray(count, np.int32).reshape(n)
        who = np.zeros((n, md), np.uint32) if who is None else who
        identity = np.zeros((n, md), np.int32) if identity is None else identity
        id_score = np.zeros((n, md), np.float32) if id_score is None else id_score
        fl = None if flags is None else (flags if flags is who else np.ascontiguousarray(flags, np.uint32).reshape(n, md))
        for a, dt in ((who, np.uint32), (identity, np.int32), (id_score, np.float32)):
            assert a.dtype == dt and a.shape == (n, md) and a.flags.c_contiguous
        _check(self._L.rfd_tracker_who(self._t, s.ctypes.data, n, tr.ctypes.data, c.ctypes.data, None if fl is None else fl.ctypes.data,
                                       who.ctypes.data, identity.ctypes.data, id_score.ctypes.data))
        return who, identity, id_score

    def who_device(self, streams, track_ptr, count_ptr, who_ptr, flags_ptr=None, identity_ptr=None, id_score_ptr=None, async_=False):
        """the same from raw device addresses; who_ptr may equal flags_ptr"""
        s = self._streams(streams)
        _check(self._L.rfd_tracker_who_device(self._t, s.ctypes.data, len(s), track_ptr, count_ptr, flags_ptr, who_ptr, identity_ptr,
                                              id_score_ptr, int(async_)))

    def identities(self, stream):
        """the entries of the live, fused tracks of a stream in ascending slot order, as rfd_track_identity structures (waits for
        the stream)"""
        n = C.c_int(0)
        _check(self._L.rfd_tracker_get_identities(self._t, int(stream), None, 0, C.byref(n)))
        arr = (rfd_track_identity * max(n.value, 1))()
        _check(self._L.rfd_tracker_get_identities(self._t, int(stream), arr, n.value, C.byref(n)))
        return list(arr[:n.value])

    def template(self, stream, serial):
        """the template S [dim] f32 of a live, fused track (waits for the stream); an unknown serial raises"""
        out = np.zeros(self.identity_cfg.dim, np.float32)
        _check(self._L.rfd_tracker_get_template(self._t, int(stream), int(serial), out.ctypes.data))
        return out


    # ---- track shots (rfd.h, "track shots") ----
    def enable_shots(self, cfg=None, **fields):
        """rfd_tracker_shots_enable, once per tracker: cfg, or the default (112 x 112 crops) with `fields` replaced"""
        self.shot_cfg = cfg if cfg is not None else track_shot_config(**fields)
        _check(self._L.rfd_tracker_shots_enable(self._t, C.byref(self.shot_cfg)))
        return self.shot_cfg

    @staticmethod
    def _stamps(stamp, n):
        return None if stamp is None else np.ascontiguousarray(stamp, np.int64).reshape(n)

    def keep_shots(self, streams, first, row, serial, crops, stamp=None, face_status=None, q=None, total=None, status=None):
        """the host form of rfd_tracker_keep_shots: streams [n]; stamp [n] int64 or None; first [n + 1], row [m], total (an int or
        None) as a FaceList holds them, serial [n, max_det] as TrackOut.due_track; crops [m, crop_h, crop_w, 3] uint8; face_status
        [m] int32 or None; q [m] f32 or None -> status [m] int32.  status: a caller-made array to write into (rows at or past the
        count keep what they hold)"""
        s = self._streams(streams)
        keep, obs, m = self._obs(len(s), first, row, serial, total)
        st = self._stamps(stamp, len(s))
        c = np.ascontiguousarray(crops, np.uint8).reshape(m, self.shot_cfg.crop_h, self.shot_cfg.crop_w, 3)
        fs = None if face_status is None else np.ascontiguousarray(face_status, np.int32).reshape(m)
        qq = None if q is None else np.ascontiguousarray(q, np.float32).reshape(m)
        status = np.zeros(m, np.int32) if status is None else status
        assert status.dtype == np.int32 and status.shape == (m,) and status.flags.c_contiguous
        p = lambda a: None if a is None else a.ctypes.data
        _check(self._L.rfd_tracker_keep_shots(self._t, s.ctypes.data, p(st), len(s), C.byref(obs), m, c.ctypes.data, p(fs), p(qq),
                                              status.ctypes.data))
        return status

    def keep_shots_device(self, streams, obs, m, crops_ptr, status_ptr, stamp=None, face_status_ptr=None, q_ptr=None, async_=False):
        """the same from raw device addresses; obs: an rfd_track_obs of device addresses.  Enqueued on the detector's stream, with
        no host synchronisation when async_ is set"""
        s = self._streams(streams)
        st = self._stamps(stamp, len(s))
        _check(self._L.rfd_tracker_keep_shots_device(self._t, s.ctypes.data, None if st is None else st.ctypes.data, len(s), C.byref(obs),
                                                     int(m), crops_ptr, face_status_ptr, q_ptr, status_ptr, int(async_)))

    def collect_ended(self, streams, stats, ended, cap, stamp=None, total=None, first=None, rec=None, crops=None, with_crops=True):
        """the host form of rfd_tracker_collect_ended: stats [n, 4] and ended [n, max_tracks] as TrackOut holds them -> (total [1]
        int32, first [n + 1] int32, rec: a ctypes array of cap rfd_track_record, crops [cap, crop_h, crop_w, 3] uint8 or None).
        total / first / rec / crops: caller-made ones to write into (rows at or past min(total, cap) keep what they hold); rec may
        also be a numpy array of cap 80-byte items"""
        s = self._streams(streams)
        n, cap = len(s), int(cap)
        st = self._stamps(stamp, n)
        sa = np.ascontiguousarray(stats, np.int32).reshape(n, 4)
        en = np.ascontiguousarray(ended, np.int32).reshape(n, self.cfg.max_tracks)
        total = np.zeros(1, np.int32) if total is None else total
        first = np.zeros(n + 1, np.int32) if first is None else first
        rec = (rfd_track_record * max(cap, 1))() if rec is None else rec
        if crops is None and with_crops:
            crops = np.zeros((max(cap, 1), self.shot_cfg.crop_h, self.shot_cfg.crop_w, 3), np.uint8)
        rec_ptr = rec.ctypes.data if isinstance(rec, np.ndarray) else C.addressof(rec)
        out = rfd_track_records(total.ctypes.data, first.ctypes.data, rec_ptr, None if crops is None else crops.ctypes.data)
        _check(self._L.rfd_tracker_collect_ended(self._t, s.ctypes.data, None if st is None else st.ctypes.data, n, sa.ctypes.data,
                                                 en.ctypes.data, cap, C.byref(out)))
        return total, first, rec, crops

    def collect_ended_device(self, streams, stats_ptr, ended_ptr, cap, out, stamp=None, async_=False):
        """the same from raw device addresses; out: an rfd_track_records of device addresses"""
        s = self._streams(streams)
        st = self._stamps(stamp, len(s))
        _check(self._L.rfd_tracker_collect_ended_device(self._t, s.ctypes.data, None if st is None else st.ctypes.data, len(s), stats_ptr,
                                                        ended_ptr, int(cap), C.byref(out), int(async_)))

    def shots(self, stream):
        """the entries of the live tracks of a stream that have a kept shot, in ascending slot order, as rfd_track_shot structures
        (waits for the stream)"""
        n = C.c_int(0)
        _check(self._L.rfd_tracker_get_shots(self._t, int(stream), None, 0, C.byref(n)))
        arr = (rfd_track_shot * max(n.value, 1))()
        _check(self._L.rfd_tracker_get_shots(self._t, int(stream), arr, n.value, C.byref(n)))
        return list(arr[:n.value])

    def shot_crop(self, stream, serial):
        """the stored crop [crop_h, crop_w, 3] uint8 of a live track (waits for the stream); an unknown serial raises"""
        out = np.zeros((self.shot_cfg.crop_h, self.shot_cfg.crop_w, 3), np.uint8)
        _check(self._L.rfd_tracker_get_shot_crop(self._t, int(stream), int(serial), out.ctypes.data))
        return out


TRACK_SHOT_KEPT, TRACK_SHOT_NO_TRACK, TRACK_SHOT_BAD_INPUT, TRACK_SHOT_PASSED = 0, 1, 2, 3   # RFD_TRACK_SHOT_*: keep's status


def track_shot_config(**fields):
    """rfd_track_shot_config: the default (112 x 112 crops) with the given fields replaced"""
    c = rfd_track_shot_config()
    _check(load_library().rfd_track_shot_config_default(C.byref(c)))
    for k, v in fields.items():
        if k not in dict(rfd_track_shot_config._fields_) or k == "reserved":
            raise TypeError("rfd_track_shot_config has no field %r" % k)
        setattr(c, k, v)
    return c


TRACK_NAMED = 8                                   # RFD_TRACK_NAMED: the bit rfd_tracker_who adds to a row's flags
TRACK_FUSE_OK, TRACK_FUSE_NO_TRACK, TRACK_FUSE_BAD_INPUT, TRACK_FUSE_OVERFLOW = 0, 1, 2, 3   # RFD_TRACK_FUSE_*: fuse's status


def track_identity_config(**fields):
    """rfd_track_identity_config: the default (dim 512, accept 0.5, release 0.4, margin 0.05 -- chosen values, not tuned on
    data) with the given fields replaced"""
    c = rfd_track_identity_config()
    _check(load_library().rfd_track_identity_config_default(C.byref(c)))
    for k, v in fields.items():
        if k not in dict(rfd_track_identity_config._fields_) or k == "reserved":
            raise TypeError("rfd_track_identity_config has no field %r" % k)
        setattr(c, k, v)
    return c


SHOT_QUALITY_PARTS = 8           # RFD_SHOT_QUALITY_PARTS: sharp, mean, expo, yaw, roll, pitch, pose, size
SHOT_QUALITY_MAX_SIDE = 32768     # RFD_SHOT_QUALITY_MAX_SIDE


def shot_quality_config(**fields):
    """rfd_shot_quality_config: the default (dark 30, bright 225, pitch0 0.495, w_yaw 1, w_roll 1, w_pitch 2, sharp_ref 64,
    size_ref 112, times_score 0 -- chosen values, not tuned on data) with the given fields replaced"""
    c = rfd_shot_quality_config()
    _check(load_library().rfd_shot_quality_config_default(C.byref(c)))
    for k, v in fields.items():
        if k not in dict(rfd_shot_quality_config._fields_) or k == "reserved":
            raise TypeError("rfd_shot_quality_config has no field %r" % k)
        setattr(c, k, v)
    return c


REDACT_FILL, REDACT_PIXELATE = 0, 1   # RFD_REDACT_*: rfd_redact_config.mode
REDACT_RECT, REDACT_ELLIPSE = 0, 1    # rfd_redact_config.shape
REDACT_MAX_SIDE = 32768               # RFD_REDACT_MAX_SIDE


def redact_config(**fields):
    """rfd_redact_config: the default (PIXELATE, ELLIPSE, cell 16, fill 0 0 0, margins 0.1 / 0.2 / 0.1, sel_mask 0, sel_value 0
    -- chosen values, not tuned on data) with the given fields replaced; fill = (B, G, R)"""
    c = rfd_redact_config()
    _check(load_library().rfd_redact_config_default(C.byref(c)))
    for k, v in fields.items():
        if k not in dict(rfd_redact_config._fields_) or k == "reserved":
            raise TypeError("rfd_redact_config has no field %r" % k)
        if k == "fill":
            v = (C.c_uint8 * 4)(*(list(v) + [0] * (4 - len(v))))
        setattr(c, k, v)
    return c


ANNOTATE_NONE, ANNOTATE_ARRAY, ANNOTATE_SCORE = 0, 1, 2   # RFD_ANNOTATE_*: rfd_annotate_config.label_source / value_source
ANNOTATE_MAX_STYLES = 4                                   # RFD_ANNOTATE_MAX_STYLES


def annotate_config(**fields):
    """rfd_annotate_config: the default (one style: every row green; thickness 2, mark_radius 2, label NONE, value SCORE,
    text_scale 2, text black, alpha 256, margins 0 -- chosen values, not tuned on data) with the given fields replaced.
    styles = [(sel_mask, sel_value, (B, G, R)), ...] sets n_styles and style[]; text_colour = (B, G, R)"""
    c = rfd_annotate_config()
    _check(load_library().rfd_annotate_config_default(C.byref(c)))
    for k, v in fields.items():
        if k == "styles":
            if len(v) > ANNOTATE_MAX_STYLES:
                raise TypeError("rfd_annotate_config holds at most %d styles" % ANNOTATE_MAX_STYLES)
            c.n_styles = len(v)
            for i in range(ANNOTATE_MAX_STYLES):
                m, w, col = v[i] if i < len(v) else (0, 0, ())
                c.style[i] = rfd_annotate_style(m, w, (C.c_uint8 * 4)(*(list(col) + [0] * (4 - len(col)))))
            continue
        if k not in dict(rfd_annotate_config._fields_) or k in ("reserved", "style"):
            raise TypeError("rfd_annotate_config has no field %r" % k)
        if k == "text_colour":
            v = (C.c_uint8 * 4)(*(list(v) + [0] * (4 - len(v))))
        setattr(c, k, v)
    return c


def annotate_glyph(glyph):
    """rfd_debug_annotate_glyph: the seven rows (top first, bit 4 = the left column) of glyph 0 .. 13 of the library's font"""
    rows = (C.c_uint8 * 7)()
    _check(load_library().rfd_debug_annotate_glyph(int(glyph), C.byref(rows)))
    return list(rows)


# rfd_pixel_format and rfd_color (rfd.h, "frames in camera and decoder formats")
PIXEL_BGR, PIXEL_RGB, PIXEL_BGRA, PIXEL_RGBA, PIXEL_GRAY, PIXEL_NV12, PIXEL_NV21, PIXEL_I420, PIXEL_YUYV, PIXEL_UYVY = range(10)
COLOR_BT601_LIMITED, COLOR_BT601_FULL, COLOR_BT709_LIMITED, COLOR_BT709_FULL = range(4)
PIXEL_FORMAT_NAMES = ("bgr", "rgb", "bgra", "rgba", "gray", "nv12", "nv21", "i420", "yuyv", "uyvy")


def pixel_format(fmt):
    """a PIXEL_* value from a value or a lower-case name ("nv12")"""
    return PIXEL_FORMAT_NAMES.index(fmt) if isinstance(fmt, str) else int(fmt)


def frame_layout(fmt, w, h):
    """rfd_frame_layout_of -> {"planes", "row_bytes" [planes], "rows" [planes]}: host only, no context"""
    l = rfd_frame_layout()
    _check(load_library().rfd_frame_layout_of(pixel_format(fmt), int(w), int(h), C.byref(l)))
    return {"planes": l.planes, "row_bytes": list(l.row_bytes[:l.planes]), "rows": list(l.rows[:l.planes])}


def frame(fmt, width, height, planes, strides=None, color=COLOR_BT601_LIMITED):
    """an rfd_frame from raw addresses: planes = the address of each plane the format has, strides = their byte strides
    (default: the layout's row_bytes)"""
    f = rfd_frame()
    f.format, f.width, f.height, f.color = pixel_format(fmt), int(width), int(height), int(color)
    if strides is None:
        strides = frame_layout(fmt, width, height)["row_bytes"]
    for k, a in enumerate(planes):
        f.plane[k] = a
        f.stride[k] = int(strides[k])
    return f


class RetinaFaceDetection:
    """Host mirror of the reference's RetinaFaceDetection (face_detection.rs:19-513).

    new(...)  -> __init__   (the Triton client / model config / model name arguments are gone)
    call      -> call       (one HxWx3 u8 BGR frame -> (det [K,5], kps [K,5,2]))
    plus call_batch and the stage-level entry points used by the parity tests.
    """

    def __init__(self, image_size=(640, 640), max_batch_size=1, confidence_threshold=0.7,
                 iou_threshold=0.45, device_id=0, max_det=1024, backbone=BACKBONE_R50, precision=0, schedule=0, max_src=None):
        self._L = load_library()
        cfg = rfd_config()
        self._L.rfd_config_default(C.byref(cfg))
        cfg.image_w, cfg.image_h = int(image_size[0]), int(image_size[1])
        cfg.max_batch_size = int(max_batch_size)
        cfg.confidence_threshold = float(confidence_threshold)
        cfg.iou_threshold = float(iou_threshold)
        cfg.precision = int(precision)   # 0 = bf16 product path, 1 = PRECISION_F32 parity mode (R50 only)
        cfg.schedule = int(schedule)     # 0 = throughput, 1 = SCHEDULE_LATENCY: split-K convolutions for passes of <= LATENCY_MAX_BATCH images
        cfg.device_id = int(device_id)
        cfg.max_det = int(max_det)
        cfg.backbone = int(backbone)
        if max_src is not None:          # (w, h) of the largest source frame: sizes the JPEG decoder's staging (default 3840 x 2160)
            cfg.max_src_w, cfg.max_src_h = int(max_src[0]), int(max_src[1])
        self.cfg = cfg
        self._ctx = C.c_void_p()
        _check(self._L.rfd_create(C.byref(cfg), C.byref(self._ctx)))
        self.image_size = (cfg.image_w, cfg.image_h)
        self.max_det = cfg.max_det
        self._jpeg_apply_orientation = False   # set_jpeg_orientation: decode_jpeg allocates by the oriented size
        self._jpeg_scale = 1                   # set_jpeg_scale: ... and by the scaled size

    def gallery(self, dim=512, capacity=1 << 20):
        """a face gallery on this detector's device and stream (rfd_gallery_create); it is closed with the detector at the latest"""
        g = Gallery(self, dim, capacity)
        self._galleries = getattr(self, "_galleries", []) + [g]
        return g

    def load_gallery(self, path, capacity=0):
        """a gallery read from a file that Gallery.save wrote (rfd_gallery_load); capacity 0 = the file's rows"""
        g = Gallery(self, 0, capacity, _load=path)
        self._galleries = getattr(self, "_galleries", []) + [g]
        return g

    def tracker(self, cfg=None, **fields):
        """a tracker on this detector's device and stream (rfd_tracker_create): cfg, or the default with `fields` replaced; it is
        closed with the detector at the latest"""
        t = Tracker(self, cfg if cfg is not None else tracker_config(self, **fields))
        self._trackers = getattr(self, "_trackers", []) + [t]
        return t

    def close(self):
        for t in getattr(self, "_trackers", []):
            t.close()
        self._trackers = []
        for g in getattr(self, "_galleries", []):
            g.close()
        self._galleries = []
        for p in getattr(self, "_pinned", []):
            self._L.rfd_host_free(p)
        self._pinned = []
        if getattr(self, "_ctx", None):
            self._L.rfd_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    # ---- weights ----
    def init_synthetic_weights(self, seed=1234):
        _check(self._L.rfd_init_synthetic_weights(self._ctx, seed))

    def save_weights(self, path):
        _check(self._L.rfd_save_weights(self._ctx, os.fsencode(path)))

    def load_weights(self, path):
        _check(self._L.rfd_load_weights(self._ctx, os.fsencode(path)))

    def get_layer(self, idx, desc):
        w = np.zeros((desc.cout, desc.kh, desc.kw, desc.cin), np.float32)  # depthwise: cin = 1
        b = np.zeros(desc.cout, np.float32)
        _check(self._L.rfd_get_layer_weights(self._ctx, idx, w.ctypes.data, b.ctypes.data))
        return w, b

    def set_layer(self, idx, w, b):
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        _check(self._L.rfd_set_layer_weights(self._ctx, idx, w.ctypes.data, b.ctypes.data))

    def get_affine(self, idx, cout):
        s = np.zeros(cout, np.float32)
        t = np.zeros(cout, np.float32)
        _check(self._L.rfd_get_layer_affine(self._ctx, idx, s.ctypes.data, t.ctypes.data))
        return s, t

    def set_affine(self, idx, scale, shift):
        s = np.ascontiguousarray(scale, np.float32)
        t = np.ascontiguousarray(shift, np.float32)
        _check(self._L.rfd_set_layer_affine(self._ctx, idx, s.ctypes.data, t.ctypes.data))

    # ---- helpers ----
    @staticmethod
    def _images(frames):
        arr = (rfd_image * len(frames))()
        keep = []
        for i, f in enumerate(frames):
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3):
                raise RfdError(RFD_ERR_INVALID_ARG, "frames must be HxWx3 uint8 arrays (BGR)")
            if f.strides[2] != 1 or f.strides[1] != 3:
                f = np.ascontiguousarray(f)
            keep.append(f)
            arr[i].data = f.ctypes.data
            arr[i].height, arr[i].width = f.shape[0], f.shape[1]
            arr[i].stride = f.strides[0]
        return arr, keep

    def _alloc_dets(self, n):
        md = self.max_det
        boxes = np.zeros((n, md, 5), np.float32)
        lmk = np.zeros((n, md, 5, 2), np.float32)
        count = np.zeros(n, np.int32)
        total = np.zeros(n, np.int32)
        d = rfd_dets(boxes.ctypes.data, lmk.ctypes.data, count.ctypes.data, total.ctypes.data)
        return d, boxes, lmk, count, total

    @staticmethod
    def _split(boxes, lmk, count):
        return [(boxes[i, :count[i]].copy(), lmk[i, :count[i]].copy()) for i in range(len(count))]

    # ---- the hot path ----
    def call_batch(self, frames):
        """Batch form of `call`: list of HxWx3 u8 BGR frames -> list of (det [K,5], kps [K,5,2])."""
        arr, keep = self._images(frames)
        d, boxes, lmk, count, total = self._alloc_dets(len(frames))
        _check(self._L.rfd_detect_batch(self._ctx, arr, len(frames), C.byref(d)))
        self.last_total = total
        return self._split(boxes, lmk, count)

    # ---- pipelined host entry: the PCIe copy of batch i+1 overlaps the compute of batch i ----
    def host_frames(self, n, h, w):
        """n frames of h x w x 3 u8 in page-locked memory (rfd_host_alloc): decode into it, then submit()."""
        p = C.c_void_p()
        _check(self._L.rfd_host_alloc(n * h * w * 3, C.byref(p)))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        buf = (C.c_uint8 * (n * h * w * 3)).from_address(p.value)
        return np.frombuffer(buf, np.uint8).reshape(n, h, w, 3)

    def submit(self, frames):
        arr, keep = self._images(frames)
        self._inflight = getattr(self, "_inflight", [])
        _check(self._L.rfd_submit_batch(self._ctx, arr, len(frames)))
        self._inflight.append((len(frames), keep))  # the frames must outlive the batch

    def collect(self):
        n, _ = self._inflight[0] if getattr(self, "_inflight", None) else (self.cfg.max_batch_size, None)
        d, boxes, lmk, count, total = self._alloc_dets(n)
        got = C.c_int(0)
        _check(self._L.rfd_collect_batch(self._ctx, C.byref(d), C.byref(got)))
        self._inflight.pop(0)
        self.last_total = total
        return self._split(boxes[:got.value], lmk[:got.value], count[:got.value])

    def call(self, image, is_debug=None):
        """RetinaFaceDetection::call (face_detection.rs:496): -> (det [K,5], kps [K,5,2])."""
        return self.call_batch([image])[0]

    def detect_device(self, frame_ptrs, shapes, out_boxes_ptr, out_lmk_ptr, out_count_ptr,
                      out_total_ptr, async_=False):
        """Frames and outputs already in device memory (raw device pointers)."""
        n = len(frame_ptrs)
        arr = (rfd_image * n)()
        for i, (p, (h, w)) in enumerate(zip(frame_ptrs, shapes)):
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = p, h, w, w * 3
        d = rfd_dets(out_boxes_ptr, out_lmk_ptr, out_count_ptr, out_total_ptr)
        _check(self._L.rfd_detect_batch_device(self._ctx, arr, n, C.byref(d), int(async_)))  # 0 sync, 1 async, 2 overlapped

    def sync(self):
        _check(self._L.rfd_sync(self._ctx))

    # ---- JPEG decode on the device (rfd.h, "JPEG decode"): byte_data_to_opencv, utils.rs:8-52 ----
    def set_decode_threads(self, threads):
        """host threads of the entropy decoder, 1..16 (default 4); the pixels do not depend on it"""
        _check(self._L.rfd_set_decode_threads(self._ctx, int(threads)))

    def set_jpeg_entropy(self, mode):
        """"host" (default): Huffman decoding on the host threads; "device": files with a restart interval are entropy-decoded
        by one device thread per interval, every other file as before (rfd.h, "entropy decoding on the device")"""
        modes = {"host": JPEG_ENTROPY_HOST, "device": JPEG_ENTROPY_DEVICE}
        _check(self._L.rfd_set_jpeg_entropy(self._ctx, modes[mode] if mode in modes else int(mode)))

    def set_jpeg_orientation(self, mode):
        """"ignore" (default): frames are written as the file stores them, whatever its EXIF orientation tag says; "apply":
        frames are written upright, in the size jpeg_orientation reports (rfd.h, "EXIF orientation")"""
        modes = {"ignore": JPEG_ORIENTATION_IGNORE, "apply": JPEG_ORIENTATION_APPLY}
        mode = modes[mode] if mode in modes else int(mode)
        _check(self._L.rfd_set_jpeg_orientation(self._ctx, mode))
        self._jpeg_apply_orientation = mode == JPEG_ORIENTATION_APPLY

    def set_jpeg_scale(self, denom):
        """1 (default): frames are written at the stored size; 2, 4, 8: at ceil(size / denom), built by libjpeg's reduced inverse
        DCTs, for every frame of the calls that follow (rfd.h, "JPEG decode, reduced size")"""
        _check(self._L.rfd_set_jpeg_scale(self._ctx, int(denom)))
        self._jpeg_scale = int(denom)

    def jpeg_last_orientations(self):
        """per frame of the last decode call: the orientation that was applied (all 1 in "ignore" mode)"""
        n = C.c_int(0)
        st = self._L.rfd_jpeg_last_orientations(self._ctx, None, 0, C.byref(n))
        if st != RFD_ERR_CAPACITY:
            _check(st)
        out = np.zeros(n.value, np.int32)
        _check(self._L.rfd_jpeg_last_orientations(self._ctx, out.ctypes.data, n.value, C.byref(n)))
        return out.tolist()

    def jpeg_last_paths(self):
        """per frame of the last decode call: 0 host (not eligible), 1 device, 2 host after the device refused the frame"""
        n = C.c_int(0)
        st = self._L.rfd_jpeg_last_paths(self._ctx, None, 0, C.byref(n))
        if st != RFD_ERR_CAPACITY:
            _check(st)
        out = np.zeros(n.value, np.int32)
        _check(self._L.rfd_jpeg_last_paths(self._ctx, out.ctypes.data, n.value, C.byref(n)))
        return out.tolist()

    def jpeg_coefficients_device(self, data):
        """jpeg_coefficients with the quantised coefficients taken from the device entropy kernel; never falls back to the host
        decoder (RFD_ERR_UNSUPPORTED where the file is not eligible or the device refused it)"""
        keep, addr, n = _byte_buffer(data)
        blocks = C.c_size_t(0)
        st = self._L.rfd_debug_jpeg_coefficients_device(self._ctx, addr, n, None, 0, C.byref(blocks))
        if st != RFD_ERR_CAPACITY:
            _check(st)
        out = np.zeros((blocks.value, 64), np.int16)
        _check(self._L.rfd_debug_jpeg_coefficients_device(self._ctx, addr, n, out.ctypes.data, blocks.value, C.byref(blocks)))
        return out

    @staticmethod
    def _jpeg_files(files):
        bufs = [_byte_buffer(f) for f in files]
        n = len(bufs)
        ptrs = (C.c_void_p * max(n, 1))(*[b[1] for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[b[2] for b in bufs])
        return bufs, ptrs, lens

    def decode_jpeg(self, files):
        """list of JPEG files (bytes) -> list of [H, W, 3] u8 BGR host arrays, decoded on the device (a grey file: B = G = R);
        in "apply" mode (set_jpeg_orientation) H, W are the oriented size, after set_jpeg_scale the scaled one"""
        bufs, ptrs, lens = self._jpeg_files(files)
        outs = []
        for k, f in enumerate(files):
            try:
                if self._jpeg_scale != 1:
                    i = jpeg_scaled_size(f, self._jpeg_scale, "apply" if self._jpeg_apply_orientation else "ignore")
                else:
                    i = jpeg_orientation(f) if self._jpeg_apply_orientation else jpeg_info(f)
            except RfdError as e:   # name the file, as the batch call itself does
                raise RfdError(e.status, "file %d: %s" % (k, e.message)) from None
            outs.append(np.zeros((i["height"], i["width"], 3), np.uint8))
        arr, keep = self._images(outs) if outs else ((rfd_image * 1)(), [])
        _check(self._L.rfd_decode_jpeg_batch(self._ctx, ptrs, lens, len(files), arr))
        return outs

    def decode_jpeg_device(self, files, frame_ptrs, shapes, strides=None, async_=False):
        """the same into caller-allocated DEVICE frames: frame_ptrs[i] a raw device address of shapes[i] = (h, w) rows of
        strides[i] bytes (default 3 * w).  Returns the rfd_image array, which is valid input to the device-resident
        detect calls; enqueued on the detector's stream, with no host synchronisation when async_ is set."""
        bufs, ptrs, lens = self._jpeg_files(files)
        n = len(files)
        arr = (rfd_image * max(n, 1))()
        for i in range(n):
            h, w = shapes[i]
            arr[i].data, arr[i].height, arr[i].width = frame_ptrs[i], int(h), int(w)
            arr[i].stride = int(strides[i]) if strides is not None else int(w) * 3
        _check(self._L.rfd_decode_jpeg_batch_device(self._ctx, ptrs, lens, n, arr, int(async_)))
        return arr

    # ---- multi-GPU: RCCL all-gather of the detection slabs behind the C ABI ----
    @staticmethod
    def comm_unique_id():
        """rank 0: 128 opaque bytes to hand to every rank (any transport)."""
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        _check(load_library().rfd_comm_get_unique_id(C.addressof(buf)))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(self._L.rfd_comm_init(self._ctx, C.addressof(buf), int(rank), int(world)))

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        _check(self._L.rfd_comm_info(self._ctx, C.byref(r), C.byref(w)))
        return r.value, w.value

    def gather_detections(self, local_ptrs, n_local, all_ptrs):
        """local_ptrs / all_ptrs: (boxes, landmarks, count, total) DEVICE addresses; enqueued on the context's stream."""
        a = rfd_dets(*local_ptrs)
        b = rfd_dets(*all_ptrs)
        _check(self._L.rfd_gather_detections(self._ctx, C.byref(a), int(n_local), C.byref(b)))

    def comm_destroy(self):
        _check(self._L.rfd_comm_destroy(self._ctx))

    def set_stream(self, hip_stream):
        """Run on a caller-owned HIP stream (e.g. torch.cuda.current_stream().cuda_stream); None restores."""
        _check(self._L.rfd_set_stream(self._ctx, hip_stream))

    # ---- next stage: FaceSelection::call (face_selection.rs:72-189) ----
    @staticmethod
    def _sel_cfg(cfg):
        c = (C.c_float * 4)(0.3, 0.3, 0.1, 0.0075)  # FaceSelectionConfig::new, config.rs:107-117
        if cfg is not None:
            for i, v in enumerate(cfg):
                c[i] = v
        return c

    @staticmethod
    def _sel_out(box, kps, found):
        return [(box[i].copy() if found[i] & 1 else None, kps[i].reshape(5, 2).copy() if found[i] == 3 else None)
                for i in range(len(found))]

    def select_faces(self, dets, sizes, is_enroll=False, cfg=None):
        """dets: list of (det [K,5], kps [K,5,2]) per image; sizes: list of (h, w) of the source frames."""
        n = len(dets)
        d, boxes, lmk, count, total = self._alloc_dets(n)
        for i, (a, b) in enumerate(dets):
            k = min(len(a), self.max_det)
            boxes[i, :k] = a[:k]
            lmk[i, :k] = b[:k]
            count[i] = k
        hh = np.array([s[0] for s in sizes], np.int32)
        ww = np.array([s[1] for s in sizes], np.int32)
        ob, ok, fd = np.zeros((n, 5), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.int32)
        c = self._sel_cfg(cfg)
        _check(self._L.rfd_select_faces(self._ctx, C.byref(d), hh.ctypes.data, ww.ctypes.data, n, C.addressof(c),
                                        1 if is_enroll else 0, ob.ctypes.data, ok.ctypes.data, fd.ctypes.data))
        return self._sel_out(ob, ok, fd)

    def detect_select(self, frames, is_enroll=False, cfg=None):
        """FacePipeline::extract lines 198-208: detect, then return only the selected face of each frame."""
        arr, keep = self._images(frames)
        n = len(frames)
        ob, ok, fd = np.zeros((n, 5), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.int32)
        c = self._sel_cfg(cfg)
        _check(self._L.rfd_detect_select_batch(self._ctx, arr, n, C.addressof(c), 1 if is_enroll else 0,
                                               ob.ctypes.data, ok.ctypes.data, fd.ctypes.data))
        return self._sel_out(ob, ok, fd)

    # ---- the stage after selection: FaceAlignment::call (face_alignment.rs:27-141) ----
    def _align_cfg(self, image_size=None, standard_landmarks=None):
        c = rfd_alignment_config()
        self._L.rfd_alignment_config_default(C.byref(c))  # FaceAlignmentConfig::new, config.rs:44-56
        if image_size is not None:
            c.out_w, c.out_h = int(image_size[0]), int(image_size[1])
        if standard_landmarks is not None:
            for i, v in enumerate(np.asarray(standard_landmarks, np.float32).reshape(10)):
                c.standard_landmarks[i] = v
        return c

    def align_faces(self, frames, selected, image_size=None, standard_landmarks=None):
        """frames: list of HxWx3 u8 BGR; selected: list of (box [5] or None, kps [5,2] or None) as select_faces /
        detect_select return them.  -> crops [n, out_h, out_w, 3] u8, status [n] (see rfd.h)."""
        arr, keep = self._images(frames)
        n = len(frames)
        ob, ok, fd = np.zeros((n, 5), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.int32)
        for i, (b, k) in enumerate(selected):
            if b is not None:
                ob[i] = b
                fd[i] |= 1
            if k is not None:
                ok[i] = np.asarray(k, np.float32).reshape(10)
                fd[i] |= 2
        c = self._align_cfg(image_size, standard_landmarks)
        crops = np.zeros((n, c.out_h, c.out_w, 3), np.uint8)
        status = np.zeros(n, np.int32)
        _check(self._L.rfd_align_faces(self._ctx, arr, n, ob.ctypes.data, ok.ctypes.data, fd.ctypes.data, C.addressof(c),
                                       crops.ctypes.data, status.ctypes.data))
        return crops, status

    def debug_align_setup(self, sizes, selected, image_size=None, standard_landmarks=None):
        """Test hook: the records align_setup_kernel leaves for faces on frames of sizes [(h, w)] (no pixels are read); selected
        as align_faces takes it.  -> dict(mode [n], M [n, 2, 3] f64: the inverted map, roi [n, 4]: x0, y0, rw, rh,
        scale [n, 2] f64: scale_x, scale_y, area_fast [n])."""
        n = len(selected)
        ob, ok, fd = np.zeros((n, 5), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.int32)
        for i, (b, k) in enumerate(selected):
            if b is not None:
                ob[i] = b
                fd[i] |= 1
            if k is not None:
                ok[i] = np.asarray(k, np.float32).reshape(10)
                fd[i] |= 2
        hh = np.array([s[0] for s in sizes], np.int32)
        ww = np.array([s[1] for s in sizes], np.int32)
        c = self._align_cfg(image_size, standard_landmarks)
        out = dict(mode=np.zeros(n, np.int32), M=np.zeros((n, 2, 3), np.float64), roi=np.zeros((n, 4), np.int32),
                   scale=np.zeros((n, 2), np.float64), area_fast=np.zeros(n, np.int32))
        _check(self._L.rfd_debug_align_setup(self._ctx, n, ob.ctypes.data, ok.ctypes.data, fd.ctypes.data, ww.ctypes.data,
                                             hh.ctypes.data, C.addressof(c), out["mode"].ctypes.data, out["M"].ctypes.data,
                                             out["roi"].ctypes.data, out["scale"].ctypes.data, out["area_fast"].ctypes.data))
        return out

    def detect_select_align(self, frames, is_enroll=False, sel_cfg=None, image_size=None, standard_landmarks=None):
        """FacePipeline::extract lines 198-216: detect, select, align -> (selected list, crops, status)."""
        arr, keep = self._images(frames)
        n = len(frames)
        ob, ok, fd = np.zeros((n, 5), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.int32)
        sc = self._sel_cfg(sel_cfg)
        c = self._align_cfg(image_size, standard_landmarks)
        crops = np.zeros((n, c.out_h, c.out_w, 3), np.uint8)
        status = np.zeros(n, np.int32)
        _check(self._L.rfd_detect_select_align_batch(self._ctx, arr, n, C.addressof(sc), 1 if is_enroll else 0,
                                                     C.addressof(c), ob.ctypes.data, ok.ctypes.data, fd.ctypes.data,
                                                     crops.ctypes.data, status.ctypes.data))
        return self._sel_out(ob, ok, fd), crops, status

    # ---- the model inputs of the quality / ID stages and what follows their models (rfd.h) ----
    def face_tensors(self, crops, cfgs):
        """crops [n, h, w, 3] u8 BGR -> one [n, 3, out_h, out_w] f32 array (R, G, B planes) per config"""
        crops = np.ascontiguousarray(crops, np.uint8)
        assert crops.ndim == 4 and crops.shape[3] == 3
        n, h, w = crops.shape[:3]
        arr, outs, ptrs = _face_tensor_args(cfgs, n)
        _check(self._L.rfd_face_tensors(self._ctx, crops.ctypes.data, n, w, h, C.addressof(arr), len(cfgs), ptrs))
        return outs

    def align_faces_tensors(self, frames, selected, cfgs, image_size=None, standard_landmarks=None, want_crops=True):
        """align_faces plus the model inputs of every face -> (crops or None, status, tensors)"""
        arr, keep = self._images(frames)
        n = len(frames)
        ob, ok, fd = np.zeros((n, 5), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.int32)
        for i, (b, k) in enumerate(selected):
            if b is not None:
                ob[i] = b
                fd[i] |= 1
            if k is not None:
                ok[i] = np.asarray(k, np.float32).reshape(10)
                fd[i] |= 2
        c = self._align_cfg(image_size, standard_landmarks)
        crops = np.zeros((n, c.out_h, c.out_w, 3), np.uint8) if want_crops else None
        status = np.zeros(n, np.int32)
        tc, outs, ptrs = _face_tensor_args(cfgs, n)
        _check(self._L.rfd_align_faces_tensors(self._ctx, arr, n, ob.ctypes.data, ok.ctypes.data, fd.ctypes.data, C.addressof(c),
                                               crops.ctypes.data if want_crops else None, status.ctypes.data,
                                               C.addressof(tc), len(cfgs), ptrs))
        return crops, status, outs

    def detect_select_align_tensors(self, frames, cfgs, is_enroll=False, sel_cfg=None, image_size=None, standard_landmarks=None,
                                    want_crops=True):
        """detect_select_align plus the model inputs of every face -> (selected list, crops or None, status, tensors)"""
        arr, keep = self._images(frames)
        n = len(frames)
        ob, ok, fd = np.zeros((n, 5), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.int32)
        sc = self._sel_cfg(sel_cfg)
        c = self._align_cfg(image_size, standard_landmarks)
        crops = np.zeros((n, c.out_h, c.out_w, 3), np.uint8) if want_crops else None
        status = np.zeros(n, np.int32)
        tc, outs, ptrs = _face_tensor_args(cfgs, n)
        _check(self._L.rfd_detect_select_align_tensors_batch(self._ctx, arr, n, C.addressof(sc), 1 if is_enroll else 0,
                                                             C.addressof(c), ob.ctypes.data, ok.ctypes.data, fd.ctypes.data,
                                                             crops.ctypes.data if want_crops else None, status.ctypes.data,
                                                             C.addressof(tc), len(cfgs), ptrs))
        return self._sel_out(ob, ok, fd), crops, status, outs

    def detect_faces_device(self, frame_ptrs, shapes, cfgs, box_ptr, kps_ptr, found_ptr, crops_ptr, status_ptr, tensor_ptrs,
                            is_enroll=False, sel_cfg=None, image_size=None, standard_landmarks=None, async_=False):
        """Frames and every output already in device memory (raw device addresses; crops_ptr may be None); enqueued on the
        context's stream, with no host synchronisation when async_ is set (then sync() before reading)."""
        n = len(frame_ptrs)
        arr = (rfd_image * n)()
        for i, (p, (h, w)) in enumerate(zip(frame_ptrs, shapes)):
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = p, h, w, w * 3
        sc = self._sel_cfg(sel_cfg)
        c = self._align_cfg(image_size, standard_landmarks)
        tc = (rfd_face_tensor_config * max(len(cfgs), 1))(*cfgs)
        out = rfd_faces(box_ptr, kps_ptr, found_ptr, crops_ptr, status_ptr)
        for j, p in enumerate(tensor_ptrs):
            out.tensors[j] = p
        _check(self._L.rfd_detect_faces_device(self._ctx, arr, n, C.addressof(sc), 1 if is_enroll else 0, C.addressof(c),
                                               C.addressof(tc), len(cfgs), C.byref(out), int(async_)))

    # ---- every detected face of a frame: the packed face list (rfd.h) ----
    def _face_list_call(self, frames, cfgs, cap, list_cfg, image_size, standard_landmarks, want_crops, out):
        arr, keep = self._images(frames)
        c = self._align_cfg(image_size, standard_landmarks)
        lc = list_cfg if list_cfg is not None else face_list_config()
        if out is None:
            out = FaceList(len(frames), cap, cfgs, (max(c.out_w, 1), max(c.out_h, 1)), want_crops)
        tc = (rfd_face_tensor_config * max(len(cfgs), 1))(*cfgs)
        return arr, keep, c, lc, tc, out

    def align_detections(self, frames, dets, cfgs=(), cap=1, list_cfg=None, image_size=None, standard_landmarks=None,
                         want_crops=True, out=None):
        """frames: list of HxWx3 u8 BGR; dets: list of (det [K,5], kps [K,5,2]) per frame, as call_batch returns them.
        -> FaceList of up to cap faces (out: a caller-made FaceList to write into)"""
        cfgs = list(cfgs)
        arr, keep, c, lc, tc, out = self._face_list_call(frames, cfgs, cap, list_cfg, image_size, standard_landmarks, want_crops, out)
        n = len(frames)
        d, boxes, lmk, count, total = self._alloc_dets(n)
        for i, (a, b) in enumerate(dets):
            k = min(len(a), self.max_det)
            boxes[i, :k] = a[:k]
            lmk[i, :k] = np.asarray(b, np.float32).reshape(-1, 5, 2)[:k]
            count[i] = k
        st = out.struct()
        _check(self._L.rfd_align_detections(self._ctx, arr, n, C.byref(d), C.addressof(lc), C.addressof(c), C.addressof(tc),
                                            len(cfgs), int(cap), C.byref(st)))
        return out

    def detect_align_all(self, frames, cfgs=(), cap=1, list_cfg=None, image_size=None, standard_landmarks=None,
                         want_crops=True, out=None):
        """detect, list every face, align and tensorise: host frames in -> FaceList of up to cap faces"""
        cfgs = list(cfgs)
        arr, keep, c, lc, tc, out = self._face_list_call(frames, cfgs, cap, list_cfg, image_size, standard_landmarks, want_crops, out)
        st = out.struct()
        _check(self._L.rfd_detect_align_all_batch(self._ctx, arr, len(frames), C.addressof(lc), C.addressof(c), C.addressof(tc),
                                                  len(cfgs), int(cap), C.byref(st)))
        return out

    def detect_all_faces_device(self, frame_ptrs, shapes, cfgs, cap, total_ptr, first_ptr, frame_ptr, row_ptr, box_ptr, kps_ptr,
                                status_ptr, crops_ptr, tensor_ptrs, list_cfg=None, image_size=None, standard_landmarks=None,
                                async_=False):
        """Frames and every output already in device memory (raw device addresses; crops_ptr may be None); enqueued on the
        context's stream, with no host synchronisation when async_ is set (then sync() before reading)."""
        n = len(frame_ptrs)
        arr = (rfd_image * n)()
        for i, (p, (h, w)) in enumerate(zip(frame_ptrs, shapes)):
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = p, h, w, w * 3
        c = self._align_cfg(image_size, standard_landmarks)
        lc = list_cfg if list_cfg is not None else face_list_config()
        cfgs = list(cfgs)
        tc = (rfd_face_tensor_config * max(len(cfgs), 1))(*cfgs)
        out = rfd_face_list(total_ptr, first_ptr, frame_ptr, row_ptr, box_ptr, kps_ptr, status_ptr, crops_ptr)
        for j, p in enumerate(tensor_ptrs):
            out.tensors[j] = p
        _check(self._L.rfd_detect_all_faces_device(self._ctx, arr, n, C.addressof(lc), C.addressof(c), C.addressof(tc), len(cfgs),
                                                   int(cap), C.byref(out), int(async_)))

    def align_detections_device(self, frame_ptrs, shapes, boxes_ptr, landmarks_ptr, count_ptr, cfgs, cap, out, list_cfg=None,
                                image_size=None, standard_landmarks=None, async_=False):
        """rfd_align_detections_device: the face list over DEVICE detection slabs (a tracker's due slab, say) of DEVICE frames;
        out: an rfd_face_list of device addresses.  Enqueued on the context's stream, as detect_all_faces_device."""
        n = len(frame_ptrs)
        arr = (rfd_image * n)()
        for i, (p, (h, w)) in enumerate(zip(frame_ptrs, shapes)):
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = p, h, w, w * 3
        c = self._align_cfg(image_size, standard_landmarks)
        lc = list_cfg if list_cfg is not None else face_list_config()
        cfgs = list(cfgs)
        tc = (rfd_face_tensor_config * max(len(cfgs), 1))(*cfgs)
        d = rfd_dets(boxes_ptr, landmarks_ptr, count_ptr, None)
        _check(self._L.rfd_align_detections_device(self._ctx, arr, n, C.byref(d), C.addressof(lc), C.addressof(c), C.addressof(tc),
                                                   len(cfgs), int(cap), C.byref(out), int(async_)))

    # ---- shot quality: a figure of merit per detection row from the frame, the box and the landmarks (rfd.h, "shot quality") ----
    def shot_quality(self, frames, dets, cfg=None, device=False, out=None, async_=False):
        """rfd_shot_quality / rfd_shot_quality_device -> (quality [n, max_det] f32, parts [n, max_det, 8] f32 (sharp, mean, expo,
        yaw, roll, pitch, pose, size), status [n, max_det] i32); cfg: an rfd_shot_quality_config (shot_quality_config()), None =
        the default.  Rows at or past a frame's count keep what `out` held.
        device=False: frames = HxWx3 u8 BGR arrays, dets = (boxes [n, max_det, 5], landmarks [n, max_det, 5, 2], count [n]) as
        the detect calls fill them; out = (quality, parts, status) arrays to write into (default: zeros), which are returned.
        device=True: frames = [(device address, height, width[, stride])], dets = (boxes, landmarks, count) device addresses, out =
        (quality, parts or None, status or None) device addresses, which are returned; enqueued on the context's stream, with no
        host synchronisation when async_ is set."""
        n, md = len(frames), self.max_det
        cp = None if cfg is None else C.byref(cfg)
        if device:
            arr = (rfd_image * max(n, 1))()
            for i, f in enumerate(frames):
                arr[i].data, arr[i].height, arr[i].width = f[0], f[1], f[2]
                arr[i].stride = f[3] if len(f) > 3 else f[2] * 3
            d = rfd_dets(dets[0], dets[1], dets[2], None)
            _check(self._L.rfd_shot_quality_device(self._ctx, arr, n, C.byref(d), cp, out[0], out[1], out[2], int(async_)))
            return out
        arr, keep = self._images(frames)
        b = np.ascontiguousarray(dets[0], np.float32).reshape(n, md, 5)
        l = np.ascontiguousarray(dets[1], np.float32).reshape(n, md, 10)
        c = np.ascontiguousarray(dets[2], np.int32).reshape(n)
        if out is None:
            out = (np.zeros((n, md), np.float32), np.zeros((n, md, SHOT_QUALITY_PARTS), np.float32), np.zeros((n, md), np.int32))
        q, parts, status = out
        d = rfd_dets(b.ctypes.data, l.ctypes.data, c.ctypes.data, None)
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(self._L.rfd_shot_quality(self._ctx, arr, n, C.byref(d), cp, ptr(q), ptr(parts), ptr(status)))
        return q, parts, status

    # ---- redaction: pixelate or fill the faces of detection rows in frames (rfd.h, "redaction") ----
    def redact_faces(self, frames, dets, sel=None, cfg=None, device=False, dst=None, applied=None, async_=False):
        """rfd_redact_faces / rfd_redact_faces_device; cfg: an rfd_redact_config (redact_config()), None = the default.
        device=False: frames = HxWx3 u8 BGR arrays (any row stride, unit pixel stride), dets = (boxes [n, max_det, 5], count [n]),
        sel = u32 [n, max_det] or None; dst = arrays of the frames' shapes to write into, None = in place (the frames
        themselves are painted) -> (the painted arrays, applied [n] i32).
        device=True: frames and dst = [(device address, height, width[, stride])], dets = (boxes, count) device addresses, sel and
        applied = device addresses or None; enqueued on the context's stream, with no host synchronisation when async_ is set."""
        n, md = len(frames), self.max_det
        cp = None if cfg is None else C.byref(cfg)
        if device:
            def descs(fr):
                arr = (rfd_image * max(n, 1))()
                for i, f in enumerate(fr):
                    arr[i].data, arr[i].height, arr[i].width = f[0], f[1], f[2]
                    arr[i].stride = f[3] if len(f) > 3 else f[2] * 3
                return arr
            d = rfd_dets(dets[0], None, dets[1], None)
            _check(self._L.rfd_redact_faces_device(self._ctx, descs(frames), None if dst is None else descs(dst), n, C.byref(d), sel, cp,
                                                   applied, int(async_)))
            return dst, applied
        for f in list(frames) + list(dst or []):
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3 and f.strides[1:] == (3, 1)):
                raise RfdError(RFD_ERR_INVALID_ARG, "frames must be HxWx3 uint8 arrays (BGR) with contiguous rows: they are written in place")
        arr, keep = self._images(frames) if n else ((rfd_image * 1)(), [])
        darr = None
        if dst is not None:
            darr, keep_dst = self._images(dst) if n else ((rfd_image * 1)(), [])
        b = np.ascontiguousarray(dets[0], np.float32).reshape(n, md, 5)
        c = np.ascontiguousarray(dets[1], np.int32).reshape(n)
        s = None if sel is None else np.ascontiguousarray(sel, np.uint32).reshape(n, md)
        if applied is None:
            applied = np.zeros(n, np.int32)
        d = rfd_dets(b.ctypes.data, None, c.ctypes.data, None)
        _check(self._L.rfd_redact_faces(self._ctx, arr, darr, n, C.byref(d), None if s is None else s.ctypes.data, cp, applied.ctypes.data))
        return (list(frames) if dst is None else list(dst)), applied

    # ---- annotation: box outlines, landmarks and text labels drawn into frames (rfd.h, "annotation") ----
    def annotate_faces(self, frames, dets, sel=None, label=None, value=None, cfg=None, device=False, dst=None, applied=None, async_=False):
        """rfd_annotate_faces / rfd_annotate_faces_device; cfg: an rfd_annotate_config (annotate_config()), None = the default.
        device=False: frames = HxWx3 u8 BGR arrays (any row stride, unit pixel stride), dets = (boxes [n, max_det, 5], landmarks
        [n, max_det, 10] or None, count [n]), sel = u32, label = i32, value = f32 [n, max_det] or None; dst = arrays of the frames'
        shapes to write into, None = in place (the frames themselves are painted) -> (the painted arrays, applied [n] i32).
        device=True: frames and dst = [(device address, height, width[, stride])], dets = (boxes, landmarks, count) device
        addresses, sel, label, value and applied = device addresses or None; enqueued on the context's stream, with no host
        synchronisation when async_ is set."""
        n, md = len(frames), self.max_det
        cp = None if cfg is None else C.byref(cfg)
        if device:
            def descs(fr):
                arr = (rfd_image * max(n, 1))()
                for i, f in enumerate(fr):
                    arr[i].data, arr[i].height, arr[i].width = f[0], f[1], f[2]
                    arr[i].stride = f[3] if len(f) > 3 else f[2] * 3
                return arr
            d = rfd_dets(dets[0], dets[1], dets[2], None)
            _check(self._L.rfd_annotate_faces_device(self._ctx, descs(frames), None if dst is None else descs(dst), n, C.byref(d), sel, label,
                                                     value, cp, applied, int(async_)))
            return dst, applied
        for f in list(frames) + list(dst or []):
            if not (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3 and f.strides[1:] == (3, 1)):
                raise RfdError(RFD_ERR_INVALID_ARG, "frames must be HxWx3 uint8 arrays (BGR) with contiguous rows: they are written in place")
        arr, keep = self._images(frames) if n else ((rfd_image * 1)(), [])
        darr = None
        if dst is not None:
            darr, keep_dst = self._images(dst) if n else ((rfd_image * 1)(), [])
        whole = lambda a, t, *shape: None if a is None else np.ascontiguousarray(a, t).reshape(n, *shape)
        ptr = lambda a: None if a is None else a.ctypes.data
        b, lm, c = whole(dets[0], np.float32, md, 5), whole(dets[1], np.float32, md, 10), whole(dets[2], np.int32)
        s, lb, va = whole(sel, np.uint32, md), whole(label, np.int32, md), whole(value, np.float32, md)
        if applied is None:
            applied = np.zeros(n, np.int32)
        d = rfd_dets(ptr(b), ptr(lm), ptr(c), None)
        _check(self._L.rfd_annotate_faces(self._ctx, arr, darr, n, C.byref(d), ptr(s), ptr(lb), ptr(va), cp, applied.ctypes.data))
        return (list(frames) if dst is None else list(dst)), applied

    # ---- frames in camera and decoder formats (rfd.h): NV12, I420, YUYV, BGRA ... -> the BGR frames every other call reads ----
    def convert_frames(self, frames):
        """rfd_convert_frames.  frames: list of (format, width, height, planes[, color]); format a PIXEL_* value or its lower-case
        name, planes the 2-D u8 host arrays of the format's planes ([rows, row_bytes], any row stride, unit byte stride), color
        a COLOR_* value (default BT.601 limited).  -> list of [H, W, 3] u8 BGR host arrays, converted on the device."""
        n = len(frames)
        src, keep, outs = (rfd_frame * max(n, 1))(), [], []
        for i, fr in enumerate(frames):
            fmt, w, h, planes = fr[0], int(fr[1]), int(fr[2]), fr[3]
            for a in planes:
                if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 2 and (a.shape[1] <= 1 or a.strides[1] == 1)):
                    raise RfdError(RFD_ERR_INVALID_ARG, "frame %d: planes must be 2-D uint8 arrays with contiguous rows" % i)
            keep.append(planes)
            src[i] = frame(fmt, w, h, [a.ctypes.data for a in planes], [a.strides[0] for a in planes], fr[4] if len(fr) > 4 else 0)
            outs.append(np.zeros((h, w, 3), np.uint8))
        arr, keep_out = self._images(outs) if outs else ((rfd_image * 1)(), [])
        _check(self._L.rfd_convert_frames(self._ctx, src, n, arr))
        return outs

    def _frames_call(self, fn, frames, frame_ptrs, strides, async_):
        n = len(frames)
        src, arr = (rfd_frame * max(n, 1))(), (rfd_image * max(n, 1))()
        for i, f in enumerate(frames):
            src[i] = f
            arr[i].data, arr[i].height, arr[i].width = frame_ptrs[i], f.height, f.width
            arr[i].stride = int(strides[i]) if strides is not None else f.width * 3
        _check(fn(self._ctx, src, n, arr, int(async_)))
        return arr

    def convert_frames_device(self, frames, frame_ptrs, strides=None, async_=False):
        """rfd_convert_frames_device.  frames: rfd_frame structures (frame()) whose planes are raw DEVICE addresses; frame_ptrs[i]:
        the raw device address of output frame i, of frames[i].height rows of strides[i] bytes (default 3 * width).  Returns the
        rfd_image array, which is valid input to the device-resident detect calls; enqueued on the detector's stream, with no
        host synchronisation when async_ is set."""
        return self._frames_call(self._L.rfd_convert_frames_device, frames, frame_ptrs, strides, async_)

    def upload_frames_device(self, frames, frame_ptrs, strides=None, async_=False):
        """rfd_upload_frames_device: the same with the planes at raw HOST addresses (pageable or host_alloc memory), which must
        stay as they are until the stream has run the copies when async_ is set."""
        return self._frames_call(self._L.rfd_upload_frames_device, frames, frame_ptrs, strides, async_)

    def encode_jpeg(self, frames, cfg=None, slot_bytes=None):
        """rfd_encode_jpeg_batch.  frames: list of [H, W, 3] u8 BGR host arrays (any row stride, unit pixel stride) -> list of
        files (bytes), encoded on the device; None where a file does not fit slot_bytes (default: the largest bound)"""
        cfg = cfg or jpeg_encode_config()
        n = len(frames)
        arr, keep = self._images(frames) if n else ((rfd_image * 1)(), [])
        if slot_bytes is None:
            slot_bytes = max([jpeg_encode_bound(f.shape[1], f.shape[0], cfg) for f in frames] + [1])
        out = np.zeros((max(n, 1), int(slot_bytes)), np.uint8)
        size = np.zeros(max(n, 1), np.int32)
        _check(self._L.rfd_encode_jpeg_batch(self._ctx, arr, n, C.byref(cfg), out.ctypes.data, int(slot_bytes), size.ctypes.data))
        return [out[i, :size[i]].tobytes() if size[i] >= 0 else None for i in range(n)]

    def encode_jpeg_device(self, frame_ptrs, shapes, out_ptr, slot_bytes, size_ptr, cfg=None, strides=None, count_ptr=None, async_=False):
        """rfd_encode_jpeg_batch_device.  frame_ptrs[i]: the raw DEVICE address of image i, shapes[i] = (h, w) rows of strides[i]
        bytes (default 3 * w); out_ptr: device slots of slot_bytes each; size_ptr: device i32 [n]; count_ptr: device i32 or
        None.  Enqueued on the detector's stream, with no host synchronisation when async_ is set."""
        cfg = cfg or jpeg_encode_config()
        n = len(frame_ptrs)
        arr = (rfd_image * max(n, 1))()
        for i in range(n):
            h, w = shapes[i]
            arr[i].data, arr[i].height, arr[i].width = frame_ptrs[i], int(h), int(w)
            arr[i].stride = int(strides[i]) if strides is not None else int(w) * 3
        _check(self._L.rfd_encode_jpeg_batch_device(self._ctx, arr, n, count_ptr, C.byref(cfg), out_ptr, int(slot_bytes), size_ptr, int(async_)))

    def jpeg_encode_blocks(self, frame, cfg=None):
        """test hook rfd_debug_jpeg_encode_blocks: one [H, W, 3] u8 BGR host frame -> [blocks, 64] i16 quantised coefficients,
        natural order, dummy blocks included"""
        cfg = cfg or jpeg_encode_config()
        arr, keep = self._images([frame])
        blocks = C.c_size_t(0)
        st = self._L.rfd_debug_jpeg_encode_blocks(self._ctx, arr, C.byref(cfg), None, 0, C.byref(blocks))
        if st != RFD_ERR_CAPACITY:
            _check(st)
        out = np.zeros((blocks.value, 64), np.int16)
        _check(self._L.rfd_debug_jpeg_encode_blocks(self._ctx, arr, C.byref(cfg), out.ctypes.data, blocks.value, C.byref(blocks)))
        return out

    def jpeg_encode_coefficients(self, coef, width, height, cfg=None, cap=None):
        """test hook rfd_debug_jpeg_encode_coefficients: [blocks, 64] i16 coefficients, natural order -> the file (bytes) the
        entropy and assembly kernels write for them, None if it does not fit cap (default: the bound)"""
        cfg = cfg or jpeg_encode_config()
        coef = np.ascontiguousarray(coef, np.int16)
        cap = int(cap if cap is not None else jpeg_encode_bound(width, height, cfg))
        out, n = np.zeros(max(cap, 1), np.uint8), C.c_int32(0)
        _check(self._L.rfd_debug_jpeg_encode_coefficients(self._ctx, coef.ctypes.data, coef.shape[0], int(width), int(height), C.byref(cfg),
                                                           out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].tobytes() if n.value >= 0 else None

    def quality_decide(self, logits, threshold):
        """logits [n, classes] of the quality model -> (score [n] f32, klass [n] i32), face_quality.rs:159-168"""
        x = np.ascontiguousarray(logits, np.float32)
        assert x.ndim == 2
        score, klass = np.zeros(x.shape[0], np.float32), np.zeros(x.shape[0], np.int32)
        _check(self._L.rfd_quality_decide(self._ctx, x.ctypes.data, x.shape[0], x.shape[1], float(threshold), score.ctypes.data,
                                          klass.ctypes.data))
        return score, klass

    def normalize_embeddings(self, emb):
        """emb [n, dim] of the ID model -> emb / its L2 norm per row, utils.rs:148-154"""
        x = np.ascontiguousarray(emb, np.float32)
        assert x.ndim == 2
        out = np.zeros_like(x)
        _check(self._L.rfd_normalize_embeddings(self._ctx, x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data))
        return out

    # ---- liveness: the inputs of the miniFAS models and the rule on their outputs (face_antispoofing.rs; rfd.h) ----
    def liveness_tensors(self, frames, boxes, found=None, cfg=None):
        """frames: list of HxWx3 u8 BGR; boxes [n, >= 4] (x1, y1, x2, y2[, score]); found [n] (default: every face has a box)
        -> (tensors: one [n, 3, out_h, out_w] f32 array per model, B, G, R planes; weights [n, k]; rois [n, k, 4]; status [n])"""
        arr, keep = self._images(frames)
        n = len(frames)
        cfg = liveness_config() if cfg is None else cfg
        k = max(min(cfg.k, MAX_FACE_TENSORS), 0)
        b = np.zeros((n, 5), np.float32)
        bx = np.asarray(boxes, np.float32).reshape(n, -1)
        b[:, :min(bx.shape[1], 5)] = bx[:, :5]
        fd = np.ones(n, np.int32) if found is None else np.ascontiguousarray(found, np.int32)
        outs = [np.zeros((n, 3, max(cfg.out_h[j], 1), max(cfg.out_w[j], 1)), np.float32) for j in range(k)]
        ptrs = (C.c_void_p * max(k, 1))(*[o.ctypes.data for o in outs])
        weights, rois, status = np.zeros((n, k), np.float32), np.zeros((n, k, 4), np.int32), np.zeros(n, np.int32)
        _check(self._L.rfd_liveness_tensors(self._ctx, arr, n, b.ctypes.data, fd.ctypes.data, C.addressof(cfg), ptrs,
                                            weights.ctypes.data, rois.ctypes.data, status.ctypes.data))
        return outs, weights, rois, status

    def liveness_tensors_device(self, frame_ptrs, shapes, box_ptr, found_ptr, tensor_ptrs, weights_ptr, rois_ptr, status_ptr,
                                cfg=None, strides=None, async_=False):
        """Frames, boxes, flags and every output already in device memory (raw device addresses; rois_ptr may be None); enqueued on
        the context's stream, with no host synchronisation when async_ is set (then sync() before reading)."""
        n = len(frame_ptrs)
        arr = (rfd_image * n)()
        for i, (p, (h, w)) in enumerate(zip(frame_ptrs, shapes)):
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = p, h, w, (w * 3 if strides is None else strides[i])
        cfg = liveness_config() if cfg is None else cfg
        ptrs = (C.c_void_p * max(len(tensor_ptrs), 1))(*tensor_ptrs)
        _check(self._L.rfd_liveness_tensors_device(self._ctx, arr, n, box_ptr, found_ptr, C.addressof(cfg), ptrs, weights_ptr,
                                                   rois_ptr, status_ptr, int(async_)))

    def liveness_decide(self, logits, weights, threshold=0.55):
        """logits: one [n, classes] array per model; weights [n, k] of liveness_tensors -> (score [n] f32, live [n] i32):
        the weighted mean of column 1 over the models, live = score > threshold (face_antispoofing.rs:219-243)"""
        xs = [np.ascontiguousarray(x, np.float32) for x in logits]
        k, (n, classes) = len(xs), xs[0].shape
        assert all(x.shape == (n, classes) for x in xs)
        w = np.ascontiguousarray(weights, np.float32).reshape(n, k)
        ptrs = (C.c_void_p * k)(*[x.ctypes.data for x in xs])
        score, live = np.zeros(n, np.float32), np.zeros(n, np.int32)
        _check(self._L.rfd_liveness_decide(self._ctx, ptrs, k, n, classes, w.ctypes.data, float(threshold), score.ctypes.data,
                                           live.ctypes.data))
        return score, live

    def liveness_decide_device(self, logit_ptrs, n, classes, weights_ptr, score_ptr, live_ptr, threshold=0.55):
        """the same on raw device addresses, enqueued on the context's stream (no synchronisation)"""
        k = len(logit_ptrs)
        ptrs = (C.c_void_p * k)(*logit_ptrs)
        _check(self._L.rfd_liveness_decide_device(self._ctx, ptrs, k, n, classes, weights_ptr, float(threshold), score_ptr, live_ptr))

    # ---- stage-level entry points ----
    def preprocess(self, frames):
        """_preprocess + tensorise: -> det_img [n,H,W,3] u8, tensor [n,3,H,W] f32, det_scale [n]."""
        arr, keep = self._images(frames)
        n = len(frames)
        w, h = self.image_size
        det_img = np.zeros((n, h, w, 3), np.uint8)
        tensor = np.zeros((n, 3, h, w), np.float32)
        scale = np.zeros(n, np.float32)
        _check(self._L.rfd_preprocess(self._ctx, arr, n, det_img.ctypes.data, tensor.ctypes.data,
                                      scale.ctypes.data))
        return det_img, tensor, scale

    def forward(self, tensor):
        """tensor [n,3,H,W] f32 -> the 9 head tensors (f32, NCHW)."""
        t = np.ascontiguousarray(tensor, np.float32)
        n = t.shape[0]
        w, h = self.image_size
        assert t.shape == (n, 3, h, w)
        heads = [np.zeros(s, np.float32) for s in head_shapes(n, h, w)]
        ptrs = (C.c_void_p * 9)(*[x.ctypes.data for x in heads])
        _check(self._L.rfd_forward(self._ctx, t.ctypes.data, n, ptrs))
        return heads

    def decode_nms(self, heads, det_scale, want_gidx=False):
        """9 head tensors [n,C,h,w] + det_scale [n] -> list of (det, kps[, gidx]) per image."""
        hs = [np.ascontiguousarray(x, np.float32) for x in heads]
        n = hs[0].shape[0]
        w, h = self.image_size
        for x, s in zip(hs, head_shapes(n, h, w)):
            if x.shape != s:
                raise RfdError(RFD_ERR_INVALID_ARG, "head shape %s != %s" % (x.shape, s))
        sc = np.ascontiguousarray(det_scale, np.float32).reshape(n)
        ptrs = (C.c_void_p * 9)(*[x.ctypes.data for x in hs])
        d, boxes, lmk, count, total = self._alloc_dets(n)
        gidx = np.zeros((n, self.max_det), np.int32)
        _check(self._L.rfd_decode_nms(self._ctx, ptrs, n, sc.ctypes.data, C.byref(d),
                                      gidx.ctypes.data if want_gidx else None))
        self.last_total = total
        res = self._split(boxes, lmk, count)
        if want_gidx:
            res = [(a, b, gidx[i, :count[i]].copy()) for i, (a, b) in enumerate(res)]
        return res

    # ---- views (rfd.h, "views"): detection over overlapping views of a frame, merged on the device ----
    def detect_views(self, frames, views, edge_margin=4.0):
        """frames: HxWx3 u8 BGR arrays; views: rfd_view or (frame, x, y, w, h, inner), sorted by frame (view_plan) -> one
        (det [K,5], kps [K,5,2]) per FRAME, in source-frame pixels"""
        arr, keep = self._images(frames)
        d, boxes, lmk, count, total = self._alloc_dets(len(frames))
        _check(self._L.rfd_detect_views_batch(self._ctx, arr, len(frames), _view_array(views), len(views), float(edge_margin), C.byref(d)))
        self.last_total = total
        return self._split(boxes, lmk, count)

    def detect_views_device(self, frame_ptrs, shapes, views, out_boxes_ptr, out_lmk_ptr, out_count_ptr, out_total_ptr, edge_margin=4.0,
                            strides=None, async_=False):
        """frames and output slabs [n_frames][max_det] already in device memory (raw device pointers)"""
        n = len(frame_ptrs)
        arr = (rfd_image * n)()
        for i, (p, (h, w)) in enumerate(zip(frame_ptrs, shapes)):
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = p, h, w, strides[i] if strides else w * 3
        d = rfd_dets(out_boxes_ptr, out_lmk_ptr, out_count_ptr, out_total_ptr)
        _check(self._L.rfd_detect_views_batch_device(self._ctx, arr, n, _view_array(views), len(views), float(edge_margin), C.byref(d), int(async_)))

    def decode_nms_views(self, heads, views, n_frames, edge_margin=4.0, want_gidx=False):
        """9 head tensors [n_views,C,h,w], image i being view i -> per FRAME (det, kps[, gidx]); gidx = v * anchors + g"""
        hs = [np.ascontiguousarray(x, np.float32) for x in heads]
        n = len(views)
        w, h = self.image_size
        for x, s in zip(hs, head_shapes(n, h, w)):
            if x.shape != s:
                raise RfdError(RFD_ERR_INVALID_ARG, "head shape %s != %s" % (x.shape, s))
        ptrs = (C.c_void_p * 9)(*[x.ctypes.data for x in hs])
        d, boxes, lmk, count, total = self._alloc_dets(max(n_frames, 1))
        gidx = np.zeros((max(n_frames, 1), self.max_det), np.int32)
        _check(self._L.rfd_decode_nms_views(self._ctx, ptrs, _view_array(views), n, int(n_frames), float(edge_margin), C.byref(d),
                                            gidx.ctypes.data if want_gidx else None))
        self.last_total = total
        res = self._split(boxes, lmk, count)
        if want_gidx:
            res = [(a, b, gidx[i, :count[i]].copy()) for i, (a, b) in enumerate(res)]
        return res

    def nms_sorted(self, boxes, thresh):
        """Greedy NMS on rows pre-sorted by score descending -> kept row indices."""
        b = np.ascontiguousarray(boxes, np.float32)
        keep = np.zeros(max(b.shape[0], 1), np.int32)
        num = C.c_int(0)
        _check(self._L.rfd_nms_sorted(self._ctx, keep.ctypes.data, C.byref(num), b.ctypes.data,
                                      b.shape[0], b.shape[1] if b.ndim == 2 else 5, float(thresh)))
        return keep[:num.value].copy()

    # ---- test hooks ----
    def debug_dtype(self, desc):
        """element type of a network tensor on the device: the f32 parity mode keeps every tensor but the network input in f32"""
        f32 = desc.is_f32 or (self.cfg.precision == PRECISION_F32 and not desc.is_input)
        return np.float32 if f32 else np.uint16

    def debug_write(self, tensor_id, arr):
        """arr: n images in device layout (NHWC), elements of the tensor's debug_dtype"""
        a = np.ascontiguousarray(arr)
        if self.cfg.precision == PRECISION_F32:   # the library copies 4 bytes per element of an intermediate tensor: hold the array to that
            if getattr(self, "_debug_graph", None) is None:
                self._debug_graph = Graph(self.cfg.backbone, *self.image_size)
            td = self._debug_graph.tensors[tensor_id]
            want = (td.height, td.width, td.channels)
            if a.ndim != 4 or a.shape[1:] != want or a.dtype != self.debug_dtype(td):
                raise RfdError(RFD_ERR_INVALID_ARG, "debug_write: tensor %d takes [n, %d, %d, %d] %s in the f32 parity mode, got %s %s" % (
                    (tensor_id,) + want + (np.dtype(self.debug_dtype(td)).name, list(a.shape), a.dtype.name)))
        _check(self._L.rfd_debug_tensor_io(self._ctx, tensor_id, a.shape[0], a.ctypes.data, 1))

    def debug_read(self, tensor_id, n, desc):
        a = np.zeros((n, desc.height, desc.width, desc.channels), self.debug_dtype(desc))
        _check(self._L.rfd_debug_tensor_io(self._ctx, tensor_id, n, a.ctypes.data, 0))
        return a

    def debug_set_conv_tile(self, tile):
        _check(self._L.rfd_debug_set_conv_tile(self._ctx, tile))

    def debug_op_kernels(self, n, op, co_running=True):
        """kernel(s) the library would run op `op` with at n images per chain (list of names, no rfd:: prefix); nothing is launched"""
        buf = C.create_string_buffer(512)
        _check(self._L.rfd_debug_op_kernels(self._ctx, n, op, 1 if co_running else 0, buf, 512))
        return buf.value.decode().split(" + ")

    def debug_set_concurrency(self, multi_stream=True, split_min_part=8, split_max_parts=2, use_graph=True):
        _check(self._L.rfd_debug_set_concurrency(self._ctx, int(multi_stream), int(split_min_part), int(split_max_parts),
                                                 int(use_graph)))

    def debug_run(self, n, first_op, last_op, batch_off=0, co_running=False):
        """ops [first_op, last_op] on images [batch_off, batch_off + n); co_running: with the kernel choice of a chain of a split pass"""
        if batch_off == 0 and not co_running:
            _check(self._L.rfd_debug_run_ops(self._ctx, n, first_op, last_op))
        else:
            _check(self._L.rfd_debug_run_chain(self._ctx, n, first_op, last_op, batch_off, 1 if co_running else 0))

    def debug_pass_chains(self, n):
        """sizes of the chains a pass of n images runs as (one entry: the pass is not split); nothing is launched"""
        sizes = (C.c_int * 8)()
        return list(sizes[:_check(self._L.rfd_debug_pass_chains(self._ctx, n, sizes, 8))])

    def debug_buffer_pitch(self, tensor_id):
        """bytes between the first images of two chains in the workspace buffer that holds the tensor"""
        pitch = C.c_size_t()
        _check(self._L.rfd_debug_buffer_io(self._ctx, tensor_id, None, 0, 0, C.byref(pitch)))
        return pitch.value

    def debug_buffer_read(self, tensor_id):
        """the whole workspace buffer that holds the tensor: max_batch_size * pitch bytes"""
        a = np.zeros(self.cfg.max_batch_size * self.debug_buffer_pitch(tensor_id), np.uint8)
        _check(self._L.rfd_debug_buffer_io(self._ctx, tensor_id, a.ctypes.data, a.nbytes, 0, None))
        return a

    def debug_buffer_write(self, tensor_id, arr):
        a = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        _check(self._L.rfd_debug_buffer_io(self._ctx, tensor_id, a.ctypes.data, a.nbytes, 1, None))

    # ---- introspection ----
    def stats(self):
        s = rfd_stats()
        _check(self._L.rfd_get_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    def set_thresholds(self, confidence_threshold, iou_threshold):
        _check(self._L.rfd_set_thresholds(self._ctx, confidence_threshold, iou_threshold))

    def set_profiling(self, enable):
        _check(self._L.rfd_set_profiling(self._ctx, 1 if enable else 0))

    def conv_profile(self):
        ms, fl, n = C.c_float(), C.c_double(), C.c_int()
        _check(self._L.rfd_get_conv_profile(self._ctx, C.byref(ms), C.byref(fl), C.byref(n)))
        return ms.value, fl.value, n.value

    def op_profile(self, nops):
        ms = np.zeros(nops, np.float32)
        _check(self._L.rfd_get_op_profile(self._ctx, ms.ctypes.data, nops))
        return ms
