"""ctypes binding of libsings_hip.so (the C ABI declared in include/sings_hip.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded this
module raises, loudly.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C sings_amd/csrc``.

This module declares the boundary: the structs, the constants and ``_PROTOTYPES``, the one table every function's ``argtypes`` /
``restype`` come from.  How tensors, cameras, skin inputs and frame batches become arguments of these functions is
``sings_amd/_marshal.py``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SINGS_HIP_LIB: another build of the SAME library (kernel experiments: tools/build_variants.sh); never a fallback
LIB_PATH = os.environ.get("SINGS_HIP_LIB") or os.path.join(_HERE, "libsings_hip.so")
_lib = None
HAS_ORDER = False                    # set by load(): the library exports the table of include/sings_order.h
HAS_SAMPLER = False                  # set by load(): the library exports the table of include/sings_sampler.h
HAS_FROZEN = False                   # set by load(): the library exports the table of include/sings_frozen.h
HAS_FEED = False                     # set by load(): the library exports the table of include/sings_feed.h
HAS_DENSITY = False                  # set by load(): the library exports the table of include/sings_density.h
HAS_SHEET = False                    # set by load(): the library exports the table of include/sings_sheet.h
HAS_SCENE = False                    # set by load(): the library exports the table of include/sings_scene.h
HAS_JPEG = False                     # set by load(): the library exports the table of include/sings_jpeg.h
HAS_PNG = False                      # set by load(): the library exports the table of include/sings_png.h
HAS_UNPNG = False                    # set by load(): the library exports the table of include/sings_unpng.h
HAS_BODY = False                     # set by load(): the library exports the table of include/sings_body.h
HAS_SILHOUETTE = False               # set by load(): the library exports the table of include/sings_silhouette.h


class SgRasterSettings(C.Structure):
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32),
        ("prefiltered", C.c_int32), ("debug", C.c_int32), ("flags", C.c_int32),
        ("bg", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
        ("count_signal", C.c_void_p), ("count_signal_host", C.c_void_p),
    ]


class SgLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "geom_recA", "geom_recB", "geom_recC", "geom_depth", "geom_flags", "geom_slot", "geom_bytes",
        "bin_header", "bin_tile_count", "bin_ranges", "bin_cursor", "bin_pair_keys", "bin_point_list",
        "bin_point_keys", "bin_pair_gid", "bin_pair_tile", "bin_pair_local", "bin_sort_items", "bin_rank_items", "bin_items", "bin_ck_start", "bin_plan", "bin_pair_mask", "bin_item_w", "bin_item_perm", "bin_rec_valid", "bin_tile_keys", "bin_bytes", "img_final_T", "img_n_contrib", "img_ckpt", "img_bytes", "bwd_bytes")]


class SgSkinInputs(C.Structure):
    _fields_ = [("J", C.c_int32), ("rot_format", C.c_int32)] + [(n, C.c_void_p) for n in (
        "xyz_canon", "rot_canon", "lbs_weights", "A", "smpl_scale", "transl", "ext_trans", "ext_rot", "ext_scale")]


class SgFrameBatch(C.Structure):
    _fields_ = [("K", C.c_int32), ("camera_stride", C.c_int32), ("transl_stride", C.c_int32), ("placement", C.c_int32)]
    # the field's name before it carried the SG_PLACEMENT_* bits (always 0 then)
    reserved = property(lambda self: self.placement, lambda self, v: setattr(self, "placement", v))


class SgSceneAvatar(C.Structure):
    """One avatar of a scene (include/sings_scene.h): a host array of them is read during the call."""
    _fields_ = [(n, C.c_int32) for n in ("P", "J", "rot_format", "reserved")] + [(n, C.c_void_p) for n in (
        "xyz_canon", "rot_canon", "lbs_weights", "scales", "opacities", "shs", "A", "transl", "smpl_scale", "ext_trans", "ext_rot",
        "ext_scale")]


MAX_FRAMES = 16                      # SG_MAX_FRAMES
SCENE_MAX_AVATARS = 8                # SG_SCENE_MAX_AVATARS
POSE_NB = 23                         # SG_POSE_NB: body joints per row of the body_pose table
PLACEMENT_EXT_TFS = 1                # SG_PLACEMENT_EXT_TFS: ext_tfs [K,3] / [K,9] / [K], one set per frame
PLACEMENT_SMPL_SCALE = 2             # SG_PLACEMENT_SMPL_SCALE: smpl_scale [K], one per frame


class SgLinearSide(C.Structure):
    _fields_ = [("cout", C.c_int), ("act", C.c_int), ("aux", C.c_void_p), ("dh", C.c_void_p), ("W", C.c_void_p),
                ("dz_out", C.c_void_p)]


class SgTriplane(C.Structure):
    _fields_ = [("n_scales", C.c_int), ("feat", C.c_int), ("res", (C.c_int * 3) * 4), ("planes", (C.c_void_p * 3) * 4),
                ("aabb", (C.c_float * 3) * 2), ("feature_minor", C.c_int), ("reserved", C.c_int)]


# The C ABI, one entry per function of include/sings_hip.h in the header's order: "<return>: <parameters>", a letter per type (_CTYPE
# below), a count behind it for a run of the same type ("p9": nine raw device pointers).  load() applies it in one loop, so every
# function has explicit argtypes AND restype; tests/test_abi.py holds every entry to the header's prototype.
_PROTOTYPES = {
    "sg_abi_version": "i:",
    "sg_version": "s:",
    "sg_last_error": "s:",
    "sg_layout": "i: i3 z L",
    "sg_rasterize_forward": "i: S i p9 z p3 i n p",
    "sg_rasterize_backward": "i: S i p10 z p12",
    "sg_rasterize_backward_records": "i: S i p2 z p4",
    "sg_rasterize_backward_gaussians": "i: S i p10 z p i p9",
    "sg_mark_visible": "i: i p5",
    "sg_read_num_rendered": "i: p n p",
    "sg_signal_alloc": "i: i V2",
    "sg_signal_free": "i: p",
    "sg_skin_ws_floats": "z: i",
    "sg_lbs_forward": "i: i2 p6",
    "sg_lbs_backward": "i: i2 p9",
    "sg_joint_transforms": "i: i2 p6",
    "sg_joint_transforms_backward": "i: i2 p8",
    "sg_pose_transforms": "i: i4 p12",
    "sg_pose_transforms_backward": "i: i4 p13",
    "sg_matrix_to_quaternion": "i: i p3",
    "sg_matrix_to_quaternion_backward": "i: i p4",
    "sg_rotation_convert": "i: i2 p3",
    "sg_rotation_convert_backward": "i: i2 p4",
    "sg_quaternion_multiply": "i: i p4",
    "sg_quaternion_multiply_backward": "i: i p6",
    "sg_skinned_forward": "i: S i K p5 z p6 n p",
    "sg_skinned_backward": "i: S i K p6 z p15",
    "sg_skinned_backward_gaussians": "i: S i K p6 z p2 i p11",
    "sg_frames_layout": "i: i3 z i L Z4",
    "sg_rasterize_forward_frames": "i: S F i p9 z p3 n p",
    "sg_skinned_forward_frames": "i: S F i K p5 z p6 n p",
    "sg_read_num_rendered_frames": "i: p i3 z i n p",
    "sg_rasterize_backward_records_frames": "i: S F i p2 z p4",
    "sg_rasterize_backward_gaussians_frames": "i: S F i p10 z p i p9",
    "sg_skin_ws_floats_frames": "z: i2",
    "sg_skinned_backward_gaussians_frames": "i: S F i K p6 z p2 i p11",
    "sg_photo_loss_frames": "i: i3 f2 p2 z p z p8",
    "sg_photo_loss_backward_frames": "i: i3 f2 p2 z p z p3 i p2",
    "sg_photo_loss_ws_bytes": "z: i2",
    "sg_photo_loss": "i: i2 f2 p11",
    "sg_photo_loss_backward": "i: i2 f2 p8",
    "sg_reg_ws_bytes": "z: i",
    "sg_region_laplacian": "i: i2 p11",
    "sg_rows_laplacian": "i: i3 p14",
    "sg_mesh_edge_loss": "i: i2 p8",
    "sg_l2norm_reg": "i: i p11",
    "sg_knn_ws_bytes": "z: i",
    "sg_gaussian_edge_loss": "i: i2 p8",
    "sg_gaussian_edge_prepare": "i: i p3",
    "sg_gaussian_edge_finish": "i: i2 p7",
    "sg_triplane_ws_bytes": "z: T",
    "sg_triplane_bwd_ws_bytes": "z: T i",
    "sg_triplane_forward": "i: T i p4",
    "sg_triplane_backward": "i: T i p3 G p2",
    "sg_triplane_backward_prepare": "i: T i p3",
    "sg_triplane_backward_prepared": "i: T i p3 G p2",
    "sg_bias_act_ws_bytes": "z: i2",
    "sg_bias_act_forward": "i: i3 p6",
    "sg_bias_act_backward": "i: i3 p7",
    "sg_scales_head_forward": "i: i p4",
    "sg_scales_head_backward": "i: i p5",
    "sg_linear_forward": "i: i4 p7",
    "sg_linear_backward": "i: i4 p7",
    "sg_linear_backward_accumulate": "i: i4 p7",
    "sg_linear_backward_fan": "i: i4 p5 D p",
    "sg_weight_grad_ws_bytes": "z: i3",
    "sg_weight_grad": "i: i3 p6",
    "sg_aux_layout": "i: i3 z Z",
    "sg_rasterize_forward_aux": "i: S i p9 z p3 i n p4",
    "sg_rasterize_backward_aux": "i: S i p10 z p15",
    "sg_skinned_forward_aux": "i: S i K p5 z p6 n p4",
    "sg_skinned_backward_aux": "i: S i K p6 z p18",
    "sg_frames_aux_layout": "i: i3 z i Z",
    "sg_skinned_forward_frames_aux": "i: S F i K p5 z p6 n p4",
    "sg_rasterize_backward_records_frames_aux": "i: S F i p2 z p7",
    "sg_skinned_backward_gaussians_frames_aux": "i: S F i K p6 z p2 i p12",
    "sg_lpips_weights_layout": "i: Z2",
    "sg_lpips_ws_bytes": "i: i3 Z",
    "sg_lpips_ws_layout": "i: i3 Z2",
    "sg_lpips_forward": "i: i4 p6",
    "sg_lpips_backward": "i: i4 p5",
    "sg_lpips_patch_gather": "i: i5 p9",
    "sg_lpips_patch_scatter": "i: i5 p7",
    "sg_frames_to_u8": "i: i3 p i p2",
    "sg_adam_chunk_elements": "z:",
    "sg_adam_step": "i: i3 p7",
    "sg_mesh_ws_bytes": "z: i2",
    "sg_mesh_edges_build": "i: i2 p5",
    "sg_mesh_edges_emit": "i: i3 p7",
    "sg_mesh_subdivide": "i: i3 p6",
    "sg_mesh_midpoints": "i: i3 p4",
    "sg_mesh_midpoints_i32": "i: i3 p4",
    "sg_mesh_collapse_max_edges": "i:",
    "sg_mesh_collapse_ws_bytes": "z: i2",
    "sg_mesh_collapse_build": "i: i3 p3 d p3",
    "sg_mesh_collapse_emit": "i: i4 p6",
    "sg_init_ws_bytes": "z: i",
    "sg_init_attributes": "i: i3 f2 p12",
    "sg_attr_mse_ws_bytes": "z:",
    "sg_attr_mse": "i: i V3 p3",
    "sg_plateau_step": "i: i3 d p4 i p i p",
    "sg_profile_enable": "i: i",
    "sg_copy_probe": "i: p2 z i p",
    "sg_profile_collect": "i: d n i",
    "sg_kernel_name": "s: i",
}
# The evaluation entry points of include/sings_eval.h, in the same mini-language: a second header and a second table, so that
# include/sings_hip.h, EXPORTS and SG_ABI_VERSION stay what callers of the render path built against.  load() binds every table.
_PROTOTYPES_EVAL = {
    "sg_image_metrics_ws_bytes": "z: i3",
    "sg_image_metrics_frames": "i: i4 p2 z p z p3",
}
# The mesh terms of the training step, include/sings_mesh_terms.h: a third header and a third table, for the same reason.
_PROTOTYPES_MESH_TERMS = {
    "sg_mesh_terms_build": "i: i3 p13",
    "sg_mesh_terms": "i: i p4 i p13",
}
# The work order of a K-camera launch, include/sings_order.h: a fourth header and a fourth table, for the same reason.
_PROTOTYPES_ORDER = {
    "sg_rasterize_forward_frames_ordered": "i: S F i p9 z p3 n p i p",
    "sg_work_order_codes": "i: i p4",
}
# The patch sampler of the LPIPS term, include/sings_sampler.h: a fifth header and a fifth table, for the same reason.
_PROTOTYPES_SAMPLER = {
    "sg_patch_sampler_ws_bytes": "z: i4",
    "sg_patch_origins": "i: i6 f p6",
}
# The decoders without a gradient, include/sings_frozen.h: a sixth header and a sixth table, for the same reason.
_PROTOTYPES_FROZEN = {
    "sg_frozen_geometry": "i: i4 p18",
    "sg_frozen_appearance": "i: i3 p13",
}
# The training frames on the device, include/sings_feed.h: a seventh header and a seventh table, for the same reason.
_PROTOTYPES_FEED = {
    "sg_frame_draw": "i: i3 p5",
    "sg_frame_expand": "i: i4 p5",
}
# The gated densification statistics, include/sings_density.h: an eighth header and an eighth table, for the same reason.
_PROTOTYPES_DENSITY = {
    "sg_density_stats": "i: i2 p7",
}
# The finished 8-bit sheets of a run's pictures, include/sings_sheet.h: a ninth header and a ninth table, for the same reason.
_PROTOTYPES_SHEET = {
    "sg_image_sheets": "i: i6 f i2 p5",
}
# Several avatars in one frame, include/sings_scene.h: a tenth header and a tenth table, for the same reason.
_PROTOTYPES_SCENE = {
    "sg_scene_forward_frames": "i: S i3 A p2 z p6 n p",
    "sg_scene_forward_frames_aux": "i: S i3 A p2 z p6 n p4",
}
# Frames to JPEG files, include/sings_jpeg.h: an eleventh header and an eleventh table, for the same reason.
_PROTOTYPES_JPEG = {
    "sg_jpeg_layout": "i: i5 Z",
    "sg_jpeg_encode_frames": "i: i5 p3 i p z p z p2",
}
# Frames to PNG files, include/sings_png.h: a twelfth header and a twelfth table, for the same reason.
_PROTOTYPES_PNG = {
    "sg_png_layout": "i: i5 Z",
    "sg_png_encode_frames": "i: i7 p3 i p z p z p2",
}
# PNG files to the frame store, include/sings_unpng.h: a thirteenth header and a thirteenth table, for the same reason.
_PROTOTYPES_UNPNG = {
    "sg_unpng_layout": "i: i z Z",
    "sg_unpng_decode": "i: i p3 z p i3 p2",
}
# The body model, include/sings_body.h: a fourteenth header and a fourteenth table, for the same reason.
_PROTOTYPES_BODY = {
    "sg_body_renorm": "i: i2 p3",
    "sg_body_joint_basis": "i: i3 p6",
    "sg_body_shaped": "i: i4 p10",
    "sg_body_smooth_ws_bytes": "z: i2",
    "sg_body_smooth": "i: i3 f p8",
}
# The soft silhouette and the pose update, include/sings_silhouette.h: a fifteenth header and a fifteenth table, for the same reason.
_PROTOTYPES_SILHOUETTE = {
    "sg_sil_layout": "i: i5 z Z",
    "sg_sil_forward": "i: i5 f5 z p6",
    "sg_sil_backward": "i: i5 f5 z p8",
    "sg_sil_pose_update": "i: i f p10 i p",
}
_P = C.POINTER
_CTYPE = {"i": C.c_int, "z": C.c_size_t, "f": C.c_float, "s": C.c_char_p,
          "p": C.c_void_p,                        # a raw device pointer (or NULL), and the stream
          "S": _P(SgRasterSettings), "F": _P(SgFrameBatch), "K": _P(SgSkinInputs), "L": _P(SgLayout), "T": _P(SgTriplane),
          "A": _P(SgSceneAvatar),                 # SgSceneAvatar[S] (host)
          "D": _P(SgLinearSide),                  # SgLinearSide[2]
          "n": _P(C.c_int64), "Z": _P(C.c_size_t), "d": _P(C.c_double),     # host outputs (one value or an array)
          "V": _P(C.c_void_p),                    # void **
          "G": _P(C.c_void_p * 3 * 4)}            # float *d_planes[4][3]
EXPORTS = tuple(_PROTOTYPES)         # every symbol include/sings_hip.h declares
LPIPS_NUM_OFFSETS = 46               # SG_LPIPS_NUM_OFFSETS
LPIPS_WS_NUM_PIECES = 28             # SG_LPIPS_WS_NUM_PIECES
LPIPS_MIN_SIZE = 16                  # SG_LPIPS_MIN_SIZE
NUM_KERNELS = 8
ABI_VERSION = 8                      # SG_ABI_VERSION
METRICS_CLAMP = 1                    # SG_METRICS_CLAMP
METRICS_FLOATS = 8                   # SG_METRICS_FLOATS
METRICS_STRIP_COLS = 64              # SG_METRICS_STRIP_COLS
METRICS_CHUNK_ROWS = 32              # SG_METRICS_CHUNK_ROWS
ORDER_WINDOW_TILES = 1536            # SG_ORDER_WINDOW_TILES
ORDER_BLOCK = 256                    # SG_ORDER_BLOCK
ORDER_CODE_BITS = 10                 # SG_ORDER_CODE_BITS
ORDER_WS_BYTES = 32                  # SG_ORDER_WS_BYTES
HIST_TILES_MAX = 4096                # SG_HIST_TILES_MAX (sings_amd/csrc/sg_common.h): tile counters up to which a frame has "few tiles"
PATCH_MAX_N = 16                     # SG_PATCH_MAX_N
PATCH_CHUNK = 4096                   # SG_PATCH_CHUNK
PATCH_STATE_WORDS = 4                # SG_PATCH_STATE_WORDS
PATCH_BRANCH_MASKED, PATCH_BRANCH_UNIFORM, PATCH_BRANCH_FORCED = 0, 1, 2         # SG_PATCH_BRANCH_*
FEED_MAX_FRAMES = 16384              # SG_FEED_MAX_FRAMES
FEED_MAX_K = 16                      # SG_FEED_MAX_K
FEED_STATE_WORDS = 4                 # SG_FEED_STATE_WORDS
DENSITY_MAX_K = 16                   # SG_DENSITY_MAX_K
DENSITY_BLOCK = 256                  # SG_DENSITY_BLOCK: Gaussians per workgroup of the gated statistics
SHEET_TRUNC, SHEET_ROUND = 0, 1      # SG_SHEET_TRUNC, SG_SHEET_ROUND
SHEET_MAX_SHEETS = 65535             # SG_SHEET_MAX_SHEETS
SHEET_BLOCK = 256                    # SG_SHEET_BLOCK: threads per workgroup, 4 pixels of a sheet each
JPEG_MAX_FRAMES = 16                 # SG_JPEG_MAX_FRAMES
JPEG_MAX_DIM = 65535                 # SG_JPEG_MAX_DIM
JPEG_TABLE_WORDS = 800               # SG_JPEG_TABLE_WORDS
JPEG_HUFF_STRIDE = 272               # SG_JPEG_HUFF_STRIDE
JPEG_MCU_BYTES = 1248                # SG_JPEG_MCU_BYTES
JPEG_LAYOUT = ("ws_bytes", "mcus", "segments", "slot_pitch", "worst_bytes", "default_capacity")      # SG_JPEG_L_*, SG_JPEG_LAYOUT_WORDS
PNG_MAX_FRAMES = 16                  # SG_PNG_MAX_FRAMES
PNG_MAX_WIDTH = 10922                # SG_PNG_MAX_WIDTH
PNG_MAX_HEIGHT = 65535               # SG_PNG_MAX_HEIGHT
PNG_MAX_SEGMENT_BYTES = 32768        # SG_PNG_MAX_SEGMENT_BYTES
PNG_HEADER_BYTES = 47                # SG_PNG_HEADER_BYTES
PNG_TABLES = 5                       # SG_PNG_TABLES
PNG_TABLE_STRIDE = 520               # SG_PNG_TABLE_STRIDE
PNG_PREFIX_STRIDE = 48               # SG_PNG_PREFIX_STRIDE
PNG_T_PREFIX = 2600                  # SG_PNG_T_PREFIX
PNG_T_CRC = 2840                     # SG_PNG_T_CRC
PNG_T_POW = 3096                     # SG_PNG_T_POW
PNG_POW_WORDS = 20                   # SG_PNG_POW_WORDS
PNG_TABLE_WORDS = 3120               # SG_PNG_TABLE_WORDS
PNG_FILTER_ADAPTIVE = 5              # SG_PNG_FILTER_ADAPTIVE (0..4: SG_PNG_FILTER_NONE, _SUB, _UP, _AVERAGE, _PAETH)
PNG_LAYOUT = ("ws_bytes", "segments", "segment_bytes", "slot_pitch", "worst_bytes")      # SG_PNG_L_*, SG_PNG_LAYOUT_WORDS
UNPNG_MAX_STREAMS = 65535            # SG_UNPNG_MAX_STREAMS
UNPNG_MAX_ROW_BYTES = 16384          # SG_UNPNG_MAX_ROW_BYTES
UNPNG_MAX_HEIGHT = 65535             # SG_UNPNG_MAX_HEIGHT
UNPNG_TABLE_COLS = 6                 # SG_UNPNG_TABLE_COLS (SG_UNPNG_T_*: offset, length, width, height, channels, dest)
UNPNG_LAYOUT = ("ws_bytes", "slot_pitch")        # SG_UNPNG_L_*, SG_UNPNG_LAYOUT_WORDS
BODY_MAX_JOINTS = 64                 # SG_BODY_MAX_JOINTS
BODY_MAX_BETAS = 32                  # SG_BODY_MAX_BETAS
BODY_MAX_VERTS = 4194304             # SG_BODY_MAX_VERTS
BODY_MAX_ROWS = 1024                 # SG_BODY_MAX_ROWS
BODY_MAX_ITERATIONS = 64             # SG_BODY_MAX_ITERATIONS
BODY_INFO_INTS = 4                   # SG_BODY_INFO_INTS
BODY_ISOLATED, BODY_NOT_FINITE, BODY_BAD_SLOPE, BODY_BAD_FACE = 1, 2, 4, 8       # SG_BODY_ISOLATED, _NOT_FINITE, _BAD_SLOPE, _BAD_FACE
SIL_TILE = 16                        # SG_SIL_TILE
SIL_CHUNK = 256                      # SG_SIL_CHUNK
SIL_SORT_LDS = 1024                  # SG_SIL_SORT_LDS
SIL_MAX_FRAMES = 64                  # SG_SIL_MAX_FRAMES
SIL_GUARD_WORDS = 64                 # SG_SIL_GUARD_WORDS
SIL_INFO_WORDS = 4                   # SG_SIL_INFO_WORDS
SIL_POSE = 72                        # SG_SIL_POSE
SIL_LAYOUT = ("info", "rec", "rect", "tile_count", "tile_start", "cursor", "Q", "face_grad", "list", "partial", "bytes")    # SG_SIL_L_*, SG_SIL_LAYOUT_WORDS
FROZEN_BLOCK = 128                   # SG_FROZEN_BLOCK: points per workgroup of the fused no-gradient decode
FROZEN_SHS = 48                      # SG_FROZEN_SHS
MESH_TERMS_INFO_INTS = 2             # SG_MESH_TERMS_INFO_INTS
MESH_TERMS_BAD_LABEL = 1             # SG_MESH_TERMS_BAD_LABEL
MESH_TERMS_BAD_EDGE = 2              # SG_MESH_TERMS_BAD_EDGE
FLAG_SHORT_LISTS = 1                 # SG_FLAG_SHORT_LISTS
COUNT_FLAG_HALF_ROWS = 4             # SG_COUNT_FLAG_HALF_ROWS
COUNT_FLAG_HALF_LONG_ROWS = 8        # SG_COUNT_FLAG_HALF_LONG_ROWS
FLAG_WS_CLEAN = 2                    # SG_FLAG_WS_CLEAN
FLAG_THROUGHPUT = 4                  # SG_FLAG_THROUGHPUT
FLAG_FORWARD_BINNING = 8             # SG_FLAG_FORWARD_BINNING
FLAG_FORWARD_COMPOSITE = 16          # SG_FLAG_FORWARD_COMPOSITE
FLAG_SH_PLANAR = 32                  # SG_FLAG_SH_PLANAR
FLAG_LONG_ROWS = 64                  # SG_FLAG_LONG_ROWS
NUM_RENDERED_LONG_LIST = -2          # SG_NUM_RENDERED_LONG_LIST
# bits of the binning header's flag word (header word 1, set where sings_amd/csrc/sg_binning.hip writes `header[1] = hflags`,
# once per scan kernel): what the "async" / "deferred" checks read instead of the count NUM_RENDERED_LONG_LIST stands for
HDR_FLAG_OVERFLOW = 1               # more pairs than the capacity of the call
HDR_FLAG_LONG_LIST = 2              # a tile list longer than a flag of the call promised (SG_FLAG_SHORT_LISTS / SG_FLAG_LONG_ROWS)


def _ctypes_of(signature):
    """"i: S i p9" -> (c_int, [POINTER(SgRasterSettings), c_int, c_void_p x 9])."""
    ret, _, params = signature.partition(":")
    return _CTYPE[ret], [_CTYPE[t[0]] for t in params.split() for _ in range(int(t[1:] or 1))]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"sings_amd: HIP library not built ({LIB_PATH} missing). There is no CPU fallback; "
            "run `make -C sings_amd/csrc` (needs hipcc, --offload-arch=gfx950).")
    # The process must hold ONE HIP runtime: import torch first so that libamdhip64.so.7 resolves to the
    # copy PyTorch-ROCm already loaded (loading ours first makes the two runtimes disagree about devices).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    # (asked first, as the `int f(void)` ctypes assumes of an undeclared function: a library of another ABI may lack table entries)
    if lib.sg_abi_version() != ABI_VERSION:
        raise RuntimeError(f"sings_amd: {LIB_PATH} speaks ABI {lib.sg_abi_version()}, this host code ABI {ABI_VERSION} "
                           "(include/sings_hip.h SG_ABI_VERSION): rebuild with `make -C sings_amd/csrc`")
    # (SINGS_HIP_LIB may name a library that predates include/sings_order.h -- an A/B run against a parent build: it exports none of
    # that table, HAS_ORDER says so, and the engines then make the unordered calls that library knows)
    global HAS_ORDER, HAS_SAMPLER, HAS_FROZEN, HAS_FEED, HAS_DENSITY, HAS_SHEET, HAS_SCENE, HAS_JPEG, HAS_PNG, HAS_UNPNG, HAS_BODY, HAS_SILHOUETTE
    HAS_ORDER = all(hasattr(lib, name) for name in _PROTOTYPES_ORDER)
    HAS_SAMPLER = all(hasattr(lib, name) for name in _PROTOTYPES_SAMPLER)    # (the same, for include/sings_sampler.h)
    HAS_FROZEN = all(hasattr(lib, name) for name in _PROTOTYPES_FROZEN)      # (the same, for include/sings_frozen.h)
    HAS_FEED = all(hasattr(lib, name) for name in _PROTOTYPES_FEED)          # (the same, for include/sings_feed.h)
    HAS_DENSITY = all(hasattr(lib, name) for name in _PROTOTYPES_DENSITY)    # (the same, for include/sings_density.h)
    HAS_SHEET = all(hasattr(lib, name) for name in _PROTOTYPES_SHEET)        # (the same, for include/sings_sheet.h)
    HAS_SCENE = all(hasattr(lib, name) for name in _PROTOTYPES_SCENE)        # (the same, for include/sings_scene.h)
    HAS_JPEG = all(hasattr(lib, name) for name in _PROTOTYPES_JPEG)          # (the same, for include/sings_jpeg.h)
    HAS_PNG = all(hasattr(lib, name) for name in _PROTOTYPES_PNG)            # (the same, for include/sings_png.h)
    HAS_UNPNG = all(hasattr(lib, name) for name in _PROTOTYPES_UNPNG)        # (the same, for include/sings_unpng.h)
    HAS_BODY = all(hasattr(lib, name) for name in _PROTOTYPES_BODY)          # (the same, for include/sings_body.h)
    HAS_SILHOUETTE = all(hasattr(lib, name) for name in _PROTOTYPES_SILHOUETTE)      # (the same, for include/sings_silhouette.h)
    for has, header in ((HAS_ORDER, "sings_order.h"), (HAS_SAMPLER, "sings_sampler.h"), (HAS_FROZEN, "sings_frozen.h"),
                        (HAS_FEED, "sings_feed.h"), (HAS_DENSITY, "sings_density.h"), (HAS_SHEET, "sings_sheet.h"),
                        (HAS_SCENE, "sings_scene.h"), (HAS_JPEG, "sings_jpeg.h"), (HAS_PNG, "sings_png.h"),
                        (HAS_UNPNG, "sings_unpng.h"), (HAS_BODY, "sings_body.h"),
                        (HAS_SILHOUETTE, "sings_silhouette.h")):
        if not has and LIB_PATH == os.path.join(_HERE, "libsings_hip.so"):
            raise RuntimeError(f"sings_amd: {LIB_PATH} lacks the entry points of include/{header}: rebuild with `make -C sings_amd/csrc`")
    for name, signature in (*_PROTOTYPES.items(), *_PROTOTYPES_EVAL.items(), *_PROTOTYPES_MESH_TERMS.items(),
                            *(_PROTOTYPES_ORDER.items() if HAS_ORDER else ()), *(_PROTOTYPES_SAMPLER.items() if HAS_SAMPLER else ()),
                            *(_PROTOTYPES_FROZEN.items() if HAS_FROZEN else ()), *(_PROTOTYPES_FEED.items() if HAS_FEED else ()),
                            *(_PROTOTYPES_DENSITY.items() if HAS_DENSITY else ()),
                            *(_PROTOTYPES_SHEET.items() if HAS_SHEET else ()),
                            *(_PROTOTYPES_SCENE.items() if HAS_SCENE else ()),
                            *(_PROTOTYPES_JPEG.items() if HAS_JPEG else ()),
                            *(_PROTOTYPES_PNG.items() if HAS_PNG else ()),
                            *(_PROTOTYPES_UNPNG.items() if HAS_UNPNG else ()),
                            *(_PROTOTYPES_BODY.items() if HAS_BODY else ()),
                            *(_PROTOTYPES_SILHOUETTE.items() if HAS_SILHOUETTE else ())):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ctypes_of(signature)
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f"sings_hip {what} failed: {load().sg_last_error().decode()}")


def layout(P, W, H, cap):
    L = SgLayout()
    check(load().sg_layout(P, W, H, cap, C.byref(L)), "sg_layout")
    return L


def aux_layout(P, W, H, cap):
    """Bytes of one view's aux workspace (depth / alpha maps: sg_aux_layout)."""
    n = C.c_size_t(0)
    check(load().sg_aux_layout(P, W, H, cap, C.byref(n)), "sg_aux_layout")
    return int(n.value)


def frames_aux_layout(P, W, H, cap, K):
    """Bytes of the aux workspace of K frames (K consecutive single-view aux workspaces: sg_frames_aux_layout)."""
    n = C.c_size_t(0)
    check(load().sg_frames_aux_layout(P, W, H, cap, K, C.byref(n)), "sg_frames_aux_layout")
    return int(n.value)
