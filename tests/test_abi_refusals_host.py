"""The argument refusals of the C ABI, on the host: the library loads without a GPU and a refusal returns before any HIP call, so each
status-returning entry point of ``_lib._PROTOTYPES`` is called once with arguments it refuses, and the status (1) and the exact text of
``sg_last_error()`` are held.  The texts are behaviour: callers match on them and ``_lib.check`` puts them into the exception.

No call here reaches a launch: every row is refused by an argument check that stands in front of the entry point's first HIP call."""
import ctypes as C

import pytest

from sings_amd import _lib

# One refused call per entry point: {position: value} over a call whose other arguments are all 0 / 0.0 / NULL, and the text.
REFUSED = {
    "sg_layout": ({}, "sg_layout"),
    "sg_rasterize_forward": ({}, "sg_rasterize_forward: bad settings"),
    "sg_rasterize_backward": ({}, "sg_rasterize_backward: bad settings"),
    "sg_rasterize_backward_records": ({}, "sg_rasterize_backward_records: bad settings"),
    "sg_rasterize_backward_gaussians": ({}, "sg_rasterize_backward_gaussians: bad settings"),
    "sg_mark_visible": ({0: 1}, "sg_mark_visible: null pointer"),                       # (P <= 0 returns 0)
    "sg_read_num_rendered": ({}, "sg_read_num_rendered: null pointer"),
    "sg_signal_alloc": ({}, "sg_signal_alloc"),
    "sg_lbs_forward": ({1: 24}, "sg_lbs_forward: bad argument (1 <= J <= 64)"),
    "sg_lbs_backward": ({1: 24}, "sg_lbs_backward: bad argument (1 <= J <= 64)"),
    "sg_joint_transforms": ({0: 1, 1: 65}, "sg_joint_transforms: bad argument (1 <= J <= 64)"),
    "sg_joint_transforms_backward": ({0: 1, 1: 65}, "sg_joint_transforms_backward: bad argument (1 <= J <= 64)"),
    "sg_pose_transforms": ({0: 1, 1: 1, 2: 24, 3: 24},
                           "sg_pose_transforms: bad argument (1 <= J <= 64, 0 <= NBu <= 23, NBu < J; tail_pose for J - 1 - NBu "
                           "joints; transl and transl_out together)"),
    "sg_pose_transforms_backward": ({0: 1, 1: 1, 2: 24, 3: 24},
                                    "sg_pose_transforms_backward: bad argument (1 <= J <= 64, 0 <= NBu <= 23, NBu < J; d_transl_rows "
                                    "and d_transl together)"),
    "sg_matrix_to_quaternion": ({}, "sg_matrix_to_quaternion: bad argument"),
    "sg_matrix_to_quaternion_backward": ({}, "sg_matrix_to_quaternion_backward: bad argument"),
    "sg_rotation_convert": ({}, "sg_rotation_convert: bad argument"),
    "sg_rotation_convert_backward": ({}, "sg_rotation_convert_backward: bad argument"),
    "sg_quaternion_multiply": ({}, "sg_quaternion_multiply: bad argument"),
    "sg_quaternion_multiply_backward": ({}, "sg_quaternion_multiply_backward: bad argument"),
    "sg_skinned_forward": ({}, "sg_skinned_forward: bad settings"),
    "sg_skinned_backward": ({}, "sg_skinned_backward: bad settings"),
    "sg_skinned_backward_gaussians": ({}, "sg_skinned_backward_gaussians: bad settings"),
    "sg_frames_layout": ({0: 1, 1: 16, 2: 16, 4: 17}, "sg_frames_layout: K must be 1..16"),
    "sg_rasterize_forward_frames": ({}, "sg_rasterize_forward_frames: bad settings"),
    "sg_skinned_forward_frames": ({}, "sg_skinned_forward_frames: bad settings"),
    "sg_read_num_rendered_frames": ({}, "sg_read_num_rendered_frames: bad argument"),
    "sg_rasterize_backward_records_frames": ({}, "sg_rasterize_backward_records_frames: bad settings"),
    "sg_rasterize_backward_gaussians_frames": ({}, "sg_rasterize_backward_gaussians_frames: bad settings"),
    "sg_skinned_backward_gaussians_frames": ({}, "sg_skinned_backward_gaussians_frames: bad settings"),
    "sg_photo_loss_frames": ({0: 17, 1: 16, 2: 16}, "sg_photo_loss: bad image size / K not in 1..16"),
    "sg_photo_loss_backward_frames": ({0: 1, 1: 16, 2: 16},
                                      "sg_photo_loss_backward_frames: bad arguments (K in 1..16, no null pointers)"),
    "sg_photo_loss": ({0: 16, 1: 16}, "sg_photo_loss: null pointer"),
    "sg_photo_loss_backward": ({}, "sg_photo_loss_backward: bad image size"),
    "sg_region_laplacian": ({}, "sg_region_laplacian: bad argument"),
    "sg_rows_laplacian": ({}, "sg_rows_laplacian: bad argument"),
    "sg_mesh_edge_loss": ({}, "sg_mesh_edge_loss: bad argument"),
    "sg_l2norm_reg": ({}, "sg_l2norm_reg: bad argument"),
    "sg_gaussian_edge_loss": ({0: 4, 1: 5}, "sg_gaussian_edge_loss: bad argument (need N >= K)"),
    "sg_gaussian_edge_prepare": ({}, "sg_gaussian_edge_prepare: bad argument"),
    "sg_gaussian_edge_finish": ({0: 4, 1: 5}, "sg_gaussian_edge_finish: bad argument (need N >= K)"),
    "sg_triplane_forward": ({}, "sg_triplane_forward: bad plane description (feat must be 32, 1..4 scales)"),
    "sg_triplane_backward": ({}, "sg_triplane_backward: bad plane description"),
    "sg_triplane_backward_prepare": ({}, "sg_triplane_backward_prepare: bad plane description"),
    "sg_triplane_backward_prepared": ({}, "sg_triplane_backward_prepared: bad plane description"),
    "sg_bias_act_forward": ({0: 1, 1: 32, 2: 4}, "sg_bias_act_forward: bad argument"),
    "sg_bias_act_backward": ({0: 1, 1: 129}, "sg_bias_act_backward: bad argument (C <= 128)"),
    "sg_scales_head_forward": ({}, "sg_scales_head_forward: bad argument"),
    "sg_scales_head_backward": ({}, "sg_scales_head_backward: bad argument"),
    "sg_linear_forward": ({0: 1, 1: 32, 2: 32, 3: 4}, "sg_linear_forward: bad argument"),
    "sg_linear_backward": ({}, "sg_linear_backward: bad argument"),
    "sg_linear_backward_accumulate": ({}, "sg_linear_backward_accumulate: bad argument"),
    "sg_linear_backward_fan": ({}, "sg_linear_backward_fan: bad argument"),
    "sg_weight_grad": ({}, "sg_weight_grad: bad argument"),
    "sg_aux_layout": ({0: 1, 1: 16, 2: 16}, "sg_aux_layout"),
    "sg_rasterize_forward_aux": ({}, "sg_rasterize_forward_aux: null pointer (aux_ws)"),
    "sg_rasterize_backward_aux": ({}, "sg_rasterize_backward_aux: bad settings"),
    "sg_skinned_forward_aux": ({}, "sg_skinned_forward_aux: null pointer (aux_ws)"),
    "sg_skinned_backward_aux": ({}, "sg_skinned_backward_aux: bad settings"),
    "sg_frames_aux_layout": ({0: 1, 1: 16, 2: 16, 4: 2}, "sg_frames_aux_layout: null pointer"),
    "sg_skinned_forward_frames_aux": ({}, "sg_skinned_forward_frames_aux: null pointer (aux_ws)"),
    "sg_rasterize_backward_records_frames_aux": ({}, "sg_rasterize_backward_records_frames_aux: bad settings"),
    "sg_skinned_backward_gaussians_frames_aux": ({}, "sg_skinned_backward_gaussians_frames_aux: bad settings"),
    "sg_lpips_weights_layout": ({}, "sg_lpips_weights_layout: null pointer"),
    "sg_lpips_ws_bytes": ({0: 1, 1: 16, 2: 16}, "sg_lpips_ws_bytes: null pointer"),
    "sg_lpips_ws_layout": ({0: 1, 1: 16, 2: 16}, "sg_lpips_ws_layout: null pointer"),
    "sg_lpips_forward": ({0: 1, 1: 15, 2: 16}, "sg_lpips_forward: B must be >= 1, H and W >= 16 (and 2 B H W 64 < 2^31)"),
    "sg_lpips_backward": ({0: 1, 1: 16, 2: 16}, "sg_lpips_backward: null pointer"),
    "sg_lpips_patch_gather": ({}, "sg_lpips_patch_gather: bad sizes (K, n >= 1, 1 <= patch <= H, W)"),
    "sg_lpips_patch_scatter": ({}, "sg_lpips_patch_scatter: bad sizes (K, n >= 1, 1 <= patch <= H, W)"),
    "sg_frames_to_u8": ({}, "sg_frames_to_u8: K must be 1..65535"),
    "sg_adam_step": ({}, "sg_adam_step: n_segments, n_chunks must be >= 0 (chunks need a segment), n_groups >= 1"),
    "sg_mesh_edges_build": ({0: 3, 1: 1}, "sg_mesh_edges_build: null pointer"),
    "sg_mesh_edges_emit": ({0: 3, 1: 1, 2: 4}, "sg_mesh_edges_emit: E must be 0 .. 3 F"),        # (F == 0 returns 0)
    "sg_mesh_subdivide": ({0: 3, 1: 1, 2: 2}, "sg_mesh_subdivide: Fs must be 0 .. F"),           # (F == 0 returns 0)
    "sg_mesh_midpoints": ({}, "sg_mesh_midpoints: V, E >= 0 and C >= 1"),
    "sg_mesh_midpoints_i32": ({}, "sg_mesh_midpoints: V, E >= 0 and C >= 1"),             # (the shared check names the float variant)
    "sg_mesh_collapse_build": ({}, "sg_mesh_collapse: V must be >= 1"),
    "sg_mesh_collapse_emit": ({0: 3, 1: 1, 2: 2}, "sg_mesh_collapse_emit: Fn must be 0 .. F and Vn 0 .. V"),
    "sg_init_attributes": ({}, "sg_init_attributes: 1 <= V <= 2^30, 0 <= F <= (2^31 - 1) / 3, E >= 0"),
    "sg_attr_mse": ({}, "sg_attr_mse: 1 <= N <= 2^30"),
    "sg_plateau_step": ({}, "sg_plateau_step: 1 <= n_groups <= 64, patience >= 0, 0 <= n_copy <= 64, log_rows >= 0"),
    "sg_copy_probe": ({}, "sg_copy_probe: 16-byte aligned buffers and a multiple of 16 bytes"),
    "sg_profile_collect": ({}, "sg_profile_collect"),
}

# Entry points that return an int and have no argument refusal in front of their first HIP runtime call.
NOT_REFUSING = {
    "sg_abi_version": "returns the ABI number, not a status",
    "sg_mesh_collapse_max_edges": "returns a constant, not a status",
    "sg_signal_free": "NULL returns 0, anything else goes straight to hipHostFree",
    "sg_profile_enable": "sets a flag and returns 0 for every argument",
}


def test_the_table_covers_every_status_returning_entry_point():
    status = {name for name, sig in _lib._PROTOTYPES.items() if sig.startswith("i:")}
    assert not set(REFUSED) & set(NOT_REFUSING)
    assert set(REFUSED) | set(NOT_REFUSING) == status


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusal_status_and_text(name):
    lib = _lib.load()
    overrides, text = REFUSED[name]
    _, argtypes = _lib._ctypes_of(_lib._PROTOTYPES[name])
    args = [0.0 if t is C.c_float else 0 if t in (C.c_int, C.c_size_t) else None for t in argtypes]
    for position, value in overrides.items():
        assert argtypes[position] is C.c_int                       # (the table overrides sizes only: every pointer stays NULL)
        args[position] = value
    assert getattr(lib, name)(*args) == 1
    assert lib.sg_last_error().decode() == text + ": invalid argument"
