"""Fused "posed-frame" operator: SMPL-LBS deformation of canonical Gaussians + rasterization.

Opt-in replacement of the LBS block of ``SinGS.forward`` (sings/rec/models/sings_hybrid.py:398-428)
followed by ``get_render_pkg`` (sings/rec/renderer/gs_renderer_single.py:12-42): the caller hands over
canonical means / rotations / scales, the skinning weights and the cano->pose joint transforms
``A_cano2pose = A_t2pose @ inv_A_t2cano`` (:398-399); posed means, rotation quaternions and the
blended T[N,4,4] never reach HBM.  Gradients flow to xyz_canon, rotmat_canon, scales, opacity, shs,
``A`` (hence body_pose / global_orient through the SMPL chain in torch) and ``transl``.

Pair capacity, overflow check and the learned long-rows hint: ``sings_amd.overflow`` (``run_forward``), the same policy as the
drop-in rasterizer's, with the per-op differences spelled out at the two calls below.  The skin inputs and the frame batch of a
call are filled by sings_amd/_marshal.py (``_skin_struct``, ``_skin_frames``), shared with the engines.
"""
import ctypes as C

import torch

from . import _lib, overflow
from ._marshal import _camera_stride, _f32, _ptr, _settings_struct, _skin_frames, _skin_struct, _stream


def _canonical_inputs(xyz_canon, rotmat_canon, scales, opacities, shs):
    """The canonical Gaussians of both skinned ops, checked and converted: (device, xyz_canon, rotmat_canon as the kernels read it
    -- None, [N,9] or [N,6] --, the shape rotmat_canon came in (its gradient's), scales, opacities, shs)."""
    dev = xyz_canon.device
    if dev.type != "cuda":
        raise RuntimeError("sings_amd fused LBS+raster runs on the MI355X only; there is no CPU fallback")
    xyz_canon = _f32(xyz_canon, "xyz_canon", dev)
    rot_shape = None if rotmat_canon is None else tuple(rotmat_canon.shape)
    if rotmat_canon is not None:
        rotmat_canon = _f32(rotmat_canon, "rotmat_canon", dev)
        if rotmat_canon.shape[-2:] == (3, 3):
            rotmat_canon = rotmat_canon.reshape(-1, 9)
        elif rotmat_canon.dim() != 2 or rotmat_canon.shape[1] not in (6, 9):
            raise RuntimeError(f"rotmat_canon must be [N,3,3], [N,9] or [N,6] (6-D form), got {tuple(rotmat_canon.shape)}")
    return (dev, xyz_canon, rotmat_canon, rot_shape, _f32(scales, "scales", dev), _f32(opacities, "opacities", dev),
            _f32(shs, "shs", dev))


class _RasterizeSkinnedGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_canon, rotmat_canon, scales, opacities, shs, A, transl, lbs_weights, smpl_scale, ext_tfs,
                raster_settings, return_posed, means2D=None, return_aux=False):
        lib = _lib.load()
        dev, xyz_canon, rotmat_canon, rot_shape, scales, opacities, shs = _canonical_inputs(xyz_canon, rotmat_canon, scales,
                                                                                            opacities, shs)
        if return_aux:
            ctx.set_materialize_grads(False)
        rs = raster_settings
        P = int(xyz_canon.shape[0]); H, W = int(rs.image_height), int(rs.image_width); M = int(shs.shape[1])
        keep = []
        s = _settings_struct(rs, dev, M, keep)
        k = _skin_struct(dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, keep)
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        pxyz, pq, psc = (e(P, 3), e(P, 4), e(P, 3)) if return_posed else (None, None, None)
        depth, alpha = (e(1, H, W), e(1, H, W)) if return_aux else (None, None)
        stream = _stream(dev)
        geom = binning = img = aux = None

        def launch(cap, flags, sync):
            nonlocal geom, binning, img, aux
            s.flags = flags
            L = _lib.layout(P, W, H, cap)
            geom = torch.empty(L.geom_bytes, dtype=torch.uint8, device=dev)
            binning = torch.empty(L.bin_bytes, dtype=torch.uint8, device=dev)
            img = torch.empty(L.img_bytes, dtype=torch.uint8, device=dev)
            nr = C.c_int64(0)
            args = (C.byref(s), P, C.byref(k), _ptr(shs), _ptr(opacities), _ptr(scales), _ptr(geom), _ptr(binning), cap, _ptr(img),
                    _ptr(color), _ptr(radii), _ptr(pxyz), _ptr(pq), _ptr(psc), C.byref(nr) if sync else None)
            if return_aux:
                aux = torch.empty(_lib.aux_layout(P, W, H, cap), dtype=torch.uint8, device=dev)
                _lib.check(lib.sg_skinned_forward_aux(*args, _ptr(aux), _ptr(depth), _ptr(alpha), stream),
                           "skinned forward (depth / alpha maps)")
            else:
                _lib.check(lib.sg_skinned_forward(*args, stream), "skinned forward")
            return (int(nr.value),) if sync else None

        cap, counts = overflow.run_forward(
            dev, P, W, H, s, launch, lambda: binning[:8].view(torch.int32), debug=rs.debug,
            hints=(_lib.FLAG_LONG_ROWS,),     # avatar frames are images of few tiles: only the long-rows hint applies
            hints_need_sync=False,            # in every mode / under capture: a violated hint is reported like an overflow there
            early_count=True)                 # "sync" forwards read R from the early-count word and learn the hints from it
        R = None if counts is None else counts[0]
        ctx.rs, ctx.cap, ctx.M, ctx.num_rendered = rs, cap, M, R
        ctx.has_rot = rotmat_canon is not None
        ctx.has_ext = ext_tfs is not None
        ctx.rot_shape = rot_shape
        ctx.has_m2d = means2D is not None
        ctx.return_posed = return_posed
        ctx.return_aux = return_aux
        ctx.aux_ws = aux
        ctx.aux = (lbs_weights, smpl_scale, A.shape, None if transl is None else transl.shape)
        z = torch.empty(0, device=dev)
        ctx.save_for_backward(xyz_canon, rotmat_canon if ctx.has_rot else z, scales, opacities, shs,
                              _f32(A, "A", dev), transl if transl is not None else z, radii, geom, binning, img)
        ctx.mark_non_differentiable(radii)
        out = (color, radii)
        if return_posed:
            ctx.mark_non_differentiable(psc)
            out += (pxyz, pq, psc)
        if return_aux:
            out += (depth, alpha)
        return out

    @staticmethod
    def backward(ctx, g_color, _g_radii=None, *g_rest):
        g_rest = g_rest + (None,) * 5
        g_pxyz, g_pq = g_rest[:2] if ctx.return_posed else (None, None)
        g_depth, g_alpha = g_rest[3:5] if ctx.return_posed else g_rest[:2]
        if not ctx.return_aux:
            g_depth = g_alpha = None
        lib = _lib.load()
        if ctx.has_ext:
            raise RuntimeError("ext_tfs are forward-only (the reference applies them under no_grad: anim_avatar.py:27)")
        xyz_canon, rotmat_canon, scales, opacities, shs, A, transl, radii, geom, binning, img = ctx.saved_tensors
        lbs_weights, smpl_scale, A_shape, transl_shape = ctx.aux
        dev = xyz_canon.device
        rs = ctx.rs
        P = int(xyz_canon.shape[0]); H, W = int(rs.image_height), int(rs.image_width)
        keep = []
        s = _settings_struct(rs, dev, ctx.M, keep)
        k = _skin_struct(dev, xyz_canon, rotmat_canon if ctx.has_rot else None, lbs_weights, A, smpl_scale,
                         transl if transl_shape is not None else None, None, keep)
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        d_xyz, d_scales, d_op, d_sh, d_m2d = e(P, 3), e(P, 3), e(P, 1), e(P, ctx.M, 3), e(P, 3)
        d_rot = e(P, int(rotmat_canon.shape[1])) if ctx.has_rot else None
        d_A = e(k.J, 16); d_tr = e(3)
        g_color = (torch.zeros((3, H, W), dtype=torch.float32, device=dev) if g_color is None
                   else _f32(g_color, "grad_out_color", dev))
        g_depth = None if g_depth is None else _f32(g_depth, "grad_depth", dev)
        g_alpha = None if g_alpha is None else _f32(g_alpha, "grad_alpha", dev)
        g_pxyz = None if g_pxyz is None else _f32(g_pxyz, "grad posed xyz", dev)
        g_pq = None if g_pq is None else _f32(g_pq, "grad posed rotq", dev)
        with torch.cuda.device(dev):
            L = _lib.layout(P, W, H, ctx.cap)
            bwd_ws = torch.empty(L.bwd_bytes, dtype=torch.uint8, device=dev)
            skin_ws = e(int(lib.sg_skin_ws_floats(P)))
            stream = _stream(dev)
            args = (C.byref(s), P, C.byref(k), _ptr(shs), _ptr(opacities), _ptr(scales), _ptr(radii), _ptr(geom),
                    _ptr(binning), ctx.cap, _ptr(img), _ptr(bwd_ws), _ptr(skin_ws), _ptr(g_color), _ptr(g_pxyz), _ptr(g_pq),
                    _ptr(d_xyz), _ptr(d_rot), _ptr(d_scales), _ptr(d_op), _ptr(d_sh), _ptr(d_m2d), _ptr(d_A), _ptr(d_tr))
            if g_depth is None and g_alpha is None:     # neither map carries a gradient: the plain backward, bit for bit
                _lib.check(lib.sg_skinned_backward(*args, stream), "skinned backward")
            else:
                _lib.check(lib.sg_skinned_backward_aux(*args, _ptr(ctx.aux_ws), _ptr(g_depth), _ptr(g_alpha), stream),
                           "skinned backward (depth / alpha maps)")
        return (d_xyz, None if d_rot is None else d_rot.view(ctx.rot_shape), d_scales, d_op.view_as(opacities), d_sh,
                d_A.view(A_shape), None if transl_shape is None else d_tr.view(transl_shape), None, None, None, None, None,
                d_m2d if ctx.has_m2d else None, None)


def rasterize_skinned_gaussians(xyz_canon, rotmat_canon, scales, opacities, shs, lbs_weights, A_cano2pose,
                                raster_settings, smpl_scale=None, transl=None, ext_tfs=None, return_posed=False,
                                means2D=None, return_aux=False):
    """color, radii[, posed_xyz, posed_rotq, posed_scales][, depth, alpha] = fused LBS + rasterization of one posed frame.

    ``rotmat_canon=None`` means isotropic Gaussians (identity canonical rotation, sings_hybrid.py:358-361); a ``[N,6]``
    tensor is the geometry decoder's 6-D output: ``rotation_6d_to_matrix`` (sings_hybrid.py:356-357) is then evaluated
    inside the kernels, forward and backward, and the gradient comes back in 6-D form.
    ``means2D``: optional ``[N,3]`` tensor with ``requires_grad`` (values unused) that receives the screen-space
    gradient the densifier reads as ITS gradient -- the reference's ``viewspace_points`` idiom
    (gs_renderer_single.py:50-56, consumer sings_hybrid.py:1013-1015), one holder per call, so several views of a
    step keep their own statistics.
    ``return_aux``: also the accumulated depth sum_i z_i alpha_i T_i and the alpha map 1 - T_final, both [1,H,W] and
    differentiable (expected depth = depth / alpha), appended at the end of the outputs.
    """
    return _RasterizeSkinnedGaussians.apply(xyz_canon, rotmat_canon, scales, opacities, shs, A_cano2pose, transl,
                                            lbs_weights, smpl_scale, ext_tfs, raster_settings, return_posed, means2D,
                                            return_aux)


class _RasterizeSkinnedFrames(torch.autograd.Function):
    """K posed frames of the SAME canonical Gaussians in ONE call per direction (the ``*_frames`` entry points of
    include/sings_hip.h): what ``SinGS.forward_chunk`` (sings_hybrid.py:474-569) + the render loop of gs_trainer.py:684-714 do for
    a chunk, as one differentiable operator.  The gradients of the canonical Gaussians are the SUM over the K frames (formed inside
    the per-Gaussian backward kernel, in frame order); dL/dA and dL/dtransl are per frame.  The pair counts of the K frames are read
    before the call returns (one strided copy + stream synchronisation): a frame that would overflow is never returned, the
    workspaces grow and the call is repeated.  With ``set_overflow_check("deferred")`` or inside a HIP-graph capture nothing is
    read on the host: the largest (pair count, overflow flag) of the K frames is folded into the device-side accumulator that
    ``check_deferred_overflow()`` polls, exactly as the single-frame operator does.  ``return_aux``: also the K frames' depth and
    alpha maps (the ``*_frames_aux`` entry points), bit for bit those of K single-frame ``return_aux`` calls."""

    @staticmethod
    def forward(ctx, xyz_canon, rotmat_canon, scales, opacities, shs, A, transl, lbs_weights, smpl_scale, raster_settings,
                means2D=None, return_aux=False):
        lib = _lib.load()
        dev, xyz_canon, rotmat_canon, rot_shape, scales, opacities, shs = _canonical_inputs(xyz_canon, rotmat_canon, scales,
                                                                                            opacities, shs)
        if return_aux:
            ctx.set_materialize_grads(False)
        rs = raster_settings
        A = _f32(A, "A", dev)
        K = int(A.shape[0])
        if A.dim() < 3 or not 1 <= K <= _lib.MAX_FRAMES:
            raise RuntimeError(f"A must be [K,J,4,4] / [K,J,16] with K in 1..{_lib.MAX_FRAMES}, got {tuple(A.shape)}")
        A16 = A.reshape(K, -1, 16)
        transl = _f32(transl, "transl", dev)
        cam_stride = _camera_stride(rs, K, RuntimeError)
        P = int(xyz_canon.shape[0]); H, W = int(rs.image_height), int(rs.image_width); M = int(shs.shape[1])
        keep = []
        s = _settings_struct(rs, dev, M, keep)
        k, fb, _ = _skin_frames(dev, xyz_canon, rotmat_canon, lbs_weights, A16, smpl_scale, transl, None, cam_stride, keep,
                                RuntimeError)
        color = torch.empty((K, 3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((K, P), dtype=torch.int32, device=dev)
        depth, alpha = ((torch.empty((K, 1, H, W), dtype=torch.float32, device=dev),
                         torch.empty((K, 1, H, W), dtype=torch.float32, device=dev)) if return_aux else (None, None))
        stream = _stream(dev)
        L = geom = binning = img = sizes = aux = None

        def launch(cap, flags, sync):
            nonlocal L, geom, binning, img, sizes, aux
            s.flags = flags
            L = _lib.SgLayout(); sizes = [C.c_size_t() for _ in range(4)]
            _lib.check(lib.sg_frames_layout(P, W, H, cap, K, C.byref(L), *[C.byref(x) for x in sizes]), "sg_frames_layout")
            geom = torch.empty(sizes[0].value, dtype=torch.uint8, device=dev)
            binning = torch.empty(sizes[1].value, dtype=torch.uint8, device=dev)
            img = torch.empty(sizes[2].value, dtype=torch.uint8, device=dev)
            nr = (C.c_int64 * K)()
            args = (C.byref(s), C.byref(fb), P, C.byref(k), _ptr(shs), _ptr(opacities), _ptr(scales), _ptr(geom), _ptr(binning), cap,
                    _ptr(img), _ptr(color), _ptr(radii), None, None, None, nr if sync else None)
            if return_aux:
                aux = torch.empty(_lib.frames_aux_layout(P, W, H, cap, K), dtype=torch.uint8, device=dev)
                _lib.check(lib.sg_skinned_forward_frames_aux(*args, _ptr(aux), _ptr(depth), _ptr(alpha), stream),
                           "skinned forward (frames, depth / alpha maps)")
            else:
                _lib.check(lib.sg_skinned_forward_frames(*args, stream), "skinned forward (frames)")
            return [int(v) for v in nr] if sync else None

        # (unread: the largest pair count and the OR of the K frames' flag words go to the check of the single-frame op)
        cap, nr = overflow.run_forward(
            dev, P, W, H, s, launch, lambda: overflow.frames_header(binning, K, L.bin_bytes), debug=rs.debug,
            base_flags=_lib.FLAG_THROUGHPUT,  # K frames share the GPU: long tile lists are not split over workgroups
            hints=(_lib.FLAG_LONG_ROWS,),     # avatar frames are images of few tiles: only the long-rows hint applies
            hints_need_sync=False,            # in every mode / under capture: a violated hint is reported like an overflow there
            early_count=False)                # one early-count word holds one frame's count: the K counts are read after the call
        if nr is None:
            nr = [0] * K
        ctx.rs, ctx.cap, ctx.M, ctx.K, ctx.fb = rs, cap, M, K, (cam_stride, fb.transl_stride)
        ctx.num_rendered = [int(v) for v in nr]
        ctx.has_rot = rotmat_canon is not None
        ctx.rot_shape = rot_shape
        ctx.has_m2d = means2D is not None
        ctx.return_aux = return_aux
        ctx.aux_ws = aux
        ctx.aux = (lbs_weights, smpl_scale, A.shape, None if transl is None else transl.shape, sizes[3].value)
        z = torch.empty(0, device=dev)
        ctx.save_for_backward(xyz_canon, rotmat_canon if ctx.has_rot else z, scales, opacities, shs, A16,
                              transl if transl is not None else z, radii, geom, binning, img)
        ctx.mark_non_differentiable(radii)
        if return_aux:
            return color, radii, depth, alpha
        return color, radii

    @staticmethod
    def backward(ctx, g_color, _g_radii=None, g_depth=None, g_alpha=None):
        lib = _lib.load()
        xyz_canon, rotmat_canon, scales, opacities, shs, A16, transl, radii, geom, binning, img = ctx.saved_tensors
        lbs_weights, smpl_scale, A_shape, transl_shape, bwd_bytes = ctx.aux
        dev = xyz_canon.device
        rs, K = ctx.rs, ctx.K
        P = int(xyz_canon.shape[0]); H, W = int(rs.image_height), int(rs.image_width)
        keep = []
        s = _settings_struct(rs, dev, ctx.M, keep)
        s.flags = _lib.FLAG_THROUGHPUT
        k, fb, _ = _skin_frames(dev, xyz_canon, rotmat_canon if ctx.has_rot else None, lbs_weights, A16, smpl_scale,
                                transl if transl_shape is not None else None, None, ctx.fb[0], keep, RuntimeError)
        e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
        d_xyz, d_scales, d_op, d_sh, d_m2d = e(P, 3), e(P, 3), e(P, 1), e(P, ctx.M, 3), e(K, P, 3)
        d_rot = e(P, int(rotmat_canon.shape[1])) if ctx.has_rot else None
        d_A = e(K, k.J, 16); d_tr = e(K, 3)
        g_color = (torch.zeros((K, 3, H, W), dtype=torch.float32, device=dev) if g_color is None
                   else _f32(g_color, "grad_out_color", dev))
        if not ctx.return_aux:
            g_depth = g_alpha = None
        g_depth = None if g_depth is None else _f32(g_depth, "grad_depth", dev)
        g_alpha = None if g_alpha is None else _f32(g_alpha, "grad_alpha", dev)
        aux = g_depth is not None or g_alpha is not None     # neither map carries a gradient: the plain backward, bit for bit
        with torch.cuda.device(dev):
            bwd_ws = torch.empty(bwd_bytes, dtype=torch.uint8, device=dev)
            skin_ws = e(int(lib.sg_skin_ws_floats_frames(P, K)))
            stream = _stream(dev)
            rec = (C.byref(s), C.byref(fb), P, _ptr(geom), _ptr(binning), ctx.cap, _ptr(img), _ptr(bwd_ws), _ptr(g_color))
            gau = (C.byref(s), C.byref(fb), P, C.byref(k), _ptr(shs), _ptr(opacities), _ptr(scales), _ptr(radii), _ptr(geom), _ptr(binning),
                   ctx.cap, _ptr(bwd_ws), _ptr(skin_ws), 0, None, None, _ptr(d_xyz), _ptr(d_rot), _ptr(d_scales), _ptr(d_op), _ptr(d_sh),
                   _ptr(d_m2d), _ptr(d_A), _ptr(d_tr))
            if aux:
                _lib.check(lib.sg_rasterize_backward_records_frames_aux(*rec, _ptr(ctx.aux_ws), _ptr(g_depth), _ptr(g_alpha), stream),
                           "skinned backward (records, frames, depth / alpha maps)")
                _lib.check(lib.sg_skinned_backward_gaussians_frames_aux(*gau, _ptr(ctx.aux_ws), stream),
                           "skinned backward (gaussians, frames, depth / alpha maps)")
            else:
                _lib.check(lib.sg_rasterize_backward_records_frames(*rec, stream), "skinned backward (records, frames)")
                _lib.check(lib.sg_skinned_backward_gaussians_frames(*gau, stream), "skinned backward (gaussians, frames)")
        if transl_shape is None:
            g_tr = None
        elif ctx.fb[1] == 3:
            g_tr = d_tr.view(transl_shape)
        else:
            g_tr = d_tr.sum(0).view(transl_shape)                 # one translation shared by the K frames
        return (d_xyz, None if d_rot is None else d_rot.view(ctx.rot_shape), d_scales, d_op.view_as(opacities), d_sh,
                d_A.view(A_shape), g_tr, None, None, None, d_m2d if ctx.has_m2d else None, None)


def rasterize_skinned_frames(xyz_canon, rotmat_canon, scales, opacities, shs, lbs_weights, A_cano2pose, raster_settings,
                             smpl_scale=None, transl=None, means2D=None, return_aux=False):
    """color [K,3,H,W], radii [K,P] = fused LBS + rasterization of K posed frames of the same canonical Gaussians in one call.

    ``A_cano2pose`` [K,J,4,4]; ``transl`` [K,3] (per frame), [3] (shared) or None; ``raster_settings``: one camera, or
    ``viewmatrix`` / ``projmatrix`` [K,4,4] and ``campos`` [K,3] for a camera per frame.  ``means2D``: optional [K,N,3] holder
    (``requires_grad``) of the per-frame screen-space gradients.  Backward: canonical-Gaussian gradients summed over the K frames.
    ``return_aux``: color, radii, depth [K,1,H,W], alpha [K,1,H,W] -- every frame's accumulated depth sum_i z_i alpha_i T_i and alpha
    map 1 - T_final, differentiable (``rasterize_skinned_gaussians(return_aux=True)`` per frame)."""
    return _RasterizeSkinnedFrames.apply(xyz_canon, rotmat_canon, scales, opacities, shs, A_cano2pose, transl, lbs_weights,
                                         smpl_scale, raster_settings, means2D, return_aux)
