"""How tensors, cameras, skin inputs and frame batches become arguments of the C ABI (``_lib._PROTOTYPES``).

The one place that knows it: the drop-in op (rasterizer.py), the skinned ops (skinned.py), the pre-allocated engines (engine.py)
and every other caller of the library take these functions from here.  Imports ``_lib`` only, so nothing above it can form an
import cycle through it.  What a caller converts or refuses before it gets here (``_f32`` or ``.contiguous().float()``) and the
exception type of a malformed input are the caller's: they differ between the ops and the engines.
"""
import ctypes as C

import torch

from . import _lib


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _stream(dev):
    """The ``void *stream`` argument: torch's current HIP stream on ``dev``."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(t, name, dev):
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.device != dev:
        raise RuntimeError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


def _settings_struct(rs, dev, sh_coeffs, keep):
    bg = _f32(rs.bg, "bg", dev); vm = _f32(rs.viewmatrix, "viewmatrix", dev)
    pm = _f32(rs.projmatrix, "projmatrix", dev); cp = _f32(rs.campos, "campos", dev)
    keep.extend([bg, vm, pm, cp])
    s = _lib.SgRasterSettings()
    s.image_height = int(rs.image_height); s.image_width = int(rs.image_width)
    s.tanfovx = float(rs.tanfovx); s.tanfovy = float(rs.tanfovy)
    s.scale_modifier = float(rs.scale_modifier)
    s.sh_degree = int(rs.sh_degree); s.sh_coeffs = int(sh_coeffs)
    s.prefiltered = int(bool(rs.prefiltered)); s.debug = int(bool(rs.debug)); s.flags = 0
    s.bg = bg.data_ptr(); s.viewmatrix = vm.data_ptr(); s.projmatrix = pm.data_ptr(); s.campos = cp.data_ptr()
    s.count_signal = None; s.count_signal_host = None
    return s


def _camera_stride(rs, K, error):
    """SgFrameBatch.camera_stride of K frames: 0, one camera for all of them ([4,4] matrices), or 1, one per frame (``viewmatrix`` /
    ``projmatrix`` [K,4,4], ``campos`` [K,3]).  ``error``: the exception class of the caller for cameras stacked otherwise."""
    if rs.viewmatrix.dim() != 3:
        return 0
    if rs.viewmatrix.shape[0] != K or rs.projmatrix.shape[0] != K or rs.campos.shape[0] != K:
        raise error(f"per-frame cameras must be stacked [{K},4,4] / [{K},3]")
    return 1


def _skin_struct(dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, keep, J=None):
    """rotmat_canon: None (isotropic), [N,9] / [N,3,3] rotation matrices, or [N,6] in the decoder's 6-D form
    (rotation_6d_to_matrix then runs inside the kernels).  ``J``: None, ``A`` holds the joints of ONE frame; else ``A`` (and
    ``transl``) are the stacked frames of a K-frame call, J joints each, and the struct points at their first frame."""
    k = _lib.SgSkinInputs()
    A = _f32(A, "A", dev).reshape(-1, 16)
    k.J = int(A.shape[0]) if J is None else int(J)
    k.rot_format = 1 if (rotmat_canon is not None and rotmat_canon.shape[-1] == 6 and rotmat_canon.dim() == 2) else 0
    lbs_weights = _f32(lbs_weights, "lbs_weights", dev)
    if lbs_weights.shape != (xyz_canon.shape[0], k.J):
        raise RuntimeError(f"lbs_weights must be [N,{k.J}], got {tuple(lbs_weights.shape)}")
    ts = [xyz_canon, rotmat_canon, lbs_weights, A,
          None if smpl_scale is None else _f32(smpl_scale, "smpl_scale", dev).reshape(-1),
          None if transl is None else _f32(transl, "transl", dev).reshape(-1)]
    if ext_tfs is not None:
        tr, rm, sc = ext_tfs
        ts += [_f32(tr, "ext trans", dev).reshape(-1), _f32(rm, "ext rotmat", dev).reshape(-1),
               _f32(sc, "ext scale", dev).reshape(-1)]
    else:
        ts += [None, None, None]
    keep.extend(ts)
    for name, t in zip(("xyz_canon", "rot_canon", "lbs_weights", "A", "smpl_scale", "transl", "ext_trans", "ext_rot",
                        "ext_scale"), ts):
        setattr(k, name, None if t is None else t.data_ptr())
    return k


def _frame_batch(K, camera_stride, transl_stride, placement=0):
    fb = _lib.SgFrameBatch()
    fb.K, fb.camera_stride, fb.transl_stride, fb.placement = int(K), int(camera_stride), int(transl_stride), int(placement)
    return fb


def _frame_rows(t, K, width, name):
    """An input of K frames that may be shared -> (tensor, per_frame): ONE set of ``width`` floats for every frame (``width``
    elements -- a leading 1 included -- or an ``.expand`` view, stride 0 along the frames: its first row, not copied), or K rows
    [K, width] (per_frame True)."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.numel() == width:
        return t.reshape(width), False
    if t.dim() >= 1 and t.shape[0] == K and t[0].numel() == width:
        if t.stride(0) == 0:
            return t[0].reshape(width), False
        return t.reshape(K, width), True
    raise ValueError(f"{name} must be [{width}] (one for all frames) or [{K},{width}] (one per frame), got {tuple(t.shape)}")


def _skin_frames(dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, camera_stride, keep, error,
                 placement=0):
    """The skin inputs and the frame batch of a K-frame call -> (SgSkinInputs, SgFrameBatch, forward_only).  ``A``: [K,J,16];
    ``transl``: None, 3 floats shared by the frames (``transl_stride`` 0) or 3 per frame (3), anything else raises ``error``;
    ``placement``: the SG_PLACEMENT_* bits of a caller that hands over ``smpl_scale`` / ``ext_tfs`` as one set per frame.
    ``forward_only``: the frames carry ext_tfs or per-frame sets, which have no backward (the reference applies them under
    no_grad)."""
    K, J = int(A.shape[0]), int(A.shape[1])
    tstride = 0
    if transl is not None and transl.numel() != 3:
        if transl.numel() != 3 * K:
            raise error(f"transl must be [{K},3] or [3], got {tuple(transl.shape)}")
        tstride = 3
    k = _skin_struct(dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, keep, J=J)
    return k, _frame_batch(K, camera_stride, tstride, placement), ext_tfs is not None or bool(placement)


def adam_step(segments, chunks, hyper, grad_flat, exp_avg, exp_avg_sq):
    """``sg_adam_step`` on torch's current stream: ``segments`` [S,4] int64, ``chunks`` [C,2] int32 and ``hyper`` [G,8] fp32 are
    device tensors (``sings_amd.optim.build_tables`` / ``hyper_row``), the other three the flat fp32 buffers of one layout."""
    dev = grad_flat.device
    for name, t, dt in (("segments", segments, torch.int64), ("chunks", chunks, torch.int32), ("hyper", hyper, torch.float32),
                        ("grad_flat", grad_flat, torch.float32), ("exp_avg", exp_avg, torch.float32),
                        ("exp_avg_sq", exp_avg_sq, torch.float32)):
        if not t.is_cuda or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"adam_step: {name} must be a contiguous {dt} tensor on {dev} (no CPU fallback)")
    if exp_avg.numel() != grad_flat.numel() or exp_avg_sq.numel() != grad_flat.numel():
        raise RuntimeError("adam_step: grad_flat, exp_avg and exp_avg_sq must have the same number of elements")
    _lib.check(_lib.load().sg_adam_step(int(segments.shape[0]), int(chunks.shape[0]), int(hyper.shape[0]), _ptr(segments), _ptr(chunks),
                                        _ptr(hyper), _ptr(grad_flat), _ptr(exp_avg), _ptr(exp_avg_sq), _stream(dev)), "sg_adam_step")
