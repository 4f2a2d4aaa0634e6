"""Drop-in replacement of the ``diff_gaussian_rasterization`` Python package on MI355X.

Same public surface the reference imports (sings/rec/renderer/gs_renderer_single.py:6-9,
gs_renderer_multiple.py:6-9; package = install_all.sh:22): ``GaussianRasterizationSettings``
(12-field NamedTuple), ``GaussianRasterizer`` (nn.Module, returns ``(color, radii)``),
``rasterize_gaussians`` and the ``_RasterizeGaussians`` autograd.Function, with the upstream
argument order and gradient order ``(means3D, means2D, sh, colors_precomp, opacities, scales,
rotations, cov3Ds_precomp, None)``.  The compute is the hand-written gfx950 library behind the
C ABI of include/sings_hip.h -- there is no CPU / eager fallback.  The op's tensors, its camera and the stream become
C arguments through sings_amd/_marshal.py, as in every other module that calls the library.
"""
import ctypes as C
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib, overflow
from ._marshal import _f32, _ptr, _settings_struct, _stream
# The pair capacity, the overflow-check modes and the learned list-length hints live in sings_amd/overflow.py; INTEGRATION.md §2
# documents importing the mode switches from here.  Its state tables stay reachable here too, as the very objects that module
# updates in place (never rebound), for code written against this module (benchkit/leg_train.py reads _capacity_hint).
from .overflow import (_capacity_hint, _mode, _pending, _rows_ok, _seen, _short_ok, _signal,  # noqa: F401
                       check_deferred_overflow, reset_overflow_state, set_deferred_overflow_check, set_overflow_check)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _backward_buffers(dev, P, M, bwd_bytes, has_sh, has_col, has_scale, has_cov):
    """The gradient tensors and the record workspace of one backward call (every element is written by the kernels)."""
    def e(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)
    return (e(P, 3), e(P, 3), e(P, 1), e(P, M, 3) if has_sh else None, e(P, 3) if has_col else None,
            e(P, 3) if has_scale else None, e(P, 4) if has_scale else None, e(P, 6) if has_cov else None,
            torch.empty(int(bwd_bytes), dtype=torch.uint8, device=dev))


_PREALLOC_SETS = 2                   # backward-buffer sets a forward may allocate ahead of their backward (two views in flight)
_PREALLOC = {"out": 0}


class _PreallocSet:
    """A forward's pre-allocated backward buffers; counted while they wait (a graph dropped without a backward frees the count too)."""

    def __init__(self, bufs):
        self.bufs = bufs
        _PREALLOC["out"] += 1

    def take(self):
        bufs, self.bufs = self.bufs, None
        if bufs is not None:
            _PREALLOC["out"] -= 1
        return bufs

    def __del__(self):
        self.take()


def _empty_to_none(t):
    return None if t is None or t.numel() == 0 else t


class _RasterizeGaussians(torch.autograd.Function):
    """The drop-in op; ``return_aux``: also the depth and alpha maps (include/sings_hip.h, "depth and alpha maps"), returning
    (color, radii, depth, alpha), depth / alpha [1,H,W]."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, write_point_keys=False, return_aux=False):
        lib = _lib.load()
        dev = means3D.device
        if dev.type != "cuda":
            raise RuntimeError("sings_amd rasterizer runs on the MI355X only (tensors must be on a 'cuda' "
                               "device); there is no CPU fallback")
        if return_aux:
            ctx.set_materialize_grads(False)
        rs = raster_settings
        means3D = _f32(means3D, "means3D", dev)
        sh = _f32(_empty_to_none(sh), "sh", dev)
        colors_precomp = _f32(_empty_to_none(colors_precomp), "colors_precomp", dev)
        opacities = _f32(opacities, "opacities", dev)
        scales = _f32(_empty_to_none(scales), "scales", dev)
        rotations = _f32(_empty_to_none(rotations), "rotations", dev)
        cov3Ds_precomp = _f32(_empty_to_none(cov3Ds_precomp), "cov3Ds_precomp", dev)
        P = int(means3D.shape[0])
        H, W = int(rs.image_height), int(rs.image_width)
        M = int(sh.shape[1]) if sh is not None else 0
        keep = []
        s = _settings_struct(rs, dev, M, keep)
        stream = _stream(dev)
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        if return_aux:
            depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
            alpha = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        need_bwd = any(ctx.needs_input_grad[:8]) and not return_aux     # (the maps' backward allocates its own buffers)
        L = geom = binning = img = bufs = aux = None

        def launch(cap, flags, sync):
            nonlocal L, geom, binning, img, bufs, aux
            L = _lib.layout(P, W, H, cap)
            geom = torch.empty(L.geom_bytes, dtype=torch.uint8, device=dev)
            binning = torch.empty(L.bin_bytes, dtype=torch.uint8, device=dev)
            img = torch.empty(L.img_bytes, dtype=torch.uint8, device=dev)
            # The backward's buffers are allocated HERE, in front of the forward's launch + wait for the pair count: the host
            # work of a "sync" forward ends when the scan kernel has published R, and from there to the backward's first
            # launch the GPU has only the forward composite (~70 us at cfg3) to run -- autograd's thread hop plus eight
            # allocations, a layout call and a settings struct on the far side of that wait left it idle for ~50 us per view
            # (drop-in surface 0.358 ms against 0.293 for the pre-allocated engine; now the allocations hide under the previous
            # view's backward).  Only when a gradient is wanted; handed out once (a second backward through a retained graph
            # allocates afresh: autograd may have adopted the first set as .grad).
            # (At most _PREALLOC_SETS such sets are outstanding: a caller that renders many views before ONE backward would hold a
            #  set -- ~80 MB at cfg3 -- per view; its later forwards leave the allocation to the backward, as before round 5.)
            bufs = None
            if need_bwd and _PREALLOC["out"] < _PREALLOC_SETS:
                bufs = _backward_buffers(dev, P, M, L.bwd_bytes, sh is not None, colors_precomp is not None, scales is not None,
                                         cov3Ds_precomp is not None)
            nr = C.c_int64(0)
            s.flags = flags
            args = (C.byref(s), P, _ptr(means3D), _ptr(sh), _ptr(colors_precomp), _ptr(opacities), _ptr(scales),
                    _ptr(rotations), _ptr(cov3Ds_precomp), _ptr(geom), _ptr(binning), cap, _ptr(img),
                    _ptr(color), _ptr(radii), int(bool(write_point_keys)), C.byref(nr) if sync else None)
            if return_aux:
                aux = torch.empty(_lib.aux_layout(P, W, H, cap), dtype=torch.uint8, device=dev)
                _lib.check(lib.sg_rasterize_forward_aux(*args, _ptr(aux), _ptr(depth), _ptr(alpha), stream),
                           "forward (depth / alpha maps)")
            else:
                _lib.check(lib.sg_rasterize_forward(*args, stream), "forward")
            return (int(nr.value),) if sync else None

        cap, counts = overflow.run_forward(
            dev, P, W, H, s, launch, lambda: binning[:8].view(torch.int32), debug=rs.debug,
            hints=(_lib.FLAG_SHORT_LISTS, _lib.FLAG_LONG_ROWS),   # both learned hints (LONG_ROWS: images of few tiles; ignored elsewhere)
            hints_need_sync=True,     # the drop-in guarantee: a hinted frame is only rendered when its count is read before returning
            early_count=True)         # "sync" forwards read R from the early-count word and learn the hints from it
        R = None if counts is None else counts[0]
        ctx.raster_settings = rs
        ctx.num_rendered = R
        ctx.capacity = cap
        ctx.sh_coeffs = M
        ctx.bwd_bufs = None if bufs is None else _PreallocSet(bufs)
        ctx.bwd_bytes = int(L.bwd_bytes)
        ctx.settings_struct = (s, keep)                     # the backward passes the same struct (same camera, same flags)
        ctx.flags = (sh is not None, colors_precomp is not None, scales is not None, cov3Ds_precomp is not None)
        z = torch.empty(0, device=dev)
        ctx.save_for_backward(means3D, sh if sh is not None else z,
                              colors_precomp if colors_precomp is not None else z,
                              opacities, scales if scales is not None else z,
                              rotations if rotations is not None else z,
                              cov3Ds_precomp if cov3Ds_precomp is not None else z,
                              radii, geom, binning, img, *((aux,) if return_aux else ()))
        ctx.mark_non_differentiable(radii)
        if return_aux:
            return color, radii, depth, alpha
        return color, radii

    @staticmethod
    def backward(ctx, grad_color, _grad_radii=None, grad_depth=None, grad_alpha=None):
        lib = _lib.load()
        (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, radii, geom, binning, img,
         *aux) = ctx.saved_tensors
        has_sh, has_col, has_scale, has_cov = ctx.flags
        rs = ctx.raster_settings
        dev = means3D.device
        P = int(means3D.shape[0])
        H, W = int(rs.image_height), int(rs.image_width)
        s, keep = ctx.settings_struct
        s.count_signal = None; s.count_signal_host = None
        g = (torch.zeros((3, H, W), dtype=torch.float32, device=dev) if grad_color is None      # (return_aux: not materialised)
             else _f32(grad_color, "grad_out_color", dev))
        gD = None if grad_depth is None else _f32(grad_depth, "grad_depth", dev)
        gA = None if grad_alpha is None else _f32(grad_alpha, "grad_alpha", dev)
        held, ctx.bwd_bufs = ctx.bwd_bufs, None
        bufs = None if held is None else held.take()
        if bufs is None:
            bufs = _backward_buffers(dev, P, ctx.sh_coeffs, ctx.bwd_bytes, has_sh, has_col, has_scale, has_cov)
        dmeans3D, dmeans2D, dopac, dsh, dcol, dscales, drots, dcov, bwd_ws = bufs
        args = (C.byref(s), P, _ptr(means3D), _ptr(sh) if has_sh else None,
                _ptr(colors_precomp) if has_col else None, _ptr(opacities),
                _ptr(scales) if has_scale else None, _ptr(rotations) if has_scale else None,
                _ptr(cov3Ds_precomp) if has_cov else None, _ptr(radii), _ptr(geom), _ptr(binning), ctx.capacity,
                _ptr(img), _ptr(bwd_ws), _ptr(g), _ptr(dmeans3D), _ptr(dmeans2D), _ptr(dsh), _ptr(dcol),
                _ptr(dopac), _ptr(dscales), _ptr(drots), _ptr(dcov))
        with torch.cuda.device(dev):
            stream = _stream(dev)
            if gD is None and gA is None:       # neither map carries a gradient: the plain backward, bit for bit
                _lib.check(lib.sg_rasterize_backward(*args, stream), "backward")
            else:
                _lib.check(lib.sg_rasterize_backward_aux(*args, _ptr(aux[0]), _ptr(gD), _ptr(gA), stream),
                           "backward (depth / alpha maps)")
        return (dmeans3D, dmeans2D, dsh, dcol, dopac.view_as(opacities), dscales, drots, dcov, None, None, None)


def rasterize_gaussians_aux(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                            raster_settings):
    """(color, radii, depth, alpha): ``rasterize_gaussians`` plus the accumulated depth sum_i z_i alpha_i T_i and the alpha map
    1 - T_final, both [1,H,W] and differentiable (expected depth = depth / alpha)."""
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, False, True)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        lib = _lib.load()
        rs = self.raster_settings
        with torch.no_grad():
            dev = positions.device
            pos = _f32(positions, "positions", dev)
            vm = _f32(rs.viewmatrix, "viewmatrix", dev)
            pm = _f32(rs.projmatrix, "projmatrix", dev)
            out = torch.empty(pos.shape[0], dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.sg_mark_visible(int(pos.shape[0]), _ptr(pos), _ptr(vm), _ptr(pm), _ptr(out), _stream(dev)),
                           "mark_visible")
        return out.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        return rasterize_gaussians(*self._inputs(means3D, means2D, opacities, shs, colors_precomp, scales, rotations,
                                                 cov3D_precomp), self.raster_settings)

    def forward_aux(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                    cov3D_precomp=None):
        """``forward`` that also returns the depth and alpha maps: (color, radii, depth, alpha)."""
        return rasterize_gaussians_aux(*self._inputs(means3D, means2D, opacities, shs, colors_precomp, scales, rotations,
                                                     cov3D_precomp), self.raster_settings)

    @staticmethod
    def _inputs(means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D '
                            'covariance!')
        empty = torch.Tensor([])
        if shs is None:
            shs = empty
        if colors_precomp is None:
            colors_precomp = empty
        if scales is None:
            scales = empty
        if rotations is None:
            rotations = empty
        if cov3D_precomp is None:
            cov3D_precomp = empty
        return means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp
