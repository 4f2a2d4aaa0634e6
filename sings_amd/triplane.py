"""The tri-plane field (``HexPlaneField``, hexplane.py:107-190 of the reference: grids.{s}.{c}, aabb) and its autograd function.

Sampling (forward, plane / coordinate gradients) runs in HIP kernels behind the C ABI (sg_triplane_*).  No CPU fallback.  The
point-only half of the backward is issued when sings_amd/side_launch.py says so ("the point-only half ... early").
"""
import ctypes as C
import itertools
import weakref

import torch
import torch.nn as nn

from . import _lib
from ._marshal import _ptr, _stream
from .grad_arena import arena_holds_any, arena_out, is_feature_minor, like_layout
from .side_launch import flush_deferred, flush_triplane_prepare, issue_triplane_prepare, triplane_prepare_stream


def _tp_struct(planes, n_scales, aabb):
    """-> (tp, keep): the C description of the planes, and the tensors whose addresses it holds."""
    grids = [planes[3 * s:3 * s + 3] for s in range(n_scales)]
    tp, keep = _lib.SgTriplane(), []
    tp.n_scales, tp.feat = len(grids), int(grids[0][0].shape[1])
    # feature-minor planes (HexPlaneField(feature_minor=True)) are used in place by the kernels: no texel-major copy per call
    tp.feature_minor = int(all(is_feature_minor(p) for planes in grids for p in planes))
    for s, planes in enumerate(grids):
        # plane (0,1) is [1, F, Ry, Rx], (0,2) is [1, F, Rz, Rx], (1,2) is [1, F, Rz, Ry]
        rx, ry, rz = int(planes[0].shape[3]), int(planes[0].shape[2]), int(planes[1].shape[2])
        tp.res[s][0], tp.res[s][1], tp.res[s][2] = rx, ry, rz
        for c in range(3):
            t = planes[c].detach() if tp.feature_minor else planes[c].detach().contiguous().float()
            keep.append(t)
            tp.planes[s][c] = t.data_ptr()
    a = _aabb_host(aabb)
    for r in range(2):
        for k in range(3):
            tp.aabb[r][k] = a[r][k]
    return tp, keep


_aabb_cache = {}


def _aabb_host(aabb):
    """Host copy of the (non-trainable) bounding box, read back once per VALUE: a D2H copy in every forward and backward
    was a host synchronisation twice per training step.  An entry belongs to ONE tensor object (weak reference + version
    counter): a different tensor that later lands at the same address (a second HexPlaneField after the first was freed;
    a fresh tensor's version is 0 too) never sees the old bounds."""
    slot, key = (aabb.data_ptr(), str(aabb.device)), aabb._version
    hit = _aabb_cache.get(slot)
    if hit is None or hit[0] != key or hit[2]() is not aabb:
        a = aabb.detach().float().cpu()
        hit = (key, [[float(a[r, k]) for k in range(3)] for r in range(2)], weakref.ref(aabb))
        if len(_aabb_cache) > 64:
            _aabb_cache.clear()
        _aabb_cache[slot] = hit
    return hit[1]


def _tp_lookup(pts, aabb, n_scales, planes):
    """the tri-plane features of ``pts`` (sg_triplane_forward) -> (feats, x, tp, lib): the lookup alone, nothing kept for a backward."""
    if not pts.is_cuda:
        raise RuntimeError("sings_amd.decode: tensors must live on the GPU (no CPU fallback)")
    lib = _lib.load()
    tp, keep = _tp_struct(planes, n_scales, aabb)
    x = pts.detach().contiguous().float()
    dev, N = x.device, int(x.shape[0])
    ws = torch.empty(int(lib.sg_triplane_ws_bytes(C.byref(tp))), dtype=torch.uint8, device=dev)
    feats = torch.empty((N, tp.n_scales * tp.feat), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sg_triplane_forward(C.byref(tp), N, _ptr(x), _ptr(ws), _ptr(feats), _stream(dev)), "triplane forward")
    return feats, x, tp, lib


def triplane_features_nograd(triplane, pts):
    """``triplane(pts)`` for a caller that will never differentiate it: no autograd node, nothing saved, and none of the backward's
    preparation (the point sorts of ``_Triplane.forward``) is launched or queued -- under ``torch.no_grad()`` the autograd function
    would still see parameters that require a gradient and prepare for one."""
    planes = [p for gp in triplane.grids for p in gp]
    return _tp_lookup(pts.reshape(-1, 3), triplane.aabb, len(triplane.grids), planes)[0]


def _plane_views(gflat, planes):
    """the pieces of ``gflat`` as gradient planes, feature-minor like the parameters."""
    views, o = [], 0
    for p in planes:
        views.append(like_layout(gflat[o:o + p.numel()], p))
        o += p.numel()
    return views


class _Triplane(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, aabb, n_scales, *planes):
        feats, x, tp, lib = _tp_lookup(pts, aabb, n_scales, planes)
        dev, N = x.device, int(x.shape[0])
        ctx.save_for_backward(x, aabb, *planes)
        ctx.n_scales = n_scales
        ctx.early = None
        side = triplane_prepare_stream(dev) if any(ctx.needs_input_grad) else None
        if side is not None:
            bws = torch.empty(int(lib.sg_triplane_bwd_ws_bytes(C.byref(tp), N)), dtype=torch.uint8, device=dev)
            cur = torch.cuda.current_stream(dev)
            # (NOT deferred like the weight gradients: issued first, this chain keeps the forward's queue and the decoders move
            #  to the next one -- one hop; issued after the first decoder layer it shares a queue with the regularisers and the weight
            #  gradients and was executed after them, 2.14 instead of 2.06 ms per step)
            ev = torch.cuda.Event()
            fork = torch.cuda.Event()
            fork.record(cur)

            gz = []                                              # feature-minor planes: the zero-filled gradient buffer, made early too

            def launch(side=side):
                side.wait_event(fork)
                with torch.cuda.device(dev), torch.cuda.stream(side):
                    _lib.check(lib.sg_triplane_backward_prepare(C.byref(tp), N, _ptr(x), _ptr(bws), C.c_void_p(side.cuda_stream)),
                               "triplane backward (prepare)")
                    if tp.feature_minor and not arena_holds_any(planes):
                        gz.append(torch.zeros(sum(p.numel() for p in planes), dtype=torch.float32, device=dev))
                    ev.record(side)
                bws.record_stream(side); x.record_stream(side)
                for p in planes:
                    p.record_stream(side)
            issue_triplane_prepare(launch)
            ctx.early = (bws, ev, gz)
        return feats

    @staticmethod
    def backward(ctx, dfeats):
        lib = _lib.load()
        x, aabb, *planes = ctx.saved_tensors
        n_scales = ctx.n_scales
        tp, keep = _tp_struct(planes, n_scales, aabb)
        dev, N = x.device, int(x.shape[0])
        flush_triplane_prepare()
        early = ctx.early
        ws = early[0] if early else torch.empty(int(lib.sg_triplane_bwd_ws_bytes(C.byref(tp), N)), dtype=torch.uint8, device=dev)
        cur = torch.cuda.current_stream(dev)
        # feature-minor: gradient planes laid out like the parameters, written in place by the scatter; they must start from zero
        gflat = None
        if tp.feature_minor and early and early[2]:
            gflat = early[2][0]                                  # zero-filled on the side stream with the preparation
            gflat.record_stream(cur)
        elif tp.feature_minor and not arena_holds_any(planes):
            gflat = torch.zeros(sum(p.numel() for p in planes), dtype=torch.float32, device=dev)      # ONE fill
        if gflat is not None:
            dplanes = _plane_views(gflat, planes)
        else:
            dplanes = [arena_out(p) for p in planes]             # (straight into the caller's flat buffer, if registered; a busy slot: fresh)
            if tp.feature_minor:
                for d in dplanes:
                    d.zero_()
        arr = ((C.c_void_p * 3) * 4)()
        for s in range(n_scales):
            for c in range(3):
                arr[s][c] = dplanes[3 * s + c].data_ptr()
        dxyz = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        df = dfeats.contiguous().float()
        with torch.cuda.device(dev):
            if early:
                cur.wait_event(early[1])                         # the prepared half (launched by the forward)
                ctx.early = None
                fn = lib.sg_triplane_backward_prepared
            else:
                fn = lib.sg_triplane_backward
            _lib.check(fn(C.byref(tp), N, _ptr(x), _ptr(ws), _ptr(df), C.byref(arr), _ptr(dxyz), _stream(dev)), "triplane backward")
        flush_deferred()                                         # (the first layers' weight gradients: behind this kernel)
        return (dxyz, None, None) + tuple(dplanes)


def init_grid_param(grid_nd, in_dim, out_dim, reso, a=0.1, b=0.5, device='cuda'):
    """hexplane.py:18-43 (3-D inputs only)."""
    assert in_dim == len(reso) == 3 and grid_nd == 2
    grid_coefs = nn.ParameterList()
    for coo_comb in itertools.combinations(range(in_dim), grid_nd):
        p = nn.Parameter(torch.empty([1, out_dim] + [reso[cc] for cc in coo_comb[::-1]], device=device))
        nn.init.uniform_(p, a=a, b=b)
        grid_coefs.append(p)
    return grid_coefs


class HexPlaneField(nn.Module):
    def __init__(self, planeconfig, bounds=1., device='cuda', feature_minor=False):
        """``feature_minor=True``: the planes keep the reference's SHAPE [1, F, H, W] (checkpoints load and save unchanged) but live
        in torch's channels_last memory format, i.e. [H][W][F] -- the layout the sampling kernels want -- so that neither the
        parameters nor their gradients are re-laid-out per call (one 18-us and one 28-us copy of the 33 MB of planes forward /
        in the backward's preparation, one 23-us copy of the gradients back, per training step at 150 k points)."""
        super().__init__()
        aabb = torch.tensor([[bounds, bounds, bounds], [-bounds, -bounds, -bounds]], dtype=torch.float32)
        self.aabb = nn.Parameter(aabb, requires_grad=False).to(device)
        self.grid_config = [planeconfig]
        self.multiscale_res_multipliers = planeconfig["multires"]
        self.concat_features = True
        self.grids = nn.ModuleList()
        self.feat_dim = 0
        for res in self.multiscale_res_multipliers:
            config = dict(self.grid_config[0])
            config["resolution"] = [r * res for r in config["resolution"][:3]]
            gp = init_grid_param(config["grid_dimensions"], config["input_coordinate_dim"], config["output_coordinate_dim"],
                                 config["resolution"], device=device)
            self.feat_dim += gp[-1].shape[1]
            if feature_minor:
                for p in gp:
                    p.data = p.data.contiguous(memory_format=torch.channels_last)
            self.grids.append(gp)

    @property
    def get_aabb(self):
        return self.aabb[0], self.aabb[1]

    def set_aabb(self, xyz_max, xyz_min):
        self.aabb = nn.Parameter(torch.tensor([xyz_max, xyz_min], dtype=torch.float32, device=self.aabb.device), requires_grad=False)

    def forward(self, pts, timestamps=None):
        assert timestamps is None, "spatial planes only (the reference's human model never passes timestamps)"
        planes = [p for gp in self.grids for p in gp]
        return _Triplane.apply(pts.reshape(-1, 3), self.aabb, len(self.grids), *planes)

    get_density = forward
