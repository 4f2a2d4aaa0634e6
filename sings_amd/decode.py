"""Attribute decode upstream of the render path: tri-plane features + the two decoder MLPs.

Module and parameter names mirror the reference so that its checkpoints load unchanged
(``SinGS.state_dict()['triplane']``, ``['geometry_dec_i']``, ``['appearance_dec_i']``):

    HexPlaneField(planeconfig, bounds)        sings/rec/models/modules/hexplane.py:107-190   (grids.{s}.{c}, aabb)      sings_amd/triplane.py
    GeometryDecoder(n_features, isotropic)    modules/decoders.py:57-110   (net.0, net.2, xyz_offsets, scales.0, scales.2, rotations.0)
    AppearanceDecoder(n_features, ...)        modules/decoders.py:16-54    (net.0, net.2, opacity, shs)
    decode_attributes(...)                    SinGS.get_gs_attrs, sings_hybrid.py:249-313 (single level)

Tri-plane sampling (sings_amd/triplane.py) and every layer (sings_amd/linear_layers.py: GEMM, bias and activation, forward and
backward) are HIP kernels behind the C ABI.  No CPU fallback.  The gradient arena (sings_amd/grad_arena.py) and the side-launch
schedule (sings_amd/side_launch.py) have modules of their own.  The public names of all four modules are also exported from here.
"""
import torch
import torch.nn as nn

from . import _lib
from ._marshal import _ptr, _stream
from .grad_arena import arena_sync, invalidate_gradient_arena, set_gradient_arena                                  # noqa: F401
from .linear_layers import (ACT_GELU, ACT_NONE, ACT_SIGMOID, ACT_SOFTPLUS_REF, activation, fuse_fan_backward,      # noqa: F401
                            linear_act, linear_act_shared, linear_fan, scales_head)
from .side_launch import (flush_triplane_prepare, overlap_weight_grads, prepare_triplane_backward_early,           # noqa: F401
                          prepare_triplane_backward_late, reset_deferred)
from .triplane import HexPlaneField, init_grid_param, triplane_features_nograd                                     # noqa: F401


class AppearanceDecoder(nn.Module):
    def __init__(self, n_features, hidden_dim=64, act='gelu', fixed_opacity=False):
        super().__init__()
        assert act == 'gelu', "the reference's default (and only configured) activation"
        self.hidden_dim = hidden_dim
        self.net = nn.Sequential(nn.Linear(n_features, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, hidden_dim), nn.GELU())
        if not fixed_opacity:
            self.opacity = nn.Linear(hidden_dim, 1)
            self.opacity_act = nn.Sigmoid()
            self.opacity_offset = 0
        self.fixed_opacity = fixed_opacity
        self.shs = nn.Linear(hidden_dim, 16 * 3)

    def _trunk(self, x):
        return linear_act(linear_act(x, self.net[0], ACT_GELU), self.net[2], ACT_GELU)

    def reset_opacity(self, x):
        with torch.no_grad():
            o = linear_act(self._trunk(x), self.opacity)
            self.opacity_offset = torch.where(o > 0, torch.zeros_like(o), -o)

    def heads(self, x):
        """the heads on the trunk output x: one fan (their input gradients are accumulated in place)."""
        if not self.fixed_opacity:
            off = self.opacity_offset if torch.is_tensor(self.opacity_offset) else None
            shs, opacity = linear_fan(x, [(self.shs, ACT_NONE, None), (self.opacity, ACT_SIGMOID, off)])
        else:
            shs = linear_act(x, self.shs)
            opacity = torch.ones((x.shape[0], 1), device=x.device)
        return {'shs': shs.reshape(-1, 16, 3), 'opacity': opacity}

    def forward(self, x, first=None):
        """``first``: the output of net[0] + GELU when the caller computed it (decode_attributes fans the tri-plane features
        out to both decoders' first layers)."""
        h1 = linear_act(x, self.net[0], ACT_GELU) if first is None else first
        return self.heads(linear_act(h1, self.net[2], ACT_GELU))


class GeometryDecoder(nn.Module):
    def __init__(self, n_features, isotropic=True, hidden_dim=128, act='gelu'):
        super().__init__()
        assert act == 'gelu'
        self.hidden_dim, self.isotropic = hidden_dim, isotropic
        self.net = nn.Sequential(nn.Linear(n_features, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, hidden_dim), nn.GELU())
        self.xyz_offsets = nn.Linear(hidden_dim, 3)
        if not isotropic:
            self.rotations = nn.Sequential(nn.Linear(hidden_dim, 6))
        self.scales = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, 1 if isotropic else 3))

    def forward(self, x, first=None):
        h1 = linear_act(x, self.net[0], ACT_GELU) if first is None else first
        x = linear_act(h1, self.net[2], ACT_GELU)
        # the heads read the same trunk output: one fan, the wide layer first (it writes dx, the narrow heads add to it)
        layers = [(self.scales[0], ACT_GELU, None), (self.xyz_offsets, ACT_NONE, None)]
        if not self.isotropic:
            layers.append((self.rotations[0], ACT_NONE, None))
        outs = linear_fan(x, layers)
        s1, xyz_offsets = outs[0], outs[1]
        rotations = outs[2] if not self.isotropic else None
        scales_aux = linear_act(s1, self.scales[2])
        if scales_aux.shape[-1] == 1:
            # isotropic: softplus and the two `.repeat(1, 3)` in one launch each way (sg_scales_head_*)
            scales, scales_aux = scales_head(scales_aux)
        else:
            # scales = log(exp(scales_aux) + 1): the activation kernel on the bias-added value (identity GEMM avoided)
            scales = activation(scales_aux, ACT_SOFTPLUS_REF)
        return {'xyz_offsets': xyz_offsets, 'rotations': rotations, 'scales': scales, 'scales_aux': scales_aux}


# ---- decoders without a gradient ---------------------------------------------------------------------------------------------
# The reference's first opt_geo_from / opt_app_from iterations run a decoder under torch.no_grad() (sings_hybrid.py:265-277): nothing
# of it is ever differentiated, so nothing of it needs saving.  One launch per decoder (include/sings_frozen.h: the hidden layers stay
# in LDS); where the library lacks that table or refuses the widths, the per-layer kernels under no_grad -- the same values up to the
# summation order.
def _fz_param(t):
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


def _fz_usable(feats, hidden, wide):
    """the fused kernels take these features and weights: the table is there, the widths are theirs, the 16-byte loads are aligned."""
    cin = int(feats.shape[1])
    return (_lib.HAS_FROZEN and feats.is_cuda and feats.shape[0] >= 1 and cin % 4 == 0 and 4 <= cin <= 128 and hidden in (64, 128)
            and all(t.data_ptr() % 16 == 0 for t in wide))


def frozen_geometry(feats, dec, fused=True, out=None):
    """GeometryDecoder.forward without autograd: {'xyz_offsets', 'rotations' | None, 'scales', 'scales_aux'}.  ``fused=False``: the
    per-layer kernels under no_grad.  ``out``: buffers (xyz_offsets, scales, scales_aux, rotations | None) of at least N rows the
    fused kernel writes its N rows into."""
    lib = _lib.load()
    feats = _fz_param(feats)
    lins = [dec.net[0], dec.net[2], dec.scales[0], dec.scales[2], dec.xyz_offsets] + ([] if dec.isotropic else [dec.rotations[0]])
    W = [_fz_param(l.weight) for l in lins]
    hidden = int(W[0].shape[0])
    if not (fused and _fz_usable(feats, hidden, W)):
        if out is not None:
            raise RuntimeError("sings_amd.decode: the fused no-gradient decode does not take these widths")
        with torch.no_grad():
            return dec(feats)
    b = [_fz_param(l.bias) for l in lins]
    dev, N = feats.device, int(feats.shape[0])
    if out is None:
        out = [torch.empty((N, 3), dtype=torch.float32, device=dev) for _ in range(3)]
        out.append(None if dec.isotropic else torch.empty((N, 6), dtype=torch.float32, device=dev))
    xyz_offsets, scales, scales_aux, rotations = out
    rot = (W[5], b[5]) if not dec.isotropic else (None, None)
    with torch.cuda.device(dev):
        _lib.check(lib.sg_frozen_geometry(
            N, int(feats.shape[1]), hidden, 0 if dec.isotropic else 1, _ptr(feats), _ptr(W[0]), _ptr(b[0]), _ptr(W[1]), _ptr(b[1]),
            _ptr(W[2]), _ptr(b[2]), _ptr(W[3]), _ptr(b[3]), _ptr(W[4]), _ptr(b[4]), _ptr(rot[0]), _ptr(rot[1]), _ptr(xyz_offsets),
            _ptr(scales), _ptr(scales_aux), _ptr(rotations), _stream(dev)), "frozen geometry decode")
    return {'xyz_offsets': xyz_offsets, 'rotations': rotations, 'scales': scales, 'scales_aux': scales_aux}


def frozen_appearance(feats, dec, fused=True, out=None):
    """AppearanceDecoder.forward without autograd: {'shs' [N,16,3], 'opacity' [N,1]}.  ``out``: (shs [>=N,48], opacity [>=N,1] |
    None) for the fused kernel."""
    lib = _lib.load()
    feats = _fz_param(feats)
    lins = [dec.net[0], dec.net[2], dec.shs] + ([] if dec.fixed_opacity else [dec.opacity])
    W = [_fz_param(l.weight) for l in lins]
    b = [_fz_param(l.bias) for l in lins]
    hidden = int(W[0].shape[0])
    if not (fused and _fz_usable(feats, hidden, W + [b[2]]) and int(W[2].shape[0]) == _lib.FROZEN_SHS):
        if out is not None:
            raise RuntimeError("sings_amd.decode: the fused no-gradient decode does not take these widths")
        with torch.no_grad():
            return dec(feats)
    dev, N = feats.device, int(feats.shape[0])
    if out is None:
        out = (torch.empty((N, _lib.FROZEN_SHS), dtype=torch.float32, device=dev),
               None if dec.fixed_opacity else torch.empty((N, 1), dtype=torch.float32, device=dev))
    shs, opacity = out
    off = None
    if not dec.fixed_opacity and torch.is_tensor(dec.opacity_offset):
        off = dec.opacity_offset.detach().contiguous().float().reshape(-1)
    op = (W[3], b[3]) if not dec.fixed_opacity else (None, None)
    with torch.cuda.device(dev):
        _lib.check(lib.sg_frozen_appearance(
            N, int(feats.shape[1]), hidden, _ptr(feats), _ptr(W[0]), _ptr(b[0]), _ptr(W[1]), _ptr(b[1]), _ptr(W[2]), _ptr(b[2]),
            _ptr(op[0]), _ptr(op[1]), _ptr(off), _ptr(shs), _ptr(opacity), _stream(dev)), "frozen appearance decode")
    if dec.fixed_opacity:
        opacity = torch.ones((N, 1), device=dev)
    return {'shs': shs[:N].reshape(-1, 16, 3), 'opacity': opacity}


def _assemble(xyz, g, a_fn, thickness_factor, scaling_multiplier, geometry_hook):
    """the tail of SinGS.get_gs_attrs (sings_hybrid.py:280-313) on a geometry decoder's outputs; ``a_fn()``: the appearance decoder's,
    issued after the geometry hook."""
    scales = g['scales']
    if thickness_factor != 1.0:
        scales = torch.cat([scales[:, :-1], scales[:, -1:] * thickness_factor], dim=1)
    if scaling_multiplier is not None:
        scales = scales * scaling_multiplier
    xyz_canon = xyz + g['xyz_offsets']
    if geometry_hook is not None:
        xyz_canon, scales = geometry_hook(xyz_canon, scales)
    a = a_fn()
    return {"xyz_canon": xyz_canon, "xyz_offsets": g['xyz_offsets'], "rot6d_canon": g['rotations'],
            "scales_aux": g['scales_aux'], "scales": scales, "opacity": a['opacity'], "shs": a['shs']}


def decode_frozen(xyz, triplane, geometry_dec, appearance_dec, thickness_factor=1.0, scaling_multiplier=None, geometry_hook=None,
                  fused=True):
    """``decode_attributes`` with both decoders frozen: the tri-plane lookup saves nothing, no backward preparation is queued, each
    decoder is one launch and its outputs carry no autograd history.  ``xyz_canon = xyz + xyz_offsets`` keeps the gradient to ``xyz``
    (and is the only output that does).  ``fused=False``: the per-layer kernels under no_grad."""
    tri_feats = triplane_features_nograd(triplane, xyz)
    g = frozen_geometry(tri_feats, geometry_dec, fused)
    return _assemble(xyz, g, lambda: frozen_appearance(tri_feats, appearance_dec, fused), thickness_factor, scaling_multiplier,
                     geometry_hook)


def _first_layers(tri_feats, decs):
    """net[0] + GELU of every LIVE decoder in ``decs`` on the tri-plane features they all read.  With gradients enabled (and a width
    the accumulating kernel takes): ONE feature gradient through a shared slot (the second layer to run its backward adds into the
    first one's), but one autograd node per decoder -- the appearance decoder's backward does not wait for the geometry decoder's.
    Otherwise one fan, or the plain layer for a single decoder."""
    if torch.is_grad_enabled() and (int(tri_feats.shape[1]) & 31) == 0:
        slot = {}
        return [linear_act_shared(tri_feats, d.net[0], ACT_GELU, slot) for d in decs]
    if len(decs) == 1:
        return [linear_act(tri_feats, decs[0].net[0], ACT_GELU)]
    return list(linear_fan(tri_feats, [(d.net[0], ACT_GELU, None) for d in decs]))


def decode_attributes(xyz, triplane, geometry_dec, appearance_dec, thickness_factor=1.0, scaling_multiplier=None,
                      geometry_hook=None, opt_geo=True, opt_app=True, fused_frozen=True):
    """SinGS.get_gs_attrs for one level (sings_hybrid.py:249-313): the dict the LBS/render path consumes.
    ``geometry_hook(xyz_canon, scales) -> (xyz_canon, scales)``: applied to the geometry decoder's outputs BEFORE the appearance
    decoder is issued -- autograd nodes the hook creates are visited after the appearance decoder's in the backward pass
    (sings_amd.train_step uses it to add the k-NN regulariser's gradient as late as possible).
    ``opt_geo`` / ``opt_app`` (gs_trainer.py:225-226): False freezes that decoder as the reference's torch.no_grad() does -- its
    outputs carry no autograd history and its parameters receive no gradient; with both False the tri-plane receives none either.
    ``fused_frozen=False``: a frozen decoder runs through the per-layer kernels under no_grad instead of the fused launch."""
    if not (opt_geo or opt_app):
        return decode_frozen(xyz, triplane, geometry_dec, appearance_dec, thickness_factor, scaling_multiplier, geometry_hook,
                             fused_frozen)
    tri_feats = triplane(xyz)
    # a live decoder reads the features through its own layers, a frozen one, detached, through the fused launch
    first = _first_layers(tri_feats, [d for d, live in ((geometry_dec, opt_geo), (appearance_dec, opt_app)) if live])
    g = geometry_dec(tri_feats, first=first[0]) if opt_geo else frozen_geometry(tri_feats, geometry_dec, fused_frozen)
    a_fn = (lambda: appearance_dec(tri_feats, first=first[-1])) if opt_app else (
        lambda: frozen_appearance(tri_feats, appearance_dec, fused_frozen))
    return _assemble(xyz, g, a_fn, thickness_factor, scaling_multiplier, geometry_hook)
