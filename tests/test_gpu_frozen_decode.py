"""The decoders without a gradient (sings_amd/csrc/sg_decode_frozen.hip through ``decode.frozen_geometry`` / ``frozen_appearance`` /
``decode_frozen`` / ``decode_attributes(opt_geo=, opt_app=)``) against the reference's own outputs (tests/golden/decode_golden.npz), the
fp64 oracle and today's per-layer kernels.

The bar for values is tests/test_gpu_decode.py's for the per-layer kernels on the same vectors: fp32 with another summation order ->
2e-5 relative + 2e-6 of the array's scale.  Gradients of the flag cases: that file's tolerances for the same arrays (1e-4 + 1e-5 of the
scale for the anchors' and the planes' gradients in its shipped-configuration test; 2e-5 + 2e-5 of the scale + 2e-5 for parameter
gradients, sums over the points, in its golden test)."""
import os

import numpy as np
import pytest
import torch

from oracle import decode_oracle as do

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "decode_golden.npz"))
R = 128                                  # the kernel's point block (SG_FROZEN_BLOCK)
CFG = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [16, 16, 16], 'multires': [1, 2, 4]}


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _close(a, b, rtol=2e-5, atol_scale=2e-6, atol=0.0, what=""):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b)
    print(f"{what}: max err {err.max():.3e}, scale {scale:.3e}")
    assert (err <= rtol * np.abs(b) + atol_scale * scale + atol).all(), (what, err.max(), scale)


def _np(t):
    return t.detach().cpu().numpy()


def test_block_constant():
    from sings_amd import _lib
    assert _lib.FROZEN_BLOCK == R


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------
def test_golden_outputs_of_the_references_modules():
    from sings_amd.decode import AppearanceDecoder, GeometryDecoder, frozen_appearance, frozen_geometry
    dev = _dev()
    for tag, iso in (("iso", True), ("aniso", False)):
        g = GeometryDecoder(n_features=64, isotropic=iso)
        g.load_state_dict({k[len(f"geo_{tag}_p_"):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"geo_{tag}_p_")})
        g = g.to(dev)
        o = frozen_geometry(torch.from_numpy(G[f"geo_{tag}_x"]).to(dev), g)
        for k in ('xyz_offsets', 'scales', 'scales_aux') + (() if iso else ('rotations',)):
            assert not o[k].requires_grad and o[k].grad_fn is None
            _close(_np(o[k]), G[f"geo_{tag}_o_{k}"], what=f"golden geo {tag} {k}")
        assert (o['rotations'] is None) == iso
    a = AppearanceDecoder(n_features=64)
    a.load_state_dict({k[len("app_p_"):]: torch.from_numpy(G[k]) for k in G.files if k.startswith("app_p_")})
    a = a.to(dev)
    a.opacity_offset = torch.from_numpy(G["app_offset"]).to(dev)
    o = frozen_appearance(torch.from_numpy(G["geo_aniso_x"]).to(dev), a)
    assert o['shs'].grad_fn is None and o['opacity'].grad_fn is None
    _close(_np(o['shs']), G["app_o_shs"], what="golden app shs")
    _close(_np(o['opacity']), G["app_o_opacity"], what="golden app opacity")


# ---- tile edges at the shipped widths ----------------------------------------------------------------------------------------------
_MODS = {}


def _decoders(dev, iso, fixed_opacity):
    """the shipped widths (96 features, hidden 128 / 64), made once per kind and left unchanged"""
    from sings_amd.decode import AppearanceDecoder, GeometryDecoder
    key = (iso, fixed_opacity)
    if key not in _MODS:
        torch.manual_seed(3 + 2 * iso + fixed_opacity)
        g = GeometryDecoder(96, isotropic=iso).to(dev)
        a = AppearanceDecoder(96, fixed_opacity=fixed_opacity).to(dev)
        with torch.no_grad():
            g.scales[2].bias.fill_(-3.7)
        sd64 = lambda m: {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        _MODS[key] = (g, a, sd64(g), sd64(a))
    return _MODS[key]


def _guarded(N, cols, dev):
    return torch.full((N + 1, cols), float("nan"), dtype=torch.float32, device=dev)


@pytest.mark.parametrize("iso", [True, False])
@pytest.mark.parametrize("N", [1, R - 1, R, R + 1, 3 * R + 5])
def test_tile_edges_against_the_oracle_and_the_per_layer_path(N, iso):
    from sings_amd.decode import frozen_appearance, frozen_geometry
    dev = _dev()
    g, a, sdg, sda = _decoders(dev, iso, False)
    rs = np.random.RandomState(100 + N)
    x = torch.from_numpy(rs.normal(0, 0.6, (N, 96)).astype(np.float32)).to(dev)
    off = torch.from_numpy(rs.uniform(0, 2, (N, 1)).astype(np.float32)).to(dev)
    x64 = x.cpu().double()
    # geometry: guard rows of NaN behind row N - 1 of every output
    out = [_guarded(N, 3, dev), _guarded(N, 3, dev), _guarded(N, 3, dev), None if iso else _guarded(N, 6, dev)]
    o = frozen_geometry(x, g, out=out)
    ref = do.geometry_decoder(x64, sdg, isotropic=iso)
    per = frozen_geometry(x, g, fused=False)
    for k in ('xyz_offsets', 'scales', 'scales_aux') + (() if iso else ('rotations',)):
        assert torch.isnan(o[k][N:]).all(), f"{k}: rows behind N written"
        _close(_np(o[k][:N]), ref[k].numpy(), what=f"geo N={N} iso={iso} {k} vs fp64")
        _close(_np(o[k][:N]), _np(per[k]), what=f"geo N={N} iso={iso} {k} vs per-layer")
    if iso:
        assert torch.equal(o['scales'][:N, :1].expand(N, 3), o['scales'][:N]) and torch.equal(o['scales_aux'][:N, :1].expand(N, 3), o['scales_aux'][:N])
    # appearance, without and with a per-row opacity offset
    old = a.opacity_offset
    try:
        for offset in (0, off):
            a.opacity_offset = offset
            shs, op = _guarded(N, 48, dev), _guarded(N, 1, dev)
            o = frozen_appearance(x, a, out=(shs, op))
            assert torch.isnan(shs[N:]).all() and torch.isnan(op[N:]).all()
            ref = do.appearance_decoder(x64, sda, opacity_offset=offset.cpu().double() if torch.is_tensor(offset) else 0)
            per = frozen_appearance(x, a, fused=False)
            tag = f"app N={N} offset={torch.is_tensor(offset)}"
            assert o['shs'].shape == (N, 16, 3)
            _close(_np(o['shs']), ref['shs'].numpy(), what=tag + " shs vs fp64")
            _close(_np(op[:N]), ref['opacity'].numpy(), what=tag + " opacity vs fp64")
            _close(_np(o['shs']), _np(per['shs']), what=tag + " shs vs per-layer")
            _close(_np(op[:N]), _np(per['opacity']), what=tag + " opacity vs per-layer")
    finally:
        a.opacity_offset = old


def _field(dev, feature_minor=False):
    from sings_amd.decode import HexPlaneField
    torch.manual_seed(21)
    return HexPlaneField(CFG, device=dev, feature_minor=feature_minor)


@pytest.mark.parametrize("iso, fixed_opacity", [(True, False), (False, False), (True, True)])
def test_decode_frozen_applies_thickness_and_multiplier_like_decode_attributes(iso, fixed_opacity):
    from sings_amd import decode, side_launch
    dev = _dev()
    N = 3 * R + 5
    g, a, sdg, sda = _decoders(dev, iso, fixed_opacity)
    f = _field(dev)
    rs = np.random.RandomState(5)
    xyz = torch.from_numpy(rs.uniform(-0.95, 0.95, (N, 3)).astype(np.float32)).to(dev)
    sm = torch.from_numpy(rs.uniform(0.5, 2.0, (N, 1)).astype(np.float32)).to(dev)
    with torch.no_grad():
        want = decode.decode_attributes(xyz, f, g, a, thickness_factor=0.7, scaling_multiplier=sm)
    got = decode.decode_frozen(xyz, f, g, a, thickness_factor=0.7, scaling_multiplier=sm)
    slow = decode.decode_frozen(xyz, f, g, a, thickness_factor=0.7, scaling_multiplier=sm, fused=False)
    assert set(got) == set(want) == set(slow)
    assert not side_launch.pending()[1]
    # fp64: the features from the oracle's lookup, the decoders on them
    feats = do.triplane_features(xyz.cpu().double(), [[p.detach().cpu().double() for p in gp] for gp in f.grids], f.aabb.detach().cpu().double())
    og = do.geometry_decoder(feats, sdg, isotropic=iso)
    ref_scales = og['scales'].clone(); ref_scales[:, -1] *= 0.7; ref_scales = ref_scales * sm.cpu().double()
    _close(_np(got["scales"]), ref_scales.numpy(), what="scales vs fp64")
    _close(_np(got["xyz_canon"]), (xyz.cpu().double() + og['xyz_offsets']).numpy(), what="xyz_canon vs fp64")
    for k, v in want.items():
        if v is None:
            assert got[k] is None and slow[k] is None and iso
            continue
        assert got[k].shape == v.shape and got[k].grad_fn is None
        _close(_np(got[k]), _np(v), what=f"decode_frozen {k} vs decode_attributes")
        _close(_np(slow[k]), _np(v), what=f"decode_frozen(fused=False) {k} vs decode_attributes")
    if fixed_opacity:
        assert bool((got["opacity"] == 1).all())


# ---- the flags, through decode_attributes ------------------------------------------------------------------------------------------
OUT_KEYS = ("xyz_canon", "xyz_offsets", "rot6d_canon", "scales_aux", "scales", "opacity", "shs")


def _weights(N, dev):
    rs = np.random.RandomState(77)
    shapes = {"xyz_canon": (N, 3), "xyz_offsets": (N, 3), "rot6d_canon": (N, 6), "scales_aux": (N, 3), "scales": (N, 3), "opacity": (N, 1),
              "shs": (N, 16, 3)}
    return {k: torch.from_numpy(rs.normal(0, 1, s).astype(np.float32)) for k, s in shapes.items()}


def _weighted_sum(out, w):
    return sum((out[k] * w[k].to(out[k].device, out[k].dtype)).sum() for k in OUT_KEYS if out[k] is not None)


@pytest.mark.parametrize("feature_minor", [False, True])
@pytest.mark.parametrize("opt_geo, opt_app", [(False, False), (False, True), (True, False)])
def test_flags_values_and_gradients(opt_geo, opt_app, feature_minor):
    from sings_amd import decode, side_launch
    from sings_amd.decode import AppearanceDecoder, GeometryDecoder
    dev = _dev()
    N = 3 * R + 5
    torch.manual_seed(9)
    f = _field(dev, feature_minor)
    g = GeometryDecoder(96, isotropic=False).to(dev); a = AppearanceDecoder(96).to(dev)
    rs = np.random.RandomState(6)
    xyz = torch.from_numpy(rs.uniform(-0.95, 0.95, (N, 3)).astype(np.float32)).to(dev).requires_grad_(True)
    a.opacity_offset = torch.from_numpy(rs.uniform(0, 1, (N, 1)).astype(np.float32)).to(dev)
    w = _weights(N, dev)
    with torch.no_grad():
        full = decode.decode_attributes(xyz, f, g, a, thickness_factor=0.7)
    with side_launch.triplane_prepare_held(True):                        # (as the training step decodes: a preparation would be QUEUED)
        out = decode.decode_attributes(xyz, f, g, a, thickness_factor=0.7, opt_geo=opt_geo, opt_app=opt_app)
    for k in OUT_KEYS:
        _close(_np(out[k]), _np(full[k]), what=f"flags ({opt_geo}, {opt_app}) {k} vs the unfrozen call")
    frozen_keys = (() if opt_geo else ("xyz_offsets", "rot6d_canon", "scales_aux", "scales")) + (() if opt_app else ("opacity", "shs"))
    for k in OUT_KEYS:
        assert out[k].requires_grad == (k not in frozen_keys), k          # (xyz_canon = xyz + offsets keeps the gradient to xyz)
    if not (opt_geo or opt_app):
        assert not side_launch.pending()[1], "a tri-plane backward preparation was queued for a lookup nobody differentiates"
    _weighted_sum(out, w).backward()
    # ---- fp64 autograd over the oracle, the frozen decoder under no_grad: the reference's literal construct
    x64 = xyz.detach().cpu().double().requires_grad_(True)
    grids = [[p.detach().cpu().double().requires_grad_(True) for p in gp] for gp in f.grids]
    sdg = {k: v.detach().cpu().double().requires_grad_(True) for k, v in g.named_parameters()}
    sda = {k: v.detach().cpu().double().requires_grad_(True) for k, v in a.named_parameters()}
    off64 = a.opacity_offset.cpu().double()

    def geo_fn(feats):
        return do.geometry_decoder(feats, sdg, isotropic=False)

    def app_fn(feats):
        return do.appearance_decoder(feats, sda, opacity_offset=off64)
    if opt_geo or opt_app:
        feats = do.triplane_features(x64, grids, f.aabb.detach().cpu().double())
    else:
        with torch.no_grad():
            feats = do.triplane_features(x64, grids, f.aabb.detach().cpu().double())
    if opt_geo:
        og = geo_fn(feats)
    else:
        with torch.no_grad():
            og = geo_fn(feats)
    if opt_app:
        oa = app_fn(feats)
    else:
        with torch.no_grad():
            oa = app_fn(feats)
    scales = torch.cat([og['scales'][:, :-1], og['scales'][:, -1:] * 0.7], dim=1)
    ref = {"xyz_canon": x64 + og['xyz_offsets'], "xyz_offsets": og['xyz_offsets'], "rot6d_canon": og['rotations'],
           "scales_aux": og['scales_aux'], "scales": scales, "opacity": oa['opacity'], "shs": oa['shs']}
    _weighted_sum(ref, w).backward()
    _close(_np(xyz.grad), x64.grad.numpy(), rtol=1e-4, atol_scale=1e-5, what="xyz.grad")
    for gp, gc in zip(f.grids, grids):
        for p, q in zip(gp, gc):
            if opt_geo or opt_app:
                _close(_np(p.grad), q.grad.numpy(), rtol=1e-4, atol_scale=1e-5, what="plane gradient")
            else:
                assert p.grad is None and q.grad is None
    for dec, sd, live in ((g, sdg, opt_geo), (a, sda, opt_app)):
        for k, p in dec.named_parameters():
            if live:
                _close(_np(p.grad), sd[k].grad.numpy(), atol_scale=2e-5, atol=2e-5, what=f"parameter gradient {k}")
            else:
                assert p.grad is None and sd[k].grad is None, k
    assert not side_launch.pending()[1]
