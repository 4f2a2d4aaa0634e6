"""CPU tests of the depth / alpha map boundary (ABI 8): the new entry points are declared and exported, the aux workspace is sized
like the others, the entry points refuse bad settings and the flags that have no AUX kernels before anything is launched, and the
Python surface is the one INTEGRATION.md documents."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

AUX_ENTRY_POINTS = ("sg_aux_layout", "sg_rasterize_forward_aux", "sg_rasterize_backward_aux", "sg_skinned_forward_aux",
                    "sg_skinned_backward_aux")


def test_aux_symbols_declared_and_exported(repo_root):
    from sings_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "sings_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sg_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.load()
    for name in AUX_ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 == lib.sg_abi_version()
    assert b"abi 8" in lib.sg_version()


def test_aux_layout_grows_with_capacity_and_rejects_bad_sizes():
    from sings_amd import _lib
    a = _lib.aux_layout(1000, 1920, 1080, 50000)
    b = _lib.aux_layout(1000, 1920, 1080, 500000)
    assert a % 256 == 0 and b % 256 == 0
    assert a >= 50000 * 4 and b >= 500000 * 4 and b > a            # one dL/dz float per pair + the D checkpoint plane
    # the D checkpoints: one float per checkpoint pixel, i.e. a quarter of the float4 (T, colour) checkpoints
    L = _lib.layout(1000, 1920, 1080, 500000)
    assert b >= (L.img_bytes - L.img_ckpt) // 4
    with pytest.raises(RuntimeError):
        _lib.aux_layout(10, 0, 10, 10)
    with pytest.raises(RuntimeError):
        _lib.aux_layout(-1, 16, 16, 10)
    with pytest.raises(RuntimeError, match="2\\^20 tiles"):
        _lib.aux_layout(10, 16 * 1024, 16 * 1024, 10)
    lib = _lib.load()
    assert lib.sg_aux_layout(10, 16, 16, 10, None) != 0


def _settings(flags=0, side=64):
    from sings_amd import _lib
    st = _lib.SgRasterSettings()
    st.image_height = st.image_width = side
    st.tanfovx = st.tanfovy = 0.5; st.scale_modifier = 1.0; st.sh_degree = 0; st.sh_coeffs = 1
    st.bg = st.viewmatrix = st.projmatrix = st.campos = 0x1000                   # never dereferenced
    st.flags = flags
    return st


FAKE = C.c_void_p(0x1000)


def _fwd(lib, st):
    f = FAKE
    return lib.sg_rasterize_forward_aux(C.byref(st), 1, f, f, None, f, f, f, None, f, f, 10, f, f, f, 0, None, f, f, f, None)


def _bwd(lib, st, P=1, aux=FAKE):
    f = FAKE
    return lib.sg_rasterize_backward_aux(C.byref(st), P, f, f, None, f, f, f, None, f, f, f, 10, f, f, f, f, f, f, None, f,
                                         f, f, None, aux, None, None, None)


def _skin_fwd(lib, st):
    from sings_amd import _lib
    k = _lib.SgSkinInputs(); k.J = 24; k.rot_format = 0
    k.xyz_canon = k.lbs_weights = k.A = 0x1000
    f = FAKE
    return lib.sg_skinned_forward_aux(C.byref(st), 1, C.byref(k), f, f, f, f, f, 10, f, f, f, None, None, None, None, f, f, f, None)


def _skin_bwd(lib, st, P=1, aux=FAKE):
    from sings_amd import _lib
    k = _lib.SgSkinInputs(); k.J = 24; k.rot_format = 0
    k.xyz_canon = k.lbs_weights = k.A = 0x1000
    f = FAKE
    return lib.sg_skinned_backward_aux(C.byref(st), P, C.byref(k), f, f, f, f, f, f, 10, f, f, f, f, None, None, f, None, f, f, f,
                                       f, f, None, aux, None, None, None)


CALLS = {"sg_rasterize_forward_aux": _fwd, "sg_rasterize_backward_aux": _bwd, "sg_skinned_forward_aux": _skin_fwd,
         "sg_skinned_backward_aux": _skin_bwd}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_aux_entry_points_reject_bad_settings(name):
    from sings_amd import _lib
    lib = _lib.load()
    rc = CALLS[name](lib, _settings(side=16 * 1024))                  # 2^20 tiles: refused before anything is dereferenced
    assert rc != 0 and b"bad settings" in lib.sg_last_error()
    st = _settings(); st.bg = 0
    assert CALLS[name](lib, st) != 0 and b"bad settings" in lib.sg_last_error()


@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("flag", ["THROUGHPUT", "FORWARD_BINNING", "FORWARD_COMPOSITE", "SH_PLANAR"])
def test_aux_entry_points_refuse_unsupported_flags(name, flag):
    from sings_amd import _lib
    lib = _lib.load()
    rc = CALLS[name](lib, _settings(getattr(_lib, "FLAG_" + flag)))
    assert rc != 0
    err = lib.sg_last_error().decode()
    assert name in err and "SG_FLAG_" + flag in err and "not supported" in err


def test_aux_forward_requires_its_workspace_and_maps():
    from sings_amd import _lib
    lib = _lib.load()
    st = _settings(_lib.FLAG_SHORT_LISTS | _lib.FLAG_LONG_ROWS | _lib.FLAG_WS_CLEAN)
    f = FAKE
    rc = lib.sg_rasterize_forward_aux(C.byref(st), 1, f, f, None, f, f, f, None, f, f, 10, f, f, f, 0, None, None, f, f, None)
    assert rc != 0 and b"aux_ws" in lib.sg_last_error()
    rc = lib.sg_rasterize_forward_aux(C.byref(st), 1, f, f, None, f, f, f, None, f, f, 10, f, f, f, 0, None, f, None, f, None)
    assert rc != 0 and b"out_depth" in lib.sg_last_error()


@pytest.mark.parametrize("P", [1, 0, -1])
@pytest.mark.parametrize("name", ["sg_rasterize_backward_aux", "sg_skinned_backward_aux"])
def test_aux_backward_requires_its_workspace_even_without_gaussians(name, P):
    """A null aux_ws is refused before the P <= 0 early return (the order of the K-frame calls); with it, P <= 0 does nothing."""
    from sings_amd import _lib
    lib = _lib.load()
    assert CALLS[name](lib, _settings(), P=P, aux=None) != 0
    err = lib.sg_last_error().decode()
    assert name in err and "null pointer (aux_ws)" in err
    if P <= 0:
        assert CALLS[name](lib, _settings(), P=P) == 0


def test_python_signatures():
    import diff_gaussian_rasterization as d
    from sings_amd import rasterizer, renderer, skinned
    assert d.rasterize_gaussians_aux is rasterizer.rasterize_gaussians_aux
    assert list(inspect.signature(rasterizer.rasterize_gaussians_aux).parameters) == [
        "means3D", "means2D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3Ds_precomp", "raster_settings"]
    assert list(inspect.signature(d.GaussianRasterizer.forward_aux).parameters)[1:] == [
        "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"]
    p = inspect.signature(skinned.rasterize_skinned_gaussians).parameters
    assert list(p)[-1] == "return_aux" and p["return_aux"].default is False
    for fn in (renderer.render, renderer.get_render_pkg_fused):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "return_aux" and p["return_aux"].default is False
    assert "return_aux" not in inspect.signature(renderer.get_render_pkg).parameters


def test_forward_aux_validates_and_has_no_cpu_fallback():
    import diff_gaussian_rasterization as d
    rs = d.GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                         torch.zeros(3), False, False)
    r = d.GaussianRasterizer(rs)
    m = torch.zeros(4, 3); o = torch.ones(4, 1); sh = torch.zeros(4, 16, 3); sc = torch.ones(4, 3); q = torch.zeros(4, 4)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r.forward_aux(m, m, o, scales=sc, rotations=q)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r.forward_aux(m, m, o, shs=sh)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward_aux(m, m, o, shs=sh, scales=sc, rotations=q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.rasterize_gaussians_aux(m, m, sh, torch.Tensor([]), o, sc, q, torch.Tensor([]), rs)
