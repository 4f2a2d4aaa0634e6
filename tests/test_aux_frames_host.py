"""CPU tests of the K-frame depth / alpha map boundary (entry points added to ABI 8): the four new symbols are declared and exported
with the ABI still at 8, the K-frame aux workspace is K single-view ones, every entry point refuses bad settings, bad frame batches,
the flags that have no AUX kernels and missing workspaces / maps before anything is launched, and the Python surface takes
``return_aux`` last with no CPU fallback."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

FRAMES_AUX = ("sg_frames_aux_layout", "sg_skinned_forward_frames_aux", "sg_rasterize_backward_records_frames_aux",
              "sg_skinned_backward_gaussians_frames_aux")
FAKE = C.c_void_p(0x1000)


def test_frames_aux_symbols_declared_and_exported_abi_still_8(repo_root):
    from sings_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "sings_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sg_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.load()
    for name in FRAMES_AUX:
        assert name in declared and name in _lib.EXPORTS
        assert hasattr(lib, name) and getattr(lib, name).argtypes
    assert _lib.ABI_VERSION == 8 == lib.sg_abi_version()
    assert b"abi 8" in lib.sg_version()


@pytest.mark.parametrize("K", [1, 3, 8, 16])
def test_frames_aux_layout_is_k_single_view_workspaces(K):
    from sings_amd import _lib
    for P, W, H, cap in ((1000, 160, 288, 50000), (150000, 512, 896, 2000000)):
        assert _lib.frames_aux_layout(P, W, H, cap, K) == K * _lib.aux_layout(P, W, H, cap)


def test_frames_aux_layout_refuses_bad_k_and_sizes():
    from sings_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(0)
    for K in (0, 17, -1):
        assert lib.sg_frames_aux_layout(100, 64, 64, 1000, K, C.byref(n)) != 0
        assert b"sg_frames_aux_layout" in lib.sg_last_error() and b"K must be 1..16" in lib.sg_last_error()
    assert lib.sg_frames_aux_layout(100, 64, 64, 1000, 2, None) != 0
    with pytest.raises(RuntimeError, match="2\\^20 tiles"):
        _lib.frames_aux_layout(10, 16 * 1024, 16 * 1024, 10, 2)


def _settings(flags=0, side=64):
    from sings_amd import _lib
    st = _lib.SgRasterSettings()
    st.image_height = st.image_width = side
    st.tanfovx = st.tanfovy = 0.5; st.scale_modifier = 1.0; st.sh_degree = 0; st.sh_coeffs = 1
    st.bg = st.viewmatrix = st.projmatrix = st.campos = 0x1000                   # never dereferenced
    st.flags = flags
    return st


def _batch(K=3, cam=0, tr=0):
    from sings_amd import _lib
    fb = _lib.SgFrameBatch()
    fb.K, fb.camera_stride, fb.transl_stride, fb.reserved = K, cam, tr, 0
    return fb


def _skin():
    from sings_amd import _lib
    k = _lib.SgSkinInputs(); k.J = 24; k.rot_format = 0
    k.xyz_canon = k.lbs_weights = k.A = 0x1000
    return k


def _fwd(lib, st, fb=None, aux=FAKE, depth=FAKE, alpha=FAKE):
    f = FAKE
    return lib.sg_skinned_forward_frames_aux(C.byref(st), C.byref(fb or _batch()), 1, C.byref(_skin()), f, f, f, f, f, 10, f, f, f,
                                             None, None, None, None, aux, depth, alpha, None)


def _rec(lib, st, fb=None, aux=FAKE):
    f = FAKE
    return lib.sg_rasterize_backward_records_frames_aux(C.byref(st), C.byref(fb or _batch()), 1, f, f, 10, f, f, f, aux, None, None,
                                                        None)


def _gau(lib, st, fb=None, aux=FAKE, accumulate=0):
    f = FAKE
    return lib.sg_skinned_backward_gaussians_frames_aux(C.byref(st), C.byref(fb or _batch()), 1, C.byref(_skin()), f, f, f, f, f, f,
                                                        10, f, f, accumulate, None, None, f, None, f, f, f, f, f, None, aux, None)


CALLS = {"sg_skinned_forward_frames_aux": _fwd, "sg_rasterize_backward_records_frames_aux": _rec,
         "sg_skinned_backward_gaussians_frames_aux": _gau}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_frames_aux_entry_points_reject_bad_settings(name):
    from sings_amd import _lib
    lib = _lib.load()
    rc = CALLS[name](lib, _settings(side=16 * 1024))                  # 2^20 tiles: refused before anything is dereferenced
    assert rc != 0 and b"bad settings" in lib.sg_last_error() and name.encode() in lib.sg_last_error()
    st = _settings(); st.bg = 0
    assert CALLS[name](lib, st) != 0 and b"bad settings" in lib.sg_last_error()


@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("flag", ["FORWARD_BINNING", "FORWARD_COMPOSITE", "SH_PLANAR"])
def test_frames_aux_entry_points_refuse_unsupported_flags(name, flag):
    from sings_amd import _lib
    lib = _lib.load()
    rc = CALLS[name](lib, _settings(getattr(_lib, "FLAG_" + flag) | _lib.FLAG_THROUGHPUT))
    assert rc != 0
    err = lib.sg_last_error().decode()
    assert name in err and "SG_FLAG_" + flag in err and "not supported" in err


@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("fb", [(0, 0, 0), (17, 0, 0), (3, 2, 0), (3, 0, 1)])
def test_frames_aux_entry_points_refuse_bad_frame_batches(name, fb):
    from sings_amd import _lib
    lib = _lib.load()
    st = _settings(_lib.FLAG_THROUGHPUT | _lib.FLAG_LONG_ROWS | _lib.FLAG_SHORT_LISTS | _lib.FLAG_WS_CLEAN)
    assert CALLS[name](lib, st, fb=_batch(*fb)) != 0
    err = lib.sg_last_error().decode()
    assert name in err and "bad frame batch" in err


@pytest.mark.parametrize("name", sorted(CALLS))
def test_frames_aux_entry_points_require_the_aux_workspace(name):
    from sings_amd import _lib
    lib = _lib.load()
    assert CALLS[name](lib, _settings(_lib.FLAG_THROUGHPUT), aux=None) != 0
    err = lib.sg_last_error().decode()
    assert name in err and "aux_ws" in err


def test_frames_aux_forward_requires_its_maps():
    from sings_amd import _lib
    lib = _lib.load()
    st = _settings(_lib.FLAG_THROUGHPUT)
    for kw in (dict(depth=None), dict(alpha=None)):
        assert _fwd(lib, st, **kw) != 0
        err = lib.sg_last_error().decode()
        assert "sg_skinned_forward_frames_aux" in err and "out_depth / out_alpha" in err


def test_frames_aux_backward_refuses_accumulate():
    from sings_amd import _lib
    lib = _lib.load()
    assert _gau(lib, _settings(_lib.FLAG_THROUGHPUT), accumulate=1) != 0
    err = lib.sg_last_error().decode()
    assert "sg_skinned_backward_gaussians_frames_aux" in err and "accumulate" in err and "not supported" in err


def test_single_frame_aux_still_refuses_throughput():
    from sings_amd import _lib
    lib = _lib.load()
    f = FAKE
    st = _settings(_lib.FLAG_THROUGHPUT)
    rc = lib.sg_skinned_forward_aux(C.byref(st), 1, C.byref(_skin()), f, f, f, f, f, 10, f, f, f, None, None, None, None, f, f, f,
                                    None)
    assert rc != 0 and "SG_FLAG_THROUGHPUT" in lib.sg_last_error().decode()


def test_python_signatures_take_return_aux_last():
    from sings_amd import posed, renderer, skinned
    for fn in (skinned.rasterize_skinned_frames, renderer.get_render_pkgs_fused, posed.FrameAnimator.render_frames_batched,
               posed.animate_chunk):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "return_aux" and p["return_aux"].default is False, fn.__name__
    from sings_amd.engine import SkinnedFramesEngine
    p = inspect.signature(SkinnedFramesEngine.__init__).parameters
    assert list(p)[-1] == "aux" and p["aux"].default is False
    p = inspect.signature(SkinnedFramesEngine.backward_records).parameters
    assert list(p)[1:] == ["dL_dcolor", "dL_ddepth", "dL_dalpha"]


def test_frames_return_aux_has_no_cpu_fallback():
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.skinned import rasterize_skinned_frames
    rs = GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False,
                                       False)
    N, J, K = 4, 2, 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rasterize_skinned_frames(torch.zeros(N, 3), None, torch.ones(N, 3), torch.ones(N, 1), torch.zeros(N, 1, 3),
                                 torch.full((N, J), 0.5), torch.eye(4).expand(K, J, 4, 4), rs, return_aux=True)


def test_animate_chunk_refuses_maps_on_the_streams_path():
    """``streams`` > 1 per frame (FrameAnimator.render_frames) has no maps: refused, not silently dropped."""
    from sings_amd import posed

    class _FakeAnimator:
        def render_frames(self, jobs, bg):
            raise AssertionError("not reached")
    canon = dict(xyz_canon=torch.zeros(4, 3))
    gen = posed.animate_chunk(canon, torch.zeros(2, 24, 3), torch.zeros(24, 3), torch.eye(4).expand(24, 4, 4), {}, torch.zeros(3),
                              animator=_FakeAnimator(), return_aux=True)
    with pytest.raises(ValueError, match="return_aux"):
        next(gen)
