"""CPU tests of the per-frame placement of the skinned K-frame forward (SgFrameBatch.placement, SG_PLACEMENT_*) and of the 8-bit
frame output (sg_frames_to_u8): the new entry point is declared and exported with the ABI still at 8, the flag constants match the
header, ``fb.reserved`` still writes the field, and every refusal comes back through ctypes before anything is launched (fake
device pointers that are never dereferenced)."""
import ctypes as C
import os
import re

import pytest
import torch

FAKE = C.c_void_p(0x1000)


def _hdr(repo_root):
    return open(os.path.join(repo_root, "include", "sings_hip.h")).read()


def test_frames_to_u8_declared_and_exported_abi_still_8(repo_root):
    from sings_amd import _lib
    declared = set(re.findall(r"\b(sg_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", _hdr(repo_root), flags=re.S)))
    lib = _lib.load()
    assert "sg_frames_to_u8" in declared and "sg_frames_to_u8" in _lib.EXPORTS
    assert hasattr(lib, "sg_frames_to_u8") and lib.sg_frames_to_u8.argtypes
    assert _lib.ABI_VERSION == 8 == lib.sg_abi_version()


def test_placement_constants_match_the_header(repo_root):
    from sings_amd import _lib
    hdr = _hdr(repo_root)
    for name in ("EXT_TFS", "SMPL_SCALE"):
        m = re.search(r"#define SG_PLACEMENT_%s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, "PLACEMENT_" + name), name
    assert re.search(r"int32_t placement;", hdr)


def test_reserved_still_writes_the_placement_field():
    from sings_amd import _lib
    fb = _lib.SgFrameBatch()
    fb.K, fb.camera_stride, fb.transl_stride, fb.reserved = 3, 0, 0, 0
    assert fb.placement == 0 and fb.reserved == 0
    fb.reserved = 2
    assert fb.placement == 2
    assert [f for f, _ in _lib.SgFrameBatch._fields_] == ["K", "camera_stride", "transl_stride", "placement"]
    assert C.sizeof(_lib.SgFrameBatch) == 16


def _settings(flags=0, side=64):
    from sings_amd import _lib
    st = _lib.SgRasterSettings()
    st.image_height = st.image_width = side
    st.tanfovx = st.tanfovy = 0.5; st.scale_modifier = 1.0; st.sh_degree = 0; st.sh_coeffs = 1
    st.bg = st.viewmatrix = st.projmatrix = st.campos = 0x1000                   # never dereferenced
    st.flags = flags
    return st


def _batch(placement, K=3):
    from sings_amd import _lib
    fb = _lib.SgFrameBatch()
    fb.K, fb.camera_stride, fb.transl_stride, fb.placement = K, 0, 0, placement
    return fb


def _skin(ext=False, scale=False):
    from sings_amd import _lib
    k = _lib.SgSkinInputs(); k.J = 24; k.rot_format = 0
    k.xyz_canon = k.lbs_weights = k.A = 0x1000
    if ext:
        k.ext_trans = k.ext_rot = k.ext_scale = 0x1000
    if scale:
        k.smpl_scale = 0x1000
    return k


def _fwd(lib, fb, skin):
    f = FAKE
    return lib.sg_skinned_forward_frames(C.byref(_settings()), C.byref(fb), 1, C.byref(skin), f, f, f, f, f, 10, f, f, f,
                                         None, None, None, None, None)


def _fwd_aux(lib, fb, skin):
    from sings_amd import _lib
    f = FAKE
    return lib.sg_skinned_forward_frames_aux(C.byref(_settings(_lib.FLAG_THROUGHPUT)), C.byref(fb), 1, C.byref(skin), f, f, f, f, f,
                                             10, f, f, f, None, None, None, None, f, f, f, None)


FORWARDS = {"sg_skinned_forward_frames": _fwd, "sg_skinned_forward_frames_aux": _fwd_aux}


@pytest.mark.parametrize("name", sorted(FORWARDS))
def test_forward_refuses_unknown_placement_bits(name):
    from sings_amd import _lib
    lib = _lib.load()
    for bits in (4, 8 | _lib.PLACEMENT_EXT_TFS, 1 << 30):
        assert FORWARDS[name](lib, _batch(bits), _skin(ext=True, scale=True)) != 0
        err = lib.sg_last_error().decode()
        assert name in err and "unknown SgFrameBatch.placement bits" in err


@pytest.mark.parametrize("name", sorted(FORWARDS))
def test_forward_refuses_ext_bit_without_ext_tfs(name):
    from sings_amd import _lib
    lib = _lib.load()
    assert FORWARDS[name](lib, _batch(_lib.PLACEMENT_EXT_TFS), _skin(scale=True)) != 0
    err = lib.sg_last_error().decode()
    assert name in err and "SG_PLACEMENT_EXT_TFS" in err and "ext_trans" in err


@pytest.mark.parametrize("name", sorted(FORWARDS))
def test_forward_refuses_scale_bit_without_smpl_scale(name):
    from sings_amd import _lib
    lib = _lib.load()
    assert FORWARDS[name](lib, _batch(_lib.PLACEMENT_SMPL_SCALE), _skin(ext=True)) != 0
    err = lib.sg_last_error().decode()
    assert name in err and "SG_PLACEMENT_SMPL_SCALE" in err and "smpl_scale" in err


def _raster_fwd(lib, fb):
    f = FAKE
    return lib.sg_rasterize_forward_frames(C.byref(_settings()), C.byref(fb), 1, f, f, None, f, f, f, None, f, f, 10, f, f, f, None,
                                           None)


def _rec(lib, fb):
    f = FAKE
    return lib.sg_rasterize_backward_records_frames(C.byref(_settings()), C.byref(fb), 1, f, f, 10, f, f, f, None)


def _rec_aux(lib, fb):
    from sings_amd import _lib
    f = FAKE
    return lib.sg_rasterize_backward_records_frames_aux(C.byref(_settings(_lib.FLAG_THROUGHPUT)), C.byref(fb), 1, f, f, 10, f, f, f, f,
                                                        None, None, None)


def _raster_gau(lib, fb):
    f = FAKE
    return lib.sg_rasterize_backward_gaussians_frames(C.byref(_settings()), C.byref(fb), 1, f, f, None, f, f, f, None, f, f, f, 10, f,
                                                      0, f, f, f, None, f, f, f, None, None)


def _skin_gau(lib, fb):
    f = FAKE
    return lib.sg_skinned_backward_gaussians_frames(C.byref(_settings()), C.byref(fb), 1, C.byref(_skin(scale=True)), f, f, f, f, f,
                                                    f, 10, f, f, 0, None, None, f, None, f, f, f, f, f, None, None)


def _skin_gau_aux(lib, fb):
    from sings_amd import _lib
    f = FAKE
    return lib.sg_skinned_backward_gaussians_frames_aux(C.byref(_settings(_lib.FLAG_THROUGHPUT)), C.byref(fb), 1,
                                                        C.byref(_skin(scale=True)), f, f, f, f, f, f, 10, f, f, 0, None, None, f, None,
                                                        f, f, f, f, f, None, f, None)


REFUSING = {"sg_rasterize_forward_frames": _raster_fwd, "sg_rasterize_backward_records_frames": _rec,
            "sg_rasterize_backward_records_frames_aux": _rec_aux, "sg_rasterize_backward_gaussians_frames": _raster_gau,
            "sg_skinned_backward_gaussians_frames": _skin_gau, "sg_skinned_backward_gaussians_frames_aux": _skin_gau_aux}


@pytest.mark.parametrize("name", sorted(REFUSING))
@pytest.mark.parametrize("bit", ["EXT_TFS", "SMPL_SCALE"])
def test_backward_and_raster_frames_refuse_placement(name, bit):
    from sings_amd import _lib
    lib = _lib.load()
    assert REFUSING[name](lib, _batch(getattr(_lib, "PLACEMENT_" + bit))) != 0
    err = lib.sg_last_error().decode()
    assert name in err and "SG_PLACEMENT_" + bit in err and "forward-only" in err


@pytest.mark.parametrize("name", sorted(REFUSING))
def test_backward_and_raster_frames_still_pass_placement_zero_to_their_other_checks(name):
    """Placement 0 is what every caller passed before: the calls go on to their usual checks (here: a bad frame batch)."""
    from sings_amd import _lib
    lib = _lib.load()
    fb = _batch(0, K=17)
    assert REFUSING[name](lib, fb) != 0
    assert "bad frame batch" in lib.sg_last_error().decode()


def test_frames_to_u8_refuses_bad_sizes_and_null_pointers():
    from sings_amd import _lib
    lib = _lib.load()
    f = FAKE
    for K, W, H in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (2, -3, 5)):
        assert lib.sg_frames_to_u8(K, W, H, f, 0, f, None) != 0, (K, W, H)
        err = lib.sg_last_error().decode()
        assert "sg_frames_to_u8" in err and ("K must be" in err or "width and height" in err)
    for rgb, out in ((None, f), (f, None)):
        assert lib.sg_frames_to_u8(1, 4, 4, rgb, 1, out, None) != 0
        assert "sg_frames_to_u8: null pointer" in lib.sg_last_error().decode()


def test_python_surface():
    import inspect
    from sings_amd import frame_out, posed
    from sings_amd.engine import SkinnedFramesEngine
    assert list(inspect.signature(SkinnedFramesEngine.set_frames).parameters)[-1] == "ext_tfs"
    for fn in (posed.FrameAnimator.render_frames_batched, posed.animate_chunk):
        p = inspect.signature(fn).parameters
        assert p["out"].default == "float32" and list(p)[-2:] == ["out", "return_aux"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        posed.frames_to_u8(torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="out must be one of"):
        frame_out.parse_out("bgr16")


def test_frame_rows_shared_or_per_frame():
    from sings_amd._marshal import _frame_rows
    K = 5
    t, per = _frame_rows(torch.tensor([0.5]).expand(K, 1), K, 1, "s")          # the reference's .expand: shared, not copied
    assert not per and t.shape == (1,)
    base = torch.eye(3)
    t, per = _frame_rows(base.expand(K, 3, 3), K, 9, "r")
    assert not per and t.data_ptr() == base.data_ptr()
    assert _frame_rows(torch.ones(1, 3), K, 3, "t")[1] is False
    t, per = _frame_rows(torch.ones(K, 1), K, 1, "s")
    assert per and t.shape == (K, 1)
    assert _frame_rows(torch.ones(K), K, 1, "s")[1] is True
    with pytest.raises(ValueError, match=r"\[5,3\]"):
        _frame_rows(torch.ones(4, 3), K, 3, "t")
