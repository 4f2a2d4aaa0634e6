"""Host tests of the scene boundary (include/sings_scene.h, ``_lib._PROTOTYPES_SCENE``, sings_amd/scene_anim.py): the tenth header is
held to its table and its struct to the header's layout, every refusal comes before any HIP call with its exact text (plausible
pointers that are never dereferenced), and the Python side -- ``SceneFramesEngine.check_frames``, the batching of scene jobs --
is tested where no GPU is needed."""
import ctypes as C
import os
import re

import pytest
import torch

from sings_amd import _lib
from sings_amd import scene_anim as sa


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def _header(repo_root):
    return open(os.path.join(repo_root, "include", "sings_scene.h")).read()


def test_header_is_bound_with_its_types(repo_root):
    text = _header(repo_root)
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_SCENE) == ["sg_scene_forward_frames", "sg_scene_forward_frames_aux"]
    others = (set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL) | set(_lib._PROTOTYPES_MESH_TERMS) | set(_lib._PROTOTYPES_ORDER)
              | set(_lib._PROTOTYPES_SAMPLER) | set(_lib._PROTOTYPES_FROZEN) | set(_lib._PROTOTYPES_FEED) | set(_lib._PROTOTYPES_DENSITY)
              | set(_lib._PROTOTYPES_SHEET))
    assert not set(_lib._PROTOTYPES_SCENE) & others
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
    assert _lib.HAS_SCENE
    for ret, name, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and ret == "int", name
        params = [p.strip() for p in params.split(",")]
        assert len(fn.argtypes) == len(params), name
        for p, t in zip(params, fn.argtypes):
            if "*" in p:
                assert issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)), (name, p)
                if "SgSceneAvatar" in p:
                    assert t is C.POINTER(_lib.SgSceneAvatar), (name, p)
                if "SgRasterSettings" in p:
                    assert t is C.POINTER(_lib.SgRasterSettings), (name, p)
            else:
                assert t is scalars[[w for w in re.findall(r"\w+", p) if w not in ("const", "unsigned")][0]], (name, p)
    # the second entry point is the first plus (aux_ws, out_depth, out_alpha) in front of the stream
    a, b = (p.split(",") for _, _, p in protos)
    assert [x.strip() for x in b[:len(a) - 1]] == [x.strip() for x in a[:-1]] and len(b) == len(a) + 3


def test_the_struct_has_the_headers_layout(repo_root):
    hdr = re.sub(r"/\*.*?\*/", "", _header(repo_root), flags=re.S)
    body = re.search(r"typedef struct SgSceneAvatar \{(.*?)\} SgSceneAvatar;", hdr, flags=re.S).group(1)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        pointer = "*" in decl
        assert decl.startswith("const float" if pointer else "int32_t"), decl
        fields += [(n.strip(" *"), pointer) for n in decl.split(None, 2 if pointer else 1)[-1].split(",")]
    assert [n for n, _ in fields] == [n for n, _ in _lib.SgSceneAvatar._fields_]
    assert [p for _, p in fields] == [False] * 4 + [True] * 12
    assert [t for _, t in _lib.SgSceneAvatar._fields_] == [C.c_int32] * 4 + [C.c_void_p] * 12
    assert C.sizeof(_lib.SgSceneAvatar) == 4 * 4 + 12 * C.sizeof(C.c_void_p) == 112
    assert _lib.SgSceneAvatar.xyz_canon.offset == 16 and _lib.SgSceneAvatar.ext_scale.offset == 104


def test_constants_match_the_header_and_the_other_tables_are_untouched(repo_root):
    m = re.search(r"#define SG_SCENE_MAX_AVATARS (\d+)", _header(repo_root))
    assert m and int(m.group(1)) == _lib.SCENE_MAX_AVATARS == 8
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES) and _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    assert not any(n.startswith("sg_scene_") for n in _lib.EXPORTS)
    m = re.search(r"#define SG_ABI_VERSION (\d+)", open(os.path.join(repo_root, "include", "sings_hip.h")).read())
    assert m and int(m.group(1)) == 8
    for other in ("sings_hip.h", "sings_eval.h", "sings_mesh_terms.h", "sings_order.h", "sings_sampler.h", "sings_frozen.h", "sings_feed.h",
                  "sings_density.h", "sings_sheet.h"):
        assert "sg_scene_" not in open(os.path.join(repo_root, "include", other)).read(), other
    # ABI 8 pins the structs the scene does not touch
    assert [n for n, _ in _lib.SgSkinInputs._fields_] == ["J", "rot_format", "xyz_canon", "rot_canon", "lbs_weights", "A", "smpl_scale",
                                                          "transl", "ext_trans", "ext_rot", "ext_scale"]
    assert [n for n, _ in _lib.SgFrameBatch._fields_] == ["K", "camera_stride", "transl_stride", "placement"]


# ---- refusals: plausible pointers that are never dereferenced ---------------------------------------------------------------------
F = 0x1000
PTRS = ("xyz_canon", "rot_canon", "lbs_weights", "scales", "opacities", "shs", "A", "transl", "smpl_scale", "ext_trans", "ext_rot",
        "ext_scale")


def _settings(**kw):
    s = _lib.SgRasterSettings()
    s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.scale_modifier = 288, 160, 0.5, 0.9, 1.0
    s.sh_degree, s.sh_coeffs, s.prefiltered, s.debug, s.flags = 0, 16, 0, 0, 0
    s.bg = s.viewmatrix = s.projmatrix = s.campos = F
    s.count_signal = s.count_signal_host = None
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _avatars(n=2, **kw):
    arr = (_lib.SgSceneAvatar * max(n, 1))()
    for a in arr:
        a.P, a.J, a.rot_format, a.reserved = 300, 24, 0, 0
        for p in PTRS:
            setattr(a, p, F)
    for k, v in kw.items():                                        # (the change goes to the LAST avatar: the message names it)
        setattr(arr[n - 1], k, v)
    return arr


def _call(aux=False, settings=None, avatars=None, **kw):
    lib = _lib.load()
    f = C.c_void_p(F)
    a = dict(K=3, camera_stride=0, S=2, geom_ws=f, binning_ws=f, cap=1 << 16, image_ws=f, out_color=f, radii=f, aux_ws=f,
             out_depth=f, out_alpha=f)
    a.update(kw)
    s = _settings() if settings is None else settings
    av = _avatars(a["S"] if 1 <= a["S"] <= 8 else 2) if avatars is None else avatars
    av = None if avatars == "null" else av
    args = (C.byref(s), a["K"], a["camera_stride"], a["S"], av, a["geom_ws"], a["binning_ws"], a["cap"], a["image_ws"], a["out_color"],
            a["radii"], None, None, None, None)
    if aux:
        rc = lib.sg_scene_forward_frames_aux(*args, a["aux_ws"], a["out_depth"], a["out_alpha"], None)
    else:
        rc = lib.sg_scene_forward_frames(*args, None)
    return rc, lib.sg_last_error().decode()


REFUSALS = [
    (dict(S=0), "S = 0 outside 1..8"),
    (dict(S=9), "S = 9 outside 1..8"),
    (dict(S=-1), "S = -1 outside 1..8"),
    (dict(K=0), "K = 0 outside 1..16"),
    (dict(K=17), "K = 17 outside 1..16"),
    (dict(camera_stride=2), "camera_stride = 2, not 0 or 1"),
    (dict(camera_stride=-1), "camera_stride = -1, not 0 or 1"),
    (dict(avatars="null"), "null pointer (avatars)"),
    (dict(avatars=_avatars(P=0)), "avatar 1: P = 0, at least one Gaussian is needed"),
    (dict(avatars=_avatars(P=-5)), "avatar 1: P = -5, at least one Gaussian is needed"),
    (dict(avatars=_avatars(J=0)), "avatar 1: J = 0 outside 1..64"),
    (dict(avatars=_avatars(J=65)), "avatar 1: J = 65 outside 1..64"),
    (dict(avatars=_avatars(rot_format=2)), "avatar 1: unknown rot_format 2"),
    (dict(avatars=_avatars(reserved=1)), "avatar 1: reserved = 1, must be 0"),
    (dict(avatars=_avatars(ext_rot=None)), "avatar 1: ext_trans / ext_rot / ext_scale must be all or none"),
    (dict(avatars=_avatars(ext_trans=None, ext_scale=None)), "avatar 1: ext_trans / ext_rot / ext_scale must be all or none"),
    (dict(S=1, avatars=_avatars(1, xyz_canon=None)), "avatar 0: null pointer"),
    (dict(avatars=_avatars(lbs_weights=None)), "avatar 1: null pointer"),
    (dict(avatars=_avatars(scales=None)), "avatar 1: null pointer"),
    (dict(avatars=_avatars(opacities=None)), "avatar 1: null pointer"),
    (dict(avatars=_avatars(shs=None)), "avatar 1: null pointer"),
    (dict(avatars=_avatars(A=None)), "avatar 1: null pointer"),
    (dict(geom_ws=None), "null pointer"), (dict(binning_ws=None), "null pointer"), (dict(image_ws=None), "null pointer"),
    (dict(out_color=None), "null pointer"), (dict(radii=None), "null pointer"),
    (dict(settings=_settings(sh_degree=3, sh_coeffs=9)), "sh_coeffs smaller than (sh_degree+1)^2"),
    (dict(settings=_settings(sh_degree=1, sh_coeffs=3)), "sh_coeffs smaller than (sh_degree+1)^2"),
    (dict(settings=_settings(image_width=0)), "bad settings"),
]


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("kw, text", REFUSALS)
def test_refuses_bad_arguments_before_any_launch(kw, text, aux):
    rc, err = _call(aux=aux, **kw)
    who = "sg_scene_forward_frames_aux" if aux else "sg_scene_forward_frames"
    assert rc == 1 and err == f"{who}: {text}: invalid argument", err


@pytest.mark.parametrize("kw, text", [
    (dict(aux_ws=None), "null pointer (aux_ws)"),
    (dict(out_depth=None), "null pointer (out_depth / out_alpha)"),
    (dict(out_alpha=None), "null pointer (out_depth / out_alpha)"),
    (dict(settings=_settings(flags=_lib.FLAG_SH_PLANAR)), "SG_FLAG_SH_PLANAR is not supported with depth / alpha maps"),
    (dict(settings=_settings(flags=_lib.FLAG_FORWARD_BINNING)), "SG_FLAG_FORWARD_BINNING is not supported with depth / alpha maps"),
])
def test_the_maps_refuse_what_the_skinned_k_frame_maps_refuse(kw, text):
    rc, err = _call(aux=True, **kw)
    assert rc == 1 and err == f"sg_scene_forward_frames_aux: {text}: invalid argument", err


def test_optional_pointers_may_be_null_in_a_refused_call():
    """transl, smpl_scale, rot_canon and the three ext pointers together are optional: the call gets past the avatars (and is then
    refused for its workspace, still before any HIP call)."""
    av = _avatars(transl=None, smpl_scale=None, rot_canon=None, ext_trans=None, ext_rot=None, ext_scale=None, rot_format=1)
    rc, err = _call(avatars=av, geom_ws=None)
    assert rc == 1 and err == "sg_scene_forward_frames: null pointer: invalid argument", err


# ---- Python: set_frames' validation -----------------------------------------------------------------------------------------------
K, M = 3, 16
AV = [(40, 24, None), (17, 52, 6), (9, 23, 9)]


def _frames(**kw):
    """Valid CPU inputs of the three avatars of AV; ``kw``: name -> tensor, replaced in avatar 1 (its ``canon`` or its frame dict)."""
    g = torch.Generator().manual_seed(0)
    fr = []
    for P, J, rw in AV:
        canon = dict(xyz_canon=torch.rand(P, 3, generator=g), lbs_weights=torch.rand(P, J, generator=g), scales=torch.rand(P, 3, generator=g),
                     opacity=torch.rand(P, 1, generator=g), shs=torch.rand(P, M, 3, generator=g),
                     rotmat_canon=None if rw is None else torch.rand((P, 6) if rw == 6 else (P, 3, 3), generator=g))
        fr.append(dict(canon=canon, A=torch.rand(K, J, 4, 4, generator=g)))
    fr[1].update(transl=torch.rand(K, 3), smpl_scale=torch.rand(1), ext_tfs=(torch.rand(K, 3), torch.rand(1, 3, 3).expand(K, 3, 3), torch.rand(K, 1)))
    fr[2].update(transl=torch.rand(3), smpl_scale=torch.rand(K, 1))
    for k, v in kw.items():
        (fr[1]["canon"] if k in fr[1]["canon"] else fr[1])[k] = v
    return fr


def test_check_frames_gives_every_per_frame_input_k_rows():
    out = sa.SceneFramesEngine.check_frames(AV, K, M, _frames())
    assert [sorted(k for k, v in d.items() if v is None) for d in out] == [
        ["ext_rot", "ext_scale", "ext_trans", "rot_canon", "smpl_scale", "transl"], [], ["ext_rot", "ext_scale", "ext_trans"]]
    for d, (P, J, rw) in zip(out, AV):
        assert d["A"].shape == (K, J, 16) and d["opacities"].shape == (P,)
        assert d["rot_canon"] is None if rw is None else d["rot_canon"].shape == (P, rw)
    assert out[1]["transl"].shape == (K, 3) and out[1]["smpl_scale"].shape == (K,) and out[1]["ext_rot"].shape == (K, 9)
    assert out[1]["ext_rot"].stride(0) == 0 and torch.equal(out[1]["ext_rot"][0], out[1]["ext_rot"][2])       # (the expand view: one shared row)
    assert out[2]["transl"].shape == (K, 3) and torch.equal(out[2]["transl"][0], out[2]["transl"][K - 1])
    assert out[2]["smpl_scale"].shape == (K,) and out[2]["smpl_scale"].stride(0) == 1


@pytest.mark.parametrize("kw, text", [
    (dict(xyz_canon=torch.zeros(16, 3)), "avatar 1: xyz_canon must be [17, 3], got (16, 3)"),
    (dict(lbs_weights=torch.zeros(17, 24)), "avatar 1: lbs_weights must be [17, 52], got (17, 24)"),
    (dict(scales=torch.zeros(17, 1)), "avatar 1: scales must be [17, 3], got (17, 1)"),
    (dict(shs=torch.zeros(17, 9, 3)), "avatar 1: shs must be [17, 16, 3], got (17, 9, 3)"),
    (dict(opacity=torch.zeros(16, 1)), "avatar 1: opacity must be [17,1], got (16, 1)"),
    (dict(rotmat_canon=None), "avatar 1: rotmat_canon must be [17, 6], got None"),
    (dict(rotmat_canon=torch.zeros(17, 3, 3)), "avatar 1: rotmat_canon must be [17, 6], got (17, 3, 3)"),
    (dict(A=torch.zeros(K, 24, 4, 4)), "avatar 1: A must be [3,52,16], got (3, 24, 4, 4)"),
    (dict(A=torch.zeros(2, 52, 16)), "avatar 1: A must be [3,52,16], got (2, 52, 16)"),
    (dict(transl=torch.zeros(2, 3)), "avatar 1: transl must be [3] (one for all frames) or [3,3] (one per frame), got (2, 3)"),
    (dict(smpl_scale=torch.zeros(2)), "avatar 1: smpl_scale must be [1] (one for all frames) or [3,1] (one per frame), got (2,)"),
    (dict(ext_tfs=(torch.zeros(3), torch.zeros(2, 3, 3), torch.zeros(1))),
     "avatar 1: ext rot must be [9] (one for all frames) or [3,9] (one per frame), got (2, 3, 3)"),
    (dict(ext_tfs=(torch.zeros(3), torch.zeros(3, 3))), "avatar 1: ext_tfs must be (trans, rotmat, scale), got 2 entries"),
])
def test_check_frames_names_the_offending_shape(kw, text):
    with pytest.raises(ValueError) as e:
        sa.SceneFramesEngine.check_frames(AV, K, M, _frames(**kw))
    assert str(e.value) == text


def test_check_frames_counts_the_avatars_and_check_avatars_the_scene():
    with pytest.raises(ValueError) as e:
        sa.SceneFramesEngine.check_frames(AV, K, M, _frames()[:2])
    assert str(e.value) == "set_frames: 2 avatars, the engine was built for 3"
    assert sa.SceneFramesEngine.check_avatars([(5, 24, None), (7.0, 52, 6)]) == [(5, 24, None), (7, 52, 6)]
    for bad, text in (([], "a scene has 1..8 avatars, got 0"), ([(1, 1, None)] * 9, "a scene has 1..8 avatars, got 9"),
                      ([(5, 24, None), (0, 24, None)], "avatar 1: (P, J, rot width) = (0, 24, None): P >= 1, J in 1..64, rot width None, 6 or 9"),
                      ([(5, 65, None)], "avatar 0: (P, J, rot width) = (5, 65, None): P >= 1, J in 1..64, rot width None, 6 or 9"),
                      ([(5, 24, 4)], "avatar 0: (P, J, rot width) = (5, 24, 4): P >= 1, J in 1..64, rot width None, 6 or 9")):
        with pytest.raises(ValueError) as e:
            sa.SceneFramesEngine.check_avatars(bad)
        assert str(e.value) == text


def test_scene_structs_point_at_the_checked_tensors():
    from sings_amd._marshal import _scene_structs
    checked = sa.SceneFramesEngine.check_frames(AV, K, M, _frames())
    keep = []
    arr = _scene_structs(torch.device("cpu"), checked, keep)
    assert len(arr) == 3 and [(a.P, a.J, a.rot_format, a.reserved) for a in arr] == [(40, 24, 0, 0), (17, 52, 1, 0), (9, 23, 0, 0)]
    held = {t.data_ptr() for t in keep}
    for a, d in zip(arr, checked):
        for n in PTRS:
            p = getattr(a, n)
            assert (p is None) == (d[n] is None), n
            assert p is None or p in held, n
    # an .expand view is materialised as K rows (every per-frame array of the header has K rows)
    ext_rot = next(t for t in keep if t.data_ptr() == arr[1].ext_rot)
    assert ext_rot.shape == (K, 9) and ext_rot.is_contiguous()
    with pytest.raises(RuntimeError, match="must be float32"):
        _scene_structs(torch.device("cpu"), [dict(checked[0], xyz_canon=checked[0]["xyz_canon"].double())], [])


# ---- Python: the batching of scene jobs -------------------------------------------------------------------------------------------
def test_scene_jobs_are_batched_by_what_their_avatars_carry():
    from sings_amd.posed import _batches
    kind = lambda job: tuple(x is None for p in job[1] for x in p[1:])
    t = torch.zeros(1)
    plain, scaled = ("A", None, None, None), ("A", None, t, None)
    jobs = [("cam", [plain, scaled])] * 5 + [("cam", [plain, plain])] * 2 + [("cam", [scaled, plain])] * 9
    got = [(i0, len(b)) for i0, b in _batches(iter(jobs), 4, kind)]
    assert got == [(0, 4), (4, 1), (5, 2), (7, 4), (11, 4), (15, 1)]
    # the single-avatar jobs of FrameAnimator keep their rule (the default)
    one = [("cam", "A", None, None, None)] * 3 + [("cam", "A", None, t, None)] * 2
    assert [(i0, len(b)) for i0, b in _batches(iter(one), 8)] == [(0, 3), (3, 2)]


def test_stacked_poses_and_cameras_pad_the_tail_with_the_last_frame():
    from sings_amd.posed import _stack_poses
    A = [torch.full((24, 4, 4), float(i)) for i in range(3)]
    tr = [torch.full((3,), float(i)) for i in range(3)]
    shared = torch.ones(1, 1).expand(3, 1)
    A4, tr4, sc, ext = _stack_poses([(A[i], tr[i], shared[i], None) for i in range(3)], 4)
    assert A4.shape == (4, 24, 16) and [float(A4[k, 0, 0]) for k in range(4)] == [0.0, 1.0, 2.0, 2.0]
    assert tr4.shape == (4, 3) and [float(tr4[k, 0]) for k in range(4)] == [0.0, 1.0, 2.0, 2.0]
    assert sc.numel() == 1 and ext is None                              # (rows of one .expand view: the one shared value)
    _, _, sc, _ = _stack_poses([(A[i], None, torch.full((1,), float(i)), None) for i in range(3)], 4)
    assert sc.shape == (4, 1) and sc.reshape(-1).tolist() == [0.0, 1.0, 2.0, 2.0]


def test_the_animator_and_the_engine_need_the_gpu_and_a_scene_is_forward_only():
    canon = dict(xyz_canon=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sa.SceneAnimator([canon, canon])
    with pytest.raises(ValueError, match="a scene has 1..8 avatars, got 9"):
        sa.SceneAnimator([canon] * 9)
    for name in ("backward", "backward_records", "backward_gaussians"):
        with pytest.raises(RuntimeError, match="forward-only"):
            getattr(sa.SceneFramesEngine, name)(None)
    import inspect
    sig = inspect.signature(sa.SceneAnimator.render_frames_batched)
    assert list(sig.parameters)[1:] == ["jobs", "bg_color", "frames_per_launch", "scaling_modifier", "out", "return_aux"]
    assert (sig.parameters["frames_per_launch"].default, sig.parameters["out"].default) == (8, "float32")
    from sings_amd.posed import FrameAnimator
    assert issubclass(sa.SceneAnimator, FrameAnimator) and sa.SceneAnimator._pipeline is FrameAnimator._pipeline
