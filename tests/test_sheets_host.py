"""Host tests of the run's pictures (include/sings_sheet.h, ``_lib._PROTOTYPES_SHEET``, sings_amd/sheets.py, canonical.py, run_outputs.py):
the ninth header is held to its table, the refusals come before any HIP call, the sheet geometry is torchvision's published layout, the
predefined poses are the reference's values, ``RunOutputs.due`` is the reference's rule, and the trainer gained a method, not a parameter."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from sings_amd import _lib
from sings_amd import canonical as cn
from sings_amd import sheets as sh


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_sheet.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_SHEET) == ["sg_image_sheets"]
    others = (set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL) | set(_lib._PROTOTYPES_MESH_TERMS) | set(_lib._PROTOTYPES_ORDER)
              | set(_lib._PROTOTYPES_SAMPLER) | set(_lib._PROTOTYPES_FROZEN) | set(_lib._PROTOTYPES_FEED) | set(_lib._PROTOTYPES_DENSITY))
    assert not set(_lib._PROTOTYPES_SHEET) & others
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
    assert _lib.HAS_SHEET
    for ret, name, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is {"int": C.c_int, "size_t": C.c_size_t}.get(ret, C.c_char_p), name
        params = [p.strip() for p in params.split(",")]
        assert len(fn.argtypes) == len(params) == 14, name
        for p, t in zip(params, fn.argtypes):
            if "*" in p:
                assert issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)), (name, p)
            else:
                assert t is scalars[[w for w in re.findall(r"\w+", p) if w not in ("const", "unsigned")][0]], (name, p)


def test_constants_match_the_header_and_the_other_tables_are_untouched(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_sheet.h")).read()
    for name in ("TRUNC", "ROUND", "MAX_SHEETS", "BLOCK"):
        m = re.search(r"#define SG_SHEET_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "SHEET_" + name), name
    assert sh.QUANT == {"trunc": _lib.SHEET_TRUNC, "round": _lib.SHEET_ROUND}
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES) and _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    assert len(_lib._PROTOTYPES) == 105
    for other in ("sings_hip.h", "sings_eval.h", "sings_mesh_terms.h", "sings_order.h", "sings_sampler.h", "sings_frozen.h",
                  "sings_feed.h", "sings_density.h"):
        assert "sg_image_sheets" not in open(os.path.join(repo_root, "include", other)).read(), other


# ---- refusals: plausible pointers that are never dereferenced ---------------------------------------------------------------------
def _sheets(**kw):
    lib = _lib.load()
    f = C.c_void_p(0x1000)
    a = dict(S=2, T=4, width=8, height=4, nrow=4, padding=2, pad_value=0.0, quant=_lib.SHEET_ROUND, bgr=0, a=f, b=None, mask=None, out=f)
    a.update(kw)
    rc = lib.sg_image_sheets(a["S"], a["T"], a["width"], a["height"], a["nrow"], a["padding"], a["pad_value"], a["quant"], a["bgr"],
                             a["a"], a["b"], a["mask"], a["out"], None)
    return rc, lib.sg_last_error().decode()


@pytest.mark.parametrize("kw, text", [
    (dict(a=None), "null pointer"), (dict(out=None), "null pointer"), (dict(a=None, out=None, S=0), "null pointer"),
    (dict(S=0), "must all be >= 1"), (dict(T=0), "must all be >= 1"), (dict(width=0), "must all be >= 1"),
    (dict(height=-4), "must all be >= 1"), (dict(nrow=0), "must all be >= 1"),
    (dict(padding=-1), "padding = -1 is negative"),
    (dict(quant=2), "unknown quant 2"), (dict(quant=-1), "unknown quant -1"),
    (dict(T=5, b=C.c_void_p(0x2000)), "T = 5 is odd with a second tensor"),
    (dict(S=65536), "S = 65536 sheets, at most 65535 per launch"),
    (dict(width=1 << 20, height=1 << 12, T=1), "at most 2^31 - 1 per sheet"),
    (dict(width=2147483647, height=1, T=1, padding=2), "at most 2^31 - 1 per sheet"),
    (dict(width=60000, height=60000, T=1, padding=0), "at most 2^31 - 1 per sheet"),
])
def test_sheets_refuses_bad_arguments_before_any_launch(kw, text):
    rc, err = _sheets(**kw)
    assert rc == 1 and err.startswith("sg_image_sheets: ") and text in err and err.endswith(": invalid argument"), err


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def test_sheet_geometry_is_make_grids():
    from sheet_case import geometry
    H, W = 48, 64
    assert sh.sheet_geometry(2, H, W, nrow=2, padding=2) == (H + 4, 2 * W + 6, 2, 1)      # the shape comparison_grid returns
    from sings_amd.validate import comparison_grid
    assert tuple(comparison_grid(torch.zeros(3, H, W), torch.zeros(3, H, W)).shape[1:]) == sh.sheet_geometry(2, H, W, 2, 2)[:2]
    assert sh.sheet_geometry(5, H, W, nrow=4, padding=2) == (2 * (H + 2) + 2, 4 * (W + 2) + 2, 4, 2)       # an incomplete last row
    assert sh.sheet_geometry(1, H, W, nrow=8, padding=0) == (H, W, 1, 1)                  # the frame itself
    assert sh.sheet_geometry(3, H, W, nrow=8, padding=2) == (H + 4, 3 * (W + 2) + 2, 3, 1)                 # T < nrow shrinks xmaps
    assert sh.sheet_geometry(2, H, W, nrow=2, padding=0) == (H, 2 * W, 2, 1)              # the training picture
    for args in ((7, 3, 5, 4, 2), (8, 4, 8, 4, 0), (1, 2, 6, 1, 3), (9, 5, 5, 2, 1)):
        assert sh.sheet_geometry(*args) == geometry(*args)
    for bad in ((0, 4, 4, 4, 2), (1, 0, 4, 4, 2), (1, 4, 4, 0, 2), (1, 4, 4, 4, -1)):
        with pytest.raises(ValueError):
            sh.sheet_geometry(*bad)


def test_the_numpy_sheet_on_a_case_worked_by_hand():
    from sheet_case import quantise, sheets
    x = np.array([np.nan, -np.inf, np.inf, -0.0, 0.5, 1 / 255, 0.999, 1.0, 254.5 / 255], np.float32)
    assert quantise(x, "trunc").tolist() == [0, 0, 255, 0, 127, 1, 254, 255, 254]
    assert quantise(x, "round").tolist() == [0, 0, 255, 0, 128, 1, 255, 255, 255]
    a = np.full((3, 3, 1, 2), 1.0, np.float32)
    out = sheets(a, nrow=2, padding=1, pad_value=0.5, quant="round")
    assert out.shape == (1, 5, 7, 3) and out[0, 1, 1:3].tolist() == [[255] * 3] * 2 and out[0, 0].tolist() == [[128] * 3] * 7
    assert out[0, 3, 1:3].tolist() == [[255] * 3] * 2 and out[0, 3, 4:6].tolist() == [[128] * 3] * 2        # the empty cell is border


# ---- predefined poses --------------------------------------------------------------------------------------------------------------
def test_predefined_poses_are_the_references(repo_root):
    g = np.load(os.path.join(repo_root, "tests", "golden", "canon_pose_golden.npz"))
    assert tuple(g["pose_types"].tolist()) == cn.POSE_TYPES and len(cn.POSE_TYPES) == 5
    betas = torch.from_numpy(g["betas_in"])
    for name in cn.POSE_TYPES:
        pose = cn.predefined_pose(name)
        assert pose.dtype == torch.float32 and tuple(pose.shape) == (69,)
        assert np.array_equal(pose.numpy().view(np.int32), g[f"pose/{name}"].view(np.int32)), name
        params = cn.smpl_static_params(betas, pose_type=name)
        assert list(params) == g[f"static_keys/{name}"].tolist(), name
        for k, v in params.items():
            want = g[f"static/{name}/{k}"]
            assert v.dtype == torch.float32 and tuple(v.shape) == want.shape and np.array_equal(v.numpy().view(np.int32), want.view(np.int32)), (name, k)
    with pytest.raises(ValueError, match="Unknown pose type"):
        cn.predefined_pose("x_pose")
    with pytest.raises(ValueError, match="Unknown pose type"):
        cn.smpl_static_params(betas, pose_type="sitting")


def test_static_A_goes_through_the_bodys_chain():
    from sings_amd import body
    rs = np.random.RandomState(4)
    joints = torch.from_numpy(rs.normal(0, 0.3, (24, 3))).double()
    A_t2cano = body.joint_transforms(torch.from_numpy(rs.normal(0, 0.2, 72)).double(), joints)
    got = cn.static_A("a_pose", joints, A_t2cano)
    pose = torch.cat([torch.zeros(3), cn.predefined_pose("a_pose")]).double()
    assert torch.equal(got, body.cano_to_pose(body.joint_transforms(pose, joints), A_t2cano)) and tuple(got.shape) == (24, 4, 4)
    assert torch.equal(cn.static_A(pose, joints, A_t2cano), got)
    parents52 = tuple([-1] + list(range(51)))
    with pytest.raises(ValueError, match="pass the full axis-angle pose"):
        cn.static_A("da_pose", torch.zeros(52, 3), torch.eye(4).repeat(52, 1, 1), parents52)
    with pytest.raises(ValueError, match="must hold 156 values"):
        cn.static_A(torch.zeros(72), torch.zeros(52, 3), torch.eye(4).repeat(52, 1, 1), parents52)


# ---- the Python objects, where no GPU is needed ------------------------------------------------------------------------------------
def test_due_is_the_references_rule():
    from sings_amd.run_outputs import RunOutputs
    collect = lambda path, array: None
    for viz, prog in ((3, 2), (5, None), (1, 4), (4, 4)):
        ro = RunOutputs("unused", None, None, viz_interval=viz, progress_interval=prog, write=collect)
        for t in range(0, 2 * viz + 1):
            want = ({"viz"} if t % viz == 0 else set()) | ({"progress"} if prog is not None and t % prog == 0 else set())
            assert ro.due(t) == want, (viz, prog, t)
    assert list(inspect.signature(RunOutputs.__init__).parameters) == ["self", "logdir", "A_static", "bg_color", "viz_interval",
                                                                       "progress_interval", "canon_nframes", "save_ply", "write"]
    with pytest.raises(ValueError):
        RunOutputs("unused", None, None, viz_interval=0, write=collect)


def test_the_trainer_gained_a_method_not_a_parameter():
    from sings_amd.train_loop import AvatarTrainer
    assert list(inspect.signature(AvatarTrainer.__init__).parameters) == [
        "self", "module", "settings_fn", "bg_color", "lrs", "smpl_scale", "transl", "use_graph", "fp", "sh_degree", "max_sh_degree",
        "betas", "eps", "optimizer", "lr_schedules", "poses", "mesh", "mesh_terms", "lpips_sampler", "decoder_schedule", "frames"]
    assert list(inspect.signature(AvatarTrainer.run).parameters) == ["self", "n_steps"]
    assert list(inspect.signature(AvatarTrainer.run_until).parameters) == ["self", "num_steps", "save_every", "save_dir"]
    assert list(inspect.signature(AvatarTrainer.set_outputs).parameters) == ["self", "outputs"]
    src = inspect.getsource(AvatarTrainer._run)
    assert src.index("self.outputs.after_step(self, self.iteration)") < src.index("self._apply_density_schedule_after(self.iteration)")
    assert src.index("self.opt.step()") < src.index("self.outputs.after_step(self, self.iteration)")


def test_the_sheets_live_on_the_gpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.image_sheets(torch.zeros(2, 3, 4, 4))
    from sings_amd.run_outputs import validation_grids
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        validation_grids(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.OrbitRenderer(10, 8, 8, 1, device="cpu")
