"""Host tests of the gated densification statistics (include/sings_density.h, ``_lib._PROTOTYPES_DENSITY``, sings_amd/density.py): the
eighth header is held to its table, the refusals come before any HIP call with their exact text, the numpy twin follows the rule on
a case worked by hand, and the trainer gained a method, not a constructor parameter."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from sings_amd import _lib
from sings_amd import density as dn


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_density.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_DENSITY) == ["sg_density_stats"]
    assert all(n.startswith("sg_density_") for n in _lib._PROTOTYPES_DENSITY)
    others = (set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL) | set(_lib._PROTOTYPES_MESH_TERMS) | set(_lib._PROTOTYPES_ORDER)
              | set(_lib._PROTOTYPES_SAMPLER) | set(_lib._PROTOTYPES_FROZEN) | set(_lib._PROTOTYPES_FEED))
    assert not set(_lib._PROTOTYPES_DENSITY) & others
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
    assert _lib.HAS_DENSITY
    for ret, name, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is {"int": C.c_int, "size_t": C.c_size_t}.get(ret, C.c_char_p), name
        params = [p.strip() for p in params.split(",")]
        assert len(fn.argtypes) == len(params) == 9, name
        for p, t in zip(params, fn.argtypes):
            if "*" in p:
                assert issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)), (name, p)
            else:
                assert t is scalars[[w for w in re.findall(r"\w+", p) if w not in ("const", "unsigned")][0]], (name, p)


def test_constants_match_the_header_and_the_other_tables_are_untouched(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_density.h")).read()
    for name in ("MAX_K", "BLOCK"):
        m = re.search(r"#define SG_DENSITY_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "DENSITY_" + name), name
    assert (_lib.DENSITY_MAX_K, _lib.DENSITY_BLOCK) == (16, 256) and _lib.DENSITY_MAX_K == _lib.MAX_FRAMES
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES) and _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    assert len(_lib._PROTOTYPES) == 105
    assert [len(t) for t in (_lib._PROTOTYPES_EVAL, _lib._PROTOTYPES_MESH_TERMS, _lib._PROTOTYPES_ORDER, _lib._PROTOTYPES_SAMPLER,
                             _lib._PROTOTYPES_FROZEN, _lib._PROTOTYPES_FEED)] == [2, 2, 2, 2, 2, 2]
    for other in ("sings_hip.h", "sings_eval.h", "sings_mesh_terms.h", "sings_order.h", "sings_sampler.h", "sings_frozen.h",
                  "sings_feed.h"):
        assert "sg_density_" not in open(os.path.join(repo_root, "include", other)).read(), other


# ---- refusals: plausible pointers that are never dereferenced ---------------------------------------------------------------------
def _stats(**kw):
    lib = _lib.load()
    f = C.c_void_p(0x1000)
    a = dict(K=3, N=1000, grad=f, radii=f, gate=f, accum=f, denom=f, max_radii=f)
    a.update(kw)
    rc = lib.sg_density_stats(a["K"], a["N"], a["grad"], a["radii"], a["gate"], a["accum"], a["denom"], a["max_radii"], None)
    return rc, lib.sg_last_error().decode()


@pytest.mark.parametrize("kw, text", [
    (dict(N=-1), "N = -1 is negative"),
    (dict(N=-1, K=0), "N = -1 is negative"),
    (dict(K=0), "K = 0 outside 1..16"),
    (dict(K=-3), "K = -3 outside 1..16"),
    (dict(K=17), "K = 17 outside 1..16"),
    (dict(K=17, N=0), "K = 17 outside 1..16"),
    (dict(grad=None), "null pointer"), (dict(radii=None), "null pointer"), (dict(accum=None), "null pointer"),
    (dict(denom=None), "null pointer"), (dict(max_radii=None), "null pointer"),
    (dict(grad=None, radii=None, gate=None, accum=None, denom=None, max_radii=None), "null pointer"),
])
def test_stats_refuses_bad_arguments_before_any_launch(kw, text):
    rc, err = _stats(**kw)
    assert rc == 1 and err == f"sg_density_stats: {text}: invalid argument", err


def test_no_gaussians_is_a_no_op_without_a_launch():
    assert _stats(N=0)[0] == 0
    assert _stats(N=0, grad=None, radii=None, gate=None, accum=None, denom=None, max_radii=None)[0] == 0


# ---- the twin --------------------------------------------------------------------------------------------------------------------
def _hand_case():
    grad = np.zeros((2, 4, 3), np.float32)
    grad[0, 0], grad[1, 0] = (3, 4, np.nan), (6, 8, np.nan)      # visible twice: 5 + 10
    grad[0, 1], grad[1, 1] = (np.nan, 1, 0), (0.5, 0, np.nan)    # visible in frame 1 only; frame 0's NaN is never read
    grad[:, 2] = np.inf                                          # never visible
    grad[0, 3] = (0, 0, 7)                                       # visible, zero gradient
    radii = np.array([[2, 0, 0, 9], [7, 3, -1, 0]], np.int32)
    return grad, radii, np.array([[1.0], [2.0], [3.0], [4.0]], np.float32), np.full((4, 1), 10.0, np.float32), \
        np.array([5.0, 5.0, 5.0, 5.0], np.float32)


def test_the_twin_on_a_case_worked_by_hand():
    grad, radii, accum, denom, mx = _hand_case()
    a, d, m = dn.densify_stats_host(grad, radii, accum, denom, mx)
    assert a.dtype == np.float64 and a.shape == (4, 1) and d.shape == (4, 1) and m.shape == (4,)
    assert a.reshape(-1).tolist() == [16.0, 2.5, 3.0, 4.0]
    assert d.reshape(-1).tolist() == [12.0, 11.0, 10.0, 11.0]
    assert m.tolist() == [7.0, 5.0, 5.0, 9.0]
    assert accum.reshape(-1).tolist() == [1.0, 2.0, 3.0, 4.0]    # (the inputs are not written)
    for gate, moved in ((None, True), ([1], True), (np.array([7], np.int32), True), ([0], False), (np.zeros(1, np.int32), False)):
        got = dn.densify_stats_host(grad, radii, accum, denom, mx, gate=gate)
        assert (got[0].reshape(-1).tolist() == [16.0, 2.5, 3.0, 4.0]) == moved
        if not moved:
            assert all(np.array_equal(x, y) for x, y in zip(got, (accum, denom, mx)))
    one = dn.densify_stats_host(grad[1], radii[1], accum, denom, mx)      # [N,3] is [1,N,3]
    assert one[0].reshape(-1).tolist() == [11.0, 2.5, 3.0, 4.0] and one[2].tolist() == [7.0, 5.0, 5.0, 5.0]


# ---- the Python objects, where no GPU is needed ------------------------------------------------------------------------------------
def test_the_trainer_gained_a_method_not_a_parameter():
    from sings_amd.train_loop import AvatarTrainer
    sig = inspect.signature(AvatarTrainer.__init__)
    assert list(sig.parameters) == ["self", "module", "settings_fn", "bg_color", "lrs", "smpl_scale", "transl", "use_graph", "fp",
                                    "sh_degree", "max_sh_degree", "betas", "eps", "optimizer", "lr_schedules", "poses", "mesh",
                                    "mesh_terms", "lpips_sampler", "decoder_schedule", "frames"]
    assert callable(AvatarTrainer.set_density_schedule) and callable(AvatarTrainer.run)
    assert list(inspect.signature(AvatarTrainer.set_density_schedule).parameters) == ["self", "schedule"]


def test_the_module_defaults_keep_todays_path():
    from sings_amd.train_step import AvatarStep
    src = inspect.getsource(AvatarStep.__init__)
    assert "self.stats_gate = None" in src and 'self.l2_keys = ("xyz_offsets", "scales", "opacity")' in src


def test_the_statistics_live_on_the_gpu():
    import torch
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dn.densify_stats(z(4, 3), z(4, dtype=torch.int32), z(4, 1), z(4, 1), z(4))
