"""Host tests of the frozen decoders (include/sings_frozen.h, ``_lib._PROTOTYPES_FROZEN``, ``train_loop.DecoderSchedule``,
``FusedAdam.set_active``'s chunk table): the sixth header is held to its table, the refusals come before any HIP call and name the
argument, the schedule is the reference's expression (gs_trainer.py:225-226) restated here, and the chunk table of an active subset
lists exactly the active parameters' chunks at their full-layout offsets."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from sings_amd import _lib


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_frozen.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_FROZEN) and len(protos) == 2
    others = (set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL) | set(_lib._PROTOTYPES_MESH_TERMS) | set(_lib._PROTOTYPES_ORDER)
              | set(_lib._PROTOTYPES_SAMPLER))
    assert not set(_lib._PROTOTYPES_FROZEN) & others
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
    assert _lib.HAS_FROZEN
    for ret, name, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is {"int": C.c_int, "size_t": C.c_size_t}.get(ret, C.c_char_p), name
        params = [p.strip() for p in params.split(",")]
        assert len(fn.argtypes) == len(params), name
        for p, t in zip(params, fn.argtypes):
            if "*" in p:
                assert issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)), (name, p)
            else:
                assert t is scalars[[w for w in re.findall(r"\w+", p) if w not in ("const", "unsigned")][0]], (name, p)


def test_constants_match_the_header_and_the_other_tables_are_untouched(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_frozen.h")).read()
    for name in ("BLOCK", "SHS"):
        m = re.search(r"#define SG_FROZEN_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "FROZEN_" + name), name
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES) and _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    for other in ("sings_hip.h", "sings_eval.h", "sings_mesh_terms.h", "sings_order.h", "sings_sampler.h"):
        assert "sg_frozen" not in open(os.path.join(repo_root, "include", other)).read(), other


# ---- refusals: plausible pointers that are never dereferenced ---------------------------------------------------------------------
GEO_PTRS = ("feats", "W_net0", "b_net0", "W_net2", "b_net2", "W_scales0", "b_scales0", "W_scales2", "b_scales2", "W_xyz", "b_xyz",
            "W_rot", "b_rot", "xyz_offsets", "scales", "scales_aux", "rotations")
APP_PTRS = ("feats", "W_net0", "b_net0", "W_net2", "b_net2", "W_shs", "b_shs", "W_opacity", "b_opacity", "opacity_offset", "shs",
            "opacity")


def _geometry(**kw):
    lib = _lib.load()
    a = dict(N=700, Cin=96, hidden=128, anisotropic=1, **{p: C.c_void_p(0x1000) for p in GEO_PTRS})
    a.update(kw)
    rc = lib.sg_frozen_geometry(a["N"], a["Cin"], a["hidden"], a["anisotropic"], *[a[p] for p in GEO_PTRS], None)
    return rc, lib.sg_last_error().decode()


def _appearance(**kw):
    lib = _lib.load()
    a = dict(N=700, Cin=96, hidden=64, **{p: C.c_void_p(0x1000) for p in APP_PTRS})
    a.update(kw)
    rc = lib.sg_frozen_appearance(a["N"], a["Cin"], a["hidden"], *[a[p] for p in APP_PTRS], None)
    return rc, lib.sg_last_error().decode()


@pytest.mark.parametrize("call, who", [(_geometry, "sg_frozen_geometry"), (_appearance, "sg_frozen_appearance")])
@pytest.mark.parametrize("kw, text", [
    (dict(N=0), "N = 0, at least one point is needed"),
    (dict(N=-5), "N = -5, at least one point is needed"),
    (dict(Cin=132), "Cin = 132 is not a multiple of 4 in 4..128"),
    (dict(Cin=6), "Cin = 6 is not a multiple of 4 in 4..128"),
    (dict(Cin=0), "Cin = 0 is not a multiple of 4 in 4..128"),
    (dict(hidden=132), "hidden = 132 is neither 64 nor 128"),
    (dict(hidden=6), "hidden = 6 is neither 64 nor 128"),
    (dict(hidden=96), "hidden = 96 is neither 64 nor 128"),
    (dict(W_net0=None), "W_net0 is a null pointer"),
    (dict(W_net2=None), "W_net2 is a null pointer"),
    (dict(b_net0=None), "b_net0 is a null pointer"),
    (dict(feats=None), "feats is a null pointer"),
    (dict(W_net2=C.c_void_p(0x1004)), "W_net2 is not 16-byte aligned"),
])
def test_bad_arguments_are_refused_before_any_launch(call, who, kw, text):
    rc, err = call(**kw)
    assert rc == 1 and err == f"{who}: {text}: invalid argument", err


@pytest.mark.parametrize("call, kw, text", [
    (_geometry, dict(W_scales0=None), "sg_frozen_geometry: W_scales0 is a null pointer"),
    (_geometry, dict(W_xyz=None), "sg_frozen_geometry: W_xyz is a null pointer"),
    (_geometry, dict(scales_aux=None), "sg_frozen_geometry: scales_aux is a null pointer"),
    (_geometry, dict(W_rot=None), "sg_frozen_geometry: W_rot is a null pointer"),                 # (anisotropic: required)
    (_geometry, dict(rotations=None), "sg_frozen_geometry: rotations is a null pointer"),
    (_appearance, dict(W_shs=None), "sg_frozen_appearance: W_shs is a null pointer"),
    (_appearance, dict(shs=None), "sg_frozen_appearance: shs is a null pointer"),
    (_appearance, dict(opacity=None), "sg_frozen_appearance: opacity is a null pointer"),           # (an opacity head: required)
    (_appearance, dict(b_shs=C.c_void_p(0x1008)), "sg_frozen_appearance: b_shs is not 16-byte aligned"),
])
def test_each_decoders_own_pointers_are_checked(call, kw, text):
    rc, err = call(**kw)
    assert rc == 1 and err == f"{text}: invalid argument", err


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
def _reference_flags(t_iter, opt_geo_from, opt_geo_until, opt_app_from, opt_app_until):
    """gs_trainer.py:225-226, as written there."""
    opt_geo = False if t_iter < opt_geo_from and t_iter < opt_geo_until else True
    opt_app = False if t_iter < opt_app_from and t_iter < opt_app_until else True
    return opt_geo, opt_app


@pytest.mark.parametrize("args", [
    (1000, 14000, 1000, 15000),          # every shipped configuration (config.py:148-151)
    (5000, 2000, 1000, 15000),           # from > until: the decoder thaws at `until`
    (0, 14000, 0, 15000),                # from = 0: never frozen
    (300, 14000, 7000, 9000),            # geometry and appearance differ
    (9000, 100, 100, 9000),
])
def test_the_schedule_is_the_references_expression(args):
    from sings_amd.train_loop import DecoderSchedule
    s = DecoderSchedule(*args)
    for t in range(16001):
        assert s.flags(t) == _reference_flags(t, *args), t
    f = s.flags(16000)
    assert f == (True, True) and all(type(x) is bool for x in f)         # `until` never freezes anything again


def test_the_shipped_defaults_and_the_trainers_new_parameter():
    from sings_amd.train_loop import AvatarTrainer, DecoderSchedule
    s = DecoderSchedule()
    assert (s.opt_geo_from, s.opt_geo_until, s.opt_app_from, s.opt_app_until) == (1000, 14000, 1000, 15000)
    assert s.flags(0) == s.flags(999) == (False, False) and s.flags(1000) == (True, True)
    sig = inspect.signature(AvatarTrainer.__init__)
    assert sig.parameters["decoder_schedule"].default is None
    from sings_amd.decode import decode_attributes
    sig = inspect.signature(decode_attributes)
    assert sig.parameters["opt_geo"].default is True and sig.parameters["opt_app"].default is True


# ---- the chunk table of an active subset -------------------------------------------------------------------------------------------
def test_the_chunk_table_lists_the_active_parameters_at_their_full_layout_offsets():
    from sings_amd.optim import build_tables
    chunk = 4096
    #         group 0            group 1             group 2        group 3
    numels = [3 * 4000, 5000, 3 * 4096, 4096, 1, 128 * 64, 128, 9000, 7]
    groups = [0, 1, 1, 1, 1, 2, 2, 3, 3]
    addresses = [0x10000 * (i + 1) for i in range(len(numels))]
    offsets = np.concatenate([[0], np.cumsum(numels)[:-1]])
    full_seg, full_chunks = build_tables(addresses, numels, groups, chunk=chunk)
    assert np.array_equal(full_seg[:, 1], offsets) and np.array_equal(full_seg[:, 3], groups)
    assert len(full_chunks) == sum(-(-n // chunk) for n in numels)
    assert np.array_equal(build_tables(addresses, numels, groups, chunk=chunk, active_groups={0, 1, 2, 3})[1], full_chunks)
    for active in ({0}, {0, 1, 3}):                                      # groups 1-3 frozen; group 2 alone
        seg, chunks = build_tables(addresses, numels, groups, chunk=chunk, active_groups=active)
        assert np.array_equal(seg, full_seg)                              # addresses, arena / moment offsets, sizes, groups: the full layout
        want = [(s, first) for s, (n, g) in enumerate(zip(numels, groups)) if g in active for first in range(0, n, chunk)]
        assert chunks.dtype == np.int32 and [tuple(r) for r in chunks.tolist()] == want
        # every element of an active parameter in exactly one chunk, none of a frozen one in any
        covered = np.zeros(sum(numels), np.int32)
        for s, first in chunks.tolist():
            covered[seg[s, 1] + first:seg[s, 1] + min(first + chunk, seg[s, 2])] += 1
        for s, (n, g) in enumerate(zip(numels, groups)):
            assert (covered[offsets[s]:offsets[s] + n] == (1 if g in active else 0)).all(), s
