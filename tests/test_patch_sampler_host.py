"""Host tests of the device patch sampler (include/sings_sampler.h, ``_lib._PROTOTYPES_SAMPLER``, sings_amd/patch_sampler.py): the
fifth header is held to its table, the refusals go through it before any HIP call, and ``origins_host`` -- the numpy rule the kernels
are compared with integer for integer in tests/test_gpu_patch_sampler.py -- has Random123's Philox, draws distinct valid pixels
inside the image, follows the branch rules and spreads its choices evenly.

The census (48 x 64 mask of eight valid pixels, P = 16, n = 4, ratio_mask 0.9, seed 1234, counters 0..1999), measured on the CPU:
the masked branch 1 801 times of 2 000, each pixel chosen 863 to 940 times.  The bounds below are 5 sigma of the binomial
distributions the rule promises, not these figures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sings_amd import _lib
from sings_amd import patch_sampler as ps

CENSUS_PIXELS = ((8, 8), (8, 55), (39, 8), (39, 55), (20, 30), (21, 30), (20, 31), (30, 40))


def census_mask():
    """48 x 64, valid at the four corners of the crop (P = 16) and at an interior cluster."""
    m = np.zeros((48, 64), np.float32)
    for r, c in CENSUS_PIXELS:
        m[r, c] = 1.0
    return m


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_sampler.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_SAMPLER) and len(protos) == 2
    others = set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL) | set(_lib._PROTOTYPES_MESH_TERMS) | set(_lib._PROTOTYPES_ORDER)
    assert not set(_lib._PROTOTYPES_SAMPLER) & others
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
    assert _lib.HAS_SAMPLER
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
    text = open(os.path.join(repo_root, "include", "sings_sampler.h")).read()
    for name in ("MAX_N", "CHUNK", "STATE_WORDS", "BRANCH_MASKED", "BRANCH_UNIFORM", "BRANCH_FORCED"):
        m = re.search(r"#define SG_PATCH_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "PATCH_" + name), name
    assert (_lib.PATCH_MAX_N, _lib.PATCH_CHUNK) == (16, 4096)
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES) and _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    for other in ("sings_hip.h", "sings_eval.h", "sings_mesh_terms.h", "sings_order.h"):
        assert "sg_patch" not in open(os.path.join(repo_root, "include", other)).read(), other


def _call(**kw):
    """One call with plausible arguments (pointers that are never dereferenced), ``kw`` replacing some."""
    lib = _lib.load()
    f = C.c_void_p(0x1000)
    a = dict(K=2, H=48, W=64, P=16, n=4, mask_stride=48 * 64, ratio=0.9, mask=f, state=f, ws=f, origins=f, info=f)
    a.update(kw)
    rc = lib.sg_patch_origins(a["K"], a["H"], a["W"], a["P"], a["n"], a["mask_stride"], a["ratio"], a["mask"], a["state"], a["ws"],
                              a["origins"], a["info"], None)
    return rc, lib.sg_last_error().decode()


@pytest.mark.parametrize("kw, text", [
    (dict(K=0), "K = 0 outside 1..65535"),
    (dict(K=-3), "K = -3 outside 1..65535"),
    (dict(n=0), "n = 0 outside 1..16"),
    (dict(n=17), "n = 17 outside 1..16"),
    (dict(P=15), "patch size 15 must be even and at least 2"),
    (dict(P=0), "patch size 0 must be even and at least 2"),
    (dict(H=16), "a 16 x 64 image has no room for a patch of 16"),
    (dict(W=10), "a 48 x 10 image has no room for a patch of 16"),
    (dict(mask_stride=48 * 64 - 1), "mask_stride 3071 is neither 0 nor H*W = 3072"),
    (dict(mask_stride=-1), "mask_stride -1 is neither 0 nor H*W = 3072"),
    (dict(mask=None), "null pointer"), (dict(state=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(origins=None), "null pointer"), (dict(info=None), "null pointer"),
])
def test_bad_arguments_are_refused_before_any_launch(kw, text):
    rc, err = _call(**kw)
    assert rc == 1 and err == f"sg_patch_origins: {text}: invalid argument", err


def test_the_workspace_is_one_word_per_chunk_and_frame():
    ws = _lib.load().sg_patch_sampler_ws_bytes
    assert ws(1, 48, 64, 16) == 4 and ws(3, 96, 112, 16) == 3 * 2 * 4
    assert ws(1, 80, 80, 16) == 4 and ws(1, 80, 81, 16) == 8              # 4 096 positions: one chunk; 4 160: two
    assert ws(2, 500, 890, 128) == 2 * 4 * -(-372 * 762 // 4096)
    assert ws(0, 48, 64, 16) == 0 and ws(1, 16, 64, 16) == 0 and ws(1, 48, 64, 15) == 0


# ---- the twin --------------------------------------------------------------------------------------------------------------------
def test_the_twins_philox_gives_the_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert ps.philox4x32(ctr, key) == out


def test_the_threshold_is_the_fp32_ratio_times_two_to_the_32():
    assert ps.threshold(1.0) == 1 << 32 and ps.threshold(0.0) == 0 and ps.threshold(0.5) == 1 << 31
    assert ps.threshold(0.9) == int(float(np.float32(0.9)) * 2.0 ** 32) == 3865470464
    assert ps.threshold(2.0) == 1 << 32 and ps.threshold(-1.0) == 0 and ps.threshold(float("nan")) == 0


def test_masked_corners_are_distinct_valid_and_inside_over_200_counters():
    rng = np.random.default_rng(5)
    H, W, P, n = 70, 53, 16, 4
    mask = (rng.random((H, W)) < 0.3).astype(np.float32)
    o, masked = P // 2, 0
    for counter in range(200):
        org, branch, M = ps.origins_host(mask, P, n, 0.9, 77, counter)
        assert org.dtype == np.int32 and org.shape == (n, 2) and M == int((mask[o:H - o, o:W - o] > 0).sum())
        assert (org >= 0).all() and (org[:, 0] < H - P).all() and (org[:, 1] < W - P).all()
        if branch == ps.BRANCH_MASKED:
            masked += 1
            assert len({tuple(c) for c in org.tolist()}) == n
            assert (mask[org[:, 0] + o, org[:, 1] + o] > 0).all()
        else:
            assert branch == ps.BRANCH_UNIFORM
    assert 150 <= masked < 200                                            # (180 +- 5 sigma of binomial(200, 0.9) = 21)
    # a pure function: the same arguments, the same corners; another frame or seed, another draw
    a = ps.origins_host(mask, P, n, 0.9, 77, 3)[0]
    assert np.array_equal(a, ps.origins_host(mask.copy(), P, n, 0.9, 77, 3)[0])
    assert not np.array_equal(a, ps.origins_host(mask, P, n, 0.9, 77, 3, frame=1)[0])
    assert not np.array_equal(a, ps.origins_host(mask, P, n, 0.9, 78, 3)[0])


def test_the_branch_rules():
    mask, n, P = census_mask(), 4, 16
    b1 = [ps.origins_host(mask, P, n, 1.0, 9, c)[1] for c in range(300)]
    b0 = [ps.origins_host(mask, P, n, 0.0, 9, c)[1] for c in range(300)]
    assert set(b1) == {ps.BRANCH_MASKED} and set(b0) == {ps.BRANCH_UNIFORM}
    few = np.zeros_like(mask)
    for r, c in CENSUS_PIXELS[:n - 1]:
        few[r, c] = 1.0
    org, branch, M = ps.origins_host(few, P, n, 1.0, 9, 0)                # M = n - 1: the reference raises, the rule counts
    assert (branch, M) == (ps.BRANCH_FORCED, n - 1)
    assert (org[:, 0] < 48 - P).all() and (org[:, 1] < 64 - P).all() and (org >= 0).all()
    assert ps.origins_host(few, P, n, 0.0, 9, 0)[1] == ps.BRANCH_UNIFORM  # (the draw comes first: nothing would have raised)
    few[CENSUS_PIXELS[n - 1]] = 1.0                                       # M = n: every valid position, each once
    for c in range(20):
        org, branch, M = ps.origins_host(few, P, n, 1.0, 9, c)
        assert (branch, M) == (ps.BRANCH_MASKED, n)
        assert sorted(map(tuple, (org + P // 2).tolist())) == sorted(CENSUS_PIXELS[:n])
    # NaN and negatives are not valid; the margin outside the crop does not count
    odd = census_mask()
    odd[10, 10], odd[11, 11], odd[3, 30], odd[45, 30], odd[20, 4], odd[20, 60] = np.nan, -1.0, 1.0, 1.0, 1.0, 1.0
    assert ps.origins_host(odd, P, n, 1.0, 9, 0)[2] == 8
    with pytest.raises(ValueError):
        ps.origins_host(mask, 15, n, 1.0, 9, 0)
    with pytest.raises(ValueError):
        ps.origins_host(mask, P, 17, 1.0, 9, 0)


def test_the_census_meets_the_binomial_bounds():
    mask, P, n = census_mask(), 16, 4
    masked, hits = 0, {p: 0 for p in CENSUS_PIXELS}
    for counter in range(2000):
        org, branch, M = ps.origins_host(mask, P, n, 0.9, 1234, counter)
        assert M == 8
        if branch == ps.BRANCH_MASKED:
            masked += 1
            for r, c in (org + P // 2).tolist():
                hits[(r, c)] += 1
    print("masked branch", masked, "of 2000; per pixel", sorted(hits.values()))
    assert abs(masked - 1800) <= 67                                       # 5 sigma of binomial(2000, 0.9)
    assert all(abs(h - 900.5) <= 106 for h in hits.values()), hits        # 5 sigma of binomial(1801, 1/2)
    assert sum(hits.values()) == n * masked


# ---- the Python object, where no GPU is needed -----------------------------------------------------------------------------------
def test_the_constructor_refuses_what_the_host_sampler_refuses():
    from sings_amd.lpips import PatchSampler
    with pytest.raises(ValueError, match="patch size has to be even"):
        ps.DevicePatchSampler(patch_size=21)
    with pytest.raises(NotImplementedError) as e:
        ps.DevicePatchSampler(dilate=1)
    with pytest.raises(NotImplementedError) as h:
        PatchSampler(dilate=1)
    assert str(e.value) == str(h.value)
    with pytest.raises(ValueError, match="num_patch"):
        ps.DevicePatchSampler(num_patch=17)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ps.DevicePatchSampler(device="cpu")
