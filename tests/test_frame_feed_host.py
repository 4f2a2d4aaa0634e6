"""Host tests of the frame feed (include/sings_feed.h, ``_lib._PROTOTYPES_FEED``, sings_amd/frame_feed.py): the seventh header is held
to its table, the refusals come before any HIP call with their exact text, and the numpy twins -- the rule the kernels are compared
with integer for integer in tests/test_gpu_frame_feed.py -- give permutations that are pure functions of (F, seed, epoch), spread
evenly, and the pinned values computed from the rule as include/sings_feed.h states it.

The census (F = 4, seed 12345, epochs 0..23999), measured on the CPU: all 24 permutations, each 954 to 1066 times.  The bound below,
850..1150, is 4.8 sigma of binomial(24000, 1/24) (mean 1000, sigma 31), not these figures."""
import collections
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from sings_amd import _lib
from sings_amd import frame_feed as ff


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_feed.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_FEED) and len(protos) == 2
    others = (set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL) | set(_lib._PROTOTYPES_MESH_TERMS) | set(_lib._PROTOTYPES_ORDER)
              | set(_lib._PROTOTYPES_SAMPLER) | set(_lib._PROTOTYPES_FROZEN))
    assert not set(_lib._PROTOTYPES_FEED) & others
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
    assert _lib.HAS_FEED
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
    text = open(os.path.join(repo_root, "include", "sings_feed.h")).read()
    for name in ("MAX_FRAMES", "MAX_K", "STATE_WORDS"):
        m = re.search(r"#define SG_FEED_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "FEED_" + name), name
    assert (_lib.FEED_MAX_FRAMES, _lib.FEED_MAX_K, _lib.FEED_STATE_WORDS) == (16384, 16, 4)
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES) and _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    for other in ("sings_hip.h", "sings_eval.h", "sings_mesh_terms.h", "sings_order.h", "sings_sampler.h", "sings_frozen.h"):
        assert "sg_frame_" not in open(os.path.join(repo_root, "include", other)).read(), other


# ---- refusals: plausible pointers that are never dereferenced ---------------------------------------------------------------------
def _draw(**kw):
    lib = _lib.load()
    f = C.c_void_p(0x1000)
    a = dict(F=300, K=4, draw_bg=1, state=f, order=f, idx_out=f, bg_out=f)
    a.update(kw)
    rc = lib.sg_frame_draw(a["F"], a["K"], a["draw_bg"], a["state"], a["order"], a["idx_out"], a["bg_out"], None)
    return rc, lib.sg_last_error().decode()


def _expand(**kw):
    lib = _lib.load()
    f = C.c_void_p(0x1000)
    a = dict(K=4, H=48, W=64, F=300, store=f, idx=f, gt=f, mask=f)
    a.update(kw)
    rc = lib.sg_frame_expand(a["K"], a["H"], a["W"], a["F"], a["store"], a["idx"], a["gt"], a["mask"], None)
    return rc, lib.sg_last_error().decode()


@pytest.mark.parametrize("kw, text", [
    (dict(F=0), "F = 0 outside 1..16384"),
    (dict(F=-2), "F = -2 outside 1..16384"),
    (dict(F=16385), "F = 16385 outside 1..16384"),
    (dict(K=0), "K = 0 outside 1..16"),
    (dict(K=17), "K = 17 outside 1..16"),
    (dict(state=None), "null pointer"), (dict(order=None), "null pointer"), (dict(idx_out=None), "null pointer"),
    (dict(bg_out=None), "draw_bg without bg_out"),
    (dict(state=None, order=None, idx_out=None, bg_out=None), "null pointer"),
])
def test_draw_refuses_bad_arguments_before_any_launch(kw, text):
    rc, err = _draw(**kw)
    assert rc == 1 and err == f"sg_frame_draw: {text}: invalid argument", err


@pytest.mark.parametrize("kw, text", [
    (dict(K=0), "K = 0 outside 1..16"),
    (dict(K=17), "K = 17 outside 1..16"),
    (dict(H=0), "a 0 x 64 image has no pixel"),
    (dict(W=-1), "a 48 x -1 image has no pixel"),
    (dict(H=65536, W=32768), "a 65536 x 32768 image has 2^31 pixels or more"),
    (dict(F=0), "F = 0, at least one frame is needed"),
    (dict(store=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(gt=None), "null pointer"),
    (dict(mask=None), "null pointer"),
    (dict(store=None, idx=None, gt=None, mask=None), "null pointer"),
])
def test_expand_refuses_bad_arguments_before_any_launch(kw, text):
    rc, err = _expand(**kw)
    assert rc == 1 and err == f"sg_frame_expand: {text}: invalid argument", err


# ---- the twins -------------------------------------------------------------------------------------------------------------------
def test_a_byte_becomes_the_references_float():
    table = ff.value_table()
    assert table.dtype == np.float32 and table.shape == (256,)
    assert np.array_equal(table.view(np.int32), (np.arange(256) / 255).astype(np.float32).view(np.int32))
    # (what the header warns against: a multiplication by the rounded reciprocal is another table)
    assert int((table != np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)).sum()) == 126


@pytest.mark.parametrize("F", [1, 2, 3, 7, 300, 16384])
def test_the_order_is_a_permutation_and_a_pure_function(F):
    a = ff.order_host(F, 7, 3)
    assert a.dtype == np.int32 and a.shape == (F,) and np.array_equal(np.sort(a), np.arange(F))
    assert np.array_equal(a, ff.order_host(F, 7, 3))
    if F >= 7:                                                           # (F! orders: small F repeats by chance)
        assert not np.array_equal(a, ff.order_host(F, 7, 4)) and not np.array_equal(a, ff.order_host(F, 8, 3))


def test_pinned_orders():
    assert ff.order_host(1, 0, 0).tolist() == [0]
    assert ff.order_host(2, 0, 0).tolist() == [1, 0]
    assert ff.order_host(2, 0, 1).tolist() == [0, 1]
    assert ff.order_host(5, 9, 0).tolist() == [0, 1, 3, 2, 4]
    assert ff.order_host(5, 9, 1).tolist() == [3, 0, 4, 1, 2]
    for F in (0, 16385):
        with pytest.raises(ValueError):
            ff.order_host(F, 0, 0)


def test_the_orders_of_four_frames_are_uniform():
    census = collections.Counter(tuple(ff.order_host(4, 12345, e).tolist()) for e in range(24000))
    print("permutations", len(census), "counts", min(census.values()), "..", max(census.values()))
    assert len(census) == 24
    assert all(850 <= n <= 1150 for n in census.values()), census


def test_the_background_is_24_bits_in_the_unit_interval():
    for seed, counter in ((0, 0), (9, 0), (9, 1), (2 ** 63 + 5, 2 ** 40 + 3)):
        bg = ff.bg_host(seed, counter)
        assert bg.dtype == np.float32 and bg.shape == (3,) and (bg >= 0).all() and (bg < 1).all()
        scaled = bg.astype(np.float64) * 2.0 ** 24
        assert np.array_equal(scaled, np.floor(scaled))
    assert float(ff.bg_host(9, 0)[0]) == 0.634746789932251
    assert not np.array_equal(ff.bg_host(9, 0), ff.bg_host(9, 1)) and not np.array_equal(ff.bg_host(9, 0), ff.bg_host(10, 0))


def test_draws_across_an_epoch_boundary_are_the_concatenated_orders():
    F, seed = 5, 9
    both = np.concatenate([ff.order_host(F, seed, 0), ff.order_host(F, seed, 1), ff.order_host(F, seed, 2)])
    assert np.array_equal(ff.indices_host(F, seed, 3, 6), both[3:9])
    assert np.array_equal(ff.indices_host(F, seed, 0, 15), both)
    assert ff.indices_host(F, seed, 3, 6).dtype == np.int32
    assert ff.indices_host(1, seed, 7, 4).tolist() == [0, 0, 0, 0]


# ---- the Python objects, where no GPU is needed ------------------------------------------------------------------------------------
def test_the_trainers_new_parameter_and_method():
    from sings_amd.train_loop import AvatarTrainer
    sig = inspect.signature(AvatarTrainer.__init__)
    assert sig.parameters["frames"].default is None and list(sig.parameters)[-1] == "frames"
    assert callable(AvatarTrainer.step_next)


def test_the_store_lives_on_the_gpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ff.FrameStore(np.zeros((1, 2, 2, 3), np.uint8), np.zeros((1, 2, 2), np.uint8), device="cpu")
