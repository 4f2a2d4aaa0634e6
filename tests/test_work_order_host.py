"""Host tests of the work order (include/sings_order.h, ``_lib._PROTOTYPES_ORDER``, sings_amd/work_order.py): the fourth header is
held to its table, the refusals go through it before any HIP call, the numpy twin of the order builder is a stable permutation,
and -- from the oracle's tile rectangles alone -- the crafted scenes of tests/test_gpu_work_order.py have the windows its GPU tests
assume, and the built order does to a copy of the bench scene what the kernels count on.

The census scene: 20 000 Gaussians of the bench's generator on 608 x 342 pixels -- a tenth of the bench's Gaussians on a tenth of
its pixels, so a workgroup's 256 Gaussians meet as many tiles as at 200 000 on 1920 x 1080.  Measured here on the CPU: distinct
(workgroup, tile) pairs 46 116 in input order, 11 208 in the built order (0.243); the bench scene itself: 734 415 -> 200 000 (0.272;
97.6 % of its workgroups have a window of at most 1 536 tiles, 93.2 % of at most 1 024).  The same 20 000 Gaussians spread over
1920 x 1080 are ten times sparser per tile and give 73 497 -> 46 915 (0.638): the count depends on the Gaussians per tile, not on the
order builder (``scene.morton_order`` gives the same three figures)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gpu_work_order as gw
from oracle import raster_oracle as ro
from sings_amd import _lib
from sings_amd import work_order as wo
from sings_amd.scene import synthetic_scene


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_order.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_ORDER)
    assert not set(_lib._PROTOTYPES_ORDER) & (set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL) | set(_lib._PROTOTYPES_MESH_TERMS))
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
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
    text = open(os.path.join(repo_root, "include", "sings_order.h")).read()
    for name in ("WINDOW_TILES", "BLOCK", "CODE_BITS", "WS_BYTES"):
        m = re.search(r"#define SG_ORDER_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "ORDER_" + name), name
    common = open(os.path.join(repo_root, "sings_amd", "csrc", "sg_common.h")).read()
    assert int(re.search(r"#define SG_HIST_TILES_MAX (\d+)", common).group(1)) == _lib.HIST_TILES_MAX
    assert 1024 <= _lib.ORDER_WINDOW_TILES <= 2048
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES) and _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    for other in ("sings_hip.h", "sings_eval.h", "sings_mesh_terms.h"):
        assert "_ordered" not in open(os.path.join(repo_root, "include", other)).read(), other


def _call(**kw):
    """One call of an ordered entry point with plausible arguments (pointers that are never dereferenced), ``kw`` replacing some."""
    lib = _lib.load()
    f = C.c_void_p(0x1000)
    s = _lib.SgRasterSettings(image_height=64, image_width=64, tanfovx=0.5, tanfovy=0.5, scale_modifier=1.0, sh_degree=0, sh_coeffs=1,
                              bg=0x1000, viewmatrix=0x1000, projmatrix=0x1000, campos=0x1000)
    fb = _lib.SgFrameBatch(K=2, camera_stride=0, transl_stride=0, placement=0)
    a = dict(P=8, order=f, order_len=8)
    a.update(kw)
    rc = lib.sg_rasterize_forward_frames_ordered(C.byref(s), C.byref(fb), a["P"], f, f, None, f, f, f, None, f, f, 4096, f, f, f, None,
                                                 a["order"], a["order_len"], None)
    return rc, lib.sg_last_error().decode()


def test_an_order_of_another_length_is_refused_before_any_launch():
    who = "sg_rasterize_forward_frames_ordered"
    for n in (7, 9, 0, -1):
        rc, err = _call(order_len=n)
        assert rc == 1 and err == f"{who}: the order has {n} entries, the call 8 Gaussians: invalid argument", err
    rc, err = _call(order=None, order_len=8)
    assert rc == 1 and err == f"{who}: order_len 8 without an order: invalid argument", err


def test_the_code_builder_refuses_bad_arguments():
    lib = _lib.load()
    f = C.c_void_p(0x1000)
    assert lib.sg_work_order_codes(-1, f, f, f, None) == 1 and "P = -1" in lib.sg_last_error().decode()
    for args in ((4, None, f, f), (4, f, None, f), (4, f, f, None)):
        assert lib.sg_work_order_codes(*args, None) == 1
        assert lib.sg_last_error().decode() == "sg_work_order_codes: null pointer: invalid argument"
    assert lib.sg_work_order_codes(0, None, None, None, None) == 0


# ---- the builder's twin ----------------------------------------------------------------------------------------------------------
def test_the_built_order_is_a_stable_permutation_and_a_pure_function_of_the_positions():
    s = synthetic_scene(gw.P, gw.W, gw.H, 3, 5)
    x = s["means3D"].copy()
    x[100:140] = x[7]                                                # forty Gaussians on one spot: equal codes
    x[2000] = [np.nan, 0.0, 1.0]                                     # a NaN coordinate: cell 0 on that axis, ignored by the box
    a, b = wo.order_host(x), wo.order_host(x.copy())
    assert a.dtype == np.int32 and np.array_equal(a, b)
    assert np.array_equal(np.sort(a), np.arange(gw.P))
    code = wo.morton_codes_host(x)
    assert code.max() < 1 << 30 and (np.diff(code[a].astype(np.int64)) >= 0).all()
    ties = np.nonzero(np.diff(code[a].astype(np.int64)) == 0)[0]
    assert len(ties) >= 39 and (a[ties + 1] > a[ties]).all()         # equal codes: in index order
    pos = np.nonzero(np.isin(a, np.r_[7, 100:140]))[0]
    assert len(pos) == 41 and a[pos].tolist() == [7] + list(range(100, 140))
    # a cloud without extent, and an empty one
    assert np.array_equal(wo.order_host(np.ones((5, 3), np.float32)), np.arange(5))
    assert wo.order_host(np.zeros((0, 3), np.float32)).shape == (0,)


def test_where_an_order_takes_effect():
    assert wo.order_applies(gw.W, gw.H, _lib.FLAG_SHORT_LISTS) and wo.order_applies(1920, 1080, _lib.FLAG_SHORT_LISTS | _lib.FLAG_LONG_ROWS)
    assert not wo.order_applies(gw.W, gw.H, _lib.FLAG_LONG_ROWS)     # no short-list hint: not binned directly
    assert not wo.order_applies(1024, 1024, _lib.FLAG_SHORT_LISTS)   # 4 096 counters: the whole-image histogram
    assert wo.order_applies(1040, 1024, _lib.FLAG_SHORT_LISTS)


def test_the_engine_builds_no_order_inside_a_graph_capture_or_where_none_applies(monkeypatch):
    """On the CPU (nothing launches): the refusal of a build inside a capture; ``order=False``, a caller's tensor and a frame outside
    the direct many-tile regime build nothing."""
    import torch
    from sings_amd import engine as E
    from sings_amd.rasterizer import GaussianRasterizationSettings
    z = torch.zeros
    cam = GaussianRasterizationSettings(image_height=gw.H, image_width=gw.W, tanfovx=0.5, tanfovy=0.5, bg=z(3), scale_modifier=1.0,
                                        viewmatrix=z(4, 4), projmatrix=z(4, 4), sh_degree=0, campos=z(3), prefiltered=False, debug=False)
    built = []
    monkeypatch.setattr(E._work_order, "build_order", lambda m: built.append(1) or torch.arange(m.shape[0], dtype=torch.int32))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    e = E.RasterFramesEngine(40, gw.W, gw.H, 1, 2, "cpu", 4096)
    e.set_camera(cam, short_lists=True)
    with pytest.raises(RuntimeError, match="graph capture"):
        e._order_for(z(40, 3))
    e.set_camera(cam)                                               # no hint: the frame is not binned directly
    assert e._order_for(z(40, 3)) is None
    e.set_camera(cam, short_lists=True)
    e.set_order(False)
    assert e._order_for(z(40, 3)) is None
    mine = torch.arange(40, dtype=torch.int32).flip(0).contiguous()
    e.set_order(mine)
    assert e._order_for(z(40, 3)) is mine and not built
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    e.set_order(None)
    first = e._order_for(z(40, 3))
    assert first is not None and e._order_for(z(40, 3)) is first and built == [1]      # built once, kept
    e.refresh_order()
    assert e._order_for(z(40, 3)) is not first and built == [1, 1]
    with pytest.raises(ValueError, match="order has 39 entries"):
        e.set_order(mine[:39].contiguous())


# ---- the scenes of the GPU tests, from the oracle's rectangles -------------------------------------------------------------------
def _census(s, order=None):
    o = gw.tw._oracle(s)
    r = o["rect"]
    return o, wo.window_census(r[:, :2], r[:, 2:], order)


def test_the_frame_of_the_gpu_tests_is_in_the_many_tile_regime():
    assert (gw.GX, gw.GY) == (65, 65) and ((gw.GX + 3) // 4) * ((gw.GY + 3) // 4) * 16 == 4624 > _lib.HIST_TILES_MAX
    assert gw.P % 64 and gw.P % 256


def test_the_crafted_cloud_has_a_compact_a_screen_filling_and_a_ragged_edge_block():
    s = gw.crafted_scene()
    o, c = _census(s)
    assert s["means3D"].shape[0] == gw.CRAFTED_P and len(c["windows"]) == 3
    assert 20 <= c["windows"][0] <= 30
    assert c["windows"][1] == gw.GX * gw.GY > _lib.ORDER_WINDOW_TILES
    r = o["rect"]
    assert (o["tiles_touched"][256:512] == gw.GX * gw.GY).sum() == 1             # ONE splat covers every tile
    rest = np.delete(r[256:512], 100, 0)
    assert ((rest[:, 2] - rest[:, 0]) * (rest[:, 3] - rest[:, 1])).max() <= 9    # ... inside an otherwise compact block
    b2 = r[512:]
    assert 0 < c["windows"][2] <= _lib.ORDER_WINDOW_TILES
    assert (b2[:, 2] == gw.GX).any() and (b2[:, 3] == gw.GY).any()               # the ragged column and the ragged row of tiles
    assert gw.W % 16 and gw.H % 16
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert tl.max() <= 1024 and o["R"] < 8 * gw.CRAFTED_P + 8192


@pytest.mark.parametrize("tiles", [gw.WMAX, gw.WMAX + 1])
def test_the_window_scenes_have_exactly_their_windows(tiles):
    o, c = _census(gw.window_scene(tiles))
    assert c["windows"].tolist() == [tiles, 16]
    assert (o["tiles_touched"][:256] > 0).sum() == 100 and (o["tiles_touched"][:256] <= 1).all()


def test_the_pile_fills_one_row_from_twelve_workgroups():
    o, c = _census(gw.pile_scene())
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert tl[10 * gw.GX + 10] == gw.P > 1024 and o["R"] == gw.P
    assert c["windows"].tolist() == [1] * 12


def test_the_built_order_more_than_halves_the_workgroup_tile_pairs_of_a_copy_of_the_bench_scene():
    s = synthetic_scene(20000, 608, 342, 3, 3)
    o = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                   s["tanfovy"], s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=3)
    r = o["rect"]
    a = wo.window_census(r[:, :2], r[:, 2:])
    b = wo.window_census(r[:, :2], r[:, 2:], wo.order_host(s["means3D"]))
    print("pairs", a["pairs"], "distinct (workgroup, tile): input order", a["group_tiles"], "built order", b["group_tiles"],
          "ratio", b["group_tiles"] / a["group_tiles"], "windows <= limit", float((b["windows"] <= _lib.ORDER_WINDOW_TILES).mean()))
    assert a["pairs"] == b["pairs"] == int(o["tiles_touched"].sum())
    assert b["group_tiles"] < 0.5 * a["group_tiles"]
