"""The work order of a K-camera launch (include/sings_order.h, sings_amd/work_order.py): lane i of the kernel that expands and counts
the (tile, Gaussian) pairs works on Gaussian order[i]; a workgroup whose tile window has at most SG_ORDER_WINDOW_TILES tiles counts
its pairs in LDS.  Whatever the order, every output carries the bits of the unordered launch (``order=False``).

All on the ragged 1034 x 1030 frame of tests/test_gpu_bwd_tile_wave.py: 65 x 65 tiles, 4 624 counter words -- the many-tile regime
-- at degree 3 with the short-list hint on, so the frames are binned directly.  P = 3037 is no multiple of 256 or 64.
tests/test_work_order_host.py asserts from the oracle's rectangles alone that the crafted scenes have the windows assumed here.

(The depth / alpha maps have no K-camera entry points on the plain path, so there is no ordered twin of them to test.)"""
import numpy as np
import pytest
import torch

import test_gpu_bwd_tile_wave as tw
from oracle import raster_oracle as ro
from sings_amd import _lib
from sings_amd.scene import synthetic_scene

pytestmark = pytest.mark.gpu

W, H, GX, GY, BORDER = tw.W, tw.H, tw.GX, tw.GY, tw.BORDER
FX = 1.2 * W
P = 3037
WMAX = _lib.ORDER_WINDOW_TILES
BLOCK = _lib.ORDER_BLOCK


# ---- scenes (numpy only: the host test reads them too) ---------------------------------------------------------------------------
def _splat(px, py, z, sigma_px, opacity):
    """An isotropic Gaussian whose centre projects to pixel (px, py) of the identity-view camera."""
    return [(px + 0.5 - W / 2) / FX * z, (py + 0.5 - H / 2) / FX * z, z], [sigma_px * z / FX] * 3, [1.0, 0.0, 0.0, 0.0], opacity


def _dot(tx, ty, z, opacity=0.4, dx=8, dy=8):
    """A splat of radius 3 pixels around local pixel (dx, dy) of tile (tx, ty): its rectangle is that tile alone (dx, dy in 4..11)."""
    return _splat(16 * tx + dx, 16 * ty + dy, z, 0.5, opacity)


def _culled():
    """Behind the camera: no radius, no pairs."""
    return [0.0, 0.0, -1.0], [0.01] * 3, [1.0, 0.0, 0.0, 0.0], 0.5


def _scene(splats, seed):
    k = len(splats)
    rs = np.random.RandomState(seed)
    s = synthetic_scene(1, W, H, 3, 9)                                  # the camera, the background and dL/dimage
    s["N"] = k
    s["means3D"] = np.array([m for m, _, _, _ in splats], np.float32)
    s["scales"] = np.array([c for _, c, _, _ in splats], np.float32)
    s["rotations"] = np.array([r for _, _, r, _ in splats], np.float32)
    s["opacities"] = np.array([[o] for _, _, _, o in splats], np.float32)
    s["shs"] = np.concatenate([rs.normal(0, 1, (k, 1, 3)), rs.normal(0, 0.15, (k, 15, 3))], 1).astype(np.float32)
    return s


CRAFTED_P = 700                                                         # blocks of 256, 256 and 188 positions (identity order)
COMPACT = (20, 30, 6, 5)                                                # block 0: tiles x 20..25, y 30..34 -- a window of 30 tiles


def crafted_scene():
    """Block 0 is compact; block 1 is compact but for ONE splat that covers every tile (the per-pair path); block 2 sits on the
    ragged right column and bottom row of tiles (10 of 16 pixel columns, 6 of 16 pixel rows inside the image)."""
    rs = np.random.RandomState(3)
    splats = []
    x0, y0, w, h = COMPACT
    for i in range(BLOCK):                                              # block 0
        splats.append(_splat(16 * x0 + rs.uniform(8, 16 * w - 8), 16 * y0 + rs.uniform(8, 16 * h - 8), 2.0 + 1e-3 * i,
                             rs.uniform(0.5, 1.5), rs.uniform(0.1, 0.6)))
    for i in range(BLOCK):                                              # block 1
        if i == 100:
            splats.append(_splat(W / 2, H / 2, 1.5, 400.0, 0.05))
        else:
            splats.append(_splat(16 * 40 + rs.uniform(8, 72), 16 * 8 + rs.uniform(8, 72), 3.0 + 1e-3 * i, rs.uniform(0.5, 1.5),
                                 rs.uniform(0.1, 0.6)))
    for i in range(CRAFTED_P - 2 * BLOCK):                              # block 2
        if i % 2:
            splats.append(_splat(W - 1 - rs.uniform(0, 9), 16 * 58 + rs.uniform(0, H - 16 * 58 - 1), 2.5 + 1e-3 * i, rs.uniform(0.5, 2.0), 0.4))
        else:
            splats.append(_splat(16 * 58 + rs.uniform(0, W - 16 * 58 - 1), H - 1 - rs.uniform(0, 5), 2.5 + 1e-3 * i, rs.uniform(0.5, 2.0), 0.4))
    return _scene(splats, 31)


WINDOW_CORNERS = {WMAX: ((2, 2), (33, 49)), WMAX + 1: ((2, 2), (30, 54))}     # 32 x 48 = 1536 tiles, 29 x 53 = 1537 tiles


def window_scene(tiles):
    """One block whose window has exactly ``tiles`` tiles: two one-tile splats at opposite corners, 98 more inside, the rest of
    the 256 culled; then a second, compact block."""
    (ax, ay), (bx, by) = WINDOW_CORNERS[tiles]
    rs = np.random.RandomState(tiles)
    splats = [_culled() for _ in range(BLOCK)]
    splats[7] = _dot(ax, ay, 2.0)
    splats[201] = _dot(bx, by, 2.1)
    for i in range(98):
        splats[20 + i] = _dot(rs.randint(ax, bx + 1), rs.randint(ay, by + 1), 2.2 + 1e-3 * i, 0.3, rs.randint(4, 12), rs.randint(4, 12))
    for i in range(150):
        splats.append(_splat(16 * 5 + rs.uniform(8, 56), 16 * 58 + rs.uniform(8, 56), 3.0 + 1e-3 * i, rs.uniform(0.5, 1.5), 0.3))
    return _scene(splats, 37)


def pile_scene():
    """Every Gaussian in tile (10, 10): 3 037 pairs in one row of 1 024 keys, from twelve workgroups (each a window of one tile)."""
    rs = np.random.RandomState(8)
    return _scene([_dot(10, 10, 2.0 + 1e-4 * i, 0.05, rs.randint(4, 12), rs.randint(4, 12)) for i in range(P)], 41)


def cloud_scene():
    return synthetic_scene(P, W, H, 3, 5)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cameras(s, K, dev, same=False):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], K, 0).copy()
    if not same:
        views[:, 3, 0] = 0.02 * np.arange(K); views[:, 3, 1] = -0.01 * np.arange(K)
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=_t(s["bg"], dev),
                                         scale_modifier=1.0, viewmatrix=_t(views, dev), projmatrix=_t(projs, dev), sh_degree=3,
                                         campos=_t(cps, dev), prefiltered=False, debug=False)


def _engine(s, K, dev, order, cap=None, same=False):
    from sings_amd.engine import RasterFramesEngine
    n = s["means3D"].shape[0]
    e = RasterFramesEngine(n, W, H, 16, K, dev, cap if cap is not None else 8 * n + 8192, order=order)
    e.set_camera(_cameras(s, K, dev, same), short_lists=True)
    return e


def _ins(s, dev):
    return [_t(s[k], dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")]


def _dL(K, dev):
    return _t(np.random.RandomState(1).normal(0, 1, (K, 3, H, W)).astype(np.float32), dev)


def _run(e, ins, dL, accumulate=False):
    """One forward + backward -> everything a caller sees, cloned: the frames, radii, pair counts, per frame the ranges and the
    sorted lists, the gradient buffer (the five gradient arrays) and the per-frame dL/dmeans2D."""
    if accumulate:
        e.grad_flat.copy_(torch.linspace(-1.0, 1.0, e.grad_flat.numel(), device=e.grad_flat.device))
    else:
        e.grad_flat.fill_(float("nan"))
    nr = e.forward(*ins, sync_num_rendered=True)
    e.backward(*ins, dL, accumulate=accumulate)
    torch.cuda.synchronize()
    T = GX * GY
    out = dict(color=e.color.clone(), radii=e.radii.clone(), grad=e.grad_flat.clone(), m2d=e.d_means2D.clone(), nr=nr)
    b = e.binning.view(e.K, e.L.bin_bytes)
    for f in range(e.K):
        rg = b[f, e.L.bin_ranges:e.L.bin_ranges + 8 * T].view(torch.int32).view(-1, 2).clone()
        ok = 0 <= nr[f] <= e.cap                                        # (a refused frame has no lists)
        R = max(int(rg[:, 1].max()), 0) if ok else 0
        out[f"ranges{f}"] = rg if ok else None
        out[f"list{f}"] = b[f, e.L.bin_point_list:e.L.bin_point_list + 4 * min(R, e.cap)].view(torch.int32).clone()
    return out


def _same(a, b, what):
    assert a["nr"] == b["nr"], (what, a["nr"], b["nr"])
    for k in a:
        if k == "nr" or a[k] is None:
            continue
        assert torch.equal(a[k], b[k]), (what, k)


def _orders(n, dev):
    ident = torch.arange(n, dtype=torch.int32, device=dev)
    return {"identity": ident, "reversed": ident.flip(0).contiguous(),
            "random": _t(np.random.RandomState(12).permutation(n).astype(np.int32), dev), "morton": None}


_REF = {}


def _reference(K, dev):
    """The unordered launch of the cloud at K cameras, plain and accumulating: computed once."""
    if K not in _REF:
        s = cloud_scene()
        e = _engine(s, K, dev, False)
        ins, dL = _ins(s, dev), _dL(K, dev)
        _REF[K] = (s, ins, dL, _run(e, ins, dL), _run(e, ins, dL, accumulate=True))
    return _REF[K]


# ---- 1. any order, the same bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("name", ["identity", "reversed", "random", "morton"])
def test_every_order_leaves_the_bits_of_the_unordered_launch(K, name):
    dev = tw._dev()
    s, ins, dL, ref, ref_acc = _reference(K, dev)
    assert all(r > 2 * P for r in ref["nr"]) and bool(torch.isfinite(ref["grad"]).all()) and bool((ref["grad"] != 0).any())
    e = _engine(s, K, dev, _orders(P, dev)[name])
    _same(_run(e, ins, dL), ref, name)
    _same(_run(e, ins, dL, accumulate=True), ref_acc, name + " (accumulate)")
    if name == "morton":
        from sings_amd.work_order import order_host
        assert e._order is not None and np.array_equal(e._order.cpu().numpy(), order_host(s["means3D"]))


def test_one_workspace_serves_calls_that_alternate_orders():
    """The counters' zero invariant: every forward leaves the tile counters zeroed for the next one, whichever path counted."""
    dev = tw._dev()
    K = 2
    s, ins, dL, ref, _ = _reference(K, dev)
    e = _engine(s, K, dev, False)
    od = _orders(P, dev)
    for name in ("morton", "random", "identity", "reversed", "morton"):
        e.set_order(od[name])
        _same(_run(e, ins, dL), ref, name)
        e.set_order(False)
        _same(_run(e, ins, dL), ref, "unordered after " + name)


def test_the_engine_refuses_a_bad_order_and_never_dereferences_an_entry_out_of_range():
    dev = tw._dev()
    s = cloud_scene()
    with pytest.raises(ValueError, match="order has"):
        _engine(s, 2, dev, torch.arange(P - 1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="int32"):
        _engine(s, 2, dev, torch.arange(P, dtype=torch.int64, device=dev))
    # an entry >= P is never dereferenced: the call runs (the frame is then another one)
    bad = torch.arange(P, dtype=torch.int32, device=dev); bad[5] = P + 7; bad[P - 1] = -1
    e = _engine(s, 2, dev, bad)
    ins, dL = _ins(s, dev), _dL(2, dev)
    e.forward(*ins); e.backward(*ins, dL)
    torch.cuda.synchronize()
    lib = _lib.load()
    from sings_amd._marshal import _ptr
    import ctypes as C
    args = (C.byref(e._s), C.byref(e._fb), P, *[_ptr(x) for x in (ins[0], ins[1])], None, *[_ptr(x) for x in ins[2:]], None,
            _ptr(e.geom), _ptr(e.binning), e.cap, _ptr(e.img), _ptr(e.color), _ptr(e.radii), None)
    assert lib.sg_rasterize_forward_frames_ordered(*args, _ptr(bad), P - 1, e._stream()) == 1
    assert "entries" in lib.sg_last_error().decode()


# ---- 2. the crafted cloud ---------------------------------------------------------------------------------------------------------
_CRAFTED = []


def _crafted_oracle():
    if not _CRAFTED:
        s = crafted_scene()
        o = tw._oracle(s)
        dL = s["dL_dimage"].copy(); dL[:, o["margin"] < BORDER] = 0
        _CRAFTED.append((s, o, dL, ro.backward(o, dL)))
    return _CRAFTED[0]


def test_compact_screen_filling_and_ragged_edge_blocks():
    dev = tw._dev()
    s, o, dLn, g = _crafted_oracle()
    K = 2
    ins = _ins(s, dev)
    dL = torch.stack([_t(dLn, dev), torch.zeros(3, H, W, device=dev)])   # one camera twice; the second frame carries no loss
    ident = torch.arange(CRAFTED_P, dtype=torch.int32, device=dev)
    ref = _run(_engine(s, K, dev, False, same=True), ins, dL)
    e = _engine(s, K, dev, ident, same=True)
    got = _run(e, ins, dL)
    _same(got, ref, "crafted")
    assert got["nr"] == [int(o["R"])] * 2
    assert np.array_equal(got["radii"][0].cpu().numpy(), o["radii"])
    strict = o["margin"] >= BORDER
    err = np.abs(got["color"][0].cpu().numpy() - o["color"]).max(0)[strict].max()
    print("image L_inf against the oracle", err)
    assert err <= 1e-5
    for name, a in (("dL_dmeans3D", e.d_means3D), ("dL_dscales", e.d_scales), ("dL_drots", e.d_rots), ("dL_dopacity", e.d_opacity),
                    ("dL_dsh", e.d_sh)):
        tw._grad_close(name, a.cpu().numpy().reshape(g[name].shape), g[name])


# ---- 3. both sides of the window branch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", [WMAX, WMAX + 1])
def test_a_window_of_exactly_the_limit_and_one_tile_more(tiles):
    dev = tw._dev()
    s = window_scene(tiles)
    n = s["means3D"].shape[0]
    ins, dL = _ins(s, dev), _dL(2, dev)
    ref = _run(_engine(s, 2, dev, False), ins, dL)
    got = _run(_engine(s, 2, dev, torch.arange(n, dtype=torch.int32, device=dev)), ins, dL)
    assert ref["nr"][0] >= 250
    _same(got, ref, tiles)


# ---- 4. a list longer than its row ------------------------------------------------------------------------------------------------
def test_a_violated_hint_reads_as_a_long_list_and_the_next_call_is_clean():
    dev = tw._dev()
    K = 2
    pile, (s, ins, dL, ref, _) = pile_scene(), _reference(K, dev)
    pins = _ins(pile, dev)
    bgv = _t(pile["bg"], dev)[None, :, None, None].expand(K, 3, H, W)
    for order in (False, torch.arange(P, dtype=torch.int32, device=dev), None):
        e = _engine(pile, K, dev, order, same=True)
        got = _run(e, pins, dL)
        assert got["nr"] == [_lib.NUM_RENDERED_LONG_LIST] * K, (order is False, got["nr"])
        assert torch.equal(got["color"], bgv) and not bool(got["grad"].any()) and not bool(got["m2d"].any())
        # the same workspace, the cloud with its cameras: nothing stale left behind
        e.set_camera(_cameras(s, K, dev), short_lists=True)
        if order is None:
            e.refresh_order()
        _same(_run(e, ins, dL), ref, "after the long list")


# ---- 5. a pair capacity that is too small -----------------------------------------------------------------------------------------
def test_too_small_a_pair_capacity_overflows_as_the_unordered_launch_does():
    dev = tw._dev()
    K = 2
    s, ins, dL, ref, _ = _reference(K, dev)
    cap = min(ref["nr"]) // 2
    a = _run(_engine(s, K, dev, False, cap=cap), ins, dL)
    b = _run(_engine(s, K, dev, None, cap=cap), ins, dL)
    assert a["nr"] == ref["nr"] and all(r > cap for r in a["nr"])
    _same(b, a, "overflow")
    assert not bool(b["grad"].any())
