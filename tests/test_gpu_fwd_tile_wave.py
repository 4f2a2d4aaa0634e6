"""The dense forward composite (frames of more than 4 096 tiles, K frames per launch): one wave per tile, four tiles per workgroup,
each lane owning one pixel of each of the tile's four 8x8 quadrants; the wave sorts its tile's keys, stages 64 entries per batch and
walks them through a ballot, the quadrants of an entry's mask under wave-uniform branches (sings_amd/csrc/sg_render_fwd.inc).

Every case runs on a 1034 x 1030 frame: 65 x 65 = 4 225 tiles (the dense kernels' regime, one more than a multiple of four: the last
workgroup has one tile and three waves past the end), the right column of tiles has 10 pixel columns inside the image, the bottom row 6
pixel rows.  The kernel under test is the K-frame one, so every case renders K = 2 frames in one launch (RasterFramesEngine, or the
skinned operator for the depth / alpha maps).  A few thousand Gaussians at most, so the scalar oracle takes a fraction of a second.

Bars: image, final_T and n_contrib against oracle/raster_oracle at the bar of tests/test_gpu_raster.py -- RGB and final_T within 1e-5,
n_contrib equal, off the pixels within 2e-5 of a hard threshold, which may be at most 0.1 % of the frame; binning (ranges, sorted
lists) bit for bit; gradients through the unchanged backward at `_grad_close` (rtol 2e-4 + 2e-6 max|g|): they prove the masks and
checkpoints the forward leaves."""
import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from sings_amd.scene import synthetic_scene

pytestmark = pytest.mark.gpu

W, H = 1034, 1030
GX, GY = (W + 15) // 16, (H + 15) // 16
T = GX * GY
BORDER = 2e-5
RGB_TOL = 1e-5
EXCLUDED_MAX = 1e-3
WAVE_SORT_MAX = 512            # SG_TWSORT_MAX: the longest list one wave sorts; up to 1024 (SG_WSORT_MAX) the workgroup sorts it
HOT = GX + 1                   # tile (1, 1): its workgroup holds tiles 64..67 -- the ragged last tile of row 0 and three ordinary ones
CORNER = T - 1                 # the bottom-right tile, 10 x 6 pixels inside the image, alone in the last workgroup (tiles T.. are past the end)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _oracle(s):
    return ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                      s["tanfovy"], s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=s["sh_degree"])


def _grad_close(name, a, b, rtol=2e-4, atol=2e-6):
    a = a.astype(np.float64); b = b.astype(np.float64)
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b)
    bad = err > rtol * np.abs(b) + atol * scale
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} off; worst abs {err.max():.3e} (scale {scale:.3e})"


# ---- scenes (numpy only: tests/test_fwd_tile_wave_scenes_host.py holds every one of them against the oracle alone, without a GPU)

NEIGHBOUR_SPLATS = 7


def _splats(rs, n, tile):
    """n small Gaussians (sigma 0.35 px, radius 3) whose 3-sigma squares lie inside tile `tile` -- and inside the image where the tile
    is ragged -- as fuzz_parity.crafted() places them in tile (1, 1) of its frame."""
    fx = 1.2 * W
    X0, Y0 = (tile % GX) * 16, (tile // GX) * 16
    x1, y1 = min(X0 + 16, W), min(Y0 + 16, H)
    z = rs.uniform(2, 10, n).astype(np.float32)
    px = rs.uniform(X0 + 4.5, max(x1 - 5.5, X0 + 4.6), n); py = rs.uniform(Y0 + 3.6, max(y1 - 5.5, Y0 + 3.7), n)
    x = ((px - W / 2) / fx * z).astype(np.float32); y = ((py - H / 2) / fx * z).astype(np.float32)
    sig = (0.35 * z / fx).astype(np.float32)
    return dict(means3D=np.stack([x, y, z], 1).astype(np.float32), scales=np.stack([sig, sig, sig], 1).astype(np.float32),
                rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (n, 1)), opacities=rs.uniform(0.01, 0.2, (n, 1)).astype(np.float32),
                shs=rs.normal(0, 0.5, (n, 16, 3)).astype(np.float32))


def hot_tile(n, seed, tile=HOT, regime=None):
    """A frame whose tile `tile` has a list of exactly n entries (the first n Gaussians of the scene); the other tiles of its workgroup
    (4 * (tile / 4) ..) that exist have 7 entries each, and 200 Gaussians are sprinkled over the rest of the frame (a fixed sprinkle that
    leaves those workgroups' tiles alone).  `regime`: fuzz_parity.aux_regime's "saturating" / "faint" opacities of the n."""
    s = synthetic_scene(200, W, H, 1, 5)
    rs = np.random.RandomState(seed)
    parts = [_splats(rs, n, tile)] + [_splats(rs, NEIGHBOUR_SPLATS, t) for t in range(tile // 4 * 4, tile // 4 * 4 + 4) if t != tile and t < T]
    out = dict(s)
    for key in ("means3D", "scales", "rotations", "opacities", "shs"):
        out[key] = np.concatenate([p[key] for p in parts] + [s[key]]).astype(np.float32)
    return out if regime is None else _regime(out, n, regime, seed)


def _regime(s, n, regime, seed):
    """fuzz_parity.aux_regime (restated: this module's scenes are also built without a GPU)."""
    s = dict(s)
    op = s["opacities"].copy()
    if regime == "saturating":
        op[:n] = np.minimum(op[:n] * 3.0, 0.99)
    else:
        keep = np.random.RandomState(seed).choice(n, min(n, 150), replace=False)
        faint = np.full((n, 1), 0.003, np.float32)
        faint[keep] = op[:n][keep]
        op[:n] = faint
    s["opacities"] = op.astype(np.float32)
    return s


def with_blockers(s, k, cx, cy, sigma_px, z0=1.2, z1=1.7):
    """`s` plus k opaque round splats of `sigma_px` pixels centred at pixel (cx, cy), in front of everything else."""
    fx = 1.2 * W
    z = np.linspace(z0, z1, k).astype(np.float32)
    means = np.stack([(cx - W / 2) / fx * z, (cy - H / 2) / fx * z, z], 1).astype(np.float32)
    sig = (sigma_px * z / fx).astype(np.float32)
    s = dict(s)
    s["means3D"] = np.concatenate([means, s["means3D"]]).astype(np.float32)
    s["scales"] = np.concatenate([np.stack([sig, sig, sig], 1), s["scales"]]).astype(np.float32)
    s["rotations"] = np.concatenate([np.tile(np.array([[1, 0, 0, 0]], np.float32), (k, 1)), s["rotations"]]).astype(np.float32)
    s["opacities"] = np.concatenate([np.full((k, 1), 0.99, np.float32), s["opacities"]]).astype(np.float32)
    s["shs"] = np.concatenate([np.zeros((k,) + s["shs"].shape[1:], np.float32), s["shs"]]).astype(np.float32)
    return s


QUADRANT_BLOCKERS = 40


def quadrant_scene():
    """300 crafted entries behind 40 opaque splats centred in quadrant 0 of the hot tile (sigma 3 px: alpha 0.27 at the quadrant's
    corners, below 1/255 seven pixels out): quadrant 0 is done among the first 40 entries -- in the middle of the first 64-entry batch --
    while the far pixels of the other three quadrants walk the list to its end."""
    return with_blockers(hot_tile(300, 77), QUADRANT_BLOCKERS, 19.5, 19.5, 3.0)


def early_exit_scene():
    """560 crafted entries behind 40 opaque splats that cover the whole hot tile (sigma 8 px): every pixel of the tile terminates in the
    first batch, so the walk leaves at the first 256-entry boundary with more than half of the list unread (and unmasked).  The list is
    longer than a wave sorts: the workgroup sorts it."""
    return with_blockers(hot_tile(560, 78), 40, 24.0, 24.0, 8.0)


def reach_scene():
    """Sub-pixel splats, splats of a few pixels (one quadrant, or straddling two or three) and splats wider than a tile."""
    s = synthetic_scene(3000, W, H, 1, 5)
    rs = np.random.RandomState(5)
    mult = rs.choice([0.03, 0.4, 1.0, 3.0], size=(3000, 1), p=[0.2, 0.3, 0.3, 0.2])
    s["scales"] = (s["scales"] * mult).astype(np.float32)
    return s


LENGTHS = [63, 64, 65, 127, 128, 129, 255, 256, 257, WAVE_SORT_MAX, WAVE_SORT_MAX + 1, 1024, 1025]


def all_scenes():
    """Every oracle-checked scene of this file, by name."""
    for n in LENGTHS:
        for regime in ("saturating", "faint"):
            yield f"hot {n} {regime}", hot_tile(n, n, HOT, regime)
    for n in (WAVE_SORT_MAX, WAVE_SORT_MAX + 1):
        yield f"corner {n}", hot_tile(n, n, CORNER, "saturating")
    yield "quadrant", quadrant_scene()
    yield "early exit", early_exit_scene()
    yield "reach", reach_scene()


def excluded_share(o):
    return float((o["margin"] < BORDER).mean())


# ---- the K = 2 launch

def _settings(s, dev, K=None):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                         scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]),
                                         sh_degree=s["sh_degree"], campos=t(s["campos"]), prefiltered=False, debug=False)


def _ins(s, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [t(s[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations")]


def _frame_state(eng, f, R):
    """(ranges, point_list, final_T, n_contrib) of frame f of a frames engine, as numpy."""
    L, K = eng.L, eng.K
    b, im = eng.binning.view(K, L.bin_bytes)[f], eng.img.view(K, L.img_bytes)[f]
    v = lambda buf, off, n, dt: buf[off:off + 4 * n].view(dt).cpu().numpy()
    return (v(b, L.bin_ranges, 2 * T, torch.int32).reshape(T, 2).astype(np.uint32), v(b, L.bin_point_list, R, torch.int32).astype(np.uint32),
            v(im, L.img_final_T, H * W, torch.float32).reshape(H, W), v(im, L.img_n_contrib, H * W, torch.int32).reshape(H, W))


def _check_scene(s, dev, o=None, short_lists_too=True):
    """Two frames of the same camera in one launch against the oracle: binning bit for bit, image / final_T / n_contrib at the bar of
    tests/test_gpu_raster.py, both frames the same bits, the direct-binning launch (SG_FLAG_SHORT_LISTS: the waves sort rows of
    tile_keys) the same bits, and every gradient element with the loss on frame 0 alone.  -> (oracle, longest list)."""
    from sings_amd.engine import RasterFramesEngine
    o = o or _oracle(s)
    N = s["means3D"].shape[0]
    cap = max(8 * N + T, 1 << 16)
    assert o["R"] <= cap
    ins = _ins(s, dev)
    eng = RasterFramesEngine(N, W, H, s["shs"].shape[1], 2, dev, cap)
    eng.set_camera(_settings(s, dev))
    Rs = eng.forward(*ins, sync_num_rendered=True)
    assert Rs == [o["R"], o["R"]], (Rs, o["R"])
    border = o["margin"] < BORDER
    strict = ~border
    share = border.mean()
    print(f"excluded pixels: {int(border.sum())} of {border.size} ({100 * share:.4f} %)")
    assert share <= EXCLUDED_MAX, share
    color = eng.color.cpu().numpy()
    states = [_frame_state(eng, f, o["R"]) for f in range(2)]
    for f in range(2):
        ranges, plist, final_T, n_contrib = states[f]
        assert np.array_equal(ranges, o["ranges"]), f
        assert np.array_equal(plist, o["point_list"]), f
        diff = np.abs(color[f] - o["color"]).max(0)
        print(f"frame {f}: rgb worst {diff[strict].max():.3e}, final_T worst {np.abs(final_T - o['final_T'])[strict].max():.3e}")
        assert diff[strict].max() <= RGB_TOL, (f, diff[strict].max())
        assert np.abs(final_T - o["final_T"])[strict].max() <= 1e-5, f
        assert np.array_equal(n_contrib[strict].astype(np.uint32), o["n_contrib"][strict]), f
    assert np.array_equal(color[0], color[1]) and all(np.array_equal(a, b) for a, b in zip(states[0], states[1]))
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    # gradients: the loss on frame 0, none on frame 1 (whose records are zero)
    dL = s["dL_dimage"].copy(); dL[:, border] = 0
    dLk = torch.zeros(2, 3, H, W, device=dev); dLk[0] = torch.from_numpy(dL).to(dev)
    eng.backward(*ins, dLk)
    torch.cuda.synchronize()
    g = ro.backward(o, dL)
    for name, a in (("dL_dmeans3D", eng.d_means3D), ("dL_dopacity", eng.d_opacity), ("dL_dscales", eng.d_scales), ("dL_drots", eng.d_rots),
                    ("dL_dsh", eng.d_sh)):
        _grad_close(name, a.cpu().numpy().reshape(g[name].shape), g[name])
    if short_lists_too and tl.max() <= 1024:
        d = RasterFramesEngine(N, W, H, s["shs"].shape[1], 2, dev, cap)
        d.set_camera(_settings(s, dev), short_lists=True)
        assert d.forward(*ins, sync_num_rendered=True) == Rs
        assert torch.equal(d.color, eng.color)
        for f in range(2):
            assert all(np.array_equal(a, b) for a, b in zip(_frame_state(d, f, o["R"]), states[f])), f
    return o, int(tl.max())


# ---- the cases

@pytest.mark.parametrize("regime", ["saturating", "faint"])
@pytest.mark.parametrize("n", LENGTHS)
def test_list_lengths_on_the_batch_sort_and_checkpoint_boundaries(n, regime):
    """A hot tile (1, 1) whose list length sits on the 64-entry staging batch, the rank-sort / bitonic switch (128), the checkpoint
    and box refresh (256), the per-wave sort limit (512: one past it the workgroup sorts the list together, next to three ordinary
    tiles -- the ragged last tile of row 0 among them) and the workgroup's own limit (1024: one past it the list arrives sorted from
    the binning pass).  Saturating: pixels terminate along the list; faint: most entries are below 1/255 and nothing terminates."""
    dev = _dev()
    s = hot_tile(n, n, HOT, regime)
    o, mx = _check_scene(s, dev)
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert mx == n == tl[HOT] and list(tl[HOT - 2:HOT + 2]) == [NEIGHBOUR_SPLATS, NEIGHBOUR_SPLATS, n, NEIGHBOUR_SPLATS], tl[HOT - 2:HOT + 2]
    assert (tl == 0).any(), "no empty tile"


@pytest.mark.parametrize("n", [WAVE_SORT_MAX, WAVE_SORT_MAX + 1])
def test_the_last_workgroup_sorts_its_only_tile(n):
    """The bottom-right tile (index T - 1 = 4 224, a multiple of four): alone in the last workgroup, whose other three waves are past
    the end, 10 x 6 pixels inside the image; at the per-wave sort limit and, one past it, sorted by the workgroup -- the waves past the
    end take part in that sort and its barriers."""
    dev = _dev()
    assert CORNER % 4 == 0 and CORNER + 1 == T
    s = hot_tile(n, n, CORNER, "saturating")
    o, mx = _check_scene(s, dev)
    assert int(o["ranges"][CORNER, 1]) - int(o["ranges"][CORNER, 0]) == n == mx


def test_one_quadrant_finishes_in_the_middle_of_a_batch():
    """Quadrant 0 of the hot tile saturates among the first 40 entries while the others walk on past the 256-entry checkpoint."""
    dev = _dev()
    s = quadrant_scene()
    o = _oracle(s)
    nc = o["n_contrib"][16:32, 16:32].reshape(2, 8, 2, 8).max(axis=(1, 3)).reshape(4)
    n = int(o["ranges"][HOT, 1]) - int(o["ranges"][HOT, 0])
    assert n > 256 and nc[0] <= QUADRANT_BLOCKERS and min(nc[1:]) > 256, (n, nc)
    _check_scene(s, dev, o)


def test_every_pixel_done_before_the_list_ends():
    """The early exit: all 256 pixels of the hot tile terminate in the first batch, the list is 600 entries long."""
    dev = _dev()
    s = early_exit_scene()
    o = _oracle(s)
    n = int(o["ranges"][HOT, 1]) - int(o["ranges"][HOT, 0])
    nc = o["n_contrib"][16:32, 16:32]
    # (some of the 40 opaque splats, which cover every pixel of the tile, contributed nowhere: every pixel terminated in front of them)
    assert n > WAVE_SORT_MAX and 0 < nc.min() and nc.max() < 40, (n, nc.min(), nc.max())
    _check_scene(s, dev, o)


def _two_cameras(dev):
    s = reach_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], 2, 0).copy(); views[:, 3, 0] = 0.05 * np.arange(2)
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])
    rs = _settings(s, dev)
    return s, rs, t(views), t(projs), t(cps)


def test_two_cameras_in_one_launch_equal_two_single_calls_and_a_second_run_bit_for_bit():
    """K = 2 cameras in one launch == two single-camera calls (image, final_T, n_contrib, sorted lists); a second run of the same
    launch leaves the same bits.  The scene has entries that reach one to four quadrants and none."""
    from sings_amd.engine import RasterEngine, RasterFramesEngine
    dev = _dev()
    s, rs, views, projs, cps = _two_cameras(dev)
    N = s["means3D"].shape[0]
    cap = 12 * N
    ins = _ins(s, dev)
    eng = RasterFramesEngine(N, W, H, 16, 2, dev, cap)
    eng.set_camera(rs._replace(viewmatrix=views, projmatrix=projs, campos=cps))
    Rs = eng.forward(*ins, sync_num_rendered=True)
    first = (eng.color.clone(), [_frame_state(eng, f, Rs[f]) for f in range(2)])
    eng.forward(*ins, sync_num_rendered=True)
    assert torch.equal(eng.color, first[0])
    for f in range(2):
        assert all(np.array_equal(a, b) for a, b in zip(_frame_state(eng, f, Rs[f]), first[1][f])), f
    ref = RasterEngine(N, W, H, 16, dev, cap)
    for f in range(2):
        ref.set_camera(rs._replace(viewmatrix=views[f], projmatrix=projs[f], campos=cps[f]))
        assert ref.forward(*ins, sync_num_rendered=True) == Rs[f]
        assert torch.equal(ref.color, eng.color[f]), f
        L = ref.L
        fT = ref.img[L.img_final_T:L.img_final_T + 4 * H * W].view(torch.float32).cpu().numpy().reshape(H, W)
        nc = ref.img[L.img_n_contrib:L.img_n_contrib + 4 * H * W].view(torch.int32).cpu().numpy().reshape(H, W)
        pl = ref.binning[L.bin_point_list:L.bin_point_list + 4 * Rs[f]].view(torch.int32).cpu().numpy().astype(np.uint32)
        _, plist, final_T, n_contrib = first[1][f]
        assert np.array_equal(fT, final_T) and np.array_equal(nc, n_contrib) and np.array_equal(pl, plist), f


def test_reach_scene_against_the_oracle():
    """Entries that reach one to four quadrants and none, ragged right / bottom tiles with entries: the whole bar."""
    dev = _dev()
    s = reach_scene()
    o, _ = _check_scene(s, dev)
    tl = (o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]).reshape(GY, GX)
    assert tl[:, GX - 1].sum() > 0 and tl[GY - 1].sum() > 0, "the ragged tiles are empty"


def test_a_pair_capacity_overflow_renders_the_background():
    from sings_amd.engine import RasterFramesEngine
    dev = _dev()
    s = reach_scene()
    N = s["means3D"].shape[0]
    eng = RasterFramesEngine(N, W, H, 16, 2, dev, 4096)            # the scene has ~12 k pairs
    eng.set_camera(_settings(s, dev))
    eng.color.fill_(float("nan"))
    Rs = eng.forward(*_ins(s, dev), sync_num_rendered=True)
    assert min(Rs) > 4096
    bg = torch.from_numpy(s["bg"]).to(dev)[None, :, None, None].expand_as(eng.color)
    assert torch.equal(eng.color, bg)


def _as_skinned(s, dev):
    """The scene as one rigid body under the identity: canonical = posed."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    N = s["means3D"].shape[0]
    q = s["rotations"].astype(np.float64); q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                   2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                   2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(N, 3, 3).astype(np.float32)
    A = torch.eye(4, device=dev).reshape(1, 1, 4, 4).repeat(2, 1, 1, 1)
    return dict(xyz=t(s["means3D"]), Rc=t(Rm), sc=t(s["scales"]), op=t(s["opacities"]), sh=t(s["shs"]), w=torch.ones(N, 1, device=dev), A=A)


@pytest.mark.parametrize("which", ["hot 257", "hot 513", "reach"])
def test_the_image_with_the_maps_requested_equals_the_plain_call_and_the_maps_the_oracle(which):
    """The depth / alpha twin of the kernel (K-frame skinned operator, return_aux): colour and radii are the plain call's bits, the
    maps are within 1e-5 (alpha absolute, depth relative to max |z|) of oracle/raster_aux's two-pass composition off the borderline
    pixels.  A list on the checkpoint boundary, one the workgroup sorts, and the many-quadrant scene."""
    from oracle.raster_aux import oracle_pair
    from sings_amd.skinned import rasterize_skinned_frames, rasterize_skinned_gaussians
    dev = _dev()
    s = reach_scene() if which == "reach" else hot_tile(int(which.split()[1]), 9, HOT, "saturating")
    k = _as_skinned(s, dev)
    rs = _settings(s, dev)
    with torch.no_grad():
        plain = rasterize_skinned_frames(k["xyz"], k["Rc"], k["sc"], k["op"], k["sh"], k["w"], k["A"], rs)
        color, radii, depth, alpha = rasterize_skinned_frames(k["xyz"], k["Rc"], k["sc"], k["op"], k["sh"], k["w"], k["A"], rs, return_aux=True)
        _, _, pxyz, pq, psc = rasterize_skinned_gaussians(k["xyz"], k["Rc"], k["sc"], k["op"], k["sh"], k["w"], k["A"][0], rs, return_posed=True)
    assert torch.equal(color, plain[0]) and torch.equal(radii, plain[1])
    assert torch.equal(depth[0], depth[1]) and torch.equal(alpha[0], alpha[1])
    o, oa = oracle_pair(pxyz.cpu().numpy(), s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"], s["tanfovy"],
                        s["bg"], psc.cpu().numpy(), pq.cpu().numpy(), s["shs"], s["sh_degree"])
    np.testing.assert_array_equal(radii[0].cpu().numpy(), o["radii"])
    strict = o["margin"] >= BORDER
    assert 1.0 - strict.mean() <= EXCLUDED_MAX
    zmax = np.abs(o["depths"][o["radii"] > 0]).max()
    a, d = alpha[0, 0].cpu().numpy(), depth[0, 0].cpu().numpy()
    print(f"alpha worst {np.abs(a - oa['color'][1])[strict].max():.3e}, depth worst {np.abs(d - oa['color'][0])[strict].max():.3e} (zmax {zmax:.3f})")
    assert np.abs(color[0].cpu().numpy() - o["color"]).max(0)[strict].max() <= RGB_TOL
    assert np.abs(a - oa["color"][1])[strict].max() <= 1e-5
    assert np.abs(d - oa["color"][0])[strict].max() <= 1e-5 * zmax
    assert np.abs(a - (1.0 - o["final_T"]))[strict].max() <= 1e-5
