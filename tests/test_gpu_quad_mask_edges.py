"""The quadrant masks of the dense composites (frames of more than 4 096 tiles, K frames per launch).  The forward's quadrant test
evaluates the two edges of a quadrant's live box that face the splat's mean (sg_min_q_rect); the backward walk keeps a batch's masks as
four lane masks in scalar registers and folds "not behind the quadrant's deepest contributor" into them once per batch
(sings_amd/csrc/sg_render.hip, sg_render_bwd.inc).  A mask bit that goes missing loses a pixel's contribution in the image and in
every gradient; these scenes put the bits on their edges:

 * splats whose accepted region (alpha >= 1/255) enters a quadrant through its single corner pixel, from each of the four sides;
 * splats that enter a quadrant through one pixel column or row, from the left, right, top and bottom: the mean inside the quadrant's
   y range and outside its x range, and the reverse;
 * a tile of the right column and one of the bottom row, whose boxes are clipped to the image, entered through the clipped edge's
   last column / row by splats whose means lie outside the image -- and the bottom tile's lower quadrants have empty boxes;
 * lists of 64, 65, 128 and 129 entries with the crafted splats in front (the first batch) or at the back (the last, which holds one
   entry when the list has 65 or 129);
 * a list longer than 256 entries behind an opaque front, so that the live boxes are strict sub-rectangles when the later batches are
   staged;
 * a quadrant whose deepest contributor lies in the middle of a batch, with entries behind it in that batch that still carry the
   quadrant's bit.

Every case runs on the ragged 1034 x 1030 frame of tests/test_gpu_fwd_tile_wave.py (65 x 65 tiles), K = 2 frames per launch, with that
file's bars: image, final_T and n_contrib against the oracle (1e-5, equal; off the pixels within 2e-5 of a hard threshold, at most
0.1 % of the frame), binning bit for bit, every gradient at `_grad_close`.  tests/test_quad_mask_edges_scenes_host.py asserts from the
oracle alone that the scenes hold these cases."""
import numpy as np
import pytest
import torch

import test_gpu_fwd_tile_wave as tw

pytestmark = pytest.mark.gpu

W, H, GX, GY, T, HOT = tw.W, tw.H, tw.GX, tw.GY, tw.T, tw.HOT
RIGHT = 3 * GX + GX - 1            # tile (64, 3): pixel columns 1024..1033 inside the image
BOTTOM = (GY - 1) * GX + 5         # tile (5, 64): pixel rows 1024..1029 inside the image
FX = 1.2 * W


def spots(specs):
    """One round splat per (px, py, reach, opacity, z): its mean projects to the pixel-centre coordinate (px, py) and its accepted
    region is the disc of `reach` pixels around it -- reach^2 = 2 ln(255 o) (sigma^2 + 0.3), the 0.3 being the preprocess' dilation."""
    px, py, reach, op, z = (np.array(v, np.float64) for v in zip(*specs))
    sig = np.sqrt(reach * reach / (2.0 * np.log(255.0 * op)) - 0.3)
    n = len(specs)
    rs = np.random.RandomState(n)
    means = np.stack([(px + 0.5 - W / 2) / FX * z, (py + 0.5 - H / 2) / FX * z, z], 1)
    s3 = (sig * z / FX)[:, None].repeat(3, 1)
    return dict(means3D=means.astype(np.float32), scales=s3.astype(np.float32), rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (n, 1)),
                opacities=op.reshape(n, 1).astype(np.float32), shs=rs.normal(0, 0.5, (n, 16, 3)).astype(np.float32))


def _join(s, *parts):
    out = dict(s)
    for key in ("means3D", "scales", "rotations", "opacities", "shs"):
        out[key] = np.concatenate([p[key] for p in parts] + [s[key]]).astype(np.float32)
    return out


# (name, pixel of the mean, reach, the quadrant entered, the accepted pixels of that quadrant) -- in the hot tile (1, 1): pixels 16..31,
# quadrants split at 24.  The accepted pixels are one corner pixel (x, y), or some pixels of one column ("x", x) or one row ("y", y).
CORNERS = [("corner 0>3", (22.0, 22.0), 3.2, 3, (24, 24)), ("corner 1>2", (25.0, 22.0), 3.2, 2, (23, 24)),
           ("corner 2>1", (22.0, 25.0), 3.2, 1, (24, 23)), ("corner 3>0", (25.0, 25.0), 3.2, 0, (23, 23))]
LINES = [("column 0>1", (21.5, 19.5), 2.7, 1, ("x", 24)), ("column 1>0", (25.5, 19.5), 2.7, 0, ("x", 23)),
         ("row 0>2", (19.5, 21.5), 2.7, 2, ("y", 24)), ("row 2>0", (19.5, 25.5), 2.7, 0, ("y", 23))]
HOT_SPOTS = CORNERS + LINES
# the ragged tiles (name, tile, ...): means outside the image, entering the clipped box through its last column / row; one entering it from
# inside the image; one whose mean lies inside the clipped box (None: the mean's own pixels are accepted)
RAGGED = [("right from outside", RIGHT, (1036.5, 51.5), 3.7, 1, ("x", 1033)), ("right from inside", RIGHT, (1029.5, 59.5), 2.7, 3, ("x", 1032)),
          ("bottom from outside", BOTTOM, (83.5, 1032.5), 3.7, 0, ("y", 1029)), ("bottom inside the clipped box", BOTTOM, (86.5, 1026.5), 2.9, 0, None)]


def edge_scene(n, front):
    """The hot tile's list has exactly n entries: the eight crafted splats of HOT_SPOTS, in front of (`front`) or behind n - 8 small
    faint ones; the four RAGGED splats sit in their tiles.  Nothing saturates: every accepted pixel blends."""
    z = 1.5 if front else 12.0
    hot = spots([(p[0], p[1], r, 0.5, z + 0.01 * i) for i, (_, p, r, _, _) in enumerate(HOT_SPOTS)])
    rag = spots([(p[0], p[1], r, 0.9, 1.5 + 0.01 * i) for i, (_, _, p, r, _, _) in enumerate(RAGGED)])
    return _join(tw.hot_tile(n - len(HOT_SPOTS), 100 + n, HOT, "faint"), hot, rag)


SHRINK_BLOCKERS = 40


def shrink_scene():
    """300 crafted entries behind 40 opaque splats of sigma 20 px centred 40 px right of the hot tile's centre: the tile's pixels within
    ~35 px of that centre -- everything right of column 18 to 20 -- terminate in the first batch, the rest stay live.  At entry 256 the
    live boxes of quadrants 0 and 2 are their left three and five columns, those of quadrants 1 and 3 are empty."""
    return tw.with_blockers(tw.hot_tile(300, 79), SHRINK_BLOCKERS, 57.0, 24.0, 20.0)


LENGTHS = [(64, True), (65, True), (65, False), (128, True), (129, True), (129, False)]


def all_scenes():
    for n, front in LENGTHS:
        yield f"edges {n} {'front' if front else 'back'}", edge_scene(n, front)
    yield "shrink", shrink_scene()
    yield "deepest", tw.quadrant_scene()


# ---- the cases

@pytest.mark.parametrize("n,front", LENGTHS)
def test_corner_pixels_single_lines_and_clipped_boxes_at_the_batch_boundaries(n, front):
    o, mx = tw._check_scene(edge_scene(n, front), tw._dev())
    assert mx == n


def test_live_boxes_that_shrank_behind_an_opaque_front():
    o, mx = tw._check_scene(shrink_scene(), tw._dev())
    assert mx > 256


def test_a_quadrant_whose_deepest_contributor_lies_inside_a_batch():
    tw._check_scene(tw.quadrant_scene(), tw._dev())


def _two_cameras(s, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], 2, 0).copy(); views[:, 3, 0] = 0.002 * np.arange(2)
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])
    return tw._settings(s, dev), t(views), t(projs), t(cps)


@pytest.mark.parametrize("which", ["edges", "shrink"])
def test_two_cameras_in_one_launch_equal_two_single_calls_and_a_second_run_bit_for_bit(which):
    """Images, final_T, n_contrib, sorted lists and the summed gradients of K = 2 cameras in one launch are those of two single-camera
    calls (the second accumulating), and a second run of the launch leaves the same bits."""
    from sings_amd.engine import RasterEngine, RasterFramesEngine
    dev = tw._dev()
    s = edge_scene(129, False) if which == "edges" else shrink_scene()
    rs, views, projs, cps = _two_cameras(s, dev)
    N = s["means3D"].shape[0]
    cap = max(8 * N + T, 1 << 16)
    ins = tw._ins(s, dev)
    dL = torch.from_numpy(np.random.RandomState(2).normal(0, 1, (2, 3, H, W)).astype(np.float32)).to(dev)
    eng = RasterFramesEngine(N, W, H, 16, 2, dev, cap)
    eng.set_camera(rs._replace(viewmatrix=views, projmatrix=projs, campos=cps))
    runs = []
    for _ in range(2):
        Rs = eng.forward(*ins, sync_num_rendered=True)
        eng.backward(*ins, dL)
        torch.cuda.synchronize()
        runs.append((eng.color.clone(), [tw._frame_state(eng, f, Rs[f]) for f in range(2)], eng.grad_flat.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    for f in range(2):
        assert all(np.array_equal(a, b) for a, b in zip(runs[0][1][f], runs[1][1][f])), f
    assert bool(torch.isfinite(runs[0][2]).all()) and float(runs[0][2].abs().max()) > 0
    ref = RasterEngine(N, W, H, 16, dev, cap); ref.throughput = True
    for f in range(2):
        ref.set_camera(rs._replace(viewmatrix=views[f], projmatrix=projs[f], campos=cps[f]))
        assert ref.forward(*ins, sync_num_rendered=True) == Rs[f]
        ref.backward(*ins, dL[f], accumulate=f > 0)
        torch.cuda.synchronize()
        assert torch.equal(ref.color, runs[0][0][f]), f
        L = ref.L
        fT = ref.img[L.img_final_T:L.img_final_T + 4 * H * W].view(torch.float32).cpu().numpy().reshape(H, W)
        nc = ref.img[L.img_n_contrib:L.img_n_contrib + 4 * H * W].view(torch.int32).cpu().numpy().reshape(H, W)
        pl = ref.binning[L.bin_point_list:L.bin_point_list + 4 * Rs[f]].view(torch.int32).cpu().numpy().astype(np.uint32)
        _, plist, final_T, n_contrib = runs[0][1][f]
        assert np.array_equal(fT, final_T) and np.array_equal(nc, n_contrib) and np.array_equal(pl, plist), f
    assert torch.equal(ref.grad_flat, runs[0][2])


@pytest.mark.parametrize("which", ["edges", "shrink"])
def test_the_depth_alpha_twin_equals_the_plain_call(which):
    """The K-frame skinned operator with the maps requested (the aux forward and backward kernels) against the plain call: colour and radii the same bits, and with no loss on the maps every gradient the same
    bits; colour and both maps against the oracle of the posed Gaussians."""
    from sings_amd.skinned import rasterize_skinned_frames
    dev = tw._dev()
    s = edge_scene(129, False) if which == "edges" else shrink_scene()
    rs = tw._settings(s, dev)
    dL = torch.from_numpy(np.random.RandomState(3).normal(0, 1, (2, 3, H, W)).astype(np.float32)).to(dev)
    got = []
    for aux in (False, True):
        k = tw._as_skinned(s, dev)
        leaves = [k[name].requires_grad_(True) for name in ("xyz", "sc", "op", "sh")]
        out = rasterize_skinned_frames(k["xyz"], k["Rc"], k["sc"], k["op"], k["sh"], k["w"], k["A"], rs, return_aux=aux)
        (out[0] * dL).sum().backward()
        got.append((out, [v.grad.clone() for v in leaves]))
    (plain, gp), (twin, ga) = got
    assert torch.equal(twin[0], plain[0]) and torch.equal(twin[1], plain[1])
    for name, a, b in zip(("xyz", "sc", "op", "sh"), ga, gp):
        assert torch.equal(a, b), name
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
    # the maps against oracle/raster_aux's two-pass composition of the POSED Gaussians (the skinned operator's own means, rotations and
    # scales), at the bars of tests/test_gpu_fwd_tile_wave.py
    from oracle.raster_aux import oracle_pair
    from sings_amd.skinned import rasterize_skinned_gaussians
    with torch.no_grad():
        _, _, pxyz, pq, psc = rasterize_skinned_gaussians(k["xyz"], k["Rc"], k["sc"], k["op"], k["sh"], k["w"], k["A"][0], rs, return_posed=True)
    o, oa = oracle_pair(pxyz.cpu().numpy(), s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"], s["tanfovy"],
                        s["bg"], psc.cpu().numpy(), pq.cpu().numpy(), s["shs"], s["sh_degree"])
    strict = o["margin"] >= tw.BORDER
    assert 1.0 - strict.mean() <= tw.EXCLUDED_MAX
    zmax = np.abs(o["depths"][o["radii"] > 0]).max()
    a, d = twin[3][0, 0].detach().cpu().numpy(), twin[2][0, 0].detach().cpu().numpy()
    print(f"alpha worst {np.abs(a - oa['color'][1])[strict].max():.3e}, depth worst {np.abs(d - oa['color'][0])[strict].max():.3e} (zmax {zmax:.3f})")
    assert np.abs(twin[0][0].detach().cpu().numpy() - o["color"]).max(0)[strict].max() <= tw.RGB_TOL
    assert np.abs(a - oa["color"][1])[strict].max() <= 1e-5
    assert np.abs(d - oa["color"][0])[strict].max() <= 1e-5 * zmax
    assert np.abs(a - (1.0 - o["final_T"]))[strict].max() <= 1e-5
