"""The dense backward composite's accumulate step (sings_amd/csrc/sg_render_bwd.inc, SG_BWD_QUAD): an entry's FIRST accumulating quadrant
assigns the nine (aux: ten) per-lane partials, every later one adds them -- quadrant 0 statically in the assigning form, quadrants
1-3 behind a scalar branch on "some earlier quadrant of this entry accumulated".

Every case runs on the 1034 x 1030 frame of tests/test_gpu_bwd_tile_wave.py: 65 x 65 = 4 225 tiles (the smallest ragged frame in the dense
kernels' regime); the right column of tiles has 10 of its 16 pixel columns inside the image, the bottom row 6 of its 16 rows
(quadrants 2 and 3 wholly outside).  A few thousand Gaussians.  Gradients against oracle/raster_oracle at the bar of
tests/test_gpu_raster.py (`_grad_close`: rtol 2e-4 + 2e-6 max|g|, pixels within 2e-5 of a hard threshold carry no loss), except
the stale-accumulator case, whose bar is per gradient ROW (see there).  tests/test_bwd_first_quadrant_scenes_host.py asserts from
the oracle alone that the scenes contain what the cases are about."""
import numpy as np
import pytest
import torch

import test_gpu_bwd_tile_wave as tw
from oracle import raster_oracle as ro
from sings_amd.scene import synthetic_scene

pytestmark = pytest.mark.gpu

W, H, GX, GY, BORDER = tw.W, tw.H, tw.GX, tw.GY, tw.BORDER
FX = 1.2 * W

# (tile x, tile y, orientation) of the blocker clusters: "h" skips quadrant 0 and assigns in quadrant 1, "v" skips quadrant 0 and
# assigns in quadrant 2.  Interior tiles, the right column (x = 64) and the bottom row (y = 64: its quadrants 2, 3 are outside)
CLUSTERS = ((10, 10, "h"), (12, 10, "v"), (GX - 1, 20, "h"), (GX - 1, 24, "v"), (20, GY - 1, "h"))
BLOCKERS = 16
# (tile x, tile y, quadrant of the faint entry) of the stale-accumulator pairs
STALE = ((10, 10, 0), (14, 10, 1), (10, 14, 2), (14, 14, 3))
STALE_WINDOW = (2, 6)                  # pixels [2, 6) x [2, 6) of the faint entry's quadrant carry the small dL/dpixel (it reaches the middle four)
STALE_BIG, STALE_SMALL = 1e6, 1e-6     # dL/dpixel scales: the big entry's pixels, the faint entry's


def _splat(px, py, z, sx, sy, opacity):
    """One axis-aligned Gaussian whose centre projects to pixel coordinate (px, py), sigma (sx, sy) pixels before the 0.3 px^2 filter."""
    mean = [(px + 0.5 - W / 2) / FX * z, (py + 0.5 - H / 2) / FX * z, z]
    return mean, [sx * z / FX, sy * z / FX, min(sx, sy) * z / FX], opacity


def _with_splats(s, splats, seed):
    """`splats` in front of scene `s` (Gaussian ids 0..len - 1)."""
    k = len(splats)
    rs = np.random.RandomState(seed)
    s = dict(s)
    s["means3D"] = np.concatenate([np.array([m for m, _, _ in splats], np.float32), s["means3D"]]).astype(np.float32)
    s["scales"] = np.concatenate([np.array([c for _, c, _ in splats], np.float32), s["scales"]]).astype(np.float32)
    s["rotations"] = np.concatenate([np.tile(np.array([[1, 0, 0, 0]], np.float32), (k, 1)), s["rotations"]]).astype(np.float32)
    s["opacities"] = np.concatenate([np.array([[o] for _, _, o in splats], np.float32), s["opacities"]]).astype(np.float32)
    s["shs"] = np.concatenate([rs.normal(0, 0.5, (k,) + s["shs"].shape[1:]).astype(np.float32), s["shs"]]).astype(np.float32)
    return s


def cluster(tx, ty, orient):
    """BLOCKERS opaque splats with a sharp edge over the inner columns (rows, "v") of quadrant 0, a small splat behind them that
    straddles the border to quadrant 1 (2) -- the pixels it reaches in quadrant 0 have terminated among the blockers, those beyond the
    border are live -- and a small splat behind both in the blockers' lee, so that quadrant 0's deepest contributor lies behind
    the straddler: the kernel evaluates the straddler in quadrant 0, finds no valid pixel, and quadrant 1 (2) is its first."""
    X0, Y0 = 16 * tx, 16 * ty
    t = (lambda a, b: (a, b)) if orient == "h" else (lambda a, b: (b, a))
    out = []
    for z in np.linspace(1.2, 1.5, BLOCKERS):
        (cx, cy), (sx, sy) = t(6.0, 2.5), t(0.837, 4.0)
        out.append(_splat(X0 + cx, Y0 + cy, float(z), sx, sy, 0.99))
    cx, cy = t(7.5, 2.5)
    out.append(_splat(X0 + cx, Y0 + cy, 1.6, 0.35, 0.35, 0.9))          # the straddler: id BLOCKERS of its cluster
    out.append(_splat(X0 + 1.0, Y0 + 1.0, 1.7, 0.35, 0.35, 0.9))        # quadrant 0's deepest contributor
    return out


CLUSTER_SPLATS = BLOCKERS + 2


def reach_scene():
    """tests/test_gpu_bwd_tile_wave.py's scene of mixed splat sizes (every first quadrant with every reach) with the blocker clusters in front."""
    splats = [sp for c in CLUSTERS for sp in cluster(*c)]
    return _with_splats(tw._reach_scene(), splats, 7)


def straddler_id(i):
    return i * CLUSTER_SPLATS + BLOCKERS


def stale_scene():
    """Per STALE tile: a splat wider than the tile (all four quadrants) and, directly in front of it in the tile's list, a faint
    sub-pixel splat (not round: its rotation takes a gradient too) in the middle of one quadrant; a sprinkle of other splats behind them."""
    splats = []
    for tx, ty, q in STALE:
        X0, Y0 = 16 * tx, 16 * ty
        splats.append(_splat(X0 + 3.5 + 8 * (q & 1), Y0 + 3.5 + 8 * (q >> 1), 1.5, 0.35, 0.45, 0.05))     # ids 0, 2, 4, 6: faint
        splats.append(_splat(X0 + 7.5, Y0 + 7.5, 1.5001, 5.0, 5.0, 0.8))                                  # ids 1, 3, 5, 7: big
    return _with_splats(synthetic_scene(1500, W, H, 1, 9), splats, 8)


def stale_dL(s, margin):
    """dL/dpixel ~ N(0, 1) times STALE_BIG over the STALE tiles, times STALE_SMALL in the window around each faint entry; borderline pixels none."""
    dL = s["dL_dimage"].copy()
    for tx, ty, q in STALE:
        X0, Y0 = 16 * tx, 16 * ty
        dL[:, Y0:Y0 + 16, X0:X0 + 16] *= STALE_BIG
        qx, qy = X0 + 8 * (q & 1), Y0 + 8 * (q >> 1)
        dL[:, qy + STALE_WINDOW[0]:qy + STALE_WINDOW[1], qx + STALE_WINDOW[0]:qx + STALE_WINDOW[1]] *= STALE_SMALL / STALE_BIG
    dL[:, margin < BORDER] = 0
    return dL.astype(np.float32)


def quadrant_census(o, tile):
    """Per list entry of `tile` and quadrant, in the oracle's composite: `geo` -- some pixel of the quadrant inside the image has
    power <= 0 and alpha >= 1/255; `hit` -- such a pixel is still live at the entry (in front of the pixel's last contributor); and
    per quadrant the deepest contributor `maxq` (the per-quadrant version of tests/test_gpu_bwd_tile_wave.py::_quadrant_reach)."""
    lo, hi = int(o["ranges"][tile, 0]), int(o["ranges"][tile, 1])
    X0, Y0 = (tile % GX) * 16, (tile // GX) * 16
    py, px = np.mgrid[Y0:Y0 + 16, X0:X0 + 16]
    inside = (px < W) & (py < H)
    nc = np.where(inside, o["n_contrib"][np.minimum(py, H - 1), np.minimum(px, W - 1)], 0)
    maxq = nc.reshape(2, 8, 2, 8).max(axis=(1, 3)).reshape(4)
    if hi == lo:
        return np.zeros((0, 4), bool), np.zeros((0, 4), bool), maxq
    ids = o["point_list"][lo:hi].astype(np.int64)
    xy, co = o["xy"][ids].astype(np.float64), o["conic_opacity"][ids].astype(np.float64)
    dx = xy[:, 0, None, None] - px[None]; dy = xy[:, 1, None, None] - py[None]
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    alpha = np.minimum(0.99, co[:, 3, None, None] * np.exp(power))
    geo = inside[None] & (power <= 0) & (alpha >= 1.0 / 255.0)
    hit = geo & (np.arange(hi - lo)[:, None, None] < nc[None])
    quads = lambda m: m.reshape(-1, 2, 8, 2, 8).any(axis=(2, 4)).reshape(-1, 4)
    return quads(geo), quads(hit), maxq


def first_and_reach(hit):
    """Per entry: its first accumulating quadrant (4: none) and the number of quadrants it accumulates in."""
    return np.where(hit.any(1), hit.argmax(1), 4), hit.sum(1)


def skipped_in_front(geo, hit, maxq):
    """Entries with a quadrant the kernel evaluates (reached geometrically, in front of the quadrant's deepest contributor) and
    skips (no reached pixel still live) in front of their first accumulating quadrant."""
    first, _ = first_and_reach(hit)
    pos = np.arange(len(geo))[:, None]
    skipped = geo & ~hit & (pos < maxq[None])
    return np.array([first[e] < 4 and skipped[e, :first[e]].any() for e in range(len(geo))], bool)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_ORACLES = {}


def oracle_of(name):
    """(scene, oracle forward, dL/dimage with the borderline pixels cleared, oracle gradients): computed once per scene, never changed."""
    if name not in _ORACLES:
        s = reach_scene() if name == "reach" else stale_scene()
        o = tw._oracle(s)
        if name == "reach":
            dL = s["dL_dimage"].copy(); dL[:, o["margin"] < BORDER] = 0
        else:
            dL = stale_dL(s, o["margin"])
        _ORACLES[name] = (s, o, dL, ro.backward(o, dL))
    return _ORACLES[name]


_PLAIN = {}


def _plain(name, dev):
    if name not in _PLAIN:
        s, _, dL, _ = oracle_of(name)
        _PLAIN[name] = {k: v.cpu().numpy() for k, v in tw._hip_grads(s, dL, dev).items()}
    return _PLAIN[name]


def test_every_first_quadrant_with_every_reach_and_the_ragged_tiles():
    """Each first quadrant, a quadrant skipped in front of the first accumulating one, and both on the ragged right column and
    bottom row (the scene is asserted to hold them in the host twin): every gradient against the oracle."""
    dev = tw._dev()
    _, _, _, g = oracle_of("reach")
    got = _plain("reach", dev)
    for name, a in got.items():
        print(name, "worst abs", np.abs(a.reshape(g[name].shape) - g[name]).max(), "scale", np.abs(g[name]).max())
        tw._grad_close(name, a.reshape(g[name].shape), g[name])


def row_close(name, a, b, rows, rtol=2e-4):
    """Rows `rows` of gradient `a` against the oracle's within rtol of THAT ROW's largest oracle magnitude."""
    a = a.astype(np.float64).reshape(b.shape); b = b.astype(np.float64)
    for r in rows:
        scale = np.abs(b[r]).max()
        err = np.abs(a[r] - b[r]).max()
        print(f"{name} row {r}: worst abs {err:.3e}, row scale {scale:.3e}, array scale {np.abs(b).max():.3e}")
        assert scale > 0 and err <= rtol * scale, f"{name} row {r}: worst abs {err:.3e} against row scale {scale:.3e}"


def test_a_faint_entry_filed_behind_an_entry_with_sums_1e12_times_larger():
    """Stale accumulators: the backward walks back to front, so the big entry's sums are what the registers hold when the faint
    entry's first quadrant (0, 1, 2 or 3) assigns.  The faint Gaussians' gradient rows against the oracle relative to the ROW's own
    magnitude (the bar over the whole array, 2e-6 of its largest element, would hide a leak of the neighbour's sums); then the
    whole arrays at the usual bar."""
    dev = tw._dev()
    _, _, _, g = oracle_of("stale")
    got = _plain("stale", dev)
    faint = [2 * i for i in range(len(STALE))]
    for name, a in got.items():
        row_close(name, a, g[name], faint)
    for name, a in got.items():
        tw._grad_close(name, a.reshape(g[name].shape), g[name])


def _engine_inputs(K, dev):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    s = reach_scene()
    t = lambda a: _t(a, dev)
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], K, 0).copy(); views[:, 3, 0] = 0.02 * np.arange(K)
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])

    def settings(vm, pm, cp):
        return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                             scale_modifier=1.0, viewmatrix=vm, projmatrix=pm, sh_degree=1, campos=cp,
                                             prefiltered=False, debug=False)
    ins = [t(s[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    dL = t(np.random.RandomState(1).normal(0, 1, (K, 3, H, W)).astype(np.float32))
    return s, settings, ins, dL, t(views), t(projs), t(cps)


def test_two_cameras_in_one_launch_equal_two_single_calls_and_a_second_run_bit_for_bit():
    """K = 2 through the frames entry points == two single calls, the second with accumulate; the K = 2 launch twice: the same bits."""
    from sings_amd.engine import RasterEngine, RasterFramesEngine
    dev = tw._dev()
    K = 2
    s, settings, ins, dL, views, projs, cps = _engine_inputs(K, dev)
    N = s["means3D"].shape[0]
    cap = 16 * N
    ref = RasterEngine(N, W, H, 4, dev, cap); ref.throughput = True
    per = []
    for f in range(K):
        ref.set_camera(settings(views[f], projs[f], cps[f]))
        ref.forward(*ins, sync_num_rendered=True)
        ref.backward(*ins, dL[f], accumulate=f > 0)
        torch.cuda.synchronize()
        per.append((ref.color.clone(), ref.d_means2D.clone()))
    eng = RasterFramesEngine(N, W, H, 4, K, dev, cap)
    eng.set_camera(settings(views, projs, cps))
    runs = []
    for _ in range(2):
        eng.forward(*ins, sync_num_rendered=True)
        eng.backward(*ins, dL)
        torch.cuda.synchronize()
        runs.append((eng.color.clone(), eng.d_means2D.clone(), eng.grad_flat.clone()))
    for f in range(K):
        assert torch.equal(runs[0][0][f], per[f][0]) and torch.equal(runs[0][1][f], per[f][1]), f
    assert torch.equal(runs[0][2], ref.grad_flat)
    assert bool(torch.isfinite(runs[0][2]).all()) and bool((runs[0][2] != 0).any())
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


AUX_KEYS = (("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacities"), ("dL_dscales", "scales"), ("dL_drots", "rotations"), ("dL_dsh", "shs"))


@pytest.mark.parametrize("name", ["reach", "stale"])
def test_the_depth_alpha_twin_without_map_adjoints_leaves_the_plain_kernels_bits(name):
    """sg_render_bwd_aux_kernel with dL/ddepth = dL/dalpha = 0: the colour-path gradients of the plain call, bit for bit."""
    dev = tw._dev()
    fp = tw._fuzz()
    s, _, dL, _ = oracle_of(name)
    zero = np.zeros((H, W), np.float32)
    x = fp.aux_abi(s, dL, zero, zero)
    plain = _plain(name, dev)
    for gname, key in AUX_KEYS:
        assert np.array_equal(x["grads"][key].cpu().numpy().reshape(plain[gname].shape), plain[gname]), gname


@pytest.mark.parametrize("name", ["reach", "stale"])
def test_the_depth_alpha_twin_with_map_adjoints_against_the_oracle(name):
    """The tenth partial (dL/dz) in its assigning and its adding form: a loss on colour, depth and alpha; every gradient against
    the oracle's colour pass + (z, 1) pass (oracle/raster_aux.py).  On the stale scene the map adjoints carry the colour adjoint's
    scales, and the faint Gaussians' rows are held to their own magnitude as in the plain case."""
    from oracle.raster_aux import oracle_pair, reference_grads
    tw._dev()
    fp = tw._fuzz()
    s, o, dL, _ = oracle_of(name)
    o2, oa = oracle_pair(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"], s["tanfovy"],
                         s["bg"], s["scales"], s["rotations"], s["shs"], s["sh_degree"])
    rng = np.random.RandomState(11)
    gD = rng.normal(0, 1, (H, W)).astype(np.float32); gA = rng.normal(0, 1, (H, W)).astype(np.float32)
    if name == "stale":                                    # the scale of dL/dimage per pixel
        scale = np.abs(stale_dL(dict(s, dL_dimage=np.ones_like(s["dL_dimage"])), np.ones((H, W), np.float32))).max(0)
        gD *= scale; gA *= scale
    border = (o["margin"] < BORDER) | (oa["margin"] < BORDER)
    gD[border] = 0; gA[border] = 0
    dLc = dL.copy(); dLc[:, border] = 0
    ref = reference_grads(o2, oa, dLc, gD, gA, s["viewmatrix"])
    x = fp.aux_abi(s, dLc, gD, gA)
    assert float(np.abs(ref["means3D"]).max()) > 0
    if name == "stale":
        for key in ("means3D", "opacities", "scales", "rotations", "shs"):
            row_close(key, x["grads"][key].cpu().numpy(), np.asarray(ref[key]), [2 * i for i in range(len(STALE))])
    for key in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        a = x["grads"][key].cpu().numpy(); b = np.asarray(ref[key])
        print(key, "worst abs", np.abs(a.reshape(b.shape) - b).max(), "scale", np.abs(b).max())
        tw._grad_close(key, a.reshape(b.shape), b)
