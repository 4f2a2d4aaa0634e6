"""The dense backward composite (frames of more than 4 096 tiles): one wave per work item (tile, depth segment), four items per
workgroup, each lane owning one pixel of each of the tile's four 8x8 quadrants; an entry's partials are added over the quadrants
it reaches and summed by ONE lane butterfly (sings_amd/csrc/sg_render_bwd.inc).

Every case runs on a 1034 x 1030 frame: 65 x 65 = 4 225 tiles (the dense kernels' regime), the right column of tiles has only its
left quadrants inside the image (10 of 16 pixel columns), the bottom row only a 6-pixel strip of its upper quadrants.  A few
thousand Gaussians, so the scalar oracle takes a fraction of a second.  Gradients against oracle/raster_oracle at the bar of
tests/test_gpu_raster.py (`_grad_close`: rtol 2e-4 + 2e-6 max|g|); crafted lists through tests/tools/fuzz_parity.py at its own."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from sings_amd.scene import synthetic_scene

pytestmark = pytest.mark.gpu

W, H = 1034, 1030
GX, GY = (W + 15) // 16, (H + 15) // 16
BORDER = 2e-5


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(__file__), "tools", "fuzz_parity.py"))
    fp = importlib.util.module_from_spec(spec); spec.loader.exec_module(fp)
    return fp


def _oracle(s):
    return ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                      s["tanfovy"], s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=s["sh_degree"])


def _grad_close(name, a, b, rtol=2e-4, atol=2e-6):
    a = a.astype(np.float64); b = b.astype(np.float64)
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b)
    bad = err > rtol * np.abs(b) + atol * scale
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} off; worst abs {err.max():.3e} (scale {scale:.3e})"


def _hip_grads(s, dL, dev):
    """Forward + backward through the drop-in autograd surface -> gradients as numpy, oracle names."""
    from diff_gaussian_rasterization import GaussianRasterizer
    fp = _fuzz()
    rs = fp.settings(s)
    req = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True)
    m, op, sh, sc, rt = req(s["means3D"]), req(s["opacities"]), req(s["shs"]), req(s["scales"]), req(s["rotations"])
    color, _ = GaussianRasterizer(rs)(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=op, shs=sh, scales=sc, rotations=rt)
    color.backward(torch.from_numpy(dL).to(dev))
    return dict(dL_dmeans3D=m.grad, dL_dopacity=op.grad, dL_dscales=sc.grad, dL_drots=rt.grad, dL_dsh=sh.grad)


def _against_oracle(s, o, dev):
    dL = s["dL_dimage"].copy(); dL[:, o["margin"] < BORDER] = 0
    g = ro.backward(o, dL)
    got = _hip_grads(s, dL, dev)
    for name, a in got.items():
        _grad_close(name, a.cpu().numpy().reshape(g[name].shape), g[name])
    return got


def _quadrant_reach(o, tile):
    """Per list entry of `tile`: the number of 8x8 quadrants in which some pixel takes a contribution from it in the oracle's
    composite (inside the image, in front of the pixel's last contributor, power <= 0, alpha >= 1/255)."""
    lo, hi = int(o["ranges"][tile, 0]), int(o["ranges"][tile, 1])
    if hi == lo:
        return np.zeros(0, int)
    ids = o["point_list"][lo:hi].astype(np.int64)
    X0, Y0 = (tile % GX) * 16, (tile // GX) * 16
    py, px = np.mgrid[Y0:Y0 + 16, X0:X0 + 16]
    inside = (px < W) & (py < H)
    nc = np.where(inside, o["n_contrib"][np.minimum(py, H - 1), np.minimum(px, W - 1)], 0)
    xy, co = o["xy"][ids].astype(np.float64), o["conic_opacity"][ids].astype(np.float64)
    dx = xy[:, 0, None, None] - px[None]; dy = xy[:, 1, None, None] - py[None]
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    alpha = np.minimum(0.99, co[:, 3, None, None] * np.exp(power))
    hit = (np.arange(hi - lo)[:, None, None] < nc[None]) & (power <= 0) & (alpha >= 1.0 / 255.0)
    quads = hit.reshape(-1, 2, 8, 2, 8).any(axis=(2, 4)).reshape(-1, 4)
    return quads.sum(1)


def _reach_scene():
    """Sub-pixel splats, splats of a few pixels (one quadrant, or straddling two or three) and splats wider than a tile."""
    s = synthetic_scene(3000, W, H, 1, 5)
    rs = np.random.RandomState(5)
    mult = rs.choice([0.03, 0.4, 1.0, 3.0], size=(3000, 1), p=[0.2, 0.3, 0.3, 0.2])
    s["scales"] = (s["scales"] * mult).astype(np.float32)
    return s


def test_entries_reaching_one_to_four_quadrants_and_none():
    """Quadrant reach: every reach count 1..4 occurs, some list entry reaches no pixel at all (its record is zero), and the ragged
    right / bottom tiles -- whole quadrants outside the image -- carry entries; gradients against the oracle."""
    dev = _dev()
    s = _reach_scene()
    o = _oracle(s)
    counts = np.concatenate([_quadrant_reach(o, t) for t in range(GX * GY)])
    for c in range(5):
        assert (counts == c).any(), f"no list entry reaches {c} quadrants: {np.bincount(counts, minlength=5)}"
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert tl.reshape(GY, GX)[:, GX - 1].sum() > 0 and tl.reshape(GY, GX)[GY - 1].sum() > 0, "the ragged tiles are empty"
    _against_oracle(s, o, dev)


@pytest.mark.parametrize("regime", ["saturating", "faint"])
@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 255, 256, 257, 513])
def test_batch_and_segment_boundaries(n, regime):
    """A hot tile whose list length sits on the 64-entry batch and 256-entry segment boundaries, on the many-tile frame: binning,
    image and every gradient element against the oracle (fuzz_parity.check and its bars)."""
    _dev()
    fp = _fuzz()
    s = fp.aux_regime(fp.crafted(n, n, W=W, H=H), n, regime, n)
    R, mx = fp.check(s, f"tile-wave crafted {n} {regime}")
    assert mx >= n


UNEQUAL_BLOCKERS = 48


def _unequal_scene(n=300):
    """crafted(n) plus 48 opaque splats in front of it, centred in quadrant 0 of the hot tile (pixels 16..23): every pixel of that
    quadrant terminates among them, the far pixels of the other three quadrants never see them and walk the list to its end."""
    fp = _fuzz()
    s = fp.crafted(n, 77, W=W, H=H)
    fx = 1.2 * W
    k = UNEQUAL_BLOCKERS
    z = np.linspace(1.2, 1.7, k).astype(np.float32)
    px = np.full(k, 19.5); py = np.full(k, 19.5)
    means = np.stack([(px - W / 2) / fx * z, (py - H / 2) / fx * z, z], 1).astype(np.float32)
    sig = (3.0 * z / fx).astype(np.float32)                     # alpha 0.27 at the quadrant's corners, < 1/255 seven pixels out
    s = dict(s)
    s["means3D"] = np.concatenate([means, s["means3D"]]).astype(np.float32)
    s["scales"] = np.concatenate([np.stack([sig, sig, sig], 1), s["scales"]]).astype(np.float32)
    s["rotations"] = np.concatenate([np.tile(np.array([[1, 0, 0, 0]], np.float32), (k, 1)), s["rotations"]]).astype(np.float32)
    s["opacities"] = np.concatenate([np.full((k, 1), 0.99, np.float32), s["opacities"]]).astype(np.float32)
    s["shs"] = np.concatenate([np.zeros((k,) + s["shs"].shape[1:], np.float32), s["shs"]]).astype(np.float32)
    return s


def test_quadrants_of_one_tile_with_unequal_depths():
    """Unequal quadrants: quadrant 0 of the hot tile saturates behind the opaque splats, so its deepest contributor is far in front
    of the other quadrants' -- per-quadrant limits differ inside one wave."""
    dev = _dev()
    s = _unequal_scene()
    o = _oracle(s)
    hot = GX + 1
    nc = o["n_contrib"][16:32, 16:32].reshape(2, 8, 2, 8).max(axis=(1, 3)).reshape(4)
    n = int(o["ranges"][hot, 1]) - int(o["ranges"][hot, 0])
    assert n > 256 and nc[0] <= UNEQUAL_BLOCKERS and min(nc[1:]) > 256, (n, nc)
    _against_oracle(s, o, dev)


def _engine_case(K, dev, N=3000, deg=1):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    s = _reach_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], K, 0).copy(); views[:, 3, 0] = 0.05 * np.arange(K)
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])

    def settings(vm, pm, cp):
        return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                             scale_modifier=1.0, viewmatrix=vm, projmatrix=pm, sh_degree=deg, campos=cp,
                                             prefiltered=False, debug=False)
    ins = [t(s[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    dL = t(np.random.RandomState(1).normal(0, 1, (K, 3, H, W)).astype(np.float32))
    return s, settings, ins, dL, t(views), t(projs), t(cps)


def test_two_cameras_in_one_launch_equal_two_single_calls_bit_for_bit():
    """K against single calls: K = 2 in one launch == two single calls, the second with accumulate."""
    from sings_amd.engine import RasterEngine, RasterFramesEngine
    dev = _dev()
    K, N = 2, 3000
    s, settings, ins, dL, views, projs, cps = _engine_case(K, dev)
    cap = 12 * N
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
    eng.forward(*ins, sync_num_rendered=True)
    eng.backward(*ins, dL)
    torch.cuda.synchronize()
    for f in range(K):
        assert torch.equal(eng.color[f], per[f][0]) and torch.equal(eng.d_means2D[f], per[f][1]), f
    assert torch.equal(eng.grad_flat, ref.grad_flat)


def test_two_runs_are_bitwise_equal_and_the_last_workgroup_has_idle_waves():
    """Reproducibility, and idle waves: the work-item count of this frame is no multiple of 4 (one item per tile, 4 225 tiles, no
    list longer than a segment), so the last workgroup's waves past it return at once."""
    from sings_amd.inspect_ws import forward_with_state
    dev = _dev()
    fp = _fuzz()
    s = _reach_scene()
    t = lambda a: torch.from_numpy(a).to(dev)
    st = forward_with_state(fp.settings(s), t(s["means3D"]), t(s["opacities"]), shs=t(s["shs"]), scales=t(s["scales"]), rotations=t(s["rotations"]))
    header = st["binning"][st["layout"].bin_header:st["layout"].bin_header + 32].view(torch.int32)
    assert int(header[5]) % 4 != 0, int(header[5])
    dL = s["dL_dimage"].copy()
    a, b = _hip_grads(s, dL, dev), _hip_grads(s, dL, dev)
    for name in a:
        assert torch.equal(a[name], b[name]), name
        assert bool(torch.isfinite(a[name]).all()), name


def test_colour_gradients_with_the_maps_requested_equal_the_plain_call():
    """Aux against plain: with the depth / alpha maps requested and no loss on them, the aux kernel's gradients are the plain
    kernel's bits (the same order of summation in both)."""
    dev = _dev()
    fp = _fuzz()
    s = _reach_scene()
    dL = s["dL_dimage"].copy()
    zero = np.zeros((H, W), np.float32)
    x = fp.aux_abi(s, dL, zero, zero)
    plain = _hip_grads(s, dL, dev)
    for name, key in (("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacities"), ("dL_dscales", "scales"), ("dL_drots", "rotations"), ("dL_dsh", "shs")):
        assert torch.equal(x["grads"][key].reshape(plain[name].shape), plain[name]), name


def test_a_capacity_overflow_gives_zero_gradients():
    """Overflow: a frame whose pairs exceed the workspace renders the background and its backward leaves zero gradients."""
    from sings_amd.engine import RasterEngine
    dev = _dev()
    N = 3000
    s, settings, ins, dL, views, projs, cps = _engine_case(1, dev)
    e = RasterEngine(N, W, H, 4, dev, 4096)                      # the scene has ~12 k pairs
    e.set_camera(settings(views[0], projs[0], cps[0]))
    R = e.forward(*ins, sync_num_rendered=True)
    assert R > 4096
    e.grad_flat.fill_(float("nan"))
    e.backward(*ins, dL[0])
    torch.cuda.synchronize()
    assert bool((e.grad_flat == 0).all())
