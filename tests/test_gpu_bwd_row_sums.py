"""The dense backward composite files an entry's nine (aux: ten) sums in the entry's own staged row of LDS (sings_amd/csrc/sg_render_bwd.inc:
floats 0-8 (9) of the 16-float row; the opacity the record store needs is staged once more in float 11).  What can go wrong with that
placement: a record built from a row that holds another entry's, an earlier batch's or merely staged floats, from the sum that
overwrote the opacity, or from the depth that the tenth sum overwrote.

One scene on the 1034 x 1030 frame of tests/test_gpu_bwd_tile_wave.py (65 x 65 = 4 225 tiles, one work item per tile: no multiple
of 4; the right column of tiles has 10 of its 16 pixel columns inside the image, the bottom row 6 of its 16 rows), made of crafted
tiles only:
  * STACKS: tiles whose list has exactly 64, 65, 128 and 129 entries, every one of them filed (a full batch of rows, and rows staged
    again behind a record store), also in the right column (64) and the bottom row (65).  From entry to entry the opacity changes by
    a factor of up to five and the conic between four orientations of a 6 : 1 ellipse.
  * ALTERNATE: two tiles of 132 entries in which filed and unfiled entries alternate -- the unfiled ones in the lee of twelve opaque
    blockers ("hidden"), or too faint to reach 1/255 anywhere ("faint": an empty mask).  Their records, hence their gradient rows,
    are zeros although their rows hold staged floats or an earlier batch's sums.
Gradients against oracle/raster_oracle at the bar of tests/test_gpu_raster.py (`_grad_close`: rtol 2e-4 + 2e-6 max|g|, pixels
within 2e-5 of a hard threshold carry no loss).  tests/test_bwd_row_sums_scenes_host.py asserts from the oracle alone that the scene
holds these cases."""
import numpy as np
import pytest
import torch

import test_gpu_bwd_first_quadrant as fq
import test_gpu_bwd_tile_wave as tw
from oracle import raster_oracle as ro
from sings_amd.scene import synthetic_scene

pytestmark = pytest.mark.gpu

W, H, GX, GY, BORDER = tw.W, tw.H, tw.GX, tw.GY, tw.BORDER
FX = 1.2 * W

# (tile x, tile y, entries, sigma of the long axis in pixels, centres' local x, centres' local y): a splat's 3-sigma box stays
# inside its tile (sigma 1.5: radius 5; 1.2: radius 4), and its centre is a pixel inside the image
STACKS = ((10, 10, 64, 1.5, (6, 7, 8, 9, 10), (6, 7, 8, 9, 10)),
          (14, 10, 65, 1.5, (6, 7, 8, 9, 10), (6, 7, 8, 9, 10)),
          (10, 14, 128, 1.5, (6, 7, 8, 9, 10), (6, 7, 8, 9, 10)),
          (14, 14, 129, 1.5, (6, 7, 8, 9, 10), (6, 7, 8, 9, 10)),
          (GX - 1, 20, 64, 1.5, (6, 7, 8, 9), (6, 7, 8, 9, 10)),        # right column: pixel columns 0..9 are inside
          (20, GY - 1, 65, 1.2, (5, 6, 7, 8, 9, 10), (5,)))             # bottom row: pixel rows 0..5 are inside
SHORT = 0.1                                                             # sigma of the short axis (the 0.3 px^2 filter dominates it)
# (tile x, tile y, kind): behind BLOCKERS opaque splats ("hidden") or from the front of the list ("faint"), PAIRS times (unfiled, filed)
ALTERNATE = ((30, 10, "hidden"), (34, 10, "faint"))
BLOCKERS, PAIRS = 12, 60
ALT_FRONT = {"hidden": BLOCKERS, "faint": 12}                            # entries in front of the alternating pairs (faint: 12 more filed ones)
R2 = float(np.sqrt(0.5))
ROT = ((1.0, 0.0, 0.0, 0.0), (R2, 0.0, 0.0, R2), (np.cos(np.pi / 8), 0.0, 0.0, np.sin(np.pi / 8)), (np.cos(np.pi / 8), 0.0, 0.0, -np.sin(np.pi / 8)))


def _splat(px, py, z, s_long, s_short, rot, opacity):
    """A Gaussian whose centre projects to pixel (px, py): sigma `s_long` along the image x axis turned by quaternion `rot` about
    the view axis (the camera looks down +z with the identity view matrix), `s_short` across."""
    mean = [(px + 0.5 - W / 2) / FX * z, (py + 0.5 - H / 2) / FX * z, z]
    return mean, [s_long * z / FX, s_short * z / FX, s_short * z / FX], list(rot), opacity


def stack(tx, ty, n, s_long, xs, ys):
    """`n` splats in tile (tx, ty) alone, back to front by index.  Neighbours differ in orientation (along x, along y, the two
    diagonals), in opacity (0.025 .. 0.133, never by less than 0.009) and in position."""
    out = []
    for i in range(n):
        out.append(_splat(16 * tx + xs[(3 * i) % len(xs)], 16 * ty + ys[(i // 2) % len(ys)], 1.5 + 1e-3 * i, s_long, SHORT, ROT[i % 4],
                          0.025 + 0.009 * ((7 * i) % 13)))
    return out


def alternate(tx, ty, kind):
    """ALT_FRONT[kind] entries, then PAIRS x (unfiled, filed).  The filed ones are a column of small ellipses over local pixels
    x 10..12; "hidden": twelve opaque blobs over local pixel (4, 4) and the unfiled entries sub-pixel splats in their lee, every
    pixel they reach terminated; "faint": the unfiled entries have opacity 0.002 < 1/255 and reach no pixel at all."""
    X0, Y0 = 16 * tx, 16 * ty
    out = []
    for i in range(ALT_FRONT[kind]):
        if kind == "hidden":
            out.append(_splat(X0 + 4, Y0 + 4, 1.2 + 1e-3 * i, 2.0, 2.0, ROT[0], 0.99))
        else:
            out.append(_splat(X0 + 10 + i % 3, Y0 + 5 + i % 6, 1.2 + 1e-3 * i, 1.0, 0.25, ROT[i % 2], 0.05 + 0.01 * (i % 5)))
    for j in range(PAIRS):
        z = 1.5 + 2e-3 * j
        if kind == "hidden":
            out.append(_splat(X0 + 4, Y0 + 4, z, 0.25, 0.25, ROT[0], 0.3))
        else:
            out.append(_splat(X0 + 8, Y0 + 8, z, 0.5, 0.5, ROT[0], 0.002))
        out.append(_splat(X0 + 10 + j % 3, Y0 + 5 + j % 6, z + 1e-3, 1.0, 0.25, ROT[j % 2], 0.03 + 0.011 * ((5 * j) % 9)))
    return out


ALT_LEN = {k: ALT_FRONT[k] + 2 * PAIRS for k in ALT_FRONT}


def layout():
    """-> (splats, first Gaussian id per STACKS tile, first id per ALTERNATE tile): ids are list order within each tile."""
    splats, s0, a0 = [], [], []
    for st in STACKS:
        s0.append(len(splats)); splats += stack(*st)
    for al in ALTERNATE:
        a0.append(len(splats)); splats += alternate(*al)
    return splats, s0, a0


def unfiled_ids():
    """Gaussian ids of the hidden and the faint entries."""
    _, _, a0 = layout()
    return [a0[i] + ALT_FRONT[kind] + 2 * j for i, (_, _, kind) in enumerate(ALTERNATE) for j in range(PAIRS)]


def rows_scene():
    splats, _, _ = layout()
    k = len(splats)
    rs = np.random.RandomState(21)
    s = synthetic_scene(1, W, H, 1, 9)                                  # the camera, the background and dL/dimage
    s["N"] = k
    s["means3D"] = np.array([m for m, _, _, _ in splats], np.float32)
    s["scales"] = np.array([c for _, c, _, _ in splats], np.float32)
    s["rotations"] = np.array([r for _, _, r, _ in splats], np.float32)
    s["opacities"] = np.array([[o] for _, _, _, o in splats], np.float32)
    s["shs"] = rs.normal(0, 0.5, (k,) + s["shs"].shape[1:]).astype(np.float32)
    return s


def neighbours_differ(o, g, tile, rtol=2e-4, atol=2e-6):
    """In `tile`'s list, every entry's dL/dopacity differs from the next entry's by more than the bar of `_grad_close` (so a record
    read from the neighbouring row cannot pass).  -> the smallest difference over its bar."""
    lo, hi = int(o["ranges"][tile, 0]), int(o["ranges"][tile, 1])
    ids = o["point_list"][lo:hi].astype(np.int64)
    v = g["dL_dopacity"].astype(np.float64).reshape(-1)[ids]
    scale = np.abs(g["dL_dopacity"]).max()
    d = np.abs(v[1:] - v[:-1]); bar = rtol * np.maximum(np.abs(v[1:]), np.abs(v[:-1])) + atol * scale
    return float((d / bar).min())


_ORACLE = []


def oracle():
    """(scene, oracle forward, dL/dimage with the borderline pixels cleared, oracle gradients): computed once, never changed."""
    if not _ORACLE:
        s = rows_scene()
        o = tw._oracle(s)
        dL = s["dL_dimage"].copy(); dL[:, o["margin"] < BORDER] = 0
        _ORACLE.append((s, o, dL, ro.backward(o, dL)))
    return _ORACLE[0]


_PLAIN = []


def _plain(dev):
    if not _PLAIN:
        s, _, dL, _ = oracle()
        _PLAIN.append({k: v.cpu().numpy() for k, v in tw._hip_grads(s, dL, dev).items()})
    return _PLAIN[0]


def test_full_batches_of_filed_rows_with_opacity_and_conic_changing_from_entry_to_entry():
    """Lists of 64, 65, 128 and 129 entries, all filed: every gradient against the oracle; and, from the oracle, neighbouring
    entries' dL/dopacity differ by more than the bar."""
    dev = tw._dev()
    _, o, _, g = oracle()
    for tx, ty, n, *_ in STACKS:
        ratio = neighbours_differ(o, g, ty * GX + tx)
        print(f"tile ({tx}, {ty}), {n} entries: neighbouring dL/dopacity differ by at least {ratio:.1f} bars")
        assert ratio > 1.0, (tx, ty, ratio)
    got = _plain(dev)
    for name, a in got.items():
        print(name, "worst abs", np.abs(a.reshape(g[name].shape) - g[name]).max(), "scale", np.abs(g[name]).max())
        tw._grad_close(name, a.reshape(g[name].shape), g[name])


def test_unfiled_entries_between_filed_ones_get_zero_records():
    """The hidden and the faint entries: every gradient row of theirs is zero (their rows hold staged floats or an earlier batch's
    sums), and the filed entries between them agree with the oracle (the whole arrays, above)."""
    dev = tw._dev()
    _, _, _, g = oracle()
    got = _plain(dev)
    ids = unfiled_ids()
    for name, a in got.items():
        a = a.reshape(g[name].shape)
        assert not np.abs(g[name][ids]).any(), name
        assert not np.abs(a[ids]).any(), (name, np.abs(a[ids]).max())
        tw._grad_close(name, a, g[name])


def test_two_cameras_in_one_launch_equal_two_single_calls_and_a_second_run_bit_for_bit():
    """K = 2 through the frames entry points == two single calls, the second with accumulate; the K = 2 launch twice: the same bits."""
    from sings_amd.engine import RasterEngine, RasterFramesEngine
    from sings_amd.rasterizer import GaussianRasterizationSettings
    dev = tw._dev()
    K = 2
    s = rows_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], K, 0).copy(); views[:, 3, 0] = 0.0007 * np.arange(K)      # half a pixel at z = 1.5
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])
    views, projs, cps = t(views), t(projs), t(cps)

    def settings(vm, pm, cp):
        return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                             scale_modifier=1.0, viewmatrix=vm, projmatrix=pm, sh_degree=1, campos=cp,
                                             prefiltered=False, debug=False)
    ins = [t(s[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    dL = t(np.random.RandomState(1).normal(0, 1, (K, 3, H, W)).astype(np.float32))
    N = s["means3D"].shape[0]
    cap = 1 << 16
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


def test_the_depth_alpha_twin_without_map_adjoints_leaves_the_plain_kernels_bits():
    """sg_render_bwd_aux_kernel with dL/ddepth = dL/dalpha = 0: the colour-path gradients of the plain call, bit for bit."""
    dev = tw._dev()
    fp = tw._fuzz()
    s, _, dL, _ = oracle()
    zero = np.zeros((H, W), np.float32)
    x = fp.aux_abi(s, dL, zero, zero)
    plain = _plain(dev)
    for gname, key in fq.AUX_KEYS:
        assert np.array_equal(x["grads"][key].cpu().numpy().reshape(plain[gname].shape), plain[gname]), gname


def test_the_depth_alpha_twin_with_map_adjoints_against_the_oracle():
    """The tenth sum (dL/dz, filed over the staged depth): a loss on colour, depth and alpha; every gradient against the oracle's
    colour pass + (z, 1) pass (oracle/raster_aux.py), and zero rows for the unfiled entries."""
    from oracle.raster_aux import oracle_pair, reference_grads
    tw._dev()
    fp = tw._fuzz()
    s, o, dL, _ = oracle()
    o2, oa = oracle_pair(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"], s["tanfovy"],
                         s["bg"], s["scales"], s["rotations"], s["shs"], s["sh_degree"])
    rng = np.random.RandomState(11)
    gD = rng.normal(0, 1, (H, W)).astype(np.float32); gA = rng.normal(0, 1, (H, W)).astype(np.float32)
    border = (o["margin"] < BORDER) | (oa["margin"] < BORDER)
    gD[border] = 0; gA[border] = 0
    dLc = dL.copy(); dLc[:, border] = 0
    ref = reference_grads(o2, oa, dLc, gD, gA, s["viewmatrix"])
    x = fp.aux_abi(s, dLc, gD, gA)
    assert float(np.abs(ref["means3D"]).max()) > 0
    ids = unfiled_ids()
    for key in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        a = x["grads"][key].cpu().numpy(); b = np.asarray(ref[key])
        a = a.reshape(b.shape)
        print(key, "worst abs", np.abs(a - b).max(), "scale", np.abs(b).max())
        assert not np.abs(a[ids]).any(), (key, np.abs(a[ids]).max())
        tw._grad_close(key, a, b)
