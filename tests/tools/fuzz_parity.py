"""Randomised HIP-vs-oracle parity sweep (GPU box): python tests/tools/fuzz_parity.py [n_cases]
Random scene sizes / SH degrees / densities / opacity scales, plus crafted tiles whose list length sits exactly on the
internal boundaries (see __main__).  FUZZ_SEED selects the random sequence.  Checks per case: binning bit-exact, RGB <= 2e-5
off borderline pixels, gradients within tolerance.  Exit code 1 on the first failure (prints the case)."""
import ctypes as C
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import raster_oracle as ro
from sings_amd.scene import synthetic_scene
from sings_amd.inspect_ws import forward_with_state
from diff_gaussian_rasterization import GaussianRasterizer
from sings_amd.rasterizer import GaussianRasterizationSettings

dev = torch.device("cuda:0")
BORDER = 2e-5


def settings(s):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return GaussianRasterizationSettings(image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                         scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]),
                                         sh_degree=s["sh_degree"], campos=t(s["campos"]), prefiltered=False, debug=False)


def check(s, tag):
    o = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"], s["tanfovy"],
                   s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=s["sh_degree"])
    rs = settings(s)
    t = lambda a: torch.from_numpy(a).to(dev)
    st = forward_with_state(rs, t(s["means3D"]), t(s["opacities"]), shs=t(s["shs"]), scales=t(s["scales"]), rotations=t(s["rotations"]))
    assert st["R"] == o["R"], (tag, "R", st["R"], o["R"])
    assert np.array_equal(st["ranges"].cpu().numpy().astype(np.uint32), o["ranges"]), (tag, "ranges")
    assert np.array_equal(st["point_list"].cpu().numpy().astype(np.uint32), o["point_list"]), (tag, "point_list")
    assert np.array_equal(st["radii"].cpu().numpy(), o["radii"]), (tag, "radii")
    border = o["margin"] < BORDER
    diff = np.abs(st["color"].cpu().numpy() - o["color"]).max(0)
    assert diff[~border].max() <= 2e-5, (tag, "rgb", diff[~border].max())
    dLn = s["dL_dimage"].copy(); dLn[:, border] = 0
    g = ro.backward(o, dLn)
    req = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)
    m, op, sh, sc, rt = req(s["means3D"]), req(s["opacities"]), req(s["shs"]), req(s["scales"]), req(s["rotations"])
    color, _ = GaussianRasterizer(rs)(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=op, shs=sh, scales=sc, rotations=rt)
    color.backward(torch.from_numpy(dLn).to(dev))
    for name, a, b in (("means3D", m.grad, g["dL_dmeans3D"]), ("opacity", op.grad, g["dL_dopacity"]), ("scales", sc.grad, g["dL_dscales"]),
                       ("rots", rt.grad, g["dL_drots"]), ("sh", sh.grad, g["dL_dsh"])):
        a = a.cpu().numpy().reshape(b.shape).astype(np.float64); b = b.astype(np.float64)
        # EVERY element, like tests/test_gpu_raster.py::_grad_close (round 3 let 1e-4 of the elements miss: nothing needed it --
        # borderline pixels carry no loss on either side); rtol / atol are those of the segmented-list tests there: the crafted
        # lists are thousands of entries deep, and a depth segment's colour-behind comes from forward sums (~1e-6 per pixel term)
        scale = np.abs(b).max() + 1e-30
        bad = np.abs(a - b) > 1e-3 * np.abs(b) + 6e-6 * scale
        assert not bad.any(), (tag, name, int(bad.sum()), np.abs(a - b).max(), scale)
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    # direct binning (include/sings_hip.h: SG_FLAG_SHORT_LISTS on images of many tiles, SG_FLAG_LONG_ROWS on few): the same lists, ranges,
    # keys and image bit for bit whenever the promise holds, a refusal (background, NUM_RENDERED_LONG_LIST) when it does not
    from sings_amd import _lib
    gx, gy = (s["W"] + 15) // 16, (s["H"] + 15) // 16
    few = ((gx + 3) // 4) * ((gy + 3) // 4) * 16 <= 4096
    flags = (_lib.FLAG_LONG_ROWS if few else _lib.FLAG_SHORT_LISTS)
    holds = int(tl.max()) <= (16384 if few else 1024)
    sd = forward_with_state(rs, t(s["means3D"]), t(s["opacities"]), shs=t(s["shs"]), scales=t(s["scales"]), rotations=t(s["rotations"]), flags=flags)
    if holds:
        assert sd["R"] == st["R"], (tag, "direct R", sd["R"], st["R"])
        for name in ("ranges", "point_list", "point_keys", "color", "final_T", "n_contrib"):
            assert torch.equal(sd[name], st[name]), (tag, "direct binning", name)
    else:
        assert sd["R"] == _lib.NUM_RENDERED_LONG_LIST, (tag, "direct binning should have refused", sd["R"])
        assert torch.equal(sd["color"], t(s["bg"])[:, None, None].expand_as(sd["color"])), (tag, "refused frame is not the background")
    return int(o["R"]), int(tl.max())


def aux_abi(s, dLc, gD, gA, flags=0, capacity=None, pad=0, sentinel=0.0, geometry=None, colors=None):
    """One forward + backward of the depth / alpha maps through the C ABI (sg_rasterize_forward_aux / _backward_aux), as
    _RasterizeGaussians with return_aux runs them but with the caller's SG_FLAG_* promise.  `pad` > 0 places out_depth / out_alpha
    and the dL_ddepth / dL_dalpha planes `pad` floats into buffers `pad` floats longer than [H,W] on both sides, filled with `sentinel`
    (gD / gA given as [H,W]).  `geometry`: None (scales + rotations) or a cov3D_precomp array; `colors`: colors_precomp instead of
    the SH.  -> dict of tensors (the padded buffers whole: depth_buf, alpha_buf), R = NUM_RENDERED_LONG_LIST on a refusal."""
    from sings_amd import _lib
    from sings_amd._marshal import _settings_struct, _ptr
    lib = _lib.load()
    rs = settings(s)
    H, W = s["H"], s["W"]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    means3D, op = t(s["means3D"]), t(s["opacities"])
    shs = None if colors is not None else t(s["shs"])
    col = t(colors)
    sc, rt = (None, None) if geometry is not None else (t(s["scales"]), t(s["rotations"]))
    cov = t(geometry)
    P = int(means3D.shape[0]); M = int(shs.shape[1]) if shs is not None else 0
    keep = []
    st = _settings_struct(rs, dev, M, keep)
    st.flags = int(flags)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    cap = capacity or max(8 * P + gx * gy, 1 << 16)
    HW = H * W
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    plane = lambda fill: torch.full((HW + 2 * pad,), float(fill), dtype=torch.float32, device=dev)
    while True:
        L = _lib.layout(P, W, H, cap)
        geom = torch.zeros(L.geom_bytes, dtype=torch.uint8, device=dev)
        binning = torch.zeros(L.bin_bytes, dtype=torch.uint8, device=dev)
        img = torch.zeros(L.img_bytes, dtype=torch.uint8, device=dev)
        aux = torch.zeros(_lib.aux_layout(P, W, H, cap), dtype=torch.uint8, device=dev)
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        dbuf, abuf = plane(sentinel), plane(sentinel)
        nr = C.c_int64(0)
        _lib.check(lib.sg_rasterize_forward_aux(
            C.byref(st), P, _ptr(means3D), _ptr(shs), _ptr(col), _ptr(op), _ptr(sc), _ptr(rt), _ptr(cov), _ptr(geom),
            _ptr(binning), cap, _ptr(img), _ptr(color), _ptr(radii), 1, C.byref(nr), _ptr(aux), _ptr(dbuf[pad:]), _ptr(abuf[pad:]),
            stream), "forward (aux)")
        R = int(nr.value)
        if R < 0:
            torch.cuda.synchronize()
            return dict(R=R, color=color, depth_buf=dbuf, alpha_buf=abuf)
        if R <= cap:
            break
        cap = R + 1024
    gDb, gAb = plane(sentinel), plane(sentinel)
    gDb[pad:pad + HW] = t(gD).reshape(-1); gAb[pad:pad + HW] = t(gA).reshape(-1)
    e = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    g = dict(means3D=e(P, 3), means2D=e(P, 3), opacities=e(P, 1), shs=e(P, M, 3) if shs is not None else None,
             colors=e(P, 3) if col is not None else None, scales=e(P, 3) if sc is not None else None,
             rotations=e(P, 4) if sc is not None else None, cov3D=e(P, 6) if cov is not None else None)
    bwd = torch.empty(int(L.bwd_bytes), dtype=torch.uint8, device=dev)
    _lib.check(lib.sg_rasterize_backward_aux(
        C.byref(st), P, _ptr(means3D), _ptr(shs), _ptr(col), _ptr(op), _ptr(sc), _ptr(rt), _ptr(cov), _ptr(radii), _ptr(geom),
        _ptr(binning), cap, _ptr(img), _ptr(bwd), _ptr(t(dLc)), _ptr(g["means3D"]), _ptr(g["means2D"]), _ptr(g["shs"]),
        _ptr(g["colors"]), _ptr(g["opacities"]), _ptr(g["scales"]), _ptr(g["rotations"]), _ptr(g["cov3D"]), _ptr(aux),
        _ptr(gDb[pad:]), _ptr(gAb[pad:]), stream), "backward (aux)")
    torch.cuda.synchronize()
    T = gx * gy
    seg = lambda buf, off, n, dt: buf[off:off + n * torch.empty(0, dtype=dt).element_size()].view(dt)
    return dict(R=R, color=color, radii=radii, depth=dbuf[pad:pad + HW].view(H, W), alpha=abuf[pad:pad + HW].view(H, W),
                depth_buf=dbuf, alpha_buf=abuf, grads={k: v for k, v in g.items() if v is not None},
                ranges=seg(binning, L.bin_ranges, T * 2, torch.int32).view(T, 2),
                point_list=seg(binning, L.bin_point_list, R, torch.int32),
                final_T=seg(img, L.img_final_T, HW, torch.float32).view(H, W),
                n_contrib=seg(img, L.img_n_contrib, HW, torch.int32).view(H, W))


def grads_close(tag, got, ref, rtol=1e-3, atol=6e-6):
    """EVERY element of every gradient the reference has, at the tolerances of check() above."""
    for name, b in ref.items():
        a = got[name].detach().cpu().numpy().astype(np.float64).reshape(np.shape(b)); b = np.asarray(b, np.float64)
        assert np.isfinite(a).all(), (tag, name, "non-finite")
        scale = np.abs(b).max() + 1e-30
        bad = np.abs(a - b) > rtol * np.abs(b) + atol * scale
        assert not bad.any(), (tag, name, int(bad.sum()), np.abs(a - b).max(), scale)


def aux_loss_seeds(s, strict, seed):
    """A loss on colour, depth and alpha; pixels within BORDER of a hard threshold of the oracle carry none."""
    rng = np.random.RandomState(seed)
    H, W = s["H"], s["W"]
    dLc = s["dL_dimage"][:, :H, :W].copy()
    gD = rng.normal(0, 1, (H, W)).astype(np.float32); gA = rng.normal(0, 1, (H, W)).astype(np.float32)
    dLc[:, ~strict] = 0; gD[~strict] = 0; gA[~strict] = 0
    return dLc, gD, gA


def check_aux(s, tag):
    """check() for the depth and alpha maps: the aux forward's binning, colour and radii are the plain forward's bits; depth /
    alpha <= 1e-5 off borderline pixels (alpha absolute, depth relative to max |z|) against oracle/raster_aux.py; every gradient
    element under a loss on colour, depth and alpha at check()'s tolerances; and with the direct-binning promise of the regime
    (SG_FLAG_LONG_ROWS on few tiles, SG_FLAG_SHORT_LISTS on many) the same bits, or a refusal where the promise does not hold."""
    from oracle.raster_aux import oracle_pair, reference_grads
    from sings_amd import _lib
    o, oa = oracle_pair(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                        s["tanfovy"], s["bg"], s["scales"], s["rotations"], s["shs"], s["sh_degree"])
    rs = settings(s)
    t = lambda a: torch.from_numpy(a).to(dev)
    st = forward_with_state(rs, t(s["means3D"]), t(s["opacities"]), shs=t(s["shs"]), scales=t(s["scales"]), rotations=t(s["rotations"]))
    strict = o["margin"] >= BORDER
    dLc, gD, gA = aux_loss_seeds(s, strict, 11)
    x = aux_abi(s, dLc, gD, gA)
    assert x["R"] == st["R"] == o["R"], (tag, "R", x["R"], st["R"], o["R"])
    for name in ("ranges", "point_list", "final_T", "n_contrib", "color", "radii"):
        assert torch.equal(x[name], st[name]), (tag, "aux forward vs plain forward", name)
    vis = o["radii"] > 0
    zmax = np.abs(o["depths"][vis]).max()
    a, d = x["alpha"].cpu().numpy(), x["depth"].cpu().numpy()
    assert np.abs(a - oa["color"][1])[strict].max() <= 1e-5, (tag, "alpha", np.abs(a - oa["color"][1])[strict].max())
    assert np.abs(d - oa["color"][0])[strict].max() <= 1e-5 * zmax, (tag, "depth", np.abs(d - oa["color"][0])[strict].max(), zmax)
    ref = reference_grads(o, oa, dLc, gD, gA, s["viewmatrix"])
    grads_close(tag, x["grads"], ref)
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    gx, gy = (s["W"] + 15) // 16, (s["H"] + 15) // 16
    few = ((gx + 3) // 4) * ((gy + 3) // 4) * 16 <= 4096
    holds = int(tl.max()) <= (16384 if few else 1024)
    y = aux_abi(s, dLc, gD, gA, flags=_lib.FLAG_LONG_ROWS if few else _lib.FLAG_SHORT_LISTS)
    if holds:
        assert y["R"] == x["R"], (tag, "direct R", y["R"], x["R"])
        for name in ("ranges", "point_list", "final_T", "n_contrib", "color", "radii", "depth", "alpha"):
            assert torch.equal(y[name], x[name]), (tag, "direct binning", name)
        for name in x["grads"]:
            assert torch.equal(y["grads"][name], x["grads"][name]), (tag, "direct binning gradient", name)
    else:
        assert y["R"] == _lib.NUM_RENDERED_LONG_LIST, (tag, "direct binning should have refused", y["R"])
    return int(o["R"]), int(tl.max()), o


def aux_regime(s, n, regime, seed):
    """Opacities of the n crafted Gaussians for the AUX boundary cases: "saturating" (x3: pixels of the hot tile terminate at
    entries spread over several depth segments), "faint" (all but 150 below 1/255 and skipped: no pixel terminates, every segment
    is walked to the end, its checkpoint carrying a few blended entries), None (crafted()'s own 0.01..0.2)."""
    if regime is None:
        return s
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


def crafted(n_in_tile, seed, depths=None, W=64, H=48):
    """n small Gaussians whose 3-sigma squares all lie inside ONE 16x16 tile of a 64x48 image -> that tile's list has
    exactly n entries (plus a sprinkle elsewhere).  `depths`: the view-space z of the n Gaussians (default: uniform in 2..10).
    W, H: a larger image puts the same tile (1,1) into a frame of many tiles (the other pair of composite kernels)."""
    s = synthetic_scene(200, W, H, 1, seed)
    rs = np.random.RandomState(seed)
    N = n_in_tile + 200
    fx = 1.2 * W
    z = rs.uniform(2, 10, n_in_tile).astype(np.float32) if depths is None else np.asarray(depths, np.float32)
    px = rs.uniform(22, 26, n_in_tile); py = rs.uniform(22, 26, n_in_tile)           # tile (1,1) spans 16..31
    x = ((px - W / 2) / fx * z).astype(np.float32); y = ((py - H / 2) / fx * z).astype(np.float32)
    means = np.concatenate([np.stack([x, y, z], 1), s["means3D"]]).astype(np.float32)
    sig = (0.35 * z / fx).astype(np.float32)                                          # sigma 0.35 px -> radius ceil(3 sqrt(.35^2+.3)) = 3
    scales = np.concatenate([np.stack([sig, sig, sig], 1), s["scales"]]).astype(np.float32)
    rot = np.concatenate([np.tile(np.array([[1, 0, 0, 0]], np.float32), (n_in_tile, 1)), s["rotations"]])
    op = np.concatenate([rs.uniform(0.01, 0.2, (n_in_tile, 1)).astype(np.float32), s["opacities"]])
    shs = np.concatenate([rs.normal(0, 0.5, (n_in_tile, 16, 3)).astype(np.float32), s["shs"]])
    out = dict(s); out.update(means3D=means, scales=scales, rotations=rot.astype(np.float32), opacities=op, shs=shs)
    return out


def clustered_depths(seed):
    """Depth distribution that walks the long-list bucket sort (sg_binning.hip) through every level: 1 500 keys with IDENTICAL
    depth bits (a plane facing the camera: level 0 puts them in one bucket, level 1 splits them by Gaussian id), 3 000 keys on
    two ADJACENT float codes (level 1 cannot split a code's 1 500 keys any further: ordered by counting), 1 200 spread out,
    and two outliers that stretch the key range."""
    rs = np.random.RandomState(seed)
    a = np.float32(7.0); b = np.nextafter(a, np.float32(8.0))
    z = np.concatenate([np.full(1500, 5.0, np.float32), np.where(rs.rand(3000) < 0.5, a, b).astype(np.float32),
                        rs.uniform(3.0, 9.0, 1200).astype(np.float32), np.array([2.0, 9.9], np.float32)])
    return z[rs.permutation(z.size)]


CRAFTED_LENGTHS = (127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 12287, 12288, 12289, 20000)


def random_case(rs, large=False):
    """One random scene of the sweep from the generator state `rs` -> (scene, tag)."""
    if large:                      # frames of more than 4096 tiles take the other pair of composite kernels
        W, H = int(rs.choice([1100, 1280, 1600])), int(rs.choice([1000, 1080]))
        N = int(rs.choice([3000, 30000])); deg = int(rs.randint(0, 4)); seed = int(rs.randint(1 << 30))
        s = synthetic_scene(N, W, H, deg, seed)
        s["scales"] = (s["scales"] * rs.choice([1.0, 3.0])).astype(np.float32)
        return s, f"large: N={N} {W}x{H} deg={deg} seed={seed}"
    W, H = int(rs.choice([33, 64, 100, 160, 257, 400])), int(rs.choice([17, 48, 96, 144, 230]))
    N = int(rs.choice([1, 7, 300, 2000, 9000, 30000]))
    deg = int(rs.randint(0, 4)); seed = int(rs.randint(1 << 30))
    s = synthetic_scene(N, W, H, deg, seed)
    s["opacities"] = (s["opacities"] * rs.choice([0.05, 0.3, 1.0])).astype(np.float32)
    s["scales"] = (s["scales"] * rs.choice([0.3, 1.0, 4.0])).astype(np.float32)
    return s, f"N={N} {W}x{H} deg={deg} seed={seed}"


if __name__ == "__main__":
    ncase = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    # 256 = depth segment / forward batch; 128 / 1024 = rank sort / in-kernel sort limits; 12 288 = keys the bucket sort keeps
    # resident in LDS; beyond: groups of <= 1024 + sg_group_sort_kernel.  (The 64x48 image is a few-tile frame: lists of more than
    # 1024 entries are also composited by four workgroups, and the backward is the sparse kernel.)
    for n in CRAFTED_LENGTHS:
        s = crafted(n, n)
        R, mx = check(s, f"crafted {n}")
        print(f"crafted list length {n}: R={R} max list {mx}  ok", flush=True)
        assert mx >= n
    for seed in (1, 2, 3):
        z = clustered_depths(seed)
        R, mx = check(crafted(z.size, 100 + seed, depths=z), f"clustered depths {seed}")
        print(f"clustered depths (seed {seed}): R={R} max list {mx}  ok", flush=True)
    rs = np.random.RandomState(int(os.environ.get("FUZZ_SEED", "1234")))
    for c in range(ncase):
        s, tag = random_case(rs)
        R, mx = check(s, f"case {c}: {tag}")
        print(f"case {c}: {tag} R={R} max list {mx}  ok", flush=True)
    for c in range(int(os.environ.get("FUZZ_LARGE", "4"))):
        s, tag = random_case(rs, large=True)
        R, mx = check(s, f"large case {c}: {tag}")
        print(f"large case {c}: {tag} R={R} max list {mx}  ok", flush=True)
    print("all cases passed")
