"""The depth and alpha maps (GaussianRasterizer.forward_aux, sg_rasterize_*_aux) on degenerate inputs and on every input form,
against oracle/raster_aux.py.  The degenerate cases mirror tests/test_gpu_degenerate.py with the same bar: the call returns,
everything is finite, a culled (poisoned) Gaussian gets zero gradients -- its means gradient included, which the dz x view-row term
would poison if the per-Gaussian backward read a stale dL/dz -- and the other Gaussians' colour, maps and gradients are
bit-identical to a run without it.  The input forms: colors_precomp, cov3D_precomp, scale_modifier 0.5 and 1.7 (dL/dscale w.r.t.
the modified scale, the oracle's convention), SH degrees 0 and 2, ragged images -- the latter also through the C ABI with the maps and
their adjoint planes inside larger sentinel-filled buffers: nothing outside [H, W] is written and nothing outside it is read."""
import numpy as np
import pytest
import torch

from oracle.raster_aux import oracle_pair, reference_grads
from sings_amd.scene import synthetic_scene

pytestmark = pytest.mark.gpu
BORDER = 2e-5
GRADS = ("means3D", "means2D", "opacities", "shs", "colors", "scales", "rotations", "cov3D")


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _close(name, a, b, rtol=1e-3, atol=6e-6):
    """tests/test_gpu_aux_maps.py::_grad_close, plus finiteness."""
    a = np.asarray(a, np.float64).reshape(np.shape(b)); b = np.asarray(b, np.float64)
    assert np.isfinite(a).all(), f"{name}: non-finite values on the HIP side"
    scale = np.abs(b).max() + 1e-30
    bad = np.abs(a - b) > rtol * np.abs(b) + atol * scale
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} off; worst {np.abs(a - b).max():.3e} (scale {scale:.3e})"


def _oracle(s, cov3D=None, colors=None, mod=1.0):
    return oracle_pair(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                       s["tanfovy"], s["bg"], s["scales"], s["rotations"], s["shs"], s["sh_degree"], colors_precomp=colors,
                       cov3D_precomp=cov3D, scale_modifier=mod)


def _seeds(s, strict, seed=5):
    rng = np.random.RandomState(seed)
    H, W = s["H"], s["W"]
    dLc = np.ascontiguousarray(s["dL_dimage"][:, :H, :W]).copy()
    gD = rng.normal(0, 1, (H, W)).astype(np.float32); gA = rng.normal(0, 1, (H, W)).astype(np.float32)
    dLc[:, ~strict] = 0; gD[~strict] = 0; gA[~strict] = 0
    return dLc, gD, gA


def _run(s, cov3D=None, colors=None, mod=1.0, check=True, seeds=None):
    """forward_aux + backward under a loss on colour, depth and alpha, and the two-pass oracle on the same arrays."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    dev = _dev()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    req = lambda a: None if a is None else t(a).requires_grad_(True)
    rs = GaussianRasterizationSettings(image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                       scale_modifier=mod, viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]),
                                       sh_degree=s["sh_degree"], campos=t(s["campos"]), prefiltered=False, debug=False)
    x = dict(means3D=req(s["means3D"]), opacities=req(s["opacities"]), shs=None if colors is not None else req(s["shs"]),
             colors=req(colors), scales=None if cov3D is not None else req(s["scales"]),
             rotations=None if cov3D is not None else req(s["rotations"]), cov3D=req(cov3D))
    x["means2D"] = torch.zeros_like(x["means3D"], requires_grad=True)
    color, radii, depth, alpha = GaussianRasterizer(rs).forward_aux(
        means3D=x["means3D"], means2D=x["means2D"], opacities=x["opacities"], shs=x["shs"], colors_precomp=x["colors"],
        scales=x["scales"], rotations=x["rotations"], cov3D_precomp=x["cov3D"])
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        o, oa = _oracle(s, cov3D, colors, mod)
    strict = o["margin"] >= BORDER
    dLc, gD, gA = seeds if seeds is not None else _seeds(s, strict)
    ((color * t(dLc)).sum() + (depth[0] * t(gD)).sum() + (alpha[0] * t(gA)).sum()).backward()
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        ref = reference_grads(o, oa, dLc, gD, gA, s["viewmatrix"])
    out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(), depth=depth.detach().cpu().numpy()[0],
               alpha=alpha.detach().cpu().numpy()[0], o=o, oa=oa, ref=ref, strict=strict, seeds=(dLc, gD, gA),
               grads={k: v.grad.cpu().numpy() for k, v in x.items() if v is not None})
    for k in ("color", "depth", "alpha"):
        assert np.isfinite(out[k]).all(), k
    for k, v in out["grads"].items():
        assert np.isfinite(v).all(), k
    if check:
        _check(out)
    return out


def _check(out, rows=slice(None)):
    o, oa, strict = out["o"], out["oa"], out["strict"]
    np.testing.assert_array_equal(out["radii"], o["radii"])
    vis = o["radii"] > 0
    zmax = np.abs(o["depths"][vis]).max() if vis.any() else 1.0
    if strict.any():
        assert np.abs(out["color"] - o["color"]).max(0)[strict].max() <= 1e-5
        assert np.abs(out["alpha"] - oa["color"][1])[strict].max() <= 1e-5
        assert np.abs(out["depth"] - oa["color"][0])[strict].max() <= 1e-5 * zmax
    for name in GRADS:
        if name in out["grads"]:
            _close(name, out["grads"][name][rows], np.nan_to_num(out["ref"][name][rows]))


def _without(s, drop):
    keep = np.setdiff1d(np.arange(s["means3D"].shape[0]), drop)
    sub = dict(s)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        sub[k] = np.ascontiguousarray(s[k][keep])
    return sub, keep


# ---- degenerate inputs (tests/test_gpu_degenerate.py) ---------------------------------------------------------------------------
def test_nan_and_inf_inputs_are_culled_and_harm_nobody():
    s = synthetic_scene(3000, 160, 96, 2, 31)
    clean = _run(s)
    vis = np.nonzero(clean["radii"] > 0)[0]
    pick = vis[:: max(1, vis.size // 60)][:60]
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    for j, i in enumerate(pick):
        k = j % 6
        if k == 0: bad["means3D"][i, j % 3] = np.nan
        elif k == 1: bad["means3D"][i, j % 3] = np.inf
        elif k == 2: bad["means3D"][i, 2] = -np.inf
        elif k == 3: bad["scales"][i, j % 3] = np.nan
        elif k == 4: bad["scales"][i, j % 3] = np.inf
        else: bad["rotations"][i, j % 4] = np.nan
    sub, keep = _without(s, pick)
    ref = _run(sub)                                                   # checked against the oracle as well
    out = _run(bad, check=False, seeds=ref["seeds"])
    assert (out["radii"][pick] == 0).all()
    for name, g in out["grads"].items():
        assert np.abs(g[pick]).max() == 0, f"{name}: a culled (non-finite) Gaussian received a gradient"
    for k in ("color", "depth", "alpha"):
        assert np.array_equal(out[k], ref[k]), k
    for name, g in out["grads"].items():
        assert np.array_equal(g[keep], ref["grads"][name]), name


def test_zero_scales():
    s = synthetic_scene(2500, 128, 96, 1, 32)
    s["scales"] = np.zeros_like(s["scales"])
    out = _run(s)
    assert (out["radii"] == 3).sum() > 1000


def test_singular_2d_covariance_with_cov3d_and_colors_precomp():
    """tests/test_gpu_degenerate.py's exact det == 0 case: four Gaussians culled by the early return, healthy ones beside them."""
    from oracle import raster_oracle as ro
    from sings_amd.camera import get_projection_matrix
    W = H = 32
    s = synthetic_scene(400, W, H, 0, 33)
    tan = W / (2 * 4.0)
    s.update(tanfovx=tan, tanfovy=tan)
    fov = 2 * np.arctan(tan)
    s["projmatrix"] = (s["viewmatrix"] @ get_projection_matrix(0.01, 100.0, fov, fov).T).astype(np.float32)
    o0 = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, tan, tan, s["bg"],
                    scales=s["scales"], rotations=s["rotations"], colors_precomp=np.full((400, 3), 0.5, np.float32))
    cov = o0["cov3D"].copy()
    s["means3D"][:4] = np.array([0, 0, 4.0], np.float32)
    cov[:4] = np.array([-0.3, 0, 0, 1, 0, 1], np.float32)
    colors = np.random.RandomState(3).uniform(0, 1, (400, 3)).astype(np.float32)
    out = _run(s, cov3D=cov, colors=colors)
    assert (out["radii"][:4] == 0).all() and (out["radii"][4:] > 0).sum() > 100
    for name in ("cov3D", "means3D", "colors", "opacities", "means2D"):
        assert np.abs(out["grads"][name][:4]).max() == 0, name


def test_opacity_exactly_zero_and_exactly_one():
    s = synthetic_scene(3000, 160, 96, 3, 34)
    s["opacities"][::2] = 0.0
    s["opacities"][1::2] = 1.0
    out = _run(s)
    assert np.abs(out["grads"]["opacities"][::2]).max() == 0 and np.abs(out["grads"]["means3D"][::2]).max() == 0
    assert np.abs(out["grads"]["opacities"][1::2]).max() > 0
    assert out["alpha"].max() > 0.99


@pytest.mark.parametrize("equal_depths", [False, True])
def test_every_gaussian_on_one_pixel(equal_depths):
    s = synthetic_scene(3000, 96, 64, 1, 35)
    rs = np.random.RandomState(35)
    z = np.full(3000, 5.0, np.float32) if equal_depths else rs.uniform(3, 8, 3000).astype(np.float32)
    s["means3D"] = np.stack([0.01 * z, -0.02 * z, z], 1).astype(np.float32)
    s["opacities"] = rs.uniform(0.002, 0.05, (3000, 1)).astype(np.float32)
    out = _run(s)
    tl = out["o"]["ranges"][:, 1].astype(int) - out["o"]["ranges"][:, 0]
    assert tl.max() == 3000
    if equal_depths:      # every blended z is 5: the depth map is 5 x alpha
        assert np.abs(out["depth"] - 5.0 * out["alpha"]).max() <= 1e-5 * 5.0


@pytest.mark.parametrize("W,H", [(1, 1), (17, 15), (16, 16), (33, 1)])
def test_tiny_and_ragged_images(W, H):
    s = synthetic_scene(500, W, H, 2, 36)
    if W < 16:
        s["scales"] = (s["scales"] * 40).astype(np.float32)
    s["dL_dimage"] = np.random.RandomState(1).normal(0, 1, (3, H, W)).astype(np.float32)
    out = _run(s)
    assert out["depth"].shape == (H, W) and (out["radii"] > 0).any() and out["alpha"].max() > 0


def test_one_sh_row_at_degree_zero_and_a_single_gaussian():
    s = synthetic_scene(2000, 96, 64, 0, 37, M=1)
    out = _run(s)
    assert out["grads"]["shs"].shape == (2000, 1, 3)
    one = synthetic_scene(1, 64, 48, 3, 38)
    one["means3D"][:] = np.array([0.1, -0.1, 4.0], np.float32); one["scales"][:] = 0.05; one["opacities"][:] = 0.7
    out = _run(one)
    assert out["radii"][0] > 0 and out["alpha"].max() > 0.5 and out["depth"].max() > 0
    one["means3D"][:] = np.array([0.0, 0.0, -1.0], np.float32)       # behind the camera: empty maps, no gradient
    out = _run(one)
    assert out["radii"][0] == 0 and out["depth"].max() == 0 and out["alpha"].max() == 0
    for name, g in out["grads"].items():
        assert np.abs(g).max() == 0, name


# ---- input forms -------------------------------------------------------------------------------------------------------------
def test_colors_precomp():
    s = synthetic_scene(3000, 160, 96, 1, 51)
    colors = np.random.RandomState(51).uniform(0, 1, (3000, 3)).astype(np.float32)
    out = _run(s, colors=colors)
    assert np.abs(out["grads"]["colors"]).max() > 0


def test_cov3d_precomp():
    from oracle import raster_oracle as ro
    s = synthetic_scene(3000, 160, 96, 2, 52)
    o0 = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                    s["tanfovy"], s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=2)
    rs = np.random.RandomState(52)
    cov = o0["cov3D"].copy()
    cov[o0["radii"] == 0] = np.array([1e-4, 0, 0, 1e-4, 0, 1e-4], np.float32)  # (culled rows were never stored)
    out = _run(s, cov3D=cov)
    assert np.abs(out["grads"]["cov3D"]).max() > 0
    # a colours-and-covariance-precomputed scene as well
    out = _run(s, cov3D=cov, colors=rs.uniform(0, 1, (3000, 3)).astype(np.float32))
    assert np.abs(out["grads"]["colors"]).max() > 0


@pytest.mark.parametrize("mod", [0.5, 1.7])
def test_scale_modifier(mod):
    s = synthetic_scene(3000, 160, 96, 3, 53)
    out = _run(s, mod=mod)
    assert np.abs(out["grads"]["scales"]).max() > 0


@pytest.mark.parametrize("deg", [0, 2])
def test_sh_degrees(deg):
    s = synthetic_scene(3000, 160, 96, deg, 54)
    _run(s)


@pytest.mark.parametrize("W,H", [(17, 15), (33, 1), (1, 1)])
def test_ragged_maps_write_and_read_nothing_outside_the_image(W, H):
    """Through the C ABI: the maps and the dL/ddepth, dL/dalpha planes sit 4 096 floats into buffers 8 192 floats longer than
    [H, W], filled with a sentinel.  The sentinels around the maps survive; a NaN sentinel around the adjoint planes changes no
    gradient bit against a finite one; the result equals the oracle."""
    from tests.tools import fuzz_parity as fp
    s = synthetic_scene(500, W, H, 2, 56)
    if W < 16:
        s["scales"] = (s["scales"] * 40).astype(np.float32)
    s["dL_dimage"] = np.random.RandomState(2).normal(0, 1, (3, H, W)).astype(np.float32)
    o, oa = _oracle(s)
    dLc, gD, gA = _seeds(s, o["margin"] >= BORDER)
    pad, HW = 4096, H * W
    runs = []
    for sentinel in (-7.25, float("nan")):
        x = fp.aux_abi(s, dLc, gD, gA, pad=pad, sentinel=sentinel)
        for buf in (x["depth_buf"], x["alpha_buf"]):
            outside = torch.cat([buf[:pad], buf[pad + HW:]])
            if sentinel == sentinel:
                assert bool((outside == sentinel).all()), "a map was written outside [H, W]"
            else:
                assert bool(torch.isnan(outside).all()), "a map was written outside [H, W]"
        runs.append(x)
    a, b = runs
    for k in ("color", "depth", "alpha"):
        assert torch.equal(a[k], b[k]), k
    for k in a["grads"]:
        assert torch.isfinite(b["grads"][k]).all(), k
        assert torch.equal(a["grads"][k], b["grads"][k]), f"{k}: the adjoint outside [H, W] reached a gradient"
    out = dict(color=a["color"].cpu().numpy(), radii=a["radii"].cpu().numpy(), depth=a["depth"].cpu().numpy(),
               alpha=a["alpha"].cpu().numpy(), o=o, oa=oa, strict=o["margin"] >= BORDER,
               ref=reference_grads(o, oa, dLc, gD, gA, s["viewmatrix"]), grads={k: v.cpu().numpy() for k, v in a["grads"].items()})
    _check(out)
