"""The depth and alpha maps' reference, restated twice and held against each other in fp64 (CPU):
 * oracle/raster_aux.py -- two passes of the scalar C oracle (colour pass + a colors_precomp = (z, 1, 0) pass), dL/dz added to the
   means by hand through the view row of z: the reference every GPU AUX test uses;
 * oracle/raster_torch.py -- depth = sum z alpha T and alpha = 1 - T_final inside one autograd graph, z the graph's own t.z.
Maps to fp64 round-off; every gradient element, means3D (with the dz term) and means2D included, to round-off as well.  If these
disagree the convention of one of them is wrong."""
import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from oracle import raster_torch as rt
from oracle.raster_aux import oracle_pair, reference_grads, view_row
from sings_amd.scene import synthetic_scene
from test_oracle_raster_twin import CASES

LOSSES = {"colour": "c", "depth": "d", "alpha": "a", "all": "cda"}


def _seeds(s, which, seed):
    H, W = s["H"], s["W"]
    rng = np.random.RandomState(seed)
    dLc = s["dL_dimage"].astype(np.float64) if "c" in which else np.zeros((3, H, W))
    gD = rng.normal(0, 1, (H, W)) if "d" in which else np.zeros((H, W))
    gA = rng.normal(0, 1, (H, W)) if "a" in which else np.zeros((H, W))
    return dLc, gD, gA


def _err(a, b):
    """Worst element error relative to the reference's largest magnitude (0 when both are exactly zero)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64).reshape(a.shape)
    d = np.abs(a - b).max() if a.size else 0.0
    return 0.0 if d == 0 else d / max(np.abs(b).max(), 1e-300)


def twin_errors(tag, mod, loss):
    N, W, H, deg, seed = CASES[tag]
    s = synthetic_scene(N, W, H, deg, seed)
    dLc, gD, gA = _seeds(s, LOSSES[loss], seed + 7)
    o, oa = oracle_pair(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"],
                        s["tanfovy"], s["bg"], s["scales"], s["rotations"], s["shs"], deg, scale_modifier=mod, dtype=np.float64)
    ref = reference_grads(o, oa, dLc, gD, gA, s["viewmatrix"])
    t, tg = rt.forward_backward(s, dLc if "c" in LOSSES[loss] else None, torch.float64, scale_modifier=mod,
                                dL_ddepth=gD if "d" in LOSSES[loss] else None, dL_dalpha=gA if "a" in LOSSES[loss] else None)
    np.testing.assert_array_equal(t["radii"], o["radii"])
    np.testing.assert_array_equal(t["n_contrib"], oa["n_contrib"])
    maps = {"depth": _err(t["depth"], oa["color"][0]), "alpha": _err(t["alpha"], oa["color"][1]),
            "alpha=1-T": _err(t["alpha"], 1.0 - o["final_T"]), "color": _err(t["color"], o["color"])}
    grads = {"means3D": _err(tg["dL_dmeans3D"], ref["means3D"]), "means2D": _err(tg["dL_dmean2D"], ref["means2D"][:, :2]),
             "opacities": _err(tg["dL_dopacity"], ref["opacities"]), "scales": _err(tg["dL_dscales"], ref["scales"]),
             "rotations": _err(tg["dL_drots"], ref["rotations"]), "shs": _err(tg["dL_dsh"], ref["shs"])}
    return s, o, oa, ref, tg, maps, grads


@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("mod", [1.0, 0.6])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_two_pass_composition_and_autograd_twin_agree(tag, mod, loss):
    s, o, oa, ref, tg, maps, grads = twin_errors(tag, mod, loss)
    assert np.abs(oa["color"][0]).max() > 0 and oa["color"][1].max() > 0.5
    for k, e in maps.items():
        assert e < 1e-12, (k, e)
    for k, e in grads.items():
        assert e < 1e-12, (k, e)


def test_depth_gradient_reaches_the_means_through_the_view_row():
    """A depth-only loss: the twin's means gradient minus the two-pass composition's WITHOUT its hand-added term is exactly that
    term, dL/dz x view row -- a convention error (sign, row vs column, a missing or doubled term) shows here first."""
    s, o, oa, ref, tg, maps, grads = twin_errors("a", 1.0, "depth")
    H, W = s["H"], s["W"]
    gD = _seeds(s, "d", CASES["a"][4] + 7)[1]
    ga = ro.backward(oa, np.stack([gD, np.zeros((H, W)), np.zeros((H, W))]))
    term = ga["dL_dcolor"][:, 0][:, None] * view_row(s["viewmatrix"])[None, :]
    assert np.abs(term).max() > 1e-3 * np.abs(ref["means3D"]).max()
    assert _err(tg["dL_dmeans3D"] - ga["dL_dmeans3D"], term) < 2e-9
