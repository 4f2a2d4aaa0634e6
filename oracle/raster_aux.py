"""ORACLE (test infrastructure only): the depth and alpha maps as a composition of the scalar raster oracle
(oracle/raster_core.inc.c through oracle/raster_oracle.py), two passes over the same Gaussians:
 * the colour pass with the scene's colours and background;
 * the aux pass with colors_precomp = (z, 1, 0) and background 0, whose channels 0 and 1 are depth (sum z alpha T) and
   alpha (1 - T_final).
Gradients: the colour pass's backward + the aux pass's backward seeded with (dL/ddepth, dL/dalpha, 0) + the aux pass's
dL/dcolour[:, 0] (= dL/dz) chained through the view row of z into the means.

tests/test_oracle_aux_twin.py holds this composition against oracle/raster_torch.py, whose depth / alpha maps are part of one
autograd graph (no hand-added view-row term).  The GPU AUX tests (tests/test_gpu_aux_*.py, tests/tools/fuzz_parity.py) use it
as their reference.
"""
import numpy as np

from oracle import raster_oracle as ro


def view_row(view):
    """d z / d mean: z = view[2] x + view[6] y + view[10] z + view[14] (column-major 4x4, as the preprocess reads it)."""
    v = np.asarray(view, np.float64).reshape(-1)
    return v[[2, 6, 10]]


def oracle_pair(means3D, opac, view, proj, campos, W, H, tx, ty, bg, scales, rots, shs, deg, colors_precomp=None,
                cov3D_precomp=None, scale_modifier=1.0, dtype=np.float32):
    """(colour pass, aux pass) of the raster oracle.  Exactly one of shs / colors_precomp and of (scales, rots) /
    cov3D_precomp is given, as for the op."""
    geo = dict(scales=None, rotations=None, cov3D_precomp=cov3D_precomp) if cov3D_precomp is not None else \
        dict(scales=scales, rotations=rots)
    kw = dict(scale_modifier=scale_modifier, dtype=dtype, sh_degree=deg, **geo)
    o = ro.forward(means3D, opac, view, proj, campos, W, H, tx, ty, bg, shs=None if colors_precomp is not None else shs,
                   colors_precomp=colors_precomp, **kw)
    P = np.asarray(means3D).reshape(-1, 3).shape[0]
    zc = np.stack([o["depths"].astype(dtype), np.ones(P, dtype), np.zeros(P, dtype)], 1)
    oa = ro.forward(means3D, opac, view, proj, campos, W, H, tx, ty, np.zeros(3, dtype), colors_precomp=np.ascontiguousarray(zc),
                    **kw)
    return o, oa


def reference_grads(o, oa, dLc, gD, gA, view):
    """Per input: colour pass + aux pass + dL/dz through the view row.  Keys: means3D, means2D, opacities, and whichever of
    shs / colors and scales + rotations / cov3D the passes were given."""
    dtype = o["_in"]["dtype"]
    gc = ro.backward(o, dLc)
    ga = ro.backward(oa, np.stack([gD, gA, np.zeros_like(gD)]).astype(dtype))
    dz = ga["dL_dcolor"][:, 0].astype(np.float64)
    out = {
        "means3D": gc["dL_dmeans3D"] + ga["dL_dmeans3D"] + dz[:, None] * view_row(view)[None, :],
        "means2D": gc["dL_dmean2D"] + ga["dL_dmean2D"],
        "opacities": gc["dL_dopacity"] + ga["dL_dopacity"],
    }
    if gc["dL_dsh"] is not None:
        out["shs"] = gc["dL_dsh"]
    else:
        out["colors"] = gc["dL_dcolor"]
    if gc["dL_dscales"] is not None:
        out["scales"] = gc["dL_dscales"] + ga["dL_dscales"]
        out["rotations"] = gc["dL_drots"] + ga["dL_drots"]
    else:
        out["cov3D"] = gc["dL_dcov3D"] + ga["dL_dcov3D"]
    return out
