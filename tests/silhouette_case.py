"""What the silhouette tests share: the camera of ``pose_refine_case`` (40 x 56: partial tiles on the right and bottom edges), the
``octa_level`` meshes at z = 4, the two twins (``pose_refine.silhouette_host`` in fp64 and fp32, each computed once per case and
never changed) with a seeded dL/dalpha, a numpy fp64 table of every (pixel, face) pair -- for the borderline pixels, the brute-force
tile lists and the division-free gradient -- and the tolerance rule, ``body_case.held``.

BORDERLINE: a pixel where, in fp64, some valid outside face has |d2 - r| <= 1e-4 r.  There fp32 may decide the band test the other
way, a step of at most 1e-4 (the coverage at the band's edge) per such face: the pixel is left out of the alpha comparison, checked
against 1.1e-4 times the number of such faces instead, and dL/dalpha is ZERO there so that no flipped pair reaches a gradient."""
import numpy as np
import torch

import body_case as bc
import pose_refine_case as prc
from sings_amd import pose_refine as PR

W, H, INTR = prc.W, prc.H, prc.INTR
LEVELS, SIGMAS = (2, 3, 4), (1e-4, 4e-3)
_CACHE = {}


def mesh(level, K=3, z=4.0, seed=11):
    """-> (verts [K,V,3] fp32 camera space, different per frame: a seeded small rotation and shift; faces [F,3] int64)."""
    v, f, _ = bc.octa_level(level)
    rs = np.random.RandomState(seed + level)
    out = []
    for k in range(K):
        a = 0.3 * rs.randn(3)
        Rm = PR.rodrigues(torch.tensor(a[None])).numpy()[0]
        out.append(v.astype(np.float64) @ Rm.T + np.array([0.08 * rs.randn(), 0.08 * rs.randn(), z + 0.1 * k]))
    return np.stack(out).astype(np.float32), f


def pair_table(verts, faces, intr, H, W, sigma):
    """One frame in numpy fp64, the definition written out: dict of [H,W,F] arrays ``on``, ``inside``, ``d2n``, ``edge``, ``t``, ``dx``,
    ``dy``, and ``valid`` [F], ``uv`` [F,3,2], ``r``, ``s2``."""
    fx, fy, cx, cy = intr
    tri = np.asarray(verts, np.float64)[np.asarray(faces)]
    with np.errstate(all="ignore"):
        z = tri[..., 2]
        valid = np.isfinite(tri).all((-1, -2)) & (z > PR.ZNEAR).all(-1)
        zs = np.where(valid[:, None], z, 1.0)
        uv = np.stack([fx * tri[..., 0] / zs + cx, fy * tri[..., 1] / zs + cy], -1)
        valid &= np.isfinite(uv).all((-1, -2))
        uv = np.where(valid[:, None, None], uv, np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]))
        s2 = (2.0 / min(H, W)) ** 2
        e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        valid &= np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) * s2 > PR.MIN_AREA
        uv = np.where(valid[:, None, None], uv, np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]))
    px = (np.arange(W) + 0.5)[None, :, None]
    py = (np.arange(H) + 0.5)[:, None, None]
    pos = neg = True
    best = None
    for e in range(3):
        a, b = uv[:, e], uv[:, (e + 1) % 3]
        ex, ey = (b - a)[:, 0], (b - a)[:, 1]
        wx, wy = px - a[:, 0], py - a[:, 1]
        cr = ex * wy - ey * wx
        pos, neg = (cr > 0) & pos, (cr < 0) & neg
        t = np.clip((wx * ex + wy * ey) / (ex * ex + ey * ey), 0, 1)
        dx, dy = wx - t * ex, wy - t * ey
        d2 = dx * dx + dy * dy
        if best is None:
            best = dict(d2=d2, edge=np.zeros(d2.shape, np.int64), t=t, dx=dx, dy=dy)
        else:
            less = d2 < best["d2"]
            best = dict(d2=np.where(less, d2, best["d2"]), edge=np.where(less, e, best["edge"]), t=np.where(less, t, best["t"]),
                        dx=np.where(less, dx, best["dx"]), dy=np.where(less, dy, best["dy"]))
    inside = pos | neg
    d2n, r = best["d2"] * s2, PR.LOGIT * sigma
    return dict(on=valid & (inside | (d2n < r)), inside=inside, d2n=d2n, edge=best["edge"], t=best["t"], dx=best["dx"], dy=best["dy"],
                valid=valid, uv=uv, r=r, s2=s2)


def borderline(table):
    """-> [H,W] int: the number of valid outside faces with |d2 - r| <= 1e-4 r."""
    return (table["valid"] & ~table["inside"] & (np.abs(table["d2n"] - table["r"]) <= 1e-4 * table["r"])).sum(-1)


def twins(verts, faces, intr, H, W, sigma, seed=3, window=None):
    """``verts`` [K,V,3] fp32 -> dict: ``alpha64`` / ``alpha32`` [K,H,W], ``g`` (the seeded dL/dalpha, zero on borderline pixels and
    outside ``window`` = (y0, y1, x0, x1)), ``grad64`` / ``grad32`` [K,V,3], ``border`` [K,H,W] int, ``counts`` [K] (fp64)."""
    K = verts.shape[0]
    border = np.stack([borderline(pair_table(verts[k], faces, intr, H, W, sigma)) for k in range(K)])
    g = np.random.RandomState(seed).randn(K, H, W)
    g[border > 0] = 0.0
    if window is not None:
        keep = np.zeros((H, W), bool)
        keep[window[0]:window[1], window[2]:window[3]] = True
        g[:, ~keep] = 0.0
    out = dict(g=g.astype(np.float32), border=border)
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        v = torch.tensor(verts, dtype=dt, requires_grad=True)
        alpha, cnt = PR.silhouette_host(v, faces, intr, H, W, sigma, return_counts=True)
        (alpha * torch.tensor(out["g"], dtype=dt)).sum().backward()
        out["alpha" + name], out["grad" + name] = alpha.detach().numpy(), v.grad.numpy()
        if name == "64":
            out["counts"] = cnt.numpy()
    return out


def case(level, sigma):
    """The three-frame parity case of (level, sigma), computed once: ``verts``, ``faces`` and the fields of ``twins``.  Frame 0 alone is
    the K = 1 case."""
    key = (level, sigma)
    if key not in _CACHE:
        verts, faces = mesh(level)
        _CACHE[key] = dict(twins(verts, faces, INTR, H, W, sigma), verts=verts, faces=faces)
    return _CACHE[key]


def check_alpha(alpha_dev, tw, what, frames=None):
    """alpha held on the pixels that are not borderline; on those, |delta| <= 1.1e-4 times the number of borderline faces.  At most
    1 % of the pixels may be left out."""
    sel = slice(None) if frames is None else frames
    a64, a32, border = tw["alpha64"][sel], tw["alpha32"][sel], tw["border"][sel]
    a = np.asarray(alpha_dev, np.float64)
    out = border > 0
    print(f"{what}: {int(out.sum())} of {out.size} pixels borderline")
    assert out.sum() <= 0.01 * out.size, what
    assert (np.abs(a - a64)[out] <= 1.1e-4 * border[out]).all(), what
    keep = ~out
    return bc.held(np.where(keep, a, 0.0), np.where(keep, a32, 0.0), np.where(keep, a64, 0.0), what + " alpha")
