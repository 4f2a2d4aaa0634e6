"""The forward composite's quadrant test evaluates only the edges of the pixel rectangle that face the mean (sg_min_q_rect in
sings_amd/csrc/sg_render.hip), where it evaluated all four.  With numpy fp32 twins of both forms (tests/quad_mask_case.py), over
1.2 million seeded random (conic, opacity, mean, rectangle) cases:

 * the new bit is set wherever a brute-force scan finds a pixel centre of the rectangle that the blend loop accepts (power <= 0 and
   alpha >= 1/255) -- the property the images, contributor counts, checkpoints and gradients rest on;
 * new and old bits differ only where the test itself is within rounding of its bound: |0.999 min q - bound| <= 1e-4 bound, for both
   forms' minimum.

The cases: rectangles inside a quadrant, down to one pixel, one row and one column; means in all eight regions around the rectangle,
inside it and exactly on its edges and corners, placed so that the alpha = 1/255 contour passes near the rectangle (both outcomes are
common); round conics and 6 : 1 ellipses at four orientations; opacities from 1/255 (where only power = 0 is accepted) to 1; tile
origins 0, 16 and 1024 (the mean's offset from the tile is a rounded difference).  And on one full oracle view: no (entry, quadrant)
that blends a pixel is dropped."""
import numpy as np

import quad_mask_case as qm
from oracle import raster_oracle as ro
from sings_amd.scene import synthetic_scene

f32 = np.float32
CASES = 1_200_000
CHUNK = 200_000


def _cases(rs, n):
    # the rectangle: inside one quadrant of the tile; a quarter each shrunk to one pixel, one row, one column
    q = rs.randint(0, 4, n)
    a, b = np.sort(rs.randint(0, 8, (2, n)), 0)
    c, d = np.sort(rs.randint(0, 8, (2, n)), 0)
    kind = rs.randint(0, 8, n)
    b = np.where((kind == 0) | (kind == 2), a, b)              # one column (0), one pixel (2)
    d = np.where((kind == 1) | (kind == 2), c, d)              # one row (1)
    x0, x1 = (8 * (q & 1) + a).astype(f32), (8 * (q & 1) + b).astype(f32)
    y0, y1 = (8 * (q >> 1) + c).astype(f32), (8 * (q >> 1) + d).astype(f32)
    # the conic: sigma 0.4 .. 12 px; round, mild, or 6 : 1 at 0 / 45 / 90 / 135 degrees
    s1 = np.exp(rs.uniform(np.log(0.4), np.log(12.0), n))
    shape = rs.randint(0, 3, n)
    ratio = np.where(shape == 0, 1.0, np.where(shape == 1, rs.uniform(1.0, 3.0, n), 6.0))
    th = np.where(shape == 2, rs.randint(0, 4, n) * (np.pi / 4), rs.uniform(0, np.pi, n))
    s2 = s1 / ratio
    cs, sn = np.cos(th), np.sin(th)
    l1, l2 = 1.0 / (s1 * s1), 1.0 / (s2 * s2)                  # eigenvalues of the conic
    A, B, C = (cs * cs * l1 + sn * sn * l2), (cs * sn * (l1 - l2)), (sn * sn * l1 + cs * cs * l2)
    # opacity: 1/255 exactly, just above it, or log-uniform up to 1
    ok = rs.randint(0, 8, n)
    op = np.where(ok == 0, 1.0 / 255.0, np.where(ok == 1, (1.0 + rs.uniform(0, 0.02, n)) / 255.0, np.exp(rs.uniform(np.log(1.0 / 255.0), 0.0, n))))
    tau2 = 2.0 * np.log(np.maximum(255.0 * op, 1.0))
    # the mean: a point of the rectangle (interior, edge or corner), pushed outwards along a direction of one of the eight regions -- or not
    # at all -- by 0.3 .. 1.7 times the distance at which the alpha = 1/255 contour sits in that direction
    u, v = rs.uniform(0, 1, n), rs.uniform(0, 1, n)
    snap = rs.randint(0, 3, (2, n))
    u = np.where(snap[0] == 0, 0.0, np.where(snap[0] == 1, 1.0, u)); v = np.where(snap[1] == 0, 0.0, np.where(snap[1] == 1, 1.0, v))
    bxp, byp = x0 + u * (x1 - x0), y0 + v * (y1 - y0)
    region = rs.randint(0, 10, n)                              # 0-7: the eight regions; 8: on the rectangle; 9: any direction
    ang = np.where(region < 8, region * (np.pi / 4), rs.uniform(0, 2 * np.pi, n))
    vx, vy = np.cos(ang), np.sin(ang)
    vx = np.where(np.abs(vx) < 1e-9, 0.0, vx); vy = np.where(np.abs(vy) < 1e-9, 0.0, vy)
    # (axis directions leave from the matching edge, diagonals from the matching corner: the mean then lies in that region)
    bxp = np.where((region < 8) & (vx > 0), x1, np.where((region < 8) & (vx < 0), x0, bxp))
    byp = np.where((region < 8) & (vy > 0), y1, np.where((region < 8) & (vy < 0), y0, byp))
    mahal = np.sqrt(A * vx * vx + 2 * B * vx * vy + C * vy * vy)
    push = np.where(region == 8, 0.0, rs.uniform(0.3, 1.7, n) * np.sqrt(tau2) / mahal + np.where(rs.randint(0, 4, n) == 0, rs.uniform(0, 1.5, n), 0.0))
    X0 = rs.choice([0.0, 16.0, 1024.0], n); Y0 = rs.choice([0.0, 16.0, 1024.0], n)
    ax, ay = X0 + bxp + push * vx, Y0 + byp + push * vy
    to = lambda *vs: tuple(np.asarray(w, f32) for w in vs)
    return to(ax, ay, A, B, C, op, X0, Y0, x0, x1, y0, y1)


def _brute(ax, ay, A, B, C, op, X0, Y0, x0, x1, y0, y1):
    """Some pixel centre of the rectangle is accepted by the blend loop."""
    hit = np.zeros(ax.shape, bool)
    for j in range(8):
        for i in range(8):
            px, py = x0 + f32(i), y0 + f32(j)
            inside = (px <= x1) & (py <= y1)
            hit |= inside & qm.accepts(ax, ay, A, B, C, op, X0 + px, Y0 + py)
    return hit


def test_the_facing_edges_form_keeps_every_accepted_pixel_and_differs_from_the_four_edges_form_only_at_the_bound():
    rs = np.random.RandomState(20241)
    tally = dict(cases=0, hit=0, set_new=0, differ=0, regions=np.zeros(9, np.int64))
    for _ in range(CASES // CHUNK):
        c = _cases(rs, CHUNK)
        new, lhs_n, bound = qm.quad_bit(qm.min_q_rect_facing_edges, *c)
        old, lhs_o, _ = qm.quad_bit(qm.min_q_rect_four_edges, *c)
        hit = _brute(*c)
        dropped = hit & ~new
        assert not dropped.any(), f"{dropped.sum()} accepted rectangles dropped, e.g. {[float(v[dropped][0]) for v in c]}"
        assert not (hit & ~old).any()
        diff = new != old
        near = (np.abs(lhs_n - bound) <= f32(1e-4) * bound) & (np.abs(lhs_o - bound) <= f32(1e-4) * bound)
        assert not (diff & ~near).any(), f"{(diff & ~near).sum()} bits differ away from the bound, e.g. {[float(v[diff & ~near][0]) for v in c]}"
        ax, ay, X0, Y0, x0, x1, y0, y1 = c[0], c[1], c[6], c[7], c[8], c[9], c[10], c[11]
        rx = np.where(ax - X0 < x0, 0, np.where(ax - X0 > x1, 2, 1)); ry = np.where(ay - Y0 < y0, 0, np.where(ay - Y0 > y1, 2, 1))
        tally["regions"] += np.bincount(3 * ry + rx, minlength=9)
        tally["cases"] += CHUNK; tally["hit"] += int(hit.sum()); tally["set_new"] += int(new.sum()); tally["differ"] += int(diff.sum())
    print(tally)
    assert tally["cases"] >= 1_000_000
    # the cases are not one-sided: every region around (and inside) the rectangle is well represented, and both outcomes are common
    assert tally["regions"].min() >= tally["cases"] // 40, tally["regions"]
    assert 0.2 <= tally["hit"] / tally["cases"] <= 0.8 and tally["set_new"] >= tally["hit"], tally
    # the mask stays tight: few rectangles kept without an accepted pixel (pixel centres are discrete, the test is continuous)
    assert tally["set_new"] - tally["hit"] <= 0.25 * tally["cases"], tally


def test_special_means_and_conics():
    """Means exactly on an edge, a corner and the centre of rectangles of every kind; an ill-conditioned conic keeps the rectangle; an
    opacity below the gate and an empty rectangle clear it."""
    one = lambda *v: tuple(np.array([w], f32) for w in v)
    for x0, x1, y0, y1 in ((8, 15, 0, 7), (3, 3, 2, 6), (1, 6, 5, 5), (12, 12, 9, 9)):
        for mx, my in ((x0, y0), (x1, y1), (x0, (y0 + y1) / 2), ((x0 + x1) / 2, y1), ((x0 + x1) / 2, (y0 + y1) / 2)):
            c = one(16 + mx, 16 + my, 0.5, 0.1, 0.3, 1.0 / 255.0, 16, 16, x0, x1, y0, y1)
            for form in (qm.min_q_rect_facing_edges, qm.min_q_rect_four_edges):
                bit, lhs, _ = qm.quad_bit(form, *c)
                assert bit[0] and lhs[0] == 0.0, (form.__name__, x0, x1, y0, y1, mx, my)
    far = one(500.0, 500.0, 1.0, 0.99999, 1.0, 0.5, 0, 0, 0, 7, 0, 7)               # det / (A C) = 2e-5: ill-conditioned
    assert qm.quad_bit(qm.min_q_rect_facing_edges, *far)[0][0]
    faint = one(3.0, 3.0, 1.0, 0.0, 1.0, 0.9 / 255.0, 0, 0, 0, 7, 0, 7)
    assert not qm.quad_bit(qm.min_q_rect_facing_edges, *faint)[0][0]
    empty = one(3.0, 3.0, 1.0, 0.0, 1.0, 0.9, 0, 0, 1, 0, 1, 0)
    assert not qm.quad_bit(qm.min_q_rect_facing_edges, *empty)[0][0]


def test_no_blended_pair_of_an_oracle_view_is_dropped():
    """S(2000, 200, 136, 3, 3) -- 13 x 9 tiles, the bottom row ragged (8 pixel rows), lists shorter than 256 entries, so the boxes are the
    quadrants' pixels inside the image: every (entry, quadrant) that blends a pixel has its bit, in the new form and the old."""
    s = synthetic_scene(2000, 200, 136, 3, 3)
    o = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"], s["tanfovy"],
                   s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=s["sh_degree"], want_margin=False)
    pairs = blended = kept = 0
    for tile in range(o["gx"] * o["gy"]):
        w = qm.walk_tile(o, tile)
        assert w["n"] <= 256
        assert not (w["blended"] & ~w["masks_new"]).any(), tile
        assert not (w["blended"] & ~w["masks_old"]).any(), tile
        pairs += 4 * w["n"]; blended += int(w["blended"].sum()); kept += int(w["masks_new"].sum())
    print(f"{pairs} (entry, quadrant) pairs, {kept} kept, {blended} blend a pixel")
    assert blended > 10_000 and kept >= blended
