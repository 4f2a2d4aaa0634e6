"""numpy fp32 twins of the forward composite's quadrant test (sings_amd/csrc/sg_render.hip: sg_min_q_rect, sg_quad_mask) -- the form
that evaluates all four edges of the rectangle and the form that evaluates the two that face the mean -- a brute-force scan of a
rectangle's pixels with the blend loop's own acceptance test, and a per-tile walk of an oracle view that says which (entry, quadrant)
pairs blend a pixel and what the live boxes are when a batch is staged.  Shared by tests/test_quad_mask_edges_host.py,
tests/test_quad_mask_edges_scenes_host.py and tests/test_gpu_quad_mask_edges.py; no GPU.

Arrays are float32 and every operation rounds to float32, in the kernel's order; a fused multiply-add is formed in float64 (the product
of two float32 is exact there) and rounded once more, v_rcp_f32 and __logf are taken as correctly rounded.  The twins are therefore
within a few ulp of the device functions, not their bits: the tests' statements carry margins far above that."""
import numpy as np

f32 = np.float32
BIG = f32(3.0e38)
LOG2E = 1.44269504088896340736
KA, KB = f32(-0.5 * LOG2E), f32(-LOG2E)


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _clamp(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def _q(A, B2, C, dx, dy):
    return fma(A * dx, dx, fma(B2 * dx, dy, C * dy * dy))


def min_q_rect_four_edges(A, B, C, mx, my, x0, x1, y0, y1):
    """The parent form: 0 if the mean is inside, else the minimum over the four edges, each a clamped parabola."""
    rA, rC = f32(1) / A, f32(1) / C
    B2 = f32(2) * B
    best = np.full(A.shape, BIG, f32)
    for xe, ye in ((x0, y0), (x1, y1)):
        dx = xe - mx
        dy = _clamp(-B * dx * rC, y0 - my, y1 - my)
        best = np.minimum(best, _q(A, B2, C, dx, dy))
        dy2 = ye - my
        dx2 = _clamp(-B * dy2 * rA, x0 - mx, x1 - mx)
        best = np.minimum(best, _q(A, B2, C, dx2, dy2))
    inside = (mx >= x0) & (mx <= x1) & (my >= y0) & (my <= y1)
    return np.where(inside, f32(0), best)


def min_q_rect_facing_edges(A, B, C, mx, my, x0, x1, y0, y1):
    """The form in the tree: the two clamped parabolas through the rectangle's point nearest the mean."""
    rA, rC = f32(1) / A, f32(1) / C
    lx, hx, ly, hy = x0 - mx, x1 - mx, y0 - my, y1 - my
    B2 = f32(2) * B
    dx = _clamp(f32(0), lx, hx)
    dy = _clamp(-B * dx * rC, ly, hy)
    qv = _q(A, B2, C, dx, dy)
    dy2 = _clamp(f32(0), ly, hy)
    dx2 = _clamp(-B * dy2 * rA, lx, hx)
    qh = _q(A, B2, C, dx2, dy2)
    return np.minimum(qv, qh)


def quad_bit(min_q_rect, ax, ay, A, B, C, op, X0, Y0, x0, x1, y0, y1):
    """sg_quad_mask's decision for ONE rectangle per case (tile-relative x0..y1, tile origin X0, Y0, absolute mean ax, ay).
    -> (bit, 0.999 * min q, bound); the last two are NaN-free only where the opacity gate passes."""
    with np.errstate(all="ignore"):
        o255 = f32(255) * op
        reach = o255 >= f32(0.999)
        bound = f32(2) * (np.log(o255).astype(f32) * f32(1.002) + f32(0.004)) + f32(0.01)
        det = A * C - B * B
        illc = ~(det > f32(1e-3) * A * C) | ~(A > 0) | ~(C > 0)
        mx, my = ax - X0, ay - Y0
        mq = np.where(illc, f32(0), min_q_rect(A, B, C, mx, my, x0, x1, y0, y1))
        lhs = mq * f32(0.999)
        bit = reach & (x0 <= x1) & (lhs <= bound)
    return bit, lhs, bound


def accepts(ax, ay, A, B, C, op, px, py):
    """Does the blend loop accept the pixel centre (px, py)?  power <= 0 and alpha >= 1/255, by the kernels' fp32 expression
    (SG_FWD_PASS: the conic scaled by log2 e, exp2) or by the same test in float64 -- either."""
    with np.errstate(all="ignore"):
        dx, dy = ax - px, ay - py
        Ap, Bp, Cp = KA * A, KB * B, KA * C
        power = fma(Cp * dy, dy, fma(Ap, dx, Bp * dy) * dx)
        alpha = np.minimum(f32(0.99), op * np.exp2(power).astype(f32))
        k32 = ~(power > 0) & ~(alpha < f32(1.0 / 255.0))
        dx, dy, A, B, C = (v.astype(np.float64) for v in (dx, dy, A, B, C))
        p64 = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
        k64 = (p64 <= 0) & (op.astype(np.float64) * np.exp(p64) >= 1.0 / 255.0)
    return k32 | k64


def live_box(live, q):
    """sg_live_box: (x0, x1, y0, y1), tile-relative, of the set pixels of an 8 x 8 boolean quadrant; empty -> (1, 0, 1, 0)."""
    if not live.any():
        return (1.0, 0.0, 1.0, 0.0)
    cols, rows = np.flatnonzero(live.any(0)), np.flatnonzero(live.any(1))
    qx, qy = 8 * (q & 1), 8 * (q >> 1)
    return (float(qx + cols[0]), float(qx + cols[-1]), float(qy + rows[0]), float(qy + rows[-1]))


def walk_tile(o, tile, refresh=256):
    """Composite tile `tile` of an oracle view front to back in fp32, as the dense forward does.  ->
    dict(n, ids, blended [n, 4] bool: the pair (entry, quadrant) blended a pixel; boxes [n, 4, 4]: the quadrants' live boxes when the
    entry is staged (refreshed every `refresh` entries); masks_new / masks_old [n, 4] bool: the twins' decisions against those boxes;
    deepest [4]: one past the quadrants' last contributors)."""
    W, H, gx = o["W"], o["H"], o["gx"]
    X0, Y0 = (tile % gx) * 16, (tile // gx) * 16
    lo, hi = (int(v) for v in o["ranges"][tile])
    ids = o["point_list"][lo:hi].astype(np.int64)
    n = len(ids)
    yy, xx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    px, py = (X0 + xx).astype(f32), (Y0 + yy).astype(f32)
    done = ~((X0 + xx < W) & (Y0 + yy < H))
    Tr = np.ones((16, 16), f32)
    quad = 2 * (yy >> 3) + (xx >> 3)
    blended = np.zeros((n, 4), bool)
    boxes = np.zeros((n, 4, 4), f32)
    deepest = np.zeros(4, np.int64)
    box = None
    xy, co = o["xy"].astype(f32), o["conic_opacity"].astype(f32)
    for i, g in enumerate(ids):
        if i % refresh == 0:
            box = np.array([live_box(~done[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8], q) for q in range(4)], f32)
        boxes[i] = box
        ax, ay = xy[g]
        A, B, C, op = co[g]
        dx, dy = ax - px, ay - py
        power = fma(np.full_like(px, KA * C) * dy, dy, fma(np.full_like(px, KA * A), dx, KB * B * dy) * dx)
        alpha = np.minimum(f32(0.99), op * np.exp2(power).astype(f32))
        test_T = Tr * (f32(1) - alpha)
        valid = ~done & ~(power > 0) & ~(alpha < f32(1.0 / 255.0))
        term = valid & (test_T < f32(0.0001))
        blend = valid & ~term
        Tr = np.where(blend, test_T, Tr)
        done |= term
        for q in range(4):
            if blend[quad == q].any():
                blended[i, q] = True
                deepest[q] = i + 1
    out = dict(n=n, ids=ids, blended=blended, boxes=boxes, deepest=deepest, X0=X0, Y0=Y0)
    if n:
        rep = lambda v: np.repeat(np.asarray(v, f32), 4)
        args = (rep(xy[ids, 0]), rep(xy[ids, 1]), rep(co[ids, 0]), rep(co[ids, 1]), rep(co[ids, 2]), rep(co[ids, 3]),
                np.full(4 * n, X0, f32), np.full(4 * n, Y0, f32)) + tuple(boxes.reshape(4 * n, 4)[:, j].copy() for j in range(4))
        out["masks_new"] = quad_bit(min_q_rect_facing_edges, *args)[0].reshape(n, 4)
        out["masks_old"] = quad_bit(min_q_rect_four_edges, *args)[0].reshape(n, 4)
    else:
        out["masks_new"] = out["masks_old"] = np.zeros((0, 4), bool)
    return out
