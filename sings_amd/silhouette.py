"""The soft silhouette of a posed triangle mesh on the device (include/sings_silhouette.h, csrc/sg_silhouette.hip), differentiable
w.r.t. the camera-space vertices: what the pose refinement (sings_amd/pose_refine.py) blends against the mask.  The definition is
``pose_refine.silhouette_host``'s docstring, unchanged; PARITY-UNPINNED against pytorch3d as that docstring says.

    soft_silhouette       the op: K frames per launch, fp32 on the GPU, host tensors raise
    SilhouetteWorkspace   the pre-allocated state of one (K, V, F, H, W, capacity): what an engine keeps across launches
    pair_counts_host      a numpy twin of the setup and binning: (tile, face) pairs per frame, tile list lengths (CPU)
    workspace_plan        the byte sizes of a workspace; refuses a case whose offsets do not fit int32 (CPU)
    corner_csr            vertex -> face corners, built once per topology

THE CAPACITY: the pair list of a launch has a fixed length.  A pair beyond it is dropped by the kernel (the index is tested before the
write) and an overflow word is set; ``soft_silhouette`` reads that word once per call and runs the call again with the capacity the
count asks for, so its result is never a silhouette with pairs missing.  An engine that may not synchronise passes ``workspace=`` with
``check=False`` and reads ``workspace.overflowed()`` when it is ready to.
"""
import math

import numpy as np
import torch

from . import _lib, _marshal

LOGIT = math.log(1.0 / 1e-4 - 1.0)
ZNEAR, MIN_AREA = 1e-3, 1e-8
TILE = _lib.SIL_TILE
GUARD = 0xA5                                     # the byte the guard words are filled with


def workspace_plan(K, V, F, H, W, capacity):
    """-> dict piece -> byte offset (``info``, ``rec``, ``rect``, ``tile_count``, ``tile_start``, ``cursor``, ``Q``, ``face_grad``, ``list``,
    ``partial``) and ``bytes``, the total; ``tiles`` (gx, gy).  ValueError for a case whose element offsets do not fit int32."""
    plan = _marshal.sil_layout(K, V, F, H, W, capacity)
    plan["tiles"] = ((int(W) + TILE - 1) // TILE, (int(H) + TILE - 1) // TILE)
    return plan


def _host_rects(verts_cam, faces, intrinsics, H, W, sigma):
    """The setup kernel in numpy fp32, operation for operation -> (valid [K,F], x0, y0, x1, y1 [K,F] int64; x1 < x0: no tile)."""
    f32 = np.float32
    v = np.asarray(verts_cam, f32)
    v = v[None] if v.ndim == 2 else v
    faces = np.asarray(faces, np.int64)
    fx, fy, cx, cy = (f32(x) for x in intrinsics)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    s = f32(2.0) / f32(min(H, W))
    s2 = s * s
    rad = f32(math.sqrt(LOGIT * float(f32(sigma))) / (2.0 / float(min(H, W))))
    inb = ((faces >= 0) & (faces < v.shape[1])).all(-1)
    tri = v[:, np.where(inb[:, None], faces, 0)]                     # [K,F,3,3]
    with np.errstate(all="ignore"):
        x, y, z = tri[..., 0], tri[..., 1], tri[..., 2]
        valid = inb[None] & np.isfinite(tri).all((-1, -2)) & (z > f32(ZNEAR)).all(-1)
        u, w = fx * x / z + cx, fy * y / z + cy
        valid &= np.isfinite(u).all(-1) & np.isfinite(w).all(-1)
        e1x, e1y, e2x, e2y = u[..., 1] - u[..., 0], w[..., 1] - w[..., 0], u[..., 2] - u[..., 0], w[..., 2] - w[..., 0]
        valid &= np.abs(e1x * e2y - e1y * e2x) * s2 > f32(MIN_AREA)
        u, w = np.where(valid[..., None], u, f32(0)), np.where(valid[..., None], w, f32(0))
        tile = lambda a, g: np.floor(np.minimum(np.maximum(a * f32(0.0625), f32(-1.0)), f32(g))).astype(np.int64)
        x0, x1 = np.maximum(tile(u.min(-1) - rad, gx), 0), np.minimum(tile(u.max(-1) + rad, gx), gx - 1)
        y0, y1 = np.maximum(tile(w.min(-1) - rad, gy), 0), np.minimum(tile(w.max(-1) + rad, gy), gy - 1)
    none = ~valid | (x1 < x0) | (y1 < y0)
    return valid, np.where(none, 0, x0), np.where(none, 0, y0), np.where(none, -1, x1), np.where(none, -1, y1)


def pair_counts_host(verts_cam, faces, intrinsics, H, W, sigma=1e-4):
    """A numpy twin of the device's setup and binning: ``verts_cam`` [K,V,3] (or [V,3]) -> (pairs per frame [K] int64, tile list
    lengths [K,gy,gx] int64).  A face is listed in every 16 x 16 tile its screen bounding box, grown by the band radius
    sqrt(LOGIT sigma) / s pixels, meets: a superset of the tiles in which the face blends into a pixel."""
    _, x0, y0, x1, y1 = _host_rects(verts_cam, faces, intrinsics, H, W, sigma)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    K = x0.shape[0]
    # a rectangle adds +1 to its tiles: the inclusive 2-D prefix sum of four corner marks
    mark = np.zeros((K, gy + 1, gx + 1), np.int64)
    kk = np.broadcast_to(np.arange(K)[:, None], x0.shape)
    has = x1 >= x0
    for ys, xs, sign in ((y0, x0, 1), (y0, x1 + 1, -1), (y1 + 1, x0, -1), (y1 + 1, x1 + 1, 1)):
        np.add.at(mark, (kk[has], ys[has], xs[has]), sign)
    lengths = mark.cumsum(1).cumsum(2)[:, :gy, :gx]
    return lengths.sum((1, 2)), lengths


def corner_csr(faces, V):
    """``faces`` [F,3] (numpy or tensor) -> (row_ptr [V+1], corner [n]) int32 numpy: the entries 3 f + c of vertex v's face corners in
    ascending order, rows one behind the other.  A corner outside [0, V) has no row."""
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64).reshape(-1)
    ok = (f >= 0) & (f < V)
    entries = np.nonzero(ok)[0]
    order = np.argsort(f[entries], kind="stable")
    row_ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(f[entries], minlength=V), out=row_ptr[1:])
    return row_ptr.astype(np.int32), entries[order].astype(np.int32)


class SilhouetteWorkspace:
    """The device state of launches of one size: the workspace bytes (guard words filled), the topology's corner CSR, the outputs."""

    def __init__(self, K, V, faces, H, W, capacity, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("silhouette: the workspace lives on the GPU (no CPU fallback)")
        self.faces = _marshal._mesh_arg(faces, "silhouette: faces", torch.int32, device, (3,))
        self.K, self.V, self.F, self.H, self.W, self.capacity = int(K), int(V), int(self.faces.shape[0]), int(H), int(W), int(capacity)
        self.plan = workspace_plan(self.K, self.V, self.F, self.H, self.W, self.capacity)
        self.ws = torch.zeros(self.plan["bytes"], dtype=torch.uint8, device=device)
        for piece, words in (("list", self.capacity), ("partial", 6 * self.capacity)):
            self._guard(piece, words).fill_(GUARD)
        row_ptr, corner = corner_csr(self.faces, self.V)
        self.row_ptr, self.corner = torch.from_numpy(row_ptr).to(device), torch.from_numpy(corner).to(device)

    def _guard(self, piece, words):
        at = self.plan[piece] + 4 * words
        return self.ws[at:at + 4 * _lib.SIL_GUARD_WORDS]

    def guards_intact(self):
        """The words behind the pair list and behind the partials are as they were filled (one host read)."""
        return all(bool((self._guard(p, w) == GUARD).all()) for p, w in (("list", self.capacity), ("partial", 6 * self.capacity)))

    def _words(self, piece, n, dtype=torch.int32):
        return self.ws[self.plan[piece]:self.plan[piece] + 4 * n].view(dtype)

    def info(self):
        """One host read -> (overflowed, pairs of all frames, pairs per frame [K] numpy)."""
        w = self._words("info", _lib.SIL_INFO_WORDS + self.K).cpu().numpy()
        return bool(w[0]), int(w[1]), w[_lib.SIL_INFO_WORDS:].astype(np.int64)

    def overflowed(self):
        return self.info()[0]

    def reset_peak(self):
        """Zero the two words that collect over launches (an overflow of any launch, the most pairs of any launch)."""
        self._words("info", _lib.SIL_INFO_WORDS)[2:4].zero_()

    def peak(self):
        """One host read -> (a launch since ``reset_peak`` overflowed, the most pairs of any launch since)."""
        w = self._words("info", _lib.SIL_INFO_WORDS).cpu().numpy()
        return bool(w[2]), int(w[3])

    def tile_lengths(self):
        """[K,gy,gx] int64 numpy: the list lengths of the last forward (one host read)."""
        gx, gy = self.plan["tiles"]
        return self._words("tile_count", self.K * gx * gy).cpu().numpy().astype(np.int64).reshape(self.K, gy, gx)

    def tile_lists(self):
        """The lists of the last forward, as far as they lie within the capacity: list of K lists of gy * gx int64 arrays (host reads)."""
        gx, gy = self.plan["tiles"]
        n = self.tile_lengths().reshape(-1)
        start = np.concatenate([[0], np.cumsum(n)[:-1]])
        lst = self._words("list", self.capacity).cpu().numpy().astype(np.int64)
        flat = [lst[min(s, self.capacity):min(s + c, self.capacity)] for s, c in zip(start, n)]
        return [flat[k * gx * gy:(k + 1) * gx * gy] for k in range(self.K)]


class _SoftSilhouette(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, work, intrinsics, sigma, counts):
        verts = verts.contiguous()
        alpha = torch.empty((work.K, work.H, work.W), dtype=torch.float32, device=verts.device)
        _marshal.sil_forward(verts, work.faces, intrinsics, work.H, work.W, sigma, work.capacity, work.ws, alpha, counts)
        ctx.save_for_backward(verts)
        ctx.work, ctx.intrinsics, ctx.sigma = work, intrinsics, sigma
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        verts, = ctx.saved_tensors
        work = ctx.work
        dverts = torch.empty_like(verts)
        _marshal.sil_backward(verts, work.faces, ctx.intrinsics, work.H, work.W, ctx.sigma, work.capacity, work.ws,
                              dalpha.contiguous().float(), work.row_ptr, work.corner, dverts)
        return dverts, None, None, None, None


def default_capacity(K, F):
    """What ``soft_silhouette`` tries first: 16 tiles per face (a body at kit size meets 7 to 8)."""
    return max(4096, 16 * int(K) * int(F))


def soft_silhouette(verts_cam, faces, intrinsics, H, W, sigma=1e-4, return_counts=False, capacity=None, workspace=None, check=True):
    """``verts_cam`` [K,V,3] (or [V,3]) fp32 on the GPU, ``faces`` [F,3] integers on the GPU, ``intrinsics`` (fx, fy, cx, cy) in pixels
    -> alpha [K,H,W] (or [H,W]), differentiable w.r.t. ``verts_cam``; with ``return_counts`` also the largest number of blended faces
    of a pixel per frame, [K] int32 (a second variant of the composite kernel, run only on request).

    ``workspace``: a ``SilhouetteWorkspace`` of this size to launch into (the backward reads it: one forward, then its backward);
    without one the call allocates its own with ``capacity`` pairs (default ``default_capacity``).  With ``check`` (the default) the
    overflow word is read once after the launch -- a host synchronisation -- and an overflowed call without a ``workspace`` is run again
    with the capacity its count asks for; with a ``workspace`` it raises.  ``check=False`` reads nothing: the caller asks
    ``workspace.overflowed()`` before it trusts the result."""
    if not torch.is_tensor(verts_cam) or not verts_cam.is_cuda or not torch.is_tensor(faces) or not faces.is_cuda:
        raise RuntimeError("silhouette.soft_silhouette: verts_cam and faces must be GPU tensors (no CPU fallback; the host definition is "
                           "pose_refine.silhouette_host)")
    if verts_cam.dtype != torch.float32:
        raise RuntimeError(f"silhouette.soft_silhouette: verts_cam must be float32 (got {verts_cam.dtype})")
    single = verts_cam.dim() == 2
    v = verts_cam[None] if single else verts_cam
    if v.dim() != 3 or v.shape[2] != 3:
        raise ValueError(f"silhouette.soft_silhouette: verts_cam must be [K,V,3] or [V,3], got {tuple(verts_cam.shape)}")
    K, V = int(v.shape[0]), int(v.shape[1])
    intrinsics = tuple(float(x) for x in intrinsics)
    work = workspace
    if work is None:
        faces32 = faces.to(torch.int32).contiguous()
        work = SilhouetteWorkspace(K, V, faces32, H, W, default_capacity(K, faces32.shape[0]) if capacity is None else capacity, v.device)
    elif (work.K, work.V, work.H, work.W) != (K, V, int(H), int(W)):
        raise ValueError(f"silhouette.soft_silhouette: the workspace is for K, V, H, W = {(work.K, work.V, work.H, work.W)}")
    counts = torch.empty(K, dtype=torch.int32, device=v.device) if return_counts else None
    alpha = _SoftSilhouette.apply(v, work, intrinsics, float(sigma), counts)
    if check:
        over, total, _ = work.info()
        if over and workspace is not None:
            raise RuntimeError(f"silhouette.soft_silhouette: {total} (tile, face) pairs, the workspace holds {work.capacity}")
        if over:
            return soft_silhouette(verts_cam, faces, intrinsics, H, W, sigma, return_counts, total, None, True)
    alpha = alpha[0] if single else alpha
    return (alpha, counts) if return_counts else alpha
