"""The reference's pose refinement: the ``--opt`` step of its ``prepare_kits.sh`` (preprocess/utils/ooptimize_smpl.py:260-364 and
ooptimize_smplh.py), which refines a kit's SMPL poses against the Sapiens keypoints and, through pytorch3d's ``MeshRasterizer`` +
``SoftSilhouetteShader``, against the mask.  Stated and executable on the host, and run on the device.

    RefineSpec            the reference's tables: keypoint map, gradient mask, joint limits, lr, iterations; ``.smpl()`` / ``.smplh()``
    silhouette_host       a soft silhouette of a posed triangle mesh, differentiable, vectorised over pixels x faces
    refine_pose_host      the reference's loop in torch on the CPU, fp64-capable, one frame after the other
    RefineEngine          the loop on the device, pre-allocated for K frames per launch, one iteration recorded as a HIP graph
    refine_pose           the device loop over any number of frames -> (global_orient, body_pose, report)
    refine_kit            a kit directory -> ``score_demo_video/poses_optimized.npz``, the file ``kit.load_kit`` prefers
    write_refined_poses   that file's writer (host): the reference's keys, atomic, refuses to overwrite

The host functions are the definition the device path is held to, and what anyone without pytorch3d reads; at a kit's size
(512 x 896, 13 776 faces, 100 iterations a frame) they are a definition, not a tool: every (pixel, face) pair is evaluated.  The device
path (``sings_amd/silhouette.py``, csrc/sg_silhouette.hip) files the faces into tiles and evaluates the pairs of a tile's list.

Per frame, independently of the others:

    parameter   pose = cat(global_orient, body_pose) [72]; betas fixed; the mesh posed with zero translation, the frame's ``transl``
                as the camera translation, R = world_view_transform[:3,:3]
    keypoints   COCO-133 keypoints with a score below ``score_threshold`` are zeroed, mapped to ``n_joint_rows`` rows of model joints
                (the regressed joints, then vertices picked by ``extra_joint_vertex_ids``), rows that sum to 0 masked out; the posed
                joints projected as ``pcd_3d_to_pcd_2d_torch(keep_z=False, norm_coord=False)`` does: a joint with z <= 0, u < 0,
                u >= W - 1 or v >= H - 1 comes back as (0, 0) -- the reference tests u >= 0 twice and v >= 0 never, kept;
                term = mse(proj[m], target[m]) / m.sum(), in pixels (no row: 0, where the reference's mean of nothing is NaN)
    silhouette  ``mse(alpha, mask)`` with the soft silhouette at ``sigma``
    update      Adam(lr); before the step grad *= grad_mask[:72] * ((pose < hi) & (pose > lo))

Two things of the reference that look unfinished stay as they are: its list holds ``'wrist'`` but the test reads ``'Wrist'``, so the
wrists never get a gradient; and the limits [0, 0] on the knees' y and z are never strictly satisfied, so only the knees' x moves.

THE SILHOUETTE is PARITY-UNPINNED: pytorch3d is not a dependency and none of its results is at hand; ``silhouette_host``'s docstring is
the definition and no more is claimed.  It blends EVERY face of the band where pytorch3d keeps the 150 nearest in depth per pixel
(``faces_per_pixel=150``); the two agree wherever a pixel has at most 150, and the count is returned.  The SMPL-H preset keeps the
betas FIXED: the reference's six learned hand betas are out of scope.
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from .body import _joint_transforms_torch, rodrigues

LOGIT = math.log(1.0 / 1e-4 - 1.0)
ZNEAR, MIN_AREA = 1e-3, 1e-8
POSE = 72                                        # global_orient + 23 body joints


# ---- the reference's tables -----------------------------------------------------------------------------------------------------------
def _limits():
    lim = np.ones([24, 3, 2])
    lim[..., 0] *= -360
    lim[..., 1] *= 360
    lim[4, 0] = lim[5, 0] = [0, 160]                                 # knees: one degree of freedom
    lim[4, 1] = lim[4, 2] = lim[5, 1] = lim[5, 2] = [0, 0]
    lim[7, 0] = lim[8, 0] = [-45, 90]                                # ankles
    lim[7, 1] = lim[8, 1] = [-60, 60]
    lim[7, 2] = lim[8, 2] = [-10, 10]
    lim[18, 1] = [-160, 0]                                           # elbows
    lim[19, 2] = [0, 160]
    return lim.reshape(-1, 2) / 180 * np.pi


def _grad_mask(rows, elbow):
    m = np.zeros([rows, 3])
    m[[18, 19]] = elbow                                              # 'Elbow'
    #   ('wrist' is in the reference's list, 'Wrist' is what it tests: rows 20 and 21 stay 0)
    m[[4, 5, 7, 8]] = 1                                              # 'Knee', 'Ankle'
    m[[29, 32, 30, 33, 31, 34]] = 1                                  # 'Big Toe', 'Little Toe', 'Heel' (rows beyond the 24 joints: never read)
    return m.reshape(-1)


_BODY_MAP = ((7, 18), (8, 19), (9, 20), (10, 21), (13, 4), (14, 5), (15, 7), (16, 8))      # elbows, wrists, knees, ankles
_SMPL_MAP = _BODY_MAP + ((17, 29), (18, 30), (19, 31), (20, 32), (21, 33), (22, 34))        # the feet
_SMPLH_MAP = _BODY_MAP + ((17, 57), (18, 58), (19, 59), (20, 60), (21, 61), (22, 62),       # the feet
                          (91, 20), (112, 21),                                               # the hand roots, over the wrists
                          (115, 51), (119, 39), (123, 42), (127, 45), (131, 48),             # right thumb, fore, middle, ring, pinky
                          (94, 36), (98, 24), (102, 27), (106, 30), (110, 33))               # left


@dataclass(frozen=True)
class RefineSpec:
    """What one of the reference's two scripts fixes.  ``keypoint_map``: (COCO-133 index, joint row) pairs applied in order, a later
    pair overwriting an earlier one's row.  ``grad_mask`` [n_joint_rows * 3] (its first 72 entries gate the pose), ``limits`` [72,2]
    radians, both fp64 as the reference builds them."""
    keypoint_map: tuple
    n_joint_rows: int
    grad_mask: np.ndarray = field(repr=False)
    limits: np.ndarray = field(repr=False)
    lr: float = 5e-3
    iterations: int = 100
    score_threshold: float = 0.8
    sigma: float = 1e-4

    @classmethod
    def smpl(cls):
        """``ooptimize_smpl.py`` to the letter: 45 joint rows (24 joints + 21 picked vertices), lr 5e-3, 100 iterations."""
        return cls(_SMPL_MAP, 45, _grad_mask(45, 1.0), _limits(), 5e-3, 100)

    @classmethod
    def smplh(cls):
        """``ooptimize_smplh.py``'s tables: 73 joint rows (52 joints + 21 picked vertices) with fingertips and hand roots, elbow mask
        0.5, lr 2e-3, 50 iterations.  The betas stay FIXED: the reference also learns six hand betas, which is out of scope here."""
        return cls(_SMPLH_MAP, 73, _grad_mask(73, 0.5), _limits(), 2e-3, 50)

    def rows_of(self, values):
        """``values`` [..., 133, C] -> [..., n_joint_rows, C]: zeros, then every pair of the map in order."""
        out = values.new_zeros(values.shape[:-2] + (self.n_joint_rows, values.shape[-1]))
        for coco, row in self.keypoint_map:
            out[..., row, :] = values[..., coco, :]
        return out

    def enabled(self):
        """[72] bool: where the mask is non-zero and the limit interval is not empty -- the entries that can move."""
        return (self.grad_mask[:POSE] != 0) & (self.limits[:, 1] > self.limits[:, 0])


# ---- the soft silhouette, executable definition -----------------------------------------------------------------------------------------
def silhouette_host(verts_cam, faces, intrinsics, H, W, sigma=1e-4, return_counts=False):
    """``verts_cam`` [K,V,3] (or [V,3]) camera-space vertices of any float dtype, ``faces`` [F,3], ``intrinsics`` (fx, fy, cx, cy) in
    pixels -> alpha [K,H,W] in that dtype, differentiable; with ``return_counts`` also the largest number of blended faces of a pixel,
    per frame [K] int64.  Memory is H W F values several times over.  The definition:

        projection   u = fx x / z + cx,  v = fy y / z + cy; pixel (i, j) has its centre at (j + 0.5, i + 0.5)
        units        one NDC unit is min(H, W) / 2 pixels (pytorch3d spans the SHORTER side by [-1, 1]): s = 2 / min(H, W), and every
                     squared distance below is a pixel distance^2 times s^2
        skipped      a face with a vertex at z <= 1e-3, with a non-finite vertex, or with a doubled screen area <= 1e-8 (NDC^2); back
                     faces count
        distance     d2: the squared distance from the pixel centre to the nearest of the face's three edges, as segments;
                     inside: the three edge functions have the same strict sign;  signed = inside ? -d2 : +d2;  an outside face
                     with d2 >= r, r = ln(1 / 1e-4 - 1) sigma, is skipped (the SQUARED distance against r, as pytorch3d)
        blend        prob = 1 / (1 + exp(signed / sigma));  alpha = 1 - prod_faces (1 - prob), in ascending face index
        gradient     reaches x, y, z through u, v only"""
    single = verts_cam.dim() == 2
    v = verts_cam[None] if single else verts_cam
    dt, dev = v.dtype, v.device
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    c = lambda x: torch.tensor(x, dtype=dt, device=dev)
    s = c(2.0) / c(float(min(H, W)))
    s2, r, sig = s * s, c(LOGIT) * c(float(sigma)), c(float(sigma))
    faces = torch.as_tensor(faces, device=dev).long()
    px = (torch.arange(W, dtype=dt, device=dev) + 0.5)[None, :, None]
    py = (torch.arange(H, dtype=dt, device=dev) + 0.5)[:, None, None]
    safe = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], dtype=dt, device=dev)
    alphas, counts = [], []
    for k in range(v.shape[0]):
        tri = v[k][faces]                                            # [F,3,3]
        z = tri[..., 2]
        valid = torch.isfinite(tri).all(-1).all(-1) & (z > ZNEAR).all(-1)
        zs = torch.where(valid[:, None], z, torch.ones_like(z))
        uv = torch.stack([c(fx) * tri[..., 0] / zs + c(cx), c(fy) * tri[..., 1] / zs + c(cy)], -1)          # [F,3,2]
        valid = valid & torch.isfinite(uv).all(-1).all(-1)
        uv = torch.where(valid[:, None, None], uv, safe[None])
        e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        area2 = (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]).abs() * s2
        valid = valid & (area2 > c(MIN_AREA))
        uv = torch.where(valid[:, None, None], uv, safe[None])
        d2s, pos, neg = [], True, True
        for e in range(3):
            a, b = uv[:, e], uv[:, (e + 1) % 3]
            ex, ey = (b - a)[:, 0], (b - a)[:, 1]
            wx, wy = px - a[:, 0], py - a[:, 1]                      # [H,W,F] by broadcast
            cr = ex * wy - ey * wx
            pos, neg = (cr > 0) & pos, (cr < 0) & neg
            t = ((wx * ex + wy * ey) / (ex * ex + ey * ey)).clamp(0, 1)
            dx, dy = wx - t * ex, wy - t * ey
            d2s.append(dx * dx + dy * dy)
        d2n = torch.stack(d2s).min(0).values * s2
        inside = pos | neg
        on = valid & (inside | (d2n < r))
        x = torch.where(on, torch.where(inside, -d2n, d2n) / sig, torch.zeros_like(d2n))
        q = torch.where(on, 1 - 1 / (1 + torch.exp(x)), torch.ones_like(x))
        alphas.append(1 - torch.prod(q, -1))
        counts.append(on.sum(-1).max())
    alpha = torch.stack(alphas)
    alpha = alpha[0] if single else alpha
    return (alpha, torch.stack(counts)) if return_counts else alpha


# ---- pieces the two loops share (torch, any dtype and device) ---------------------------------------------------------------------------
def keypoint_targets(keypoints, scores, spec):
    """``keypoints`` [F,133,2], ``scores`` [F,133] -> (target [F,rows,2], used [F,rows] bool): low scores zeroed, the map applied, rows
    that sum to 0 masked out."""
    if keypoints.shape[-2:] != (133, 2) or scores.shape != keypoints.shape[:-1]:
        raise ValueError(f"pose_refine: keypoints {list(keypoints.shape)} / scores {list(scores.shape)} must be [F,133,2] / [F,133]")
    kp = torch.where((scores < spec.score_threshold)[..., None], torch.zeros_like(keypoints), keypoints)
    target = spec.rows_of(kp)
    return target, target.sum(-1) != 0


def project_joints(pts_cam, intrinsics, H, W):
    """[...,3] camera space -> [...,2] pixels, (0, 0) for z <= 0, u < 0, u >= W - 1 or v >= H - 1."""
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    z = pts_cam[..., 2]
    front = z > 0
    zs = torch.where(front, z, torch.ones_like(z))
    u, v = fx * pts_cam[..., 0] / zs + cx, fy * pts_cam[..., 1] / zs + cy
    keep = front & (u >= 0) & (u < W - 1) & (v < H - 1)
    return torch.where(keep[..., None], torch.stack([u, v], -1), torch.zeros_like(pts_cam[..., :2]))


def keypoint_term(proj, target, used):
    """Per frame: mse(proj[m], target[m]) / m.sum() = sum of squares / (2 n) / n; 0 without a row.  -> ([F], n [F])."""
    n = used.sum(-1)
    sq = (((proj - target) ** 2) * used[..., None].to(proj.dtype)).sum((-1, -2))
    nn = n.clamp(min=1).to(proj.dtype)
    return sq / (2 * nn * nn), n


def silhouette_term(alpha, mask):
    """Per frame: mse(alpha, mask) over the H W pixels."""
    return ((alpha - mask) ** 2).mean((-1, -2))


def gate(pose, spec_mask, lo, hi):
    """grad_mask[:72] * ((pose < hi) & (pose > lo)), in ``pose``'s dtype."""
    return spec_mask * ((pose < hi) & (pose > lo)).to(pose.dtype)


def _spec_tensors(spec, dtype, device):
    return (torch.as_tensor(spec.grad_mask[:POSE], dtype=dtype, device=device),
            torch.as_tensor(spec.limits[:, 0], dtype=dtype, device=device), torch.as_tensor(spec.limits[:, 1], dtype=dtype, device=device))


def _camera_parts(camera):
    Kmat = np.asarray(camera["cam_intrinsics"], np.float64)
    R = camera["world_view_transform"]
    R = R.detach().cpu().numpy() if torch.is_tensor(R) else np.asarray(R)
    return (float(Kmat[0, 0]), float(Kmat[1, 1]), float(Kmat[0, 2]), float(Kmat[1, 2])), np.asarray(R, np.float64)[:3, :3], \
        int(camera["image_height"]), int(camera["image_width"])


def _check_inputs(global_orient, body_pose, transl, keypoints, scores, n_masks):
    F = int(global_orient.shape[0])
    if tuple(global_orient.shape) != (F, 3) or tuple(body_pose.shape) != (F, 69) or tuple(transl.shape) != (F, 3):
        raise ValueError(f"pose_refine: global_orient {list(global_orient.shape)}, body_pose {list(body_pose.shape)}, transl "
                         f"{list(transl.shape)} must be [F,3], [F,69], [F,3]")
    if keypoints.shape[0] != F or scores.shape[0] != F or n_masks != F:
        raise ValueError(f"pose_refine: {F} poses, {keypoints.shape[0]} keypoint rows, {n_masks} masks")
    if F < 1:
        raise ValueError("pose_refine: no frame")
    return F


def _report(first, last, n_used, max_faces):
    """Per frame: dicts of numpy arrays."""
    return {"first_loss": first.sum(-1), "last_loss": last.sum(-1), "first_keypoint_term": first[:, 0], "first_silhouette_term": first[:, 1],
            "last_keypoint_term": last[:, 0], "last_silhouette_term": last[:, 1], "keypoints_used": n_used,
            "max_faces_per_pixel": max_faces}


# ---- the loop on the host ---------------------------------------------------------------------------------------------------------------
def host_model(body):
    """A ``BodyModel`` or the dict of its arrays -> dict of numpy arrays (``v_template``, ``shapedirs``, ``J_regressor``,
    ``lbs_weights``, ``parents``, ``faces``, ``posedirs`` | None, ``pose_mean`` | None)."""
    get = (lambda k: body.get(k)) if isinstance(body, dict) else (lambda k: getattr(body, k, None))
    out = {}
    for k in ("v_template", "shapedirs", "J_regressor", "lbs_weights", "parents", "faces", "posedirs", "pose_mean"):
        a = get(k)
        out[k] = None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
    return out


def host_forward(model, betas, pose, transl, R, extra_ids, dtype=torch.float64):
    """One frame in torch on the CPU: ``pose`` [72] (a leaf or not) -> (verts_cam [V,3], joint rows in camera space [J + extras, 3])."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)
    vt, sd, Jr, w = t(model["v_template"]), t(model["shapedirs"]), t(model["J_regressor"]), t(model["lbs_weights"])
    parents = [int(p) for p in model["parents"]]
    J = Jr.shape[0]
    full = pose if 3 * J == POSE else torch.cat([pose, torch.zeros(3 * J - POSE, dtype=dtype)])
    if model.get("pose_mean") is not None:
        full = full + t(model["pose_mean"]).reshape(-1)
    v_shaped = vt + torch.einsum("vcb,b->vc", sd, t(betas).reshape(-1))
    jr = Jr @ v_shaped
    A = _joint_transforms_torch(full, jr, parents)
    v_posed = v_shaped
    if model.get("posedirs") is not None:
        Rm = rodrigues(full.reshape(J, 3))
        feat = (Rm[1:] - torch.eye(3, dtype=dtype)).reshape(-1)
        v_posed = v_shaped + (feat @ t(model["posedirs"])).reshape(-1, 3)
    T = torch.einsum("vj,jab->vab", w, A)
    verts = torch.einsum("vab,vb->va", T[:, :3, :3], v_posed) + T[:, :3, 3]
    joints = torch.einsum("jab,jb->ja", A[:, :3, :3], jr) + A[:, :3, 3]
    rows = torch.cat([joints, verts[torch.as_tensor(np.asarray(extra_ids, np.int64))]]) if len(extra_ids) else joints
    Rt, tr = t(R), t(transl)
    return verts @ Rt + tr, rows @ Rt + tr


def host_loss(model, betas, pose, transl, camera, mask, target, used, spec, extra_ids, dtype=torch.float64):
    """One frame's two terms -> (keypoint term, silhouette term, max faces per pixel)."""
    intr, R, H, W = _camera_parts(camera)
    verts_cam, rows = host_forward(model, betas, pose, transl, R, extra_ids, dtype)
    kp, _ = keypoint_term(project_joints(rows, intr, H, W), target, used)
    alpha, cnt = silhouette_host(verts_cam, model["faces"], intr, H, W, spec.sigma, return_counts=True)
    return kp, silhouette_term(alpha, mask), cnt


def refine_pose_host(body, betas, global_orient, body_pose, transl, camera, masks, keypoints, scores, spec, extra_joint_vertex_ids=(),
                     dtype=torch.float64, iterations=None):
    """The loop in torch on the CPU, one frame after the other, every operation in ``dtype``: arrays in (numpy or tensors),
    -> (global_orient [F,3], body_pose [F,69], report) as numpy arrays of ``dtype``.  ``body``: a ``BodyModel`` or the dict of its
    arrays.  ``masks`` [F,H,W] in 0..1.  Adam as ``torch.optim.Adam`` computes it (betas 0.9 / 0.999, eps 1e-8), written out."""
    model = host_model(body)
    t = lambda a: torch.as_tensor(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).to(dtype)
    go, bp, tr, kp, sc, masks = t(global_orient), t(body_pose), t(transl), t(keypoints), t(scores), t(masks)
    F = _check_inputs(go, bp, tr, kp, sc, masks.shape[0])
    if model["J_regressor"].shape[0] + len(extra_joint_vertex_ids) != spec.n_joint_rows:
        raise ValueError(f"pose_refine: {model['J_regressor'].shape[0]} joints + {len(extra_joint_vertex_ids)} picked vertices are not the "
                         f"spec's {spec.n_joint_rows} joint rows")
    target, used = keypoint_targets(kp, sc, spec)
    gm, lo, hi = _spec_tensors(spec, dtype, "cpu")
    iters = spec.iterations if iterations is None else int(iterations)
    b1, b2, eps = 0.9, 0.999, 1e-8
    out = torch.cat([go, bp], 1).clone()
    first, last, faces_max = np.zeros((F, 2)), np.zeros((F, 2)), np.zeros(F, np.int64)
    for f in range(F):
        pose = out[f].clone().requires_grad_(True)
        m, v = torch.zeros_like(pose), torch.zeros_like(pose)
        for it in range(1, iters + 1):
            a, b, cnt = host_loss(model, betas, pose, tr[f], camera, masks[f], target[f], used[f], spec, extra_joint_vertex_ids, dtype)
            g, = torch.autograd.grad(a + b, pose)
            terms = (a.item(), b.item())
            if it == 1:
                first[f] = terms
            last[f] = terms
            faces_max[f] = max(faces_max[f], int(cnt))
            with torch.no_grad():
                g = g * gate(pose, gm, lo, hi)
                m = b1 * m + (1 - b1) * g
                v = b2 * v + (1 - b2) * g * g
                pose -= (spec.lr / (1 - b1 ** it)) * m / (v.sqrt() / math.sqrt(1 - b2 ** it) + eps)
        out[f] = pose.detach()
    out = out.numpy()
    return out[:, :3], out[:, 3:], _report(first, last, used.sum(-1).numpy(), faces_max)


# ---- the loop on the device ---------------------------------------------------------------------------------------------------------------
def _gpu_body(body, device):
    from .body_model import BodyModel
    if isinstance(body, BodyModel):
        return body
    m = dict(body)
    if "vertex_label" not in m:
        m["vertex_label"] = np.zeros(np.asarray(m["v_template"]).shape[0], np.int64)
    return BodyModel(device=device, **m)


class RefineEngine:
    """The loop for K frames at once, every buffer allocated here: ``RefineEngine(body, betas, camera, spec, extra_joint_vertex_ids,
    frames_per_launch=8)``.  ``body``: a ``BodyModel`` (or the dict of its arrays, put on ``betas``' device); ``betas`` [B] fp32 on the GPU.

    One iteration (``_iteration``), for K independent frames: ``joint_transforms_hip`` -> ``lbs_extra`` (pose correctives and
    ``pose_mean`` as ``host_forward`` has them) -> ``verts @ R + transl`` -> the joint rows -> ``project_joints`` / ``keypoint_term`` in
    their masked-sum form -> ``soft_silhouette`` / ``silhouette_term`` -> backward -> ONE update launch (gate, Adam, the step counter and
    the row ``[it - 1]`` of the ``[iterations, K, 2]`` table of terms, all in device memory).  Nothing in it reads the device.

    ``run_batch`` is the entry: it loads up to K frames (a shorter batch is padded with copies of its first frame), counts the (tile,
    face) pairs of the starting poses once (a host read), makes the pair list hold twice that, runs the iterations and reads the
    overflow words once; a batch that overflowed is run again from its starting poses with twice the most pairs any launch had.

    With ``capture`` the first iteration of the first batch runs eagerly, the second is recorded as a HIP graph and every further
    one, of this and of later batches, is a replay.  A captured engine is only replayed: ``iterate()`` raises."""

    def __init__(self, body, betas, camera, spec, extra_joint_vertex_ids=(), frames_per_launch=8, iterations=None, capture=True,
                 capacity=None):
        from . import silhouette as _sil
        if not torch.is_tensor(betas) or not betas.is_cuda:
            raise RuntimeError("pose_refine.RefineEngine: betas must be a GPU tensor (no CPU fallback; the host loop is refine_pose_host)")
        self.device = betas.device
        self.body = _gpu_body(body, self.device)
        self.spec, self.K = spec, int(frames_per_launch)
        if not 1 <= self.K <= _sil._lib.SIL_MAX_FRAMES:
            raise ValueError(f"pose_refine.RefineEngine: frames_per_launch = {self.K} outside 1..{_sil._lib.SIL_MAX_FRAMES}")
        self.iterations = spec.iterations if iterations is None else int(iterations)
        self.capture, self.graph = bool(capture), None
        self.intr, R, self.H, self.W = _camera_parts(camera)
        J, V = self.body.num_joints, self.body.num_verts
        self.extra = tuple(int(i) for i in extra_joint_vertex_ids)
        if J + len(self.extra) != spec.n_joint_rows:
            raise ValueError(f"pose_refine: {J} joints + {len(self.extra)} picked vertices are not the spec's {spec.n_joint_rows} joint rows")
        if 3 * J < POSE:
            raise ValueError(f"pose_refine: a body of {J} joints has no {POSE}-entry pose")
        dev, K, f32 = self.device, self.K, torch.float32
        with torch.cuda.device(dev), torch.no_grad():
            b = betas.detach().to(f32).reshape(-1)
            self.v_shaped = self.body.shaped(b)["v_shaped"][0].contiguous()
            self.joints_rest = self.body.joints_rest(b).contiguous()
            self.R = torch.as_tensor(R, dtype=f32, device=dev)
            self.extra_t = torch.as_tensor(self.extra, dtype=torch.long, device=dev)
            self.gm, self.lo, self.hi = _spec_tensors(spec, f32, dev)
            z = lambda *shape, dt=f32: torch.zeros(shape, dtype=dt, device=dev)
            self.pose, self.m, self.v, self.step = z(K, POSE), z(K, POSE), z(K, POSE), z(1, dt=torch.int32)
            self.transl, self.mask = z(K, 3), z(K, self.H, self.W)
            self.target, self.used = z(K, spec.n_joint_rows, 2), z(K, spec.n_joint_rows, dt=torch.bool)
            self.terms, self.table = z(K, 2), z(max(1, self.iterations), K, 2)
            self.pad = z(K, 3 * J - POSE) if 3 * J > POSE else None
        self._sil = _sil
        self.forced_capacity = None if capacity is None else int(capacity)
        self.work = self.count_work = None
        self.start_pairs = self.peak_pairs = self.reruns = 0

    # -- one iteration
    def _forward(self, pose):
        from .body import joint_transforms_hip
        from .lbs import lbs_extra
        body = self.body
        full = pose if self.pad is None else torch.cat([pose, self.pad], 1)
        if body.pose_mean is not None:
            full = full + body.pose_mean
        A = joint_transforms_hip(full, self.joints_rest, body.parents)
        verts = lbs_extra(A, self.v_shaped[None], body.posedirs, body.lbs_weights, full, disable_posedirs=body.posedirs is None)[0]
        # (products and sums written out: element-wise launches only, nothing of a BLAS library inside the recorded iteration)
        joints = (A[:, :, :3, :3] * self.joints_rest[None, :, None, :]).sum(-1) + A[:, :, :3, 3]
        rows = torch.cat([joints, verts.index_select(1, self.extra_t)], 1) if self.extra else joints
        to_cam = lambda p: (p[..., :, None] * self.R).sum(-2) + self.transl[:, None]
        return to_cam(verts), to_cam(rows)

    def _terms(self, pose, counts=False, work=None):
        verts_cam, rows = self._forward(pose)
        kp, _ = keypoint_term(project_joints(rows, self.intr, self.H, self.W), self.target, self.used)
        out = self._sil.soft_silhouette(verts_cam.contiguous(), self.body.faces, self.intr, self.H, self.W, self.spec.sigma,
                                        return_counts=counts, workspace=self.work if work is None else work, check=False)
        alpha, cnt = out if counts else (out, None)
        return kp, silhouette_term(alpha, self.mask), cnt

    def gradient(self):
        """The two terms and dL/dpose of the loaded frames at the current pose, without an update -> (terms [K,2], dkeypoint [K,72],
        dsilhouette [K,72]) (for tests; eager)."""
        self._need_work()
        pose = self.pose.detach().clone().requires_grad_(True)
        kp, sil, _ = self._terms(pose)
        g_kp, = torch.autograd.grad(kp.sum(), pose, retain_graph=True)
        g_sil, = torch.autograd.grad(sil.sum(), pose)
        return torch.stack([kp, sil], 1).detach(), g_kp, g_sil

    def _iteration(self):
        pose = self.pose.detach().requires_grad_(True)
        kp, sil, _ = self._terms(pose)
        grad, = torch.autograd.grad((kp + sil).sum(), pose)
        self.terms.copy_(torch.stack([kp.detach(), sil.detach()], 1))
        from ._marshal import sil_pose_update
        sil_pose_update(self.spec.lr, self.pose, grad.contiguous(), self.m, self.v, self.gm, self.lo, self.hi, self.step, self.terms,
                        self.table)

    def iterate(self):
        """One eager iteration on the loaded frames.  Raises on an engine that has been captured: its buffers belong to the graph."""
        if self.graph is not None:
            raise RuntimeError("pose_refine.RefineEngine: this engine has been captured; it is only replayed (run_batch)")
        self._need_work()
        self._iteration()

    def _record(self):
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._iteration()
        self.graph = graph

    # -- a batch
    def load(self, pose, transl, masks, target, used):
        """Up to K frames into the engine's buffers (tensors on any device); the moments, the step counter and the table start anew."""
        n = int(pose.shape[0])
        if not 1 <= n <= self.K:
            raise ValueError(f"pose_refine.RefineEngine: a batch of {n} frames for K = {self.K}")
        idx = torch.cat([torch.arange(n), torch.zeros(self.K - n, dtype=torch.long)])
        with torch.no_grad():
            for dst, src in ((self.pose, pose), (self.transl, transl), (self.mask, masks), (self.target, target), (self.used, used)):
                dst.copy_(torch.as_tensor(src)[idx].to(dst.dtype))
            for t in (self.m, self.v, self.step, self.table, self.terms):
                t.zero_()
        self.n_loaded = n

    def _need_work(self, capacity=None):
        V, F = self.body.num_verts, int(self.body.faces.shape[0])
        if self.work is None or (capacity is not None and capacity > self.work.capacity):
            cap = self._sil.default_capacity(self.K, F) if capacity is None else capacity
            self.work = self._sil.SilhouetteWorkspace(self.K, V, self.body.faces, self.H, self.W, cap, self.device)
            self.graph = None                                        # (a graph holds the addresses and the capacity of its workspace)

    def count(self):
        """One counting forward at the current pose, synchronous -> (pairs of all K frames, max faces per pixel [K] numpy).  It has a
        workspace of its own: the one the iterations run in, which a graph may hold, is never launched into from here."""
        V, F = self.body.num_verts, int(self.body.faces.shape[0])
        capacity = self._sil.default_capacity(self.K, F) if self.count_work is None else self.count_work.capacity
        while True:
            if self.count_work is None or self.count_work.capacity < capacity:
                self.count_work = self._sil.SilhouetteWorkspace(self.K, V, self.body.faces, self.H, self.W, capacity, self.device)
            with torch.no_grad():
                _, _, cnt = self._terms(self.pose, counts=True, work=self.count_work)
            over, total, _ = self.count_work.info()
            if not over:
                return total, cnt.cpu().numpy().astype(np.int64)
            capacity = total

    def run_batch(self, pose, transl, masks, target, used):
        """-> (pose [n,72] fp32 numpy, table [iterations,n,2] numpy, max faces per pixel at the starting poses [n])."""
        self.load(pose, transl, masks, target, used)
        with torch.cuda.device(self.device):
            self.start_pairs, faces_max = self.count()
            capacity = max(1, 2 * self.start_pairs) if self.forced_capacity is None else self.forced_capacity
            self.reruns = 0
            while True:
                self._need_work(capacity)
                self.load(pose, transl, masks, target, used)
                self.work.reset_peak()
                left = self.iterations
                if self.capture and self.graph is None and left > 0:
                    self._iteration()                                # the first iteration runs eagerly
                    left -= 1
                    if left > 0:
                        self._record()
                for _ in range(left):
                    if self.capture:
                        self.graph.replay()
                    else:
                        self._iteration()
                over, self.peak_pairs = self.work.peak()
                if not over:
                    break
                self.reruns += 1
                if self.reruns > 8:
                    raise RuntimeError(f"pose_refine.RefineEngine: the pair list overflowed {self.reruns} times (last: {self.peak_pairs} pairs)")
                capacity = 2 * self.peak_pairs
            n = self.n_loaded
            return self.pose[:n].cpu().numpy(), self.table[:, :n].cpu().numpy(), faces_max[:n]


def refine_pose(body, betas, global_orient, body_pose, transl, camera, masks, keypoints, scores, spec, extra_joint_vertex_ids=(),
                frames_per_launch=8, capture=True, iterations=None, engine=None, trace=None):
    """The loop on the device: ``betas`` [B] and the per-frame inputs as GPU tensors (host tensors raise), -> (global_orient [F,3],
    body_pose [F,69], report) as fp32 numpy arrays.  The report has ``refine_pose_host``'s keys; ``max_faces_per_pixel`` comes from one
    counting forward at the starting poses.  ``trace``: a list that receives every batch's [iterations, n, 2] table of terms."""
    for name, t in (("betas", betas), ("global_orient", global_orient), ("body_pose", body_pose), ("transl", transl), ("masks", masks),
                    ("keypoints", keypoints), ("scores", scores)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"pose_refine.refine_pose: {name} must be a GPU tensor (no CPU fallback; the host loop is refine_pose_host)")
    F = _check_inputs(global_orient, body_pose, transl, keypoints, scores, masks.shape[0])
    if engine is None:
        engine = RefineEngine(body, betas, camera, spec, extra_joint_vertex_ids, min(int(frames_per_launch), F), iterations, capture)
    target, used = keypoint_targets(keypoints.float(), scores.float(), spec)
    start = torch.cat([global_orient, body_pose], 1).float()
    iters, K = engine.iterations, engine.K
    out = np.zeros((F, POSE), np.float32)
    first, last, faces_max = np.zeros((F, 2)), np.zeros((F, 2)), np.zeros(F, np.int64)
    for at in range(0, F, K):
        sl = slice(at, min(at + K, F))
        out[sl], table, faces_max[sl] = engine.run_batch(start[sl], transl[sl], masks[sl], target[sl], used[sl])
        if iters > 0:
            first[sl], last[sl] = table[0], table[iters - 1]
        if trace is not None:
            trace.append(table)
    return out[:, :3], out[:, 3:], _report(first, last, used.sum(-1).cpu().numpy(), faces_max)


# ---- a kit ------------------------------------------------------------------------------------------------------------------------------
REFINED_FILE = "poses_optimized.npz"


def write_refined_poses(path, betas, global_orient, body_pose, transl, overwrite=False):
    """``np.savez_compressed`` of the reference's keys (ooptimize_smpl.py:401-411): ``betas`` [B], ``global_orient`` [F,3], ``body_pose``
    [F,69], ``transl`` [F,3], fp32.  Atomic: written beside ``path`` and renamed.  ``FileExistsError`` unless ``overwrite``."""
    import os
    import tempfile
    path = str(path)
    arrays = {"betas": np.asarray(betas, np.float32).reshape(-1), "global_orient": np.asarray(global_orient, np.float32),
              "body_pose": np.asarray(body_pose, np.float32), "transl": np.asarray(transl, np.float32)}
    F = arrays["global_orient"].shape[0] if arrays["global_orient"].ndim == 2 else -1
    if arrays["global_orient"].shape != (F, 3) or arrays["body_pose"].shape != (F, 69) or arrays["transl"].shape != (F, 3) or F < 1:
        raise ValueError(f"write_refined_poses: global_orient {arrays['global_orient'].shape}, body_pose {arrays['body_pose'].shape}, "
                         f"transl {arrays['transl'].shape} must be [F,3], [F,69], [F,3]")
    if not all(np.isfinite(a).all() for a in arrays.values()):
        raise ValueError("write_refined_poses: an array is not finite")
    if os.path.exists(path) and not overwrite:
        raise FileExistsError(f"write_refined_poses: {path} exists (overwrite=True replaces it)")
    folder = os.path.dirname(path) or "."
    os.makedirs(folder, exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".npz", prefix=".poses_", dir=folder)
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez_compressed(f, **arrays)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return path


def refine_kit(root, body, extra_joint_vertex_ids, spec=None, split="train+val", out=None, overwrite=False, frames_per_launch=8,
               capture=True):
    """What replaces ``prepare_kits.sh ... --opt``: ``load_kit(root, split)``, ``load_keypoints``, the masks from the store's fourth
    channel as byte / 255 -> ``refine_pose`` -> ``<root>/score_demo_video/poses_optimized.npz`` (or ``out``).  The starting poses are
    ``poses.npz``'s when a refined file is being replaced.  -> (path, report)."""
    import os
    from . import kit as _kit
    spec = RefineSpec.smpl() if spec is None else spec
    path = os.path.join(str(root), "score_demo_video", REFINED_FILE) if out is None else str(out)
    if os.path.exists(path) and not overwrite:
        raise FileExistsError(f"refine_kit: {path} exists (overwrite=True replaces it)")
    k = _kit.load_kit(root, split)
    dev = k.store.device
    smpl = k.smpl
    raw = os.path.join(str(root), "score_demo_video", "poses.npz")
    if os.path.exists(os.path.join(str(root), "score_demo_video", REFINED_FILE)) and os.path.exists(raw):
        p = _kit.load_smpl_param(raw)
        drop = 0 if split == "train+val" else _kit.DROP_FIRST
        idx = np.asarray(k.indices, np.int64) + drop
        smpl = {"betas": torch.from_numpy(p["betas"]).to(dev),
                **{key: torch.from_numpy(np.ascontiguousarray(p[key][idx])).to(dev) for key in ("global_orient", "body_pose", "transl")}}
    kp, sc = _kit.load_keypoints(root, [i + (0 if split == "train+val" else _kit.DROP_FIRST) for i in k.indices])
    masks = k.store.data[..., 3].float() / 255
    go, bp, report = refine_pose(body, smpl["betas"].reshape(-1), smpl["global_orient"], smpl["body_pose"], smpl["transl"], k.camera, masks,
                                 torch.from_numpy(kp).to(dev), torch.from_numpy(sc).to(dev), spec, extra_joint_vertex_ids,
                                 frames_per_launch, capture)
    write_refined_poses(path, smpl["betas"].cpu().numpy(), go, bp, smpl["transl"].cpu().numpy(), overwrite)
    return path, report
