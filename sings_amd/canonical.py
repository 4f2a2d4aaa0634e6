"""The canonical turntable and the training-progress sheet of the reference's ``render_canonical`` (gs_trainer.py:757-851), posed once.

The reference decodes the attributes once and then, for each of ``canon_nframes`` orbiting cameras, skins the avatar into the same
predefined pose (datasets/utils.py:123-182) and renders it: 60 skin + raster calls for one static set of Gaussians.  A turntable is K
cameras of ONE posed set, which is the launch ``RasterFramesEngine`` makes:

    ``predefined_pose`` / ``smpl_static_params``   the five pose types and the reference's static SMPL parameters, values and keys
    ``static_A``          the pose's joint transforms A_cano2pose through ``body.joint_transforms`` and ``body.cano_to_pose``
    ``pose_once``         ONE ``SkinnedEngine.forward(..., posed_out=...)``: the posed means, quaternions and scales
    ``OrbitRenderer``     K cameras of the posed set per launch, pair counts read and settled per launch (``overflow.EngineCapacity``)
    ``render_canonical``  the turntable as uint8 [H,W,3] frames, one ``sheets.image_sheets`` launch per K cameras
    ``progress_sheet``    the reference's ``is_train_progress`` sheet: every camera at ``scaling_modifier`` 0.5, then 1.0; ``nrow=4``

Everything works at engine level: the process-wide overflow state of the autograd ops (``overflow._mode``, the capacity hint), which
a trainer's captured step relies on, is never touched.  Forward only.
"""
import math

import torch

from .body import SMPL_PARENTS, cano_to_pose, joint_transforms
from .overflow import EngineCapacity
from .renderer import _settings

POSE_TYPES = ("da_pose", "a_pose", "little_a_pose", "little_little_a_pose", "t_pose")
# datasets/utils.py:123-157: the non-zero entries of the 69 body-pose values (23 joints x axis-angle), by pose type
_POSE_ENTRIES = {
    "da_pose": {2: 1.0, 5: -1.0},
    "a_pose": {2: 0.2, 5: -0.2, 47: -0.8, 50: 0.8},
    "little_a_pose": {2: 0.1, 5: -0.1, 47: -0.8, 50: 0.8},
    "little_little_a_pose": {2: 0.02, 5: -0.02, 47: -0.9, 50: 0.9},
    "t_pose": {},
}


def predefined_pose(pose_type, device="cpu"):
    """The reference's ``get_predefined_pose(pose_type)[0]``: fp32 [69].  An unknown type is a ValueError."""
    if pose_type not in _POSE_ENTRIES:
        raise ValueError(f"Unknown pose type: {pose_type}")
    pose = torch.zeros(69, dtype=torch.float32)
    for i, v in _POSE_ENTRIES[pose_type].items():
        pose[i] = v
    return pose.to(device)


def smpl_static_params(betas, pose_type="da_pose", device="cpu"):
    """The reference's ``get_smpl_static_params``: dict(betas [flattened], global_orient [3] zeros, body_pose [69], transl [3] zeros,
    smpl_scale [1] ones), fp32 tensors on ``device``."""
    body_pose = predefined_pose(pose_type)
    betas = torch.as_tensor(betas)
    if betas.dim() != 1:
        betas = betas.reshape(-1)
    datum = {"betas": betas, "global_orient": torch.zeros(3, dtype=torch.float32), "body_pose": body_pose,
             "transl": torch.tensor([0.0, 0.0, 0.0]).float(), "smpl_scale": torch.ones(1, dtype=torch.float32)}
    return {k: v.to(device) for k, v in datum.items()}


def static_A(pose_type_or_pose, joints_rest, A_t2cano, parents=SMPL_PARENTS):
    """A_cano2pose [J,4,4] of a static pose: ``body.joint_transforms`` of the pose, then ``body.cano_to_pose``.  A pose type (a name of
    ``POSE_TYPES``) stands for ``global_orient = 0`` + ``predefined_pose`` and is accepted for the 24 SMPL joints only; for any other
    J (the SMPL-H layer's 52: its hand pose is the layer's, not guessed here) pass the full axis-angle pose [J*3] / [J,3]."""
    J = int(joints_rest.shape[0])
    if isinstance(pose_type_or_pose, str):
        if J != 24:
            raise ValueError(f"static_A: a pose type names the 24 SMPL joints' pose; for J = {J} pass the full axis-angle pose [J*3]")
        pose = torch.cat([torch.zeros(3, dtype=torch.float32), predefined_pose(pose_type_or_pose)])
    else:
        pose = torch.as_tensor(pose_type_or_pose)
        if pose.numel() != 3 * J:
            raise ValueError(f"static_A: the pose must hold {3 * J} values for {J} joints, got {pose.numel()}")
    pose = pose.reshape(-1).to(device=joints_rest.device, dtype=joints_rest.dtype)
    return cano_to_pose(joint_transforms(pose, joints_rest, parents), A_t2cano)


@torch.no_grad()
def pose_once(canon, A_cano2pose, camera, bg_color, smpl_scale=None, transl=None):
    """The set posed ONCE: one ``SkinnedEngine.forward(..., posed_out=...)`` at ``camera`` (any camera of the orbit: the posed values
    do not depend on it) -> dict(xyz [P,3], rotq [P,4], scales [P,3], shs, opacity, active_sh_degree), what ``get_render_pkg`` and
    ``OrbitRenderer.render`` take.  ``canon`` as in ``get_render_pkg_fused``."""
    from .engine import SkinnedEngine
    from .skinned import _canonical_inputs
    dev, xyz, rot, _, scales, opacity, shs = _canonical_inputs(canon["xyz_canon"], canon.get("rotmat_canon"), canon["scales"],
                                                               canon["opacity"], canon["shs"])
    P, M = int(xyz.shape[0]), int(shs.shape[1])
    W, H = int(camera["image_width"]), int(camera["image_height"])
    A = A_cano2pose.detach().contiguous().float()
    e = SkinnedEngine(P, int(A.reshape(-1, 16).shape[0]), W, H, M, dev, capacity_pairs=EngineCapacity.floor(0, P, W, H))
    f32 = dict(dtype=torch.float32, device=dev)
    posed = (torch.empty((P, 3), **f32), torch.empty((P, 4), **f32), torch.empty((P, 3), **f32))
    with torch.cuda.device(dev):
        e.set_camera(_settings(camera, bg_color, 1.0, canon["active_sh_degree"]))
        e.set_frame(xyz.detach(), None if rot is None else rot.detach(), canon["lbs_weights"], A, smpl_scale, transl, None)
        # (the image of this call is not used: a pair count beyond the capacity leaves the posed values as they are)
        e.forward(shs.detach(), opacity.detach(), scales.detach(), posed_out=posed)
    return {"xyz": posed[0], "rotq": posed[1], "scales": posed[2], "shs": shs.detach(), "opacity": opacity.detach(),
            "active_sh_degree": canon["active_sh_degree"]}


class OrbitRenderer:
    """K cameras of ONE posed set of Gaussians per launch (one ``RasterFramesEngine``, its default work order), forward only.

    ``posed_or_P``: the number of Gaussians, or a dict of ``pose_once`` to take it from.  ``capacity_pairs``: the pair capacity of the
    first engine (None: ``EngineCapacity.floor``).  Every launch reads its K pair counts and settles them through
    ``overflow.EngineCapacity``: a launch whose pairs exceed the capacity (or whose long-rows hint failed) is rendered again, on a
    grown engine, before any of its frames is handed out -- never returned as a background frame."""

    def __init__(self, posed_or_P, W, H, M, K=8, device="cuda", capacity_pairs=None):
        self.P = int(posed_or_P["xyz"].shape[0]) if isinstance(posed_or_P, dict) else int(posed_or_P)
        self.W, self.H, self.M, self.K = int(W), int(H), int(M), int(K)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("sings_amd.canonical.OrbitRenderer runs on the MI355X only; there is no CPU fallback")
        self.policy = EngineCapacity()
        self.engine, self.launches, self.redone = None, 0, 0
        self._build(EngineCapacity.floor(0, self.P, self.W, self.H) if capacity_pairs is None else int(capacity_pairs))

    cap = property(lambda self: self.engine.cap)

    def _build(self, cap):
        from .engine import RasterFramesEngine
        self.engine = None                                       # (drop the old workspaces before the new ones are sized)
        self.engine = RasterFramesEngine(self.P, self.W, self.H, self.M, self.K, self.dev, capacity_pairs=int(cap))

    def _launch(self, posed, rs, cap):
        """One launch with at least ``cap`` pairs -> (raw [K,3,H,W], a new tensor; the K pair counts; the capacity it ran with)."""
        if cap > self.engine.cap:
            torch.cuda.synchronize(self.dev)
            self._build(cap)
        e = self.engine
        e.set_camera(rs, long_rows=self.policy.long_rows)
        counts = e.forward(posed["xyz"], posed["shs"], posed["opacity"], posed["scales"], posed["rotq"], sync_num_rendered=True)
        self.launches += 1
        return e.color.clone(), counts, e.cap

    @torch.no_grad()
    def chunks(self, posed, cameras, bg_color, scaling_modifier=1.0):
        """Yields (index of the chunk's first camera, k, raw [K,3,H,W]) per launch; only the first k frames are cameras of the list."""
        if int(posed["xyz"].shape[0]) != self.P or int(posed["shs"].shape[1]) != self.M:
            raise ValueError(f"OrbitRenderer: built for {self.P} Gaussians of {self.M} SH coefficients")
        cameras, K = list(cameras), self.K
        with torch.cuda.device(self.dev):
            for i0 in range(0, len(cameras), K):
                cams = cameras[i0:i0 + K]
                k = len(cams)
                if any(int(c["image_width"]) != self.W or int(c["image_height"]) != self.H for c in cams):
                    raise ValueError(f"OrbitRenderer: built for {self.W} x {self.H} images")
                pad = cams + [cams[-1]] * (K - k)                # (stacked as FrameAnimator.render_frames_batched stacks them)
                rs = _settings(cams[0], bg_color, scaling_modifier, posed["active_sh_degree"])._replace(
                    viewmatrix=torch.stack([c["world_view_transform"] for c in pad]).contiguous(),
                    projmatrix=torch.stack([c["full_proj_transform"] for c in pad]).contiguous(),
                    campos=torch.stack([c["camera_center"] for c in pad]).contiguous())
                raw, counts, ran_with = self._launch(posed, rs, 0)
                cap = self.policy.settle(counts[:k], ran_with)
                if cap is not None:
                    def again(cap):
                        raw, counts, ran_with = self._launch(posed, rs, cap)
                        return raw, counts[:k], ran_with
                    self.redone += 1
                    raw = self.policy.redo(cap, again)
                yield i0, k, raw

    def render(self, posed, cameras, bg_color, scaling_modifier=1.0):
        """Yields (index, raw [3,H,W]) in camera order: the unclamped image of ``renderer.render`` for that camera, bit for bit."""
        for i0, k, raw in self.chunks(posed, cameras, bg_color, scaling_modifier):
            for j in range(k):
                yield i0 + j, raw[j]


def _orbit(posed, cameras, frames_per_launch, renderer):
    W, H = int(cameras[0]["image_width"]), int(cameras[0]["image_height"])
    if renderer is None:
        K = max(1, min(int(frames_per_launch), 16, len(cameras)))
        renderer = OrbitRenderer(posed, W, H, int(posed["shs"].shape[1]), K=K, device=posed["xyz"].device)
    return renderer


@torch.no_grad()
def render_canonical_chunks(canon, A_static, bg_color, nframes=60, img_size=512, dist=5.0, angle_limit=2 * math.pi, frames_per_launch=8,
                            fov=0.4, smpl_scale=None, transl=None, renderer=None, cameras=None):
    """``render_canonical`` a launch at a time: yields (index of the first frame, uint8 [k,H,W,3] on the GPU), so that a caller that
    wants the frames on the host copies them once per launch."""
    from .camera import get_rotating_camera
    from .sheets import image_sheets
    dev = canon["xyz_canon"].device
    if cameras is None:
        cameras = get_rotating_camera(img_size=img_size, fov=fov, dist=dist, device=dev, nframes=int(nframes), angle_limit=angle_limit)
    posed = pose_once(canon, A_static, cameras[0], bg_color, smpl_scale=smpl_scale, transl=transl)
    for i0, k, raw in _orbit(posed, cameras, frames_per_launch, renderer).chunks(posed, cameras, bg_color):
        yield i0, image_sheets(raw[:k], tiles_per_sheet=1, padding=0, quant="round")


def render_canonical(canon, A_static, bg_color, nframes=60, img_size=512, dist=5.0, angle_limit=2 * math.pi, frames_per_launch=8,
                     **kwargs):
    """The turntable of gs_trainer.py:757-851: ``nframes`` orbit cameras (``camera.get_rotating_camera``; ``img_size`` an int or
    (height, width)) of the avatar in the static pose ``A_static`` (``static_A``).  Yields (index, uint8 [H,W,3] on the GPU), quantised
    as ``save_image`` does: the set is posed once, rendered ``frames_per_launch`` cameras per launch, and each launch's frames become
    bytes in one ``image_sheets`` launch.  Keywords: ``fov``, ``smpl_scale``, ``transl``; ``renderer``: an ``OrbitRenderer`` to reuse;
    ``cameras``: the camera dicts to use instead of the orbit."""
    for i0, u8 in render_canonical_chunks(canon, A_static, bg_color, nframes=nframes, img_size=img_size, dist=dist,
                                          angle_limit=angle_limit, frames_per_launch=frames_per_launch, **kwargs):
        for j in range(int(u8.shape[0])):
            yield i0 + j, u8[j]


@torch.no_grad()
def progress_sheet(canon, A_static, bg_color, nframes=2, img_size=256, dist=5.0, angle_limit=math.pi, fov=0.4, smpl_scale=None,
                   transl=None, renderer=None, cameras=None):
    """The reference's training-progress sheet (``render_canonical(is_train_progress=True)``, gs_trainer.py:806-842): for each of
    ``nframes`` cameras the render at ``scaling_modifier`` 0.5 and then at 1.0, tiled by ``make_grid(nrow=4, pad_value=0)`` ->
    uint8 [Hs,Ws,3] on the GPU.  Two K-camera passes (the modifier is a field of the launch's settings), one sheet launch."""
    from .camera import get_rotating_camera
    from .sheets import image_sheets
    dev = canon["xyz_canon"].device
    if cameras is None:
        cameras = get_rotating_camera(img_size=img_size, fov=fov, dist=dist, device=dev, nframes=int(nframes), angle_limit=angle_limit)
    posed = pose_once(canon, A_static, cameras[0], bg_color, smpl_scale=smpl_scale, transl=transl)
    orbit = _orbit(posed, cameras, 16, renderer)
    half, full = (torch.cat([raw[:k] for _, k, raw in orbit.chunks(posed, cameras, bg_color, sm)]) for sm in (0.5, 1.0))
    return image_sheets(half, full, nrow=4, padding=2, pad_value=0.0, quant="round")[0]
