"""Posed-frame driver: the callers' glue either side of the fused kernels.

 * ``joint_transforms_batch``: the SMPL(-H) kinematic chain for a CHUNK of frames in J batched 4x4 products
   (reference: ``forward_chunk`` -> ``smpl_template`` -> ``batch_rigid_transform``, sings_hybrid.py:474-531,
   body_model/smpl.py:462-513) -- without the per-step template work the reference discards
   (blend shapes, the J_regressor einsum over 110k vertices, full template skinning).
 * ``amass_to_smpl_pose``: the 156 -> 72 AMASS joint selection of sings/rec/defaults/constants.py:13-18.
 * ``animate_chunk``: forward-only rendering of a chunk of posed frames through the LBS-fused kernels, one
   fused call per frame (trainer counterpart: gs_trainer.py:664-728); posed means / quaternions never exist in HBM.
   ``streams > 1`` renders that many frames at a time on separate HIP streams through pre-allocated engines
   (``FrameAnimator``): an avatar frame is a chain of short, latency-bound kernels and a few very long tile lists, so
   frames in flight together fill the GPU (150k-Gaussian avatar, 120 frames: 3 100 -> 8 550 frames/s with 4 streams).
   ``frames_per_launch = K`` (round 4): K consecutive frames of the chunk per DISPATCH through ``SkinnedFramesEngine`` -- what
   ``SinGS.forward_chunk`` + the render loop of gs_trainer.py:684-714 do for a chunk of 16 frames, in one pass over the kernels.
"""
from collections import deque

import numpy as np
import torch

from . import _lib
from .body import SMPL_PARENTS, rodrigues
from .frame_out import JPEG_QUALITY, FrameOut, frames_to_u8, parse_out       # noqa: F401 (frames_to_u8, JPEG_QUALITY: their names here)
from .overflow import EngineCapacity
from .renderer import _settings, get_render_pkg_fused

# sings/rec/defaults/constants.py:13-18: SMPL-H (52 joints, AMASS order) -> the 24 SMPL joints
AMASS_SMPLH_TO_SMPL_JOINTS = np.arange(0, 156).reshape((-1, 3))[[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16,
                                                                   17, 18, 19, 20, 21, 22, 37]].reshape(-1)


def amass_to_smpl_pose(poses156):
    """[F,156] AMASS SMPL-H axis-angle poses -> [F,72] SMPL poses (AnimDataset_opt.py:109-110)."""
    return poses156[..., AMASS_SMPLH_TO_SMPL_JOINTS]


def joint_transforms_batch(poses, joints_rest, parents=SMPL_PARENTS):
    """poses [B, J*3] axis-angle, joints_rest [J,3] -> A [B,J,4,4].  fp32 on the GPU: ONE launch (sg_joint_transforms, one wave
    per frame); otherwise J-1 batched matmuls for the whole chunk in torch."""
    if poses.is_cuda and poses.dtype == torch.float32 and joints_rest.dtype == torch.float32 and joints_rest.shape[0] <= 64:
        from .body import joint_transforms_hip
        return joint_transforms_hip(poses, joints_rest, parents)
    B = poses.shape[0]
    J = joints_rest.shape[0]
    R = rodrigues(poses.reshape(B * J, 3)).view(B, J, 3, 3)
    rel = joints_rest.clone()
    par = torch.as_tensor(parents[1:], device=joints_rest.device, dtype=torch.long)
    rel[1:] = joints_rest[1:] - joints_rest[par]
    T = torch.zeros(B, J, 4, 4, dtype=poses.dtype, device=poses.device)
    T[:, :, :3, :3] = R
    T[:, :, :3, 3] = rel[None]
    T[:, :, 3, 3] = 1
    chain = [T[:, 0]]
    for i in range(1, J):
        chain.append(torch.bmm(chain[parents[i]], T[:, i]))
    G = torch.stack(chain, 1)
    jh = torch.cat([joints_rest, torch.zeros_like(joints_rest[:, :1])], 1)[None, :, :, None]
    corr = torch.matmul(G, jh)
    return G - torch.cat([torch.zeros(B, J, 4, 3, dtype=G.dtype, device=G.device), corr], -1)


def forward_chunk(gs_attrs, lbs_weights, A_t2pose, inv_A_t2cano=None, transl=None, smpl_scale=None, ext_tfs=None,
                  isotropic=False, active_sh_degree=0):
    """The batched deformation of ``SinGS.forward_chunk`` (sings/rec/models/sings_hybrid.py:474-569) for callers that want
    the reference's dict of POSED Gaussians for B frames at once (gs_trainer.py:695-714 then renders them one by one);
    ``animate_chunk`` below is the fused alternative that never materialises them.

    gs_attrs: dict(xyz_canon [N,3], xyz_offsets, rot6d_canon [N,6] | None, scales [N,3], opacity [N,1], shs [N,M,3]);
    A_t2pose [B,J,4,4]: the joint transforms the reference takes from ``smpl_template(...).A`` (here:
    ``joint_transforms_batch``; shape blending needs the licensed SMPL model and stays with the caller);
    inv_A_t2cano [J,4,4] | None; transl [B,3], smpl_scale [B,1], ext_tfs = (trans [B,3], rotmat [B,3,3], scale [B,1]).
    Returns the reference's keys with the same shapes ([B,N,...], canonical tensors expanded, not copied).
    Device work: ``sg_lbs_forward`` per frame (T and vertices in one kernel, W.A on the matrix cores), the rotation kernels
    of sings_amd.rotations for 6-D -> matrix, matrix -> quaternion ([B*N] in one launch) and the quaternion product."""
    from . import rotations as R
    from .lbs import lbs_extra
    xyz_canon = gs_attrs['xyz_canon']
    dev = xyz_canon.device
    if dev.type != "cuda":
        raise RuntimeError("sings_amd.posed.forward_chunk runs on the MI355X only; there is no CPU fallback")
    B, N = int(A_t2pose.shape[0]), int(xyz_canon.shape[0])
    rot6d = gs_attrs.get('rot6d_canon')
    if not isotropic:
        rotmat_canon = R.rotation_6d_to_matrix(rot6d)
        rotq_canon = R.matrix_to_quaternion(rotmat_canon)
    else:
        rotmat_canon = torch.eye(3, device=dev).unsqueeze(0).repeat(N, 1, 1)
        rotq_canon = torch.zeros(N, 4, device=dev)
    scales = gs_attrs['scales'].unsqueeze(0).expand(B, -1, -1)
    A = A_t2pose if inv_A_t2cano is None else A_t2pose @ inv_A_t2cano.unsqueeze(0)
    xyz, _, lbs_T, _, _ = lbs_extra(A, xyz_canon.unsqueeze(0).expand(B, -1, -1), None, lbs_weights, None, disable_posedirs=True)
    if smpl_scale is not None:
        xyz = xyz * smpl_scale.unsqueeze(-1)
        scales = scales * smpl_scale.unsqueeze(-1)
    if transl is not None:
        xyz = xyz + transl.unsqueeze(1)
    rotq = R.matrix_to_quaternion(lbs_T[..., :3, :3] @ rotmat_canon.unsqueeze(0))
    if ext_tfs is not None:
        trans, rotmat, scale = ext_tfs
        xyz = trans[:, None, :] + scale[:, None] * (rotmat[:, None, ...] @ xyz[..., None]).squeeze(-1)
        scales = scale[..., None] * scales
        rotq = R.quaternion_multiply(R.matrix_to_quaternion(rotmat.contiguous())[:, None, :], rotq)
    return {
        'xyz': xyz, 'xyz_canon': xyz_canon.unsqueeze(0).expand(B, -1, -1), 'xyz_offsets': gs_attrs.get('xyz_offsets'),
        'scales': scales, 'scales_canon': scales,                    # (the reference returns the scaled tensor under both keys)
        'rotq': rotq, 'rotq_canon': rotq_canon,
        'shs': gs_attrs['shs'].unsqueeze(0).expand(B, -1, -1, -1), 'opacity': gs_attrs['opacity'].unsqueeze(0).expand(B, -1, -1),
        'active_sh_degree': active_sh_degree,
    }


def _shared(ts):
    """The tensors of a batch's frames are one and the same values: the same object, or views of the same memory (the frames'
    rows of an ``.expand`` view)."""
    t0 = ts[0]
    return all(t is t0 or (t.data_ptr() == t0.data_ptr() and t.shape == t0.shape and t.stride() == t0.stride()
                           and t.dtype == t0.dtype) for t in ts)


def _batch_rows(ts, K, width):
    """Per-frame inputs of a batch of k <= K frames -> one shared tensor (every frame's is the same) or [K, width] rows, the tail
    padded with the last frame's (as A and transl are)."""
    if _shared(ts):
        return ts[0]
    return torch.stack([t.reshape(width) for t in ts] + [ts[-1].reshape(width)] * (K - len(ts))).contiguous()


def _stack_poses(rows, K):
    """The (A, transl | None, smpl_scale | None, ext_tfs | None) of a batch's k <= K frames of ONE avatar -> what ``set_frames``
    takes: A [K,J,16] and transl [K,3] stacked, the tail padded with the last frame's; smpl_scale and ext_tfs through
    ``_batch_rows``."""
    k = len(rows)
    A = torch.stack([r[0].reshape(-1, 16) for r in rows] + [rows[-1][0].reshape(-1, 16)] * (K - k)).contiguous()
    tr = None
    if rows[0][1] is not None:
        tr = torch.stack([r[1].reshape(3) for r in rows] + [rows[-1][1].reshape(3)] * (K - k)).contiguous()
    sc = None if rows[0][2] is None else _batch_rows([r[2] for r in rows], K, 1)
    ext = None
    if rows[0][3] is not None:
        ext = tuple(_batch_rows([r[3][n] for r in rows], K, w) for n, w in enumerate((3, 9, 1)))
    return A, tr, sc, ext


def _stack_cameras(cams, K, bg_color, scaling_modifier, sh_degree):
    """The settings of a batch of k <= K frames: the one camera dict they share, or their cameras stacked [K,4,4] / [K,3] (the tail
    padded with the last frame's)."""
    rs = _settings(cams[0], bg_color, scaling_modifier, sh_degree)
    if any(cm is not cams[0] for cm in cams):
        pad = cams + [cams[-1]] * (K - len(cams))
        rs = rs._replace(viewmatrix=torch.stack([cm['world_view_transform'] for cm in pad]).contiguous(),
                         projmatrix=torch.stack([cm['full_proj_transform'] for cm in pad]).contiguous(),
                         campos=torch.stack([cm['camera_center'] for cm in pad]).contiguous())
    return rs


_capacity_floor, _grown = EngineCapacity.floor, EngineCapacity.grown      # (the names the two rules had in this module)


def _optional_inputs(job):
    return job[3] is None, job[4] is None


def _batches(jobs, K, kind=_optional_inputs):
    """The job stream as (index of the first job, batch): at most K consecutive jobs per batch, and a new batch where ``kind(job)``
    -- ``(smpl_scale is None, ext_tfs is None)`` -- changes (frames with and without scale / placement cannot share a launch)."""
    batch, i0 = [], 0
    for i, job in enumerate(jobs):
        if batch and kind(job) != kind(batch[0]):
            yield i0, batch
            batch = []
        if not batch:
            i0 = i
        batch.append(job)
        if len(batch) == K:
            yield i0, batch
            batch = []
    if batch:
        yield i0, batch


class FrameAnimator:
    """Forward-only rendering of posed frames, ``streams`` launches in flight: one pre-allocated engine (workspaces) per stream,
    nothing allocated or synchronised per frame except the read of its pair counts (``overflow.EngineCapacity``: a unit whose
    (tile, Gaussian) pairs exceed the capacity, or whose long-rows hint failed, is rendered again before it is handed out)."""

    def __init__(self, canon, streams=3):
        self.canon = canon
        self.dev = canon['xyz_canon'].device
        if self.dev.type != "cuda":
            raise RuntimeError("sings_amd.posed.FrameAnimator runs on the MI355X only; there is no CPU fallback")
        self.n = max(1, int(streams))
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(self.n)]
        self.engs, self.key, self.cap = [], None, 0
        self.policy = EngineCapacity()
        self._out = FrameOut(self.dev)

    long_rows = property(lambda self: self.policy.long_rows)

    def _engines(self, key, cap):
        """The ``n`` engines of ``key`` (``_unit_key``) that hold at least ``cap`` pairs.  A set of another key or a smaller capacity
        is replaced."""
        if key != self.key or cap > self.cap:
            if self.engs:
                torch.cuda.synchronize(self.dev)                 # (engines in flight are about to be replaced)
            self.engs = []                                       # (drop the old workspaces before the new ones are sized)
            self.engs = [self._build(key, cap) for _ in range(self.n)]
            self.key, self.cap = key, cap
        return self.engs

    def _unit_key(self, unit, K, aux):
        """What decides the engines a unit needs -> (key, Gaussians, image width, height); key = (P, J, W, H, M, K, rot width | None,
        aux)."""
        cam, A = unit[0][0], unit[0][1]
        c = self.canon
        P, rot = int(c['xyz_canon'].shape[0]), c.get('rotmat_canon')
        key = (P, int(A.reshape(-1, 16).shape[0]), int(cam['image_width']), int(cam['image_height']), int(c['shs'].shape[1]), K,
               None if rot is None else int(rot.reshape(P, -1).shape[1]), bool(aux))
        return key, P, key[2], key[3]

    def _build(self, key, cap):
        """One engine of ``key`` with ``cap`` pairs: SkinnedEngine (K None) or SkinnedFramesEngine."""
        from .engine import SkinnedEngine, SkinnedFramesEngine
        P, J, W, H, M, K, rw, aux = key
        if K is None:
            return SkinnedEngine(P, J, W, H, M, self.dev, capacity_pairs=cap)
        return SkinnedFramesEngine(P, J, W, H, M, K, self.dev, capacity_pairs=cap, with_rot=rw is not None,
                                   rot_width=9 if rw is None else rw, aux=aux)

    def _pipeline(self, units, launch, K=None, aux=False, depth=None):
        """What the three public methods go through.  ``units``: an iterable of (index of the first job, unit); a unit is a list of
        one job for a single-frame engine (``K`` None), of at most K jobs for a K-frame engine.  ``launch(e, unit)`` renders the
        unit through engine ``e`` on the current stream -> a tuple of new tensors.  Unit number s goes to engine and stream s % n,
        forked from the caller's stream.  Yields (index, unit, tensors) in order, each once ITS launch has finished and its
        pair counts have been settled (``EngineCapacity.settle``; a unit that fails is rendered again: ``EngineCapacity.redo``).
        ``depth`` None: one unit per engine in flight, whose counts ``num_rendered()`` reads at the hand-out.  ``depth`` = d: up to
        d + 1 units in flight, several per engine, so every launch is followed by a non-blocking copy of its header words 0 and 1
        (pair count R, flags) to pinned memory, and nothing but the unit's event is waited for."""
        cur = torch.cuda.current_stream(self.dev)
        bound = self.n if depth is None else depth + 1
        slots = None if depth is None else [torch.empty(2, dtype=torch.int32).pin_memory() for _ in range(bound)]
        q = deque()

        def render(s, unit, cap, slot=None):
            """Unit number s on engine and stream s % n of a set that holds at least ``cap`` pairs -> (engine, stream, tensors)."""
            key, P, W, H = self._unit_key(unit, K, aux)
            e = self._engines(key, EngineCapacity.floor(max(cap, self.cap), P, W, H))[s % self.n]
            st = self.streams[s % self.n]
            st.wait_stream(cur)                                  # the jobs' tensors were produced on the caller's stream
            with torch.cuda.stream(st):
                out = launch(e, unit)
                for t in out:
                    t.record_stream(cur)                         # ... and the images are used there
                if slot is not None:
                    slot.copy_(e.binning[:8].view(torch.int32), non_blocking=True)
            return e, st, out

        def again(s, unit, cap):
            torch.cuda.synchronize(self.dev)                     # rare: the engines are idle, a grown set may replace them
            e, st, out = render(s, unit, cap)
            with torch.cuda.stream(st):
                Rs = e.num_rendered()                            # (waits for the render)
            return out, [Rs] if K is None else Rs[:len(unit)], e.cap

        def pop():
            s, i0, unit, e, st, out, ev, slot = q.popleft()
            ev.synchronize()
            # compared with the capacity of the engine that rendered it: an earlier pop may have grown the set while this unit
            # was queued, and a count between the two capacities means a background-only image
            if slot is None:
                with torch.cuda.stream(st):
                    Rs = e.num_rendered()                        # (this engine has nothing else queued)
                cap = self.policy.settle([Rs] if K is None else Rs[:len(unit)], e.cap)
            else:
                cap = self.policy.settle([int(slot[0])], e.cap, int(slot[1]))
            if cap is not None:
                # on engine s % n again: its own counts have been read, the queued units' are in their slots or on other engines
                out = self.policy.redo(cap, lambda cap: again(s, unit, cap))
            return i0, unit, out

        for s, (i0, unit) in enumerate(units):
            while len(q) >= bound:
                yield pop()
            slot = None if slots is None else slots[s % bound]
            e, st, out = render(s, unit, 0, slot)
            ev = torch.cuda.Event()
            ev.record(st)
            q.append((s, i0, unit, e, st, out, ev, slot))
        while q:
            yield pop()

    def _launch(self, e, job, bg_color, scaling_modifier):
        """One frame on the current stream: ``job`` (a tuple of ``render_round``) through engine ``e`` -> the clamped image (a new
        tensor: the engine's image buffer is reused)."""
        cam, A, transl, smpl_scale, ext = job
        c = self.canon
        e.set_camera(_settings(cam, bg_color, scaling_modifier, c['active_sh_degree']), long_rows=self.long_rows)
        e.set_frame(c['xyz_canon'], c.get('rotmat_canon'), c['lbs_weights'], A, smpl_scale, transl, ext)
        e.forward(c['shs'], c['opacity'], c['scales'])
        return (torch.clamp(e.color, 0.0, 1.0),)

    def render_round(self, jobs, bg_color, scaling_modifier=1.0):
        """jobs: up to ``streams`` tuples (camera dict, A_cano2pose [J,4,4], transl | None, smpl_scale | None,
        ext_tfs | None) -> list of clamped images [3,H,W] (the keys 'render' of get_render_pkg_fused)."""
        assert 0 < len(jobs) <= self.n
        launch = lambda e, unit: self._launch(e, unit[0], bg_color, scaling_modifier)
        return [out[0] for _, _, out in self._pipeline(((i, [job]) for i, job in enumerate(jobs)), launch)]

    def render_frames(self, jobs, bg_color, scaling_modifier=1.0, depth=None):
        """Pipelined variant: ``jobs`` is an iterable of the tuples ``render_round`` takes; frame i goes to stream
        i % streams and NOTHING waits between frames -- a frame is handed out (in order) once ITS forward has finished
        (its pair count comes back with an asynchronous copy, checked then), while up to ``depth`` later frames are
        already queued.  Yields (index, clamped image)."""
        depth = 2 * self.n if depth is None else max(1, int(depth))
        launch = lambda e, unit: self._launch(e, unit[0], bg_color, scaling_modifier)
        for i, _, out in self._pipeline(((i, [job]) for i, job in enumerate(jobs)), launch, depth=depth):
            yield i, out[0]

    def render_frames_batched(self, jobs, bg_color, frames_per_launch=8, scaling_modifier=1.0, out="float32", return_aux=False):
        """``render_frames`` with K = ``frames_per_launch`` consecutive frames per DISPATCH: the reference's chunk
        (``SinGS.forward_chunk``, sings_hybrid.py:474-569, rendered one frame at a time at gs_trainer.py:684-714) goes through
        every kernel of the forward once -- canonical inputs read once for the K poses, K frames' worth of workgroups for the
        latency-bound kernels.  One launch per stream in flight.  Jobs as in ``render_round``; every frame may have its own camera,
        ``smpl_scale`` and ``ext_tfs`` (a batch's values are stacked -- one per frame, SgFrameBatch.placement -- unless its frames
        share one: the same tensor, or rows of an ``.expand`` view).  A frame without ``smpl_scale`` / ``ext_tfs`` starts a new batch
        when its neighbour has one.  Yields (index, clamped image) in order; images are bit-identical to the per-frame path's.
        ``out``: "float32" (the clamped [3,H,W] image), "rgb8" / "bgr8" (uint8 [H,W,3], ``frames_to_u8``: one conversion launch
        per batch), "jpeg" or ("jpeg", quality) (a ``bytes`` per frame: a complete baseline JPEG file at quality 90 or ``quality``,
        encoded on the device behind that conversion -- ``video.JpegEncoder``, one per engine key; the padded frames of a last batch
        are not encoded), "png" (a ``bytes`` per frame: a complete PNG file, lossless, by ``png.PngEncoder`` in the same place).
        ``return_aux``: yields (index, image, depth [1,H,W], alpha [1,H,W]) -- the maps of
        ``get_render_pkg_fused(return_aux=True)``, re-rendered fallbacks included; the maps stay fp32."""
        c = self.canon

        def set_inputs(e, batch):
            A, tr, sc, ext = _stack_poses([j[1:] for j in batch], e.K)
            rs = _stack_cameras([j[0] for j in batch], e.K, bg_color, scaling_modifier, c['active_sh_degree'])
            e.set_camera(rs, long_rows=self.long_rows)
            e.set_frames(c['xyz_canon'], c.get('rotmat_canon'), c['lbs_weights'], A, sc, tr, ext)
            e.forward(c['shs'], c['opacity'], c['scales'])

        return self._render_batched(jobs, set_inputs, _optional_inputs, frames_per_launch, out, return_aux)

    def _render_batched(self, jobs, set_inputs, kind, frames_per_launch, out, return_aux):
        """The body of ``render_frames_batched``, here and in ``scene_anim.SceneAnimator``: ``set_inputs(e, batch)`` renders a batch of
        at most ``e.K`` jobs through engine ``e`` on the current stream; ``kind(job)``: what must agree within a batch (``_batches``)."""
        spec = parse_out(out)
        K = max(1, min(int(frames_per_launch), _lib.MAX_FRAMES))

        def launch(e, batch):
            set_inputs(e, batch)
            # [K,3,H,W] (or [K,H,W,3] uint8): a new tensor, the engine's image buffer is reused (so are its map buffers)
            img = self._out.convert(spec, e.color)
            return (img, e.depth.clone(), e.alpha.clone()) if return_aux else (img,)

        for i0, batch, outs in self._pipeline(_batches(jobs, K, kind), launch, K=K, aux=return_aux):
            outs = (self._out.finish(spec, outs[0], len(batch)),) + tuple(outs[1:])
            for k in range(len(batch)):
                yield (i0 + k,) + tuple(t[k] for t in outs)


@torch.no_grad()
def animate_chunk(canon, poses, joints_rest, A_t2cano, cameras, bg_color, transl=None, smpl_scale=None, ext_tfs=None,
                  parents=SMPL_PARENTS, chunk_size=16, streams=1, animator=None, frames_per_launch=1, out="float32",
                  return_aux=False):
    """Renders frames ``poses[f]`` with camera dict ``cameras[f]`` (or one shared dict); yields (f, image[3,H,W]).

    canon: dict(xyz_canon, rotmat_canon|None, scales, opacity, shs, lbs_weights, active_sh_degree);
    transl [F,3] or None; smpl_scale: [1] (every frame) or [F,1] / [F] (one per frame: AnimDataset_opt.get_chunk) or None;
    ext_tfs: per-frame tuple (trans[F,3], rotmat[F,3,3], scale[F,1]) -- the reference's ``.expand`` views of one placement
    included -- or None.
    streams > 1 (or an existing ``animator``): that many frames in flight (FrameAnimator); same images.
    frames_per_launch = K > 1: K consecutive frames per DISPATCH (FrameAnimator.render_frames_batched), one such launch per stream
    in flight, with or without ext_tfs / per-frame smpl_scale; same images.
    out: "float32" (clamped [3,H,W]) or "rgb8" / "bgr8": uint8 [H,W,3] on the GPU (frames_to_u8: one launch per batch of K frames,
    per frame elsewhere) -- the reference's (clamp * 255).astype(uint8) + cvtColor (gs_trainer.py:717-719) -- or "jpeg" /
    ("jpeg", quality): a ``bytes`` per frame, a complete JPEG file at quality 90 / ``quality`` encoded on the device
    (``video.JpegEncoder``; ``video.animate_to_video`` writes them into a Motion-JPEG AVI) -- or "png": a ``bytes`` per frame, a
    complete PNG file encoded on the device (``png.PngEncoder``; ``png.animate_to_frames`` writes them into numbered files).
    return_aux: yields (f, image, depth [1,H,W], alpha [1,H,W]) -- the maps of get_render_pkg_fused(return_aux=True), fp32 -- on the
    K-frame path and on the plain per-frame loop; the ``streams`` > 1 per-frame path (render_frames) has no maps: ValueError."""
    F = poses.shape[0]
    spec = parse_out(out)
    one = FrameOut(canon['xyz_canon'].device)                     # of the two per-frame paths: K = 1

    def per_frame(img):
        """A clamped frame [3,H,W] of a per-frame path through the output stage."""
        return img if spec.bgr is None else one.finish(spec, one.convert(spec, img[None]), 1)[0]

    inv_cano = torch.inverse(A_t2cano)
    batched = int(frames_per_launch) > 1
    # one smpl_scale per frame ([F,1] / [F]: frame f's row) or one for all
    scale_of = (lambda f: smpl_scale) if smpl_scale is None or smpl_scale.numel() == 1 else (lambda f: smpl_scale.reshape(-1, 1)[f])

    def jobs(jt):
        """The frames as ``FrameAnimator.render_round``'s tuples, the kinematic chain ``jt`` frames at a time."""
        for c0 in range(0, F, jt):
            A = joint_transforms_batch(poses[c0:c0 + jt], joints_rest, parents) @ inv_cano[None]
            for i in range(A.shape[0]):
                f = c0 + i
                yield (cameras[f] if isinstance(cameras, (list, tuple)) else cameras, A[i],
                       None if transl is None else transl[f], scale_of(f),
                       None if ext_tfs is None else (ext_tfs[0][f], ext_tfs[1][f], ext_tfs[2][f]))

    if animator is None and (streams > 1 or batched):
        animator = FrameAnimator(canon, streams)
    if animator is not None:
        # ONE pipelined pass over all chunks: the joint transforms of chunk k + 1 are computed (on the caller's stream) while
        # the frames of chunk k are still in flight -- nothing drains between chunks
        # (the kinematic chain is ~80 small launches per chunk whatever its size: at least 128 frames per chain here)
        jt = max(int(chunk_size), 128)
        if batched:
            yield from animator.render_frames_batched(jobs(jt), bg_color, frames_per_launch=int(frames_per_launch), out=out,
                                                      return_aux=return_aux)
        elif return_aux:
            raise ValueError("animate_chunk: return_aux needs frames_per_launch > 1 or the per-frame loop (streams=1, no animator); "
                             "FrameAnimator.render_frames has no depth / alpha maps")
        else:
            for f, img in animator.render_frames(jobs(jt), bg_color):
                yield f, per_frame(img)
        return
    for f, (cam, A, tr, sc, ext) in enumerate(jobs(chunk_size)):
        pkg = get_render_pkg_fused(cam, canon, A, bg_color, smpl_scale=sc, transl=tr, ext_tfs=ext, return_aux=return_aux)
        if return_aux:
            yield f, per_frame(pkg["render"]), pkg["depth"], pkg["alpha"]
        else:
            yield f, per_frame(pkg["render"])
