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
import numpy as np
import torch

from . import _lib
from ._marshal import _ptr, _stream
from .body import SMPL_PARENTS, rodrigues
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


def frames_to_u8(img, bgr=False):
    """[3,H,W] or [K,3,H,W] fp32 frames on the GPU -> uint8 [H,W,3] / [K,H,W,3] on the GPU: the reference's last step,
    ``(clamp(x, 0, 1) * 255).astype(uint8)`` (+ cvtColor to BGR with ``bgr``: gs_trainer.py:717-719), in ONE launch
    (sg_frames_to_u8; NaN gives 0).  A quarter of the fp32 bytes to copy to the host."""
    import ctypes as C
    if not torch.is_tensor(img) or img.device.type != "cuda":
        raise RuntimeError("sings_amd.posed.frames_to_u8 runs on the MI355X only; there is no CPU fallback")
    if img.dtype != torch.float32 or img.dim() not in (3, 4) or img.shape[-3] != 3:
        raise ValueError(f"frames_to_u8: fp32 [3,H,W] or [K,3,H,W] expected, got {img.dtype} {tuple(img.shape)}")
    x = img.contiguous()
    K, H, W = (1 if x.dim() == 3 else int(x.shape[0])), int(x.shape[-2]), int(x.shape[-1])
    out = torch.empty(tuple(x.shape[:-3]) + (H, W, 3), dtype=torch.uint8, device=x.device)
    if out.numel() == 0:
        return out
    _lib.check(_lib.load().sg_frames_to_u8(K, W, H, _ptr(x), int(bool(bgr)), _ptr(out),
                                           _stream(x.device)), "frames_to_u8")
    return out


_OUT = {"float32": None, "rgb8": False, "bgr8": True}      # out= of the animation paths -> frames_to_u8(bgr=...)


def _out_bgr(out):
    if out not in _OUT:
        raise ValueError(f"out must be one of {sorted(_OUT)}, got {out!r}")
    return _OUT[out]


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


def _capacity_floor(cap, P, W, H):                   # the FrameAnimator's engines: 8 pairs per Gaussian + 1 per tile, at least
    return max(cap, 8 * P + ((W + 15) // 16) * ((H + 15) // 16), 1 << 16)


def _grown(need):                                    # ... and what a count of `need` pairs asks for
    return need + need // 4 + 1024


class FrameAnimator:
    """Forward-only rendering of posed frames, ``streams`` frames in flight: one pre-allocated SkinnedEngine (workspaces)
    per stream, nothing allocated or synchronised per frame except one read of the pair counts per round (a frame whose
    (tile, Gaussian) pairs exceed the capacity is re-rendered after the engines have grown)."""

    def __init__(self, canon, streams=3):
        self.canon = canon
        self.dev = canon['xyz_canon'].device
        if self.dev.type != "cuda":
            raise RuntimeError("sings_amd.posed.FrameAnimator runs on the MI355X only; there is no CPU fallback")
        self.n = max(1, int(streams))
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(self.n)]
        self.engs, self.shape, self.cap = [], None, 0
        self._fengs, self._fshape, self._fcap = [], None, 0             # (the K-frame engines: _frame_engines)
        # SG_FLAG_LONG_ROWS (direct binning of few-tile frames: no tile list beyond 16384 entries), passed optimistically: every path
        # below reads the frames' counts before it hands an image out, and a frame that reports NUM_RENDERED_LONG_LIST is rendered
        # again without the hint -- which then stays off
        self.long_rows = True

    def _engines(self, J, W, H, cap):
        from .engine import SkinnedEngine
        c = self.canon
        P, M = int(c['xyz_canon'].shape[0]), int(c['shs'].shape[1])
        if self.shape != (P, J, W, H, M) or cap > self.cap:
            self.engs = []                                       # (drop the old workspaces before the new ones are sized)
            self.engs = [SkinnedEngine(P, J, W, H, M, self.dev, capacity_pairs=cap) for _ in range(self.n)]
            self.shape, self.cap = (P, J, W, H, M), cap
        return self.engs

    def _settle(self, counts, cap, flags=0):
        """Frames rendered with capacity ``cap`` have reported their pair counts (``num_rendered()``, or the header's count and
        flag word of a frame whose count was not read): drops the long-rows hint for good if a list outgrew its row.  Returns None
        if the frames stand, else the capacity to render them again with: ``cap`` after a NUM_RENDERED_LONG_LIST count (it hides
        the frame's R: the plain path counts it), ``_grown(R)`` if R exceeded ``cap``."""
        if self.long_rows and min(counts) == _lib.NUM_RENDERED_LONG_LIST:
            self.long_rows = False
            return cap
        long_list = bool(flags & _lib.HDR_FLAG_LONG_LIST)        # (the header's R is the frame's: it may also have overflowed)
        if long_list:
            self.long_rows = False
        need = max(counts)
        if need > cap:
            return _grown(need)
        return cap if long_list else None

    def _launch(self, e, job, bg_color, scaling_modifier, cur):
        """One frame on the current stream: ``job`` (a tuple of ``render_round``) through engine ``e`` -> the clamped image, for
        use on stream ``cur``."""
        cam, A, transl, smpl_scale, ext = job
        c = self.canon
        e.color = torch.empty((3, e.H, e.W), dtype=torch.float32, device=self.dev)    # handed to the caller
        e.set_camera(_settings(cam, bg_color, scaling_modifier, c['active_sh_degree']), long_rows=self.long_rows)
        e.set_frame(c['xyz_canon'], c.get('rotmat_canon'), c['lbs_weights'], A, smpl_scale, transl, ext)
        e.forward(c['shs'], c['opacity'], c['scales'])
        img = torch.clamp(e.color, 0.0, 1.0)
        img.record_stream(cur)
        return img

    def render_round(self, jobs, bg_color, scaling_modifier=1.0):
        """jobs: up to ``streams`` tuples (camera dict, A_cano2pose [J,4,4], transl | None, smpl_scale | None,
        ext_tfs | None) -> list of clamped images [3,H,W] (the keys 'render' of get_render_pkg_fused)."""
        c = self.canon
        assert 0 < len(jobs) <= self.n
        J = int(jobs[0][1].reshape(-1, 16).shape[0])
        W, H = int(jobs[0][0]['image_width']), int(jobs[0][0]['image_height'])
        P = int(c['xyz_canon'].shape[0])
        cap = _capacity_floor(self.cap, P, W, H)
        cur = torch.cuda.current_stream(self.dev)
        while True:
            engs = self._engines(J, W, H, cap)
            outs = []
            for st in self.streams[:len(jobs)]:
                st.wait_stream(cur)
            for job, e, st in zip(jobs, engs, self.streams):
                with torch.cuda.stream(st):
                    outs.append(self._launch(e, job, bg_color, scaling_modifier, cur))
            for st in self.streams[:len(jobs)]:
                cur.wait_stream(st)
            cap = self._settle([e.num_rendered() for e in engs[:len(jobs)]], self.cap)
            if cap is None:
                return outs


    def render_frames(self, jobs, bg_color, scaling_modifier=1.0, depth=None):
        """Pipelined variant: ``jobs`` is an iterable of the tuples ``render_round`` takes; frame i goes to stream
        i % streams and NOTHING waits between frames -- a frame is handed out (in order) once ITS forward has finished
        (its pair count comes back with an asynchronous copy, checked then), while up to ``depth`` later frames are
        already queued.  Yields (index, clamped image)."""
        from collections import deque
        c = self.canon
        depth = 2 * self.n if depth is None else max(1, int(depth))
        cur = torch.cuda.current_stream(self.dev)
        P = int(c['xyz_canon'].shape[0])
        slots = [torch.empty(2, dtype=torch.int32).pin_memory() for _ in range(depth + self.n + 1)]
        q = deque()

        def submit(i, job):
            cam, A = job[0], job[1]
            J = int(A.reshape(-1, 16).shape[0])
            W, H = int(cam['image_width']), int(cam['image_height'])
            cap = _capacity_floor(self.cap, P, W, H)
            if self.shape != (P, J, W, H, int(c['shs'].shape[1])) or cap > self.cap:
                torch.cuda.synchronize(self.dev)                 # (engines in flight are about to be replaced)
            e, st = self._engines(J, W, H, cap)[i % self.n], self.streams[i % self.n]
            st.wait_stream(cur)                                  # the job's tensors were produced on the caller's stream
            with torch.cuda.stream(st):
                img = self._launch(e, job, bg_color, scaling_modifier, cur)
                slot = slots[i % len(slots)]
                slot.copy_(e.binning[:8].view(torch.int32), non_blocking=True)      # header words 0, 1 = pair count R, flags
                ev = torch.cuda.Event()
                ev.record(st)
            q.append((i, job, img, ev, slot, e.cap))          # (the capacity THIS frame was rendered with)

        def pop():
            i, job, img, ev, slot, cap_used = q.popleft()
            ev.synchronize()
            # compared with the capacity of the engine that rendered it: an earlier pop may have grown self.cap while this
            # frame was still queued, and a count between the two capacities means a background-only image
            cap = self._settle([int(slot[0])], cap_used, int(slot[1]))
            if cap is not None:                                  # rare: grow the workspaces / drop the hint, render this frame again
                torch.cuda.synchronize(self.dev)
                if cap > cap_used:
                    self._engines(self.shape[1], self.shape[2], self.shape[3], cap)
                img = self.render_round([job], bg_color, scaling_modifier)[0]
                torch.cuda.synchronize(self.dev)
            return i, img

        for i, job in enumerate(jobs):
            submit(i, job)
            while len(q) > depth:
                yield pop()
        while q:
            yield pop()


    # ---- K frames of the same Gaussians per dispatch (round 4: sings_amd.engine.SkinnedFramesEngine) -------------------------
    def _frame_engines(self, J, W, H, K, cap, aux=False):
        from .engine import SkinnedFramesEngine
        c = self.canon
        P, M = int(c['xyz_canon'].shape[0]), int(c['shs'].shape[1])
        rot = c.get('rotmat_canon')
        key = (P, J, W, H, M, K, None if rot is None else int(rot.reshape(P, -1).shape[1]), bool(aux))
        if self._fshape != key or cap > self._fcap:
            self._fengs = []
            self._fengs = [SkinnedFramesEngine(P, J, W, H, M, K, self.dev, capacity_pairs=cap, with_rot=rot is not None,
                                               rot_width=9 if rot is None else key[6], aux=aux) for _ in range(self.n)]
            self._fshape, self._fcap = key, cap
        return self._fengs

    def render_frames_batched(self, jobs, bg_color, frames_per_launch=8, scaling_modifier=1.0, out="float32", return_aux=False):
        """``render_frames`` with K = ``frames_per_launch`` consecutive frames per DISPATCH: the reference's chunk
        (``SinGS.forward_chunk``, sings_hybrid.py:474-569, rendered one frame at a time at gs_trainer.py:684-714) goes through
        every kernel of the forward once -- canonical inputs read once for the K poses, K frames' worth of workgroups for the
        latency-bound kernels.  One launch per stream in flight.  Jobs as in ``render_round``; every frame may have its own camera,
        ``smpl_scale`` and ``ext_tfs`` (a batch's values are stacked -- one per frame, SgFrameBatch.placement -- unless its frames
        share one: the same tensor, or rows of an ``.expand`` view).  A frame without ``smpl_scale`` / ``ext_tfs`` starts a new batch
        when its neighbour has one.  Yields (index, clamped image) in order; images are bit-identical to the per-frame path's.
        ``out``: "float32" (the clamped [3,H,W] image), "rgb8" / "bgr8" (uint8 [H,W,3], ``frames_to_u8``: one conversion launch
        per batch).  ``return_aux``: yields (index, image, depth [1,H,W], alpha [1,H,W]) -- the maps of
        ``get_render_pkg_fused(return_aux=True)``, re-rendered fallbacks included; the maps stay fp32."""
        from collections import deque
        c = self.canon
        bgr = _out_bgr(out)
        K = max(1, min(int(frames_per_launch), 16))
        cur = torch.cuda.current_stream(self.dev)
        P = int(c['xyz_canon'].shape[0])
        q = deque()
        state = dict(b=0)

        def launch(i0, batch, e, st):
            k = len(batch)
            cams = [j[0] for j in batch]
            A = torch.stack([j[1].reshape(-1, 16) for j in batch] + [batch[-1][1].reshape(-1, 16)] * (K - k)).contiguous()
            tr = None
            if batch[0][2] is not None:
                tr = torch.stack([j[2].reshape(3) for j in batch] + [batch[-1][2].reshape(3)] * (K - k)).contiguous()
            sc = None if batch[0][3] is None else _batch_rows([j[3] for j in batch], K, 1)
            ext = None
            if batch[0][4] is not None:
                ext = tuple(_batch_rows([j[4][n] for j in batch], K, w) for n, w in enumerate((3, 9, 1)))
            st.wait_stream(cur)                                  # the jobs' tensors were produced on the caller's stream
            with torch.cuda.stream(st):
                rs = _settings(cams[0], bg_color, scaling_modifier, c['active_sh_degree'])
                if any(cm is not cams[0] for cm in cams):        # per-frame cameras: stacked [K,4,4] / [K,3]
                    pad = cams + [cams[-1]] * (K - k)
                    rs = rs._replace(viewmatrix=torch.stack([cm['world_view_transform'] for cm in pad]).contiguous(),
                                     projmatrix=torch.stack([cm['full_proj_transform'] for cm in pad]).contiguous(),
                                     campos=torch.stack([cm['camera_center'] for cm in pad]).contiguous())
                e.set_camera(rs, long_rows=self.long_rows)
                e.set_frames(c['xyz_canon'], c.get('rotmat_canon'), c['lbs_weights'], A, sc, tr, ext)
                e.forward(c['shs'], c['opacity'], c['scales'])
                # [K,3,H,W] (or [K,H,W,3] uint8): a new tensor, the engine's image buffer is reused
                img = torch.clamp(e.color, 0.0, 1.0) if bgr is None else frames_to_u8(e.color, bgr)
                maps = (e.depth.clone(), e.alpha.clone()) if return_aux else None      # (so are its map buffers)
                ev = torch.cuda.Event(); ev.record(st)
            img.record_stream(cur)
            if maps is not None:
                for m in maps:
                    m.record_stream(cur)
            return (img, maps), ev

        def submit(i0, batch):
            J = int(batch[0][1].reshape(-1, 16).shape[0])
            W, H = int(batch[0][0]['image_width']), int(batch[0][0]['image_height'])
            cap = _capacity_floor(self._fcap, P, W, H)
            engs = self._frame_engines(J, W, H, K, cap, return_aux)
            e, st = engs[state['b'] % self.n], self.streams[state['b'] % self.n]
            state['b'] += 1
            img, ev = launch(i0, batch, e, st)
            q.append((i0, batch, img, ev, e, st))

        def pop():
            i0, batch, img, ev, e, st = q.popleft()
            ev.synchronize()
            with torch.cuda.stream(st):
                Rs = e.num_rendered()                            # (this engine has nothing else queued: one launch per engine)
            if self._settle(Rs[:len(batch)], e.cap) is not None:    # rare: grow the workspaces / drop the hint, render this batch again
                torch.cuda.synchronize(self.dev)
                # (a NEW set of engines either way: the queued batches keep theirs, whose counts are still to be read)
                need = max(max(Rs[:len(batch)]), self._fcap - self._fcap // 5)
                J, W, H = self._fshape[1], self._fshape[2], self._fshape[3]
                e2 = self._frame_engines(J, W, H, K, _grown(need), return_aux)[0]
                img, ev = launch(i0, batch, e2, self.streams[0])
                torch.cuda.synchronize(self.dev)
                Rs2 = e2.num_rendered()
                if max(Rs2[:len(batch)]) > e2.cap:               # (both at once: the plain path has now counted the batch)
                    need = max(Rs2[:len(batch)])
                    e2 = self._frame_engines(J, W, H, K, _grown(need), return_aux)[0]
                    img, ev = launch(i0, batch, e2, self.streams[0])
                    torch.cuda.synchronize(self.dev)
            img, maps = img
            for k in range(len(batch)):
                if maps is not None:
                    yield i0 + k, img[k], maps[0][k], maps[1][k]
                else:
                    yield i0 + k, img[k]

        kind = lambda job: (job[3] is None, job[4] is None)     # (frames with and without scale / placement: separate batches)
        batch, i0, i = [], 0, 0
        for i, job in enumerate(jobs):
            if batch and kind(job) != kind(batch[0]):
                while len(q) >= self.n:
                    yield from pop()
                submit(i0, batch)
                batch = []
            if not batch:
                i0 = i
            batch.append(job)
            if len(batch) == K:
                while len(q) >= self.n:
                    yield from pop()
                submit(i0, batch)
                batch = []
        if batch:
            while len(q) >= self.n:
                yield from pop()
            submit(i0, batch)
        while q:
            yield from pop()


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
    per frame elsewhere) -- the reference's (clamp * 255).astype(uint8) + cvtColor (gs_trainer.py:717-719).
    return_aux: yields (f, image, depth [1,H,W], alpha [1,H,W]) -- the maps of get_render_pkg_fused(return_aux=True), fp32 -- on the
    K-frame path and on the plain per-frame loop; the ``streams`` > 1 per-frame path (render_frames) has no maps: ValueError."""
    F = poses.shape[0]
    bgr = _out_bgr(out)
    to_out = (lambda img: img) if bgr is None else (lambda img: frames_to_u8(img, bgr))
    inv_cano = torch.inverse(A_t2cano)
    batched = int(frames_per_launch) > 1
    # one smpl_scale per frame ([F,1] / [F]: frame f's row) or one for all
    scale_of = (lambda f: smpl_scale) if smpl_scale is None or smpl_scale.numel() == 1 else (lambda f: smpl_scale.reshape(-1, 1)[f])
    if animator is None and (streams > 1 or batched):
        animator = FrameAnimator(canon, streams)
    if animator is not None:
        # ONE pipelined pass over all chunks: the joint transforms of chunk k + 1 are computed (on the caller's stream) while
        # the frames of chunk k are still in flight -- nothing drains between chunks
        # (the kinematic chain is ~80 small launches per chunk whatever its size: at least 128 frames per chain here)
        jt = max(int(chunk_size), 128)

        def jobs():
            for c0 in range(0, F, jt):
                A = joint_transforms_batch(poses[c0:c0 + jt], joints_rest, parents) @ inv_cano[None]
                for i in range(A.shape[0]):
                    f = c0 + i
                    yield (cameras[f] if isinstance(cameras, (list, tuple)) else cameras, A[i],
                           None if transl is None else transl[f], scale_of(f),
                           None if ext_tfs is None else (ext_tfs[0][f], ext_tfs[1][f], ext_tfs[2][f]))
        if batched:
            yield from animator.render_frames_batched(jobs(), bg_color, frames_per_launch=int(frames_per_launch), out=out,
                                                      return_aux=return_aux)
        elif return_aux:
            raise ValueError("animate_chunk: return_aux needs frames_per_launch > 1 or the per-frame loop (streams=1, no animator); "
                             "FrameAnimator.render_frames has no depth / alpha maps")
        else:
            for f, img in animator.render_frames(jobs(), bg_color):
                yield f, to_out(img)
        return
    for c0 in range(0, F, chunk_size):
        A = joint_transforms_batch(poses[c0:c0 + chunk_size], joints_rest, parents) @ inv_cano[None]
        for i in range(A.shape[0]):
            f = c0 + i
            cam = cameras[f] if isinstance(cameras, (list, tuple)) else cameras
            ext = None if ext_tfs is None else (ext_tfs[0][f], ext_tfs[1][f], ext_tfs[2][f])
            pkg = get_render_pkg_fused(cam, canon, A[i], bg_color, smpl_scale=scale_of(f),
                                       transl=None if transl is None else transl[f], ext_tfs=ext, return_aux=return_aux)
            if return_aux:
                yield f, to_out(pkg["render"]), pkg["depth"], pkg["alpha"]
            else:
                yield f, to_out(pkg["render"])
