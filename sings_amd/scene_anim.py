"""Several avatars in one frame through the fused K-frame forward (include/sings_scene.h).

The reference renders a scene by posing every avatar (``SinGaussianTrainer.animate_more_without_render``, gs_trainer.py:732-754),
concatenating the posed Gaussians and rasterizing once (``gs_renderer_multiple.get_render_pkgs``, gs_renderer_multiple.py:12-68);
``sings_amd.renderer.get_render_pkgs`` is that renderer's twin.  Here the avatars stay canonical: the LBS-fused preprocess skins a
block of 256 Gaussians with the joints, weights and placement of the avatar it belongs to and writes ONE set of geometry records,
K frames per dispatch -- nothing is concatenated, and no posed value touches HBM unless it is asked for.

 * ``SceneFramesEngine``: pre-allocated workspaces for S avatars and K frames (``sg_scene_forward_frames[_aux]``);
 * ``SceneAnimator``: ``posed.FrameAnimator``'s pipeline and capacity policy (``overflow.EngineCapacity``) over such engines;
 * ``animate_scene``: ``posed.animate_chunk`` for a list of avatars.

Forward only, as the reference uses it (no_grad).  Avatar s owns the Gaussian ids [starts[s], starts[s] + P_s) of ``radii`` and of
the posed outputs.  One SH width M and one ``sh_degree`` for the scene (the reference takes the first avatar's degree for all).
"""
import ctypes as C

import torch

from . import _lib
from ._marshal import _frame_rows, _ptr, _scene_structs
from .body import SMPL_PARENTS
from .engine import _FramesEngine
from .posed import FrameAnimator, _stack_cameras, _stack_poses, joint_transforms_batch

_FORWARD_ONLY = "SceneFramesEngine: a scene of avatars is forward-only (the reference renders it under no_grad)"


def _shape(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t).__name__


class SceneFramesEngine(_FramesEngine):
    """K frames of S avatars per call.  ``avatars``: [(P_s, J_s, rot width)] with rot width None (isotropic), 9 (rotation matrices)
    or 6 (the decoder's 6-D form).  ``color`` [K,3,H,W], ``radii`` [K,Ptot] (``radii_of(s)``: avatar s's columns), with ``aux``
    ``depth`` / ``alpha`` [K,1,H,W]; ``starts[s]``: the first Gaussian id of avatar s."""

    def __init__(self, avatars, W, H, sh_coeffs, K, device, capacity_pairs, aux=False):
        self.avatars = self.check_avatars(avatars)
        self.starts = [sum(p for p, _, _ in self.avatars[:s]) for s in range(len(self.avatars))]
        super().__init__(sum(p for p, _, _ in self.avatars), W, H, sh_coeffs, device, capacity_pairs, K)
        if not _lib.HAS_SCENE:
            raise RuntimeError("SceneFramesEngine: the loaded library predates include/sings_scene.h (no fallback): rebuild it")
        self.bwd_ws = None                                        # (forward only: the gradient records' workspace goes back to the allocator)
        self.aux, self.sh_planar = bool(aux), False
        self.aux_ws = self.depth = self.alpha = None
        if self.aux:
            f32 = dict(dtype=torch.float32, device=self.dev)
            self.aux_ws = torch.empty(_lib.frames_aux_layout(self.P, self.W, self.H, self.cap, self.K), dtype=torch.uint8, device=self.dev)
            self.depth = torch.empty((self.K, 1, self.H, self.W), **f32)
            self.alpha = torch.empty((self.K, 1, self.H, self.W), **f32)
        self._arr = None

    @staticmethod
    def check_avatars(avatars):
        """[(P, J, rot width | None)] of 1..8 avatars, as a list of int tuples; ValueError otherwise."""
        avatars = [(int(p), int(j), None if rw is None else int(rw)) for p, j, rw in avatars]
        if not 1 <= len(avatars) <= _lib.SCENE_MAX_AVATARS:
            raise ValueError(f"a scene has 1..{_lib.SCENE_MAX_AVATARS} avatars, got {len(avatars)}")
        for s, (p, j, rw) in enumerate(avatars):
            if p < 1 or not 1 <= j <= 64 or rw not in (None, 6, 9):
                raise ValueError(f"avatar {s}: (P, J, rot width) = {(p, j, rw)}: P >= 1, J in 1..64, rot width None, 6 or 9")
        return avatars

    def set_camera(self, raster_settings, short_lists=False, long_rows=False):
        """One camera for the K frames or one per frame ([K,4,4] / [K,3]).  ``short_lists`` / ``long_rows``: the list-length hints of
        ``RasterEngine.set_camera`` (a longer list: ``num_rendered()`` reports NUM_RENDERED_LONG_LIST for that frame)."""
        self._camera(raster_settings, (_lib.FLAG_SHORT_LISTS if short_lists else 0) | (_lib.FLAG_LONG_ROWS if long_rows else 0))

    @staticmethod
    def check_frames(avatars, K, M, frames):
        """``set_frames``'s validation, usable without an engine: ``frames`` [dict(canon=, A=, transl=, smpl_scale=, ext_tfs=)] against
        ``avatars`` [(P, J, rot width | None)], K frames and M SH coefficients -> one dict per avatar of the tensors
        ``_marshal._scene_structs`` takes, every per-frame input as K rows.  ValueError with the offending shape otherwise."""
        if len(frames) != len(avatars):
            raise ValueError(f"set_frames: {len(frames)} avatars, the engine was built for {len(avatars)}")
        out = []
        for s, (fr, (P, J, rw)) in enumerate(zip(frames, avatars)):
            c = fr["canon"]
            want = (("xyz_canon", c["xyz_canon"], (P, 3)), ("lbs_weights", c["lbs_weights"], (P, J)), ("scales", c["scales"], (P, 3)),
                    ("shs", c["shs"], (P, M, 3)))
            for name, t, shape in want:
                if not torch.is_tensor(t) or tuple(t.shape) != shape:
                    raise ValueError(f"avatar {s}: {name} must be {list(shape)}, got {_shape(t)}")
            op = c["opacity"]
            if not torch.is_tensor(op) or op.numel() != P or (op.dim() and op.shape[0] != P):
                raise ValueError(f"avatar {s}: opacity must be [{P},1], got {_shape(op)}")
            rot = c.get("rotmat_canon")
            if (rot is None) != (rw is None) or (rot is not None and (not torch.is_tensor(rot) or rot.dim() < 2 or rot.shape[0] != P
                                                                       or rot[0].numel() != rw or (rw == 6 and rot.dim() != 2))):
                raise ValueError(f"avatar {s}: rotmat_canon must be {None if rw is None else [P, rw]}, got "
                                 f"{None if rot is None else _shape(rot)}")
            A = fr["A"]
            if not torch.is_tensor(A) or A.numel() != K * J * 16 or A.shape[0] != K:
                raise ValueError(f"avatar {s}: A must be [{K},{J},16], got {_shape(A)}")

            def rows(t, w, name):                                 # shared ([w], a leading 1, an .expand view) or [K,w] -> K rows
                x, per_frame = _frame_rows(t, K, w, f"avatar {s}: {name}")
                return x.reshape(K, w) if per_frame else x.reshape(1, w).expand(K, w)
            d = dict(xyz_canon=c["xyz_canon"], rot_canon=None if rot is None else rot.reshape(P, rw), lbs_weights=c["lbs_weights"],
                     scales=c["scales"], opacities=op.reshape(P), shs=c["shs"], A=A.reshape(K, J, 16))
            d["transl"] = None if fr.get("transl") is None else rows(fr["transl"], 3, "transl")
            d["smpl_scale"] = None if fr.get("smpl_scale") is None else rows(fr["smpl_scale"], 1, "smpl_scale").reshape(K)
            ext = fr.get("ext_tfs")
            if ext is not None and len(ext) != 3:
                raise ValueError(f"avatar {s}: ext_tfs must be (trans, rotmat, scale), got {len(ext)} entries")
            for n, (name, w) in enumerate((("ext_trans", 3), ("ext_rot", 9), ("ext_scale", 1))):
                d[name] = None if ext is None else rows(ext[n], w, name.replace("_", " "))
            out.append(d)
        return out

    def set_frames(self, frames):
        """``frames``: one dict per avatar -- ``canon`` (dict(xyz_canon, rotmat_canon | None, scales, opacity, shs, lbs_weights)),
        ``A`` [K,J,4,4] / [K,J,16], and optionally ``transl`` ([K,3] / [3]), ``smpl_scale`` ([K] / [K,1] / [1]), ``ext_tfs`` (trans,
        rotmat, scale: shared, per frame or ``.expand`` views, as ``SkinnedFramesEngine.set_frames``).  Everything is validated
        before anything is stored; a shared value is repeated for the K frames."""
        checked = self.check_frames(self.avatars, self.K, self.M, frames)
        keep = []
        arr = _scene_structs(self.dev, checked, keep)
        self._arr, self._kkeep = arr, keep

    def radii_of(self, s):
        """Avatar s's radii [K, P_s] (a view of ``radii``)."""
        return self.radii[:, self.starts[s]:self.starts[s] + self.avatars[s][0]]

    def forward(self, sync_num_rendered=False, posed_out=None):
        """``posed_out``: optional (xyz [K,Ptot,3], quaternions [K,Ptot,4], scales [K,Ptot,3]) fp32 tensors that also receive the
        posed values; avatar s's in the rows [starts[s], starts[s] + P_s).  Returns the K pair counts with ``sync_num_rendered``."""
        if self._s is None or self._arr is None:
            raise RuntimeError("SceneFramesEngine: set_camera() and set_frames() first")
        if posed_out is not None:
            for x, wdt in zip(posed_out, (3, 4, 3)):
                if (tuple(x.shape) != (self.K, self.P, wdt) or x.dtype != torch.float32 or not x.is_contiguous() or x.device != self.geom.device):
                    raise ValueError(f"posed_out: contiguous fp32 [{self.K},{self.P},3|4|3] tensors on {self.geom.device}")
        pxyz, pq, psc = posed_out if posed_out is not None else (None, None, None)
        nr = (C.c_int64 * self.K)()
        self._s.flags = self._flags()
        self._clean = False
        args = (C.byref(self._s), self.K, self._cam_stride, len(self.avatars), self._arr, _ptr(self.geom), _ptr(self.binning), self.cap,
                _ptr(self.img), _ptr(self.color), _ptr(self.radii), _ptr(pxyz), _ptr(pq), _ptr(psc), nr if sync_num_rendered else None)
        if self.aux:
            _lib.check(self.lib.sg_scene_forward_frames_aux(*args, _ptr(self.aux_ws), _ptr(self.depth), _ptr(self.alpha), self._stream()),
                       "scene forward (frames, depth / alpha maps)")
        else:
            _lib.check(self.lib.sg_scene_forward_frames(*args, self._stream()), "scene forward (frames)")
        self._clean = True
        return [int(v) for v in nr] if sync_num_rendered else None

    def backward(self, *a, **k):
        raise RuntimeError(_FORWARD_ONLY)

    backward_records = backward_gaussians = backward


class SceneAnimator(FrameAnimator):
    """``FrameAnimator`` for a list of avatars: the same pipeline (``streams`` launches in flight, one pre-allocated engine per
    stream) and the same guarantees -- a batch's pair counts are settled before its frames are handed out, a refused long-rows hint
    is dropped and the batch rendered again, an overflow grows the engines (``overflow.EngineCapacity`` with P = the scene's
    Gaussians), at most two re-renders, RuntimeError otherwise."""

    def __init__(self, canons, streams=2):
        self.canons = list(canons)
        if not 1 <= len(self.canons) <= _lib.SCENE_MAX_AVATARS:
            raise ValueError(f"a scene has 1..{_lib.SCENE_MAX_AVATARS} avatars, got {len(self.canons)}")
        super().__init__(self.canons[0], streams)

    def _unit_key(self, unit, K, aux):
        cam, poses = unit[0]
        if len(poses) != len(self.canons):
            raise ValueError(f"a job poses {len(poses)} avatars, the scene has {len(self.canons)}")
        avatars = []
        for c, p in zip(self.canons, poses):
            P, rot = int(c['xyz_canon'].shape[0]), c.get('rotmat_canon')
            avatars.append((P, int(p[0].reshape(-1, 16).shape[0]), None if rot is None else int(rot.reshape(P, -1).shape[1])))
        key = (tuple(avatars), int(cam['image_width']), int(cam['image_height']), int(self.canons[0]['shs'].shape[1]), K, bool(aux))
        return key, sum(a[0] for a in avatars), key[1], key[2]

    def _build(self, key, cap):
        avatars, W, H, M, K, aux = key
        return SceneFramesEngine(avatars, W, H, M, K, self.dev, capacity_pairs=cap, aux=aux)

    def render_round(self, *a, **k):
        raise TypeError("SceneAnimator renders through render_frames_batched (frames_per_launch=1 for one frame per launch)")

    render_frames = render_round

    def render_frames_batched(self, jobs, bg_color, frames_per_launch=8, scaling_modifier=1.0, out="float32", return_aux=False):
        """``jobs``: an iterable of (camera dict, [(A [J,4,4], transl | None, smpl_scale | None, ext_tfs | None) per avatar]); K =
        ``frames_per_launch`` consecutive jobs per dispatch, the last batch padded with its last frame; a job whose avatars carry
        other optional inputs than its neighbour's starts a new batch.  Yields (index, clamped image) in order -- with ``out`` "rgb8" /
        "bgr8" uint8 [H,W,3] (``frames_to_u8``), with "jpeg" / ("jpeg", quality) or "png" a ``bytes`` per frame (a JPEG / PNG file, encoded on
        the device as in ``FrameAnimator.render_frames_batched``), with ``return_aux`` (index, image, depth [1,H,W], alpha [1,H,W])."""
        deg = self.canons[0]['active_sh_degree']

        def set_inputs(e, batch):
            e.set_camera(_stack_cameras([j[0] for j in batch], e.K, bg_color, scaling_modifier, deg), long_rows=self.long_rows)
            frames = []
            for s, c in enumerate(self.canons):
                A, tr, sc, ext = _stack_poses([j[1][s] for j in batch], e.K)
                frames.append(dict(canon=c, A=A, transl=tr, smpl_scale=sc, ext_tfs=ext))
            e.set_frames(frames)
            e.forward()

        kind = lambda job: tuple(x is None for p in job[1] for x in p[1:])
        return self._render_batched(jobs, set_inputs, kind, frames_per_launch, out, return_aux)


@torch.no_grad()
def animate_scene(canons, poses, joints_rest, A_t2cano, cameras, bg_color, transl=None, smpl_scale=None, ext_tfs=None,
                  parents=SMPL_PARENTS, streams=2, animator=None, frames_per_launch=8, out="float32", return_aux=False):
    """``posed.animate_chunk`` for a scene: per-avatar lists ``canons``, ``poses`` ([F, 3 J_s] each), ``joints_rest``, ``A_t2cano``,
    and ``transl`` / ``smpl_scale`` / ``ext_tfs`` (a list with an entry -- or None -- per avatar, in ``animate_chunk``'s conventions; None:
    no avatar has one); ``parents``: one tuple for all avatars or a list of them.  ``cameras``: one dict or a list of F.  Yields what
    ``SceneAnimator.render_frames_batched`` yields, frames in order."""
    S = len(canons)
    F = int(poses[0].shape[0])
    per = lambda x: [None] * S if x is None else list(x)
    transl, smpl_scale, ext_tfs = per(transl), per(smpl_scale), per(ext_tfs)
    parents = list(parents) if isinstance(parents[0], (list, tuple)) else [parents] * S
    if any(len(x) != S for x in (poses, joints_rest, A_t2cano, transl, smpl_scale, ext_tfs, parents)) or any(p.shape[0] != F for p in poses):
        raise ValueError(f"animate_scene: every per-avatar list needs {S} entries and every avatar {F} poses")
    animator = SceneAnimator(canons, streams) if animator is None else animator
    inv = [torch.inverse(a) for a in A_t2cano]
    scale_of = lambda s, f: (smpl_scale[s] if smpl_scale[s] is None or smpl_scale[s].numel() == 1 else smpl_scale[s].reshape(-1, 1)[f])
    jt = 128                                                      # frames per kinematic chain launch (posed.animate_chunk)

    def jobs():
        for c0 in range(0, F, jt):
            A = [joint_transforms_batch(poses[s][c0:c0 + jt], joints_rest[s], parents[s]) @ inv[s][None] for s in range(S)]
            for i in range(A[0].shape[0]):
                f = c0 + i
                yield (cameras[f] if isinstance(cameras, (list, tuple)) else cameras,
                       [(A[s][i], None if transl[s] is None else transl[s][f], scale_of(s, f),
                         None if ext_tfs[s] is None else tuple(x[f] for x in ext_tfs[s])) for s in range(S)])
    yield from animator.render_frames_batched(jobs(), bg_color, frames_per_launch=int(frames_per_launch), out=out, return_aux=return_aux)


def animate_scene_to_video(path, canons, poses, joints_rest, A_t2cano, cameras, bg_color, fps=20, quality=90, frames_per_launch=8, **kwargs):
    """``video.animate_to_video`` for a scene: ``animate_scene(..., out="jpeg")`` into a Motion-JPEG AVI at ``path`` (``kwargs``:
    ``animate_scene``'s other arguments).  Returns the number of frames written."""
    from .video import _write_video
    return _write_video(path, cameras, fps, animate_scene(canons, poses, joints_rest, A_t2cano, cameras, bg_color,
                                                          frames_per_launch=frames_per_launch, out=("jpeg", int(quality)), **kwargs))
