"""Learned per-frame SMPL(-H) poses: the reference's ``global_orient [F,6]`` / ``body_pose [F,23*6]`` parameter tables in the 6-D
rotation form (sings_hybrid.py:142-150, ``create_global_orient`` / ``create_body_pose``), a row of which every training step converts to
axis-angle and runs through the SMPL chain (:370-399) so that the photometric loss moves it through Adam (:761-765).

``PoseTable(frame_idx)`` is that path as ONE launch each way (``sg_pose_transforms[_backward]``, csrc/sg_pose.hip): gather of the
row, rotation_6d_to_matrix -> matrix_to_quaternion -> quaternion_to_axis_angle per joint, Rodrigues, the kinematic chain, ``A = G -
pad(G J)``, ``@ inverse(A_t2cano)``.  The frame index is read from DEVICE memory, so a step captured into a HIP graph at one frame
replays at any other; the gradient comes back DENSE over the whole table (zeros for the rows the step did not visit -- what the
reference's ``table[idx]`` autograd produces), written entirely by the backward launch, without atomics and bit-reproducible.

Two body layouts: ``"smpl"`` (J = 24, the row's 23 body joints) and ``"smplh"`` (J = 52: the row's first 21 body joints,
``body_pose[:63]`` of sings_hybrid.py:387-388; the 30 hand joints are the constants ``tail_pose``, the layer's
``left/right_hand_pose + pose_mean``, zeros by default; the row's joints 22 and 23 are unused and receive zero gradient).

``transl``: the reference puts ``transl`` into the optimiser only ``if ... self.betas.requires_grad`` (sings_hybrid.py:770), so under
every shipped config (``optim_betas: false``) it is NEVER updated, ``optim_trans: true`` notwithstanding.  ``learn_transl`` therefore
defaults to False: the table is a buffer and its rows are only gathered.

There is no CPU path: host tensors raise.
"""
import numpy as np
import torch

from . import _lib
from ._marshal import _ptr, _stream
from .body import SMPL_PARENTS
from .grad_arena import arena_out

NB = _lib.POSE_NB                                          # body joints per row of the body_pose table (SMPL's 23)
_LAYOUT = {"smpl": (24, 23), "smplh": (52, 21)}            # body -> (J, NBu: body joints of the row the chain uses)


def _on_gpu(t, name):
    if not torch.is_tensor(t):
        raise TypeError(f"sings_amd.pose: {name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"sings_amd.pose: {name}: tensors must live on the MI355X (no CPU fallback; got {t.device})")
    if t.dtype != torch.float32:
        raise RuntimeError(f"sings_amd.pose: {name}: float32 only (got {t.dtype})")
    return t.detach().contiguous()


def _check_parents(parents, J):
    parents = tuple(int(x) for x in parents)
    if len(parents) != J:
        raise ValueError(f"sings_amd.pose: parents must have {J} entries, got {len(parents)}")
    if parents[0] >= 0 or any(parents[i] >= i or parents[i] < 0 for i in range(1, J)):
        raise ValueError("sings_amd.pose: parents must describe a tree in topological order: parents[0] < 0, 0 <= parents[i] < i")
    return parents


class _PoseTransforms(torch.autograd.Function):
    """(global_orient, body_pose, transl tables; frame_idx [K] on the device) -> A [K,J,4,4], axis-angle [K,J,3], transl rows [K,3]."""

    @staticmethod
    def forward(ctx, global_orient, body_pose, transl, frame_idx, table):
        lib = _lib.load()
        dev = global_orient.device
        K, F, J, NBu = int(frame_idx.shape[0]), int(global_orient.shape[0]), table.J, table.NBu
        A = torch.empty((K, J, 4, 4), dtype=torch.float32, device=dev)
        aa = torch.empty((K, J, 3), dtype=torch.float32, device=dev)
        rows = torch.empty((K, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sg_pose_transforms(K, F, J, NBu, _ptr(frame_idx), _ptr(global_orient), _ptr(body_pose), _ptr(table.tail_pose),
                                              _ptr(transl), _ptr(table.joints_rest), _ptr(table.parents), _ptr(table.post), _ptr(A),
                                              _ptr(aa), _ptr(rows), _stream(dev)), "pose transforms")
        ctx.table = table
        ctx.save_for_backward(global_orient, body_pose, transl, frame_idx, aa)
        ctx.mark_non_differentiable(aa)
        return A, aa, rows

    @staticmethod
    def backward(ctx, dA, _daa, d_rows):
        lib = _lib.load()
        global_orient, body_pose, transl, frame_idx, aa = ctx.saved_tensors
        table, dev = ctx.table, global_orient.device
        K, F = int(frame_idx.shape[0]), int(global_orient.shape[0])
        dA = dA.contiguous().float()
        want_t = ctx.needs_input_grad[2]
        # the dense gradients, straight into the parameters' slots of a registered gradient arena
        d_go, d_bp = arena_out(global_orient), arena_out(body_pose)
        d_t = arena_out(transl) if want_t else None
        d_rows = d_rows.contiguous().float() if want_t else None
        with torch.cuda.device(dev):
            _lib.check(lib.sg_pose_transforms_backward(K, F, table.J, table.NBu, _ptr(frame_idx), _ptr(global_orient), _ptr(body_pose),
                                                       _ptr(aa), _ptr(table.joints_rest), _ptr(table.parents), _ptr(table.post),
                                                       _ptr(dA), _ptr(d_rows), _ptr(d_go), _ptr(d_bp), _ptr(d_t), _stream(dev)),
                       "pose transforms backward")
        return (d_go if ctx.needs_input_grad[0] else None, d_bp if ctx.needs_input_grad[1] else None, d_t, None, None)


class PoseTable(torch.nn.Module):
    """The pose tables of F frames and what turns a row into ``A_cano2pose``.

    Parameters ``global_orient`` [F,6] and ``body_pose`` [F,138] (``requires_grad`` = ``learn_pose``); ``transl`` [F,3] is a parameter
    only with ``learn_transl`` (see the module docstring: the reference never updates it under its shipped configs), else a buffer.
    Buffers: ``joints_rest`` [J,3], ``parents`` [J] int32, ``post`` [J,4,4] = ``inverse(A_t2cano)``, ``tail_pose`` [J-1-NBu,3].

    ``forward(frame_idx) -> (A_cano2pose, transl_rows)``: an int gives ``[J,4,4]`` and ``[3]``; an int32 tensor ``[K]`` on the GPU
    gives ``[K,J,4,4]`` and ``[K,3]`` (an index outside ``[0, F)`` in such a tensor is clamped into it: the host never reads it).  One
    autograd node, one launch each way; the last call's axis-angle pose ``[K,J,3]`` is kept in ``last_axis_angle``.

    The reference's own ``state_dict`` does not carry the pose tables at all (sings_hybrid.py:169-199): refined poses leave it only
    through ``save_kit_poses``, which writes them in the layout of a training kit's ``poses_optimized.npz``."""

    def __init__(self, global_orient, body_pose, transl, joints_rest, post=None, parents=SMPL_PARENTS, body="smpl", tail_pose=None,
                 learn_pose=True, learn_transl=False):
        super().__init__()
        if body not in _LAYOUT:
            raise ValueError(f"sings_amd.pose: body must be 'smpl' or 'smplh', got {body!r}")
        self.body = body
        self.J, self.NBu = _LAYOUT[body]
        J, n_tail = self.J, self.J - 1 - self.NBu
        F = int(global_orient.shape[0]) if torch.is_tensor(global_orient) and global_orient.dim() == 2 else -1
        for name, t, width in (("global_orient", global_orient, 6), ("body_pose", body_pose, NB * 6), ("transl", transl, 3)):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != width or t.shape[0] != F or F < 1:
                raise ValueError(f"sings_amd.pose: {name} must be [F,{width}] with the same F >= 1 as global_orient, got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if not torch.is_tensor(joints_rest) or tuple(joints_rest.shape) != (J, 3):
            raise ValueError(f"sings_amd.pose: joints_rest must be [{J},3] for body={body!r}")
        if post is not None and tuple(post.shape) != (J, 4, 4):
            raise ValueError(f"sings_amd.pose: post (inverse(A_t2cano)) must be [{J},4,4]")
        if tail_pose is not None and tuple(tail_pose.shape) != (n_tail, 3):
            raise ValueError(f"sings_amd.pose: tail_pose must have {n_tail} rows [{n_tail},3] for body={body!r}, got {tuple(tail_pose.shape)}")
        parents = _check_parents(parents, J)
        dev = global_orient.device
        self.global_orient = torch.nn.Parameter(_on_gpu(global_orient, "global_orient").clone(), requires_grad=bool(learn_pose))
        self.body_pose = torch.nn.Parameter(_on_gpu(body_pose, "body_pose").clone(), requires_grad=bool(learn_pose))
        if learn_transl:
            self.transl = torch.nn.Parameter(_on_gpu(transl, "transl").clone())
        else:
            self.register_buffer("transl", _on_gpu(transl, "transl").clone())
        self.register_buffer("joints_rest", _on_gpu(joints_rest, "joints_rest").clone())
        self.register_buffer("parents", torch.tensor(parents, dtype=torch.int32, device=dev))
        self.register_buffer("post", None if post is None else _on_gpu(post, "post").clone())
        tail = torch.zeros((n_tail, 3), dtype=torch.float32, device=dev) if tail_pose is None else _on_gpu(tail_pose, "tail_pose").clone()
        self.register_buffer("tail_pose", tail)
        self.last_axis_angle = None

    @classmethod
    def from_axis_angle(cls, global_orient, body_pose, transl, joints_rest, A_t2cano=None, parents=SMPL_PARENTS, body="smpl",
                        tail_pose=None, learn_pose=True, learn_transl=False):
        """Tables from a kit's axis-angle poses (``global_orient`` [F,3], ``body_pose`` [F,69], ``transl`` [F,3]), converted with
        ``axis_angle_to_rotation_6d`` as ``create_global_orient`` / ``create_body_pose`` do; ``A_t2cano`` [J,4,4] (None: identity)."""
        from . import rotations as R
        if body not in _LAYOUT:
            raise ValueError(f"sings_amd.pose: body must be 'smpl' or 'smplh', got {body!r}")
        J, n_tail = _LAYOUT[body][0], _LAYOUT[body][0] - 1 - _LAYOUT[body][1]
        if not torch.is_tensor(global_orient) or global_orient.dim() != 2 or global_orient.shape[1] != 3 or global_orient.shape[0] < 1:
            raise ValueError("sings_amd.pose: global_orient must be [F,3] axis-angle")
        F = int(global_orient.shape[0])
        for name, t, width in (("body_pose", body_pose, NB * 3), ("transl", transl, 3)):
            if not torch.is_tensor(t) or tuple(t.shape) != (F, width):
                raise ValueError(f"sings_amd.pose: {name} must be [{F},{width}] (F = {F} rows of global_orient), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if not torch.is_tensor(joints_rest) or tuple(joints_rest.shape) != (J, 3):
            raise ValueError(f"sings_amd.pose: joints_rest must be [{J},3] for body={body!r}")
        if A_t2cano is not None and tuple(A_t2cano.shape) != (J, 4, 4):
            raise ValueError(f"sings_amd.pose: A_t2cano must be [{J},4,4]")
        if tail_pose is not None and tuple(tail_pose.shape) != (n_tail, 3):
            raise ValueError(f"sings_amd.pose: tail_pose must have {n_tail} rows [{n_tail},3] for body={body!r}, got {tuple(tail_pose.shape)}")
        _check_parents(parents, J)
        go, bp = _on_gpu(global_orient, "global_orient"), _on_gpu(body_pose, "body_pose")
        with torch.no_grad():
            go6 = R.axis_angle_to_rotation_6d(go)
            bp6 = R.axis_angle_to_rotation_6d(bp.reshape(F, NB, 3)).reshape(F, NB * 6)
            post = None if A_t2cano is None else torch.inverse(_on_gpu(A_t2cano, "A_t2cano"))
        return cls(go6, bp6, transl, joints_rest, post, parents, body, tail_pose, learn_pose, learn_transl)

    def forward(self, frame_idx):
        F = int(self.global_orient.shape[0])
        dev = self.global_orient.device
        single = not torch.is_tensor(frame_idx)
        if single:
            i = int(frame_idx)
            if not 0 <= i < F:
                raise IndexError(f"sings_amd.pose: frame {i} outside the table's {F} rows")
            frame_idx = torch.tensor([i], dtype=torch.int32, device=dev)
        else:
            if not frame_idx.is_cuda:
                raise RuntimeError(f"sings_amd.pose: frame_idx: tensors must live on the MI355X (no CPU fallback; got {frame_idx.device})")
            if frame_idx.dtype != torch.int32 or frame_idx.dim() != 1 or frame_idx.shape[0] < 1 or not frame_idx.is_contiguous():
                raise ValueError(f"sings_amd.pose: frame_idx must be a contiguous int32 tensor [K], got {frame_idx.dtype} {tuple(frame_idx.shape)}")
        A, aa, rows = _PoseTransforms.apply(self.global_orient, self.body_pose, self.transl, frame_idx, self)
        self.last_axis_angle = aa
        return (A[0], rows[0]) if single else (A, rows)

    @torch.no_grad()
    def axis_angle(self):
        """-> (global_orient [F,3], body_pose [F,69], transl [F,3]) float32 numpy arrays, the kit's layout (``rotation_6d_to_axis_angle``
        of every joint of every row, the SMPL-H layout's unused joints 22 and 23 included)."""
        from . import rotations as R
        F = int(self.global_orient.shape[0])
        go = R.rotation_6d_to_axis_angle(self.global_orient.detach())
        bp = R.rotation_6d_to_axis_angle(self.body_pose.detach().reshape(F, NB, 6)).reshape(F, NB * 3)
        return tuple(t.cpu().numpy().astype(np.float32) for t in (go, bp, self.transl.detach()))

    def save_kit_poses(self, path, betas):
        """Write the (refined) poses as an ``.npz`` with the keys, shapes and dtypes of a training kit's ``poses_optimized.npz``:
        ``global_orient`` [F,3], ``body_pose`` [F,69], ``transl`` [F,3] and the kit's own ``betas`` passed through unchanged (the
        table does not know the shape coefficients or how many the kit carries: [16] in the shipped kits) -- what ``animate_chunk``
        and validation read.  (The reference's ``state_dict`` does not carry the tables: sings_hybrid.py:169-199.)"""
        if betas is None:
            raise ValueError("sings_amd.pose: save_kit_poses needs the kit's betas (they are passed through to the file)")
        go, bp, tr = self.axis_angle()
        betas = np.asarray(betas.detach().cpu().numpy() if torch.is_tensor(betas) else betas, np.float32)
        np.savez(path, betas=betas, global_orient=go, body_pose=bp, transl=tr)
