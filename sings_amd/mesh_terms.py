"""The four mesh terms every shipped configuration adds to the photometric loss, L2Norm and the k-NN edge loss (gs_trainer.py:366-399
with loss_items.py:93-192), for ``AvatarStep`` / ``AvatarTrainer``:

    region_mesh_lap         alpha(t) * RegionLaplacianLoss_v2(position_regions_w)(xyz_anchor_canon)       gs_trainer.py:372, 382
    region_mesh_lap_color   color_strength * RegionLaplacianLoss_v2(color_regions_w)(shs[:, 0])           :373, 383
    hand_lap                1e-5 * region_mesh_lap_pos.forward_hands(xyz_canon)                           :394-396
    mesh_edge_loss          loss.mesh_edge * pytorch3d.loss.mesh_edge_loss(human_gs._mesh)                :366

with ``xyz_anchor_canon = xyz_canon + mean(scales, -1) * n / 2`` (sings_hybrid.py:437-443; ``n``: the constant vertex normals of the
current mesh).  New rows inherit the last level id (sings_hybrid.py:1116-1119), so the reference's ``[:num_level_0]`` slices are the whole
arrays.  Only the ``standard`` Laplacian, which is what the trainer constructs (gs_trainer.py:176-192).

The three Laplacians are ONE forward and ONE backward launch over one CSR (csrc/sg_mesh_terms.hip, include/sings_mesh_terms.h): the anchor of a
neighbour is formed where it is read, the step weights are read from device memory, and the CSR of the same-label edges -- with the
degrees, the label counts and the per-vertex scales -- is built on the device from ``MeshState.edges`` without a host copy of the mesh.

Three things the reference does, and what becomes of them here:

    mesh_edge_loss is a constant per topology.  ``human_gs._mesh`` holds tensors that are not the optimised parameter (sings_hybrid.py:708,
        :1113, :1245; the latter two under no_grad): no gradient of the term reaches an optimised parameter.  It is computed once per
        ``reset`` with ``regularizers.mesh_edge_loss``, kept as a device scalar, reported, added to the loss, and has no gradient.
    The ``alpha *= 2`` after iteration 8000 (gs_trainer.py:386-387) runs after the terms are formed and changes nothing: not reproduced.
    ``impose_from_iter`` must be positive: the reference divides by it.  ValueError at construction otherwise.

No CPU fallback: the HIP library must be present.
"""
import numpy as np
import torch

from . import _lib
from ._marshal import _ptr, _stream
from .regularizers import _MeshEdges, mesh_edge_loss

HAND_LABELS, HAND_STRENGTH, HAND_WEIGHT = (6, 7), 1000.0, 1e-5     # loss_items.py:172-180, gs_trainer.py:396
_SLOTS = 8                                                         # pinned rows the weights are copied from, used in turn


def lap_weights(t_iter, position_strength, color_strength, impose_from_iter):
    """-> (alpha, beta, 1e-5): the step weights of the position, colour and hand term at iteration ``t_iter`` (gs_trainer.py:376-383,
    396), the reference's arithmetic in double."""
    lap_start = impose_from_iter
    if lap_start <= 0:
        raise ValueError(f"lap_weights: impose_from_iter must be positive (the reference divides by it), got {impose_from_iter}")
    alpha = 0.
    if t_iter > lap_start:
        alpha = position_strength * min(1, (t_iter - lap_start) / float(lap_start))
    return float(alpha), float(color_strength), HAND_WEIGHT


def _table(weights, n):
    """Per-label weights as fp32 [n]: a sequence indexed by label or a dict label -> weight; labels it does not name weigh 1 (as
    ``RegionLaplacianLoss_v2`` without ``region_weights``)."""
    w = np.ones(n, np.float32)
    if isinstance(weights, dict):
        for k, v in weights.items():
            w[int(k)] = v
    elif weights is not None:
        a = np.asarray(weights, dtype=np.float32).reshape(-1)
        w[:len(a)] = a
    return w


def _n_labels(weights):
    if isinstance(weights, dict):
        return max((int(k) for k in weights), default=-1) + 1
    return 0 if weights is None else int(np.asarray(weights).reshape(-1).shape[0])


class _TermsGrad(torch.autograd.Function):
    """The three weighted terms as ONE node whose gradients the kernel computed with the values (unit upstream): backward scales them.
    Position and hand term share ``d_xyz_canon`` and reach the loss through the same sum, so both take the position term's upstream."""

    @staticmethod
    def forward(ctx, terms, xyz, scales, colour, d_xyz, d_scales, d_colour):
        ctx.save_for_backward(d_xyz, d_scales, d_colour)
        return terms[0], terms[1], terms[2]              # (views of the kernel's own output buffer: no copy kernel)

    @staticmethod
    def backward(ctx, g_pos, g_col, g_hand):
        d_xyz, d_scales, d_colour = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gs = torch._foreach_mul([d_xyz, d_scales], g_pos.reshape(()))
        return (None, gx if need[1] else None, gs if need[2] else None, d_colour * g_col.reshape(()) if need[3] else None, None, None,
                None)


class MeshTerms:
    """``MeshTerms(region_weights_pos, region_weights_color, mesh_edge_w, position_strength, color_strength, impose_from_iter)``

    ``region_weights_*``: per-label weights (``parse_weights`` of ``loss.laplacian.position_regions_w`` / ``color_regions_w``): a sequence
    indexed by label, or a dict.  ``hands=False`` drops the hand term (the reference's ``force_hand`` is always on).

        reset(mesh, normals, verts)   a new topology: the device build from ``mesh.edges`` / ``mesh.vertex_label`` (``MeshState``), the
                                      constant edge term from ``verts`` [V,3], every buffer sized.  ONE host read (8 bytes: the error
                                      flags, with the number of CSR entries); a label outside the weight tables or an edge row that is not
                                      0 <= a < b < V is a ValueError.
        set_weights((a, b, h))        the three step weights into device memory as given; ``set_iteration`` is this with ``weights_at(t)``
        set_iteration(t)              the step weights of iteration t into device memory -- from pinned memory, non-blocking, and only when
                                      a value changed (after the ramp: nothing is copied).  A graph captured at one iteration replays with
                                      the weights of the moment.
        __call__(attrs)               ``attrs``: ``xyz_canon`` [V,3], ``scales`` [V,3], ``shs`` [V,K,3] (or the DC rows [V,3]) -> a dict
                                      with ``region_mesh_lap``, ``region_mesh_lap_color``, ``hand_lap``, ``mesh_edge_loss``: weighted 0-dim
                                      device tensors, autograd attached.  Three launches, no allocation: the values are views of buffers
                                      this module owns, overwritten by the next call.
        last_grads                    what the kernel computed besides the values, for an upstream gradient of 1: ``xyz_canon`` [V,3]
                                      (position + hand), ``scales`` [V,3], ``shs_dc`` [V,3] (the gradient of ``shs[:, 0]``).

    An input whose row count is not the built V raises ValueError (a holder of the set before a densify / prune)."""

    KEYS = ("region_mesh_lap", "region_mesh_lap_color", "hand_lap", "mesh_edge_loss")

    def __init__(self, region_weights_pos, region_weights_color, mesh_edge_w, position_strength, color_strength, impose_from_iter,
                 hands=True):
        if impose_from_iter <= 0:
            raise ValueError(f"MeshTerms: impose_from_iter must be positive (the reference divides by it), got {impose_from_iter}")
        self.position_strength, self.color_strength = float(position_strength), float(color_strength)
        self.impose_from_iter, self.mesh_edge_w, self.hands = impose_from_iter, float(mesh_edge_w), bool(hands)
        self.L = max(_n_labels(region_weights_pos), _n_labels(region_weights_color), max(HAND_LABELS) + 1 if hands else 1)
        self._tables = [_table(region_weights_pos, self.L), _table(region_weights_color, self.L), np.zeros(self.L, np.float32)]
        if hands:
            self._tables[2][list(HAND_LABELS)] = HAND_STRENGTH
        self.V = self.E = self.nnz = 0
        self.dev = self.term_w = None
        self.last_grads = None
        self._w = None                                   # the weights term_w holds (or will hold after the first reset)
        self.set_iteration(0)

    # ---- step weights
    def weights_at(self, t_iter):
        a, b, h = lap_weights(t_iter, self.position_strength, self.color_strength, self.impose_from_iter)
        return (a, b, h if self.hands else 0.0)

    def set_iteration(self, t_iter):
        self.set_weights(self.weights_at(t_iter))

    def set_weights(self, w):
        """The three step weights as given (``set_iteration`` computes them from the iteration)."""
        w = tuple(float(x) for x in w)
        if len(w) != 3:
            raise ValueError("MeshTerms.set_weights: three weights (position, colour, hand)")
        if w == self._w:
            return
        self._w = w
        if self.term_w is not None:
            self._upload()

    def _upload(self):
        """pinned row -> term_w on the current stream.  The rows are used in turn, each behind the event of its last copy: a row is not
        rewritten while a copy that the device has not executed yet still reads it."""
        k = self._slot = (self._slot + 1) % _SLOTS
        self._events[k].synchronize()
        self._pinned[k].copy_(torch.tensor(self._w, dtype=torch.float32))
        self.term_w.copy_(self._pinned[k], non_blocking=True)
        self._events[k].record(torch.cuda.current_stream(self.dev))

    # ---- a new topology
    def reset(self, mesh, normals, verts):
        lib = _lib.load()
        for name, t in (("mesh.edges", mesh.edges), ("mesh.vertex_label", mesh.vertex_label), ("normals", normals), ("verts", verts)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"sings_amd.mesh_terms: {name} must be a GPU tensor (no CPU fallback)")
        dev = verts.device
        V = int(mesh.vertex_label.shape[0])
        edges = mesh.edges.to(torch.int32).reshape(-1, 2).contiguous()
        label = mesh.vertex_label.reshape(-1).to(torch.int32).contiguous()
        E = int(edges.shape[0])
        for name, t in (("normals", normals), ("verts", verts)):
            if tuple(t.shape) != (V, 3):
                raise ValueError(f"MeshTerms.reset: {name} must be [{V},3] (the mesh's vertices), got {tuple(t.shape)}")
        if V < 1 or V > 2 ** 30 or E >= 2 ** 30:
            raise ValueError(f"MeshTerms.reset: {V} vertices / {E} edges (1 .. 2^30 vertices, fewer than 2^30 edges)")
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if self.dev != dev:
                self.dev = dev
                self.term_w = f32(3)
                self._pinned = torch.zeros((_SLOTS, 3), dtype=torch.float32).pin_memory()
                self._events, self._slot = [torch.cuda.Event() for _ in range(_SLOTS)], -1
                self._w_dev = [torch.from_numpy(w).to(dev) for w in self._tables]
                self._upload()
            self.row_ptr, self.col, self.deg_inv = i32(V + 1), i32(max(2 * E, 1)), f32(V)
            self.count, self.vscale = i32(self.L), f32(V, 3)
            deg_ws, info = i32(V), i32(2 * _lib.MESH_TERMS_INFO_INTS)
            wp, wc, wh = self._w_dev
            _lib.check(lib.sg_mesh_terms_build(V, E, self.L, _ptr(edges), _ptr(label), _ptr(wp), _ptr(wc), _ptr(wh), _ptr(self.row_ptr),
                                               _ptr(self.col), _ptr(self.deg_inv), _ptr(self.count), _ptr(self.vscale), _ptr(deg_ws),
                                               _ptr(info[:2]), _stream(dev)), "mesh terms (build)")
            # the whole mesh's CSR for the constant edge term: the same build without labels
            whole = _MeshEdges.__new__(_MeshEdges)
            whole.V, whole.E, whole.row_ptr, whole.col = V, E, i32(V + 1), i32(max(2 * E, 1))
            _lib.check(lib.sg_mesh_terms_build(V, E, 1, _ptr(edges), None, None, None, None, _ptr(whole.row_ptr), _ptr(whole.col),
                                               _ptr(f32(V)), None, None, _ptr(deg_ws), _ptr(info[2:]), _stream(dev)),
                       "mesh terms (edge CSR)")
            flags, nnz, flags_whole, _ = info.tolist()               # the one host read
            if (flags | flags_whole) & _lib.MESH_TERMS_BAD_EDGE:
                raise ValueError(f"MeshTerms.reset: an edge row is not 0 <= a < b < {V}")
            if flags & _lib.MESH_TERMS_BAD_LABEL:
                raise ValueError(f"MeshTerms.reset: a vertex label outside [0, {self.L}) (the weight tables' labels)")
            with torch.no_grad():
                x = verts.detach().float().contiguous().clone()
                edge = mesh_edge_loss(x, whole) if E > 0 else torch.zeros((), dtype=torch.float32, device=dev)
                self.mesh_edge = (self.mesh_edge_w * edge).reshape(()).detach()
            self.verts = x                                           # (what the constant edge term was computed from)
            self.normals = normals.detach().contiguous().float().clone()
            self.ws = torch.empty(int(lib.sg_reg_ws_bytes(V)), dtype=torch.uint8, device=dev)
            self.g, self.terms = f32(3, V, 3), torch.zeros(3, dtype=torch.float32, device=dev)
            self.last_grads = {"xyz_canon": f32(V, 3), "scales": f32(V, 3), "shs_dc": f32(V, 3)}
        self.V, self.E, self.nnz = V, E, int(nnz)

    # ---- checkpoint
    def state_dict(self):
        """What the last ``reset`` was given besides the mesh: ``verts`` and ``normals`` [V,3].  Everything else the terms hold -- both
        CSRs, the degrees, the constant edge term -- is rebuilt from them and the mesh, and ``reset`` is deterministic; the step
        weights follow ``set_iteration``."""
        if self.V == 0:
            raise RuntimeError("MeshTerms.state_dict: call reset(mesh, normals, verts) first")
        return {"verts": self.verts, "normals": self.normals}

    def load_state_dict(self, sd, mesh):
        """``reset`` for ``mesh`` (the saved run's ``MeshState``) with the saved vertices and normals."""
        dev = mesh.vertex_label.device
        self.reset(mesh, sd["normals"].to(dev), sd["verts"].to(dev))

    # ---- the terms
    def __call__(self, attrs):
        if self.V == 0:
            raise RuntimeError("MeshTerms: call reset(mesh, normals, verts) first")
        xyz, scales, shs = attrs["xyz_canon"], attrs["scales"], attrs["shs"]
        colour = shs[:, 0] if shs.dim() == 3 else shs
        for name, t in (("xyz_canon", xyz), ("scales", scales), ("shs", colour)):
            if not t.is_cuda:
                raise RuntimeError(f"sings_amd.mesh_terms: {name} must live on the GPU (no CPU fallback)")
            if t.shape[0] != self.V:
                raise ValueError(f"MeshTerms: {name} has {t.shape[0]} rows, the terms were built for {self.V} vertices (reset() after "
                                 "a densify / prune)")
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or t.stride(1) != 1:
                raise ValueError(f"MeshTerms: {name} must be fp32 rows of 3 contiguous floats, got {t.dtype} {tuple(t.shape)}")
        if not (xyz.is_contiguous() and scales.is_contiguous()):
            raise ValueError("MeshTerms: xyz_canon and scales must be contiguous [V,3]")
        grads = self.last_grads if torch.is_grad_enabled() else {}
        dev = self.dev
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sg_mesh_terms(
                self.V, _ptr(xyz), _ptr(scales), _ptr(self.normals), _ptr(colour), int(colour.stride(0)), _ptr(self.row_ptr),
                _ptr(self.col), _ptr(self.deg_inv), _ptr(self.vscale), _ptr(self.term_w), _ptr(self.ws), _ptr(self.g), _ptr(self.terms),
                None, _ptr(grads.get("xyz_canon")), _ptr(grads.get("scales")), _ptr(grads.get("shs_dc")), _stream(dev)), "mesh terms")
        if grads and any(t.requires_grad for t in (xyz, scales, colour)):
            vals = _TermsGrad.apply(self.terms, xyz, scales, colour, grads["xyz_canon"], grads["scales"], grads["shs_dc"])
        else:
            vals = (self.terms[0], self.terms[1], self.terms[2])
        return dict(zip(self.KEYS, (*vals, self.mesh_edge)))
