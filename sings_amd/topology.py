"""The mesh side of the reference's ``hybrid`` densification (``SinGS.densify_and_subdivide``, sings_hybrid.py:1022-1150): which faces
to split, the 1-to-4 split itself, the new vertices' attributes and the unique-edge list the regularisers read -- on the device
(csrc/sg_mesh.hip), without a host mesh library and without the mesh ever leaving the GPU.

    subdivide_decision     sings_hybrid.py:1026-1088   pure torch (runs on CPU tensors too, like ``train_loop.densify_decision``)
    subdivide_meshes       geometry_ops.py:8-76        drop-in: same arguments, same return triple
    unique_edges           the ``torch.unique(sorted edges, dim=0, return_inverse, return_counts)`` inside it, and the
                           ``trimesh.Trimesh(...).edges_unique`` of sings_hybrid.py:1106-1110 as a SET (below)
    MeshState              what a trainer carries between steps: faces, edges, vertex labels, level ids

and of its pruning (``SinGS.prune_and_simplify``, sings_hybrid.py:1153-1257):

    simplify_decision      sings_hybrid.py:1157-1222   pure torch: which vertices may go, which edges may collapse, or why not
    collapse_edges         geometry_ops.py:79-167      drop-in: same arguments, same return tuple; the whole sequential loop is one launch

Every output is a deterministic function of the inputs (no output depends on the order atomics land in): ranks of a frame-parallel
run that hold the same reduced statistics build the same mesh, bit for bit.

``edges`` are the unique sorted rows (a < b) of the faces' edges in lexicographic order.  That is what ``trimesh.edges_unique`` holds
as a set when no two vertices coincide; trimesh's own row order and its merging of coincident vertices (``process=True``) are not
reproduced.
"""
import torch

from . import _marshal

AVERAGED_NOT = ("vertex_id", "vertex_label")     # geometry_ops.py:66-69: these take the smaller endpoint's value


def _faces_i32(faces, num_verts):
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise RuntimeError("sings_amd.topology: faces must be a GPU tensor (no CPU fallback)")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"sings_amd.topology: faces must be an [F,3] int32 / int64 tensor, got {tuple(faces.shape)} {faces.dtype}")
    if int(num_verts) < 0 or int(num_verts) > 2 ** 30:
        raise ValueError(f"sings_amd.topology: {num_verts} vertices (0 .. 2^30)")
    if faces.dtype == torch.int64 and faces.numel():
        # (an int64 index that does not fit 32 bits must not alias a valid one in the conversion)
        faces = faces.clamp(-1, int(num_verts))
    return faces.to(torch.int32).contiguous()


def _face_flags(face_mask, F, dev):
    if face_mask is None:
        return None
    if not torch.is_tensor(face_mask) or not face_mask.is_cuda:
        raise RuntimeError("sings_amd.topology: face_mask must be a GPU tensor (no CPU fallback)")
    if tuple(face_mask.shape) != (F,) or face_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"sings_amd.topology: face_mask must be a [{F}] bool / uint8 tensor")
    return face_mask.to(device=dev, dtype=torch.uint8).contiguous()


def unique_edges(faces, num_verts, face_mask=None):
    """-> (edges [E,2], counts [E], face_edges [F,3]), int32 on the device.  ``edges``: the unique undirected edges (a < b) of the
    faces ``face_mask`` selects (None: all) in ascending lexicographic order -- the rows of ``torch.unique(sorted_edges, dim=0)``;
    ``counts``: how many selected faces hold each; ``face_edges``: per selected face the positions of its edges (v0v1, v1v2, v2v0) in
    ``edges`` (-1 for the others).  One host read (E).  Faces that index at or past ``num_verts`` raise IndexError."""
    f32 = _faces_i32(faces, num_verts)
    edges, counts, face_edges, _ = _marshal.mesh_unique_edges(f32, num_verts, _face_flags(face_mask, f32.shape[0], f32.device))
    return edges, counts, face_edges


def _midpoint_rows(edges, values, average):
    """[E, ...] rows for the new vertices of ``edges``: the endpoints' mean (fp32) or the smaller endpoint's value, in ``values``'
    dtype and trailing shape."""
    if not torch.is_tensor(values) or not values.is_cuda:
        raise RuntimeError("sings_amd.topology: vertex attributes must be GPU tensors (no CPU fallback)")
    v = values.detach()
    flat = v.reshape(v.shape[0], -1)
    if average:
        if v.dtype != torch.float32:
            raise ValueError(f"sings_amd.topology: an averaged attribute must be float32 (got {v.dtype})")
        out = _marshal.mesh_midpoints(edges, flat.contiguous())
    elif v.dtype == torch.float32:
        # a float label: its bits are copied (the int32 kernel moves 32-bit words, whatever they mean)
        out = _marshal.mesh_midpoints(edges, flat.contiguous().view(torch.int32)).view(torch.float32)
    else:
        if v.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.bool):
            raise ValueError(f"sings_amd.topology: a label attribute must be an integer or float32 tensor (got {v.dtype})")
        if v.dtype == torch.int64 and flat.numel() and int(flat.abs().max()) >= 2 ** 31:
            raise ValueError("sings_amd.topology: int64 labels beyond 32 bits")
        out = _marshal.mesh_midpoints(edges, flat.to(torch.int32).contiguous()).to(v.dtype)
    return out.reshape((out.shape[0],) + tuple(v.shape[1:]))


def subdivide_meshes(vertices, faces, face_index=None, vertex_attributes=None):
    """Drop-in for ``geometry_ops.subdivide_meshes``: the faces ``face_index`` names (None: all; duplicates are harmless) are split
    1-to-4 at their edge midpoints, the others are kept, in front.  -> (new_vertices [V+E,3], new_faces [F+3Fs,3] int64,
    new_attributes): ``'vertex_id'`` / ``'vertex_label'`` rows of the new vertices take the smaller endpoint's value, every other key
    the endpoints' mean.  Midpoint ``V + k`` belongs to row k of ``torch.unique(sorted_edges, dim=0)``, as in the reference.
    (``vertex_attributes=None`` returns ``None`` for the attributes; the reference raises UnboundLocalError there.)"""
    if not torch.is_tensor(vertices) or not vertices.is_cuda:
        raise RuntimeError("sings_amd.topology: vertices must be a GPU tensor (no CPU fallback)")
    if vertices.dim() != 2 or vertices.dtype != torch.float32:
        raise ValueError("sings_amd.topology: vertices must be [V,C] float32")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    f32 = _faces_i32(faces, V)
    dev = f32.device
    flags = None
    if face_index is not None:
        if not torch.is_tensor(face_index) or not face_index.is_cuda:
            raise RuntimeError("sings_amd.topology: face_index must be a GPU tensor (no CPU fallback)")
        flags = torch.zeros(F, dtype=torch.uint8, device=dev)
        if face_index.dtype == torch.bool:
            flags[face_index] = 1
        else:
            flags[face_index.to(torch.int64)] = 1                 # (an index outside [0, F) raises here, as in the reference)
    edges, _, face_edges, Fs = _marshal.mesh_unique_edges(f32, V, flags)
    new_faces = _marshal.mesh_subdivide(f32, V, flags, face_edges, Fs).to(torch.int64)
    new_vertices = torch.cat([vertices.detach(), _midpoint_rows(edges, vertices, True)])
    new_attributes = None
    if vertex_attributes is not None:
        new_attributes = {}
        for key, values in vertex_attributes.items():
            if values.shape[0] != V:
                raise ValueError(f"sings_amd.topology: attribute {key!r} has {values.shape[0]} rows, the mesh {V} vertices")
            new_attributes[key] = torch.cat([values.detach(), _midpoint_rows(edges, values, key not in AVERAGED_NOT)])
    return new_vertices, new_faces, new_attributes


def collapse_edges(verts, verts_attr, selected_edges, faces, collapse_rate=0.5, return_collapses=False):
    """Drop-in for ``geometry_ops.collapse_edges``: ``int(n * collapse_rate)`` times (n: the distinct vertices of ``selected_edges``) the
    longest live selected edge is collapsed into its smaller endpoint, which keeps its position and attributes; edges are relabelled,
    self-edges dropped, duplicates merged; the loop ends early when no edge is left.  Faces are mapped, degenerate ones and all but the
    first of those on the same three vertices dropped, unreferenced vertices (isolated ones included) pruned, faces renumbered.
    -> (new_verts [V',3], new_faces [F',3] int64, new_verts_attr [V',...], prune_mask [V] bool); with ``return_collapses`` the number
    of collapses done is appended.  ``new_verts`` / ``new_verts_attr`` are the survivors' input rows, bit for bit.

    GPU tensors only; ``verts`` [V,3] float32 and finite (ValueError otherwise); ``selected_edges`` rows ``0 <= a < b < V`` (ValueError),
    at most ``collapse_max_edges()`` of them (ValueError; 10 240 -- the reference's caller skips above 10 000); duplicate rows are
    harmless, the row order does not matter.  One host read (F', V', collapses, the refusal flags), after which the refusals are
    raised.  When no face survives: RuntimeError (the reference fails in ``vstack`` there).  ``smooth`` is not offered: the reference's
    branch is a ``pass``.  The inputs are not written (the reference overwrites the deleted rows of ``verts`` / ``verts_attr`` in
    place).

    Deviations from the reference: (1) the surviving face rows are in their ORIGINAL order, the first occurrence of a vertex set
    kept -- the reference's order is that of ``trimesh.grouping.unique_rows``' hash; (2) the longest edge is the one with the larger
    squared length ``(dx*dx + dy*dy) + dz*dz`` (fp32), then the smaller ``a``, then the smaller ``b`` -- the reference's CPU ``argmax`` of
    ``linalg.norm`` over a lexicographic list names the same edge on an exact tie; (3) among edges whose lengths agree to within fp32
    rounding the order is this kernel's, not torch's; (4) trimesh's merging of coincident vertices is not reproduced (``unique_edges``
    says the same)."""
    for name, t in (("verts", verts), ("verts_attr", verts_attr), ("selected_edges", selected_edges), ("faces", faces)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"sings_amd.topology: {name} must be a GPU tensor (no CPU fallback)")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("sings_amd.topology: verts must be [V,3] float32")
    V = int(verts.shape[0])
    if verts_attr.shape[0] != V:
        raise ValueError(f"sings_amd.topology: verts_attr has {verts_attr.shape[0]} rows, the mesh {V} vertices")
    if selected_edges.dim() != 2 or selected_edges.shape[1] != 2 or selected_edges.dtype not in (torch.int32, torch.int64):
        raise ValueError("sings_amd.topology: selected_edges must be an [Es,2] int32 / int64 tensor")
    if int(selected_edges.shape[0]) > collapse_max_edges():
        raise ValueError(f"sings_amd.topology: {int(selected_edges.shape[0])} selected edges, one call takes at most {collapse_max_edges()}")
    f32 = _faces_i32(faces, V)
    sel = selected_edges
    if sel.dtype == torch.int64 and sel.numel():
        sel = sel.clamp(-1, V)                                       # (as _faces_i32: no aliasing in the conversion)
    sel = sel.to(torch.int32).contiguous()
    new_faces, prune_mask, survivors, done = _marshal.mesh_collapse(verts.detach().contiguous(), sel, f32, collapse_rate)
    if new_faces.shape[0] == 0:
        raise RuntimeError("sings_amd.topology: collapse_edges left no face")
    rows = survivors.to(torch.int64)
    out = (verts.detach()[rows], new_faces.to(torch.int64), verts_attr.detach()[rows], prune_mask.to(torch.bool))
    return out + (done,) if return_collapses else out


def collapse_max_edges():
    """The most selected edges ``collapse_edges`` takes (``sg_mesh_collapse_max_edges``: they stay resident in LDS)."""
    return _marshal.mesh_collapse_max_edges()


def simplify_decision(xyz_gradient_accum, denom, opacity, scales, vertex_label, faces, opacity_threshold, scale_threshold,
                      dead_grad=0.0005, large_scale=0.01, prune_max_n_gs_once=5000, min_n_gs=None, exclude=(6, 7)):
    """-> (vert_mask [N] bool, selected_edges [Es,2] int64, skip_reason or None) -- sings_hybrid.py:1157-1222 as a PURE function of its
    arguments (CPU or GPU tensors): every rank that holds the same reduced statistics takes the same decision.

        skip     ``N <= min_n_gs``                                                          -> ``"min_n_gs"`` (mask all false, no edges)
        points   ``opacity < opacity_threshold`` AND ``scales[:, :1] < scale_threshold`` (transparent and small); OR
                 ``scales[:, :1] > large_scale`` AND ``accum / denom < dead_grad`` (big and dead); never a label in ``exclude``
        faces    ALL corners selected
        edges    the unique sorted edges of those faces that exactly two of THOSE faces share (``counts == 2``: the boundary of the
                 selected region is excluded), in lexicographic order
        skip     no edge (the reference tests "no point" first: the same outcome)            -> ``"no_edges"``
                 more than ``2 * prune_max_n_gs_once`` edges                                 -> ``"too_many_edges"``

    ``scales``: as in the reference's ``human_gs_out`` the decoded scale times ``smpl_scale`` when the step has one (its ``'scales'`` and
    ``'scales_canon'`` are one tensor).  The reference's quirks: (1) NaN is NOT zeroed here (it is in ``subdivide_decision``): a NaN
    gradient (0 / 0: never visible) compares false and is not "dead" -- kept; (2) its ``exclude`` argument is overwritten with
    ``[6, 7]`` -- here (6, 7) is the default and another tuple (or None) is honoured; (3) ``min_n_gs=None``, its default, raises
    TypeError there -- here it means no floor; (4) its ``max_n_gs_once`` is never read -- there is no such argument; (5) the
    configuration's ``prune_collapse_rate`` never reaches its ``collapse_edges`` call, which always runs at 0.5."""
    N = int(xyz_gradient_accum.shape[0])
    dev = xyz_gradient_accum.device
    none = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    if min_n_gs is not None and N <= min_n_gs:
        return torch.zeros(N, dtype=torch.bool, device=dev), none, "min_n_gs"
    s = scales[:, :1]
    vert_mask = (opacity.reshape(N, 1) < opacity_threshold) & (s < scale_threshold)
    grads = xyz_gradient_accum.reshape(N, 1) / denom.reshape(N, 1)
    vert_mask = vert_mask | ((s > large_scale) & (grads < dead_grad))
    vert_mask = vert_mask.reshape(-1)
    if exclude is not None and len(exclude):
        lab = vertex_label.reshape(-1)
        vert_mask = vert_mask & ~torch.isin(lab, torch.as_tensor(list(exclude), dtype=lab.dtype, device=lab.device))
    faces = faces.to(torch.int64)
    face_mask = vert_mask[faces].all(dim=1)
    e = torch.sort(faces[face_mask][:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    unique, counts = torch.unique(e, dim=0, return_counts=True)
    selected_edges = unique[counts == 2].reshape(-1, 2)
    if selected_edges.shape[0] == 0:
        return vert_mask, selected_edges, "no_edges"
    if selected_edges.shape[0] > 2 * prune_max_n_gs_once:
        return vert_mask, selected_edges, "too_many_edges"
    return vert_mask, selected_edges, None


def subdivide_decision(xyz_gradient_accum, denom, scales_canon, max_radii2D, vertex_label, faces, grad_threshold, scale_threshold,
                       max_screen_size=None, max_n_gs=None, exclude=(6, 7)):
    """-> (selected_pts_mask [N] bool, selected_faces_idx int64) -- sings_hybrid.py:1026-1088 as a PURE function of its arguments
    (CPU or GPU tensors): every rank that holds the same reduced statistics takes the same decision.

        grads    accum / denom, NaN -> 0
        scales   ``scales_canon[:, :1]`` -- as in the reference's ``human_gs_out``: the decoded scale times ``smpl_scale`` when the step
                 has one
        points   ``|grad| > grad_threshold`` AND ``scale > scale_threshold``; OR ``max_radii2D > max_screen_size`` when that is given
                 (and truthy: the reference tests ``if max_screen_size:``); never a point whose label is in ``exclude``
        faces    ANY corner selected
        cap      when the unique edges of the selected faces number at least ``max_n_gs - N``: only the ``(max_n_gs - N) // 3`` faces with
                 the largest summed corner scale, in that order (``argsort(descending=True)``: ties are the sort's to break)

    The reference's quirks, kept: (1) its ``exclude`` argument is overwritten with ``[6, 7]`` (the hands) whatever the caller passes --
    here (6, 7) is the default and another tuple (or None: nobody excluded) is honoured; (2) when ``max_n_gs - N <= 0`` it only PRINTS
    that it skips and subdivides every selected face anyway -- so does this; (3) the screen-size term bypasses the scale AND the
    gradient condition; (4) ``max_n_gs=None`` fails there (None - int): here it means no cap."""
    N = int(xyz_gradient_accum.shape[0])
    grads = xyz_gradient_accum / denom
    grads = torch.where(torch.isnan(grads), torch.zeros_like(grads), grads)
    scales = scales_canon[:, :1]
    selected = (torch.norm(grads, dim=-1) > grad_threshold) & (torch.max(scales, dim=1).values > scale_threshold)
    if max_screen_size:
        selected = selected | (max_radii2D > max_screen_size)
    if exclude is not None and len(exclude):
        lab = vertex_label.reshape(-1)
        selected = selected & ~torch.isin(lab, torch.as_tensor(list(exclude), dtype=lab.dtype, device=lab.device))
    faces = faces.to(torch.int64)
    face_idx = selected[faces].any(dim=1).nonzero(as_tuple=False).view(-1)
    if max_n_gs is not None:
        num_left = int(max_n_gs) - N
        if num_left > 0:
            e = torch.sort(faces[face_idx][:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
            num_to_add = int(torch.unique(e, dim=0).shape[0])
            if num_to_add >= num_left:
                face_scores = scales[faces[face_idx]].sum(dim=[1, 2])
                face_idx = face_idx[torch.argsort(face_scores, descending=True)[:num_left // 3]]
        # else: "close to the maximum, just skip densification" is only a message in the reference: every selected face is split
    return selected, face_idx


def rescaled_multiplier(scaling_multiplier, scales_canon, selected_pts_mask):
    """The old rows' ``scaling_multiplier`` after a subdivision (sings_hybrid.py:1034-1036, 1127): a selected row is multiplied by
    ``mean_scale / scale`` with ``scale = scales_canon[:, :1]`` and the mean over ALL points; the others are kept.  ``scaling_multiplier``:
    [N,1], or a scalar / None (ones) that becomes per-Gaussian here.  Pure torch."""
    scales = scales_canon[:, :1]
    N = int(scales.shape[0])
    if scaling_multiplier is None:
        sm = torch.ones((N, 1), dtype=scales.dtype, device=scales.device)
    else:
        sm = torch.as_tensor(scaling_multiplier, dtype=scales.dtype, device=scales.device).detach()
        sm = sm.reshape(-1, 1).expand(N, 1).clone() if sm.numel() == 1 else sm.reshape(N, 1).clone()
    ratio = (scales.mean() / scales.mean(-1)).detach()
    sm[selected_pts_mask] *= ratio[selected_pts_mask].unsqueeze(1)
    return sm


class MeshState:
    """The mesh a trainer carries between densifications: ``faces`` [F,3] int32, ``edges`` [E,2] int32 (the unique edges of ALL faces,
    lexicographic), ``vertex_label`` [N] int32, ``level_id`` [N] fp32 and ``gs_level_mark`` (sings_hybrid.py:133-136, 728).  It owns
    these entries of ``export.checkpoint_keys()``: ``vertex_label``, ``level_id``, ``gs_level_mark``."""

    CHECKPOINT_KEYS = ("vertex_label", "level_id", "gs_level_mark")

    def __init__(self, faces, edges, vertex_label, level_id, gs_level_mark):
        self.faces, self.edges, self.vertex_label, self.level_id = faces, edges, vertex_label, level_id
        self.gs_level_mark = list(gs_level_mark)

    @classmethod
    def from_faces(cls, faces, vertex_label, level_id=None):
        """``faces`` [F,3] and ``vertex_label`` [N] on the GPU; level ids start at 0 (``_level_id = zeros(n_gs)``)."""
        if not torch.is_tensor(vertex_label) or not vertex_label.is_cuda:
            raise RuntimeError("MeshState: vertex_label must be a GPU tensor (no CPU fallback)")
        N = int(vertex_label.shape[0])
        f32 = _faces_i32(faces, N)
        edges, _, _ = unique_edges(f32, N)
        if level_id is None:
            level_id = torch.zeros(N, dtype=torch.float32, device=f32.device)
        return cls(f32, edges, vertex_label.reshape(-1).to(torch.int32), level_id, [0, N])

    @property
    def num_verts(self):
        return int(self.vertex_label.shape[0])

    def replace(self, faces, vertex_label):
        """The mesh after a subdivision: new faces and labels, the unique edges of the new faces (same kernel), the new vertices at
        the last vertex' level (sings_hybrid.py:1116-1124)."""
        n_old, N = self.num_verts, int(vertex_label.shape[0])
        self.faces = _faces_i32(faces, N)
        self.edges, _, _ = unique_edges(self.faces, N)
        self.vertex_label = vertex_label.reshape(-1).to(torch.int32)
        if N > n_old:
            self.level_id = torch.cat([self.level_id, self.level_id[-1:].expand(N - n_old)])
        self.gs_level_mark[-1] = N

    def prune(self, new_faces, keep_mask, edges=None):
        """The mesh after a simplification (sings_hybrid.py:1243-1252): ``new_faces`` index the kept vertices; the unique edges of the
        new faces (same kernel; ``edges``: given instead -- a caller that holds them, or a host without the library); the kept
        vertices' labels.  ``level_id`` is TRUNCATED to the new count, not masked -- the reference's ``_level_id[:n_gs]``: with more
        than one level a pruned vertex of an early level shifts the later levels' ids; kept as it is there."""
        keep = keep_mask.reshape(-1).to(torch.bool)
        if keep.shape[0] != self.num_verts:
            raise ValueError(f"MeshState.prune: keep_mask has {keep.shape[0]} entries, the mesh {self.num_verts} vertices")
        self.vertex_label = self.vertex_label[keep]
        N = int(self.vertex_label.shape[0])
        if edges is None:
            self.faces = _faces_i32(new_faces, N)
            edges, _, _ = unique_edges(self.faces, N)
        else:
            self.faces = new_faces.to(torch.int32).contiguous()
        self.edges = edges
        self.level_id = self.level_id[:N]
        self.gs_level_mark[-1] = N

    def checkpoint_entries(self):
        return {"vertex_label": self.vertex_label, "level_id": self.level_id, "gs_level_mark": list(self.gs_level_mark)}

    def state_dict(self):
        """The three ``CHECKPOINT_KEYS`` plus ``faces`` and ``edges`` (which the reference does not save: a reloaded model of its own has
        lost its mesh after the first density event)."""
        return dict(self.checkpoint_entries(), faces=self.faces, edges=self.edges)

    def load_state_dict(self, sd, device=None):
        """The five arrays as saved (the edges are NOT recomputed: they are the saved mesh's, bit for bit), on ``device`` (None: where
        the current arrays live).  The caller has checked the indices against the vertex count (``checkpoint.validate_model``)."""
        dev = self.vertex_label.device if device is None else device
        n = int(sd["vertex_label"].shape[0])
        level = sd.get("level_id")
        self.faces = sd["faces"].to(dev, torch.int32).contiguous()
        self.edges = sd["edges"].to(dev, torch.int32).contiguous()
        self.vertex_label = sd["vertex_label"].to(dev, torch.int32).reshape(-1).contiguous()
        self.level_id = torch.zeros(n, dtype=torch.float32, device=dev) if level is None else level.to(dev).contiguous()
        mark = sd.get("gs_level_mark")
        self.gs_level_mark = [0, n] if mark is None else [int(x) for x in mark]
