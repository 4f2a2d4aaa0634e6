"""A body model from SMPL arrays: the template, its subdivision, the rest joints of a betas vector and the canonical-pose mesh -- what
the reference takes from its ``SMPL`` / ``SMPLH`` layer (smpl_layer.py, smplh_layer.py) with ``smplx`` and ``trimesh`` installed, and what
every other entry point here takes as given (``joints_rest``, ``A_t2cano``, the mesh of ``avatar_init.from_mesh``).

    load_body_arrays      an ``.npz`` with the SMPL-H key names -> the arrays ``BodyModel`` takes
    BodyModel             the arrays on the device, validated
      .subdivided(n)      smpl_layer.py:296-353: ``topology.subdivide_meshes`` per level, the regressor renormalised, the filter below
      .joint_basis()      the regressor folded through [v_template | shapedirs], once: joints_rest(betas) = J0 + JS . betas
      .joints_rest(betas) the rest joints of one or K betas vectors, differentiable w.r.t. betas
      .shaped(betas, pose)    blend shapes and pose correctives of K rows, one launch (body_model/lbs.py:129-165)
      .canonical(betas)   sings_hybrid.py:578-596 ``get_canonical_verts``
    smooth_filter         the mutable diffusion Laplacian filter with volume constraint, five iterations without a host read

Kernels: csrc/sg_body.hip (include/sings_body.h).  There is no CPU fallback: host tensors raise.  Beside each numeric piece stands its
numpy twin (``*_host``, fp64 unless told otherwise): the stated definition, and what the tests hold the kernels to.

What the reference wastes here: every ``forward`` of its layer computes blend shapes over all vertices, a [J,V] regressor product and a
full template skinning only to read ``A``.  The joints are affine in betas: once the regressor is folded through the
shape basis, the rest joints of any betas cost a [3J, B] product.

The filter is PARITY-UNPINNED, like the vertex normals of ``avatar_init``: the reference calls
``trimesh.smoothing.filter_mut_dif_laplacian(lamb=0.5, iterations=5, volume_constraint=True)``, trimesh is not a dependency and the
reference pins no version.  What is built is the definition in ``smooth_host``' docstring and no more is claimed; ``smooth`` may be a
callable ``verts -> verts`` for a user who wants the library's own.
"""
import numpy as np
import torch

from . import _lib, _marshal, topology
from ._marshal import _ptr, _stream
from .body import _parents_tensor, joint_transforms_hip, rodrigues
from .canonical import predefined_pose

MAX_JOINTS, MAX_BETAS, MAX_VERTS = _lib.BODY_MAX_JOINTS, _lib.BODY_MAX_BETAS, _lib.BODY_MAX_VERTS
NPZ_KEYS = ("v_template", "shapedirs", "J_regressor", "weights", "kintree_table", "f", "posedirs")


# ---- the numpy twins ------------------------------------------------------------------------------------------------------------------
def subdivide_host(verts, faces, attributes):
    """One level of geometry_ops.py:8-76 over all faces in numpy: midpoint V + k belongs to row k of the unique sorted edges; keys
    ``vertex_id`` / ``vertex_label`` take the smaller endpoint's value, every other key the endpoints' mean (in the array's dtype)."""
    verts, faces = np.asarray(verts), np.asarray(faces).astype(np.int64)
    V = verts.shape[0]
    e = np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    uniq, inv = np.unique(e, axis=0, return_inverse=True)
    mid = inv.reshape(-1, 3) + V
    new_faces = np.column_stack([faces[:, 0], mid[:, 0], mid[:, 2], mid[:, 0], faces[:, 1], mid[:, 1], mid[:, 2], mid[:, 1], faces[:, 2],
                                 mid[:, 0], mid[:, 1], mid[:, 2]]).reshape(-1, 3)
    mean = lambda a: (a[uniq[:, 0]] + a[uniq[:, 1]]) * a.dtype.type(0.5)
    out = {k: np.concatenate([a, a[uniq[:, 0]] if k in topology.AVERAGED_NOT else mean(a)]) for k, a in attributes.items()}
    return np.concatenate([verts, mean(verts)]), new_faces, out, uniq


def renorm_host(Jt, dtype=np.float64):
    """J_regressor [J,V] of the averaged J^T [V,J]: every row divided by its sum (smpl_layer.py:349-350)."""
    J = np.asarray(Jt).astype(dtype).T
    return J / J.sum(axis=1, keepdims=True)


def joint_basis_host(v_template, shapedirs, J_regressor, dtype=np.float64):
    """-> (J0 [J,3], JS [J,3,B]): the regressor applied to the template and to every shape direction."""
    Jr = np.asarray(J_regressor).astype(dtype)
    return Jr @ np.asarray(v_template).astype(dtype), np.einsum("jv,vcb->jcb", Jr, np.asarray(shapedirs).astype(dtype))


def joints_rest_host(J0, JS, betas):
    betas = np.asarray(betas, dtype=np.float64)
    return np.asarray(J0, np.float64) + np.einsum("jcb,...b->...jc", np.asarray(JS, np.float64), betas)


def rodrigues_host(pose, dtype=np.float64):
    """[J,3] axis-angle -> [J,3,3], angle = |theta + 1e-8| as the reference's ``batch_rodrigues``."""
    p = np.asarray(pose).astype(dtype).reshape(-1, 3)
    angle = np.linalg.norm(p + dtype(1e-8), axis=1, keepdims=True)
    d = p / angle
    K = np.zeros((p.shape[0], 3, 3), dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    return np.eye(3, dtype=dtype)[None] + np.sin(angle)[:, :, None] * K + (1 - np.cos(angle))[:, :, None] * (K @ K)


def joint_transforms_host(pose, joints_rest, parents):
    """``batch_rigid_transform`` of one pose in fp64 -> A [J,4,4] (relative to the rest joints)."""
    R, j = rodrigues_host(pose), np.asarray(joints_rest, np.float64)
    J = j.shape[0]
    G = np.zeros((J, 4, 4))
    for i in range(J):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R[i], j[i] - (j[parents[i]] if i else 0.0)
        G[i] = T if i == 0 else G[parents[i]] @ T
    A = G.copy()
    A[:, :3, 3] -= np.einsum("jab,jb->ja", G[:, :3, :3], j)
    return A


def shaped_host(v_template, shapedirs, betas, posedirs=None, pose=None, dtype=np.float64):
    """-> (v_shaped, shape_offsets, pose_offsets, v_posed) [K,V,3] of ``betas`` [K,B] and ``pose`` [K,J*3] (body_model/lbs.py:129-165
    with ``disable_posedirs=False``); without ``posedirs`` the pose offsets are zeros."""
    vt, sd = np.asarray(v_template).astype(dtype), np.asarray(shapedirs).astype(dtype)
    betas = np.asarray(betas).astype(dtype).reshape(-1, sd.shape[-1])
    so = np.einsum("kb,vcb->kvc", betas, sd)
    po = np.zeros_like(so)
    if posedirs is not None:
        pose = np.asarray(pose).astype(dtype).reshape(betas.shape[0], -1, 3)
        feat = np.stack([(rodrigues_host(p, dtype)[1:] - np.eye(3, dtype=dtype)).reshape(-1) for p in pose])
        po = (feat @ np.asarray(posedirs).astype(dtype)).reshape(so.shape)
    vs = vt[None] + so
    return vs, so, po, vs + po


def skin_host(A, lbs_weights, v_posed):
    """-> (verts [V,3], T [V,4,4]): T = W . A, verts = (T [v; 1])[:3] in fp64."""
    T = np.einsum("vj,jab->vab", np.asarray(lbs_weights, np.float64), np.asarray(A, np.float64))
    v = np.asarray(v_posed, np.float64)
    return np.einsum("vab,vb->va", T[:, :3, :3], v) + T[:, :3, 3], T


def smooth_host(verts, faces, edges, lamb=0.5, iterations=5, dtype=np.float64, trace=None):
    """The filter as built here, every operation in ``dtype``.  With ``x0`` the input vertices:

        L      the uniform umbrella: (L x)[v] is the mean of v's edge neighbours (``edges``: the unique rows a < b)
        n      the unit vector of the unweighted sum of the unit normals of v's faces, of x0, not updated
        eps    0.01 sqrt(max face area of x0)
        vol    vol(x) = sum_f x_a . (x_b x x_c) / 6,  vol0 = vol(x0)

    and per iteration i, x updated in place:  d = |n . (x - L x)|;  a = 1 / max(1e-12, d);  lambda_v = max(0.2 lamb, min(1, lamb a_v /
    mean(a)));  x += lambda (L x - x);  at i = 0 only: slope = eps / (vol(x + eps n) - vol(x));  x += n slope (vol0 - vol(x)).

    A vertex without a neighbour, a non-finite vertex, or a zero or non-finite vol(x + eps n) - vol(x) is a ValueError (the library
    would drag an isolated vertex to the origin).  ``trace``: a list that receives (lambda [V], vol before the correction, vol after it, vol0) per
    iteration."""
    T = np.dtype(dtype).type
    x = np.array(verts, dtype=dtype)
    faces, edges = np.asarray(faces).astype(np.int64), np.asarray(edges).astype(np.int64)
    V = x.shape[0]
    if not np.isfinite(x).all():
        raise ValueError("smooth_host: a vertex is not finite")
    src, dst = np.concatenate([edges[:, 0], edges[:, 1]]), np.concatenate([edges[:, 1], edges[:, 0]])
    deg = np.bincount(src, minlength=V)
    if (deg == 0).any():
        raise ValueError("smooth_host: a vertex has no neighbour")

    def umbrella(x):
        s = np.zeros_like(x)
        np.add.at(s, src, x[dst])
        return s / deg[:, None].astype(dtype)

    def vol(x):
        return (x[faces[:, 0]] * np.cross(x[faces[:, 1]], x[faces[:, 2]])).sum(axis=1).sum() / T(6)

    fn = np.cross(x[faces[:, 1]] - x[faces[:, 0]], x[faces[:, 2]] - x[faces[:, 0]])
    nn = np.sqrt((fn * fn).sum(axis=1))
    ok = (nn > 0) & np.isfinite(nn)
    unit = np.where(ok[:, None], fn / np.where(ok, nn, T(1))[:, None], T(0))
    n = np.zeros_like(x)
    for k in range(3):
        np.add.at(n, faces[:, k], unit)
    ln = np.sqrt((n * n).sum(axis=1))
    n = np.where(ln[:, None] > 0, n / np.where(ln > 0, ln, T(1))[:, None], T(0))
    eps = T(0.01) * np.sqrt(np.where(ok, T(0.5) * nn, T(0)).max())
    vol0, lamb, slope = vol(x), T(lamb), T(0)
    for i in range(int(iterations)):
        Lx = umbrella(x)
        d = np.abs((n * (x - Lx)).sum(axis=1))
        a = T(1) / np.maximum(T(1e-12), d)
        lam = np.maximum(T(0.2) * lamb, np.minimum(T(1), lamb * a / a.mean(dtype=dtype)))
        x = x + lam[:, None] * (Lx - x)
        if i == 0:
            dv = vol(x + eps * n) - vol(x)
            if dv == 0 or not np.isfinite(dv):
                raise ValueError("smooth_host: the volume does not change along the normals")
            slope = eps / dv
        before = vol(x)
        x = x + n * (slope * (vol0 - before))
        if trace is not None:
            trace.append((lam, before, vol(x), vol0))
    return x


# ---- the filter on the device ---------------------------------------------------------------------------------------------------------
def _edge_csr(edges, V, dev):
    """The CSR of the unique edges, both directions, columns ascending (``sg_mesh_terms_build`` without labels) -> (row_ptr [V+1], col,
    info [2] on the device)."""
    E = int(edges.shape[0])
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    row_ptr, col, info = i32(V + 1), i32(max(2 * E, 1)), i32(_lib.MESH_TERMS_INFO_INTS)
    deg_inv = torch.empty(V, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().sg_mesh_terms_build(V, E, 1, _ptr(edges), None, None, None, None, _ptr(row_ptr), _ptr(col), _ptr(deg_inv), None,
                                               None, _ptr(i32(V)), _ptr(info), _stream(dev)), "body model (edge CSR)")
    return row_ptr, col, info


def smooth_filter(verts, faces, edges=None, lamb=0.5, iterations=5):
    """``smooth_host`` on the device -> new vertices [V,3] fp32; ``verts`` is not written.  ``faces`` [F,3] int32 / int64, ``edges`` the
    unique rows a < b (None: ``topology.unique_edges``).  All arithmetic is fp64, the sums in a fixed order (the normals in 64-bit fixed
    point): two runs give the same bits.  The iterations run without a host read; ONE error word is read at the end, and a vertex
    without a neighbour, a non-finite vertex or a volume that does not change along the normals is a ValueError."""
    if not torch.is_tensor(verts) or not verts.is_cuda:
        raise RuntimeError("sings_amd.body_model: verts must be a GPU tensor (no CPU fallback)")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("sings_amd.body_model: verts must be [V,3] float32")
    if not 0 <= int(iterations) <= _lib.BODY_MAX_ITERATIONS:
        raise ValueError(f"sings_amd.body_model: iterations outside 0..{_lib.BODY_MAX_ITERATIONS}")
    dev, V = verts.device, int(verts.shape[0])
    if not 1 <= V <= MAX_VERTS:
        raise ValueError(f"sings_amd.body_model: {V} vertices (1 .. {MAX_VERTS})")
    f32 = topology._faces_i32(faces, V)
    with torch.cuda.device(dev):
        if edges is None:
            edges = topology.unique_edges(f32, V)[0]
        edges = _marshal._mesh_arg(edges.to(torch.int32).contiguous(), "edges", torch.int32, dev, (2,))
        row_ptr, col, csr_info = _edge_csr(edges, V, dev)
        out, info = _marshal.body_smooth(verts.detach().contiguous(), f32, row_ptr, col, lamb, iterations)
        csr_flags, _, flags = torch.cat([csr_info, info])[:3].tolist()               # the one host read
    if csr_flags & _lib.MESH_TERMS_BAD_EDGE:
        raise ValueError(f"smooth_filter: an edge row is not 0 <= a < b < {V}")
    if flags & _lib.BODY_BAD_FACE:
        raise ValueError(f"smooth_filter: a face indexes a vertex outside [0, {V})")
    if flags & _lib.BODY_NOT_FINITE:
        raise ValueError("smooth_filter: a vertex is not finite")
    if flags & _lib.BODY_ISOLATED:
        raise ValueError("smooth_filter: a vertex has no neighbour (the filter would drag it to the origin)")
    if flags & _lib.BODY_BAD_SLOPE:
        raise ValueError("smooth_filter: the volume does not change along the normals (a flat or closed-up mesh)")
    return out


# ---- reading a model file -------------------------------------------------------------------------------------------------------------
def load_body_arrays(path, num_betas=10):
    """An ``.npz`` with the SMPL-H key names -> the keyword arguments of ``BodyModel`` but ``vertex_label`` (numpy arrays):
    ``v_template`` [V,3], ``shapedirs`` [V,3,>=num_betas] (truncated to ``num_betas``), ``J_regressor`` [J,V] DENSE, ``weights`` [V,J],
    ``kintree_table`` [2,J], ``f`` [F,3], ``posedirs`` [V,3,(J-1)*9] and, when present, ``hands_meanl`` / ``hands_meanr`` [45] (they become
    ``pose_mean``: zeros for the body, then the two hands, as the SMPL-H layer's flat hand mean is laid out).

    Read with ``allow_pickle=False``: an object array (a scipy sparse regressor, a chumpy object) is refused.  A ``.pkl`` is refused
    outright: the published SMPL pickles hold chumpy objects, and unpickling runs arbitrary code.  Convert once, elsewhere, to an
    ``.npz`` of plain arrays.  ``vertex_label`` is an argument of ``BodyModel``: the reference's parsing table is its data."""
    path = str(path)
    if path.lower().endswith((".pkl", ".pickle")):
        raise ValueError(f"load_body_arrays: {path}: a pickle is not read -- the published model files hold chumpy objects and unpickling "
                         "runs arbitrary code; convert it once to an .npz of plain arrays")
    try:
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in NPZ_KEYS if k not in z.files]
            if missing:
                raise ValueError(f"load_body_arrays: {path} lacks {', '.join(missing)}")
            a = {k: z[k] for k in NPZ_KEYS + tuple(k for k in ("hands_meanl", "hands_meanr") if k in z.files)}
    except ValueError as e:
        if "allow_pickle" in str(e) or "Object arrays" in str(e):
            raise ValueError(f"load_body_arrays: {path} holds an object array (a sparse regressor or a chumpy object): only plain dense "
                             "arrays are read (allow_pickle=False)") from e
        raise
    sd = np.asarray(a["shapedirs"], np.float32)
    if sd.ndim != 3 or sd.shape[-1] < int(num_betas) or int(num_betas) < 1:
        raise ValueError(f"load_body_arrays: shapedirs {sd.shape} cannot give {num_betas} betas")
    Jr = np.asarray(a["J_regressor"], np.float32)
    J, V = Jr.shape
    pd = np.asarray(a["posedirs"], np.float32)
    out = dict(v_template=np.asarray(a["v_template"], np.float32), shapedirs=np.ascontiguousarray(sd[:, :, :int(num_betas)]),
               J_regressor=Jr, lbs_weights=np.asarray(a["weights"], np.float32),
               parents=np.asarray(a["kintree_table"]).astype(np.int64)[0].copy(), faces=np.asarray(a["f"]).astype(np.int64),
               posedirs=np.ascontiguousarray(pd.reshape(-1, pd.shape[-1]).T), pose_mean=None)       # smpl_layer.py:262-266
    if "hands_meanl" in a and "hands_meanr" in a:
        hands = np.concatenate([np.asarray(a["hands_meanl"], np.float32).reshape(-1), np.asarray(a["hands_meanr"], np.float32).reshape(-1)])
        mean = np.zeros(3 * J, np.float32)
        if hands.shape[0] > 3 * J:
            raise ValueError(f"load_body_arrays: {hands.shape[0]} hand-mean values for {J} joints")
        mean[3 * J - hands.shape[0]:] = hands
        out["pose_mean"] = mean
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class BodyModel:
    """``BodyModel(v_template [V,3], shapedirs [V,3,B], J_regressor [J,V], lbs_weights [V,J], parents [J], faces [F,3],
    vertex_label [V], posedirs=None | [(J-1)*9, V*3], pose_mean=None | [J*3], device="cuda")`` -- arrays or tensors; they are held as
    fp32 / int32 tensors on ``device``, which must be the GPU.

    ``vertex_id = arange(V)``; ``parents[0]`` is forced to -1 (smpl_layer.py:269-270) and the tree must be in topological order
    (``body._parents_tensor``); ``edges`` are the unique edges of ``faces``.

    The envelope, beyond which the constructor refuses with ValueError: 1 <= J <= 64 (the joint-transform kernels hold a joint per
    lane), 1 <= B <= 32 (a thread of the joint basis keeps B + 1 sums), 3 <= V <= 4 194 304 (2^22), 1 <= F with 3 F < 2^31, face
    corners in [0, V), every array finite."""

    def __init__(self, v_template, shapedirs, J_regressor, lbs_weights, parents, faces, vertex_label, posedirs=None, pose_mean=None,
                 device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("sings_amd.body_model.BodyModel lives on the GPU; there is no CPU fallback")
        as_t = lambda a, dt: None if a is None else (a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dt)
        vt, sd, Jr, w = (as_t(a, torch.float32) for a in (v_template, shapedirs, J_regressor, lbs_weights))
        faces, label = as_t(faces, torch.int64), as_t(vertex_label, torch.int64)
        posedirs, pose_mean = as_t(posedirs, torch.float32), as_t(pose_mean, torch.float32)
        if vt.dim() != 2 or vt.shape[1] != 3:
            raise ValueError(f"BodyModel: v_template must be [V,3], got {tuple(vt.shape)}")
        V = int(vt.shape[0])
        if sd.dim() != 3 or tuple(sd.shape[:2]) != (V, 3):
            raise ValueError(f"BodyModel: shapedirs must be [{V},3,B], got {tuple(sd.shape)}")
        B = int(sd.shape[2])
        if Jr.dim() != 2 or Jr.shape[1] != V:
            raise ValueError(f"BodyModel: J_regressor must be [J,{V}], got {tuple(Jr.shape)}")
        J = int(Jr.shape[0])
        if not (1 <= J <= MAX_JOINTS and 1 <= B <= MAX_BETAS and 3 <= V <= MAX_VERTS):
            raise ValueError(f"BodyModel: J = {J}, B = {B}, V = {V} outside the envelope (J <= {MAX_JOINTS}, B <= {MAX_BETAS}, "
                             f"3 <= V <= {MAX_VERTS})")
        if tuple(w.shape) != (V, J):
            raise ValueError(f"BodyModel: lbs_weights must be [{V},{J}], got {tuple(w.shape)}")
        parents = [int(p) for p in (parents.tolist() if hasattr(parents, "tolist") else parents)]
        if len(parents) != J:
            raise ValueError(f"BodyModel: parents must hold {J} entries, got {len(parents)}")
        parents[0] = -1
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or 3 * int(faces.shape[0]) >= 2 ** 31:
            raise ValueError(f"BodyModel: faces must be [F,3], 1 <= F, 3 F < 2^31, got {tuple(faces.shape)}")
        if int(faces.min()) < 0 or int(faces.max()) >= V:
            raise ValueError(f"BodyModel: a face indexes a vertex outside [0, {V})")
        if tuple(label.shape) != (V,):
            raise ValueError(f"BodyModel: vertex_label must be [{V}], got {tuple(label.shape)}")
        if posedirs is not None and tuple(posedirs.shape) != ((J - 1) * 9, V * 3):
            raise ValueError(f"BodyModel: posedirs must be [{(J - 1) * 9},{V * 3}], got {tuple(posedirs.shape)}")
        if pose_mean is not None and pose_mean.numel() != 3 * J:
            raise ValueError(f"BodyModel: pose_mean must hold {3 * J} values, got {pose_mean.numel()}")
        for name, t in (("v_template", vt), ("shapedirs", sd), ("J_regressor", Jr), ("lbs_weights", w), ("posedirs", posedirs),
                        ("pose_mean", pose_mean)):
            if t is not None and not bool(torch.isfinite(t).all()):
                raise ValueError(f"BodyModel: {name} is not finite")
        self.parents = tuple(parents)
        _parents_tensor(self.parents, dev)                            # (validates the tree: ValueError)
        put = lambda t: None if t is None else t.to(dev).contiguous()
        self.device = dev
        self.v_template, self.shapedirs, self.J_regressor, self.lbs_weights = put(vt), put(sd), put(Jr), put(w)
        self.faces, self.vertex_label = put(faces.to(torch.int32)), put(label.to(torch.int32))
        self.vertex_id = torch.arange(V, dtype=torch.int32, device=dev)
        self.posedirs, self.pose_mean = put(posedirs), None if pose_mean is None else put(pose_mean.reshape(-1))
        with torch.cuda.device(dev):
            self.edges = topology.unique_edges(self.faces, V)[0]
        self._basis = None

    num_verts = property(lambda self: int(self.v_template.shape[0]))
    num_joints = property(lambda self: int(self.J_regressor.shape[0]))
    num_betas = property(lambda self: int(self.shapedirs.shape[2]))

    @classmethod
    def from_arrays(cls, arrays, vertex_label, device="cuda"):
        """``BodyModel(**load_body_arrays(path), vertex_label=...)``."""
        return cls(vertex_label=vertex_label, device=device, **arrays)

    # ---- subdivision
    def subdivided(self, n, smooth=True, lamb=0.5, iterations=5):
        """smpl_layer.py:296-353 -> a new ``BodyModel`` after ``n`` levels.  Each level is ONE ``topology.subdivide_meshes`` over all
        faces: ``vertex_id`` / ``vertex_label`` take the smaller endpoint's value, ``lbs_weights``, ``shapedirs`` (as [V,3B]) and
        ``J_regressor^T`` the endpoint mean; then ``J_regressor`` is renormalised per joint (one launch, fixed-order sums), ``posedirs``
        dropped (the reference replaces it with zeros), ``edges`` rebuilt, and with ``smooth`` the template passes through
        ``smooth_filter`` (``smooth``: True, False, or a callable ``verts -> verts``).  The reference's ``smooth=False`` fails on an
        undefined ``sub_mesh``; here it means no filter."""
        if int(n) < 0:
            raise ValueError("BodyModel.subdivided: n >= 0")
        m = self
        for _ in range(int(n)):
            V = m.num_verts
            if V + int(m.edges.shape[0]) > MAX_VERTS:
                raise ValueError(f"BodyModel.subdivided: {V + int(m.edges.shape[0])} vertices (at most {MAX_VERTS})")
            with torch.cuda.device(m.device):
                verts, faces, attrs = topology.subdivide_meshes(m.v_template, m.faces, None, {
                    "vertex_id": m.vertex_id, "vertex_label": m.vertex_label, "lbs_weights": m.lbs_weights,
                    "shapedirs": m.shapedirs.reshape(V, -1), "J_regressor": m.J_regressor.t().contiguous()})
                new = object.__new__(BodyModel)
                new.device, new.parents, new.pose_mean, new.posedirs, new._basis = m.device, m.parents, m.pose_mean, None, None
                new.faces = faces.to(torch.int32).contiguous()
                new.vertex_id, new.vertex_label, new.lbs_weights = attrs["vertex_id"], attrs["vertex_label"], attrs["lbs_weights"]
                new.shapedirs = attrs["shapedirs"].reshape(-1, 3, m.num_betas).contiguous()
                new.J_regressor = _marshal.body_renorm(attrs["J_regressor"].contiguous())
                new.edges = topology.unique_edges(new.faces, int(verts.shape[0]))[0]
                if callable(smooth):
                    out = smooth(verts)
                    if not torch.is_tensor(out) or tuple(out.shape) != tuple(verts.shape):
                        raise ValueError("BodyModel.subdivided: smooth must return the vertices, [V,3]")
                    verts = out.to(device=m.device, dtype=torch.float32)
                elif smooth:
                    verts = smooth_filter(verts, new.faces, new.edges, lamb=lamb, iterations=iterations)
                new.v_template = verts.contiguous()
            m = new
        return m

    # ---- shape and joints
    def joint_basis(self):
        """-> (J0 [J,3], JS [J,3,B]): ``J_regressor`` folded through [v_template | shapedirs] in one launch (fp64 sums over V in a fixed
        order), computed once per model and cached."""
        if self._basis is None:
            with torch.cuda.device(self.device):
                self._basis = _marshal.body_joint_basis(self.v_template, self.shapedirs, self.J_regressor)
        return self._basis

    def _betas(self, betas):
        if not torch.is_tensor(betas) or not betas.is_cuda:
            raise RuntimeError("sings_amd.body_model: betas must be a GPU tensor (no CPU fallback)")
        if betas.dim() not in (1, 2) or betas.shape[-1] != self.num_betas or betas.dtype != torch.float32:
            raise ValueError(f"sings_amd.body_model: betas must be float32 [{self.num_betas}] or [K,{self.num_betas}], got "
                             f"{tuple(betas.shape)} {betas.dtype}")
        return betas

    def joints_rest(self, betas):
        """``J0 + JS . betas``: [J,3] for betas [B], [K,J,3] for [K,B].  Plain torch ops on the cached basis: differentiable w.r.t.
        ``betas``, so ``joint_transforms_hip``'s dL/djoints_rest reaches a learned betas."""
        betas = self._betas(betas)
        J0, JS = self.joint_basis()
        return J0 + torch.matmul(JS, betas.unsqueeze(-1)).squeeze(-1) if betas.dim() == 1 else \
            J0[None] + torch.einsum("jcb,kb->kjc", JS, betas)

    def pose_feature(self, pose):
        """``(R[1:] - I).flatten()`` of ``pose`` [K, J*3] axis-angle -> [K, (J-1)*9] (lbs.py:142-145)."""
        J = self.num_joints
        R = rodrigues(pose.reshape(-1, 3)).reshape(-1, J, 3, 3)
        return (R[:, 1:] - torch.eye(3, dtype=R.dtype, device=R.device)).reshape(R.shape[0], -1)

    def shaped(self, betas, pose=None):
        """One launch over V -> dict of ``v_shaped``, ``shape_offsets``, ``pose_offsets``, ``v_posed``, [K,V,3] each for ``betas`` [K,B] (a
        [B] vector is one row).  ``shape_offsets = shapedirs . betas``; ``pose_offsets = (R[1:] - I).flatten() . posedirs`` when the model
        has ``posedirs`` and ``pose`` [K,J*3] (or [J*3]) is given -- the unsubdivided model with ``disable_posedirs=False`` -- else zeros.
        No gradient."""
        betas = self._betas(betas).detach().reshape(-1, self.num_betas).contiguous()
        feat = posedirs = None
        if pose is not None and self.posedirs is not None:
            if not torch.is_tensor(pose) or not pose.is_cuda:
                raise RuntimeError("sings_amd.body_model: pose must be a GPU tensor (no CPU fallback)")
            pose = pose.detach().float().reshape(-1, 3 * self.num_joints)
            if pose.shape[0] != betas.shape[0]:
                raise ValueError(f"BodyModel.shaped: {pose.shape[0]} poses for {betas.shape[0]} betas rows")
            feat, posedirs = self.pose_feature(pose).contiguous(), self.posedirs
        with torch.cuda.device(self.device):
            outs = _marshal.body_shaped(self.v_template, self.shapedirs, betas, posedirs, feat)
        return dict(zip(("v_shaped", "shape_offsets", "pose_offsets", "v_posed"), outs))

    # ---- the canonical pose
    def canonical_pose(self, pose_type="da_pose", body="smpl"):
        """The full axis-angle pose [J*3] of ``get_canonical_verts``: zero ``global_orient``, ``canonical.predefined_pose``; for
        ``'smplh'`` its first 63 values, zero hand poses, plus ``pose_mean``."""
        J = self.num_joints
        if body not in ("smpl", "smplh"):
            raise ValueError(f"BodyModel.canonical: body must be 'smpl' or 'smplh', got {body!r}")
        if J != (24 if body == "smpl" else 52):
            raise ValueError(f"BodyModel.canonical: body {body!r} has {24 if body == 'smpl' else 52} joints, the model {J}")
        pose = torch.zeros(3 * J, dtype=torch.float32)
        body_pose = predefined_pose(pose_type)
        if body == "smplh":
            body_pose = body_pose[:63]
        pose[3:3 + body_pose.shape[0]] = body_pose
        pose = pose.to(self.device)
        return pose + self.pose_mean if body == "smplh" and self.pose_mean is not None else pose

    @torch.no_grad()
    def canonical(self, betas, pose_type="da_pose", body="smpl"):
        """``get_canonical_verts`` (sings_hybrid.py:578-596) for one betas vector [B] -> dict of ``verts`` [V,3], ``A_t2cano`` [J,4,4],
        ``inv_A_t2cano``, ``T_t2cano`` [V,4,4], ``inv_T_t2cano``, ``canonical_offsets`` [V,3] (shape plus pose offsets) and ``joints_rest``
        [J,3].  ``A_t2cano`` comes from ``joint_transforms_hip``, the skinning of ``v_posed`` goes through the LBS kernel
        (``lbs.lbs_extra``)."""
        from .lbs import lbs_extra
        betas = self._betas(betas)
        if betas.dim() != 1:
            raise ValueError("BodyModel.canonical: one betas vector [B]")
        pose = self.canonical_pose(pose_type, body)
        with torch.cuda.device(self.device):
            jr = self.joints_rest(betas).contiguous()
            A = joint_transforms_hip(pose[None], jr, self.parents)
            s = self.shaped(betas, pose)
            verts, _, T, _, _ = lbs_extra(A, s["v_posed"], None, self.lbs_weights, pose[None], disable_posedirs=True)
            A, T = A[0], T[0]
            return {"verts": verts[0], "A_t2cano": A, "inv_A_t2cano": torch.inverse(A), "T_t2cano": T, "inv_T_t2cano": torch.inverse(T),
                    "canonical_offsets": (s["shape_offsets"] + s["pose_offsets"])[0], "joints_rest": jr}
