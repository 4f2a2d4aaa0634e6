"""How tensors, cameras, skin inputs and frame batches become arguments of the C ABI (``_lib._PROTOTYPES``).

The one place that knows it: the drop-in op (rasterizer.py), the skinned ops (skinned.py), the pre-allocated engines (engine.py)
and every other caller of the library take these functions from here.  Imports ``_lib`` only, so nothing above it can form an
import cycle through it.  What a caller converts or refuses before it gets here (``_f32`` or ``.contiguous().float()``) and the
exception type of a malformed input are the caller's: they differ between the ops and the engines.
"""
import ctypes as C

import torch

from . import _lib


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _stream(dev):
    """The ``void *stream`` argument: torch's current HIP stream on ``dev``."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(t, name, dev):
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.device != dev:
        raise RuntimeError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


def _settings_struct(rs, dev, sh_coeffs, keep):
    bg = _f32(rs.bg, "bg", dev); vm = _f32(rs.viewmatrix, "viewmatrix", dev)
    pm = _f32(rs.projmatrix, "projmatrix", dev); cp = _f32(rs.campos, "campos", dev)
    keep.extend([bg, vm, pm, cp])
    s = _lib.SgRasterSettings()
    s.image_height = int(rs.image_height); s.image_width = int(rs.image_width)
    s.tanfovx = float(rs.tanfovx); s.tanfovy = float(rs.tanfovy)
    s.scale_modifier = float(rs.scale_modifier)
    s.sh_degree = int(rs.sh_degree); s.sh_coeffs = int(sh_coeffs)
    s.prefiltered = int(bool(rs.prefiltered)); s.debug = int(bool(rs.debug)); s.flags = 0
    s.bg = bg.data_ptr(); s.viewmatrix = vm.data_ptr(); s.projmatrix = pm.data_ptr(); s.campos = cp.data_ptr()
    s.count_signal = None; s.count_signal_host = None
    return s


def _camera_stride(rs, K, error):
    """SgFrameBatch.camera_stride of K frames: 0, one camera for all of them ([4,4] matrices), or 1, one per frame (``viewmatrix`` /
    ``projmatrix`` [K,4,4], ``campos`` [K,3]).  ``error``: the exception class of the caller for cameras stacked otherwise."""
    if rs.viewmatrix.dim() != 3:
        return 0
    if rs.viewmatrix.shape[0] != K or rs.projmatrix.shape[0] != K or rs.campos.shape[0] != K:
        raise error(f"per-frame cameras must be stacked [{K},4,4] / [{K},3]")
    return 1


def _skin_struct(dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, keep, J=None):
    """rotmat_canon: None (isotropic), [N,9] / [N,3,3] rotation matrices, or [N,6] in the decoder's 6-D form
    (rotation_6d_to_matrix then runs inside the kernels).  ``J``: None, ``A`` holds the joints of ONE frame; else ``A`` (and
    ``transl``) are the stacked frames of a K-frame call, J joints each, and the struct points at their first frame."""
    k = _lib.SgSkinInputs()
    A = _f32(A, "A", dev).reshape(-1, 16)
    k.J = int(A.shape[0]) if J is None else int(J)
    k.rot_format = 1 if (rotmat_canon is not None and rotmat_canon.shape[-1] == 6 and rotmat_canon.dim() == 2) else 0
    lbs_weights = _f32(lbs_weights, "lbs_weights", dev)
    if lbs_weights.shape != (xyz_canon.shape[0], k.J):
        raise RuntimeError(f"lbs_weights must be [N,{k.J}], got {tuple(lbs_weights.shape)}")
    ts = [xyz_canon, rotmat_canon, lbs_weights, A,
          None if smpl_scale is None else _f32(smpl_scale, "smpl_scale", dev).reshape(-1),
          None if transl is None else _f32(transl, "transl", dev).reshape(-1)]
    if ext_tfs is not None:
        tr, rm, sc = ext_tfs
        ts += [_f32(tr, "ext trans", dev).reshape(-1), _f32(rm, "ext rotmat", dev).reshape(-1),
               _f32(sc, "ext scale", dev).reshape(-1)]
    else:
        ts += [None, None, None]
    keep.extend(ts)
    for name, t in zip(("xyz_canon", "rot_canon", "lbs_weights", "A", "smpl_scale", "transl", "ext_trans", "ext_rot",
                        "ext_scale"), ts):
        setattr(k, name, None if t is None else t.data_ptr())
    return k


def _frame_batch(K, camera_stride, transl_stride, placement=0):
    fb = _lib.SgFrameBatch()
    fb.K, fb.camera_stride, fb.transl_stride, fb.placement = int(K), int(camera_stride), int(transl_stride), int(placement)
    return fb


def _frame_rows(t, K, width, name):
    """An input of K frames that may be shared -> (tensor, per_frame): ONE set of ``width`` floats for every frame (``width``
    elements -- a leading 1 included -- or an ``.expand`` view, stride 0 along the frames: its first row, not copied), or K rows
    [K, width] (per_frame True)."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.numel() == width:
        return t.reshape(width), False
    if t.dim() >= 1 and t.shape[0] == K and t[0].numel() == width:
        if t.stride(0) == 0:
            return t[0].reshape(width), False
        return t.reshape(K, width), True
    raise ValueError(f"{name} must be [{width}] (one for all frames) or [{K},{width}] (one per frame), got {tuple(t.shape)}")


def _skin_frames(dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, camera_stride, keep, error,
                 placement=0):
    """The skin inputs and the frame batch of a K-frame call -> (SgSkinInputs, SgFrameBatch, forward_only).  ``A``: [K,J,16];
    ``transl``: None, 3 floats shared by the frames (``transl_stride`` 0) or 3 per frame (3), anything else raises ``error``;
    ``placement``: the SG_PLACEMENT_* bits of a caller that hands over ``smpl_scale`` / ``ext_tfs`` as one set per frame.
    ``forward_only``: the frames carry ext_tfs or per-frame sets, which have no backward (the reference applies them under
    no_grad)."""
    K, J = int(A.shape[0]), int(A.shape[1])
    tstride = 0
    if transl is not None and transl.numel() != 3:
        if transl.numel() != 3 * K:
            raise error(f"transl must be [{K},3] or [3], got {tuple(transl.shape)}")
        tstride = 3
    k = _skin_struct(dev, xyz_canon, rotmat_canon, lbs_weights, A, smpl_scale, transl, ext_tfs, keep, J=J)
    return k, _frame_batch(K, camera_stride, tstride, placement), ext_tfs is not None or bool(placement)


def _scene_structs(dev, avatars, keep):
    """The avatars of a scene (include/sings_scene.h) -> the host array ``SgSceneAvatar[S]``.  ``avatars``: one dict per avatar of
    fp32 tensors on ``dev`` -- ``xyz_canon`` [P,3], ``rot_canon`` [P,9] / [P,6] / None, ``lbs_weights`` [P,J], ``scales``,
    ``opacities``, ``shs`` [P,M,3], ``A`` [K,J,16], and with K rows each or None: ``transl``, ``smpl_scale``, ``ext_trans``, ``ext_rot``,
    ``ext_scale`` (shapes are the caller's to check: SceneFramesEngine.set_frames).  ``keep``: receives every tensor the structs
    point at; the array itself must also outlive the call."""
    arr = (_lib.SgSceneAvatar * len(avatars))()
    for a, av in zip(arr, avatars):
        ts = {n: _f32(av.get(n), n, dev) for n in ("xyz_canon", "rot_canon", "lbs_weights", "scales", "opacities", "shs", "A", "transl",
                                                  "smpl_scale", "ext_trans", "ext_rot", "ext_scale")}
        a.P, a.J = int(ts["xyz_canon"].shape[0]), int(ts["A"].shape[-2])
        rot = ts["rot_canon"]
        a.rot_format, a.reserved = (1 if rot is not None and rot.dim() == 2 and rot.shape[-1] == 6 else 0), 0
        for n, t in ts.items():
            setattr(a, n, None if t is None else t.data_ptr())
        keep.extend(t for t in ts.values() if t is not None)
    return arr


def adam_step(segments, chunks, hyper, grad_flat, exp_avg, exp_avg_sq):
    """``sg_adam_step`` on torch's current stream: ``segments`` [S,4] int64, ``chunks`` [C,2] int32 and ``hyper`` [G,8] fp32 are
    device tensors (``sings_amd.optim.build_tables`` / ``hyper_row``), the other three the flat fp32 buffers of one layout."""
    dev = grad_flat.device
    for name, t, dt in (("segments", segments, torch.int64), ("chunks", chunks, torch.int32), ("hyper", hyper, torch.float32),
                        ("grad_flat", grad_flat, torch.float32), ("exp_avg", exp_avg, torch.float32),
                        ("exp_avg_sq", exp_avg_sq, torch.float32)):
        if not t.is_cuda or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"adam_step: {name} must be a contiguous {dt} tensor on {dev} (no CPU fallback)")
    if exp_avg.numel() != grad_flat.numel() or exp_avg_sq.numel() != grad_flat.numel():
        raise RuntimeError("adam_step: grad_flat, exp_avg and exp_avg_sq must have the same number of elements")
    _lib.check(_lib.load().sg_adam_step(int(segments.shape[0]), int(chunks.shape[0]), int(hyper.shape[0]), _ptr(segments), _ptr(chunks),
                                        _ptr(hyper), _ptr(grad_flat), _ptr(exp_avg), _ptr(exp_avg_sq), _stream(dev)), "sg_adam_step")


# ---- mesh topology (csrc/sg_mesh.hip)
def _mesh_arg(t, name, dtype, dev, shape_tail=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (no CPU fallback)")
    if t.device != dev or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor on {dev}")
    if shape_tail is not None and tuple(t.shape[1:]) != shape_tail:
        raise ValueError(f"{name} must be [n, {', '.join(map(str, shape_tail))}], got {tuple(t.shape)}")
    return t


def mesh_unique_edges(faces, num_verts, flags=None):
    """``sg_mesh_edges_build`` + ONE host read of (E, flagged faces, bad-index flag) + ``sg_mesh_edges_emit`` on torch's current
    stream: ``faces`` [F,3] int32, ``flags`` [F] uint8 or None -> (edges [E,2], edge_faces [E], face_edges [F,3], Fs), all int32."""
    dev = faces.device if torch.is_tensor(faces) else None
    faces = _mesh_arg(faces, "faces", torch.int32, dev, (3,))
    V, F = int(num_verts), int(faces.shape[0])
    if flags is not None and tuple(_mesh_arg(flags, "flags", torch.uint8, dev).shape) != (F,):
        raise ValueError(f"flags must be [{F}], got {tuple(flags.shape)}")
    lib = _lib.load()
    nbytes = int(lib.sg_mesh_ws_bytes(V, F))
    if nbytes == 0:
        raise ValueError(f"mesh_unique_edges: {V} vertices / {F} faces are outside what the kernels cover (V <= 2^30, 3 F < 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.sg_mesh_edges_build(V, F, _ptr(faces), _ptr(flags), _ptr(ws), _ptr(info), _stream(dev)), "sg_mesh_edges_build")
        E, Fs, bad, _ = info.tolist()                                 # the one host read: E sizes the outputs
        if bad:
            raise IndexError(f"mesh_unique_edges: a face indexes a vertex outside [0, {V})")
        edges = torch.empty((E, 2), dtype=torch.int32, device=dev)
        edge_faces = torch.empty(E, dtype=torch.int32, device=dev)
        face_edges = torch.empty((F, 3), dtype=torch.int32, device=dev)
        _lib.check(lib.sg_mesh_edges_emit(V, F, E, _ptr(faces), _ptr(flags), _ptr(ws), _ptr(edges), _ptr(edge_faces), _ptr(face_edges),
                                          _stream(dev)), "sg_mesh_edges_emit")
    return edges, edge_faces, face_edges, Fs


def mesh_subdivide(faces, num_verts, flags, face_edges, num_flagged):
    """``sg_mesh_subdivide``: -> new_faces [F - Fs + 4 Fs, 3] int32 (the unflagged faces, then four children per flagged face)."""
    dev = faces.device if torch.is_tensor(faces) else None
    faces = _mesh_arg(faces, "faces", torch.int32, dev, (3,))
    V, F, Fs = int(num_verts), int(faces.shape[0]), int(num_flagged)
    face_edges = _mesh_arg(face_edges, "face_edges", torch.int32, dev, (3,))
    if flags is not None:
        _mesh_arg(flags, "flags", torch.uint8, dev)
    if face_edges.shape[0] != F or (flags is not None and tuple(flags.shape) != (F,)):
        raise ValueError("mesh_subdivide: flags [F] and face_edges [F,3] must describe the faces")
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(lib.sg_mesh_ws_bytes(V, F)), 1), dtype=torch.uint8, device=dev)
        out = torch.empty((F - Fs + 4 * Fs, 3), dtype=torch.int32, device=dev)
        _lib.check(lib.sg_mesh_subdivide(V, F, Fs, _ptr(faces), _ptr(flags), _ptr(face_edges), _ptr(ws), _ptr(out), _stream(dev)),
                   "sg_mesh_subdivide")
    return out


def mesh_midpoints(edges, src):
    """``sg_mesh_midpoints`` (fp32 ``src`` [V,C]: the endpoints' mean) / ``sg_mesh_midpoints_i32`` (int32: the smaller endpoint's
    value) -> [E,C] of ``src``'s dtype."""
    dev = edges.device if torch.is_tensor(edges) else None
    edges = _mesh_arg(edges, "edges", torch.int32, dev, (2,))
    if not torch.is_tensor(src) or src.dtype not in (torch.float32, torch.int32) or src.dim() != 2 or src.shape[1] < 1:
        raise ValueError("mesh_midpoints: src must be a [V,C] float32 or int32 tensor, C >= 1")
    src = _mesh_arg(src, "src", src.dtype, dev)
    V, C, E = int(src.shape[0]), int(src.shape[1]), int(edges.shape[0])
    lib = _lib.load()
    fn, what = (lib.sg_mesh_midpoints, "sg_mesh_midpoints") if src.dtype == torch.float32 else (lib.sg_mesh_midpoints_i32,
                                                                                                  "sg_mesh_midpoints_i32")
    with torch.cuda.device(dev):
        dst = torch.empty((E, C), dtype=src.dtype, device=dev)
        _lib.check(fn(V, E, C, _ptr(edges), _ptr(src), _ptr(dst), _stream(dev)), what)
    return dst


def mesh_collapse_max_edges():
    """``sg_mesh_collapse_max_edges``: the most selected edges one ``mesh_collapse`` takes (they stay resident in LDS)."""
    return int(_lib.load().sg_mesh_collapse_max_edges())


def mesh_collapse(verts, selected_edges, faces, collapse_rate):
    """``sg_mesh_collapse_build`` + ONE host read of info[8] + ``sg_mesh_collapse_emit`` on torch's current stream: ``verts`` [V,3]
    fp32, ``selected_edges`` [Es,2] and ``faces`` [F,3] int32 -> (new_faces [F',3] int32, prune_mask [V] uint8, survivors [V'] int32,
    collapses done).  A selected row that is not 0 <= a < b < V or a non-finite vertex raises ValueError, a face corner outside
    [0, V) IndexError."""
    dev = verts.device if torch.is_tensor(verts) else None
    verts = _mesh_arg(verts, "verts", torch.float32, dev, (3,))
    selected_edges = _mesh_arg(selected_edges, "selected_edges", torch.int32, dev, (2,))
    faces = _mesh_arg(faces, "faces", torch.int32, dev, (3,))
    V, F, Es = int(verts.shape[0]), int(faces.shape[0]), int(selected_edges.shape[0])
    lib = _lib.load()
    cap = int(lib.sg_mesh_collapse_max_edges())
    if Es > cap:
        raise ValueError(f"mesh_collapse: {Es} selected edges, one call takes at most {cap}")
    nbytes = int(lib.sg_mesh_collapse_ws_bytes(V, F))
    if nbytes == 0:
        raise ValueError(f"mesh_collapse: {V} vertices / {F} faces are outside what the kernels cover (1 <= V <= 2^30, 3 F < 2^31)")
    rate = C.c_double(float(collapse_rate))
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        info = torch.empty(8, dtype=torch.int32, device=dev)
        _lib.check(lib.sg_mesh_collapse_build(V, F, Es, _ptr(verts), _ptr(selected_edges), _ptr(faces), C.byref(rate), _ptr(ws), _ptr(info),
                                              _stream(dev)), "sg_mesh_collapse_build")
        Fn, Vn, done, bad_edge, bad_face = info.tolist()[:5]          # the one host read: F' and V' size the outputs
        if bad_edge & 2:
            raise ValueError("mesh_collapse: a vertex is not finite")
        if bad_edge:
            raise ValueError(f"mesh_collapse: a selected edge is not a row 0 <= a < b < {V}")
        if bad_face:
            raise IndexError(f"mesh_collapse: a face indexes a vertex outside [0, {V})")
        new_faces = torch.empty((Fn, 3), dtype=torch.int32, device=dev)
        prune_mask = torch.empty(V, dtype=torch.uint8, device=dev)
        survivors = torch.empty(Vn, dtype=torch.int32, device=dev)
        _lib.check(lib.sg_mesh_collapse_emit(V, F, Fn, Vn, _ptr(faces), _ptr(ws), _ptr(new_faces), _ptr(prune_mask), _ptr(survivors),
                                             _stream(dev)), "sg_mesh_collapse_emit")
    return new_faces, prune_mask, survivors, done


# ---- initial values and the decoder pre-fit (csrc/sg_init.hip)
ATTR_MSE_WIDTHS = (3, 3, 3, 6, 48, 1)             # floats per row of xyz_offsets, scales, scales_aux, rot6d_canon, shs, opacity


def init_attributes(verts, faces, edges, init_scale_multiplier, thickness_factor):
    """``sg_init_attributes`` on torch's current stream: ``verts`` [V,3] fp32, ``faces`` [F,3] and ``edges`` [E,2] int32 -> (dict of
    ``first`` / ``second`` [V] int32, ``scales`` / ``scales_aux`` / ``normals`` [V,3] and ``rotmat`` [V,3,3] fp32, info [4] int32 on the
    device: the caller reads it)."""
    dev = verts.device if torch.is_tensor(verts) else None
    verts = _mesh_arg(verts, "verts", torch.float32, dev, (3,))
    faces = _mesh_arg(faces, "faces", torch.int32, dev, (3,))
    edges = _mesh_arg(edges, "edges", torch.int32, dev, (2,))
    V, F, E = int(verts.shape[0]), int(faces.shape[0]), int(edges.shape[0])
    lib = _lib.load()
    nbytes = int(lib.sg_init_ws_bytes(V))
    if V < 1 or nbytes == 0:
        raise ValueError(f"init_attributes: {V} vertices are outside what the kernels cover (1 <= V <= 2^30)")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = {"first": torch.empty(V, dtype=torch.int32, device=dev), "second": torch.empty(V, dtype=torch.int32, device=dev)}
        for k in ("scales", "scales_aux", "normals"):
            out[k] = torch.empty((V, 3), dtype=torch.float32, device=dev)
        out["rotmat"] = torch.empty((V, 3, 3), dtype=torch.float32, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.sg_init_attributes(V, F, E, float(init_scale_multiplier), float(thickness_factor), _ptr(verts), _ptr(faces),
                                          _ptr(edges), _ptr(ws), _ptr(out["first"]), _ptr(out["second"]), _ptr(out["scales"]),
                                          _ptr(out["scales_aux"]), _ptr(out["normals"]), _ptr(out["rotmat"]), _ptr(info), _stream(dev)),
                   "sg_init_attributes")
    return out, info


def attr_mse_ws_bytes():
    return int(_lib.load().sg_attr_mse_ws_bytes())


def _pointer_row(tensors):
    """Six tensors (or None) -> the host array of six device pointers ``sg_attr_mse`` takes."""
    return (C.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in tensors])


def attr_mse(N, outputs, targets, grads, ws, terms):
    """``sg_attr_mse`` on torch's current stream.  ``outputs`` / ``targets`` / ``grads``: six entries each in the order of
    ``ATTR_MSE_WIDTHS``, a contiguous fp32 GPU tensor of N rows or None (``grads``: None for no gradient at all); ``ws``:
    ``attr_mse_ws_bytes()`` bytes; ``terms``: 8 floats.  Nothing is allocated here."""
    dev = terms.device
    if not terms.is_cuda or terms.dtype != torch.float32 or terms.numel() < 8 or not ws.is_cuda or ws.numel() * ws.element_size() < attr_mse_ws_bytes():
        raise RuntimeError("attr_mse: terms must be 8 fp32 values and ws attr_mse_ws_bytes() bytes on the GPU (no CPU fallback)")
    rows = [outputs, targets] + ([grads] if grads is not None else [])
    for row in rows:
        if len(row) != 6:
            raise ValueError("attr_mse: six entries per row (None for an absent pair)")
        for t, w in zip(row, ATTR_MSE_WIDTHS):
            if t is None:
                continue
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError("attr_mse: tensors must live on the GPU (no CPU fallback)")
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != int(N) * w:
                raise ValueError(f"attr_mse: every tensor must be contiguous fp32 on {dev} with {int(N)} rows of its width ({w})")
    for k in range(6):
        if (outputs[k] is None) != (targets[k] is None) or (grads is not None and grads[k] is not None and outputs[k] is None):
            raise ValueError("attr_mse: a pair needs both its output and its target")
    _lib.check(_lib.load().sg_attr_mse(int(N), _pointer_row(outputs), _pointer_row(targets),
                                       None if grads is None else _pointer_row(grads), _ptr(ws), _ptr(terms), _stream(dev)), "sg_attr_mse")


def plateau_step(n_groups, begin, patience, settings, loss, state, hyper, terms, n_copy, log, log_rows):
    """``sg_plateau_step`` on torch's current stream.  ``settings``: a ``ctypes.c_double * 3`` (factor, threshold, eps); ``loss``: a
    view of one fp32 value; ``state`` / ``log``: fp64 device tensors (``log`` may be None); ``hyper``: ``FusedAdam.hyper`` or None."""
    dev = state.device
    for name, t, dt in (("loss", loss, torch.float32), ("state", state, torch.float64), ("hyper", hyper, torch.float32),
                        ("terms", terms, torch.float32), ("log", log, torch.float64)):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dtype != dt or not t.is_contiguous()):
            raise RuntimeError(f"plateau_step: {name} must be a contiguous {dt} tensor on {dev} (no CPU fallback)")
    if state.numel() < 4 + 2 * int(n_groups) or (hyper is not None and tuple(hyper.shape) != (int(n_groups), 8)):
        raise ValueError("plateau_step: state must hold 4 + 2 G doubles and hyper be [G,8]")
    if log is not None and log.numel() < int(log_rows) * (int(n_copy) + int(n_groups)):
        raise ValueError("plateau_step: log must hold log_rows rows of n_copy + G doubles")
    if terms is not None and terms.numel() < int(n_copy):
        raise ValueError("plateau_step: terms must hold n_copy floats")
    _lib.check(_lib.load().sg_plateau_step(int(n_groups), int(bool(begin)), int(patience), settings, _ptr(loss), _ptr(state), _ptr(hyper),
                                           _ptr(terms), int(n_copy), _ptr(log), int(log_rows), _stream(dev)), "sg_plateau_step")


# ---- densification statistics (csrc/sg_density.hip)
def density_stats(grad, radii, gate, accum, denom, max_radii):
    """``sg_density_stats`` on torch's current stream: ``grad`` [N,3] / [K,N,3] fp32 and ``radii`` [N] / [K,N] int32 of one step;
    ``accum``, ``denom``, ``max_radii``: N contiguous fp32 each ([N] or [N,1]), updated in place; ``gate``: int32 [1] on the device
    or None."""
    if not torch.is_tensor(grad) or not grad.is_cuda:
        raise RuntimeError("density_stats: grad must be a GPU tensor (no CPU fallback)")
    dev = grad.device
    if grad.dim() not in (2, 3) or grad.shape[-1] != 3:
        raise ValueError(f"density_stats: grad must be [N,3] or [K,N,3], got {tuple(grad.shape)}")
    N, K = int(grad.shape[-2]), (int(grad.shape[0]) if grad.dim() == 3 else 1)
    if not torch.is_tensor(radii) or tuple(radii.shape) not in ((K, N),) + (((N,),) if K == 1 else ()):
        raise ValueError(f"density_stats: radii must be [{K},{N}]" + (f" or [{N}]" if K == 1 else "") +
                         f", got {tuple(radii.shape) if torch.is_tensor(radii) else type(radii).__name__}")
    for name, t, dt in (("grad", grad, torch.float32), ("radii", radii, torch.int32), ("gate", gate, torch.int32),
                        ("accum", accum, torch.float32), ("denom", denom, torch.float32), ("max_radii", max_radii, torch.float32)):
        if t is None and name == "gate":
            continue
        if not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"density_stats: {name} must be a contiguous {dt} tensor on {dev} (no CPU fallback)")
        if name in ("accum", "denom", "max_radii") and t.numel() != N:
            raise ValueError(f"density_stats: {name} must hold {N} values, got {tuple(t.shape)}")
    if gate is not None and gate.numel() != 1:
        raise ValueError(f"density_stats: gate must hold one int32, got {tuple(gate.shape)}")
    if not 1 <= K <= _lib.DENSITY_MAX_K:
        raise ValueError(f"density_stats: K = {K} outside 1..{_lib.DENSITY_MAX_K}")
    lib = _lib.load()
    if not _lib.HAS_DENSITY:
        raise RuntimeError("density_stats: the loaded library predates include/sings_density.h (no fallback): rebuild it")
    with torch.cuda.device(dev):
        _lib.check(lib.sg_density_stats(K, N, _ptr(grad), _ptr(radii), _ptr(gate), _ptr(accum), _ptr(denom), _ptr(max_radii),
                                        _stream(dev)), "sg_density_stats")


# ---- the body model (csrc/sg_body.hip)
def _body_lib():
    lib = _lib.load()
    if not _lib.HAS_BODY:
        raise RuntimeError("the loaded library predates include/sings_body.h (no fallback): rebuild it")
    return lib


def body_renorm(Jt):
    """``sg_body_renorm`` on torch's current stream: ``Jt`` [V,J] fp32 (the subdivided J_regressor^T) -> J_regressor [J,V], every row
    divided by its sum."""
    dev = Jt.device if torch.is_tensor(Jt) else None
    Jt = _mesh_arg(Jt, "Jt", torch.float32, dev)
    V, J = int(Jt.shape[0]), int(Jt.shape[1])
    with torch.cuda.device(dev):
        out = torch.empty((J, V), dtype=torch.float32, device=dev)
        _lib.check(_body_lib().sg_body_renorm(J, V, _ptr(Jt), _ptr(out), _stream(dev)), "sg_body_renorm")
    return out


def body_joint_basis(v_template, shapedirs, J_regressor):
    """``sg_body_joint_basis`` on torch's current stream: ``v_template`` [V,3], ``shapedirs`` [V,3,B], ``J_regressor`` [J,V] fp32 ->
    (J0 [J,3], JS [J,3,B])."""
    dev = v_template.device if torch.is_tensor(v_template) else None
    v_template = _mesh_arg(v_template, "v_template", torch.float32, dev, (3,))
    V, B, J = int(v_template.shape[0]), int(shapedirs.shape[-1]), int(J_regressor.shape[0])
    shapedirs = _mesh_arg(shapedirs, "shapedirs", torch.float32, dev, (3, B))
    J_regressor = _mesh_arg(J_regressor, "J_regressor", torch.float32, dev, (V,))
    if shapedirs.shape[0] != V:
        raise ValueError(f"body_joint_basis: shapedirs has {shapedirs.shape[0]} rows, the template {V} vertices")
    with torch.cuda.device(dev):
        J0 = torch.empty((J, 3), dtype=torch.float32, device=dev)
        JS = torch.empty((J, 3, B), dtype=torch.float32, device=dev)
        _lib.check(_body_lib().sg_body_joint_basis(V, J, B, _ptr(v_template), _ptr(shapedirs), _ptr(J_regressor), _ptr(J0), _ptr(JS),
                                                   _stream(dev)), "sg_body_joint_basis")
    return J0, JS


def body_shaped(v_template, shapedirs, betas, posedirs=None, pose_feature=None):
    """``sg_body_shaped`` on torch's current stream: ``betas`` [K,B]; ``posedirs`` [P,3V] with ``pose_feature`` [K,P], or both None ->
    (v_shaped, shape_offsets, pose_offsets, v_posed), [K,V,3] fp32 each."""
    dev = v_template.device if torch.is_tensor(v_template) else None
    v_template = _mesh_arg(v_template, "v_template", torch.float32, dev, (3,))
    V, B = int(v_template.shape[0]), int(shapedirs.shape[-1])
    shapedirs = _mesh_arg(shapedirs, "shapedirs", torch.float32, dev, (3, B))
    betas = _mesh_arg(betas, "betas", torch.float32, dev, (B,))
    K, P = int(betas.shape[0]), 0
    if shapedirs.shape[0] != V:
        raise ValueError(f"body_shaped: shapedirs has {shapedirs.shape[0]} rows, the template {V} vertices")
    if (posedirs is None) != (pose_feature is None):
        raise ValueError("body_shaped: posedirs and pose_feature come together")
    if posedirs is not None:
        posedirs = _mesh_arg(posedirs, "posedirs", torch.float32, dev, (3 * V,))
        P = int(posedirs.shape[0])
        pose_feature = _mesh_arg(pose_feature, "pose_feature", torch.float32, dev, (P,))
        if pose_feature.shape[0] != K:
            raise ValueError(f"body_shaped: pose_feature has {pose_feature.shape[0]} rows, betas {K}")
    with torch.cuda.device(dev):
        outs = [torch.empty((K, V, 3), dtype=torch.float32, device=dev) for _ in range(4)]
        _lib.check(_body_lib().sg_body_shaped(V, B, K, P, _ptr(v_template), _ptr(shapedirs), _ptr(betas), _ptr(posedirs), _ptr(pose_feature),
                                              *(_ptr(o) for o in outs), _stream(dev)), "sg_body_shaped")
    return tuple(outs)


def body_smooth(verts, faces, row_ptr, col, lamb, iterations):
    """``sg_body_smooth`` on torch's current stream: ``verts`` [V,3] fp32, ``faces`` [F,3] int32, ``row_ptr`` [V+1] / ``col`` int32 (the
    CSR of the unique edges) -> (x_out [V,3] fp32, written only when no error bit is set; info [``_lib.BODY_INFO_INTS``] int32 on the
    device: the caller reads it)."""
    dev = verts.device if torch.is_tensor(verts) else None
    verts = _mesh_arg(verts, "verts", torch.float32, dev, (3,))
    faces = _mesh_arg(faces, "faces", torch.int32, dev, (3,))
    row_ptr = _mesh_arg(row_ptr, "row_ptr", torch.int32, dev)
    col = _mesh_arg(col, "col", torch.int32, dev)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if tuple(row_ptr.shape) != (V + 1,):
        raise ValueError(f"body_smooth: row_ptr must be [{V + 1}], got {tuple(row_ptr.shape)}")
    lib = _body_lib()
    nbytes = int(lib.sg_body_smooth_ws_bytes(V, F))
    if nbytes == 0:
        raise ValueError(f"body_smooth: {V} vertices / {F} faces are outside what the kernels cover (1 <= V <= {_lib.BODY_MAX_VERTS}, "
                         "1 <= F, 3 F < 2^31)")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        info = torch.empty(_lib.BODY_INFO_INTS, dtype=torch.int32, device=dev)
        _lib.check(lib.sg_body_smooth(V, F, int(iterations), float(lamb), _ptr(verts), _ptr(faces), _ptr(row_ptr), _ptr(col), _ptr(ws),
                                      _ptr(out), _ptr(info), _stream(dev)), "sg_body_smooth")
    return out, info


# ---- frames to JPEG and PNG files, PNG files to the frame store (csrc/sg_jpeg.hip, sg_png.hip, sg_unpng.hip)
def _codec_lib(codec):
    """The library, once ``_lib.HAS_<CODEC>`` says that it holds include/sings_<codec>.h."""
    lib = _lib.load()
    if not getattr(_lib, f"HAS_{codec.upper()}"):
        raise RuntimeError(f"the loaded library predates include/sings_{codec}.h (no fallback): rebuild it")
    return lib


def _codec_layout(codec, *args):
    """``sg_<codec>_layout(*args, out)`` -> dict of ``_lib.<CODEC>_LAYOUT``."""
    names, fn = getattr(_lib, f"{codec.upper()}_LAYOUT"), f"sg_{codec}_layout"
    out = (C.c_size_t * len(names))()
    _lib.check(getattr(_codec_lib(codec), fn)(*(int(a) for a in args), out), fn)
    return {name: int(v) for name, v in zip(names, out)}


def _codec_tensors(who, dev, rows):
    """``rows`` of (name, tensor, dtype, least elements): every tensor of its type on ``dev``, contiguous and large enough.  ``out``
    alone may be a view with a row pitch: ``_encoder_tensors`` checks its shape."""
    for name, t, dt, least in rows:
        if not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dtype != dt:
            raise RuntimeError(f"{who}: {name} must be a {dt} tensor on {dev} (no CPU fallback)")
        if name == "out":
            continue
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: {name} must be contiguous")
        if t.numel() < least:
            raise ValueError(f"{who}: {name} holds {t.numel()} elements, {least} needed")


def _encoder_tensors(who, K, W, H, table_words, frames, tables, header, ws, out, capacity, sizes):
    """What the two ``*_encode_frames`` take: ``frames`` uint8 [K,H,W,3]; ``tables`` int32 words and ``header`` uint8, the caller's; ``ws``
    uint8; ``out`` uint8 rows of ``capacity`` bytes (its row pitch) and ``sizes`` int32 [K]."""
    _codec_tensors(who, frames.device, (("frames", frames, torch.uint8, int(K) * int(H) * int(W) * 3), ("tables", tables, torch.int32, table_words),
                                        ("header", header, torch.uint8, 1), ("ws", ws, torch.uint8, 1), ("out", out, torch.uint8, 0),
                                        ("sizes", sizes, torch.int32, int(K))))
    if out.dim() != 2 or out.stride(1) != 1 or out.stride(0) != int(capacity) or out.shape[0] < int(K) or out.shape[1] != int(capacity):
        raise ValueError(f"{who}: out must be [>= {int(K)}, {int(capacity)}] uint8 with rows of capacity bytes, got "
                         f"{tuple(out.shape)} strides {tuple(out.stride())}")


def jpeg_layout(W, H, K, restart_interval, header_bytes):
    """``sg_jpeg_layout`` -> dict of ``_lib.JPEG_LAYOUT``: the workspace bytes of K frames, MCUs and restart segments per frame, the
    bytes of a segment's slot, the largest file a frame can become and the default capacity."""
    return _codec_layout("jpeg", W, H, K, restart_interval, header_bytes)


def jpeg_encode_frames(K, W, H, restart_interval, bgr, frames, tables, header, ws, out, capacity, sizes, stream):
    """``sg_jpeg_encode_frames`` on ``stream`` (a torch stream): ``_encoder_tensors`` with ``_lib.JPEG_TABLE_WORDS`` table words
    (``sings_amd.video``) and ``jpeg_layout``'s ``ws_bytes``.  Nothing is allocated here."""
    _encoder_tensors("jpeg_encode_frames", K, W, H, _lib.JPEG_TABLE_WORDS, frames, tables, header, ws, out, capacity, sizes)
    _lib.check(_codec_lib("jpeg").sg_jpeg_encode_frames(int(K), int(W), int(H), int(restart_interval), int(bool(bgr)), _ptr(frames),
                                                        _ptr(tables), _ptr(header), int(header.numel()), _ptr(ws), int(ws.numel()), _ptr(out),
                                                        int(capacity), _ptr(sizes), C.c_void_p(stream.cuda_stream)), "sg_jpeg_encode_frames")


def png_layout(W, H, K, rows_per_segment, header_bytes):
    """``sg_png_layout`` -> dict of ``_lib.PNG_LAYOUT``: the workspace bytes of K frames, segments per frame, the bytes of a segment and
    of its slot, and the largest file a frame can become (the default capacity)."""
    return _codec_layout("png", W, H, K, rows_per_segment, header_bytes)


def png_encode_frames(K, W, H, rows_per_segment, filter, bgr, force, frames, tables, header, ws, out, capacity, sizes, stream):
    """``sg_png_encode_frames`` on ``stream`` (a torch stream): ``filter`` 0..5 (SG_PNG_FILTER_*); ``force`` -1 or a candidate;
    ``_encoder_tensors`` with ``_lib.PNG_TABLE_WORDS`` table words (``sings_amd.png``) and ``png_layout``'s ``ws_bytes``.  Nothing is
    allocated here."""
    _encoder_tensors("png_encode_frames", K, W, H, _lib.PNG_TABLE_WORDS, frames, tables, header, ws, out, capacity, sizes)
    _lib.check(_codec_lib("png").sg_png_encode_frames(int(K), int(W), int(H), int(rows_per_segment), int(filter), int(bool(bgr)), int(force),
                                                      _ptr(frames), _ptr(tables), _ptr(header), int(header.numel()), _ptr(ws), int(ws.numel()),
                                                      _ptr(out), int(capacity), _ptr(sizes), C.c_void_p(stream.cuda_stream)),
               "sg_png_encode_frames")


def unpng_layout(n_streams, max_raw_bytes):
    """``sg_unpng_layout`` -> dict of ``_lib.UNPNG_LAYOUT``: the workspace bytes of ``n_streams`` streams of at most ``max_raw_bytes``
    filtered scanline bytes each, and the bytes of a stream's slot."""
    return _codec_layout("unpng", n_streams, max_raw_bytes)


def unpng_decode(n, streams, table, ws, dst, status, stream):
    """``sg_unpng_decode`` on ``stream`` (a torch stream): ``streams`` uint8, the concatenated zlib streams; ``table`` int64
    [>= n, ``_lib.UNPNG_TABLE_COLS``], whose offsets and lengths are checked against ``streams`` by the caller; ``ws`` uint8,
    ``unpng_layout``'s ``ws_bytes``; ``dst`` uint8 [F,H,W,4]; ``status`` int32 [>= n].  Nothing is allocated here."""
    _codec_tensors("unpng_decode", dst.device, (("streams", streams, torch.uint8, 1), ("table", table, torch.int64, int(n) * _lib.UNPNG_TABLE_COLS),
                                                ("ws", ws, torch.uint8, 1), ("dst", dst, torch.uint8, 1), ("status", status, torch.int32, int(n))))
    if dst.dim() != 4 or dst.shape[3] != 4:
        raise ValueError(f"unpng_decode: dst must be uint8 [F,H,W,4], got {tuple(dst.shape)}")
    F, H, W = (int(v) for v in dst.shape[:3])
    _lib.check(_codec_lib("unpng").sg_unpng_decode(int(n), _ptr(streams), _ptr(table), _ptr(ws), int(ws.numel()), _ptr(dst), F, H, W,
                                                   _ptr(status), C.c_void_p(stream.cuda_stream)), "sg_unpng_decode")


# ---- the soft silhouette and the pose update (csrc/sg_silhouette.hip)
def _sil_lib():
    lib = _lib.load()
    if not _lib.HAS_SILHOUETTE:
        raise RuntimeError("the loaded library predates include/sings_silhouette.h (no fallback): rebuild it")
    return lib


def sil_layout(K, V, F, H, W, capacity):
    """``sg_sil_layout`` (host only): dict piece -> byte offset, ``bytes`` the total.  ValueError where the library refuses."""
    out = (C.c_size_t * len(_lib.SIL_LAYOUT))()
    if _sil_lib().sg_sil_layout(int(K), int(V), int(F), int(H), int(W), int(capacity), out) != 0:
        raise ValueError(_lib.load().sg_last_error().decode())
    return dict(zip(_lib.SIL_LAYOUT, (int(x) for x in out)))


def _sil_dims(verts, faces, what):
    dev = verts.device if torch.is_tensor(verts) else None
    verts = _mesh_arg(verts, what + ": verts_cam", torch.float32, dev)
    faces = _mesh_arg(faces, what + ": faces", torch.int32, dev, (3,))
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError(f"{what}: verts_cam must be [K,V,3], got {tuple(verts.shape)}")
    return dev, int(verts.shape[0]), int(verts.shape[1]), int(faces.shape[0])


def sil_forward(verts, faces, intrinsics, H, W, sigma, capacity, ws, alpha, counts=None):
    """``sg_sil_forward`` on torch's current stream: ``verts`` [K,V,3] fp32, ``faces`` [F,3] int32, ``ws`` the bytes of ``sil_layout``
    (uint8), ``alpha`` [K,H,W] fp32 and ``counts`` [K] int32 | None are written."""
    dev, K, V, F = _sil_dims(verts, faces, "sil_forward")
    _mesh_arg(ws, "sil_forward: ws", torch.uint8, dev); _mesh_arg(alpha, "sil_forward: alpha", torch.float32, dev)
    if counts is not None:
        _mesh_arg(counts, "sil_forward: counts", torch.int32, dev)
    if tuple(alpha.shape) != (K, H, W) or (counts is not None and tuple(counts.shape) != (K,)):
        raise ValueError(f"sil_forward: alpha must be [{K},{H},{W}] and counts [{K}]")
    if ws.numel() < sil_layout(K, V, F, H, W, capacity)["bytes"]:
        raise ValueError(f"sil_forward: a workspace of {ws.numel()} bytes is too small")
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    with torch.cuda.device(dev):
        _lib.check(_sil_lib().sg_sil_forward(K, V, F, int(H), int(W), fx, fy, cx, cy, float(sigma), int(capacity), _ptr(verts), _ptr(faces),
                                             _ptr(ws), _ptr(alpha), _ptr(counts), _stream(dev)), "sg_sil_forward")


def sil_backward(verts, faces, intrinsics, H, W, sigma, capacity, ws, dalpha, row_ptr, corner, dverts):
    """``sg_sil_backward`` on torch's current stream, after ``sil_forward`` with the same arguments on the same ``ws``:
    ``dalpha`` [K,H,W], ``row_ptr`` [V+1] / ``corner`` [3F] int32 -> ``dverts`` [K,V,3] is written."""
    dev, K, V, F = _sil_dims(verts, faces, "sil_backward")
    _mesh_arg(ws, "sil_backward: ws", torch.uint8, dev); _mesh_arg(dalpha, "sil_backward: dalpha", torch.float32, dev)
    _mesh_arg(row_ptr, "sil_backward: row_ptr", torch.int32, dev); _mesh_arg(corner, "sil_backward: corner", torch.int32, dev)
    _mesh_arg(dverts, "sil_backward: dverts", torch.float32, dev)
    if tuple(dalpha.shape) != (K, H, W) or tuple(dverts.shape) != (K, V, 3) or tuple(row_ptr.shape) != (V + 1,) or corner.numel() > 3 * F:
        raise ValueError(f"sil_backward: dalpha must be [{K},{H},{W}], dverts [{K},{V},3], row_ptr [{V + 1}], corner at most [{3 * F}]")
    if ws.numel() < sil_layout(K, V, F, H, W, capacity)["bytes"]:
        raise ValueError(f"sil_backward: a workspace of {ws.numel()} bytes is too small")
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    with torch.cuda.device(dev):
        _lib.check(_sil_lib().sg_sil_backward(K, V, F, int(H), int(W), fx, fy, cx, cy, float(sigma), int(capacity), _ptr(verts), _ptr(faces),
                                              _ptr(ws), _ptr(dalpha), _ptr(row_ptr), _ptr(corner), _ptr(dverts), _stream(dev)),
                   "sg_sil_backward")


def sil_pose_update(lr, pose, grad, m, v, grad_mask, lo, hi, step, terms=None, table=None):
    """``sg_sil_pose_update`` on torch's current stream: ``pose`` / ``grad`` / ``m`` / ``v`` [K,72] fp32, ``grad_mask`` / ``lo`` / ``hi``
    [72], ``step`` [1] int32; ``terms`` [K,2] with ``table`` [iterations,K,2], or neither."""
    dev = pose.device if torch.is_tensor(pose) else None
    pose = _mesh_arg(pose, "sil_pose_update: pose", torch.float32, dev, (_lib.SIL_POSE,))
    K = int(pose.shape[0])
    for name, t in (("grad", grad), ("m", m), ("v", v)):
        if tuple(_mesh_arg(t, "sil_pose_update: " + name, torch.float32, dev).shape) != (K, _lib.SIL_POSE):
            raise ValueError(f"sil_pose_update: {name} must be [{K},{_lib.SIL_POSE}], got {tuple(t.shape)}")
    for name, t in (("grad_mask", grad_mask), ("lo", lo), ("hi", hi)):
        if tuple(_mesh_arg(t, "sil_pose_update: " + name, torch.float32, dev).shape) != (_lib.SIL_POSE,):
            raise ValueError(f"sil_pose_update: {name} must be [{_lib.SIL_POSE}], got {tuple(t.shape)}")
    if tuple(_mesh_arg(step, "sil_pose_update: step", torch.int32, dev).shape) != (1,):
        raise ValueError("sil_pose_update: step must be [1]")
    iters = 0
    if (terms is None) != (table is None):
        raise ValueError("sil_pose_update: terms and table come together")
    if terms is not None:
        _mesh_arg(terms, "sil_pose_update: terms", torch.float32, dev); _mesh_arg(table, "sil_pose_update: table", torch.float32, dev)
        iters = int(table.shape[0])
        if tuple(terms.shape) != (K, 2) or tuple(table.shape) != (iters, K, 2):
            raise ValueError(f"sil_pose_update: terms must be [{K},2] and table [iterations,{K},2]")
    with torch.cuda.device(dev):
        _lib.check(_sil_lib().sg_sil_pose_update(K, float(lr), _ptr(pose), _ptr(grad), _ptr(m), _ptr(v), _ptr(grad_mask), _ptr(lo), _ptr(hi),
                                                 _ptr(step), _ptr(terms), _ptr(table), iters, _stream(dev)), "sg_sil_pose_update")
