"""The start of a SinGS training run: a trainable avatar from a body mesh -- what the reference does in ``SinGS.initialize`` and
``SinGS.init_attrs`` (sings_hybrid.py:608-741, called from gs_trainer.py:151-153) before its first training step.

    initial_attributes        sings_hybrid.py:674-741   the values the decoders are pre-fitted to, from the mesh, on the device
    attribute_mse             :645-656                  the pre-fit's loss: up to six MSE terms, value and gradient in one march
    AttrMSEEngine                                       the same, pre-allocated, for a captured loop
    PlateauRule / DevicePlateau   :621, :665            ``ReduceLROnPlateau`` restated in Python / with its state in device memory
    fit_initial_attributes    :608-671                  the 500-step pre-fit: ``FusedAdam``, no host read per step, replayed from a graph
    from_mesh                                           mesh -> (``AvatarStep``, ``MeshState``, targets): the three-call sequence of
                                                        INTEGRATION.md 13
    from_body                                           the same from a ``body_model.BodyModel`` and betas: the canonical-pose mesh is
                                                        made here too

Kernels: csrc/sg_init.hip.  There is no CPU fallback: host tensors raise.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _marshal
from . import rotations as _rot
from .grad_arena import set_gradient_arena
from .optim import FusedAdam
from .photo_loss import _is_unit
from .topology import MeshState
from .train_step import AvatarStep, capture_step

ATTR_KEYS = ("xyz_offsets", "scales", "scales_aux", "rot6d_canon", "shs", "opacity")      # canon_forward's keys (:316-328)
ATTR_WIDTHS = _marshal.ATTR_MSE_WIDTHS
GROUPS = ("xyz", "triplane", "geometry", "appearance")                                   # the trainer's group names


# ---- initial values -------------------------------------------------------------------------------------------------------------------
def initial_attributes(verts, faces, edges, init_scale_multiplier=0.8, thickness_factor=1.0, init_opacity=0.8, sh_coeffs=16):
    """``SinGS.initialize`` (sings_hybrid.py:674-741) on the device -> a dict with the reference's keys ``xyz_offsets`` [V,3], ``scales``
    [V,3], ``scales_aux`` [V,3], ``rot6d_canon`` [V,6], ``shs`` [V,sh_coeffs,3], ``opacity`` [V,1], and what the reference computes on
    the way and keeps: ``normals`` [V,3], ``rotq`` [V,4] (real part first), ``first`` / ``second`` [V] int32 (below).

    ``verts`` [V,3] fp32: the canonical-pose vertices; ``faces`` [F,3], ``edges`` [E,2]: int32 as ``MeshState`` holds them (edges: the
    unique sorted rows a < b in lexicographic order).  GPU tensors only.  A handful of launches and ONE host read, for the error flags.

    Scales -- the reference's rule AS WRITTEN (:687-702), not as probably intended.  For vertex v the loop selects the rows of the edge
    list that contain v and then indexes ``self._edges[selected_edges][0]`` and ``[1]``: those are the first two such ROWS, in list
    order, (a0, b0) and (a1, b1) -- not the endpoints of one edge.  ``t_pose_verts[row0] - t_pose_verts[row1]`` is therefore the pair of
    differences x[a0] - x[a1], x[b0] - x[b1], and

        len = init_scale_multiplier * max(|x[a0] - x[a1]|, |x[b0] - x[b1]|)

    (one of the two is usually 0: v itself sits in the same column of both rows).  This is NOT "the longest incident edge": it is the
    distance between two neighbours of v, or one edge, depending on where v stands in the two rows.  All three components of the
    log-scale are log(len), the last is multiplied by ``thickness_factor`` -- a factor on the LOGARITHM --, ``scales = exp(.)``,
    ``scales_aux = log(exp(scales) - 1)``.  ``first`` / ``second`` are the two row indices.

    Normals -- the reference takes ``trimesh.Trimesh(...).vertex_normals`` on the host (:704-705).  Here: the normalised sum over a
    vertex' faces of the unit face normal weighted by the corner angle at the vertex, trimesh's published default for a mesh without
    stored normals.  trimesh is not a dependency and the reference pins no version: parity is UNPINNED -- the published definition,
    checked against an fp64 restatement, and no more than that.  The sum is 64-bit fixed point with integer atomics: bit-reproducible.

    Rotation -- ``torch_rotation_matrix_from_vectors((0,0,1), n)`` (rotations.py:606-627), then ``matrix_to_rotation_6d`` and
    ``matrix_to_quaternion`` (``sings_amd.rotations``).

    The rest: zero offsets, ``shs`` 0.5 in the DC row and zero elsewhere, ``opacity = init_opacity``.

    Errors: a vertex with fewer than two incident edges (the reference fails at ``[1]``) and an edge row that is not
    ``0 <= a < b < V`` are a ValueError, a face corner outside [0, V) an IndexError; all three are found on the device (a bad row is
    skipped, never dereferenced) and reported after the one host read.

    Deviations: (1) the factor ``(1 - c) / s^2`` of the rotation, 0 / 0 in fp32 for n = +z and cancelling badly near it, is evaluated
    as ``1 / (1 + c)`` -- the same number for unit vectors; n = +z gives the identity; (2) at n = -z, where the reference is
    non-finite, the result is the half-turn about x, diag(1, -1, -1); (3) the arithmetic is fp64 from the fp32 inputs, rounded once
    (the reference's is fp32); (4) a vertex no non-degenerate face holds has a zero normal and the identity rotation."""
    if not torch.is_tensor(verts) or not verts.is_cuda:
        raise RuntimeError("sings_amd.avatar_init: verts must be a GPU tensor (no CPU fallback)")
    for name, t, w in (("faces", faces, 3), ("edges", edges, 2)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"sings_amd.avatar_init: {name} must be a GPU tensor (no CPU fallback)")
        if t.dim() != 2 or t.shape[1] != w or t.dtype != torch.int32:
            raise ValueError(f"sings_amd.avatar_init: {name} must be an [n,{w}] int32 tensor (as MeshState holds it)")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32 or verts.shape[0] < 1:
        raise ValueError("sings_amd.avatar_init: verts must be [V,3] float32, V >= 1")
    dev, V = verts.device, int(verts.shape[0])
    out, info = _marshal.init_attributes(verts.detach().contiguous(), faces.contiguous(), edges.contiguous(), init_scale_multiplier,
                                         thickness_factor)
    rotmat = out.pop("rotmat")
    with torch.cuda.device(dev):
        out["rot6d_canon"] = _rot.matrix_to_rotation_6d(rotmat)
        out["rotq"] = _rot.matrix_to_quaternion(rotmat)
        out["xyz_offsets"] = torch.zeros((V, 3), dtype=torch.float32, device=dev)
        shs = torch.zeros((V, int(sh_coeffs), 3), dtype=torch.float32, device=dev)
        shs[:, 0, :] = 0.5
        out["shs"] = shs
        out["opacity"] = torch.full((V, 1), float(init_opacity), dtype=torch.float32, device=dev)
    bad_edge, lonely, bad_face, _ = info.tolist()                    # the one host read
    if bad_edge:
        raise ValueError(f"initial_attributes: an edge is not a row 0 <= a < b < {V}")
    if bad_face:
        raise IndexError(f"initial_attributes: a face indexes a vertex outside [0, {V})")
    if lonely:
        raise ValueError("initial_attributes: a vertex has fewer than two incident edges (the scale rule needs two rows of the edge list)")
    return out


# ---- the pre-fit's loss -----------------------------------------------------------------------------------------------------------------
def _flat_rows(t, width, name, n=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"sings_amd.avatar_init: {name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() < 1 or t.numel() != t.shape[0] * width or (n is not None and t.shape[0] != n):
        raise ValueError(f"sings_amd.avatar_init: {name} must be float32 with {'N' if n is None else n} rows of {width} values, "
                         f"got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


class _AttrMSE(torch.autograd.Function):
    """(out_0, tgt_0, ..., out_5, tgt_5), None for an absent pair -> six 0-dim terms (zeros for absent pairs).  The forward computes
    the gradients for unit upstream weights in the same march; the backward multiplies each by its upstream scalar (or hands it over
    as it is for a registered unit scalar, ``photo_loss.register_unit_scalar``)."""

    @staticmethod
    def forward(ctx, *pairs):
        outs, tgts = list(pairs[0::2]), list(pairs[1::2])
        first = next(o for o in outs if o is not None)
        dev, N = first.device, int(first.shape[0])
        need = [o is not None and ctx.needs_input_grad[2 * k] for k, o in enumerate(outs)]
        with torch.cuda.device(dev):
            ws = torch.empty(_marshal.attr_mse_ws_bytes(), dtype=torch.uint8, device=dev)
            terms = torch.empty(8, dtype=torch.float32, device=dev)
            grads = [torch.empty_like(o) if nd else None for o, nd in zip(outs, need)]
            _marshal.attr_mse(N, outs, tgts, grads if any(need) else None, ws, terms)
        ctx.unit = grads
        ctx.set_materialize_grads(False)
        return tuple(terms[k] for k in range(6))

    @staticmethod
    def backward(ctx, *gs):
        unit, ctx.unit = ctx.unit, None
        res = []
        for u, g in zip(unit, gs):
            if u is None or g is None:
                res += [None, None]
            else:
                res += [u if _is_unit(g) else u * g.reshape(()).float(), None]
        return tuple(res)


def attribute_mse(outputs, targets):
    """The loss of ``init_attrs`` (sings_hybrid.py:645-656): for every key of ``targets`` that ``outputs`` holds (and is not None there:
    ``rot6d_canon`` of an isotropic model is skipped, :647) ``loss_<key> = mean((outputs[key] - targets[key])^2)`` -> the
    reference's ``loss_dict``; ``sum(loss_dict.values())`` is its loss.  ONE march over all pairs computes values and, for outputs
    that require grad, gradients (``sg_attr_mse``); deterministic.  A shape mismatch is a ValueError (the reference prints and
    skips the key)."""
    pairs, present = [], []
    n = None
    for key, w in zip(ATTR_KEYS, ATTR_WIDTHS):
        o, t = outputs.get(key), targets.get(key)
        if o is None or t is None:
            pairs += [None, None]
            continue
        o = _flat_rows(o, w, f"outputs[{key!r}]", n)
        n = int(o.shape[0])
        pairs += [o, _flat_rows(t.detach(), w, f"targets[{key!r}]", n)]
        present.append(key)
    if not present:
        raise ValueError("attribute_mse: outputs and targets share no key of " + ", ".join(ATTR_KEYS))
    terms = _AttrMSE.apply(*pairs)
    return {"loss_" + key: terms[ATTR_KEYS.index(key)] for key in present}


class AttrMSEEngine:
    """``sg_attr_mse`` pre-allocated, for a captured loop (as ``photo_loss.PhotoLossEngine``; the render engines' shared base is
    sized by pixels and pair capacities and does not fit): no allocation, no synchronisation per call.  ``keys``: the pairs that are
    present.  ``__call__(outputs, targets)`` (dicts of contiguous fp32 GPU tensors with N rows) fills ``terms`` (8 floats: the six
    terms in ``ATTR_KEYS``' order, their sum at [6]) and ``grads[key]`` = d sum / d outputs[key]."""

    def __init__(self, N, device, keys=ATTR_KEYS):
        unknown = [k for k in keys if k not in ATTR_KEYS]
        if unknown or not keys:
            raise ValueError(f"AttrMSEEngine: keys must be a non-empty subset of {ATTR_KEYS}")
        self.N, self.dev, self.keys = int(N), torch.device(device), tuple(k for k in ATTR_KEYS if k in keys)
        if self.dev.type != "cuda":
            raise RuntimeError("AttrMSEEngine: the device must be the GPU (no CPU fallback)")
        self.ws = torch.empty(_marshal.attr_mse_ws_bytes(), dtype=torch.uint8, device=self.dev)
        self.terms = torch.zeros(8, dtype=torch.float32, device=self.dev)
        self.grads = {k: torch.empty((self.N, w), dtype=torch.float32, device=self.dev)
                      for k, w in zip(ATTR_KEYS, ATTR_WIDTHS) if k in self.keys}

    @property
    def loss(self):
        return self.terms[6:7]

    def __call__(self, outputs, targets):
        row = lambda d: [d[k] if k in self.keys else None for k in ATTR_KEYS]
        _marshal.attr_mse(self.N, row(outputs), row(targets), row(self.grads), self.ws, self.terms)
        return self.grads


# ---- ReduceLROnPlateau ------------------------------------------------------------------------------------------------------------------
class PlateauRule:
    """``torch.optim.lr_scheduler.ReduceLROnPlateau(optim, patience, factor)`` -- mode min, relative threshold 1e-4, cooldown 0, min_lr
    0, eps 1e-8: the settings of ``init_attrs`` (:621) -- restated in plain Python, the state machine ``sg_plateau_step`` runs on the
    device: ``step(loss)`` digests one loss; ``lrs`` = base rate x ``multipliers``, per group."""

    def __init__(self, base_lrs, patience=100, factor=0.5, threshold=1e-4, eps=1e-8):
        if not 0.0 < factor < 1.0:
            raise ValueError("PlateauRule: 0 < factor < 1")
        self.base = [float(x) for x in base_lrs]
        self.patience, self.factor, self.threshold, self.eps = int(patience), float(factor), float(threshold), float(eps)
        self.best, self.bad, self.multipliers = math.inf, 0, [1.0] * len(self.base)

    @property
    def lrs(self):
        return [b * m for b, m in zip(self.base, self.multipliers)]

    def step(self, loss):
        loss = float(loss)
        if loss < self.best * (1.0 - self.threshold):
            self.best, self.bad = loss, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            for g, (b, m) in enumerate(zip(self.base, self.multipliers)):
                old = b * m
                if old - old * self.factor > self.eps:               # torch's rule, per group, on the rate itself
                    self.multipliers[g] = m * self.factor
            self.bad = 0
        return self.lrs


class DevicePlateau:
    """``PlateauRule`` with its state in device memory (``sg_plateau_step``): ``begin_step(hyper, loss, terms)`` is ONE launch that
    first digests the previous step's loss -- read from the device scalar ``loss`` -- and then multiplies column 5 of every group's
    row of ``hyper`` (``FusedAdam.hyper``, rewritten from the base rates by ``advance()`` before every step) by the group's
    multiplier: the loss of step i decides the rate of step i + 1, and nothing is read on the host.  ``finish(loss, terms)`` digests
    the last step's loss.  With ``log_steps`` > 0 row i of the log takes step i's ``n_terms`` floats at ``terms`` and the
    multipliers the step ran with.  ``read()`` is the one host read: (multipliers now, log [steps, n_terms], multipliers per step)."""

    def __init__(self, base_lrs, device, patience=100, factor=0.5, threshold=1e-4, eps=1e-8, log_steps=0, n_terms=0):
        rule = PlateauRule(base_lrs, patience, factor, threshold, eps)                # (validates)
        self.G, self.patience, self.log_steps, self.n_terms = len(rule.base), rule.patience, int(log_steps), int(n_terms)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("DevicePlateau: the device must be the GPU (no CPU fallback)")
        self._settings = (C.c_double * 3)(rule.factor, rule.threshold, rule.eps)
        G = self.G
        host = np.zeros(4 + 2 * G + self.log_steps * (self.n_terms + G), np.float64)
        host[0] = np.inf
        host[4:4 + G] = 1.0
        host[4 + G:4 + 2 * G] = rule.base
        self.buf = torch.from_numpy(host).to(self.dev)               # state and log in ONE buffer: one read at the end
        self.state = self.buf[:4 + 2 * G]
        self.log = self.buf[4 + 2 * G:] if self.log_steps else None

    def _launch(self, begin, hyper, loss, terms):
        _marshal.plateau_step(self.G, begin, self.patience, self._settings, loss, self.state, hyper, terms, self.n_terms if self.log is not None
                              else 0, self.log, self.log_steps)

    def begin_step(self, hyper, loss, terms=None):
        self._launch(True, hyper, loss, terms)

    def finish(self, loss, terms=None):
        self._launch(False, None, loss, terms)

    def read(self):
        host = self.buf.cpu().numpy()
        G = self.G
        mult = host[4:4 + G].copy()
        rows = host[4 + 2 * G:].reshape(self.log_steps, self.n_terms + G)
        return mult, rows[:, :self.n_terms].copy(), rows[:, self.n_terms:].copy()


# ---- the fit ----------------------------------------------------------------------------------------------------------------------------
def _fit_groups(module, lrs):
    missing = [n for n in GROUPS if n not in lrs]
    if missing:
        raise ValueError(f"fit_initial_attributes: lrs has no entry for the groups {missing}")
    return [{"params": [module.xyz], "lr": float(lrs["xyz"]), "name": "xyz"},
            {"params": list(module.triplane.parameters()), "lr": float(lrs["triplane"]), "name": "triplane"},
            {"params": list(module.geometry_dec.parameters()), "lr": float(lrs["geometry"]), "name": "geometry"},
            {"params": list(module.appearance_dec.parameters()), "lr": float(lrs["appearance"]), "name": "appearance"}]


def fit_initial_attributes(module, targets, lrs, init_steps=500, patience=100, factor=0.5, use_graph=True):
    """``SinGS.init_attrs`` (sings_hybrid.py:608-671): ``init_steps`` Adam steps that fit the decoded attributes of ``module`` (an
    ``AvatarStep``) to ``targets`` (``initial_attributes``), with ``ReduceLROnPlateau(patience, factor)`` on the summed loss.  ``lrs``:
    the trainer's group names ``xyz``, ``triplane``, ``geometry``, ``appearance`` (the reference: ``position_init * smpl_spatial``,
    ``vembed``, ``geometry``, ``appearance`` of ``cfg.human.lr``).  Leaves ``module`` fitted and returns

        {"keys": ["loss_<name>", ..., "loss"], "losses": float32 array [init_steps, len(keys)], "lr_steps": float64 array
         [init_steps, 4] (the rate every step ran with), "lrs": {group: rate after the last step}}

    One step: gradients cleared; the plateau launch (``DevicePlateau``); ``module.decode()`` (``decode_attributes`` with the module's
    ``thickness_factor`` and ``scaling_multiplier``); ``sg_attr_mse`` against the targets on the keys of ``canon_forward`` (:316-328)
    that the model produces; backward; ``FusedAdam`` over ALL four groups.  That includes the anchors: ``xyz`` receives a gradient
    through the tri-plane lookup and the reference lets it move during the pre-fit; so does this.  With ``use_graph`` the step is
    captured once (``capture_step``) and replayed: ``FusedAdam.advance()`` is the only host work per step.  The per-step loss terms
    stay on the device and are read ONCE, after the last step.

    The capture's warm-up runs are not steps: parameters, moments, step counts and the scheduler's state are put back.  The gradient
    arena is released at the end, and the optimiser of the fit is dropped: build the ``AvatarTrainer`` afterwards, it starts with
    fresh moments, as the reference's second ``setup_optimizer`` does (gs_trainer.py:153).  A target whose shape differs from the
    model's output is a ValueError (the reference prints and skips it)."""
    if not isinstance(module, AvatarStep) or not module.xyz.is_cuda:
        raise RuntimeError("fit_initial_attributes: module must be an AvatarStep on the GPU (no CPU fallback)")
    dev, N, steps = module.xyz.device, int(module.xyz.shape[0]), int(init_steps)
    if steps < 1:
        raise ValueError("fit_initial_attributes: init_steps >= 1")
    with torch.cuda.device(dev):
        with torch.no_grad():
            probe = module.decode()
        keys = [k for k in ATTR_KEYS if targets.get(k) is not None and probe.get(k) is not None]
        if not keys:
            raise ValueError("fit_initial_attributes: the targets and the decoded attributes share no key")
        tg = {}
        for k in keys:
            if tuple(targets[k].shape) != tuple(probe[k].shape):
                raise ValueError(f"fit_initial_attributes: targets[{k!r}] is {tuple(targets[k].shape)}, the model gives {tuple(probe[k].shape)}")
            tg[k] = _flat_rows(targets[k].detach(), ATTR_WIDTHS[ATTR_KEYS.index(k)], f"targets[{k!r}]", N).clone()
        del probe
        groups = _fit_groups(module, lrs)
        opt = FusedAdam(groups)
        params = [p for g in opt.param_groups for p in g["params"]]
        flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
        try:
            opt.bind_arena(flat, set_gradient_arena(params, flat))
            engine = AttrMSEEngine(N, dev, keys)
            plateau = DevicePlateau([g["lr"] for g in groups], dev, patience=patience, factor=factor, log_steps=steps, n_terms=7)

            def body():
                for p in params:
                    p.grad = None
                plateau.begin_step(opt.hyper, engine.loss, engine.terms)
                attrs = module.decode()
                outs = {k: attrs[k].reshape(N, -1).contiguous() for k in keys}
                grads = engine({k: v.detach() for k, v in outs.items()}, tg)
                roots = [k for k in keys if outs[k].requires_grad]
                torch.autograd.backward([outs[k] for k in roots], [grads[k] for k in roots])
                opt.apply()
                return engine.terms

            graph = None
            for _ in range(steps):
                opt.advance()
                if not use_graph:
                    body()
                    continue
                if graph is None:
                    # (the capture's warm-up runs execute the body without being steps: everything they change goes back)
                    live = [p.detach() for p in params] + [opt.exp_avg, opt.exp_avg_sq, plateau.buf]
                    keep, counts = [x.clone() for x in live], list(opt.steps)
                    graph, _ = capture_step(body, warmup=2, device=dev)
                    for dst, src in zip(live, keep):
                        dst.copy_(src)
                    opt.steps[:] = counts
                graph.replay()
            plateau.finish(engine.loss, engine.terms)
            mult, log, mult_steps = plateau.read()                   # the one host read
        finally:
            graph = None
            for p in params:
                p.grad = None
            set_gradient_arena(None, None)
    base = np.array([g["lr"] for g in groups], np.float64)
    cols = [ATTR_KEYS.index(k) for k in keys] + [6]
    return {"keys": ["loss_" + k for k in keys] + ["loss"], "losses": log[:, cols].astype(np.float32), "lr_steps": mult_steps * base,
            "lrs": {g["name"]: float(b * m) for g, b, m in zip(groups, base, mult)}}


def from_mesh(verts, faces, lbs_weights, vertex_label, triplane, geometry_dec, appearance_dec, **init_kwargs):
    """Mesh -> ``(module, mesh, targets)``: ``mesh = MeshState.from_faces(faces, vertex_label)``, ``targets =
    initial_attributes(verts, mesh.faces, mesh.edges, **init_kwargs)`` and ``module = AvatarStep(verts, lbs_weights, ...)`` with the
    same ``thickness_factor`` and ``scaling_multiplier`` ones [V,1] (sings_hybrid.py:677).  Then ``fit_initial_attributes(module,
    targets, lrs)`` and ``AvatarTrainer(module, ..., mesh=mesh)``."""
    if not torch.is_tensor(verts) or not verts.is_cuda:
        raise RuntimeError("sings_amd.avatar_init: verts must be a GPU tensor (no CPU fallback)")
    dev, V = verts.device, int(verts.shape[0])
    mesh = MeshState.from_faces(faces, vertex_label)
    targets = initial_attributes(verts, mesh.faces, mesh.edges, **init_kwargs)
    module = AvatarStep(verts, lbs_weights, triplane, geometry_dec, appearance_dec,
                        thickness_factor=init_kwargs.get("thickness_factor", 1.0),
                        scaling_multiplier=torch.ones((V, 1), dtype=torch.float32, device=dev)).to(dev)
    return module, mesh, targets


def from_body(body, betas, triplane, geometry_dec, appearance_dec, canonical_pose_type="da_pose", **init_kwargs):
    """``body_model.BodyModel`` + betas [B] -> ``(module, mesh, targets, canon)``: ``canon = body.canonical(betas, canonical_pose_type,
    'smplh' for 52 joints, else 'smpl')`` and ``from_mesh(canon['verts'], body.faces, body.lbs_weights, body.vertex_label, ...)``.  ``canon``
    carries what the pose tables take: ``joints_rest`` and ``A_t2cano``."""
    canon = body.canonical(betas, canonical_pose_type, "smplh" if body.num_joints == 52 else "smpl")
    module, mesh, targets = from_mesh(canon["verts"], body.faces, body.lbs_weights, body.vertex_label, triplane, geometry_dec,
                                      appearance_dec, **init_kwargs)
    return module, mesh, targets, canon
