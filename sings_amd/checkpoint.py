"""Checkpoint and resume of a whole ``AvatarTrainer`` run: ONE dict in the layout of the reference's ``SinGS.state_dict()``
(sings_hybrid.py:169-199: the top level is exactly ``export.checkpoint_keys(1)``) plus ONE key, ``"sings_amd"``, with what the reference
does not save and a resumed run needs -- the mesh's faces and edges, the pose tables, the vertices and normals the mesh terms were last
reset with, the appearance decoder's opacity offset (what ``reset_opacity`` leaves behind every change of the set: a plain attribute, in
no ``state_dict()``), the schedules' states, the gate word, the iteration, the decoders' flags, ``density_log``.

    trainer_state_dict(trainer)                  -> the dict; every leaf a CPU tensor, a Python number / bool / str / None, or a list / dict
                                                    of those: ``torch.load(path, weights_only=True)`` reads the file
    load_trainer_state_dict(trainer, sd, strict) make a trainer that was built the usual way (same optional parts, the initial body) the
                                                    saved one.  EVERYTHING is validated before ANYTHING is changed (``validate``: a refusal is a
                                                    ValueError that names the entry, and the trainer is as it was)
    load_reference(trainer, sd, faces=None)      a dict WITHOUT the extra key (the reference's ``save_ckpt``): the model alone
    atomic_save(obj, path)                       a temporary file in the target directory, then ``os.replace``

What is NOT in the file: the frame store, the LPIPS weights, the cameras and ``settings_fn`` -- the caller's; ``last_subdivision`` /
``last_simplification`` -- diagnostics of the last call.  Of the frame store a fingerprint (F, H, W, K, random_bg) is kept and checked.

Nothing here runs inside a training step, and nothing a step executes is changed: this module is host bookkeeping between steps (device
to host copies on save, host to device copies and one ``_rebuild()`` on load).  With ``fp=`` every rank holds the same state and
``trainer_state_dict`` needs no collective: rank 0 saves, every rank loads.

The pure parts -- the schema walk, ``validate``, the optimiser-group mapping, the atomic write -- work on CPU tensors and plain dicts.
"""
import copy
import os
import tempfile
import warnings

import torch

from .export import checkpoint_keys

FORMAT_VERSION = 1
EXTRA_KEY = "sings_amd"
COMPONENTS = ("poses", "mesh", "mesh_terms", "lpips_sampler", "decoder_schedule", "frames", "density_schedule")
MODULE_KEYS = ("triplane", "geometry_dec_0", "appearance_dec_0")
STATS_KEYS = ("xyz_gradient_accum", "denom", "max_radii2D")
# the reference's optimiser groups (sings_hybrid.py:750-771) -> this trainer's
REFERENCE_GROUPS = {"xyz": "xyz", "v_embed": "triplane", "geometry_dec_0": "geometry", "appearance_dec_0": "appearance",
                    "global_orient": "global_orient", "body_pose": "body_pose", "transl": "transl"}


# ---- the schema -------------------------------------------------------------------------------------------------------------------
def to_host(obj):
    """A deep copy with every tensor detached on the CPU, tuples as lists, mappings as plain dicts, 0-dim numpy scalars as Python ones."""
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [to_host(v) for v in obj]
    if hasattr(obj, "item") and getattr(obj, "shape", None) == ():
        return obj.item()
    return obj


def check_leaves(obj, path="checkpoint"):
    """The schema walk: ValueError, with the entry's path, for anything but a CPU tensor, a Python number, bool, str or None, or a
    list / dict (str or int keys) of those."""
    if torch.is_tensor(obj):
        if obj.device.type != "cpu":
            raise ValueError(f"{path}: a tensor on {obj.device} (a checkpoint holds CPU tensors)")
        return
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return
    if type(obj) is dict:
        for k, v in obj.items():
            if not isinstance(k, (str, int)) or isinstance(k, bool):
                raise ValueError(f"{path}: a dict key of type {type(k).__name__}")
            check_leaves(v, f"{path}[{k!r}]")
        return
    if type(obj) is list:
        for i, v in enumerate(obj):
            check_leaves(v, f"{path}[{i}]")
        return
    raise ValueError(f"{path}: a leaf of type {type(obj).__name__} (CPU tensors, numbers, bools, strs, None, lists and dicts only)")


def leaves_equal(a, b, path="checkpoint"):
    """-> None when ``a`` and ``b`` are equal leaf for leaf (tensors: dtype, shape and BITS), else the path of the first difference."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
            return path
        bits = lambda t: t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)
        return None if a.numel() == 0 or torch.equal(bits(a), bits(b)) else path
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)) or list(a.keys()) != list(b.keys()):
            return path
        for k in a:
            bad = leaves_equal(a[k], b[k], f"{path}[{k!r}]")
            if bad:
                return bad
        return None
    if isinstance(a, list) or isinstance(b, list):
        if not (isinstance(a, list) and isinstance(b, list)) or len(a) != len(b):
            return path
        for i, (x, y) in enumerate(zip(a, b)):
            bad = leaves_equal(x, y, f"{path}[{i}]")
            if bad:
                return bad
        return None
    return None if type(a) is type(b) and a == b else path


def atomic_save(obj, path):
    """``torch.save`` into a temporary file of ``path``'s directory, then ``os.replace``: a failure while writing leaves an existing
    ``path`` as it was, and no reader ever sees half a file."""
    check_leaves(obj)
    path = os.fspath(path)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=d)
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def load_file(path, map_location="cpu"):
    return torch.load(path, map_location=map_location, weights_only=True)


# ---- the optimiser's groups -------------------------------------------------------------------------------------------------------
def remap_optimizer(saved, template_groups, rename=None, strict=True):
    """A torch-Adam state dict ``saved`` laid out for the groups ``template_groups`` (the loading optimiser's own
    ``state_dict()["param_groups"]``: names, parameter counts, hyper-parameters) -> (state dict, report).  Groups are matched by NAME
    (``rename``: saved name -> template name; a saved group it does not name is dropped), parameters of a group by position.  The
    result keeps the template's hyper-parameters except ``lr`` / ``betas`` / ``eps``, which the file gives.

    A group of the template that the file lacks, or the reverse: ValueError under ``strict``; otherwise the first starts without a state
    and the second is left out, both named in ``report`` (``missing_groups`` / ``dropped_groups``).  A matched group with another number
    of parameters is a ValueError either way.  Pure: ``saved`` is not written."""
    groups = saved["param_groups"]
    names = [g.get("name", f"group{i}") for i, g in enumerate(groups)]
    if rename is not None:
        names = [rename.get(n) for n in names]
    by_name = {}
    for n, g in zip(names, groups):
        if n is not None:
            if n in by_name:
                raise ValueError(f"optimizer: two groups map to {n!r}")
            by_name[n] = g
    wanted = [g["name"] for g in template_groups]
    report = {"missing_groups": [n for n in wanted if n not in by_name],
              "dropped_groups": [g.get("name", f"group{i}") for i, (n, g) in enumerate(zip(names, groups)) if n is None or n not in wanted]}
    if strict and (report["missing_groups"] or report["dropped_groups"]):
        raise ValueError(f"optimizer: the file's groups {[g.get('name') for g in groups]} do not match the trainer's {wanted}")
    state, out_groups, k = {}, [], 0
    for t in template_groups:
        idx = list(range(k, k + len(t["params"])))
        g = dict(t, params=idx)
        src = by_name.get(t["name"])
        if src is not None:
            if len(src["params"]) != len(idx):
                raise ValueError(f"optimizer: group {t['name']!r} has {len(src['params'])} parameters in the file, {len(idx)} in the trainer")
            for key in ("lr", "betas", "eps"):
                if key in src:
                    g[key] = tuple(src[key]) if key == "betas" else src[key]
            for i, j in zip(idx, src["params"]):
                if j in saved["state"]:
                    state[i] = saved["state"][j]
        out_groups.append(g)
        k += len(idx)
    return {"state": state, "param_groups": out_groups}, report


def _check_optimizer_shapes(opt_sd, shapes, path="optimizer"):
    """``shapes``: the parameters' shapes in the optimiser's order.  Every state entry: ``step`` and two moments of that shape."""
    for i, st in opt_sd["state"].items():
        if not isinstance(i, int) or not 0 <= i < len(shapes):
            raise ValueError(f"{path}['state']: an entry for parameter {i!r} of {len(shapes)}")
        for key in ("exp_avg", "exp_avg_sq"):
            if key not in st or not torch.is_tensor(st[key]) or tuple(st[key].shape) != tuple(shapes[i]):
                got = tuple(st[key].shape) if key in st and torch.is_tensor(st[key]) else None
                raise ValueError(f"{path}['state'][{i}][{key!r}]: shape {got}, the parameter is {tuple(shapes[i])}")
        if "step" not in st:
            raise ValueError(f"{path}['state'][{i}]: no step")
    for g in opt_sd["param_groups"]:
        steps = {int(float(opt_sd["state"][i]["step"])) for i in g["params"] if i in opt_sd["state"]}
        if len(steps) > 1:
            raise ValueError(f"{path}: the parameters of group {g.get('name')!r} are at different steps {sorted(steps)}")


# ---- validation (pure) ------------------------------------------------------------------------------------------------------------
def _shape(t):
    return tuple(t.shape) if torch.is_tensor(t) else None


def _module_shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def validate_model(sd, expect, faces=None, edges=None):
    """The model entries (the reference's keys) against each other and against ``expect`` (``expectations``' ``J`` and ``modules``);
    -> N.  ValueError names the entry."""
    for k in ("active_sh_degree", "xyz", "lbs_weights", "scaling_multiplier") + MODULE_KEYS:
        if k not in sd:
            raise ValueError(f"{k}: missing from the checkpoint")
    deg = sd["active_sh_degree"]
    if isinstance(deg, bool) or not isinstance(deg, int) or not 0 <= deg <= expect["max_sh_degree"]:
        raise ValueError(f"active_sh_degree: {deg!r} is not an int in 0..{expect['max_sh_degree']}")
    xyz = sd["xyz"]
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1 or xyz.dtype != torch.float32:
        raise ValueError(f"xyz: must be a float32 tensor [N,3] with N >= 1, got {_shape(xyz)}")
    N = int(xyz.shape[0])
    if _shape(sd["lbs_weights"]) != (N, expect["J"]):
        raise ValueError(f"lbs_weights: shape {_shape(sd['lbs_weights'])}, expected {(N, expect['J'])} (xyz has {N} rows, the body {expect['J']} joints)")
    sm = sd["scaling_multiplier"]
    if torch.is_tensor(sm):
        if sm.numel() != 1 and _shape(sm) != (N, 1):
            raise ValueError(f"scaling_multiplier: shape {_shape(sm)}, expected a scalar or {(N, 1)}")
    elif sm is not None and (isinstance(sm, bool) or not isinstance(sm, (int, float))):
        raise ValueError(f"scaling_multiplier: a {type(sm).__name__} (None, a number, a scalar or [N,1] tensor)")
    for k, want in (("xyz_gradient_accum", (N, 1)), ("denom", (N, 1)), ("max_radii2D", (N,))):
        if sd.get(k) is not None and _shape(sd[k]) != want:
            raise ValueError(f"{k}: shape {_shape(sd[k])}, expected {want} (xyz has {N} rows)")
    for k in MODULE_KEYS:
        got, want = sd[k], expect["modules"][k]
        if not isinstance(got, dict):
            raise ValueError(f"{k}: must be the module's state_dict()")
        if set(got) != set(want):
            raise ValueError(f"{k}: keys {sorted(set(got) ^ set(want))} are in the file or in the module, not in both")
        for name, shape in want.items():
            if _shape(got[name]) != tuple(shape):
                raise ValueError(f"{k}[{name!r}]: shape {_shape(got[name])}, the module's is {tuple(shape)}")
    has_mesh = sd.get("vertex_label") is not None
    if has_mesh:
        if _shape(sd["vertex_label"]) != (N,):
            raise ValueError(f"vertex_label: shape {_shape(sd['vertex_label'])}, expected {(N,)}")
        if sd.get("level_id") is not None and _shape(sd["level_id"]) != (N,):
            raise ValueError(f"level_id: shape {_shape(sd['level_id'])}, expected {(N,)}")
        mark = sd.get("gs_level_mark")
        if mark is not None and (not isinstance(mark, list) or not mark or int(mark[-1]) != N):
            raise ValueError(f"gs_level_mark: {mark!r} does not end at N = {N}")
    for name, t, width in (("faces", faces, 3), ("edges", edges, 2)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != width or t.dtype.is_floating_point:
            raise ValueError(f"{name}: must be an integer tensor [.,{width}], got {_shape(t)}")
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= N):
            raise ValueError(f"{name}: an index outside [0, {N})")
    return N


def validate(sd, expect, strict=True):
    """A whole checkpoint against ``expect`` (``expectations(trainer)``, or the same dict written by hand) -> the report
    ``{"skipped": [...], "absent": [...], "missing_groups": [...], "dropped_groups": [...], "optimizer": <remapped state dict>}``.
    ``skipped``: components the file has and the trainer lacks; ``absent``: the reverse -- both a ValueError under ``strict``.
    Pure: nothing is written, ``sd`` included."""
    if not isinstance(sd, dict):
        raise ValueError("checkpoint: not a dict")
    if EXTRA_KEY not in sd:
        raise ValueError(f"{EXTRA_KEY}: missing -- a file of the reference's layout loads through checkpoint.load_reference")
    extra = sd[EXTRA_KEY]
    version = extra.get("version") if isinstance(extra, dict) else None
    if isinstance(version, bool) or not isinstance(version, int) or not 1 <= version <= FORMAT_VERSION:
        raise ValueError(f"{EXTRA_KEY}['version']: {version!r}; this build reads versions 1..{FORMAT_VERSION}")
    want_keys = set(checkpoint_keys(1)) | {EXTRA_KEY}
    if set(sd) != want_keys:
        raise ValueError(f"checkpoint: keys {sorted(set(sd) ^ want_keys)} are in the file or in the layout, not in both")
    for k in ("iteration", "opt_geo", "opt_app", "l2_keys", "components", "density_log", "gate", "store"):
        if k not in extra:
            raise ValueError(f"{EXTRA_KEY}[{k!r}]: missing")
    comp = extra["components"]
    if not isinstance(comp, dict) or set(comp) != set(COMPONENTS):
        raise ValueError(f"{EXTRA_KEY}['components']: must name exactly {list(COMPONENTS)}")
    skipped = [c for c in COMPONENTS if comp[c] and not expect["components"][c]]
    absent = [c for c in COMPONENTS if expect["components"][c] and not comp[c]]
    if strict and (skipped or absent):
        raise ValueError(f"{EXTRA_KEY}['components']: the file has {skipped} that the trainer lacks, the trainer {absent} that the file "
                         "lacks (strict=False loads what both have)")
    both = {c: bool(comp[c] and expect["components"][c]) for c in COMPONENTS}
    if isinstance(extra["iteration"], bool) or not isinstance(extra["iteration"], int) or extra["iteration"] < 0:
        raise ValueError(f"{EXTRA_KEY}['iteration']: {extra['iteration']!r}")
    if not isinstance(extra["l2_keys"], list) or not all(isinstance(k, str) for k in extra["l2_keys"]):
        raise ValueError(f"{EXTRA_KEY}['l2_keys']: a list of attribute names")
    mesh = extra.get("mesh") if both["mesh"] else None
    if both["mesh"] and (not isinstance(mesh, dict) or "faces" not in mesh or "edges" not in mesh or sd.get("vertex_label") is None):
        raise ValueError(f"{EXTRA_KEY}['mesh']: faces, edges and the top-level vertex_label are needed")
    N = validate_model(sd, expect, faces=None if mesh is None else mesh["faces"], edges=None if mesh is None else mesh["edges"])
    for k in STATS_KEYS:
        if sd.get(k) is None:
            raise ValueError(f"{k}: missing from the checkpoint")
    offset = extra.get("opacity_offset")
    if offset is not None and _shape(offset) != (N, 1):
        raise ValueError(f"{EXTRA_KEY}['opacity_offset']: shape {_shape(offset)}, expected {(N, 1)} or None")
    if expect["components"]["mesh"] and not comp["mesh"] and expect["mesh_verts"] != N:
        raise ValueError(f"xyz: {N} rows, the trainer's mesh (which the file does not replace) has {expect['mesh_verts']} vertices")
    if both["frames"]:
        if extra["store"] != expect["store"]:
            raise ValueError(f"{EXTRA_KEY}['store']: the run was saved with {extra['store']}, the trainer's frame store is {expect['store']}")
    for c in ("frames", "lpips_sampler", "density_schedule"):
        if both[c] and not isinstance(extra.get(c), dict):
            raise ValueError(f"{EXTRA_KEY}[{c!r}]: the component's state_dict() is missing")
    for c, keys in (("frames", ("seed", "counter")), ("lpips_sampler", ("seed", "counter")), ("density_schedule", ("densify_interval", "last_t"))):
        if both[c] and not all(k in extra[c] for k in keys):
            raise ValueError(f"{EXTRA_KEY}[{c!r}]: needs {list(keys)}")
    if both["poses"]:
        tables = extra.get("poses")
        if not isinstance(tables, dict) or set(tables) != set(expect["poses"]):
            raise ValueError(f"{EXTRA_KEY}['poses']: must be PoseTable.state_dict() with the keys {sorted(expect['poses'])}")
        for name, shape in expect["poses"].items():
            if _shape(tables[name]) != tuple(shape):
                what = "rows" if _shape(tables[name]) is not None and _shape(tables[name])[1:] == tuple(shape)[1:] else "shape"
                raise ValueError(f"{EXTRA_KEY}['poses'][{name!r}]: {what} {_shape(tables[name])}, the trainer's table is {tuple(shape)}")
    if both["mesh_terms"]:
        mt = extra.get("mesh_terms")
        if not isinstance(mt, dict) or _shape(mt.get("verts")) != (N, 3) or _shape(mt.get("normals")) != (N, 3):
            raise ValueError(f"{EXTRA_KEY}['mesh_terms']: verts and normals must be {(N, 3)}")
    if both["density_schedule"] and (isinstance(extra["gate"], bool) or not isinstance(extra["gate"], int)):
        raise ValueError(f"{EXTRA_KEY}['gate']: {extra['gate']!r} is not the gate's word")
    log = extra["density_log"]
    if not isinstance(log, list) or not all(isinstance(e, dict) and set(e) == {"t", "mode", "n_old", "n_new", "skipped"} for e in log):
        raise ValueError(f"{EXTRA_KEY}['density_log']: a list of {{t, mode, n_old, n_new, skipped}} records")
    # the optimiser: the file's groups in the trainer's layout (the pose groups come and go with `poses` under strict=False)
    if not isinstance(sd["optimizer"], dict) or "state" not in sd["optimizer"] or "param_groups" not in sd["optimizer"]:
        raise ValueError("optimizer: must be a torch-Adam state dict (state, param_groups)")
    opt, rep = remap_optimizer(sd["optimizer"], expect["opt_groups"], strict=strict)
    shapes = [((N,) + tuple(s[1:]) if g["name"] == "xyz" else tuple(s)) for g, ss in zip(expect["opt_groups"], expect["opt_shapes"]) for s in ss]
    _check_optimizer_shapes(opt, shapes)
    return dict(skipped=skipped, absent=absent, optimizer=opt, N=N, **rep)


# ---- what a trainer expects -------------------------------------------------------------------------------------------------------
def store_fingerprint(feed):
    return None if feed is None else {"F": feed.store.F, "H": feed.store.H, "W": feed.store.W, "K": feed.K, "random_bg": feed.random_bg}


def _template_groups(trainer):
    groups, k = [], 0
    for g in trainer.opt.param_groups:
        out = {key: val for key, val in g.items() if key != "params"}
        out["params"] = list(range(k, k + len(g["params"])))
        k += len(g["params"])
        groups.append(out)
    return groups


def expectations(trainer):
    """What ``validate`` holds a file against, read off a trainer: plain Python, no device read."""
    m = trainer.m
    return {"components": {c: getattr(trainer, c) is not None for c in COMPONENTS},
            "store": store_fingerprint(trainer.frames),
            "J": int(m.lbs_weights.shape[1]), "max_sh_degree": trainer.max_sh_degree,
            "modules": {"triplane": _module_shapes(m.triplane), "geometry_dec_0": _module_shapes(m.geometry_dec),
                        "appearance_dec_0": _module_shapes(m.appearance_dec)},
            "poses": None if trainer.poses is None else _module_shapes(trainer.poses),
            "mesh_verts": None if trainer.mesh is None else trainer.mesh.num_verts,
            "opt_groups": _template_groups(trainer),
            "opt_shapes": [[tuple(p.shape) for p in g["params"]] for g in trainer.opt.param_groups]}


# ---- save -------------------------------------------------------------------------------------------------------------------------
def trainer_state_dict(trainer, spatial_lr_scale=None, betas=None):
    """The checkpoint of ``trainer`` as it stands between two steps (module docstring).  ``spatial_lr_scale`` / ``betas``: the
    reference's entries of those names, the caller's, passed through.  Reads the device (it synchronises); no collective."""
    m = trainer.m
    sd = {"active_sh_degree": int(trainer.sh_degree), "optimizer": trainer.opt.state_dict(), "spatial_lr_scale": spatial_lr_scale,
          "betas": betas}
    sd.update(m.checkpoint_entries())
    opacity_offset = sd.pop("opacity_offset")                    # (the module names it; it is not one of the reference's keys)
    sd.update(trainer.mesh.checkpoint_entries() if trainer.mesh is not None else {k: None for k in ("vertex_label", "level_id", "gs_level_mark")})
    part = lambda obj: None if obj is None else obj.state_dict()
    sd[EXTRA_KEY] = {
        "version": FORMAT_VERSION, "iteration": int(trainer.iteration), "opt_geo": bool(m.opt_geo), "opt_app": bool(m.opt_app),
        "l2_keys": list(m.l2_keys), "optimizer_kind": "fused" if trainer.fused else "torch", "opacity_offset": opacity_offset,
        "components": {c: getattr(trainer, c) is not None for c in COMPONENTS},
        "mesh": None if trainer.mesh is None else {k: v for k, v in trainer.mesh.state_dict().items() if k in ("faces", "edges")},
        "poses": None if trainer.poses is None else dict(trainer.poses.state_dict()),
        "mesh_terms": part(trainer.mesh_terms), "density_schedule": part(trainer.density_schedule), "frames": part(trainer.frames),
        "lpips_sampler": part(trainer.lpips_sampler),
        "gate": None if trainer._gate is None else int(trainer._gate.item()),
        "density_log": [dict(e) for e in trainer.density_log], "store": store_fingerprint(trainer.frames)}
    sd = to_host(sd)
    check_leaves(sd)
    order = checkpoint_keys(1) + [EXTRA_KEY]
    assert set(sd) == set(order)
    return {k: sd[k] for k in order}


# ---- load -------------------------------------------------------------------------------------------------------------------------
def _load_optimizer(trainer, opt_sd):
    """``opt_sd``: in the trainer's own layout (``remap_optimizer``).  torch moves the state to the parameters' device; the fused
    optimiser copies it into its flat moments."""
    if trainer.fused:
        trainer.opt.load_state_dict(opt_sd)
    else:                                                        # (a copy: torch adopts the ``step`` tensors as they are and counts in place)
        trainer.opt.load_state_dict(copy.deepcopy(opt_sd))


def _apply_model(trainer, sd, opt_sd, mesh_sd=None, flags=None, before_rebuild=None):
    """The model entries into the trainer -- the modules in place, the set through ``AvatarTrainer._replace_set`` with a row map of -1s
    (every row is new to the optimiser, whose state ``opt_sd`` then fills), ONE rebuild, the statistics put back behind it."""
    m, dev = trainer.m, trainer.dev
    on = lambda t: t.to(dev) if torch.is_tensor(t) else t
    N = int(sd["xyz"].shape[0])
    trainer.sh_degree = int(sd["active_sh_degree"])
    if mesh_sd is not None:
        trainer.mesh.load_state_dict(mesh_sd, device=dev)
    if flags is not None:
        m.set_trainable(*flags)

    def restore():                                               # (behind the swap of the anchor parameter, before the rebuild)
        _load_optimizer(trainer, opt_sd)
        if trainer.fused:
            trainer.opt.set_active(set(trainer.active_groups()))
        for g in trainer.opt.param_groups:
            for p in g["params"]:
                p.grad = None
        if before_rebuild is not None:
            before_rebuild()

    def replace_set(xyz, lbs_weights, scaling_multiplier):
        trainer._replace_set(xyz, lbs_weights, torch.full((N,), -1, dtype=torch.int64, device=dev), scaling_multiplier=scaling_multiplier,
                             then=restore)
    m.load_checkpoint_entries({k: (on(v) if not isinstance(v, dict) else v) for k, v in sd.items()}, replace_set=replace_set)


def load_trainer_state_dict(trainer, sd, strict=True):
    """Make ``trainer`` the saved one (module docstring) -> the report of ``validate`` without the optimiser's state.  Everything is
    validated first: a ValueError leaves the trainer untouched and usable."""
    report = validate(sd, expectations(trainer), strict=strict)
    extra, opt_sd = sd[EXTRA_KEY], report.pop("optimizer")
    report.pop("N")
    both = {c: bool(extra["components"][c]) and getattr(trainer, c) is not None for c in COMPONENTS}
    dev = trainer.dev

    def before_rebuild():
        if both["poses"]:
            trainer.poses.load_state_dict(extra["poses"])
        if both["mesh_terms"]:                                   # (the rebuild resets the terms with these: reset is deterministic)
            trainer._mesh_verts = extra["mesh_terms"]["verts"].to(dev)
            trainer._mesh_normals = extra["mesh_terms"]["normals"].to(dev)
        trainer.iteration = int(extra["iteration"])
        m = trainer.m
        if tuple(m.l2_keys) != tuple(extra["l2_keys"]):
            m.l2_keys = tuple(extra["l2_keys"])
        if both["density_schedule"]:
            trainer.density_schedule.load_state_dict(extra["density_schedule"])
            trainer._gate.fill_(int(extra["gate"]))
            trainer._gate_value = int(extra["gate"])
        if both["frames"]:
            trainer.frames.load_state_dict(extra["frames"])
        if both["lpips_sampler"]:
            trainer.lpips_sampler.load_state_dict(extra["lpips_sampler"])
        trainer.density_log[:] = [dict(e) for e in extra["density_log"]]

    mesh_sd = None
    if both["mesh"]:
        mesh_sd = dict(extra["mesh"], **{k: sd[k] for k in ("vertex_label", "level_id", "gs_level_mark")})
    model = {k: sd[k] for k in checkpoint_keys(1)}
    model["opacity_offset"] = extra.get("opacity_offset")
    _apply_model(trainer, model, opt_sd, mesh_sd=mesh_sd, flags=(bool(extra["opt_geo"]), bool(extra["opt_app"])),
                 before_rebuild=before_rebuild)
    if both["mesh_terms"]:
        trainer.mesh_terms.set_iteration(trainer.iteration)
    return report


def load_reference(trainer, sd, faces=None):
    """A dict in the reference's own layout (``SinGS.state_dict()``, no ``"sings_amd"`` key): ONLY the model loads -- the anchors, the
    tri-plane, the decoders of level 0 (entries ``*_dec_1``, ... are ignored), ``scaling_multiplier``, the statistics, the skinning weights,
    the SH degree, Adam's state.  Iteration, schedules, feed, sampler and pose tables stay as the trainer has them.

    ``faces``: the file has no faces.  With them the trainer's mesh becomes ``MeshState.from_faces(faces, vertex_label, level_id)``; a
    trainer built with ``mesh=`` refuses a load without.  The reference's optimiser groups are mapped to this trainer's names
    (``REFERENCE_GROUPS``); if the mapped layout does not match the moments start at zero, with a warning (sings_hybrid.py:233-237).
    -> the report.  Validation first, as in ``load_trainer_state_dict``."""
    if not isinstance(sd, dict):
        raise ValueError("checkpoint: not a dict")
    if EXTRA_KEY in sd:
        raise ValueError(f"{EXTRA_KEY}: present -- this is a whole-run checkpoint: AvatarTrainer.load_state_dict")
    expect = expectations(trainer)
    if trainer.mesh is not None and faces is None:
        raise ValueError("faces: a trainer with mesh= needs them (the reference's file keeps vertex_label and level_id, not the faces)")
    if faces is not None and (trainer.mesh is None or sd.get("vertex_label") is None):
        raise ValueError("faces: given, but the trainer has no mesh= or the file no vertex_label")
    N = validate_model(sd, expect, faces=None if faces is None else torch.as_tensor(faces).cpu())
    report = {"ignored": sorted(k for k in sd if k not in checkpoint_keys(1)), "optimizer": "loaded"}
    try:
        opt_sd, rep = remap_optimizer(sd["optimizer"], expect["opt_groups"], rename=REFERENCE_GROUPS, strict=False)
        if rep["missing_groups"]:
            raise ValueError(f"optimizer: the file has no group for {rep['missing_groups']}")
        shapes = [((N,) + tuple(s[1:]) if g["name"] == "xyz" else tuple(s)) for g, ss in zip(expect["opt_groups"], expect["opt_shapes"]) for s in ss]
        _check_optimizer_shapes(opt_sd, shapes)
        report["dropped_groups"] = rep["dropped_groups"]
    except (ValueError, KeyError, TypeError) as e:
        warnings.warn(f"sings_amd.checkpoint: the optimiser's state does not fit ({e}); continuing without a pretrained optimiser")
        opt_sd, _ = remap_optimizer({"state": {}, "param_groups": expect["opt_groups"]}, expect["opt_groups"])
        report["optimizer"] = "zero"
    dev, mesh_sd = trainer.dev, None
    if faces is not None:
        from .topology import MeshState
        # (built before anything is changed; the mesh terms are reset for it by the rebuild, from the loaded anchors)
        level = sd.get("level_id")
        mesh_sd = MeshState.from_faces(torch.as_tensor(faces).to(dev), sd["vertex_label"].to(dev),
                                       None if level is None else level.to(dev).to(torch.float32)).state_dict()
    _apply_model(trainer, {k: sd.get(k) for k in checkpoint_keys(1)}, opt_sd, mesh_sd=mesh_sd)
    return report
