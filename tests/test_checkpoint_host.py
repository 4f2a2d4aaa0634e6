"""The pure parts of ``sings_amd.checkpoint`` on CPU tensors: the schema walk and the ``weights_only`` round trip, every refusal of
``validate`` (each leaving its inputs as they were), the mapping of the reference's optimiser groups, ``strict=False`` reporting, and
the atomic write.  The trainer's side (a live resume) is tests/test_gpu_checkpoint.py."""
import copy
import inspect
import os

import pytest
import torch

from sings_amd import checkpoint as ck
from sings_amd import export

N, J, F = 5, 4, 3
GROUPS = ("xyz", "triplane", "geometry", "appearance", "global_orient", "body_pose")
SHAPES = {"xyz": (N, 3), "triplane": (1, 2, 3, 3), "geometry": (2, 2), "appearance": (3,), "global_orient": (F, 6), "body_pose": (F, 138)}


def _adam_groups(names, step=7.0, extra=None):
    """A torch-Adam state dict with one parameter per group, the moments filled with the group's index."""
    state, groups = {}, []
    for i, n in enumerate(names):
        shape = SHAPES.get((extra or {}).get(n, n), (2,))
        state[i] = {"step": torch.tensor(step), "exp_avg": torch.full(shape, float(i + 1)), "exp_avg_sq": torch.full(shape, 0.5 * (i + 1))}
        groups.append({"name": n, "lr": 1e-3 * (i + 1), "betas": [0.9, 0.999], "eps": 1e-15, "weight_decay": 0, "amsgrad": False,
                       "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                       "decoupled_weight_decay": False, "params": [i]})
    return {"state": state, "param_groups": groups}


def _valid():
    """-> (a checkpoint as ``trainer_state_dict`` lays it out, what a matching trainer expects)."""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    sd = {"active_sh_degree": 1, "xyz": r(N, 3), "triplane": {"grids.0.0": r(1, 2, 3, 3)}, "scaling_multiplier": r(N, 1),
          "max_radii2D": r(N), "xyz_gradient_accum": r(N, 1), "denom": r(N, 1), "optimizer": _adam_groups(GROUPS),
          "spatial_lr_scale": 2.5, "betas": r(16), "lbs_weights": r(N, J), "vertex_label": torch.arange(N, dtype=torch.int32),
          "level_id": torch.zeros(N), "gs_level_mark": [0, N], "appearance_dec_0": {"w": r(3)}, "geometry_dec_0": {"w": r(2, 2)}}
    store = {"F": F, "H": 8, "W": 8, "K": 2, "random_bg": True}
    tables = {"global_orient": r(F, 6), "body_pose": r(F, 138), "transl": r(F, 3)}
    sd[ck.EXTRA_KEY] = {
        "version": ck.FORMAT_VERSION, "iteration": 9, "opt_geo": True, "opt_app": False, "l2_keys": ["xyz_offsets", "scales"],
        "optimizer_kind": "fused", "opacity_offset": r(N, 1), "components": {c: c != "lpips_sampler" for c in ck.COMPONENTS},
        "mesh": {"faces": torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32),
                 "edges": torch.tensor([[0, 1], [0, 2], [1, 2], [2, 3], [2, 4], [3, 4]], dtype=torch.int32)},
        "poses": tables, "mesh_terms": {"verts": r(N, 3), "normals": r(N, 3)},
        "density_schedule": {"densify_interval": 4, "last_t": 8}, "frames": {"seed": (1 << 64) - 3, "counter": 18},
        "lpips_sampler": None, "gate": 1, "store": dict(store),
        "density_log": [{"t": 3, "mode": "prune", "n_old": 9, "n_new": 5, "skipped": None}]}
    template = [{k: v for k, v in grp.items()} for grp in _adam_groups(GROUPS)["param_groups"]]
    expect = {"components": dict(sd[ck.EXTRA_KEY]["components"]), "store": dict(store), "J": J, "max_sh_degree": 3,
              "modules": {"triplane": {"grids.0.0": (1, 2, 3, 3)}, "geometry_dec_0": {"w": (2, 2)}, "appearance_dec_0": {"w": (3,)}},
              "poses": {k: tuple(v.shape) for k, v in tables.items()}, "mesh_verts": 86, "opt_groups": template,
              "opt_shapes": [[(86, 3) if n == "xyz" else SHAPES[n]] for n in GROUPS]}
    return sd, expect


def test_the_layout_is_the_references_keys_plus_one():
    sd, expect = _valid()
    assert set(sd) == set(export.checkpoint_keys(1)) | {"sings_amd"}
    rep = ck.validate(sd, expect)
    assert rep["skipped"] == rep["absent"] == rep["missing_groups"] == rep["dropped_groups"] == [] and rep["N"] == N
    assert ck.leaves_equal(rep["optimizer"]["state"], sd["optimizer"]["state"]) is None


def test_schema_walk_and_weights_only_round_trip(tmp_path):
    sd, _ = _valid()
    ck.check_leaves(sd)
    for bad, where in (((1, 2), r"\['a'\]"), ({1, 2}, r"\['a'\]"), (object(), r"\['a'\]"), (b"x", r"\['a'\]")):
        with pytest.raises(ValueError, match=where):
            ck.check_leaves({"a": bad})
    with pytest.raises(ValueError, match=r"\['l'\]\[1\]"):
        ck.check_leaves({"l": [1, (2,)]})
    with pytest.raises(ValueError, match="dict key"):
        ck.check_leaves({(1, 2): 3})
    import numpy as np
    with pytest.raises(ValueError, match="ndarray"):
        ck.check_leaves({"a": np.zeros(2)})
    # to_host makes any nest conform: tuples -> lists, numpy scalars -> numbers
    host = ck.to_host({"betas": (0.9, 0.999), "n": np.int64(3), "t": torch.ones(2)})
    ck.check_leaves(host)
    assert host["betas"] == [0.9, 0.999] and host["n"] == 3 and type(host["n"]) is int
    path = tmp_path / "human_000009.pth"
    ck.atomic_save(sd, path)
    back = torch.load(path, weights_only=True)
    assert ck.leaves_equal(sd, back) is None
    assert back["sings_amd"]["frames"]["seed"] == (1 << 64) - 3      # (a 64-bit seed survives as a Python int)
    assert ck.leaves_equal(ck.load_file(path), sd) is None
    # leaves_equal is about bits: -0.0 is not +0.0, and it names the entry
    other = copy.deepcopy(sd)
    other["denom"][2, 0] = -0.0
    sd["denom"][2, 0] = 0.0
    assert ck.leaves_equal(sd, other) == "checkpoint['denom']"
    with pytest.raises(ValueError, match="tuple"):
        ck.atomic_save({"a": (1, 2)}, tmp_path / "bad.pth")
    assert not (tmp_path / "bad.pth").exists()


def _set(path, value):
    def go(sd):
        node = sd
        for k in path[:-1]:
            node = node[k]
        node[path[-1]] = value
    return go


def _drop(path):
    def go(sd):
        node = sd
        for k in path[:-1]:
            node = node[k]
        del node[path[-1]]
    return go


X = "sings_amd"
REFUSALS = [
    ("a component the trainer lacks", _set((X, "components", "lpips_sampler"), True), "components"),
    ("a component the file lacks", _set((X, "components", "frames"), False), "components"),
    ("store fingerprint", _set((X, "store", "H"), 16), r"\['store'\]"),
    ("store K", _set((X, "store", "K"), 1), r"\['store'\]"),
    ("lbs rows", _set(("lbs_weights",), torch.zeros(N + 1, J)), "lbs_weights"),
    ("lbs joints", _set(("lbs_weights",), torch.zeros(N, J + 1)), "lbs_weights"),
    ("statistics rows", _set(("denom",), torch.zeros(N - 1, 1)), "denom"),
    ("radii rows", _set(("max_radii2D",), torch.zeros(N + 2)), "max_radii2D"),
    ("multiplier rows", _set(("scaling_multiplier",), torch.ones(N + 1, 1)), "scaling_multiplier"),
    ("xyz columns", _set(("xyz",), torch.zeros(N, 4)), "xyz"),
    ("moment rows", _set(("optimizer", "state", 0, "exp_avg"), torch.zeros(N + 1, 3)), r"optimizer\['state'\]\[0\]\['exp_avg'\]"),
    ("optimizer group", _set(("optimizer", "param_groups", 1, "name"), "v_embed"), "optimizer"),
    ("decoder shape", _set(("geometry_dec_0", "w"), torch.zeros(2, 3)), r"geometry_dec_0\['w'\]"),
    ("decoder key", _set(("appearance_dec_0", "extra"), torch.zeros(1)), "appearance_dec_0"),
    ("tri-plane shape", _set(("triplane", "grids.0.0"), torch.zeros(1, 2, 4, 4)), r"triplane\['grids.0.0'\]"),
    ("pose rows", _set((X, "poses", "body_pose"), torch.zeros(F + 1, 138)), r"\['poses'\]\['body_pose'\]: rows"),
    ("level mark", _set(("gs_level_mark",), [0, N - 1]), "gs_level_mark"),
    ("label rows", _set(("vertex_label",), torch.zeros(N + 1, dtype=torch.int32)), "vertex_label"),
    ("edge index", _set((X, "mesh", "edges"), torch.tensor([[0, N]], dtype=torch.int32)), "edges"),
    ("face index", _set((X, "mesh", "faces"), torch.tensor([[0, 1, -1]], dtype=torch.int32)), "faces"),
    ("opacity offset rows", _set((X, "opacity_offset"), torch.zeros(N + 1, 1)), "opacity_offset"),
    ("mesh terms rows", _set((X, "mesh_terms", "verts"), torch.zeros(N + 1, 3)), "mesh_terms"),
    ("future version", _set((X, "version"), ck.FORMAT_VERSION + 1), "version"),
    ("version zero", _set((X, "version"), 0), "version"),
    ("SH degree", _set(("active_sh_degree",), 4), "active_sh_degree"),
    ("a reference file", _drop((X,)), "load_reference"),
    ("an unknown top-level key", _set(("geometry_dec_1",), {}), "geometry_dec_1"),
    ("schedule state", _set((X, "density_schedule"), None), "density_schedule"),
    ("iteration", _set((X, "iteration"), -1), "iteration"),
]


@pytest.mark.parametrize("what,mutate,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_names_the_entry_and_writes_nothing(what, mutate, match):
    sd, expect = _valid()
    mutate(sd)
    before_sd, before_expect = copy.deepcopy(sd), copy.deepcopy(expect)
    with pytest.raises(ValueError, match=match):
        ck.validate(sd, expect)
    assert ck.leaves_equal(sd, before_sd) is None and expect == before_expect


def test_a_trainer_mesh_the_file_does_not_replace_must_have_n_vertices():
    sd, expect = _valid()
    sd[X]["components"]["mesh"] = sd[X]["components"]["mesh_terms"] = sd[X]["components"]["density_schedule"] = False
    with pytest.raises(ValueError, match="xyz: 5 rows, the trainer's mesh"):
        ck.validate(sd, expect, strict=False)
    expect["mesh_verts"] = N
    assert ck.validate(sd, expect, strict=False)["absent"] == ["mesh", "mesh_terms", "density_schedule"]


def test_strict_false_reports_what_it_skips():
    sd, expect = _valid()
    sd[X]["components"]["lpips_sampler"] = True                  # the file has a sampler, the trainer none
    sd[X]["lpips_sampler"] = {"seed": 1, "counter": 2}
    expect["components"]["decoder_schedule"] = True
    sd[X]["components"]["decoder_schedule"] = False              # the trainer has a decoder schedule, the file none
    # ... and the trainer learns no poses: its optimiser lacks the file's two pose groups
    expect["components"]["poses"] = False
    expect["opt_groups"], expect["opt_shapes"] = expect["opt_groups"][:4], expect["opt_shapes"][:4]
    with pytest.raises(ValueError, match="components"):
        ck.validate(sd, expect)
    before = copy.deepcopy(sd)
    rep = ck.validate(sd, expect, strict=False)
    assert rep["skipped"] == ["poses", "lpips_sampler"] and rep["absent"] == ["decoder_schedule"]
    assert rep["dropped_groups"] == ["global_orient", "body_pose"] and rep["missing_groups"] == []
    assert [g["name"] for g in rep["optimizer"]["param_groups"]] == list(GROUPS[:4]) and sorted(rep["optimizer"]["state"]) == [0, 1, 2, 3]
    assert ck.leaves_equal(sd, before) is None
    # the reverse: the trainer has a group the file lacks -> it starts without a state
    sd2, expect2 = _valid()
    sd2["optimizer"] = _adam_groups(GROUPS[:4])
    sd2[X]["components"]["poses"], sd2[X]["poses"] = False, None
    rep = ck.validate(sd2, expect2, strict=False)
    assert rep["missing_groups"] == ["global_orient", "body_pose"] and rep["absent"] == ["poses"]
    assert sorted(rep["optimizer"]["state"]) == [0, 1, 2, 3] and len(rep["optimizer"]["param_groups"]) == 6


def test_the_references_groups_map_to_the_trainers_names():
    ref_names = ["xyz", "v_embed", "geometry_dec_0", "appearance_dec_0", "geometry_dec_1", "appearance_dec_1", "global_orient",
                 "body_pose", "betas"]
    shape_of = {"v_embed": "triplane", "geometry_dec_0": "geometry", "appearance_dec_0": "appearance"}
    saved = _adam_groups(ref_names, step=12.0, extra=shape_of)
    template = _adam_groups(GROUPS)["param_groups"]
    for g in template:
        g["lr"] = 123.0
    before = copy.deepcopy(saved)
    out, rep = ck.remap_optimizer(saved, template, rename=ck.REFERENCE_GROUPS, strict=False)
    assert ck.leaves_equal(saved, before) is None
    assert rep == {"missing_groups": [], "dropped_groups": ["geometry_dec_1", "appearance_dec_1", "betas"]}
    assert [g["name"] for g in out["param_groups"]] == list(GROUPS) and [g["params"] for g in out["param_groups"]] == [[i] for i in range(6)]
    # the file's indices 0 1 2 3 6 7 became 0 .. 5; moments and steps are the file's objects, the rates the file's
    for new, old in enumerate((0, 1, 2, 3, 6, 7)):
        assert out["state"][new] is saved["state"][old]
        assert out["param_groups"][new]["lr"] == saved["param_groups"][old]["lr"] and out["param_groups"][new]["betas"] == (0.9, 0.999)
    assert ck.REFERENCE_GROUPS["v_embed"] == "triplane" and "betas" not in ck.REFERENCE_GROUPS
    with pytest.raises(ValueError, match="do not match"):
        ck.remap_optimizer(saved, template, rename=ck.REFERENCE_GROUPS, strict=True)
    # a matched group with another number of parameters is refused either way
    saved["param_groups"][1]["params"] = [1, 4]
    with pytest.raises(ValueError, match="'triplane' has 2 parameters in the file, 1"):
        ck.remap_optimizer(saved, template, rename=ck.REFERENCE_GROUPS, strict=False)
    # the parameters of one group must be at one step (what FusedAdam keeps per group)
    two = _adam_groups(GROUPS)
    two["param_groups"][2]["params"], two["param_groups"][3]["params"] = [2, 3], []
    ck._check_optimizer_shapes(two, [SHAPES[n] for n in GROUPS])
    two["state"][3]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="'geometry' are at different steps"):
        ck._check_optimizer_shapes(two, [SHAPES[n] for n in GROUPS])


def test_a_failed_write_leaves_the_existing_file(tmp_path, monkeypatch):
    sd, _ = _valid()
    path = tmp_path / "ckpt" / "human_000004.pth"
    ck.atomic_save(sd, path)
    good = path.read_bytes()

    def dies_half_way(obj, f, *a, **k):
        f.write(b"half a file")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", dies_half_way)
    other = copy.deepcopy(sd)
    other["sings_amd"]["iteration"] = 10
    with pytest.raises(OSError, match="disk full"):
        ck.atomic_save(other, path)
    monkeypatch.undo()
    assert path.read_bytes() == good and os.listdir(path.parent) == [path.name]      # (and no temporary file is left behind)
    assert torch.load(path, weights_only=True)["sings_amd"]["iteration"] == 9
    ck.atomic_save(other, path)                                                      # a second save replaces it
    assert torch.load(path, weights_only=True)["sings_amd"]["iteration"] == 10 and os.listdir(path.parent) == [path.name]


def test_the_trainer_gained_methods_not_parameters():
    from sings_amd.mesh_terms import MeshTerms
    from sings_amd.topology import MeshState
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    sig = inspect.signature(AvatarTrainer.__init__)
    assert list(sig.parameters) == ["self", "module", "settings_fn", "bg_color", "lrs", "smpl_scale", "transl", "use_graph", "fp",
                                    "sh_degree", "max_sh_degree", "betas", "eps", "optimizer", "lr_schedules", "poses", "mesh",
                                    "mesh_terms", "lpips_sampler", "decoder_schedule", "frames"]
    assert list(inspect.signature(AvatarTrainer.run).parameters) == ["self", "n_steps"]
    assert list(inspect.signature(AvatarTrainer.run_until).parameters) == ["self", "num_steps", "save_every", "save_dir"]
    for name in ("state_dict", "load_state_dict", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(AvatarTrainer, name)), name
    assert list(inspect.signature(AvatarTrainer.load_state_dict).parameters) == ["self", "sd", "strict"]
    for cls in (MeshState, MeshTerms):
        assert callable(cls.state_dict) and callable(cls.load_state_dict)
    assert callable(AvatarStep.checkpoint_entries) and callable(AvatarStep.load_checkpoint_entries)


def test_mesh_state_round_trip_keeps_the_saved_edges():
    from sings_amd.topology import MeshState
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    edges = torch.tensor([[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]], dtype=torch.int32)
    mesh = MeshState(faces, edges, torch.tensor([1, 1, 6, 7], dtype=torch.int32), torch.tensor([0.0, 0.0, 1.0, 1.0]), [0, 2, 4])
    sd = mesh.state_dict()
    assert set(sd) == set(MeshState.CHECKPOINT_KEYS) | {"faces", "edges"}
    other = MeshState(faces[:1], edges[:3], torch.zeros(3, dtype=torch.int32), torch.zeros(3), [0, 3])
    other.load_state_dict(ck.to_host(sd))
    assert ck.leaves_equal(ck.to_host(other.state_dict()), ck.to_host(sd)) is None and other.num_verts == 4
    assert other.gs_level_mark == [0, 2, 4] and other.gs_level_mark is not sd["gs_level_mark"]
