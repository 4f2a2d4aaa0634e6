"""The decoder pre-fit on the GPU (``sings_amd.avatar_init.fit_initial_attributes``, the reference's ``SinGS.init_attrs``,
sings_hybrid.py:608-671): eager, replayed from a HIP graph, and a twin built here from torch ops -- torch's Adam, torch's
ReduceLROnPlateau fed with ``loss.item()`` -- around the library's ``decode_attributes``; then the whole sequence mesh -> module ->
fit -> trainer -> training steps on the tiny scene of tests/test_gpu_subdivide_train.py."""
import gc
import math
import os
import weakref

import numpy as np
import pytest
import torch

from mesh_case import bumpy_sphere
from test_gpu_train_loop import H, LRS, W, _modules, _scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
STEPS, PATIENCE = 60, 5
# the reference's rates (cfg.human.lr: position_init * smpl_spatial, vembed, geometry, appearance)
FIT_LRS = {"xyz": 0.00016 * 2.0, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}


def _sphere_module(seed=3):
    """bumpy_sphere(24, 16), 362 vertices, inside the tri-plane's box; a small tri-plane (one scale) and the library's decoders."""
    from sings_amd.avatar_init import from_mesh
    from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField
    v, f, lab = bumpy_sphere(24, 16)
    torch.manual_seed(seed)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [16, 12, 10], 'multires': [1]}
    tri = HexPlaneField(cfg, device=DEV); geo = GeometryDecoder(32).to(DEV); app = AppearanceDecoder(32).to(DEV)
    verts = torch.from_numpy(v * np.float32(0.5)).to(DEV)
    w = torch.full((len(v), 4), 0.25, dtype=torch.float32, device=DEV)
    return from_mesh(verts, torch.from_numpy(f).to(DEV), w, torch.from_numpy(lab).to(DEV), tri, geo, app)


def _twin(module, targets, steps, patience):
    """``init_attrs`` with torch ops around the library's decode: six ``mse_loss`` terms, ``torch.optim.Adam(eps=1e-15)``,
    ``ReduceLROnPlateau`` on ``loss.item()``.  -> (losses [steps], rates [steps, 4] each step ran with)."""
    from sings_amd.avatar_init import ATTR_KEYS
    groups = [{"params": [module.xyz], "lr": FIT_LRS["xyz"]}, {"params": list(module.triplane.parameters()), "lr": FIT_LRS["triplane"]},
              {"params": list(module.geometry_dec.parameters()), "lr": FIT_LRS["geometry"]},
              {"params": list(module.appearance_dec.parameters()), "lr": FIT_LRS["appearance"]}]
    opt = torch.optim.Adam(groups, betas=(0.9, 0.999), eps=1e-15)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=patience, factor=0.5)
    losses, rates = [], []
    for _ in range(steps):
        out = module.decode()
        terms = [torch.nn.functional.mse_loss(out[k], targets[k]) for k in ATTR_KEYS if out.get(k) is not None]
        loss = sum(terms)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        rates.append([float(g["lr"]) for g in opt.param_groups])
        opt.step()
        sch.step(loss.item())
        losses.append(loss.item())
    opt.zero_grad(set_to_none=True)
    return np.asarray(losses), np.asarray(rates)


@pytest.fixture(scope="module")
def runs():
    """The three runs from identically initialised modules, computed once."""
    from sings_amd import avatar_init, grad_arena
    out = {}
    seen, made = [], []
    real_capture, real_adam = avatar_init.capture_step, avatar_init.FusedAdam

    def watching_capture(fn, warmup=3, device=None):
        def watched():
            res = fn()
            seen.append(sum(1 for t in ([res] if torch.is_tensor(res) else list(res or ())) if t.requires_grad or t.grad_fn is not None))
            return res
        return real_capture(watched, warmup=warmup, device=device)

    def recording_adam(*a, **k):
        opt = real_adam(*a, **k)
        made.append(weakref.ref(opt))
        return opt

    avatar_init.capture_step, avatar_init.FusedAdam = watching_capture, recording_adam
    try:
        for name, use_graph in (("eager", False), ("graph", True)):
            module, mesh, targets = _sphere_module()
            before = [p.detach().clone() for p in module.parameters() if p.requires_grad]
            res = avatar_init.fit_initial_attributes(module, targets, FIT_LRS, init_steps=STEPS, patience=PATIENCE, use_graph=use_graph)
            out[name] = dict(res=res, module=module, before=before, arena=grad_arena.arena_registration())
    finally:
        avatar_init.capture_step, avatar_init.FusedAdam = real_capture, real_adam
    module, mesh, targets = _sphere_module()
    out["twin"] = _twin(module, targets, STEPS, PATIENCE)
    out["captured_outputs_with_graph"], out["optimisers"] = seen, made
    return out


def test_fit_eager_graph_and_torch_twin_agree(runs):
    e, g = runs["eager"]["res"], runs["graph"]["res"]
    t_loss, t_rates = runs["twin"]
    assert e["keys"] == g["keys"] == ["loss_xyz_offsets", "loss_scales", "loss_scales_aux", "loss_shs", "loss_opacity", "loss"]
    assert e["losses"].shape == g["losses"].shape == (STEPS, 6) and e["lr_steps"].shape == (STEPS, 4)
    le, lg = e["losses"][:, -1].astype(np.float64), g["losses"][:, -1].astype(np.float64)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    print("loss first / last:", le[0], le[-1], " rel eager-graph", rel(le, lg), " eager-twin", rel(le, t_loss), " graph-twin", rel(lg, t_loss))
    print("rates of the last step:", e["lr_steps"][-1], " reductions at", np.nonzero(np.diff(e["lr_steps"][:, 1]))[0] + 1)
    # the terms add up to the loss (fp32, in order)
    assert np.allclose(e["losses"][:, :-1].sum(1), e["losses"][:, -1], rtol=1e-6)
    # the bar of tests/test_gpu_train_loop_fused.py: 1e-4 relative at every step, between each pair
    assert rel(le, lg) <= 1e-4 and rel(le, t_loss) <= 1e-4 and rel(lg, t_loss) <= 1e-4
    # the rate trajectories: equal (halvings are exact); at least one reduction fired
    assert np.array_equal(e["lr_steps"], g["lr_steps"]) and np.array_equal(e["lr_steps"], t_rates)
    assert e["lr_steps"][-1, 1] < FIT_LRS["triplane"]
    assert np.array_equal(e["lr_steps"][0], [FIT_LRS[n] for n in ("xyz", "triplane", "geometry", "appearance")])
    assert set(e["lrs"]) == {"xyz", "triplane", "geometry", "appearance"} and e["lrs"] == g["lrs"]
    assert le[-1] < le[0] and lg[-1] < lg[0]


def test_fit_leaves_a_fitted_module_and_nothing_else(runs):
    from sings_amd import grad_arena
    for name in ("eager", "graph"):
        r = runs[name]
        after = [p for p in r["module"].parameters() if p.requires_grad]
        assert len(after) == len(r["before"])
        moved = [not torch.equal(a.detach(), b) for a, b in zip(after, r["before"])]
        assert all(moved), name                                         # every group moved, the anchors included
        assert all(p.grad is None for p in after)
        assert r["arena"] == ({}, None)                                 # decode has no arena set
    assert grad_arena.arena_registration() == ({}, None)
    # the capture saw only detached tensors (2 warm-up runs and the capture itself)
    assert runs["captured_outputs_with_graph"] == [0, 0, 0]
    # the optimiser the fit used, and with it the moments, is gone
    gc.collect()
    assert len(runs["optimisers"]) == 2 and all(r() is None for r in runs["optimisers"])


def test_fit_refuses():
    from sings_amd.avatar_init import fit_initial_attributes
    module, mesh, targets = _sphere_module()
    with pytest.raises(ValueError, match="lrs"):
        fit_initial_attributes(module, targets, {"xyz": 1e-4}, init_steps=2)
    bad = dict(targets, scales=targets["scales"][:-1])
    with pytest.raises(ValueError, match="scales"):
        fit_initial_attributes(module, bad, FIT_LRS, init_steps=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_initial_attributes(torch.nn.Linear(2, 2), targets, FIT_LRS, init_steps=2)


# ---- mesh -> module -> fit -> trainer -> steps
def _mesh_scene(golden):
    """The scene of test_gpu_train_loop with the 86 vertices of bumpy_sphere(12, 8) as anchors (the mesh, labels and skinning weights of
    the golden composite): the helper of tests/test_gpu_subdivide_train.py."""
    sc = _scene()
    v, f, lab = bumpy_sphere(12, 8)
    assert np.array_equal(f, golden["comp_faces"]) and np.array_equal(lab, golden["comp_vertex_label"])
    sc["xyz"] = (v * np.array([0.2, 0.42, 0.15])).astype(np.float32)
    sc["w"] = golden["comp_lbs_weights"]
    sc["faces"], sc["labels"] = f, lab
    return sc


@pytest.mark.parametrize("use_graph", [False, True])
def test_mesh_to_trainer(use_graph):
    from sings_amd.avatar_init import fit_initial_attributes, from_mesh
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.topology import MeshState
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topology_golden.npz"))
    sc = _mesh_scene(golden)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tri, geo, app = _modules(DEV)
    module, mesh, targets = from_mesh(t(sc["xyz"]), t(sc["faces"]), t(sc["w"]), t(sc["labels"]), tri, geo, app, init_opacity=0.83)
    V = len(sc["xyz"])
    assert isinstance(module, AvatarStep) and isinstance(mesh, MeshState) and mesh.num_verts == V == int(module.xyz.shape[0])
    assert tuple(module.scaling_multiplier.shape) == (V, 1) and bool((module.scaling_multiplier == 1).all())
    assert float(targets["opacity"][0]) == float(np.float32(0.83)) and targets["scales"].shape == (V, 3)
    first = fit_initial_attributes(module, targets, LRS, init_steps=20, patience=5, use_graph=use_graph)
    assert first["losses"].shape == (20, 6) and np.isfinite(first["losses"]).all() and first["losses"][-1, -1] < first["losses"][0, -1]
    cam = sc["cam"]
    consts = dict(bg=t(sc["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    tr = AvatarTrainer(module, settings, consts["bg"], LRS, smpl_scale=t(sc["smpl_scale"]), transl=t(sc["transl"]), use_graph=use_graph,
                       sh_degree=0, max_sh_degree=1, optimizer="fused", mesh=mesh)
    assert tr.opt.steps == [0, 0, 0, 0] and float(tr.opt.exp_avg.abs().max()) == 0.0      # fresh moments (gs_trainer.py:153)
    for i in range(2):
        ld = tr.step(t(sc["frames"][i]), t(sc["gts"][i]), t(sc["mask"]))
        assert math.isfinite(float(ld["loss"]))
    assert tr.opt.steps == [2, 2, 2, 2] and float(tr.opt.exp_avg.abs().max()) > 0.0
