"""Times the frozen decoders on the GPU box:  python tools/frozen_decode_time.py [--reps N] [--calls K] [--steps S] [--sizes N ...] [--out FILE]

At 102 146 and 150 000 points (an SMPL-H mesh subdivided twice; the benchmark's set) with the shipped widths -- 96 tri-plane features,
geometry decoder 128 wide, appearance decoder 64 wide:

    the decode    ``decode.decode_frozen`` -- tri-plane lookup + ONE launch per decoder (csrc/sg_decode_frozen.hip) -- against the same
                  function with ``fused=False``: today's per-layer kernels under ``torch.no_grad()``.  Also the two decoders alone on
                  features computed once.  Blocks of ``--calls`` calls between two HIP events, the candidates ALTERNATING, ``--reps``
                  blocks each; reported: the median per call and the spread (min .. max) of the blocks.  One beats the other when the
                  difference of the medians exceeds the larger spread; otherwise the two are NOT RESOLVED from each other.
    the step      ``AvatarTrainer.step`` replayed from a HIP graph (L2Norm + k-NN edge loss, deferred join, fused optimiser) with both
                  decoders frozen (``DecoderSchedule`` that never thaws) against the same trainer without a schedule -- the step every
                  iteration ran before the flags existed.  Blocks of ``--steps`` steps; the two trainers are built twice each, in
                  alternation.

Writes profiles/frozen_decode_time.json (``--out``)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from sings_amd import decode, grad_arena, overflow                # noqa: E402
from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField      # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings   # noqa: E402
from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm      # noqa: E402
from sings_amd.scene import avatar_scene                          # noqa: E402
from sings_amd.train_loop import AvatarTrainer, DecoderSchedule   # noqa: E402
from sings_amd.train_step import AvatarStep                       # noqa: E402

LRS = {"xyz": 3.2e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}
CFG = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [64, 64, 64], 'multires': [1, 2, 4]}
NEVER = 10 ** 9


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def block(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternating(fns, n, reps, warmup=2):
    """{name: per-call ms of each block}: the blocks of the candidates alternate, so that a drift of the box hits all of them."""
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            ms = block(fn, n)
            if r >= warmup:
                out[k].append(ms)
    return out


def verdict(a, b):
    """a against b (per-call ms of alternating blocks): resolved when the medians differ by more than the larger spread."""
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = statistics.median(b) - statistics.median(a)
    return {"difference_ms": diff, "spread_ms": spread, "resolved": abs(diff) > spread}


def modules(dev):
    torch.manual_seed(0)
    tri = HexPlaneField(CFG, bounds=1.2, device=dev, feature_minor=True)
    geo = GeometryDecoder(96).to(dev); app = AppearanceDecoder(96).to(dev)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-5.3); geo.scales[2].weight.mul_(0.1)
        geo.xyz_offsets.weight.mul_(0.01); geo.xyz_offsets.bias.zero_()
    return tri, geo, app


def build_trainer(dev, s, frozen):
    W, H = s["W"], s["H"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cam = s["cam"]
    consts = dict(bg=t(s["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    tri, geo, app = modules(dev)
    mod = AvatarStep(t(s["xyz_canon"]), t(s["lbs_weights"]), tri, geo, app, l2_norm=L2Norm(), gaussian_connect=GaussiansEdgeLoss(),
                     gaussian_connect_w=1.0, defer_regulariser_join=True).to(dev)
    A = torch.eye(4, device=dev).repeat(s["J"], 1, 1).contiguous()
    gt = torch.rand((3, H, W), device=dev)
    mask = torch.ones((H, W), device=dev)
    tr = AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), use_graph=True,
                       sh_degree=0, max_sh_degree=0, optimizer="fused",
                       decoder_schedule=DecoderSchedule(NEVER, NEVER, NEVER, NEVER) if frozen else None)
    return tr, A, gt, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[102146, 150000])
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_decode_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "frozen_decode_time.py needs the GPU"
    dev = torch.device("cuda:0")
    out = {"reps": a.reps, "calls_per_block": a.calls, "steps_per_block": a.steps, "device_name": torch.cuda.get_device_name(0), "sizes": {}}
    for N in a.sizes:
        s = avatar_scene(N=N, J=52)
        res = out["sizes"][str(N)] = {}
        tri, geo, app = modules(dev)
        xyz = torch.from_numpy(s["xyz_canon"]).to(dev)
        feats = decode.triplane_features_nograd(tri, xyz)

        # ---- (a) the no-gradient decode: fused against per-layer under no_grad
        fns = {"fused": lambda: decode.decode_frozen(xyz, tri, geo, app),
               "per_layer": lambda: decode.decode_frozen(xyz, tri, geo, app, fused=False),
               "fused_geometry": lambda: decode.frozen_geometry(feats, geo),
               "per_layer_geometry": lambda: decode.frozen_geometry(feats, geo, fused=False),
               "fused_appearance": lambda: decode.frozen_appearance(feats, app),
               "per_layer_appearance": lambda: decode.frozen_appearance(feats, app, fused=False)}
        x, y = fns["fused"](), fns["per_layer"]()
        res["max_rel_difference"] = {k: float((x[k] - y[k]).abs().max() / y[k].abs().max().clamp_min(1e-30)) for k in x if x[k] is not None}
        t = alternating(fns, a.calls, a.reps)
        res["decode_ms"] = {k: stats(v) for k, v in t.items()}
        res["decode_fused_against_per_layer"] = verdict(t["fused"], t["per_layer"])
        res["geometry_fused_against_per_layer"] = verdict(t["fused_geometry"], t["per_layer_geometry"])
        res["appearance_fused_against_per_layer"] = verdict(t["fused_appearance"], t["per_layer_appearance"])
        del tri, geo, app, feats

        # ---- (b) the captured step, both decoders frozen against the step without flags: one trainer at a time (they share the
        #      module-level gradient arena), built twice each in alternation; every block is `--steps` replayed steps
        if not a.skip_step:
            steps = {"unfrozen": [], "frozen": []}
            try:
                for _ in range(2):
                    for k in steps:
                        tr, A, gt, mask = build_trainer(dev, s, k == "frozen")
                        for _ in range(6):                        # sizing steps, the capture, replays
                            tr.step(A, gt, mask)
                        assert tr.captured is not None and (tr.m.opt_geo, tr.m.opt_app) == ((False, False) if k == "frozen" else (True, True))
                        steps[k] += [block(lambda: tr.step(A, gt, mask), a.steps) for _ in range(a.reps)]
                        del tr
                        overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
                        grad_arena.set_gradient_arena(None, None)
                res["captured_step_ms"] = {k: stats(v) for k, v in steps.items()}
                res["captured_step_frozen_against_unfrozen"] = verdict(steps["frozen"], steps["unfrozen"])
            finally:
                overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
                grad_arena.set_gradient_arena(None, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
