"""Animation throughput on the reference's own workload (anim_avatar.py -> trainer.animate_chunk -> forward_chunk): every frame
carries ext_tfs -- ONE manual_alignment('AMASS') placement as `.expand` views, what AnimDataset_opt.get_chunk builds -- and
smpl_scale ones [F,1].  150k-Gaussian avatar, 120 AMASS frames, 512x896.
    python tools/anim_placement_time.py
Prints frames/s for one frame per launch and for K = 8 / 16 frames per launch on 1-3 streams, the same K-frame run without ext_tfs
(the LAB 4.8 / 6.7 workload), and frames delivered to host memory (per-frame `.cpu()`) as float32 and as 8-bit BGR (out='bgr8').
The translation puts the placed avatar on the camera axis at half the scene's depth: at scale 0.5 it covers as many pixels as the
unplaced avatar does (seen from another side: the AMASS placement turns it 90 degrees about x)."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sings_amd.body import joint_transforms, rodrigues
from sings_amd.motion import manual_alignment
from sings_amd.posed import FrameAnimator, animate_chunk
from sings_amd.scene import avatar_scene
dev = torch.device("cuda:0")
s = avatar_scene(N=150000, J=52)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
cam = s["cam"]
data = dict(fovx=cam["fovx"], fovy=cam["fovy"], image_height=s["H"], image_width=s["W"],
            world_view_transform=t(cam["world_view_transform"]), full_proj_transform=t(cam["full_proj_transform"]),
            camera_center=t(cam["camera_center"]))
poses72 = np.load(os.path.join(ROOT, "tests", "golden", "lbs_golden.npz"))["amass_poses_72"]
F, J = poses72.shape[0], s["J"]
poses = np.zeros((F, J * 3), np.float32); poses[:, :72] = poses72; poses[:, :3] = 0
poses = t(poses); jr = t(s["joints_rest"])
canon = dict(xyz_canon=t(s["xyz_canon"]), rotmat_canon=None, scales=t(s["scales"]), opacity=t(s["opacities"]), shs=t(s["shs"]),
             lbs_weights=t(s["lbs_weights"]), active_sh_degree=0)
A_cano = joint_transforms(torch.zeros(J * 3, device=dev), jr, tuple(s["parents"]))
bg = t(s["bg"])
tr, aa, sc = manual_alignment("AMASS")
Rm = rodrigues(torch.tensor(aa, dtype=torch.float32)[None])[0].numpy().astype(np.float64)
centroid = s["xyz_canon"].mean(0).astype(np.float64)
target = np.array([0.0, 0.0, 0.5 * float(s["transl"][2])])
transl0 = (Rm.T @ ((target - np.asarray(tr, np.float64)) / sc) - centroid).astype(np.float32)   # p' = tr + sc R (p + transl)
transl = t(np.tile(transl0, (F, 1)))
ext_tfs = (torch.tensor(tr, dtype=torch.float32, device=dev)[None].expand(F, -1),
           torch.tensor(Rm, dtype=torch.float32, device=dev)[None].expand(F, -1, -1),
           torch.tensor([[sc]], dtype=torch.float32, device=dev).expand(F, -1))
ones = torch.ones(F, 1, device=dev)
plain_transl = t(np.tile(s["transl"], (F, 1)))


def run(label, streams, K, placed=True, out="float32", host=False, reps=3):
    anim = FrameAnimator(canon, streams) if streams > 1 or K > 1 else None
    kw = dict(transl=transl, smpl_scale=ones, ext_tfs=ext_tfs) if placed else dict(transl=plain_transl, smpl_scale=t(s["smpl_scale"]))
    for rep in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n = 0
        for f, img in animate_chunk(canon, poses, jr, A_cano, data, bg, parents=tuple(s["parents"]), chunk_size=16, animator=anim,
                                    frames_per_launch=K, out=out, **kw):
            if host:
                img = img.cpu()
            n += 1
        torch.cuda.synchronize(); el = time.perf_counter() - t0
    cover = float((img.float() < (0.99 if out == "float32" else 252)).float().mean())
    print(f"{label:<34s} streams={streams} K={K:2d} out={out:<7s}: {n / el:8.1f} frames/s ({el / n * 1e3:.3f} ms per frame, {n} frames,"
          f" {cover * 100:.1f} % of the last frame covered)", flush=True)


run("ext_tfs, one frame per launch", 1, 1)
for K in (8, 16):
    for streams in (1, 2, 3):
        run("ext_tfs + smpl_scale [F,1]", streams, K)
run("no ext_tfs (LAB 4.8 / 6.7 workload)", 2, 8, placed=False)
run("no ext_tfs (LAB 4.8 / 6.7 workload)", 3, 8, placed=False)
for out in ("float32", "bgr8"):
    for streams, K in ((2, 8), (3, 16)):
        run("to host memory (.cpu() per frame)", streams, K, out=out, host=True)
run("to host memory, one frame per launch", 1, 1, out="bgr8", host=True)
