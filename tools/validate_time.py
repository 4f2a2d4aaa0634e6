"""Times validation on the GPU box:  python tools/validate_time.py [--reps N] [--frames F] [--lpips] [--launch-only] [--out FILE]

At 512 x 896 and at 1920 x 1080, for K = 1 and K = 8 frames per launch, per frame:

    the metrics launch   ``metrics.MetricsEngine`` (csrc/sg_metrics.hip: two launches for K frames, no host read), without and with a
                         mask, against a torch-ops twin of the reference's ``psnr`` + ``ssim`` on the same GPU (utils/image/image.py:15-17,
                         losses/utils.py:28-70 restated: the window built per call as ``create_window`` does, five depth-wise
                         ``conv2d``, about thirty kernels per frame, K frames = K passes; no host read either, so this is the
                         arithmetic alone).  The inputs rotate over a pool of frames larger than the Infinity Cache (> 600 MB), so
                         every call reads its planes from HBM.  The launch's byte floor is K H W (24 + 4 if masked) bytes; the
                         fraction of the copy rate of this run (``benchkit.roofline.measure_copy_peak``) it reaches is reported.
    a whole validation   ``validate.validate`` over ``--frames`` (32) frames of the synthetic avatar (150 000 Gaussians), rendered and
                         measured K at a time with ONE host read at the end, against the reference's shape: one frame per call
                         (``get_render_pkg_fused``), the torch-ops twin, and a host read per metric (``.item()``).  ``--lpips`` adds
                         the LPIPS column to both (the same HIP network with stand-in weights, whole frames: it dominates both arms).

Every timed block starts and ends in a device synchronise and is bracketed by HIP events; warm-up first, medians over ``--reps``
(>= 5) blocks and their spread.  Writes profiles/validate_time.json (``--out``)."""
import argparse
import json
import os
import statistics
import sys
from math import exp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import torch.nn.functional as F                                   # noqa: E402

from sings_amd import metrics, validate as V                      # noqa: E402

SIZES = ((512, 896), (1920, 1080))
POOL_BYTES = 600e6


def twin_psnr(img1, img2):
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def twin_ssim(img1, img2):
    ch = img1.size(-3)
    g = torch.Tensor([exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    w = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(ch, 1, 11, 11).contiguous().cuda(img1.get_device()).type_as(img1)
    mu1, mu2 = F.conv2d(img1, w, padding=5, groups=ch), F.conv2d(img2, w, padding=5, groups=ch)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img1 * img1, w, padding=5, groups=ch) - mu1_sq
    s2 = F.conv2d(img2 * img2, w, padding=5, groups=ch) - mu2_sq
    s12 = F.conv2d(img1 * img2, w, padding=5, groups=ch) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()


def twin_frame(raw, gt, mask=None):
    """gs_trainer.py:577-585 for one frame -> (psnr, ssim) 0-dim float64 device tensors."""
    image = torch.clamp(raw, 0.0, 1.0)
    if mask is not None:
        image, gt = image * mask, gt * mask
    return twin_psnr(image, gt).mean().double(), twin_ssim(image, gt).mean().double()


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), res


def stats(ms, per):
    us = [m * 1e3 / per for m in ms]
    return {"median_us_per_frame": statistics.median(us), "min": min(us), "max": max(us)}


def launch_times(dev, W, H, reps, copy_gbs):
    hw = H * W
    P = max(16, (int(POOL_BYTES // (24 * hw)) + 8) // 8 * 8)          # frames in the pool, a multiple of 8
    g = torch.Generator(device=dev).manual_seed(W + H)
    gt = torch.rand((P, 3, H, W), device=dev, generator=g)
    raw = gt + 0.1 * torch.randn((P, 3, H, W), device=dev, generator=g)
    mask = (torch.rand((P, H, W), device=dev, generator=g) * 2 - 0.5).clamp_(0, 1)
    out = {"pool_frames": P}
    # the two agree on a frame before anything is timed
    ours = metrics.image_metrics_table(raw[:1], gt[:1], mask[:1])[0]
    tp, ts = twin_frame(raw[0], gt[0], mask[0].unsqueeze(0))
    out["psnr_difference_dB"], out["ssim_difference"] = abs(float(ours[6]) - float(tp)), abs(float(ours[7]) - float(ts))
    for K in (1, 8):
        eng = metrics.MetricsEngine(W, H, dev, K=K)
        calls = P // K

        def device(masked):
            for i in range(calls):
                s = slice(i * K, i * K + K)
                eng(raw[s], gt[s], mask[s] if masked else None)

        def twin(masked):
            for i in range(P):
                twin_frame(raw[i], gt[i], mask[i].unsqueeze(0) if masked else None)

        for masked in (False, True):
            key = f"K{K}{'_masked' if masked else ''}"
            for name, fn in (("device", device), ("torch", twin)):
                if name == "torch" and K != 1:
                    continue                                          # (the twin has no K: it is K passes)
                fn(masked)
                ms = [timed(lambda: fn(masked))[0] for _ in range(reps)]
                r = stats(ms, P)
                if name == "device":
                    floor = hw * (24 + (4 if masked else 0))
                    r["byte_floor_per_frame"] = floor
                    r["GBs"] = floor / (r["median_us_per_frame"] * 1e-6) / 1e9
                    r["fraction_of_copy_rate"] = r["GBs"] / copy_gbs
                out[f"{key}_{name}"] = r
        for masked in (False, True):
            k = f"K{K}{'_masked' if masked else ''}"
            out[f"{k}_torch_over_device"] = out[f"K1{'_masked' if masked else ''}_torch"]["median_us_per_frame"] / out[f"{k}_device"]["median_us_per_frame"]
    return out


def avatar_frames(dev, W, H, nframes):
    from sings_amd.body import joint_transforms
    from sings_amd.camera import make_camera
    from sings_amd.scene import avatar_scene
    s = avatar_scene(N=150000, J=52, W=W, H=H, seed=4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    canon = dict(xyz_canon=t(s["xyz_canon"]), rotmat_canon=None, scales=t(s["scales"]), opacity=t(s["opacities"]), shs=t(s["shs"]),
                 lbs_weights=t(s["lbs_weights"]), active_sh_degree=0)
    rs = np.random.RandomState(8)
    f = 5000.0 * min(H / 896.0, 1.0)
    cm = make_camera(np.eye(4, dtype=np.float32), f, f, W / 2, H / 2, W, H)
    cam = dict(fovx=cm["fovx"], fovy=cm["fovy"], image_height=H, image_width=W, world_view_transform=t(cm["world_view_transform"]),
               full_proj_transform=t(cm["full_proj_transform"]), camera_center=t(cm["camera_center"]))
    jr = t(s["joints_rest"])
    frames = []
    for _ in range(nframes):
        pose = np.zeros(52 * 3, np.float32); pose[3:72] = rs.normal(0, 0.2, 69)
        d = dict(cam)
        d["A_cano2pose"] = joint_transforms(t(pose), jr, tuple(s["parents"]))
        d["transl"] = t(s["transl"])
        d["rgb"] = torch.rand((3, H, W), device=dev)
        d["mask"] = torch.ones((1, H, W), device=dev)
        frames.append(d)
    return canon, frames


def reference_shaped_loop(canon, frames, bg, lpips):
    """One frame per call, a host read per metric."""
    from sings_amd.renderer import get_render_pkg_fused
    vals = {"psnr": [], "ssim": [], "lpips": []}
    with torch.no_grad():
        for d in frames:
            pkg = get_render_pkg_fused(d, canon, d["A_cano2pose"], bg, transl=d["transl"])
            p, s = twin_frame(pkg["render"], d["rgb"])
            vals["psnr"].append(p.item()); vals["ssim"].append(s.item())
            if lpips is not None:
                vals["lpips"].append(lpips(pkg["render"].clip(max=1), d["rgb"]).mean().double().item())
    return {k: float(np.mean(v)) for k, v in vals.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--lpips", action="store_true")
    ap.add_argument("--launch-only", action="store_true", help="the metrics launch alone (e.g. for a variant library: SINGS_HIP_LIB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "validate_time.py needs the GPU"
    from benchkit.roofline import measure_copy_peak
    dev = torch.device("cuda:0")
    out = {"reps": a.reps, "frames": a.frames, "lpips": bool(a.lpips), "device_name": torch.cuda.get_device_name(0),
           "copy_GBs": measure_copy_peak(dev)}
    lp = None
    if a.lpips:
        from lpips_case import make_weights
        from sings_amd.lpips import LPIPS
        wt = make_weights(seed=0)
        lp = LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"], device=dev)
    for W, H in SIZES:
        key = f"{W}x{H}"
        out[f"launch_{key}"] = launch_times(dev, W, H, a.reps, out["copy_GBs"])
        torch.cuda.empty_cache()
        if a.launch_only:
            continue
        canon, frames = avatar_frames(dev, W, H, a.frames)
        bg = torch.zeros(3, device=dev)
        arms = {"K1": lambda: V.validate(canon, frames, lpips=lp, frames_per_launch=1),
                "K8": lambda: V.validate(canon, frames, lpips=lp, frames_per_launch=8),
                "one_frame_host_reads": lambda: reference_shaped_loop(canon, frames, bg, lp)}
        res = {}
        for name, fn in arms.items():
            fn()
            runs = [timed(fn) for _ in range(a.reps)]
            res[name] = stats([r[0] for r in runs], a.frames)
            res[name]["psnr"], res[name]["ssim"] = runs[-1][1]["psnr"], runs[-1][1]["ssim"]
        for k in ("K1", "K8"):
            res[f"one_frame_over_{k}"] = res["one_frame_host_reads"]["median_us_per_frame"] / res[k]["median_us_per_frame"]
        out[f"validate_{key}"] = res
        del canon, frames
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
