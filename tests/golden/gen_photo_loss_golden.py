"""Generates tests/golden/photo_loss_golden.npz and tests/golden/photo_loss_smooth_golden.npz by IMPORTING the reference's own loss functions (read-only at
/root/reference) in the build container.  Only the vectors ship.

    python tests/golden/gen_photo_loss_golden.py

sings/rec/losses/utils.py imports pytorch3d at module level for its (unrelated) regularisers; pytorch3d is not installed
here, so empty placeholder modules satisfy that import -- l1_loss / ssim / create_window below are pure torch and run
exactly as shipped.  The composite + weighting of loss.py:55-69 is applied here with the same expressions.

photo_loss_golden.npz: three frames of uniform noise (SSIM near 0) and the reference's window.  photo_loss_smooth_golden.npz: the regime
training runs in -- cases s1-s4 of tests/photo_smooth_case.py (GOLDEN_CASES: a smooth target, a render close to it inside a
silhouette, the constant background outside), same keys.  s1 is 109 x 33: at that size an fp64 evaluation with left-to-right fp32
window weights is 5.8e-6 from the fp64 twin's SSIM mean (tests/test_oracle_photo_loss_smooth.py asks for at least 4e-6), so the case did not
have to grow.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, REF)
for name in ("pytorch3d", "pytorch3d.ops"):
    sys.modules.setdefault(name, types.ModuleType(name))
for fn in ("knn_points", "laplacian", "cot_laplacian", "norm_laplacian"):
    setattr(sys.modules["pytorch3d.ops"], fn, None)
sp = types.ModuleType("sings.rec.utils.body_model.smpl_parsing"); sp.parse_weights = None
sys.modules.setdefault("sings.rec.utils.body_model.smpl_parsing", sp)
from sings.rec.losses import utils as ru                         # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from photo_smooth_case import GOLDEN_CASES, smooth_frame         # noqa: E402

l1_w, ssim_w = 0.8, 0.2


def reference_case(tag, raw, gt, mask, bg):
    t_raw = torch.from_numpy(raw).requires_grad_(True)
    t_mask = torch.from_numpy(mask).unsqueeze(0)
    pred = torch.clamp(t_raw, 0.0, 1.0)                                       # gs_renderer_single.py:96
    gt_img = torch.from_numpy(gt) * t_mask + torch.from_numpy(bg)[:, None, None] * (1. - t_mask)   # loss.py:58
    Ll1 = ru.l1_loss(pred, gt_img, t_mask)
    sm = ru.ssim(pred, gt_img)
    loss_ssim = (1.0 - sm) * (t_mask.sum() / (pred.shape[-1] * pred.shape[-2]))
    total = l1_w * Ll1 + ssim_w * loss_ssim
    total.backward()
    return {f"{tag}_raw": raw, f"{tag}_gt": gt, f"{tag}_mask": mask, f"{tag}_bg": bg,
            f"{tag}_l1": np.float32(Ll1.item()), f"{tag}_ssim_mean": np.float32(sm.item()),
            f"{tag}_loss_l1": np.float32((l1_w * Ll1).item()), f"{tag}_loss_ssim": np.float32((ssim_w * loss_ssim).item()),
            f"{tag}_grad": t_raw.grad.numpy().copy(), f"{tag}_gt_img": gt_img.detach().numpy()}


out = {}
rs = np.random.RandomState(77)
for tag, (H, W) in (("a", (48, 64)), ("b", (37, 53)), ("c", (96, 80))):
    raw = (rs.uniform(-0.2, 1.2, (3, H, W))).astype(np.float32)              # exercises the clamp on both sides
    gt = rs.uniform(0, 1, (3, H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((xx - W / 2) / (W / 3)) ** 2 + ((yy - H / 2) / (H / 2.5)) ** 2 < 1).astype(np.float32)
    mask[rs.uniform(size=mask.shape) < 0.05] = 0.5                            # soft mask values occur at silhouettes
    bg = rs.uniform(0, 1, 3).astype(np.float32)
    out.update(reference_case(tag, raw, gt, mask, bg))
out["weights"] = np.array([l1_w, ssim_w], np.float32)
out["window_1d"] = ru.gaussian(11, 1.5).numpy()
path = os.path.join(HERE, "photo_loss_golden.npz")
np.savez_compressed(path, **out)
print("wrote", path, {k: getattr(v, "shape", v) for k, v in out.items() if k.startswith("a_")})

smooth = {}
for tag, kw in GOLDEN_CASES.items():
    smooth.update(reference_case(tag, *smooth_frame(**kw)))
assert (smooth["s3_raw"] < 0).sum() > 20 and smooth["s3_gt"].max() <= 0.02 and smooth["s3_gt"].min() >= 0.0      # the dark case clamps
smooth["weights"] = out["weights"]
path = os.path.join(HERE, "photo_loss_smooth_golden.npz")
np.savez_compressed(path, **smooth)
print("wrote", path, {t: float(smooth[f"{t}_ssim_mean"]) for t in GOLDEN_CASES}, os.path.getsize(path), "bytes")
