"""Generates tests/golden/metrics_golden.npz by IMPORTING the reference's own ``psnr`` (sings/rec/utils/image/image.py) and ``ssim``
(sings/rec/losses/utils.py), read-only at /root/reference, in the build container.  Only the vectors ship.

    python tests/golden/gen_metrics_golden.py

utils/image/image.py imports torchvision.utils.make_grid for its (unrelated) image writers and losses/utils.py imports pytorch3d
for its regularisers; neither is installed here, so empty placeholder modules satisfy those imports -- ``psnr`` and ``ssim`` are pure
torch and run exactly as shipped.  The frame preparation of SinGaussianTrainer.validate (gs_trainer.py:577-585) is applied here with
the same expressions: ``image`` is the clamped render (gs_renderer_single.py:96), both images times the mask for dataset `zju`.

Per case <tag>: the inputs (``raw``, ``gt``, ``mask`` where there is one) and, as the reference computes them in fp32, ``mse`` [3],
``psnr`` [3], ``psnr_mean`` and ``ssim_mean``; ``psnr_ref_err`` is the largest distance of those four fp32 PSNR figures from an fp64
evaluation of the same fp32 images (infinite figures left out): what the reference's own fp32 chain is off by.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, REF)
for name in ("pytorch3d", "pytorch3d.ops", "torchvision", "torchvision.utils"):
    sys.modules.setdefault(name, types.ModuleType(name))
for fn in ("knn_points", "laplacian", "cot_laplacian", "norm_laplacian"):
    setattr(sys.modules["pytorch3d.ops"], fn, None)
sys.modules["torchvision.utils"].make_grid = None
sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
sp = types.ModuleType("sings.rec.utils.body_model.smpl_parsing"); sp.parse_weights = None
sys.modules.setdefault("sings.rec.utils.body_model.smpl_parsing", sp)
from sings.rec.losses import utils as ru                         # noqa: E402
from sings.rec.utils.image import image as ri                    # noqa: E402


def soft_mask(rs, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((xx - W / 2) / (W / 3)) ** 2 + ((yy - H / 2) / (H / 2.5)) ** 2 < 1).astype(np.float32)
    mask[rs.uniform(size=mask.shape) < 0.05] = 0.5                            # soft mask values occur at silhouettes
    edge = rs.uniform(size=mask.shape) < 0.05
    mask[edge] = rs.uniform(0, 1, int(edge.sum())).astype(np.float32)
    return mask


out = {}
rs = np.random.RandomState(91)
CASES = (("a", (48, 64), False, False), ("b", (37, 53), False, False), ("c", (96, 80), False, False),
         ("zju", (48, 64), True, False), ("exact", (37, 53), False, True))
for tag, (H, W), masked, exact_green in CASES:
    raw = rs.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)                # exercises the clamp on both sides
    gt = rs.uniform(0, 1, (3, H, W)).astype(np.float32)
    if exact_green:
        raw[1] = gt[1]                                                        # in [0,1): the clamp leaves it, mse of the channel is 0
    if masked:
        # channels of very different quality: the mean of the channel PSNRs is far from the PSNR of the whole-image mse
        raw[0] = gt[0] + rs.normal(0, 0.02, (H, W)).astype(np.float32)
    out.update({f"{tag}_raw": raw, f"{tag}_gt": gt})
    image = torch.clamp(torch.from_numpy(raw), 0.0, 1.0)                      # gs_renderer_single.py:96
    gt_image = torch.from_numpy(gt)
    if masked:
        mask = soft_mask(rs, H, W)
        out[f"{tag}_mask"] = mask
        t_mask = torch.from_numpy(mask).unsqueeze(0)                          # data['mask'] is [1,H,W]
        image = image * t_mask                                                # gs_trainer.py:581-582
        gt_image = gt_image * t_mask
    p = ri.psnr(image, gt_image)                                              # [3,1]
    p_mean = p.mean()                                                         # :584
    s_mean = ru.ssim(image, gt_image).mean()                                  # :585
    mse = ri.mse(image, gt_image)
    # the same fp32 images, evaluated in fp64
    d64 = (image.double() - gt_image.double()) ** 2
    mse64 = d64.view(3, -1).mean(1)
    with np.errstate(divide="ignore"):
        p64 = 20.0 * np.log10(1.0 / np.sqrt(mse64.numpy()))
    ref = np.concatenate([p.reshape(3).numpy().astype(np.float64), [float(p_mean)]])
    exact = np.concatenate([p64, [p64.mean()]])
    finite = np.isfinite(exact)
    assert (np.isfinite(ref) == finite).all()
    out.update({f"{tag}_mse": mse.reshape(3).numpy().copy(), f"{tag}_psnr": p.reshape(3).numpy().copy(),
                f"{tag}_psnr_mean": np.float32(p_mean.item()), f"{tag}_ssim_mean": np.float32(s_mean.item()),
                f"{tag}_psnr_ref_err": np.float64(np.abs(ref[finite] - exact[finite]).max() if finite.any() else 0.0)})
    print(tag, (H, W), "psnr", p.reshape(3).tolist(), float(p_mean), "ssim", float(s_mean), "ref err", out[f"{tag}_psnr_ref_err"])
out["cases"] = np.array([c[0] for c in CASES])
out["masked"] = np.array([c[2] for c in CASES])
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics_golden.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
