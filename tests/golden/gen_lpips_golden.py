"""Generates tests/golden/lpips_golden.npz by IMPORTING the reference's own HumanLoss (sings/rec/losses/loss.py) and PatchSampler
(sings/rec/utils/image/sampler.py), read-only at /root/reference, in the build container.  Only the vectors ship.

    python tests/golden/gen_lpips_golden.py

cv2, lpips and pytorch3d are not installed here: empty placeholder modules satisfy the imports (cv2 is only used with dilate > 0,
the configs use 0), and the placeholder ``lpips.LPIPS`` is the fp64 oracle of tests/lpips_case.py.  What the vectors pin is the
glue around the network: the composition over the random background, the crop orientation, ``.clip(max=1)``, ``.mean()``, the
weight and the sampler's RNG calls.  Per seed: the origins the sampler drew (row, col), the random background, the
``lpips_patch`` value and dL/draw (raw: the UNCLAMPED render; the reference's ``render`` is clamp(raw, 0, 1)).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_case as lc                                           # noqa: E402

REF = "/root/reference"
sys.path.insert(0, REF)
for name in ("pytorch3d", "pytorch3d.ops", "cv2", "lpips"):
    sys.modules.setdefault(name, types.ModuleType(name))
for fn in ("knn_points", "laplacian", "cot_laplacian", "norm_laplacian"):
    setattr(sys.modules["pytorch3d.ops"], fn, None)
sp = types.ModuleType("sings.rec.utils.body_model.smpl_parsing"); sp.parse_weights = None
sys.modules.setdefault("sings.rec.utils.body_model.smpl_parsing", sp)
WT = lc.make_weights(5)


class _OracleLPIPS(lc.StandInLPIPS):
    def __init__(self, net="vgg", pretrained=True):
        super().__init__(WT)

    def to(self, *a, **k):                                        # (HumanLoss moves it to 'cuda')
        return self


sys.modules["lpips"].LPIPS = _OracleLPIPS
from sings.rec.losses.loss import HumanLoss                       # noqa: E402
from sings.rec.utils.image.sampler import PatchSampler            # noqa: E402

P, N, LPIPS_W = 32, 4, 1.0
out = {"patch_size": np.int32(P), "num_patches": np.int32(N), "lpips_w": np.float32(LPIPS_W), "weights_seed": np.int32(5)}
for seed in (3, 11, 21):
    raw, gt, mask, bg = lc.golden_inputs(seed)
    H, W = mask.shape
    t_mask = torch.from_numpy(mask)
    # the origins the sampler draws: the same seed, a coordinate image as the sampled argument
    np.random.seed(seed)
    coords = torch.from_numpy(np.stack(np.mgrid[0:H, 0:W]).astype(np.int64))
    _, cp = PatchSampler(num_patch=N, patch_size=P, ratio_mask=0.9, dilate=0).sample(t_mask.unsqueeze(0), coords)
    origins = cp[:, :, 0, 0].numpy().astype(np.int32)
    # the loss itself: the same numpy seed for the sampler, a torch seed for rand_like
    loss_fn = HumanLoss(l_ssim_w=0.0, l_l1_w=0.0, l_lpips_w=LPIPS_W, num_patches=N, patch_size=P, use_patches=True)
    t_raw = torch.from_numpy(raw).requires_grad_(True)
    np.random.seed(seed)
    torch.manual_seed(seed)
    _, loss_dict, _ = loss_fn({"rgb": torch.from_numpy(gt), "mask": t_mask}, {"render": torch.clamp(t_raw, 0.0, 1.0)},
                              bg_color=torch.from_numpy(bg))
    loss_dict["lpips_patch"].backward()
    torch.manual_seed(seed)
    bg_rand = torch.rand_like(torch.from_numpy(raw)).numpy()
    out.update({f"s{seed}_origins": origins, f"s{seed}_bg_rand": bg_rand.astype(np.float32),
                f"s{seed}_lpips_patch": np.float64(loss_dict["lpips_patch"].item()), f"s{seed}_grad": t_raw.grad.numpy().copy()})
    print(seed, origins.tolist(), loss_dict["lpips_patch"].item())
path = os.path.join(HERE, "lpips_golden.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
