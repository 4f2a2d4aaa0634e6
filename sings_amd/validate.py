"""Validation on the device: PSNR, SSIM and LPIPS of a set of frames, K frames per launch, one host read at the end.

Mirrors ``SinGaussianTrainer.validate`` (sings/rec/trainer/gs_trainer.py:546-608), the source of a run's reported numbers:

    for data in val_dataset:                                   # one frame per pass, three host-visible reductions each
        image, gt = render_pkg["render"], data['rgb']          # (both * data['mask'] for dataset `zju`)
        psnr(image, gt).mean().double(); ssim(image, gt).mean().double(); lpips(image.clip(max=1), gt).mean().double()
    eval_metrics[iter_s][k] = torch.stack(v).mean().item()     # the fp64 mean over the frames of the fp32 per-frame values
    torch.save(metrics, 'val/eval_<iter>.pth')                 # the per-frame lists

``validate`` renders ``frames_per_launch`` frames per fused call (renderer.get_render_pkgs_fused), ``Validator`` turns each chunk into
rows of a device table (metrics.image_metrics: two launches; lpips.LPIPS on the whole chunk) and reads the table back ONCE in
``result()``.  ``comparison_grid`` is the reference's gt-beside-render log image.  Writing image files and ``results_{mode}.json``
stays with the caller.  No CPU fallback: the HIP library must be present.
"""
import torch

from . import _lib
from .metrics import image_metrics_table


class Validator:
    """Accumulates the per-frame figures of a validation pass on the device.

    ``add(raw, gt, mask=None)``: up to ``frames_per_launch`` frames -- ``raw`` [k,3,H,W] (or [3,H,W]) the UNCLAMPED render
    (``render_pkg['render_raw']``), ``gt`` [k,3,H,W] (or one [3,H,W]), ``mask`` [k,H,W] / [k,1,H,W] / [H,W] / [1,H,W], required
    and multiplied into both images when ``mask_images`` (the reference's `zju` branch), ignored otherwise.  No host read.
    ``result()``: ONE device-to-host copy -> {'psnr', 'ssim', 'lpips': float, 'per_frame': {the same keys: fp32 CPU tensors [F]}};
    'lpips' is absent without a network, as the reference skips an empty list.  ``save(path)``: the reference's ``eval_<iter>.pth``."""

    def __init__(self, W, H, device, lpips=None, frames_per_launch=8, mask_images=False):
        self.W, self.H, self.dev = int(W), int(H), torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("sings_amd.validate.Validator runs on the GPU only (no CPU fallback)")
        if self.W < 1 or self.H < 1 or int(frames_per_launch) < 1:
            raise ValueError("Validator: W, H and frames_per_launch must be >= 1")
        self.lpips, self.frames_per_launch, self.mask_images = lpips, int(frames_per_launch), bool(mask_images)
        self.keys = ("psnr", "ssim") + (("lpips",) if lpips is not None else ())
        self._rows = []                      # device tensors [k, len(keys)], in the order the frames were added
        self._host = None

    @torch.no_grad()
    def add(self, raw, gt, mask=None):
        if not torch.is_tensor(raw) or not raw.is_cuda:
            raise RuntimeError("sings_amd.validate: tensors must live on the GPU (no CPU fallback)")
        if raw.dim() == 3:
            raw = raw.unsqueeze(0)
        k = int(raw.shape[0])
        if raw.dim() != 4 or tuple(raw.shape[1:]) != (3, self.H, self.W):
            raise ValueError(f"Validator.add: raw must be [k,3,{self.H},{self.W}], got {tuple(raw.shape)}")
        if not 1 <= k <= self.frames_per_launch:
            raise ValueError(f"Validator.add: {k} frames in one call, frames_per_launch is {self.frames_per_launch}")
        if self.mask_images and mask is None:
            raise ValueError("Validator.add: mask_images is set, a mask is required")
        m = mask if self.mask_images else None
        table = image_metrics_table(raw, gt, m, clamp=True)
        cols = [table[:, 6:8]]
        if self.lpips is not None:
            image = torch.clamp(raw.detach().float(), 0.0, 1.0)
            target = gt.detach().float().expand(k, 3, self.H, self.W)
            if m is not None:
                m4 = m.detach().float().reshape(-1, 1, self.H, self.W)
                image, target = image * m4, target * m4
            cols.append(self.lpips(image.clip(max=1), target.contiguous()).reshape(k, 1))
        self._rows.append(torch.cat(cols, 1) if len(cols) > 1 else cols[0].clone())
        self._host = None

    def __len__(self):
        return sum(int(r.shape[0]) for r in self._rows)

    def _table(self):
        if self._host is None:
            if not self._rows:
                raise RuntimeError("Validator: no frame was added")
            self._host = torch.cat(self._rows, 0).cpu()          # the one device-to-host copy
        return self._host

    def result(self):
        t = self._table()
        out = {key: t[:, i].double().mean().item() for i, key in enumerate(self.keys)}      # torch.stack(v).mean().item()
        out["per_frame"] = {key: t[:, i].clone() for i, key in enumerate(self.keys)}
        return out

    def save(self, path):
        """What ``torch.save(metrics, f'{logdir}/val/eval_{iter_s}.pth')`` writes: {'lpips', 'psnr', 'ssim'} -> a list per key of
        0-dim float64 tensors, one per frame (on the CPU); the list of a metric that was not computed is empty."""
        t = self._table().double()
        metrics = {key: [] for key in ("lpips", "psnr", "ssim")}
        for i, key in enumerate(self.keys):
            metrics[key] = [t[f, i].clone() for f in range(t.shape[0])]
        torch.save(metrics, path)


@torch.no_grad()
def validate(canon, frames, bg_color=None, lpips=None, frames_per_launch=8, mask_images=False, smpl_scale=None):
    """The loop of gs_trainer.py:557-586 over ``frames``, a sequence of the validation dataset's dicts: the camera keys
    (``image_height``, ``image_width``, ``fovx``, ``fovy``, ``world_view_transform``, ``full_proj_transform``, ``camera_center``),
    ``rgb`` [3,H,W], ``mask`` ([H,W] or [1,H,W]; read with ``mask_images``), ``A_cano2pose`` [J,4,4] and optionally ``transl`` [3].
    ``canon``: the canonical Gaussians as ``get_render_pkg_fused`` takes them.  ``frames_per_launch`` (<= 16) frames are rendered per
    fused call and measured per metrics launch; the last chunk may be shorter.  ``bg_color`` defaults to zeros (:549).
    -> ``Validator.result()``.  All frames must share one image size and field of view (ValueError otherwise)."""
    from .renderer import get_render_pkgs_fused
    frames = list(frames)
    if not frames:
        raise ValueError("validate: no frames")
    n = int(frames_per_launch)
    if not 1 <= n <= _lib.MAX_FRAMES:
        raise ValueError(f"validate: frames_per_launch must be in 1..{_lib.MAX_FRAMES}")
    H, W = int(frames[0]["image_height"]), int(frames[0]["image_width"])
    for i, d in enumerate(frames):
        if (int(d["image_height"]), int(d["image_width"])) != (H, W) or tuple(d["rgb"].shape[-2:]) != (H, W):
            raise ValueError(f"validate: frame {i} is {int(d['image_width'])} x {int(d['image_height'])} (rgb {tuple(d['rgb'].shape)}), "
                             f"frame 0 is {W} x {H}: all frames must share one image size")
        if (float(d["fovx"]), float(d["fovy"])) != (float(frames[0]["fovx"]), float(frames[0]["fovy"])):
            raise ValueError(f"validate: frame {i} has another field of view than frame 0")
        if ("transl" in d and d["transl"] is not None) != ("transl" in frames[0] and frames[0]["transl"] is not None):
            raise ValueError("validate: 'transl' must be given for every frame or for none")
    dev = canon["xyz_canon"].device
    if bg_color is None:
        bg_color = torch.zeros(3, dtype=torch.float32, device=dev)
    has_transl = frames[0].get("transl") is not None
    val = Validator(W, H, dev, lpips=lpips, frames_per_launch=n, mask_images=mask_images)
    for c0 in range(0, len(frames), n):
        chunk = frames[c0:c0 + n]
        A = torch.stack([d["A_cano2pose"] for d in chunk]).to(dev).contiguous()
        transl = torch.stack([d["transl"].reshape(3) for d in chunk]).to(dev).contiguous() if has_transl else None
        pkg = get_render_pkgs_fused(chunk, canon, A, bg_color, smpl_scale=smpl_scale, transl=transl)
        gt = torch.stack([d["rgb"] for d in chunk]).to(dev)
        mask = torch.stack([d["mask"].reshape(H, W) for d in chunk]).to(dev) if mask_images else None
        val.add(pkg["render_raw"], gt, mask)
    return val.result()


def comparison_grid(gt, pred):
    """The reference's log image ``torchvision.utils.make_grid([gt_image, image], nrow=2, pad_value=1)`` (gs_trainer.py:588) by
    geometry alone: [3, H + 4, 2 W + 6], ones outside the two images, ``gt`` at rows 2..H+1 and columns 2..W+1, ``pred`` at
    columns W+4..2W+3.  Torch ops on the inputs' device; ``posed.frames_to_u8`` turns it into bytes."""
    if gt.dim() != 3 or gt.shape[0] != 3 or pred.shape != gt.shape:
        raise ValueError(f"comparison_grid: two [3,H,W] images expected, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    H, W = int(gt.shape[1]), int(gt.shape[2])
    grid = torch.ones((3, H + 4, 2 * W + 6), dtype=gt.dtype, device=gt.device)
    grid[:, 2:H + 2, 2:W + 2] = gt
    grid[:, 2:H + 2, W + 4:2 * W + 4] = pred.to(gt.dtype)
    return grid
