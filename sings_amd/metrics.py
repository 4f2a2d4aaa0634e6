"""PSNR and SSIM of K rendered frames through the C ABI (sg_image_metrics_frames, csrc/sg_metrics.hip).

The figures of ``SinGaussianTrainer.validate`` (sings/rec/trainer/gs_trainer.py:577-585) as the reference computes them:

    image = clamp(raw, 0, 1)  [* mask];  gt = rgb  [* mask]         (the mask: dataset `zju` only)
    psnr(image, gt).mean()   -- PER-CHANNEL mse, 20 log10(1 / sqrt(mse_c)), the mean of the three (utils/image/image.py:15-17);
                                a channel that equals its target gives +inf, and so does the mean
    ssim(image, gt).mean()   -- 11 x 11, sigma 1.5, zero padding, over all 3 H W elements (losses/utils.py:39-70)

``image_metrics`` takes the UNCLAMPED render (``render_pkg['render_raw']``; the clamp is fused) of K frames and returns the per-frame
values as device tensors: two launches, no host synchronisation.  ``MetricsEngine`` is the pre-allocated form.  Nothing here is
differentiable.  The LPIPS figure: sings_amd/lpips.py; the validation loop over a dataset: sings_amd/validate.py.
No CPU fallback: the HIP library must be present.
"""
import torch

from . import _lib
from ._marshal import _ptr, _stream

STRIP_COLS = _lib.METRICS_STRIP_COLS      # columns a wave's strip emits
CHUNK_ROWS = _lib.METRICS_CHUNK_ROWS      # an image of up to this many rows is one chunk; taller ones are cut into chunks at least this tall


def _frames(pred, gt, mask):
    """-> (pred [K,3,H,W], gt, gt_stride, mask or None, mask_stride) contiguous fp32, shapes checked."""
    for name, t in (("pred", pred), ("gt", gt), ("mask", mask)):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"sings_amd.metrics: {name} must be a tensor on the GPU (no CPU fallback)")
        if t.device != pred.device:
            raise RuntimeError(f"sings_amd.metrics: {name} is on {t.device}, pred on {pred.device}")
    if pred.dim() == 3:
        pred = pred.unsqueeze(0)
    if pred.dim() != 4 or pred.shape[1] != 3 or not 1 <= pred.shape[0] <= 65535 or pred.shape[2] < 1 or pred.shape[3] < 1:
        raise ValueError(f"image_metrics: pred must be [K,3,H,W] or [3,H,W] with K in 1..65535, got {tuple(pred.shape)}")
    K, H, W = int(pred.shape[0]), int(pred.shape[2]), int(pred.shape[3])
    if tuple(gt.shape) not in ((K, 3, H, W), (3, H, W)):
        raise ValueError(f"image_metrics: gt must be [{K},3,{H},{W}] or one [3,{H},{W}] for all frames, got {tuple(gt.shape)}")
    gt_stride = 3 * H * W if gt.dim() == 4 and K > 1 else 0
    mask_stride = 0
    if mask is not None:
        if tuple(mask.shape) not in ((K, H, W), (K, 1, H, W), (H, W), (1, H, W)):
            raise ValueError(f"image_metrics: mask must be [K,H,W], [K,1,H,W], [H,W] or [1,H,W] for {K} frames of {H} x {W}, "
                             f"got {tuple(mask.shape)}")
        # (K = 1: [1,H,W] is both forms, and the same bytes)
        mask_stride = H * W if K > 1 and mask.numel() == K * H * W else 0
        mask = mask.detach().contiguous().float()
    return pred.detach().contiguous().float(), gt.detach().contiguous().float(), gt_stride, mask, mask_stride


def _launch(lib, K, W, H, clamp, pred, gt, gt_stride, mask, mask_stride, ws, table, dev):
    with torch.cuda.device(dev):
        _lib.check(lib.sg_image_metrics_frames(K, W, H, _lib.METRICS_CLAMP if clamp else 0, _ptr(pred), _ptr(gt), gt_stride,
                                               _ptr(mask), mask_stride, _ptr(ws), _ptr(table), _stream(dev)), "image metrics")


def image_metrics_table(pred, gt, mask=None, clamp=True):
    """The launch of ``image_metrics`` -> its [K, 8] device table (include/sings_eval.h: mse x 3, psnr x 3, mean psnr, mean ssim)."""
    if torch.is_grad_enabled() and any(t is not None and torch.is_tensor(t) and t.requires_grad for t in (pred, gt, mask)):
        raise RuntimeError("sings_amd.metrics: image_metrics is not differentiable; call it under torch.no_grad() or detach the inputs")
    pred, gt, gt_stride, mask, mask_stride = _frames(pred, gt, mask)
    lib = _lib.load()
    K, H, W = int(pred.shape[0]), int(pred.shape[2]), int(pred.shape[3])
    dev = pred.device
    ws = torch.empty(int(lib.sg_image_metrics_ws_bytes(K, W, H)), dtype=torch.uint8, device=dev)
    table = torch.empty((K, _lib.METRICS_FLOATS), dtype=torch.float32, device=dev)
    _launch(lib, K, W, H, clamp, pred, gt, gt_stride, mask, mask_stride, ws, table, dev)
    return table


def image_metrics(pred, gt, mask=None, clamp=True):
    """``pred`` [K,3,H,W] or [3,H,W] (the unclamped render with ``clamp``); ``gt`` the same, or one [3,H,W] for all frames; ``mask``
    [K,H,W], [K,1,H,W], [H,W] or [1,H,W] multiplies both images (None: no mask).
    -> dict(mse_channels [K,3], psnr_channels [K,3], psnr [K], ssim [K]) of fp32 device tensors.  Not differentiable: inputs that
    require grad are refused unless the call is under ``torch.no_grad()``."""
    t = image_metrics_table(pred, gt, mask, clamp)
    return {"mse_channels": t[:, 0:3], "psnr_channels": t[:, 3:6], "psnr": t[:, 6], "ssim": t[:, 7]}


class MetricsEngine:
    """Pre-allocated variant (as ``PhotoLossEngine``): fixed workspace and table, no allocation and no synchronisation per call, so a
    call can sit in a captured graph.  ``engine(pred, gt, mask=None, clamp=True)`` -> its [K, 8] table (overwritten by every call);
    ``pred`` [K,3,H,W] contiguous fp32 ([3,H,W] for K = 1), ``gt`` that or one [3,H,W], ``mask`` [K,H,W] or one [H,W]."""

    def __init__(self, W, H, device, K=1):
        self.lib = _lib.load()
        self.W, self.H, self.K = int(W), int(H), int(K)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("sings_amd.metrics.MetricsEngine runs on the GPU only (no CPU fallback)")
        n = int(self.lib.sg_image_metrics_ws_bytes(self.K, self.W, self.H))
        if n == 0:
            raise ValueError(f"MetricsEngine: K must be 1..65535 and the image at least 1 x 1, got K = {K}, {W} x {H}")
        self.ws = torch.empty(n, dtype=torch.uint8, device=self.dev)
        self.table = torch.zeros((self.K, _lib.METRICS_FLOATS), dtype=torch.float32, device=self.dev)

    def __call__(self, pred, gt, mask=None, clamp=True):
        hw = self.H * self.W
        for name, t, sizes in (("pred", pred, (self.K * 3 * hw,)), ("gt", gt, (3 * hw, self.K * 3 * hw)), ("mask", mask, (hw, self.K * hw))):
            if t is None and name == "mask":
                continue
            if not t.is_cuda:
                raise RuntimeError(f"sings_amd.metrics: {name} must live on the GPU (no CPU fallback)")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() not in sizes:
                raise ValueError(f"MetricsEngine: {name} must be contiguous fp32 of {' or '.join(map(str, sizes))} elements, got "
                                 f"{t.dtype} {tuple(t.shape)}")
        gt_stride = 3 * hw if gt.numel() == self.K * 3 * hw and self.K > 1 else 0
        mask_stride = hw if mask is not None and mask.numel() == self.K * hw and self.K > 1 else 0
        _launch(self.lib, self.K, self.W, self.H, clamp, pred, gt, gt_stride, mask, mask_stride, self.ws, self.table, self.dev)
        return self.table
