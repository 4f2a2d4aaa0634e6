"""Shared by tests/test_gpu_metrics.py and tests/test_gpu_validate.py: the derived tolerances of the validation metrics, the fp64 /
CPU-oracle expectation of one frame (computed on the host, once per frame) and deterministic test frames."""
import numpy as np
import torch

from oracle.photo_loss_oracle import ssim_map
from sings_amd import metrics

MSE_RTOL = 5e-7
SSIM_ATOL = 2e-6
S, R = metrics.STRIP_COLS, metrics.CHUNK_ROWS       # the kernel's strip width and least chunk height


def psnr_tol(p):
    return 2.2e-6 + 2.0 ** -23 * abs(p)


def prepare(raw, gt, mask, clamp=True):
    """The fp32 images the reference measures: clamp, then both times the mask (fp32 products)."""
    x = np.clip(raw, np.float32(0), np.float32(1)) if clamp else raw
    y = gt
    if mask is not None:
        x, y = x * mask[None], y * mask[None]
    return x.astype(np.float32), y.astype(np.float32)


def expected(raw, gt, mask, clamp=True):
    """-> (mse64 [3], psnr64 [3], mean psnr, ssim mean of the CPU oracle) of one frame."""
    x, y = prepare(raw, gt, mask, clamp)
    mse = ((x.astype(np.float64) - y.astype(np.float64)) ** 2).reshape(3, -1).mean(1)
    with np.errstate(divide="ignore"):
        psnr = 20.0 * np.log10(1.0 / np.sqrt(mse))
    ssim = float(ssim_map(torch.from_numpy(x)[None], torch.from_numpy(y)[None]).double().mean())
    return mse, psnr, psnr.mean(), ssim


def check_row(row, exp, what, extra_psnr=0.0):
    mse, psnr, pmean, ssim = exp
    row = np.asarray(row, np.float64)
    print(f"{what}: mse rel {np.abs(row[0:3] - mse).max() / mse.max():.2e}, psnr {np.abs(row[3:6] - psnr).max():.2e} dB, "
          f"mean {abs(row[6] - pmean):.2e} dB, ssim {abs(row[7] - ssim):.2e}")
    assert np.all(np.abs(row[0:3] - mse) <= MSE_RTOL * mse), (what, row[0:3], mse)
    for c in range(3):
        assert abs(row[3 + c] - psnr[c]) <= psnr_tol(psnr[c]) + extra_psnr, (what, c, row[3 + c], psnr[c])
    assert abs(row[6] - pmean) <= psnr_tol(pmean) + extra_psnr, (what, row[6], pmean)
    assert abs(row[7] - ssim) <= SSIM_ATOL, (what, row[7], ssim)


def frame(seed, H, W, smooth=False):
    rs = np.random.RandomState(seed)
    if smooth:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        gt = np.stack([0.5 + 0.45 * np.sin(xx / (17 + 3 * c) + c) * np.cos(yy / (23 - 2 * c)) for c in range(3)]).astype(np.float32)
        raw = (gt + rs.normal(0, 0.08, gt.shape)).astype(np.float32)
    else:
        gt = rs.uniform(0, 1, (3, H, W)).astype(np.float32)
        raw = rs.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
    mask = np.clip(rs.uniform(-0.5, 1.5, (H, W)), 0, 1).astype(np.float32)      # zeros, ones and soft values
    return raw, gt, mask
