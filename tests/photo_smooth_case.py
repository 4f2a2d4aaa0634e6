"""Shared by tests/golden/gen_photo_loss_golden.py, tests/test_oracle_photo_loss_smooth.py and tests/test_gpu_photo_loss_smooth.py:
the smooth-frame regime of the photometric loss -- a low-frequency target, a render close to it inside a silhouette and the constant
background outside, SSIM between 0.3 and 0.999 -- its frames, the fp64 expectation of one frame (computed on the host, once per
frame and pair of upstream weights) and the bounds.

Bounds.  None comes from the kernel's output.
  scalars   the project's 2e-6: absolute for the SSIM mean and the weighted SSIM loss, 2e-6 relative + 1e-7 for the L1 terms
            (tests/test_gpu_photo_loss.py)
  gradient  max(4 x the distance of the fp32 oracle from the fp64 twin on the SAME frame, 1e-5 x max |grad64|), elementwise in the
            max norm.  On a smooth frame E[x^2] - mu^2 and 2 sigma12 + C2 are small differences of window sums of magnitude 0.3, so
            the fp32 restatement of the reference is itself 2e-5 to 9e-5 of the gradient's maximum away from fp64; the kernel's
            separable 11 + 11 fma chains and the reference's 121-tap conv2d round differently in those same sums, and a small multiple
            (4) of the reference's own fp32 error is what fp32 can promise.
"""
import functools

import numpy as np
import torch

from oracle import photo_loss_oracle as plo

L1_W, SSIM_W = 0.8, 0.2
SSIM_ATOL = 2e-6
GRAD_FACTOR, GRAD_FLOOR = 4.0, 1e-5
WHITE = (1.0, 1.0, 1.0)


def l1_tol(v):
    return 2e-6 * abs(v) + 1e-7


def left_to_right_taps():
    """The eleven weights as a left-to-right fp32 sum gives them (what sg_loss.hip's host code computed before it shared the metrics
    kernel's window): the sum is one ulp below the correctly rounded one, nine weights one ulp too large."""
    g = np.array([np.float32(np.exp(-((x - 5) ** 2) / (2.0 * 1.5 * 1.5))) for x in range(11)], np.float32)
    s = np.float32(0.0)
    for v in g:
        s = np.float32(s + v)
    return (g / s).astype(np.float32)


def silhouette(H, W, soft_px=0.0, fill=0.46):
    """An ellipse in the middle of the frame (semi-axes ``fill`` W and ``fill`` H); ``soft_px``: a linear ramp 0 -> 1 over that many
    pixels across its outline (distance measured along the shorter semi-axis)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.sqrt(((xx - W / 2) / (fill * W)) ** 2 + ((yy - H / 2) / (fill * H)) ** 2)
    if soft_px <= 0.0:
        return (r < 1.0).astype(np.float32)
    d = (1.0 - r) * fill * min(W, H)                          # pixels inside the outline (negative: outside)
    return np.clip(d / soft_px + 0.5, 0.0, 1.0).astype(np.float32)


def smooth_frame(seed, H, W, sigma, bg=WHITE, lo=0.3, hi=0.9, soft_px=0.0, period=1.0):
    """-> raw, gt, mask, bg (fp32).  The target is low-frequency in [lo, hi] (``period`` scales its wavelengths, 119 px across and
    82 px down at 1.0); the render is the composited target plus N(0, sigma) wherever the mask is not zero, and IS the background
    outside the silhouette, bit for bit.  (Noise at full strength on the soft rim too: where the render equals the composited
    target to the last few bits, sign(pred - gt) of the L1 term depends on the rounding of the composite, and no two
    precisions agree on it.  ``Expect`` refuses such frames.)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    mid, amp = 0.5 * (lo + hi), 0.5 * (hi - lo)
    gt = np.stack([mid + amp * np.sin(xx / (period * (19.0 + 3 * c)) + c) * np.cos(yy / (period * (13.0 - 2 * c)))
                   for c in range(3)]).astype(np.float32)
    mask = silhouette(H, W, soft_px)
    bg = np.asarray(bg, np.float32)
    comp = gt * mask[None] + bg[:, None, None] * (np.float32(1.0) - mask[None])              # fp32, as loss.py:58
    raw = (comp + rs.normal(0.0, sigma, gt.shape).astype(np.float32) * (mask[None] > 0)).astype(np.float32)
    return raw, gt, mask, bg


# the golden cases: name -> arguments of smooth_frame (tests/golden/gen_photo_loss_golden.py stores them with the reference's outputs)
GOLDEN_CASES = {
    "s1": dict(seed=101, H=33, W=109, sigma=0.03),                                   # mid SSIM: exposes the window's weights
    "s2": dict(seed=102, H=17, W=55, sigma=0.003),                                   # SSIM about 0.996
    # dark: C1, C2 dominate both denominators; the render goes below 0 (clamp) where the target is under the noise
    "s3": dict(seed=103, H=32, W=64, sigma=1e-3, bg=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, period=0.3),
    "s4": dict(seed=104, H=48, W=65, sigma=0.03, soft_px=6.0),                       # soft silhouette
}


class Expect:
    """fp64 twin and fp32 oracle of one frame for one pair of upstream weights (a on the weighted L1 term, b on the SSIM term)."""

    def __init__(self, raw, gt, mask, bg, a=1.0, b=1.0, grad=True):
        t = [torch.from_numpy(np.ascontiguousarray(v)) for v in (gt, mask, bg)]
        if not grad:                                          # the fp64 scalars alone, two 11-tap passes (a large frame: a 30th of the time)
            with torch.no_grad():
                o = plo.photometric_loss(torch.from_numpy(raw).double(), *t, L1_W, SSIM_W, dtype=torch.float64, separable=True)
            self.s64 = self.s32 = {k: o[k].item() for k in ("l1", "ssim", "l1_raw", "ssim_mean")}
            return
        r64 = torch.from_numpy(raw).double().requires_grad_(True)
        o = plo.photometric_loss(r64, *t, L1_W, SSIM_W, dtype=torch.float64)
        (a * o["l1"] + b * o["ssim"]).backward()
        self.s64 = {k: o[k].item() for k in ("l1", "ssim", "l1_raw", "ssim_mean")}
        self.g64 = r64.grad.numpy()
        r32 = torch.from_numpy(raw).requires_grad_(True)
        o32 = plo.photometric_loss(r32, *t, L1_W, SSIM_W)
        (a * o32["l1"] + b * o32["ssim"]).backward()
        self.s32 = {k: o32[k].item() for k in ("l1", "ssim", "l1_raw", "ssim_mean")}
        self.g32 = r32.grad.numpy()
        self.gt_img = o32["gt_img"].detach().numpy()
        # the frame must not sit on the L1 term's discontinuity: pred == gt in one precision and not in the other
        d32, d64 = (o32["pred_img"] - o32["gt_img"]).detach().numpy(), (o["pred_img"] - o["gt_img"]).detach().numpy()
        assert np.array_equal(np.sign(d32), np.sign(d64)), "frame has pixels where sign(pred - gt) depends on the precision"
        self.pred_img = o32["pred_img"].detach().numpy()
        self.gmax = float(np.abs(self.g64).max())
        self.oracle_grad_dist = float(np.abs(self.g32.astype(np.float64) - self.g64).max())
        self.grad_bound = max(GRAD_FACTOR * self.oracle_grad_dist, GRAD_FLOOR * self.gmax)

    def check_scalars(self, what, l1, ssim, l1_raw, ssim_mean):
        s = self.s64
        print(f"{what}: ssim_mean {s['ssim_mean']:.6f} kernel-fp64 {ssim_mean - s['ssim_mean']:+.2e} (oracle-fp64 "
              f"{self.s32['ssim_mean'] - s['ssim_mean']:+.2e}), l1_raw rel {(l1_raw - s['l1_raw']) / s['l1_raw']:+.2e} (oracle "
              f"{(self.s32['l1_raw'] - s['l1_raw']) / s['l1_raw']:+.2e})")
        assert abs(l1_raw - s["l1_raw"]) <= l1_tol(s["l1_raw"]), (what, l1_raw, s["l1_raw"])
        assert abs(ssim_mean - s["ssim_mean"]) <= SSIM_ATOL, (what, ssim_mean, s["ssim_mean"])
        assert abs(l1 - s["l1"]) <= l1_tol(s["l1"]), (what, l1, s["l1"])
        assert abs(ssim - s["ssim"]) <= SSIM_ATOL, (what, ssim, s["ssim"])

    def check_grad(self, what, g):
        err = float(np.abs(g.astype(np.float64) - self.g64).max())
        print(f"{what}: grad kernel-fp64 {err:.2e} = {err / self.gmax:.2e} of max, oracle-fp64 {self.oracle_grad_dist:.2e} = "
              f"{self.oracle_grad_dist / self.gmax:.2e} of max, bound {self.grad_bound:.2e}, ratio {err / max(self.oracle_grad_dist, 1e-300):.2f}")
        assert err <= self.grad_bound, (what, err, self.grad_bound, self.oracle_grad_dist, self.gmax)


@functools.lru_cache(maxsize=None)
def generated(seed, H, W, sigma=0.03):
    """A frame of the s1 recipe at another size (inputs made in the test, not stored)."""
    return smooth_frame(seed, H, W, sigma)


@functools.lru_cache(maxsize=None)
def generated_expect(seed, H, W, a=1.0, b=1.0, sigma=0.03):
    return Expect(*generated(seed, H, W, sigma), a=a, b=b)
