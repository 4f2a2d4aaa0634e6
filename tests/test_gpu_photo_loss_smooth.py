"""GPU: the photometric loss (csrc/sg_loss.hip) in the regime training runs in -- a smooth render close to a smooth target over a
constant background, SSIM 0.8 to 0.999 -- against the fp64 twin of the oracle, on all three kernels (fused forward + gradient, forward
only, gradient alone), at strip and chunk seams, with a K that changes the chunking, and against the validation metrics.

Every comparison is with fp64 (oracle/photo_loss_oracle.py, ``dtype=torch.float64``); frames, expectations and bounds:
tests/photo_smooth_case.py.  Scalars 2e-6; gradient max(4 x the fp32 oracle's own distance from fp64, 1e-5 x max |grad64|).
Measured on one MI355X (the table: LAB.md "Photometric loss on smooth frames"): SSIM mean within 5.5e-7 of fp64 on every case, the
gradient at 0.15 to 0.63 of the fp32 oracle's own distance.  A library whose window weights are summed left to right in fp32 (the
parent of this file) fails 18 of the 21 tests, each on the SSIM mean: -4.9e-6 to -9.2e-6."""
import os
import re

import numpy as np
import pytest
import torch

from photo_smooth_case import (GOLDEN_CASES, L1_W, SSIM_ATOL, SSIM_W, Expect, generated, generated_expect, l1_tol, smooth_frame)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
S = np.load(os.path.join(HERE, "golden", "photo_loss_smooth_golden.npz"))
UP = (1.7, -0.4)                       # different upstream gradients for the two terms: the gradient-alone kernel


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _gpu(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _fused(dev, raw, gt, mask, bg, images=False):
    """l1 + ssim under one sum: sg_photo_kernel<true>, the backward a multiplication by the shared upstream scalar."""
    from sings_amd.photo_loss import photometric_loss
    r, g, m, b = _gpu(dev, raw, gt, mask, bg)
    r.requires_grad_(True)
    ld, ex = photometric_loss(r, g, m, b, L1_W, SSIM_W, return_images=images)
    (ld["l1"] + ld["ssim"]).backward()
    return ld, ex, r.grad.cpu().numpy()


def _scalars(ld, ex):
    return ld["l1"].item(), ld["ssim"].item(), ex["l1_raw"].item(), ex["ssim_mean"].item()


@pytest.mark.parametrize("tag", sorted(GOLDEN_CASES))
def test_golden_smooth_cases_against_fp64(tag):
    """(a) s1 mid SSIM (-5.91e-6 on a library whose window weights are summed left to right in fp32; s4 -6.50e-6), s2 SSIM 0.9985, s3 dark
    with the clamp at 0, s4 soft silhouette with the clamp at 1: scalars and gradient against fp64, the reference's stored fp32
    scalars at 2e-6, the images exact."""
    dev = _dev()
    raw, gt, mask, bg = (S[f"{tag}_{k}"] for k in ("raw", "gt", "mask", "bg"))
    e = Expect(raw, gt, mask, bg)
    ld, ex, grad = _fused(dev, raw, gt, mask, bg, images=True)
    np.testing.assert_array_equal(ex["gt_img"].cpu().numpy(), S[f"{tag}_gt_img"])
    np.testing.assert_array_equal(ex["pred_img"].cpu().numpy(), np.clip(raw, 0, 1))
    e.check_scalars(tag, *_scalars(ld, ex))
    e.check_grad(tag, grad)
    assert abs(ex["l1_raw"].item() - S[f"{tag}_l1"]) <= 2e-6 * abs(S[f"{tag}_l1"])
    assert abs(ex["ssim_mean"].item() - S[f"{tag}_ssim_mean"]) <= 2e-6
    assert abs(ld["l1"].item() - S[f"{tag}_loss_l1"]) <= 2e-6
    assert abs(ld["ssim"].item() - S[f"{tag}_loss_ssim"]) <= 2e-6


# (b) the gradient kernel emits 54 columns per strip, the forward-only kernel 64; H = 33 is three chunks of 11 rows, 15 / 16 / 17 and
# 31 / 32 / 33 rows sit on either side of one -> two and two -> three chunks
SEAMS = [(W, 33) for W in (53, 54, 55, 63, 64, 65, 108, 109)] + [(55, H) for H in (15, 16, 17, 31, 32)]


@pytest.mark.parametrize("W,H", SEAMS)
def test_seam_shapes_all_three_kernels_against_fp64(W, H):
    from sings_amd.photo_loss import photometric_loss
    dev = _dev()
    seed = 1000 + 7 * W + H
    raw, gt, mask, bg = generated(seed, H, W)
    e = generated_expect(seed, H, W)
    what = f"{W}x{H}"
    # fused
    ld, ex, grad = _fused(dev, raw, gt, mask, bg)
    fused = _scalars(ld, ex)
    e.check_scalars(what + " fused", *fused)
    e.check_grad(what + " fused", grad)
    # forward only: `raw` does not require grad
    r, g, m, b = _gpu(dev, raw, gt, mask, bg)
    ld, ex = photometric_loss(r, g, m, b, L1_W, SSIM_W, return_images=True)
    fwd = _scalars(ld, ex)
    np.testing.assert_array_equal(ex["pred_img"].cpu().numpy(), e.pred_img)
    np.testing.assert_array_equal(ex["gt_img"].cpu().numpy(), e.gt_img)
    e.check_scalars(what + " forward-only", *fwd)
    for k, (a_, b_) in enumerate(zip(fwd, fused)):
        tol = 2 * (l1_tol(b_) if k in (0, 2) else SSIM_ATOL)
        assert abs(a_ - b_) <= tol, (what, k, a_, b_)
    # gradient alone: different upstream weights for the two terms
    e2 = generated_expect(seed, H, W, *UP)
    r.requires_grad_(True)
    ld, ex = photometric_loss(r, g, m, b, L1_W, SSIM_W)
    (UP[0] * ld["l1"] + UP[1] * ld["ssim"]).backward()
    e2.check_scalars(what + " gradient-alone (its forward)", *_scalars(ld, ex))
    e2.check_grad(what + " gradient-alone", r.grad.cpu().numpy())


def _loss_units():
    src = open(os.path.join(HERE, "..", "sings_amd", "csrc", "sg_loss.hip")).read()
    return int(re.search(r"^#define SG_LOSS_UNITS (\d+)", src, re.M).group(1))


def _rows_per_chunk(K, W, H, units, nout=54):
    nstrips = (W + nout - 1) // nout
    nch = max(1, min(units // (3 * nstrips * K), (H + 15) // 16))
    return (H + nch - 1) // nch


def test_k_frames_with_another_chunking_than_one_frame():
    """(c) K = 16 frames of 1080 x 64 are two chunks of 32 rows each, one frame alone four chunks of 16.  A pixel's sums run in the same
    order whatever the chunk, so the gradients are bit-equal to 16 single calls.  The four scalars are NOT asserted bit-equal: they are
    fixed-order sums of fp32 per-wave partials, and a wave that sums 32 rows rounds differently from two that sum 16 each; they are
    held to fp64 like every other scalar here."""
    from sings_amd import _lib
    from sings_amd.photo_loss import photometric_loss, photometric_loss_frames
    dev = _dev()
    K, W, H = 16, 1080, 64
    units = _loss_units()
    # the library was built from that source: workspace = 1024 + (units + 3 strips + 8) x 16 rounded to 256, + 256
    assert int(_lib.load().sg_photo_loss_ws_bytes(W, H)) == 1024 + ((units + 3 * 20 + 8) * 16 + 255) // 256 * 256 + 256
    assert _rows_per_chunk(K, W, H, units) == 32 and _rows_per_chunk(1, W, H, units) == 16
    assert K == _lib.MAX_FRAMES
    frames = [smooth_frame(500 + f, H, W, 0.03 if f % 2 else 0.003) for f in range(K)]
    raw, gt, mask = (np.stack([fr[i] for fr in frames]) for i in range(3))
    bg = frames[0][3]
    a = np.linspace(-1.0, 2.0, K).astype(np.float32); b = np.linspace(1.5, -0.5, K).astype(np.float32)
    tr, tg, tm, tb, ta, tbb = _gpu(dev, raw, gt, mask, bg, a, b)
    r1 = tr.clone().requires_grad_(True)
    tot = 0
    for f in range(K):
        ld, _ = photometric_loss(r1[f], tg[f], tm[f], tb, L1_W, SSIM_W)
        tot = tot + ta[f] * ld["l1"] + tbb[f] * ld["ssim"]
    tot.backward()
    r2 = tr.clone().requires_grad_(True)
    ld, ex = photometric_loss_frames(r2, tg, tm, tb, L1_W, SSIM_W)
    ((ta * ld["l1"]).sum() + (tbb * ld["ssim"]).sum()).backward()
    assert torch.equal(r2.grad, r1.grad)
    l1, ss, l1r, sm = (t.detach().cpu().numpy() for t in (ld["l1"], ld["ssim"], ex["l1_raw"], ex["ssim_mean"]))
    g = r2.grad.cpu().numpy()
    for f in range(K):
        e = Expect(*frames[f], a=float(a[f]), b=float(b[f]), grad=f == 1)
        e.check_scalars(f"K=16 frame {f}", float(l1[f]), float(ss[f]), float(l1r[f]), float(sm[f]))
        if f == 1:                                             # (every other frame: bit-equal to its single call, above)
            e.check_grad(f"K=16 frame {f}", g[f])


@pytest.mark.parametrize("case", ["s1", "250x131"])
def test_training_and_validation_agree_on_ssim(case):
    """(d) sg_loss.hip and sg_metrics.hip are fp32 marches with the same window weights (one host helper); only the summation of the
    SSIM values differs -- fp32 partials per wave there, fp64 here -- so the two SSIM means of one frame agree to 5e-7 (the metrics
    kernel's own distance from the oracle is 2e-9 to 1.2e-7: LAB.md).  With left-to-right weights on one side it was about 5e-6."""
    from sings_amd.metrics import image_metrics
    from sings_amd.photo_loss import photometric_loss
    dev = _dev()
    raw, gt, mask, bg = [S[f"s1_{k}"] for k in ("raw", "gt", "mask", "bg")] if case == "s1" else generated(77, 131, 250)
    r, g, m, b = _gpu(dev, raw, gt, mask, bg)
    _, ex = photometric_loss(r, g, m, b, L1_W, SSIM_W, return_images=True)
    with torch.no_grad():
        val = image_metrics(r, ex["gt_img"])["ssim"][0].item()
    train = ex["ssim_mean"].item()
    print(f"{case}: training {train:.8f} validation {val:.8f} difference {train - val:+.2e}")
    assert abs(train - val) <= 5e-7, (train, val)
    r.requires_grad_(True)
    _, ex2 = photometric_loss(r, g, m, b, L1_W, SSIM_W)
    print(f"{case}: fused kernel {ex2['ssim_mean'].item():.8f} difference {ex2['ssim_mean'].item() - val:+.2e}")
    assert abs(ex2["ssim_mean"].item() - val) <= 5e-7, (ex2["ssim_mean"].item(), val)


def test_smooth_frame_is_deterministic():
    """(e) two calls, bit-equal scalars and gradient (no atomics, fixed-order sums), on a frame with flat background rows (the
    repeated-row path of the gradient kernel's first wave) next to the silhouette."""
    dev = _dev()
    raw, gt, mask, bg = generated(77, 131, 250)
    ld1, ex1, g1 = _fused(dev, raw, gt, mask, bg)
    ld2, ex2, g2 = _fused(dev, raw, gt, mask, bg)
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    for k in ("l1", "ssim"):
        assert torch.equal(ld1[k], ld2[k])
    for k in ("l1_raw", "ssim_mean"):
        assert torch.equal(ex1[k], ex2[k])
