"""GPU tests of the validation metrics launch (``sings_amd.metrics``, csrc/sg_metrics.hip) against fp64 numpy, the CPU oracle of the
SSIM window (oracle/photo_loss_oracle.py) and the reference's own figures (tests/golden/metrics_golden.npz).

Tolerances, derived:
  MSE   per channel against fp64 numpy on the same fp32 (clamped, masked) images: relative 5e-7 -- the kernel's difference x - y is
        fp32 (relative 2^-24 in the difference, 2^-23 = 1.2e-7 in its square, at worst in every pixel alike); the square, the sums
        and the division are fp64 and the result is rounded once to fp32 (6e-8).
  PSNR  against 20 log10(1 / sqrt(mse64)): 2.2e-6 + 2^-23 |psnr| dB = 10 / ln 10 times the MSE bound, plus one rounding to fp32.
  PSNR  against the golden (the reference's fp32 chain): that bound plus 2 x the case's ``psnr_ref_err`` (what the generator measured
        the reference's chain to be off by; the factor covers a torch build whose log10 differs by an ulp).
  SSIM  mean against the oracle's ``ssim_map(...).mean()`` on the CPU and against the golden: 2e-6 absolute, the bar
        tests/test_gpu_photo_loss.py holds the same window scheme to.
Shapes: smaller than the window; one column fewer than, exactly, and one more than a strip (``metrics.STRIP_COLS``); one row fewer
than, exactly, and one more than a chunk (``metrics.CHUNK_ROWS``); ragged; one 512 x 896 and one 1920 x 1080 frame."""
import os

import numpy as np
import pytest
import torch

from metrics_case import R, S, SSIM_ATOL, check_row, expected, frame, psnr_tol
from sings_amd import metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_golden.npz")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


SHAPES = [(8, 5), (11, 10), (S - 1, 20), (S, 20), (S + 1, 20), (40, R - 1), (40, R), (40, R + 1), (S + 1, R + 1), (250, 131)]


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_small_shapes_against_fp64_and_the_oracle(W, H, masked):
    raw, gt, mask = frame(100 + W + 7 * H, H, W)
    m = mask if masked else None
    out = metrics.image_metrics(t(raw), t(gt), None if m is None else t(m))
    assert out["psnr"].shape == (1,) and out["mse_channels"].shape == (1, 3) and out["psnr_channels"].shape == (1, 3)
    row = torch.cat([out["mse_channels"][0], out["psnr_channels"][0], out["psnr"], out["ssim"]]).cpu().numpy()
    check_row(row, expected(raw, gt, m), f"{W}x{H}{' masked' if masked else ''}")


@pytest.mark.parametrize("W,H", [(512, 896), (1920, 1080)])
def test_full_frames_against_the_cpu_oracle(W, H):
    raw, gt, mask = frame(5, H, W, smooth=True)
    row = metrics.image_metrics_table(t(raw), t(gt))[0].cpu().numpy()
    check_row(row, expected(raw, gt, None), f"{W}x{H}")
    assert 0.1 < row[7] < 0.95                                       # a structured frame: the SSIM figure is not the one of noise


def test_golden_cases():
    """The reference's own fp32 figures.  Measured worst differences on the MI355X over the five cases: PSNR 9.5e-7 dB (case b;
    bounds 4.0e-6 to 9.7e-6), SSIM mean 1.2e-7 (case zju), MSE 1.4e-7 relative to the reference's fp32 mean (case c)."""
    G = np.load(GOLDEN)
    for tag in (str(c) for c in G["cases"]):
        raw, gt = G[f"{tag}_raw"], G[f"{tag}_gt"]
        mask = G[f"{tag}_mask"] if f"{tag}_mask" in G else None
        row = metrics.image_metrics_table(t(raw), t(gt), None if mask is None else t(mask))[0].cpu().numpy().astype(np.float64)
        ref_p = np.concatenate([G[f"{tag}_psnr"], [G[f"{tag}_psnr_mean"]]]).astype(np.float64)
        extra = 2.0 * float(G[f"{tag}_psnr_ref_err"])
        finite = np.isfinite(ref_p)
        print(f"golden {tag}: psnr {np.abs(row[3:7][finite] - ref_p[finite]).max():.2e} dB (ref err {extra / 2:.2e}), "
              f"ssim {abs(row[7] - float(G[f'{tag}_ssim_mean'])):.2e}, "
              f"mse rel {np.abs(row[0:3] / np.maximum(G[f'{tag}_mse'], 1e-30) - 1)[G[f'{tag}_mse'] > 0].max():.2e}")
        for i in range(4):
            if finite[i]:
                assert abs(row[3 + i] - ref_p[i]) <= psnr_tol(ref_p[i]) + extra, (tag, i, row[3 + i], ref_p[i])
            else:
                assert np.isposinf(row[3 + i]), (tag, i, row[3 + i])
        assert abs(row[7] - float(G[f"{tag}_ssim_mean"])) <= SSIM_ATOL, tag
        # the reference's fp32 mse (a float32 mean over H W values) is itself only good to its own rounding: fp64 numpy decides
        if finite.all():
            check_row(row, expected(raw, gt, mask), f"golden {tag} vs fp64")
        if tag == "exact":
            assert row[1] == 0.0 and np.isposinf(row[4]) and np.isposinf(row[6]) and np.isfinite(row[[3, 5]]).all()


@pytest.mark.parametrize("shared_gt", [True, False])
@pytest.mark.parametrize("mask_kind", ["none", "shared", "per_frame"])
def test_five_frames_in_one_launch_equal_five_launches(shared_gt, mask_kind):
    K, W, H = 5, S + 6, R + 13                                        # two strips, two chunks
    fr = [frame(40 + k, H, W) for k in range(K)]
    raw = t(np.stack([f[0] for f in fr]))
    gt = t(fr[0][1]) if shared_gt else t(np.stack([f[1] for f in fr]))
    mask = None if mask_kind == "none" else t(fr[0][2]) if mask_kind == "shared" else t(np.stack([f[2] for f in fr]))
    batch = metrics.image_metrics_table(raw, gt, mask)
    assert batch.shape == (K, 8)
    for k in range(K):
        one = metrics.image_metrics_table(raw[k], gt if shared_gt else gt[k], mask if mask_kind != "per_frame" else mask[k])
        assert torch.equal(batch[k], one[0]), (k, batch[k], one[0])
    # a frame's bits do not depend on its position in the batch either
    perm = [3, 0, 4, 2, 1]
    moved = metrics.image_metrics_table(raw[perm], gt if shared_gt else gt[perm], mask[perm] if mask_kind == "per_frame" else mask)
    assert torch.equal(moved, batch[perm])
    assert len({float(v) for v in batch[:, 7]}) == K                  # (the frames differ)
    check_row(batch[K - 1].cpu().numpy(), expected(fr[K - 1][0], fr[0][1] if shared_gt else fr[K - 1][1],
                                                   None if mask_kind == "none" else fr[0][2] if mask_kind == "shared" else fr[K - 1][2]),
              f"frame {K - 1} of the batch")


def test_two_calls_give_the_same_bits_and_mask_layouts_agree():
    raw, gt, mask = frame(9, 131, 250)
    a = metrics.image_metrics_table(t(raw), t(gt), t(mask))
    b = metrics.image_metrics_table(t(raw), t(gt), t(mask))
    assert torch.equal(a, b)
    assert torch.equal(a, metrics.image_metrics_table(t(raw)[None], t(gt)[None], t(mask)[None, None]))      # [K,1,H,W]
    assert torch.equal(a, metrics.image_metrics_table(t(raw), t(gt), t(mask)[None]))                        # [1,H,W]
    with pytest.raises(ValueError):
        metrics.image_metrics(t(raw), t(gt)[:, :-1])
    with pytest.raises(ValueError):
        metrics.image_metrics(t(raw), t(gt), t(mask)[:-1])
    with pytest.raises(RuntimeError, match="not differentiable"):
        metrics.image_metrics(t(raw).requires_grad_(True), t(gt))
    with torch.no_grad():
        assert torch.equal(metrics.image_metrics_table(t(raw).requires_grad_(True), t(gt), t(mask)), a)


@pytest.mark.parametrize("masked", [False, True])
def test_clamp_off_on_clamped_input_equals_clamp_on(masked):
    raw, gt, mask = frame(11, R + 5, S + 9)
    m = t(mask) if masked else None
    on = metrics.image_metrics_table(t(raw), t(gt), m, clamp=True)
    off = metrics.image_metrics_table(t(np.clip(raw, 0, 1)), t(gt), m, clamp=False)
    assert torch.equal(on, off)
    unclamped = metrics.image_metrics_table(t(raw), t(gt), m, clamp=False)
    assert not torch.equal(on, unclamped)
    check_row(unclamped[0].cpu().numpy(), expected(raw, gt, mask if masked else None, clamp=False), "clamp off")


def test_engine_in_a_captured_graph_equals_the_eager_call():
    """No host synchronisation: a MetricsEngine call captured on one stream, replayed after its input buffers were overwritten."""
    K, W, H = 3, S + 6, R + 13
    sets = [[frame(70 + 10 * j + k, H, W) for k in range(K)] for j in range(2)]
    stack = lambda j, i: t(np.stack([f[i] for f in sets[j]]))
    raw_s, gt_s, mask_s = stack(0, 0), stack(0, 1), stack(0, 2)
    eng = metrics.MetricsEngine(W, H, DEV, K=K)
    ref = [metrics.image_metrics_table(stack(j, 0), stack(j, 1), stack(j, 2)).clone() for j in range(2)]
    assert torch.equal(eng(raw_s, gt_s, mask_s), ref[0])
    side = torch.cuda.Stream(DEV); side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eng(raw_s, gt_s, mask_s)
    torch.cuda.current_stream(DEV).wait_stream(side); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng(raw_s, gt_s, mask_s)
    for j in (1, 0, 1):
        raw_s.copy_(stack(j, 0)); gt_s.copy_(stack(j, 1)); mask_s.copy_(stack(j, 2))
        eng.table.zero_()
        g.replay(); torch.cuda.synchronize()
        assert torch.equal(out, ref[j]), j
    assert not torch.equal(ref[0], ref[1])
    with pytest.raises(ValueError):
        eng(raw_s[:2], gt_s, mask_s)
