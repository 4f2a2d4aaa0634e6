"""CPU: the fp64 twin of the photometric-loss oracle, and the smooth-frame golden cases produced by the reference's own l1_loss / ssim
(tests/golden/gen_photo_loss_golden.py -> photo_loss_smooth_golden.npz; the recipe: tests/photo_smooth_case.py)."""
import os

import numpy as np
import torch

from oracle import photo_loss_oracle as plo
from photo_smooth_case import GOLDEN_CASES, Expect, left_to_right_taps

HERE = os.path.dirname(__file__)
G = np.load(os.path.join(HERE, "golden", "photo_loss_golden.npz"))
S = np.load(os.path.join(HERE, "golden", "photo_loss_smooth_golden.npz"))


def _inputs(Z, tag):
    return Z[f"{tag}_raw"], Z[f"{tag}_gt"], Z[f"{tag}_mask"], Z[f"{tag}_bg"]


def test_twin_window_is_the_reference_window_cast_up():
    g = G["window_1d"]
    w = plo.window(3, dtype=torch.float64)
    assert w.dtype == torch.float64 and w.shape == (3, 1, 11, 11)
    np.testing.assert_array_equal(w[0, 0].numpy(), g.astype(np.float64)[:, None] * g.astype(np.float64)[None, :])
    # the left-to-right weights: nine of the eleven one ulp above the reference's, none below
    ulps = left_to_right_taps().view(np.int32) - g.view(np.int32)
    assert sorted(ulps.tolist()) == [0, 0] + [1] * 9 and ulps.tolist() == ulps[::-1].tolist(), ulps


def test_twin_agrees_with_fp32_oracle_on_noise_cases():
    """On uniform noise (SSIM near 0) the fp32 oracle is as accurate as tests/test_oracle_photo_loss.py holds it to the reference:
    1e-6 on the scalars; the gradient within 1e-5 of its maximum (what tests/test_gpu_photo_loss.py allows the kernel there)."""
    for tag in "abc":
        e = Expect(*_inputs(G, tag))
        print(tag, {k: e.s32[k] - e.s64[k] for k in e.s64}, e.oracle_grad_dist / e.gmax)
        assert abs(e.s32["l1_raw"] - e.s64["l1_raw"]) <= 1e-6 * e.s64["l1_raw"]
        assert abs(e.s32["ssim_mean"] - e.s64["ssim_mean"]) <= 1e-6
        assert abs(e.s32["l1"] - e.s64["l1"]) <= 1e-6 and abs(e.s32["ssim"] - e.s64["ssim"]) <= 1e-6
        assert e.oracle_grad_dist <= 1e-5 * e.gmax
        np.testing.assert_array_equal(e.gt_img, G[f"{tag}_gt_img"])


def test_oracle_matches_reference_on_smooth_cases():
    assert sorted(GOLDEN_CASES) == ["s1", "s2", "s3", "s4"]
    for tag, kw in GOLDEN_CASES.items():
        assert S[f"{tag}_raw"].shape == (3, kw["H"], kw["W"])
        raw = torch.from_numpy(S[f"{tag}_raw"]).requires_grad_(True)
        o = plo.photometric_loss(raw, torch.from_numpy(S[f"{tag}_gt"]), torch.from_numpy(S[f"{tag}_mask"]),
                                 torch.from_numpy(S[f"{tag}_bg"]), float(S["weights"][0]), float(S["weights"][1]))
        (o["l1"] + o["ssim"]).backward()
        np.testing.assert_array_equal(o["gt_img"].detach().numpy(), S[f"{tag}_gt_img"])
        assert abs(o["l1_raw"].item() - S[f"{tag}_l1"]) <= 1e-6 * abs(S[f"{tag}_l1"])
        assert abs(o["ssim_mean"].item() - S[f"{tag}_ssim_mean"]) <= 1e-6
        assert abs(o["l1"].item() - S[f"{tag}_loss_l1"]) <= 1e-6 and abs(o["ssim"].item() - S[f"{tag}_loss_ssim"]) <= 1e-6
        np.testing.assert_allclose(raw.grad.numpy(), S[f"{tag}_grad"], rtol=1e-5, atol=1e-9)


def test_smooth_cases_are_in_their_regimes():
    e = {tag: Expect(*_inputs(S, tag)) for tag in GOLDEN_CASES}
    assert 0.8 < e["s1"].s64["ssim_mean"] < 0.9 and 0.99 < e["s2"].s64["ssim_mean"] < 0.9995
    assert (S["s3_bg"] == 0).all() and 0.0 <= S["s3_gt"].min() and S["s3_gt"].max() <= 0.02 and (S["s3_raw"] < 0).sum() > 20
    rim = (S["s4_mask"] > 0) & (S["s4_mask"] < 1)
    assert rim.sum() > 300 and np.unique(S["s4_mask"][rim]).size > 100 and (S["s4_bg"] == 1).all()
    for tag in ("s1", "s2", "s3"):
        assert set(np.unique(S[f"{tag}_mask"])) == {0.0, 1.0}


def test_s1_exposes_left_to_right_window_weights():
    """The condition that makes the GPU test of s1 fail on a library with the left-to-right fp32 weights: evaluated in fp64, those
    weights move the SSIM mean of s1 by at least 4e-6 -- twice the 2e-6 the GPU test allows -- while the fp32 oracle stays within
    2e-6 of the twin."""
    e = Expect(*_inputs(S, "s1"))
    t = [torch.from_numpy(v) for v in _inputs(S, "s1")]
    wrong = plo.photometric_loss(t[0].double(), *t[1:], dtype=torch.float64, taps=left_to_right_taps())["ssim_mean"].item()
    print("s1: ssim", e.s64["ssim_mean"], "left-to-right weights", wrong - e.s64["ssim_mean"], "fp32 oracle", e.s32["ssim_mean"] - e.s64["ssim_mean"])
    assert abs(wrong - e.s64["ssim_mean"]) >= 4e-6
    assert abs(e.s32["ssim_mean"] - e.s64["ssim_mean"]) <= 2e-6


def test_twin_in_two_passes_is_the_twin():
    """The twin's scalars on large frames come from two 11-tap passes (tests/photo_smooth_case.py, ``grad=False``): the same numbers
    to 1e-13, a hundred million times below the bounds they serve."""
    for tag in ("s1", "s3", "s4"):
        a, b = Expect(*_inputs(S, tag)), Expect(*_inputs(S, tag), grad=False)
        for k in a.s64:
            assert abs(a.s64[k] - b.s64[k]) <= 1e-13, (tag, k, a.s64[k], b.s64[k])
