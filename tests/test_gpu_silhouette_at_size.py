"""The soft silhouette at the size the pose refinement exists for: 512 x 896, ``octa_level(5)`` (8 192 faces) spanning about 400
pixels, K = 1, one forward and one backward -- a test of its own, to be run on its own.

The host twin cannot evaluate 458 752 x 8 192 pairs, so the comparison is made on two 48 x 48 windows, one across the outline and one
inside, with dL/dalpha zero outside them.  A crop of the picture IS the twin's picture of the window's own camera: principal point
(cx - x0, cy - y0) and sigma (min(H, W) / 48)^2 (the NDC unit follows the shorter side, so sigma is rescaled to keep distance^2 / sigma
what it was).  The twin gets only the faces whose grown bounding box meets the window's tiles; the others contribute the factor 1 to
every pixel of it.  Held: alpha in the windows and the whole dL/dverts_cam, by ``body_case.held``."""
import numpy as np
import pytest
import torch

import body_case as bc
import silhouette_case as sc
from sings_amd import silhouette as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W, H, SIGMA = 512, 896, 1e-4
INTR = (600.0, 600.0, 256.3, 447.6)
WIN = 48
WINDOWS = ((432, 32), (432, 240))                # (y0, x0), multiples of 16: across the outline at the left tip, and inside


def test_at_kit_size_on_two_windows():
    v, faces, _ = bc.octa_level(5)
    verts = (1.33 * v + np.array([0.0, 0.0, 4.0])).astype(np.float32)[None]
    assert len(faces) == 8192
    pairs, lengths = S.pair_counts_host(verts, faces, INTR, H, W, SIGMA)
    capacity = 2 * int(pairs.sum())
    plan = S.workspace_plan(1, verts.shape[1], len(faces), H, W, capacity)
    print(f"host count: {int(pairs[0])} pairs, {int((lengths > 0).sum())} tiles in use, longest list {int(lengths.max())}; capacity {capacity}, "
          f"workspace {plan['bytes']} bytes")
    span = verts[0, :, 0].max() - verts[0, :, 0].min()
    assert 380 < span * INTR[0] / 4.0 < 420
    _, x0, y0, x1, y1 = S._host_rects(verts, faces, INTR, H, W, SIGMA)
    g = np.zeros((1, H, W), np.float32)
    wins = []
    for wy, wx in WINDOWS:
        tx0, ty0 = wx // 16, wy // 16
        sub = np.nonzero((x0[0] <= tx0 + 2) & (x1[0] >= tx0) & (y0[0] <= ty0 + 2) & (y1[0] >= ty0))[0]
        tw = sc.twins(verts, faces[sub], (INTR[0], INTR[1], INTR[2] - wx, INTR[3] - wy), WIN, WIN, SIGMA * (min(H, W) / WIN) ** 2,
                      seed=wy + wx)
        g[0, wy:wy + WIN, wx:wx + WIN] = tw["g"][0]
        wins.append(tw)
        print(f"window at ({wx}, {wy}): {len(sub)} faces, alpha from {tw['alpha64'].min():.3f} to {tw['alpha64'].max():.3f}")
    assert wins[0]["alpha64"].min() < 1e-3 and wins[0]["alpha64"].max() > 0.999 and wins[1]["alpha64"].min() > 0.99

    f32 = torch.from_numpy(faces).to(DEV, torch.int32)
    work = S.SilhouetteWorkspace(1, verts.shape[1], f32, H, W, capacity, DEV)
    assert work.ws.numel() == plan["bytes"]
    vt = torch.from_numpy(verts).to(DEV).requires_grad_(True)
    alpha = S.soft_silhouette(vt, f32, INTR, H, W, SIGMA, workspace=work, check=False)
    alpha.backward(torch.from_numpy(g).to(DEV))
    torch.cuda.synchronize()
    over, total, per_frame = work.info()
    assert not over and total == pairs[0] and np.array_equal(work.tile_lengths(), lengths) and work.guards_intact()
    a = alpha.detach().cpu().numpy()
    for (wy, wx), tw in zip(WINDOWS, wins):
        sc.check_alpha(a[:, wy:wy + WIN, wx:wx + WIN], tw, f"window at ({wx}, {wy})")
    bc.held(vt.grad.cpu().numpy(), wins[0]["grad32"] + wins[1]["grad32"], wins[0]["grad64"] + wins[1]["grad64"], "at size dL/dverts_cam")
    assert a.min() == 0.0 and a.max() > 0.999 and 0.12 < a.mean() < 0.22        # (the outline encloses 0.17 of the picture)
