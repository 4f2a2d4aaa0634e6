"""GPU tests of the validation driver (``sings_amd.validate``): a small skinned scene, F = 5 frames with different poses and cameras
in chunks of 3 and 2, checked per frame against a one-frame path -- ``get_render_pkg_fused`` alone, PSNR and SSIM by the CPU oracle
at the tolerances of tests/test_gpu_metrics.py, LPIPS by a direct call of the same network on the same tensors (bit-equal)."""
import numpy as np
import pytest
import torch

from lpips_case import make_weights
from metrics_case import check_row, expected

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W, H, F, J, N = 64, 48, 5, 24, 2500


@pytest.fixture(scope="module")
def case():
    from sings_amd.body import joint_transforms
    from sings_amd.camera import make_camera
    from sings_amd.lpips import LPIPS
    from sings_amd.renderer import get_render_pkg_fused
    from sings_amd.scene import avatar_scene
    s = avatar_scene(N=N, J=J, W=W, H=H, seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rs = np.random.RandomState(21)
    canon = dict(xyz_canon=t(s["xyz_canon"]), rotmat_canon=None, scales=t(s["scales"]), opacity=t(s["opacities"]), shs=t(s["shs"]),
                 lbs_weights=t(s["lbs_weights"]), active_sh_degree=0)
    jr = t(s["joints_rest"])
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    frames = []
    for f in range(F):
        V = np.eye(4, dtype=np.float32); V[3, 0] = 0.03 * f; V[3, 1] = -0.02 * f
        cm = make_camera(V, 250.0, 250.0, W / 2, H / 2, W, H)
        d = dict(fovx=cm["fovx"], fovy=cm["fovy"], image_height=H, image_width=W, world_view_transform=t(cm["world_view_transform"]),
                 full_proj_transform=t(cm["full_proj_transform"]), camera_center=t(cm["camera_center"]))
        d["A_cano2pose"] = joint_transforms(t(rs.normal(0, 0.2, J * 3).astype(np.float32)), jr, tuple(s["parents"]))
        d["transl"] = t(s["transl"] + rs.normal(0, 0.02, 3).astype(np.float32))
        frames.append(d)
    # targets: the frame rendered with another pose noise-free would be a still better stand-in; a render of the frame itself plus
    # noise keeps PSNR / SSIM in the range validation sees (20-30 dB), and values outside [0,1] do not occur in a dataset
    one = []
    with torch.no_grad():
        for d in frames:
            one.append(get_render_pkg_fused(d, canon, d["A_cano2pose"], bg, transl=d["transl"]))
    for d, pkg in zip(frames, one):
        noise = torch.from_numpy(rs.normal(0, 0.05, (3, H, W)).astype(np.float32)).to(DEV)
        d["rgb"] = torch.clamp(pkg["render"] + noise, 0.0, 1.0)
        d["mask"] = t(np.clip(rs.uniform(-0.5, 1.5, (1, H, W)), 0, 1).astype(np.float32))
    wt = make_weights(seed=3)
    lp = LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"], device=DEV)
    return dict(canon=canon, frames=frames, bg=bg, one=one, lpips=lp)


def test_chunked_frames_equal_the_one_frame_renders(case):
    """What ``validate`` relies on: a frame rendered in a chunk of 3 or 2 has the bits of the frame rendered alone."""
    from sings_amd.renderer import get_render_pkgs_fused
    fr = case["frames"]
    with torch.no_grad():
        for c0 in (0, 3):
            chunk = fr[c0:c0 + 3]
            pk = get_render_pkgs_fused(chunk, case["canon"], torch.stack([d["A_cano2pose"] for d in chunk]), case["bg"],
                                       transl=torch.stack([d["transl"] for d in chunk]))
            for k in range(len(chunk)):
                assert torch.equal(pk["render_raw"][k], case["one"][c0 + k]["render_raw"]), c0 + k
                assert torch.equal(pk["render"][k], case["one"][c0 + k]["render"]), c0 + k
    assert float(case["one"][0]["render_raw"].max()) > 0.35           # (the avatar is in the frame)


@pytest.mark.parametrize("mask_images", [False, True])
def test_validate_rows_against_the_one_frame_path(case, mask_images, tmp_path):
    from sings_amd.validate import Validator, validate
    fr, lp = case["frames"], case["lpips"]
    res = validate(case["canon"], fr, bg_color=case["bg"], lpips=lp, frames_per_launch=3, mask_images=mask_images)
    assert set(res) == {"psnr", "ssim", "lpips", "per_frame"} and set(res["per_frame"]) == {"psnr", "ssim", "lpips"}
    rows = res["per_frame"]
    for key in ("psnr", "ssim", "lpips"):
        assert rows[key].shape == (F,) and rows[key].dtype == torch.float32 and rows[key].device.type == "cpu"
        # the reported figure: the fp64 mean of the fp32 per-frame values, as torch.stack(v).mean().item() of the reference
        assert isinstance(res[key], float) and res[key] == torch.stack([v.double() for v in rows[key]]).mean().item()
    for f, (d, pkg) in enumerate(zip(fr, case["one"])):
        raw, gt = pkg["render_raw"], d["rgb"]
        m = d["mask"][0].cpu().numpy() if mask_images else None
        mse, psnr, pmean, ssim = expected(raw.cpu().numpy(), gt.cpu().numpy(), m)
        # (the driver keeps the two report columns of the table; the channel columns are tests/test_gpu_metrics.py's)
        row = np.concatenate([mse, psnr, [float(rows["psnr"][f]), float(rows["ssim"][f])]])
        check_row(row, (mse, psnr, pmean, ssim), f"frame {f}{' masked' if mask_images else ''}")
        image, target = torch.clamp(raw, 0.0, 1.0), gt
        if mask_images:
            image, target = image * d["mask"], target * d["mask"]
        with torch.no_grad():
            direct = lp(image.clip(max=1), target).reshape(())
        assert float(direct) == float(rows["lpips"][f]), (f, float(direct), float(rows["lpips"][f]))
    assert 15.0 < res["psnr"] < 40.0 and 0.0 < res["lpips"]
    # Validator by hand in the same chunks, and the file of the reference
    val = Validator(W, H, DEV, lpips=lp, frames_per_launch=3, mask_images=mask_images)
    for c0 in (0, 3):
        val.add(torch.stack([p["render_raw"] for p in case["one"][c0:c0 + 3]]), torch.stack([d["rgb"] for d in fr[c0:c0 + 3]]),
                torch.stack([d["mask"] for d in fr[c0:c0 + 3]]) if mask_images else None)
    assert len(val) == F
    again = val.result()
    for key in ("psnr", "ssim", "lpips"):
        assert again[key] == res[key] and torch.equal(again["per_frame"][key], rows[key])
    path = str(tmp_path / "eval_final.pth")
    val.save(path)
    saved = torch.load(path)
    assert set(saved) == {"lpips", "psnr", "ssim"}
    for key, lst in saved.items():
        assert isinstance(lst, list) and len(lst) == F
        assert all(v.dtype == torch.float64 and v.dim() == 0 and v.device.type == "cpu" for v in lst)
        assert torch.stack(lst).mean().item() == res[key]              # gs_trainer.py:605-606 on the loaded file
        assert torch.equal(torch.stack(lst), rows[key].double())
    with pytest.raises(ValueError):
        val.add(torch.zeros(4, 3, H, W, device=DEV), torch.zeros(3, H, W, device=DEV))      # more than frames_per_launch


def test_without_a_network_the_key_is_absent_and_sizes_must_agree(case, tmp_path):
    from sings_amd.validate import Validator, validate
    fr = case["frames"]
    res = validate(case["canon"], fr, bg_color=case["bg"], frames_per_launch=3)
    assert set(res) == {"psnr", "ssim", "per_frame"} and set(res["per_frame"]) == {"psnr", "ssim"}
    full = validate(case["canon"], fr, bg_color=case["bg"], frames_per_launch=8)              # one chunk of 5
    assert full["psnr"] == res["psnr"] and torch.equal(full["per_frame"]["ssim"], res["per_frame"]["ssim"])
    val = Validator(W, H, DEV)
    val.add(case["one"][0]["render_raw"], fr[0]["rgb"])
    path = str(tmp_path / "eval.pth")
    val.save(path)
    saved = torch.load(path)
    assert saved["lpips"] == [] and len(saved["psnr"]) == 1 and float(saved["psnr"][0]) == float(res["per_frame"]["psnr"][0])
    # the default background is zeros (gs_trainer.py:549): another image than with this case's background
    zeros = validate(case["canon"], fr[:1], frames_per_launch=3)
    assert zeros["psnr"] != float(res["per_frame"]["psnr"][0])
    other = dict(fr[1]); other["image_width"] = W + 16
    with pytest.raises(ValueError, match="one image size"):
        validate(case["canon"], [fr[0], other], bg_color=case["bg"])
    other = dict(fr[1]); other["rgb"] = fr[1]["rgb"][:, :-1]
    with pytest.raises(ValueError, match="one image size"):
        validate(case["canon"], [fr[0], other], bg_color=case["bg"])
    with pytest.raises(ValueError):
        validate(case["canon"], fr, bg_color=case["bg"], frames_per_launch=17)
    with pytest.raises(ValueError):
        Validator(W, H, DEV, mask_images=True).add(case["one"][0]["render_raw"], fr[0]["rgb"])
