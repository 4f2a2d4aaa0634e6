"""Generates tests/golden/pose_refine_golden.npz and tests/golden/pose_refine_keypoints_000000.json from a checkout of the reference (beside
this repository, or where ``SINGS_REFERENCE`` points).  The reference source never ships; only these arrays do.

From its shipped kit ``examples/training_kits/f_2``: ``poses.npz`` and ``poses_optimized.npz`` (every array), ``cameras.npz``, and the
keypoints and scores of frames 0-3 as arrays; one keypoint file is copied as it is, for the parser test.

RESULTS of the reference's own functions: ``turn_smpl_gradient_on``, ``clip_smpl_vals`` and ``coco133_to_smpl`` of
``preprocess/utils/ooptimize_smpl.py``, the first two and ``coco133_to_smplh`` of ``ooptimize_smplh.py``.  The scripts cannot be imported
(their module-level imports need pytorch3d), so each function is cut out of its file with ``ast`` and executed on its own with numpy
and torch in scope.  The keypoint map is recovered from an ``arange`` input: row r of the result holds the COCO index that lands there
(0: none -- COCO index 0, the nose, is used by neither table).
"""
import ast
import glob
import json
import os
import shutil

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SINGS_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
KIT = os.path.join(REF, "examples", "training_kits", "f_2")


def cut(path, names):
    """The functions ``names`` of the file, compiled alone -> dict name -> function."""
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), (path, names)
    scope = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), scope)
    return {n: scope[n] for n in names}


def recorded(script, map_name, prefix, out):
    fns = cut(os.path.join(REF, "preprocess", "utils", script), ["turn_smpl_gradient_on", "clip_smpl_vals", map_name])
    out[prefix + "grad_mask"] = np.asarray(fns["turn_smpl_gradient_on"](), np.float64)
    out[prefix + "limits"] = np.asarray(fns["clip_smpl_vals"](), np.float64)
    src = torch.arange(133, dtype=torch.float32)[:, None].repeat(1, 2)
    rows = fns[map_name](src).numpy()
    assert (rows[:, 0] == rows[:, 1]).all() and (rows == np.round(rows)).all()
    out[prefix + "map"] = rows[:, 0].astype(np.int64)                # [rows]: the COCO index of every joint row, 0 for none


def main():
    out = {}
    recorded("ooptimize_smpl.py", "coco133_to_smpl", "smpl_", out)
    recorded("ooptimize_smplh.py", "coco133_to_smplh", "smplh_", out)
    est = os.path.join(KIT, "score_demo_video")
    for name, pre in (("poses.npz", "poses_"), ("poses_optimized.npz", "opt_"), ("cameras.npz", "cam_")):
        with np.load(os.path.join(est, name)) as z:
            for k in z.files:
                out[pre + k] = z[k]
    files = sorted(glob.glob(os.path.join(KIT, "keypoints_coco133", "sapiens_0.6b", "*.json")))
    out["n_keypoint_files"] = np.int64(len(files))
    kp, sc = [], []
    for f in files[:4]:
        inst = json.load(open(f))["instance_info"][0]
        kp.append(np.asarray(inst["keypoints"], np.float64))
        sc.append(np.asarray(inst["keypoint_scores"], np.float64))
    out["keypoints"], out["scores"] = np.stack(kp), np.stack(sc)
    np.savez_compressed(os.path.join(HERE, "pose_refine_golden.npz"), **out)
    shutil.copyfile(files[0], os.path.join(HERE, "pose_refine_keypoints_000000.json"))
    for k, v in out.items():
        print(k, np.asarray(v).shape, np.asarray(v).dtype)


if __name__ == "__main__":
    main()
