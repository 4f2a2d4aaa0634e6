"""Generates tests/golden/canon_pose_golden.npz by executing the reference's ``get_predefined_pose`` and ``get_smpl_static_params``
(sings/rec/datasets/utils.py) on the CPU.  The module's ``import cv2`` (and the ``graphics`` import behind it, cv2 again) are satisfied
by empty placeholder modules, likewise loguru, and the functions' ``device='cuda'`` defaults are replaced by ``'cpu'`` in the text that
is executed.  The file holds arrays and key names only.

    python tests/golden/gen_canon_pose_golden.py <path of the reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch

ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SINGS_REFERENCE"]
sys.path.insert(0, ref)
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
lg = types.ModuleType("loguru"); lg.logger = None
sys.modules.setdefault("loguru", lg)
path = os.path.join(ref, "sings", "rec", "datasets", "utils.py")
du = types.ModuleType("reference_datasets_utils")
exec(compile(open(path).read().replace("device='cuda'", "device='cpu'"), path, "exec"), du.__dict__)

TYPES = ("da_pose", "a_pose", "little_a_pose", "little_little_a_pose", "t_pose")
out = {"pose_types": np.array(TYPES)}
betas = torch.from_numpy(np.random.RandomState(3).normal(0, 1, (1, 10)).astype(np.float32))
out["betas_in"] = betas.numpy()
for name in TYPES:
    pose = du.get_predefined_pose(name)
    assert tuple(pose.shape) == (1, 69) and pose.dtype == torch.float32
    out[f"pose/{name}"] = pose[0].numpy()
    params = du.get_smpl_static_params(betas, pose_type=name)
    out[f"static_keys/{name}"] = np.array(list(params))
    for k, v in params.items():
        out[f"static/{name}/{k}"] = v.numpy()
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "canon_pose_golden.npz"), **out)
print("wrote canon_pose_golden.npz", len(out))
