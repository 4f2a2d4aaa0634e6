"""What the pose-refinement tests share: a small synthetic kit built from the level models of ``body_case`` -- true poses, perturbed
starting poses, the target masks (the fp64 twin's silhouette of the true pose, thresholded at 0.5) and the keypoints (the projected
joint rows of the true pose, score 1) -- and a small camera: W x H = 40 x 56, not square, so the NDC scale comes from the width
(s = 2 / 40); fx = fy = 56, principal point a little off the centre; the level-2 model (radius about 1) at z = 4 spans about 28 pixels.

The 21 extra joint rows are vertices 3, 6, 9, ... of the model: any fixed choice serves, the map only reads rows 29-34 of them."""
import numpy as np
import torch

import body_case as bc
from sings_amd import pose_refine as PR

W, H = 40, 56
INTR = (56.0, 56.0, 19.6, 28.3)

CAMERA = {"cam_intrinsics": np.array([[INTR[0], 0.0, INTR[2]], [0.0, INTR[1], INTR[3]], [0.0, 0.0, 1.0]]),
          "image_height": H, "image_width": W, "world_view_transform": np.eye(4, dtype=np.float32)}
DELTA = 0.15                                     # rad, on the knees' x, the ankles and the elbows
PERTURBED = (12, 15, 21, 22, 23, 24, 25, 26, 54, 55, 56, 57, 58, 59)        # RefineSpec.smpl().enabled()
_CACHE = {}


def extra_ids(V, n=21):
    return tuple(int(i) for i in (3 * np.arange(1, n + 1)) % V)


def model(J=24, level=2):
    return bc.model_arrays(J, 10, level)


def reverse_coco(spec, rows_2d):
    """Joint rows [rows,2] -> COCO-133 keypoints [133,2] that ``spec.rows_of`` maps back onto them (rows the map does not read: 0)."""
    kp = np.zeros((133, 2))
    for coco, row in spec.keypoint_map:
        kp[coco] = rows_2d[row]
    return kp


def kit(n_frames=4, seed=6, J=24, level=2, spec=None):
    """-> dict: ``model``, ``extra``, ``betas`` [10], ``true`` / ``start`` [F,72] fp32, ``transl`` [F,3] fp32, ``masks`` [F,H,W] fp32 of 0 / 1,
    ``keypoints`` [F,133,2], ``scores`` [F,133] fp32."""
    key = (n_frames, seed, J, level)
    if key in _CACHE:
        return _CACHE[key]
    spec = PR.RefineSpec.smpl() if spec is None else spec
    rs = np.random.RandomState(seed)
    m = model(J, level)
    V = np.asarray(m["v_template"]).shape[0]
    ex = extra_ids(V, spec.n_joint_rows - J)
    betas = (0.3 * rs.randn(10)).astype(np.float32)
    true = (0.12 * rs.randn(n_frames, 72)).astype(np.float32)
    true[:, 12] = true[:, 15] = 0.5                                  # knees bent within their limit [0, 160 deg]
    true[:, [13, 14, 16, 17]] = 0.0
    true[:, 55] = -0.5                                               # elbows within theirs: [-160, 0] on y, [0, 160] on z
    true[:, 59] = 0.5
    true[:, [23, 26]] = 0.0                                          # the ankles' z: its limit is +-10 deg, DELTA must fit inside
    sign = np.where(rs.rand(n_frames, len(PERTURBED)) < 0.5, -1.0, 1.0)
    start = true.copy()
    start[:, PERTURBED] += (DELTA * sign).astype(np.float32)
    transl = np.stack([[0.05 * f, -0.04 * f, 4.0 + 0.2 * f] for f in range(n_frames)]).astype(np.float32)
    host = PR.host_model(m)
    masks, kps = [], []
    for f in range(n_frames):
        with torch.no_grad():
            vc, rows = PR.host_forward(host, betas, torch.tensor(true[f], dtype=torch.float64), transl[f], np.eye(3), ex)
            alpha = PR.silhouette_host(vc, host["faces"], INTR, H, W, spec.sigma)
            masks.append((alpha > 0.5).float().numpy())
            kps.append(reverse_coco(spec, PR.project_joints(rows, INTR, H, W).numpy()))
    out = dict(model=m, extra=ex, betas=betas, true=true, start=start, transl=transl, masks=np.stack(masks).astype(np.float32),
               keypoints=np.stack(kps).astype(np.float32), scores=np.ones((n_frames, 133), np.float32))
    _CACHE[key] = out
    return out


def pose_error(pose, true, enabled):
    """Per frame: the root mean square of pose - true over the enabled entries."""
    return np.sqrt(((np.asarray(pose, np.float64) - np.asarray(true, np.float64))[:, enabled] ** 2).mean(1))
