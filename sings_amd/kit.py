"""A training kit from disk to the device: where ``CustomDataset.__init__`` stands (sings/rec/datasets/Customdataset.py:45-82).

The kit's layout: ``images/*.png`` (8-bit RGB or RGBA), ``masks/*.png`` (8-bit grey), ``score_demo_video/cameras.npz`` and
``score_demo_video/poses_optimized.npz`` (``poses.npz`` when that is absent).  ``load_kit`` lists the files as the reference does (sorted
glob), applies its split rule, reads the poses and the camera, and fills a ``FrameStore`` with the split's frames through the device
PNG decoder (``sings_amd/unpng.py``): no cv2, no per-file decode on the host, nothing of the reference's code.

The split rule (``get_data_splits``, :31-42, and :57-74): ``train`` and ``val`` drop the first two frames ("sam2 is not good at the early
frames"), then every ``length``-th frame from ``length // 2`` on is a validation frame, ``length = int(1 / (n // 10) * n)``, the others
train; ``train+val`` keeps every frame.  The poses are sliced the same way, so ``indices`` index both.
"""
import glob
import os
from collections import namedtuple

import numpy as np

from . import camera as _camera
from . import unpng

Kit = namedtuple("Kit", ["store", "smpl", "camera", "indices", "image_paths", "mask_paths"])
Kit.__doc__ = """``store``: a ``FrameStore`` of the split's frames, in the split's order.  ``smpl``: ``betas`` [1,B], and ``global_orient`` [n,3],
``body_pose`` [n,69], ``transl`` [n,3] of the split's frames, fp32 tensors on the device.  ``camera``: the dict of
``Customdataset.init_camera`` (its matrices fp32 tensors on the device).  ``indices``: the split's frames, as indices into the kit's
list (after the dropped frames).
``image_paths`` / ``mask_paths``: the files the store's frames came from."""
SPLITS = ("train", "val", "train+val")
DROP_FIRST = 2


def get_data_splits(n):
    """``get_data_splits`` of the reference for a list of ``n`` frames -> (train, val), lists of indices."""
    n = int(n)
    num_val = n // 10
    if num_val < 1:
        raise ValueError(f"a kit of {n} frames has no validation frame: the split rule needs at least 10")
    length = int(1 / num_val * n)
    val = list(range(n))[length // 2::length]
    train = sorted(set(range(n)) - set(val))
    return train, val


def load_smpl_param(path):
    """``load_smpl_param`` (:18-28) in numpy: the ``thetas`` alias honoured, fp32, ``betas`` as one row."""
    p = dict(np.load(str(path)))
    if "thetas" in p:
        p["body_pose"] = p["thetas"][..., 3:]
        p["global_orient"] = p["thetas"][..., :3]
    for key in ("betas", "body_pose", "global_orient", "transl"):
        if key not in p:
            raise ValueError(f"{path}: no array {key!r}")
    return {"betas": p["betas"].astype(np.float32).reshape(1, -1), "body_pose": p["body_pose"].astype(np.float32),
            "global_orient": p["global_orient"].astype(np.float32), "transl": p["transl"].astype(np.float32)}


def init_camera(path, znear=0.01, zfar=100.0):
    """``Customdataset.init_camera`` (:96-157) through ``sings_amd/camera.py`` -> its dict, numpy values.  The extrinsic must be the
    identity, as the reference asserts; a principal point more than a pixel off the centre takes the off-centre projection."""
    cam = np.load(str(path))
    K, ext = np.asarray(cam["intrinsic"], np.float64), np.asarray(cam["extrinsic"], np.float64)
    if not np.allclose(ext, np.eye(4)):
        raise ValueError(f"{path}: the extrinsic is not the identity")
    height, width = int(cam["height"]), int(cam["width"])
    wvt = np.ascontiguousarray(ext.astype(np.float32).T)
    c2w = np.linalg.inv(ext).astype(np.float32)
    if abs(height // 2 - K[1, 2]) > 1.0 or abs(width // 2 - K[0, 2]) > 1.0:
        fovx = float(np.arctan(K[0, 2] / K[0, 0]) + np.arctan((width - K[0, 2]) / K[0, 0]))
        fovy = float(np.arctan(K[1, 2] / K[1, 1]) + np.arctan((height - K[1, 2]) / K[1, 1]))
        P = _camera.get_projection_matrix_center(znear, zfar, K[0, 0], K[1, 1], K[0, 2], K[1, 2], width, height)
    else:
        fovx = float(2 * np.arctan(width / (2 * K[0, 0])))
        fovy = float(2 * np.arctan(height / (2 * K[1, 1])))
        P = _camera.get_projection_matrix(znear, zfar, fovx, fovy)
    return {"near": znear, "far": zfar, "fovx": fovx, "fovy": fovy, "image_height": height, "image_width": width,
            "world_view_transform": wvt, "c2w": c2w, "full_proj_transform": (wvt @ P.T).astype(np.float32),
            "camera_center": np.linalg.inv(wvt)[3, :3].astype(np.float32), "cam_intrinsics": K}


def load_kit(root, split="train", device=None, verify_crc=True):
    """-> ``Kit``.  ``ValueError`` naming the file for unequal counts of images and masks, a file that is not an 8-bit non-interlaced
    PNG of colour type 2 or 6 (images) or 0 (masks), and sizes that differ from ``cameras.npz``.  ``device``: the GPU the store and
    the tensors live on (None: the current one)."""
    import torch
    from .frame_feed import FrameStore
    if split not in SPLITS:
        raise ValueError(f"load_kit: split must be one of {SPLITS}, got {split!r}")
    root = str(root)
    images = sorted(glob.glob(os.path.join(root, "images", "*.png")))
    masks = sorted(glob.glob(os.path.join(root, "masks", "*.png")))
    if len(images) != len(masks) or not images:
        raise ValueError(f"{root}: {len(images)} files in images/ and {len(masks)} in masks/: the counts must be equal and not zero")
    est = os.path.join(root, "score_demo_video")
    smpl_path = os.path.join(est, "poses_optimized.npz")
    if not os.path.exists(smpl_path):
        smpl_path = os.path.join(est, "poses.npz")
    cam = init_camera(os.path.join(est, "cameras.npz"))
    smpl = load_smpl_param(smpl_path)
    if len(smpl["body_pose"]) < len(images):
        raise ValueError(f"{smpl_path}: {len(smpl['body_pose'])} poses for {len(images)} frames")
    if split == "train+val":
        indices = list(range(len(images)))
    else:
        images, masks = images[DROP_FIRST:], masks[DROP_FIRST:]
        for key in ("body_pose", "global_orient", "transl"):
            smpl[key] = smpl[key][DROP_FIRST:]
        train, val = get_data_splits(len(images))
        indices = train if split == "train" else val
    images, masks = [images[i] for i in indices], [masks[i] for i in indices]
    checked = unpng.check_kit_files(images, masks, (cam["image_width"], cam["image_height"]))   # (cameras.npz says the size)
    store = FrameStore.from_png_files(images, masks, device, verify_crc=verify_crc, checked=checked)   # (refuses a device that is no GPU)
    dev = store.device
    idx = np.asarray(indices, np.int64)
    cam = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) and k != "cam_intrinsics" else v) for k, v in cam.items()}
    on_dev = {"betas": torch.from_numpy(smpl["betas"]).to(dev)}
    for key in ("global_orient", "body_pose", "transl"):
        on_dev[key] = torch.from_numpy(np.ascontiguousarray(smpl[key][idx])).to(dev)
    return Kit(store, on_dev, cam, indices, images, masks)


# ---- the keypoints the reference's pose refinement reads (``prepare_kits.sh ... --opt``: preprocess/utils/ooptimize_smpl.py)
KEYPOINT_DIR = os.path.join("keypoints_coco133", "sapiens_0.6b")


def load_keypoints(root, indices=None):
    """The Sapiens COCO-133 files of a kit, ``keypoints_coco133/sapiens_0.6b/*.json`` in sorted order -> (keypoints [n,133,2],
    scores [n,133]) fp32 numpy arrays: ``instance_info[0].keypoints`` and ``.keypoint_scores`` of every file (of ``indices`` when given).
    ``ValueError`` naming the file for a missing key or a wrong shape, and naming the directory when the number of files differs from
    the number of images."""
    import json
    root = str(root)
    files = sorted(glob.glob(os.path.join(root, KEYPOINT_DIR, "*.json")))
    images = sorted(glob.glob(os.path.join(root, "images", "*.png")))
    if len(files) != len(images) or not files:
        raise ValueError(f"{os.path.join(root, KEYPOINT_DIR)}: {len(files)} keypoint files for {len(images)} images: the counts must be "
                         "equal and not zero")
    if indices is not None:
        files = [files[int(i)] for i in indices]
    kps, scs = [], []
    for path in files:
        try:
            with open(path) as f:
                inst = json.load(f)["instance_info"][0]
            kp, sc = np.asarray(inst["keypoints"], np.float32), np.asarray(inst["keypoint_scores"], np.float32)
        except (KeyError, IndexError, TypeError, ValueError) as e:
            raise ValueError(f"{path}: no instance_info[0].keypoints / .keypoint_scores ({type(e).__name__}: {e})") from e
        if kp.ndim != 2 or kp.shape[0] != 133 or kp.shape[1] < 2 or sc.shape != (133,):
            raise ValueError(f"{path}: keypoints {kp.shape} / keypoint_scores {sc.shape} are not [133, >= 2] / [133]")
        kps.append(kp[:, :2])
        scs.append(sc)
    return np.stack(kps), np.stack(scs)

