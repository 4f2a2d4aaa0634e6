"""``kit.load_kit`` on the device: a training kit written with PIL (24 frames of 22 x 9, one of them RGBA) becomes a ``FrameStore`` whose
bytes are the pixels that were written, split by the reference's rule (tests/golden/kit_splits_golden.json); the frames a ``FrameFeed``
draws from that store are bit-equal to ``value_table()[pixels]``; and the reference kit's own files under tests/golden/ -- cv2's
streams -- decode to what PIL reads from them."""
import os

import numpy as np
import pytest
import torch

import unpng_case as uc
from sings_amd import frame_feed as FF
from sings_amd import kit as KIT

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kit"))
    return (root,) + uc.write_kit(root, rgba_at=(5,))


def test_load_kit_fills_the_store_with_the_pixels_of_the_split(written):
    root, rgb, mask, poses = written
    g = uc.golden_splits()
    for split, want, first in (("train", g["train"]["22"], 2), ("val", g["val"]["22"], 2), ("train+val", list(range(24)), 0)):
        kit = KIT.load_kit(root, split=split, device=_dev())
        assert kit.indices == want
        at = [first + i for i in want]
        data = kit.store.data
        assert data.dtype == torch.uint8 and tuple(data.shape) == (len(want), 9, 22, 4) and data.device == _dev()
        assert (kit.store.F, kit.store.H, kit.store.W) == (len(want), 9, 22) and kit.store.nbytes == data.numel()
        got = data.cpu().numpy()
        assert np.array_equal(got[..., :3], rgb[at]) and np.array_equal(got[..., 3], mask[at]), split
        for key in ("global_orient", "body_pose", "transl"):
            assert kit.smpl[key].device == _dev() and np.array_equal(kit.smpl[key].cpu().numpy(), poses[key][at])
        assert kit.camera["world_view_transform"].device == _dev() and kit.camera["image_width"] == 22


def test_a_feed_draws_frames_bit_equal_to_the_value_table_of_the_pixels(written):
    root, rgb, mask, _ = written
    kit = KIT.load_kit(root, split="train", device=_dev())
    at = [2 + i for i in kit.indices]
    feed = FF.FrameFeed(kit.store, seed=5, frames_per_step=4)
    table = FF.value_table()
    seen = set()
    for _ in range(6):
        feed.draw()
        idx = feed.last_indices.tolist()
        seen.update(idx)
        frames = [at[i] for i in idx]
        want_gt = table[rgb[frames]].transpose(0, 3, 1, 2)
        assert np.array_equal(feed.gt.cpu().numpy().view(np.int32), np.ascontiguousarray(want_gt).view(np.int32))
        assert np.array_equal(feed.mask.cpu().numpy().view(np.int32), table[mask[frames]].view(np.int32))
    assert seen == set(range(20)), "24 draws over 20 frames: every frame of the split was drawn"
    # and the eager read validation uses
    gt, m = kit.store.frames([0, 19])
    assert np.array_equal(gt.cpu().numpy(), table[rgb[[at[0], at[19]]]].transpose(0, 3, 1, 2)) and np.array_equal(m.cpu().numpy(), table[mask[[at[0], at[19]]]])


def test_the_reference_kits_own_files_decode_to_what_pil_reads():
    files = {f: os.path.join(uc.GOLDEN, f) for f in uc.KIT_FILES}
    image = files["kit_image_000040.png"]
    store = FF.FrameStore.from_png_files([image, image], [files["kit_mask_000000.png"], files["kit_mask_000040.png"]], _dev())
    assert (store.F, store.H, store.W) == (2, 896, 512)
    got = store.data.cpu().numpy()
    want = uc.pil_pixels(dict(uc.VALID)["kit_image_000040.png"])
    assert np.array_equal(got[0, ..., :3], want) and np.array_equal(got[1, ..., :3], want)
    for f, name in enumerate(("kit_mask_000000.png", "kit_mask_000040.png")):
        assert np.array_equal(got[f, ..., 3], uc.pil_pixels(dict(uc.VALID)[name])[..., 0]), name
    # the store refuses what is not a kit's file, by name, and a CPU
    with pytest.raises(ValueError, match="kit_mask_000000.png: a PNG of 1 channels"):
        FF.FrameStore.from_png_files([files["kit_mask_000000.png"]], [files["kit_mask_000040.png"]], _dev())
    with pytest.raises(RuntimeError, match="GPU"):
        FF.FrameStore.from_png_files([image], [files["kit_mask_000000.png"]], "cpu")
