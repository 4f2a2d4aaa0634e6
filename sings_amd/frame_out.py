"""The output stage of the animation paths: what ``out=`` names, and the two steps that apply it to rendered frames.

 * ``parse_out``: the one place that knows the accepted values of ``out``.
 * ``frames_to_u8``: fp32 frames to 8-bit HWC bytes in one launch (``sg_frames_to_u8``).
 * ``FrameOut``: ``convert`` inside a launch (the clamp, or ``frames_to_u8``), ``finish`` behind the hand-out (nothing, or the frames'
   files from a device encoder: ``video.JpegEncoder`` / ``png.PngEncoder`` through ``new_encoder``).
"""
from collections import namedtuple

import torch

from . import _lib
from ._marshal import _ptr, _stream

JPEG_QUALITY = 90                    # of out="jpeg"; out=("jpeg", quality) names another
# bgr: None (fp32 frames), or the ``bgr`` of frames_to_u8; codec: None, "jpeg" or "png" (RGB bytes, then a ``bytes`` per frame)
OutSpec = namedtuple("OutSpec", "bgr codec quality")
_OUT = {"float32": OutSpec(None, None, None), "rgb8": OutSpec(False, None, None), "bgr8": OutSpec(True, None, None),
        "jpeg": OutSpec(False, "jpeg", JPEG_QUALITY), "png": OutSpec(False, "png", None)}


def parse_out(out):
    """``out`` of the animation paths -> ``OutSpec``: "float32", "rgb8", "bgr8", "jpeg" (quality ``JPEG_QUALITY``), ("jpeg", q) with q
    in 1..100, or "png".  ValueError otherwise."""
    if isinstance(out, tuple) and len(out) == 2 and out[0] == "jpeg":
        if not isinstance(out[1], int) or not 1 <= out[1] <= 100:
            raise ValueError(f"out=(\"jpeg\", quality): quality must be an int in 1..100, got {out[1]!r}")
        return OutSpec(False, "jpeg", out[1])
    if not isinstance(out, str) or out not in _OUT:
        raise ValueError(f"out must be one of {sorted(_OUT)} (or (\"jpeg\", quality)), got {out!r}")
    return _OUT[out]


def frames_to_u8(img, bgr=False):
    """[3,H,W] or [K,3,H,W] fp32 frames on the GPU -> uint8 [H,W,3] / [K,H,W,3] on the GPU: the reference's last step,
    ``(clamp(x, 0, 1) * 255).astype(uint8)`` (+ cvtColor to BGR with ``bgr``: gs_trainer.py:717-719), in ONE launch
    (sg_frames_to_u8; NaN gives 0).  A quarter of the fp32 bytes to copy to the host."""
    if not torch.is_tensor(img) or img.device.type != "cuda":
        raise RuntimeError("sings_amd.posed.frames_to_u8 runs on the MI355X only; there is no CPU fallback")
    if img.dtype != torch.float32 or img.dim() not in (3, 4) or img.shape[-3] != 3:
        raise ValueError(f"frames_to_u8: fp32 [3,H,W] or [K,3,H,W] expected, got {img.dtype} {tuple(img.shape)}")
    x = img.contiguous()
    K, H, W = (1 if x.dim() == 3 else int(x.shape[0])), int(x.shape[-2]), int(x.shape[-1])
    out = torch.empty(tuple(x.shape[:-3]) + (H, W, 3), dtype=torch.uint8, device=x.device)
    if out.numel() == 0:
        return out
    _lib.check(_lib.load().sg_frames_to_u8(K, W, H, _ptr(x), int(bool(bgr)), _ptr(out),
                                           _stream(x.device)), "frames_to_u8")
    return out


def new_encoder(codec, W, H, K, dev, quality=None):
    """The device encoder of ``codec`` for K frames of W x H: ``video.JpegEncoder`` at ``quality`` or ``png.PngEncoder``."""
    if codec == "jpeg":
        from .video import JpegEncoder
        return JpegEncoder(W, H, K, dev, quality=int(quality))
    from .png import PngEncoder
    return PngEncoder(W, H, K, dev)


class FrameOut:
    """The two steps of an ``OutSpec`` on device ``dev``.  It holds at most one encoder per codec, of one (W, H, K, quality) -- what
    of an engine key decides an encoder; frames of another size replace it, as they replace the engines."""

    def __init__(self, dev):
        self.dev, self.key, self.enc = dev, {}, {}

    def convert(self, spec, color):
        """Inside the launch, on the engine's stream: ``color`` [K,3,H,W] (the engine's buffer, which is reused) -> a new tensor, the
        clamped frames or their bytes [K,H,W,3]."""
        return torch.clamp(color, 0.0, 1.0) if spec.bgr is None else frames_to_u8(color, spec.bgr)

    def finish(self, spec, img, k):
        """Behind the hand-out, on the caller's stream: ``img`` as it is, or the files of its first k frames (the padded frames of a
        last batch are not encoded) -- a list of k ``bytes`` by ``encode_to_host``: one read of the sizes, one of the used bytes."""
        if spec.codec is None:
            return img
        key = (int(img.shape[2]), int(img.shape[1]), int(img.shape[0]), spec.quality)
        if self.key.get(spec.codec) != key:
            self.enc[spec.codec] = None                          # (drop the old workspaces before the new ones are sized)
            self.enc[spec.codec] = new_encoder(spec.codec, *key[:3], self.dev, key[3])
            self.key[spec.codec] = key
        return self.enc[spec.codec].encode_to_host(img[:k])
