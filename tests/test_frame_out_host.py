"""The output stage of the animation paths (sings_amd/frame_out.py) without a device: every value ``out=`` accepts and refuses, the
names that stay importable from ``posed``, and that nothing in the stage falls back to the CPU."""
import pytest
import torch

from sings_amd import frame_out as fo
from sings_amd import posed


def test_parse_out_accepts_and_refuses_the_whole_table():
    accepted = {"float32": (None, None, None), "rgb8": (False, None, None), "bgr8": (True, None, None), "jpeg": (False, "jpeg", 90),
                ("jpeg", 1): (False, "jpeg", 1), ("jpeg", 50): (False, "jpeg", 50), ("jpeg", 100): (False, "jpeg", 100),
                "png": (False, "png", None)}
    for out, want in accepted.items():
        spec = fo.parse_out(out)
        assert tuple(spec) == want and (spec.bgr, spec.codec, spec.quality) == want, out
    for bad in (("jpeg", 0), ("jpeg", 101), ("jpeg", 7.5), ("jpeg", "90"), ("jpeg", None)):
        with pytest.raises(ValueError, match="quality"):
            fo.parse_out(bad)
    for bad in (("png", 3), ("jpeg",), ("jpeg", 90, 1), ["jpeg", 90], ("rgb8", 90), "jpg", "bgr16", "JPEG", "", None, 8, b"png"):
        with pytest.raises(ValueError, match="out must be one of"):
            fo.parse_out(bad)
    assert posed.JPEG_QUALITY == fo.JPEG_QUALITY == 90 and posed.frames_to_u8 is fo.frames_to_u8


def test_frame_out_has_no_cpu_fallback():
    one = fo.FrameOut(torch.device("cpu"))
    for out in ("rgb8", "bgr8", "jpeg", ("jpeg", 50), "png"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            one.convert(fo.parse_out(out), torch.zeros(2, 3, 4, 4))
    u8 = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    assert one.finish(fo.parse_out("bgr8"), u8, 1) is u8
    for out in ("jpeg", ("jpeg", 50), "png"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            one.finish(fo.parse_out(out), u8, 1)
    assert not any(one.enc.values())
