"""The device PNG decoder (include/sings_unpng.h, ``unpng.PngDecoder``).

The bar is exact: the bytes the two launches leave in the store ARE the pixels PIL reads from the same file, and every stream's status
IS the Python restatement's (``unpng.inflate_host`` / ``unfilter_host``, which tests/test_unpng_host.py holds to zlib and PIL), for
every file of tests/unpng_case.py -- all of one picture size in one call, whatever their channels, block kinds and lengths.  Corrupt
streams report their code and touch nothing; the streams beside them are decoded.  The corrupt batch is ``unpng_case.CORRUPT``, the
streams csrc/sg_inflate.h reads on the host in tests/test_inflate_sanitized.py, a CPU test: that program, and any sanitizer, runs there
and not here.  The point is an error code, never a fault."""
import numpy as np
import pytest
import torch

import unpng_case as uc
from sings_amd import unpng as U

pytestmark = pytest.mark.gpu
FILL = 0xA5


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _groups():
    """The VALID files by picture size: {(W, H): [name, ...]}."""
    out = {}
    for name, data in uc.VALID:
        W, H, _ = U.read_png_header(data)
        out.setdefault((W, H), []).append(name)
    return out


GROUPS = _groups()


def _check_frame(frame, data, name):
    """One frame of the store uint8 [H,W,4] against the file that was decoded into it: its channels are PIL's, the others untouched."""
    want = uc.pil_pixels(data)
    if want.shape[2] == 1:
        assert np.array_equal(frame[..., 3], want[..., 0]), name
        assert (frame[..., :3] == FILL).all(), name
    else:
        assert np.array_equal(frame[..., :3], want[..., :3]), name
        assert (frame[..., 3] == FILL).all(), name


@pytest.mark.parametrize("size", sorted(GROUPS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_pixels_are_pils_and_statuses_are_the_twins(size):
    W, H = size
    names = GROUPS[size]
    files = [dict(uc.VALID)[n] for n in names]
    chans = [U.read_png_header(f)[2] for f in files]
    store = torch.full((len(files), H, W, 4), FILL, dtype=torch.uint8, device=_dev())
    dec = U.PngDecoder(_dev(), len(files), H * (1 + 4 * W))
    assert dec.decode_into(store, files, [4 * i + (3 if ch == 1 else 0) for i, ch in enumerate(chans)]) == len(files)
    assert (dec.uploads, dec.launches) == (1, 2), "one upload and two launches for the whole batch"
    status = dec.status[:len(files)].cpu().tolist()
    assert status == [uc.twin_valid(n)[5] for n in names] == [0] * len(files)
    got = store.cpu().numpy()
    for i, name in enumerate(names):
        _check_frame(got[i], files[i], name)
    if len(set(chans)) > 1:
        assert len({len(U.parse_png(f)[3]) for f in files}) > 1, "streams of different lengths and channels in one call"


def test_colour_and_mask_of_one_frame_meet_in_its_four_channels_and_fewer_streams_leave_the_rest():
    W, H = 85, 7
    rgb, rgba, grey = (dict(uc.VALID)[f"zlib-85x7x{ch}-rle1"] for ch in (3, 4, 1))
    store = torch.full((4, H, W, 4), FILL, dtype=torch.uint8, device=_dev())
    dec = U.PngDecoder(_dev(), 8, H * (1 + 4 * W))
    dec.status.fill_(77)
    dec.decode_into(store, [rgb, grey, rgba], [4 * 1, 4 * 1 + 3, 4 * 2])
    got = store.cpu().numpy()
    assert np.array_equal(got[1, ..., :3], uc.pil_pixels(rgb)) and np.array_equal(got[1, ..., 3], uc.pil_pixels(grey)[..., 0])
    assert np.array_equal(got[2, ..., :3], uc.pil_pixels(rgba)[..., :3]) and (got[2, ..., 3] == FILL).all(), "alpha is dropped"
    assert (got[0] == FILL).all() and (got[3] == FILL).all(), "the frames no stream names are untouched"
    assert dec.status.cpu().tolist() == [0, 0, 0] + [77] * 5
    # batches: five files through a decoder of two streams
    dec2 = U.PngDecoder(_dev(), 2, H * (1 + 4 * W))
    store.fill_(FILL)
    dec2.decode_into(store, [rgb, grey, rgba, grey, rgb], [0, 3, 4, 7, 12])
    assert (dec2.uploads, dec2.launches) == (3, 6)
    got = store.cpu().numpy()
    assert np.array_equal(got[0, ..., :3], uc.pil_pixels(rgb)) and np.array_equal(got[0, ..., 3], uc.pil_pixels(grey)[..., 0])
    assert np.array_equal(got[1, ..., :3], uc.pil_pixels(rgba)[..., :3]) and np.array_equal(got[1, ..., 3], uc.pil_pixels(grey)[..., 0])
    assert (got[2] == FILL).all() and np.array_equal(got[3, ..., :3], uc.pil_pixels(rgb)) and (got[3, ..., 3] == FILL).all()


def test_corrupt_streams_report_their_status_and_touch_nothing_beside_valid_ones():
    W, H, ch = uc.CORRUPT_SHAPE
    # ONE batch on the device: corrupt and valid streams interleaved, a picture of another size and a wrong first channel too
    valid = [n for n in GROUPS[(W, H)] if n.startswith("zlib-85x7x")]
    assert len(valid) == 18
    files, want = [], []
    for i, c in enumerate(uc.CORRUPT):
        files += [uc.png_file(W, H, ch, c[1]), dict(uc.VALID)[valid[i]]]
        want += [uc.twin_corrupt(c[0])[1], 0]
    files += [dict(uc.VALID)["zlib-22x9x3-level9"], dict(uc.VALID)["zlib-85x7x1-level9"], dict(uc.VALID)["zlib-85x7x3-level9"]]
    want += [U.E_SIZE, U.E_TABLE, U.E_TABLE]
    chans = [U.read_png_header(f)[2] for f in files]
    dest = [4 * i + (3 if c == 1 else 0) for i, c in enumerate(chans)]
    dest[-2] -= 3                                                 # a grey stream sent to channel 0
    dest[-1] = 4 * len(files)                                     # a frame the store does not have
    assert all(w != 0 for w in want[0:2 * len(uc.CORRUPT):2]) and [c[2] for c in uc.CORRUPT] == want[0:2 * len(uc.CORRUPT):2]
    store = torch.full((len(files), H, W, 4), FILL, dtype=torch.uint8, device=_dev())
    dec = U.PngDecoder(_dev(), len(files), H * (1 + 4 * W))
    with pytest.raises(ValueError) as e:
        dec.decode_into(store, files, dest)
    assert (dec.uploads, dec.launches) == (1, 2)
    assert dec.status[:len(files)].cpu().tolist() == want
    for i, w in enumerate(want):
        assert (f"<file {i}>: SG_UNPNG_{U.STATUS[w]} ({w})" in str(e.value)) == (w != 0), i
    got = store.cpu().numpy()
    for i, w in enumerate(want):
        if w:
            assert (got[i] == FILL).all(), ("a failed stream wrote", i)
        else:
            _check_frame(got[i], files[i], i)


def test_a_stream_larger_than_its_slot_is_refused_not_written():
    rgb, grey = dict(uc.VALID)["zlib-85x7x3-level9"], dict(uc.VALID)["zlib-85x7x1-level9"]
    store = torch.full((1, 7, 85, 4), FILL, dtype=torch.uint8, device=_dev())
    dec = U.PngDecoder(_dev(), 2, 7 * (1 + 85))                   # slots for grey pictures only
    with pytest.raises(ValueError, match=r"<file 0>: SG_UNPNG_E_WORKSPACE \(19\)"):
        dec.decode_into(store, [rgb, grey], [0, 3])
    got = store.cpu().numpy()
    assert (got[..., :3] == FILL).all() and np.array_equal(got[0, ..., 3], uc.pil_pixels(grey)[..., 0])
    with pytest.raises(ValueError, match="colour type 3"):        # refused on the host, by name, before anything is uploaded
        from PIL import Image
        import io
        b = io.BytesIO()
        Image.fromarray(uc.pil_pixels(rgb)).convert("P").save(b, "PNG")
        dec.decode_into(store, [grey, b.getvalue()], [3, 0])
