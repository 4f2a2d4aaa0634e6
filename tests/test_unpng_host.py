"""Host tests of sings_amd/unpng.py and sings_amd/kit.py (include/sings_unpng.h, ``_lib._PROTOTYPES_UNPNG``): the Python restatement
of the decode is held to two decoders we did not write -- ``zlib.decompress`` for the inflate, PIL for the pixels -- on every case of
tests/unpng_case.py, and to zlib's verdict on the corrupt ones; the kit loader to the reference's split rule (a golden of its own
``get_data_splits``).  Everything is exact.  The device path is held to the restatement in tests/test_gpu_unpng.py, csrc/sg_inflate.h on
the host in tests/test_inflate_sanitized.py."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

import unpng_case as uc
from sings_amd import _lib
from sings_amd import kit as KIT
from sings_amd import unpng as U


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_unpng.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_UNPNG) == ["sg_unpng_layout", "sg_unpng_decode"]
    assert not set(_lib._PROTOTYPES_UNPNG) & set(_lib._PROTOTYPES) and not set(_lib._PROTOTYPES_UNPNG) & set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert _lib.HAS_UNPNG
    scalars = {"int": C.c_int, "size_t": C.c_size_t}
    for ret, name, params in protos:
        fn = getattr(lib, name)
        params = [p.strip() for p in params.split(",")]
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params), name
        for p, t in zip(params, fn.argtypes):
            if "*" in p or "[" in p:
                assert issubclass(t, (C._Pointer, C.c_void_p)), (name, p)
            else:
                assert t is scalars[[w for w in re.findall(r"\w+", p) if w != "const"][0]], (name, p)
    for name in ("MAX_STREAMS", "MAX_ROW_BYTES", "MAX_HEIGHT", "TABLE_COLS"):
        assert int(re.search(rf"#define\s+SG_UNPNG_{name}\s+(\d+)", text).group(1)) == getattr(_lib, "UNPNG_" + name), name
    assert int(re.search(r"#define\s+SG_UNPNG_LAYOUT_WORDS\s+(\d+)", text).group(1)) == len(_lib.UNPNG_LAYOUT)
    # every status has a name in the header, and the Python names are those
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+SG_UNPNG_(OK|E_[A-Z_]+)\s+(\d+)", text)}
    assert codes == {name: i for i, name in enumerate(U.STATUS)} and all(getattr(U, name) == i for name, i in codes.items())
    # the core is one header without HIP types that the device source and the host program both include
    core = open(os.path.join(repo_root, "sings_amd", "csrc", "sg_inflate.h")).read()
    assert "hip/" not in core and "hipStream" not in core and "__host__ __device__" in core
    assert '#include "sg_inflate.h"' in open(os.path.join(repo_root, "sings_amd", "csrc", "sg_unpng.hip")).read()
    assert "sg_inflate.h" in open(os.path.join(repo_root, "tests", "tools", "inflate_check.cpp")).read()
    make = open(os.path.join(repo_root, "sings_amd", "csrc", "Makefile")).read()
    assert "sg_unpng.hip" in make and "sg_inflate.h" in make and "sings_unpng.h" in make


def test_layout_and_refusals_come_before_any_hip_call():
    from sings_amd import _marshal
    L = _marshal.unpng_layout(160, 512 * (1 + 3 * 896))
    assert L["slot_pitch"] == 512 * (1 + 3 * 896) and L["ws_bytes"] == 160 * L["slot_pitch"]
    assert _marshal.unpng_layout(3, 17) == {"ws_bytes": 96, "slot_pitch": 32}
    for args, word in (((0, 16), "n_streams = 0"), ((65536, 16), "n_streams = 65536"), ((1, 0), "max_raw_bytes = 0"), ((2, 1 << 39), "max_raw_bytes")):
        with pytest.raises(RuntimeError, match=word):
            _marshal.unpng_layout(*args)
    lib = _lib.load()
    assert lib.sg_unpng_layout(1, 16, None) == 1 and b"null pointer" in lib.sg_last_error()
    # every refusal of the decode call: before any HIP call, so without a device.  (The pointers are never followed.)
    p = C.c_void_p(4096)
    assert lib.sg_unpng_decode(1, None, None, None, 0, None, 1, 1, 1, None, None) == 1 and b"null pointer" in lib.sg_last_error()
    for args, word in (((0, p, p, p, 4096, p, 1, 8, 8, p), b"n = 0"), ((65536, p, p, p, 1 << 30, p, 1, 8, 8, p), b"n = 65536"),
                       ((1, p, p, p, 4096, p, 0, 8, 8, p), b"0 frames"), ((1, p, p, p, 4096, p, 1, 0, 8, p), b"8 x 0"),
                       ((1, p, p, p, 4096, p, 1, 65536, 8, p), b"8 x 65536"), ((1, p, p, p, 4096, p, 1, 8, 0, p), b"0 x 8"),
                       ((1, p, p, p, 4096, p, 1, 8, 4097, p), b"4097 x 8"), ((1, p, p, p, 4096, p, 1 << 30, 65535, 4096, p), b"2\\^40"),
                       ((2, p, p, p, 31, p, 1, 8, 8, p), b"at least 16 each"), ((1, p, p, C.c_void_p(4100), 4096, p, 1, 8, 8, p), b"16-byte aligned")):
        assert lib.sg_unpng_decode(*args, None) == 1, args
        assert re.search(word, lib.sg_last_error()), (args, lib.sg_last_error())
    with pytest.raises(RuntimeError, match="MI355X only"):
        U.PngDecoder("cpu", 4, 1000)


# ---- the restatement, against zlib and PIL -----------------------------------------------------------------------------------------
def test_the_case_list_holds_what_it_promises():
    names = [n for n, _ in uc.VALID]
    assert len(set(names)) == len(names) and all(f in names for f in uc.KIT_FILES)
    kinds = set()
    for name, data in uc.VALID:
        W, H, ch, stream = U.parse_png(data)
        if name.startswith("zlib-200x120x3-level0"):              # more than one stored block: 72 120 raw bytes
            assert H * (1 + W * ch) == 72120 and stream[2] & 6 == 0 and len(stream) > 72120 + 2 * 5
        kinds.add((ch, (stream[2] >> 1) & 3))
    assert kinds >= {(ch, t) for ch in (1, 3, 4) for t in (0, 1, 2)}, "stored, fixed and dynamic first blocks at 1, 3 and 4 channels"
    W, H, ch, stream = uc.handmade()
    assert (W, H, ch) == (255, 130, 1) and zlib.decompress(stream)[:256] == zlib.decompress(stream)[32768:33024]
    # a stream that reaches further back than the 256-byte window its header declares: zlib reads it, so it stands among the VALID
    W, H, ch, stream = uc.beyond_declared_window()
    assert stream[:2] == b"\x08\x1d" and 1 << ((stream[0] >> 4) + 8) == 256 < 384 and len(zlib.decompress(stream)) == H * (1 + W * ch)
    assert U.inflate_host(stream, H * (1 + W * ch)) == (zlib.decompress(stream), U.OK)
    # the kit's files are what the issue says they are: cv2's streams, every row of type Sub
    for f, size, shape in zip(uc.KIT_FILES, (7416, 4891, 165722), ((512, 896, 1),) * 2 + ((512, 896, 3),)):
        data = dict(uc.VALID)[f]
        W, H, ch, stream, raw, status = uc.twin_valid(f)
        assert len(data) == size and (W, H, ch) == shape and stream[:2] == b"\x78\x01" and status == 0
        assert set(np.frombuffer(raw, np.uint8).reshape(H, -1)[:, 0].tolist()) == {1}


@pytest.mark.parametrize("name", [n for n, _ in uc.VALID])
def test_inflate_host_is_zlib_and_unfilter_host_is_pil(name):
    W, H, ch, stream, raw, status = uc.twin_valid(name)
    assert status == U.OK and raw == zlib.decompress(stream) and len(raw) == H * (1 + W * ch)
    pixels, status = U.unfilter_host(raw, W, H, ch)
    want = uc.pil_pixels(dict(uc.VALID)[name])
    assert status == U.OK and pixels.dtype == np.uint8 and pixels.shape == want.shape == (H, W, ch) and np.array_equal(pixels, want)


# ---- the corrupt cases -------------------------------------------------------------------------------------------------------------
def test_the_corrupt_list_is_the_issues():
    assert [c[0] for c in uc.CORRUPT] == [
        "truncated-half", "truncated-last-byte", "block-type-3", "zlib-header", "wrong-adler", "stored-nlen", "distance-before-start",
        "fixed-symbol-286", "fixed-distance-30", "oversubscribed-lengths", "oversubscribed-code-length-code", "repeat-without-previous",
        "repeat-past-the-end", "raw-one-byte-long", "raw-one-byte-short", "filter-byte-5"]
    assert len({c[2] for c in uc.CORRUPT}) >= 13, "the cases stand for different codes"


@pytest.mark.parametrize("name", [c[0] for c in uc.CORRUPT])
def test_corrupt_streams_get_their_named_status_where_zlib_refuses_them(name):
    _, stream, named, inflate_level = next(c for c in uc.CORRUPT if c[0] == name)
    raw, status = uc.twin_corrupt(name)
    W, H, ch = uc.CORRUPT_SHAPE
    if not inflate_level:                                         # a valid zlib stream that is not this picture's
        assert len(zlib.decompress(stream)) - H * (1 + W * ch) == {U.E_OUTPUT_LONG: 1, U.E_OUTPUT_SHORT: -1, U.E_FILTER: 0}[named]
        assert status == named
        return
    try:
        want = zlib.decompress(stream)
    except zlib.error:
        assert status == named and status != U.OK
    else:
        assert status == U.OK and raw == want


# ---- parse_png -------------------------------------------------------------------------------------------------------------------
def test_parse_png_joins_idat_payloads_cut_anywhere():
    W, H, ch, stream = U.parse_png(dict(uc.VALID)["zlib-85x7x3-level9"])
    assert len(stream) > 40
    for cut in range(41):
        assert U.parse_png(uc.png_file(W, H, ch, stream, cut=cut)) == (W, H, ch, stream), cut
    raw, status = U.inflate_host(stream, H * (1 + W * ch))
    assert status == 0
    # the kit's image: 21 IDAT chunks, one stream
    data = dict(uc.VALID)["kit_image_000040.png"]
    assert data.count(b"IDAT") >= 21 and zlib.decompress(U.parse_png(data)[3])[:1] == b"\x01"


def test_parse_png_refusals():
    good = dict(uc.VALID)["zlib-22x9x3-level9"]
    W, H, ch, stream = U.parse_png(good)
    ihdr = lambda *f: uc._chunk(b"IHDR", struct.pack(">IIBBBBB", *f))
    idat, iend = uc._chunk(b"IDAT", stream), uc._chunk(b"IEND", b"")
    flipped = bytearray(good)
    flipped[60] ^= 1
    for data, word in ((b"\x89PNX" + good[4:], "signature"), (good[:50], "truncated"), (good[:-12], "no IEND"), (good[:-5], "truncated"),
                       (bytes(flipped), "CRC-32"), (U.SIGNATURE + idat + iend, "not a 13-byte IHDR"),
                       (U.SIGNATURE + ihdr(22, 9, 16, 2, 0, 0, 0) + idat + iend, "bit depth 16"),
                       (U.SIGNATURE + ihdr(22, 9, 8, 3, 0, 0, 0) + idat + iend, "colour type 3"),
                       (U.SIGNATURE + ihdr(22, 9, 8, 4, 0, 0, 0) + idat + iend, "colour type 4"),
                       (U.SIGNATURE + ihdr(22, 9, 8, 2, 0, 0, 1) + idat + iend, "interlaced"),
                       (U.SIGNATURE + ihdr(22, 9, 8, 2, 1, 0, 0) + idat + iend, "compression method 1"),
                       (U.SIGNATURE + ihdr(0, 9, 8, 2, 0, 0, 0) + idat + iend, "0 x 9"),
                       (U.SIGNATURE + ihdr(22, 9, 8, 2, 0, 0, 0) + iend, "no IDAT"),
                       (U.SIGNATURE + ihdr(22, 9, 8, 2, 0, 0, 0) + idat + uc._chunk(b"tEXt", b"a\x00b") + idat + iend, "consecutive"),
                       (U.SIGNATURE + ihdr(22, 9, 8, 2, 0, 0, 0) + ihdr(22, 9, 8, 2, 0, 0, 0) + idat + iend, "second IHDR")):
        with pytest.raises(ValueError, match=word):
            U.parse_png(data)
    assert U.parse_png(bytes(flipped), verify_crc=False)[:3] == (W, H, ch)
    # ancillary chunks before and behind the IDATs are walked over
    assert U.parse_png(U.SIGNATURE + ihdr(22, 9, 8, 2, 0, 0, 0) + uc._chunk(b"gAMA", b"\0\0\0\1") + idat + uc._chunk(b"tEXt", b"a\x00b") + iend)[3] == stream
    assert U.read_png_header(good[:33]) == (W, H, ch)
    with pytest.raises(ValueError, match="bit depth 16"):
        U.read_png_header(U.SIGNATURE + ihdr(22, 9, 16, 2, 0, 0, 0))


# ---- the kit ---------------------------------------------------------------------------------------------------------------------
def test_get_data_splits_is_the_references_for_every_length():
    g = uc.golden_splits()
    assert len(g["train"]) == len(g["val"]) == 391
    for n in range(10, 401):
        train, val = KIT.get_data_splits(n)
        assert train == g["train"][str(n)] and val == g["val"][str(n)], n
    with pytest.raises(ValueError, match="at least 10"):
        KIT.get_data_splits(9)


class _StubStore:
    device = "cpu"

    def __init__(self, images, masks):
        self.images, self.masks = list(images), list(masks)


def _stub(monkeypatch):
    from sings_amd import frame_feed
    monkeypatch.setattr(frame_feed.FrameStore, "from_png_files", classmethod(lambda cls, images, masks, device=None, verify_crc=True, checked=None: _StubStore(images, masks)))


def test_load_kit_splits_and_slices_the_poses(tmp_path, monkeypatch):
    _stub(monkeypatch)
    g = uc.golden_splits()
    root = str(tmp_path / "kit")
    rgb, mask, poses = uc.write_kit(root, rgba_at=(5,))
    for split, want in (("train", g["train"]["22"]), ("val", g["val"]["22"]), ("train+val", list(range(24)))):
        kit = KIT.load_kit(root, split=split, device="cpu")
        first = 0 if split == "train+val" else 2
        assert kit.indices == want and len(kit.indices) == {"train": 20, "val": 2, "train+val": 24}[split]
        assert [os.path.basename(p) for p in kit.store.images] == [f"{first + i:06d}.png" for i in want] == [os.path.basename(p) for p in kit.image_paths]
        assert [os.path.basename(p) for p in kit.store.masks] == [f"{first + i:06d}.png" for i in want]
        assert kit.smpl["betas"].shape == (1, 16) and np.array_equal(kit.smpl["betas"].numpy()[0], poses["betas"])
        for key in ("global_orient", "body_pose", "transl"):
            assert kit.smpl[key].dtype.is_floating_point and np.array_equal(kit.smpl[key].numpy(), poses[key][[first + i for i in want]]), (split, key)
        cam = kit.camera
        assert (cam["image_width"], cam["image_height"], cam["near"], cam["far"]) == (22, 9, 0.01, 100.0)
        assert cam["fovx"] == 2 * np.arctan(22 / (2 * 5000.0)) and cam["fovy"] == 2 * np.arctan(9 / (2 * 5000.0))
    assert g["val"]["22"] == [5, 16] and set(g["train"]["22"]) | set(g["val"]["22"]) == set(range(22))


def test_load_kit_reads_thetas_falls_back_to_poses_npz_and_takes_both_camera_branches(tmp_path, monkeypatch):
    from sings_amd import camera
    _stub(monkeypatch)
    root = str(tmp_path / "kit")
    _, _, poses = uc.write_kit(root, thetas=True, optimized=False, cx=3.0)
    kit = KIT.load_kit(root, split="train+val", device="cpu")
    assert np.array_equal(kit.smpl["body_pose"].numpy(), poses["body_pose"]) and np.array_equal(kit.smpl["global_orient"].numpy(), poses["global_orient"])
    cam = kit.camera                                              # cx = 3 of 22: off centre
    assert cam["fovx"] == float(np.arctan(3.0 / 5000.0) + np.arctan(19.0 / 5000.0))
    P = camera.get_projection_matrix_center(0.01, 100.0, 5000.0, 5000.0, 3.0, 4.5, 22, 9)
    assert np.array_equal(cam["full_proj_transform"].numpy(), (np.eye(4, dtype=np.float32) @ P.T).astype(np.float32))
    # the centred branch is make_camera's
    root2 = str(tmp_path / "kit2")
    uc.write_kit(root2)
    c2 = KIT.init_camera(os.path.join(root2, "score_demo_video", "cameras.npz"))
    m = camera.make_camera(np.eye(4), 5000.0, 5000.0, 11.0, 4.5, 22, 9)
    for key in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert np.array_equal(c2[key], m[key]), key
    assert c2["fovx"] == m["fovx"] and c2["fovy"] == m["fovy"]
    # the optimised poses are preferred when both exist
    np.savez(os.path.join(root, "score_demo_video", "poses_optimized.npz"), **{k: v + 1 for k, v in poses.items()})
    assert np.array_equal(KIT.load_kit(root, split="train+val", device="cpu").smpl["transl"].numpy(), poses["transl"] + 1)
    # the extrinsic must be the identity
    ext = np.eye(4)
    ext[0, 3] = 0.5
    np.savez(os.path.join(root, "score_demo_video", "cameras.npz"), intrinsic=np.eye(3), extrinsic=ext, height=np.int64(9), width=np.int64(22))
    with pytest.raises(ValueError, match="identity"):
        KIT.load_kit(root, split="train+val", device="cpu")


def test_load_kit_refusals_name_the_file(tmp_path, monkeypatch):
    from PIL import Image
    _stub(monkeypatch)
    root = str(tmp_path / "kit")
    rgb, mask, _ = uc.write_kit(root)
    with pytest.raises(ValueError, match="split"):
        KIT.load_kit(root, split="test", device="cpu")
    image, msk = os.path.join(root, "images", "000008.png"), os.path.join(root, "masks", "000009.png")
    keep = open(image, "rb").read(), open(msk, "rb").read()

    def refused(path, save, word):
        save(path)
        with pytest.raises(ValueError, match=word) as e:
            KIT.load_kit(root, split="train", device="cpu")
        assert os.path.basename(path) in str(e.value)
    refused(image, lambda p: Image.fromarray(mask[8], "L").save(p), "1 channels")
    refused(image, lambda p: Image.fromarray(rgb[8].astype(np.uint16).sum(-1).astype(np.uint16)).save(p), "bit depth 16")
    refused(image, lambda p: Image.fromarray(rgb[8], "RGB").convert("P").save(p), "colour type 3")
    refused(image, lambda p: Image.fromarray(rgb[8, :, :21].copy(), "RGB").save(p), "21 x 9")
    refused(image, lambda p: open(p, "wb").write(b"JFIF" * 20), "signature")
    open(image, "wb").write(keep[0])
    refused(msk, lambda p: Image.fromarray(rgb[9], "RGB").save(p), "3 channels")
    refused(msk, lambda p: Image.fromarray(mask[9], "L").convert("LA").save(p), "colour type 4")
    open(msk, "wb").write(keep[1])
    assert len(KIT.load_kit(root, split="train", device="cpu").indices) == 20
    # a file of the frames the split drops is not looked at
    open(os.path.join(root, "images", "000000.png"), "wb").write(b"junk")
    assert len(KIT.load_kit(root, split="val", device="cpu").indices) == 2
    os.remove(os.path.join(root, "masks", "000003.png"))
    with pytest.raises(ValueError, match="24 files in images/ and 23 in masks/"):
        KIT.load_kit(root, split="train", device="cpu")
    # without the stub: no GPU, no store -- never a host decode in its place
    monkeypatch.undo()
    root3 = str(tmp_path / "kit3")
    uc.write_kit(root3)
    with pytest.raises(RuntimeError, match="GPU"):
        KIT.load_kit(root3, split="train", device="cpu")
