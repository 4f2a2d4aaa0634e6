"""Host tests of sings_amd/video.py (include/sings_jpeg.h, ``_lib._PROTOTYPES_JPEG``): the tables are the Annex K tables a libjpeg file
carries, the numpy twin writes the stream INTEGRATION.md §23 fixes -- checked by a marker walker written here and by a decoder we did
not write (PIL's libjpeg) -- its quality is libjpeg's within a measured margin, and ``MjpegWriter`` writes the RIFF AVI a walker
written here reads back.  The device path is held to the twin's bytes in tests/test_gpu_video.py."""
import ctypes as C
import io
import os
import re
import struct

import numpy as np
import pytest

import video_case as vc
from sings_amd import _lib
from sings_amd import video as V

CASES = vc.cases()


def _ri(frame, ri):
    return (frame.shape[1] + 7) // 8 if ri is None else ri


def _pil_jpeg(frame, quality):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(frame, "RGB").save(f, "JPEG", quality=quality, subsampling=0, optimize=False)
    return f.getvalue()


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_jpeg.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_JPEG) == ["sg_jpeg_layout", "sg_jpeg_encode_frames"]
    assert not set(_lib._PROTOTYPES_JPEG) & set(_lib._PROTOTYPES) and "sg_jpeg_layout" not in _lib.EXPORTS and _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert _lib.HAS_JPEG
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
    for name, value in (("MAX_FRAMES", V.MAX_FRAMES), ("MAX_DIM", V.MAX_DIM), ("TABLE_WORDS", V.TABLE_WORDS), ("HUFF_STRIDE", V.HUFF_STRIDE)):
        assert int(re.search(rf"#define\s+SG_JPEG_{name}\s+(\d+)", text).group(1)) == value == getattr(_lib, "JPEG_" + name)
    assert int(re.search(r"#define\s+SG_JPEG_LAYOUT_WORDS\s+(\d+)", text).group(1)) == len(_lib.JPEG_LAYOUT)


def test_layout_and_refusals_come_before_any_hip_call():
    from sings_amd import _marshal
    L = _marshal.jpeg_layout(512, 896, 8, 64, 623)
    assert L["mcus"] == 64 * 112 and L["segments"] == 112 and L["slot_pitch"] >= 64 * _lib.JPEG_MCU_BYTES
    assert L["default_capacity"] == 623 + 512 * 896 * 3 // 2 and L["worst_bytes"] >= 623 + L["mcus"] * _lib.JPEG_MCU_BYTES
    assert L["ws_bytes"] >= 8 * (L["mcus"] * 384 + L["segments"] * L["slot_pitch"])
    assert _marshal.jpeg_layout(13, 21, 1, 65535, 623)["segments"] == 1
    for args, word in (((0, 8, 1, 1, 623), "pixels"), ((8, 65536, 1, 1, 623), "pixels"), ((8, 8, 0, 1, 623), "K = 0"),
                       ((8, 8, 17, 1, 623), "K = 17"), ((8, 8, 1, 0, 623), "restart_interval"), ((8, 8, 1, 65536, 623), "restart_interval"),
                       ((65535, 65535, 1, 1, 623), "2\\^31")):
        with pytest.raises(RuntimeError, match=word):
            _marshal.jpeg_layout(*args)
    with pytest.raises(ValueError, match="quality"):
        V.quant_tables(0)
    with pytest.raises(ValueError, match="restart_interval"):
        V.jpeg_header(8, 8, 90, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.JpegEncoder(8, 8, 1, "cpu")


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def test_tables_are_the_golden_tables(repo_root):
    g = np.load(os.path.join(repo_root, "tests", "golden", "jpeg_tables.npz"))
    assert g["quant_luma"][:8].tolist() == [16, 11, 12, 14, 12, 10, 16, 14] and len(g["ac0_vals"]) == 162
    assert g["dc0_bits"].tolist() == [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(g["quant_luma"], V.QUANT_LUMA) and np.array_equal(g["quant_chroma"], V.QUANT_CHROMA)
    for name, bits, vals in V.HUFFMAN:
        assert np.array_equal(g[name + "_bits"], bits) and np.array_equal(g[name + "_vals"], vals), name
        assert sum(bits) == len(vals) == len(set(vals))
    assert all(int(x) == 1 for t in V.quant_tables(100) for x in t)
    assert V.ZIGZAG[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and sorted(V.ZIGZAG.tolist()) == list(range(64))


def test_device_tables_restate_the_host_tables():
    t = V.device_tables(75)
    assert t.dtype == np.uint32 and t.shape == (V.TABLE_WORDS,)
    assert np.array_equal(t[:64].view(np.float32).reshape(8, 8), V.dct_basis())
    ql, qc = V.quant_tables(75)
    pos = t[192:256].astype(np.int64)
    assert sorted(pos.tolist()) == list(range(64)) and np.array_equal(V.ZIGZAG[pos], np.arange(64))
    assert np.array_equal(t[64:128].view(np.float32), ql[pos].astype(np.float32))
    assert np.array_equal(t[128:192].view(np.float32), qc[pos].astype(np.float32))
    for c in (0, 1):
        base = 256 + V.HUFF_STRIDE * c
        assert int(np.count_nonzero(t[base:base + 16])) == 12 and int(np.count_nonzero(t[base + 16:base + 272])) == 162
        assert int((t[base:base + 272] & 255).max()) <= 16


def test_dct_basis_is_orthonormal_and_rounded_once():
    Cb = V.dct_basis()
    assert Cb.dtype == np.float32
    assert np.abs(Cb.astype(np.float64) @ Cb.astype(np.float64).T - np.eye(8)).max() < 1e-7
    assert Cb[0, 0] == np.float32(0.5 / np.sqrt(2.0))


@pytest.mark.parametrize("q", [1, 25, 50, 75, 90, 100])
def test_dqt_bytes_are_libjpegs_at_the_same_quality(q):
    pytest.importorskip("PIL")
    frame = CASES["16x8"][0]
    mine = vc.walk_jpeg(V.jpeg_encode_host(frame, q)[0])["segments"][vc.DQT]
    theirs = b"".join(vc.walk_jpeg(_pil_jpeg(frame, q))["segments"][vc.DQT])         # (libjpeg may put both tables in one segment)
    assert b"".join(mine) == theirs


def test_dht_bytes_are_libjpegs():
    pytest.importorskip("PIL")
    frame = CASES["16x8"][0]
    mine = vc.walk_jpeg(V.jpeg_encode_host(frame, 50)[0])["segments"][vc.DHT]
    theirs = b"".join(vc.walk_jpeg(_pil_jpeg(frame, 50))["segments"][vc.DHT])
    assert sorted(len(m) for m in mine) == [29, 29, 179, 179]
    assert all(m in theirs for m in mine) and sum(len(m) for m in mine) == len(theirs)


# ---- the stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_marker_walker_finds_the_fixed_stream(name):
    frame, q, ri = CASES[name]
    H, W = frame.shape[:2]
    data = V.jpeg_encode_host(frame, q, ri)[0]
    w = vc.check_stream(data, W, H, _ri(frame, ri))
    assert data.startswith(V.jpeg_header(W, H, q, ri)) and len(V.jpeg_header(W, H, q, ri)) == len(data) - len(w["entropy"]) - 2
    nmcu = ((W + 7) // 8) * ((H + 7) // 8)
    assert len(w["pieces"]) == -(-nmcu // _ri(frame, ri))


def test_the_cases_reach_what_they_are_there_for():
    log = {}
    walk = {}
    for name, (frame, q, ri) in CASES.items():
        log[name] = []
        walk[name] = vc.walk_jpeg(V.jpeg_encode_host(frame, q, ri, symbol_log=log[name])[0])
    assert walk["96x80_rows"]["rst"] == [0, 1, 2, 3, 4, 5, 6, 7, 0], "10 segments: the RST numbering wraps"
    assert len(walk["96x80_ri5"]["pieces"]) == 24 and len(walk["96x80_ri7"]["pieces"]) == 18      # (120 = 17 * 7 + 1: a short last one)
    assert set(log["constant"]) == {0x00}, "a constant image is DC and EOB only"
    assert walk["noise_q100"]["stuffed"] >= 1 and walk["noise_q100_ri48"]["stuffed"] >= 1, "byte stuffing occurs"
    assert 0xF0 in log["cosine_q10"], "ZRL occurs"
    assert 0x00 in log["noise_q100"] or len(log["noise_q100"]) > 0
    # the checkerboard's DC differences: white 8 * (255 - 128) = 1016 against black -1024: category 11
    q = V.jpeg_coefficients(CASES["checkerboard_q100"][0], 100)
    assert sorted(set(q[..., 0, 0].ravel().tolist())) == [-1024, 1016] and abs(1016 + 1024).bit_length() == 11
    # a block whose coefficient 63 is not zero ends without EOB
    q = V.jpeg_coefficients(CASES["noise_q100"][0], 100)
    assert (q[..., 63] != 0).any()
    assert walk["one_segment"]["rst"] == []


@pytest.mark.parametrize("name", list(CASES))
def test_pil_decodes_every_stream(name):
    pytest.importorskip("PIL")
    frame, q, ri = CASES[name]
    im = _decode(V.jpeg_encode_host(frame, q, ri)[0])
    assert im.mode == "RGB" and im.size == (frame.shape[1], frame.shape[0])
    err = np.abs(np.asarray(im).astype(np.int32) - frame.astype(np.int32))
    if name in ("constant", "checkerboard_q100"):
        assert err.max() <= 2, err.max()                              # flat blocks come back as they went in


def test_restart_interval_does_not_change_the_picture():
    pytest.importorskip("PIL")
    frame = CASES["96x80_rows"][0]
    a, b, c = (np.asarray(_decode(V.jpeg_encode_host(frame, 90, ri)[0])) for ri in (None, 5, 65535))
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_edges_repeat_the_last_column_and_row():
    frame = CASES["13x21_edges"][0]
    padded = np.pad(frame, ((0, 3), (0, 3), (0, 0)), mode="edge")
    assert np.array_equal(V.jpeg_coefficients(frame, 75), V.jpeg_coefficients(padded, 75))


def test_bgr_on_swapped_channels_gives_the_bytes_of_rgb():
    frame, q, ri = CASES["96x80_ri5"]
    want = V.jpeg_encode_host(frame, q, ri)
    assert V.jpeg_encode_host(np.ascontiguousarray(frame[..., ::-1]), q, ri, bgr=True) == want
    assert V.jpeg_encode_host(frame, q, ri, bgr=True) != want
    three = np.stack([frame, frame[::-1], frame[:, ::-1]])
    assert V.jpeg_encode_host(three, q, ri) == [V.jpeg_encode_host(f, q, ri)[0] for f in three]


# ---- quality ---------------------------------------------------------------------------------------------------------------------
# The twin's float DCT against libjpeg's integer one: PSNR(libjpeg) - PSNR(twin) measured with the twin on the CPU over these images
# and qualities was +0.209 dB at most (gradient, q 50; the others -0.164 .. +0.065: LAB.md "JPEG on the device").  Three times that.
PSNR_MARGIN_DB = 0.63


def _psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("image", ["gradient", "noise", "avatar"])
def test_quality_is_libjpegs_within_the_measured_margin(image, q):
    pytest.importorskip("PIL")
    frame = {"gradient": lambda: vc.gradient(64, 48), "noise": lambda: vc._noise(64, 48, 11), "avatar": lambda: vc.avatar_like(96, 80)}[image]()
    mine = _psnr(np.asarray(_decode(V.jpeg_encode_host(frame, q)[0])), frame)
    theirs = _psnr(np.asarray(_decode(_pil_jpeg(frame, q))), frame)
    print(f"{image} q={q}: twin {mine:.4f} dB, libjpeg {theirs:.4f} dB, gap {theirs - mine:+.4f} dB")
    assert mine >= theirs - PSNR_MARGIN_DB, (mine, theirs)


# ---- AVI -------------------------------------------------------------------------------------------------------------------------
def _payloads():
    even = V.jpeg_encode_host(CASES["16x8"][0], 90)[0]
    return [even, even + b"\x00" if len(even) % 2 else even[:-2] + b"\x00\xff\xd9", b"\xff\xd8odd\xff\xd9", even]


def test_mjpeg_writer_writes_the_avi_a_riff_walker_reads_back(tmp_path):
    path = str(tmp_path / "clip.avi")
    frames = _payloads()
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)
    with V.MjpegWriter(path, 16, 8, 20) as w:
        for f in frames:
            w.write(f)
        assert not os.path.exists(path), "the file appears under its name on close"
    data = open(path, "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == ["clip.avi"]
    r = vc.walk_riff(data)
    avih = struct.unpack("<14I", r["avih"])
    assert avih[0] == 50000 and avih[4] == len(frames) and avih[6] == 1 and avih[8:10] == (16, 8) and avih[3] & 0x10
    assert avih[7] == max(len(f) for f in frames)
    strh = struct.unpack("<4s4sIHHIIIIIIII4h", r["strh"])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and (strh[7], strh[6]) == (20, 1) and strh[9] == len(frames)
    strf = struct.unpack("<IiiHH4sIiiII", r["strf"])
    assert strf[:6] == (40, 16, 8, 1, 24, b"MJPG")
    assert r["frames"] == frames
    assert r["padded"] == [bool(len(f) & 1) for f in frames]
    assert len(r["idx1"]) == len(frames)
    for (tag, flags, off, n), f, at in zip(r["idx1"], frames, r["offsets"]):
        assert tag == b"00dc" and flags & 0x10 and n == len(f) and off == at
        chunk = r["movi_at"] + off
        assert data[chunk:chunk + 4] == b"00dc" and struct.unpack("<I", data[chunk + 4:chunk + 8])[0] == n
        assert data[chunk + 8:chunk + 8 + n] == f


@pytest.mark.parametrize("fps,usec,rate,scale", [(10, 100000, 10, 1), (29.97, 33367, 2997, 100), (0.5, 2000000, 1, 2)])
def test_mjpeg_writer_turns_fps_into_scale_and_rate(tmp_path, fps, usec, rate, scale):
    path = str(tmp_path / "t.avi")
    with V.MjpegWriter(path, 8, 8, fps) as w:
        w.write(b"\xff\xd8\xff\xd9")
    r = vc.walk_riff(open(path, "rb").read())
    strh = struct.unpack("<4s4sIHHIIIIIIII4h", r["strh"])
    assert struct.unpack("<14I", r["avih"])[0] == usec and (strh[7], strh[6]) == (rate, scale)


def test_mjpeg_writer_raises_before_two_gib_and_keeps_the_file_valid(tmp_path, monkeypatch):
    path = str(tmp_path / "big.avi")
    w = V.MjpegWriter(path, 8, 8, 20)
    assert w.MAX_BYTES == 2 ** 31 - 1
    w.write(b"\xff\xd8\xff\xd9")
    w._bytes = 2 ** 31 - 1 - 8 - 4 - 8 - 32 + 1                       # (a stubbed size: one byte too many for a 4-byte frame and the index)
    with pytest.raises(RuntimeError, match="2147483647"):
        w.write(b"\xff\xd8\xff\xd9")
    w._bytes -= 1
    assert w._final_bytes(4) == w.MAX_BYTES
    w.abort()
    assert os.listdir(str(tmp_path)) == []
    # with a small limit, for real: the refused frame is not written and the file closes whole
    monkeypatch.setattr(V.MjpegWriter, "MAX_BYTES", 400)
    with V.MjpegWriter(path, 8, 8, 20) as w:
        w.write(b"\xff\xd8" + b"x" * 60 + b"\xff\xd9")
        with pytest.raises(RuntimeError, match="would pass 400 bytes"):
            w.write(b"\xff\xd8" + b"x" * 60 + b"\xff\xd9")
    data = open(path, "rb").read()
    assert len(vc.walk_riff(data)["frames"]) == 1 and len(data) <= 400


def test_a_writer_closed_by_an_exception_leaves_no_file(tmp_path):
    path = str(tmp_path / "never.avi")
    with pytest.raises(KeyError):
        with V.MjpegWriter(path, 8, 8, 20) as w:
            w.write(b"\xff\xd8\xff\xd9")
            raise KeyError("stop")
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(ValueError, match="after close"):
        w.write(b"")
    # an existing file is replaced only by a finished one
    open(path, "wb").write(b"old")
    with pytest.raises(KeyError):
        with V.MjpegWriter(path, 8, 8, 20):
            raise KeyError("stop")
    assert open(path, "rb").read() == b"old"


# ---- the animation paths know the new output --------------------------------------------------------------------------------------
def test_out_jpeg_is_an_output_of_the_animation_paths():
    import inspect
    from sings_amd import posed, run_outputs, scene_anim
    from sings_amd.frame_out import parse_out
    assert parse_out("jpeg").bgr is False and parse_out("bgr8").bgr is True and parse_out("float32").bgr is None
    assert parse_out(("jpeg", 75)).bgr is False
    assert parse_out("jpeg")[1:] == ("jpeg", 90) and parse_out(("jpeg", 75))[1:] == ("jpeg", 75) and parse_out("bgr8")[1:] == (None, None)
    for bad in (("jpeg", 0), ("jpeg", 101), ("jpeg", 7.5)):
        with pytest.raises(ValueError, match="quality"):
            parse_out(bad)
    for bad in (("png", 3), "jpg", None):
        with pytest.raises(ValueError, match="out must be one of"):
            parse_out(bad)
    for fn in (posed.FrameAnimator.render_frames_batched, posed.animate_chunk, scene_anim.SceneAnimator.render_frames_batched,
               scene_anim.animate_scene):                            # (the quality travels in ``out``: the signatures are what they were)
        assert list(inspect.signature(fn).parameters)[-2:] == ["out", "return_aux"]
    sig = inspect.signature(V.animate_to_video).parameters
    assert (sig["fps"].default, sig["quality"].default, sig["frames_per_launch"].default) == (20, 90, 8)
    ro = run_outputs.RunOutputs("log", None, None, viz_interval=1, write=lambda p, a: None)
    assert ro.progress_video is False and (ro.video_name, ro.video_quality) == ("progress", 90)     # attributes, like the sizes: off by default
    ro.finish()                                                       # nothing to close without the video
    assert ro.video_path == os.path.join("log", "train_progress.avi")
