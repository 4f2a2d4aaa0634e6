"""Host tests of sings_amd/png.py (include/sings_png.h, ``_lib._PROTOTYPES_PNG``): the pre-built Huffman tables are complete codes that
zlib's inflate accepts, and the numpy twin writes the stream INTEGRATION.md §24 fixes -- checked by a chunk walker written here and by
two decoders we did not write (zlib and PIL).  Everything is exact.  The device path is held to the twin's bytes in
tests/test_gpu_png.py."""
import ctypes as C
import importlib.util
import inspect
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

import png_case as pc
from sings_amd import _lib
from sings_amd import png as P


def _pixels(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGB"
    return np.array(im)


def _chunks(data):
    """A PNG file -> [(type, data)], every length and CRC-32 checked, nothing before, between or behind the chunks."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert len(body) == n and struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), (at, kind)
        out.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return out


# ---- the header and its table ----------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_png.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_PNG) == ["sg_png_layout", "sg_png_encode_frames"]
    assert not set(_lib._PROTOTYPES_PNG) & set(_lib._PROTOTYPES) and not set(_lib._PROTOTYPES_PNG) & set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert _lib.HAS_PNG
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
    for name in ("MAX_FRAMES", "MAX_WIDTH", "MAX_HEIGHT", "MAX_SEGMENT_BYTES", "HEADER_BYTES", "TABLES", "TABLE_STRIDE", "PREFIX_STRIDE",
                 "T_PREFIX", "T_CRC", "T_POW", "POW_WORDS", "TABLE_WORDS"):
        assert int(re.search(rf"#define\s+SG_PNG_{name}\s+(\d+)", text).group(1)) == getattr(P, name) == getattr(_lib, "PNG_" + name), name
    assert (P.MAX_SEGMENT_BYTES, P.TABLES, P.MAX_WIDTH) == (32768, 5, 10922) and 1 + 3 * P.MAX_WIDTH <= P.MAX_SEGMENT_BYTES < 1 + 3 * (P.MAX_WIDTH + 1)
    assert int(re.search(r"#define\s+SG_PNG_LAYOUT_WORDS\s+(\d+)", text).group(1)) == len(_lib.PNG_LAYOUT)
    for i, f in enumerate(P.FILTERS):
        assert int(re.search(rf"#define\s+SG_PNG_FILTER_{f.upper()}\s+(\d+)", text).group(1)) == i
    assert _lib.PNG_FILTER_ADAPTIVE == P.FILTERS.index("adaptive")


def test_layout_and_refusals_come_before_any_hip_call():
    from sings_amd import _marshal
    L = _marshal.png_layout(896, 512, 8, 6, 47)
    n = 6 * (1 + 3 * 896)
    assert L["segments"] == 86 and L["segment_bytes"] == n and L["slot_pitch"] >= n + 5 and L["slot_pitch"] % 16 == 0
    assert L["worst_bytes"] == 47 + 512 * (1 + 3 * 896) + 86 * 17 + 30          # header + sum(n + 17) + 30
    assert L["ws_bytes"] >= 8 * (512 * (1 + 3 * 896) + 86 * L["slot_pitch"])
    assert _marshal.png_layout(13, 21, 1, 1000, 47)["segments"] == 1
    for args, word in (((0, 8, 1, 1, 47), "pixels"), ((10923, 8, 1, 1, 47), "pixels"), ((8, 65536, 1, 1, 47), "pixels"), ((8, 8, 0, 1, 47), "K = 0"),
                       ((8, 8, 17, 1, 47), "K = 17"), ((8, 8, 1, 0, 47), "rows_per_segment"), ((5000, 8, 1, 3, 47), "a segment holds"),
                       ((8, 8, 1, 1, 0), "header_bytes"), ((10922, 65535, 1, 1, 47), "2\\^31")):
        with pytest.raises(RuntimeError, match=word):
            _marshal.png_layout(*args)
    lib = _lib.load()
    assert lib.sg_png_layout(8, 8, 1, 1, 47, None) == 1 and b"null pointer" in lib.sg_last_error()
    # every refusal of the encode call that needs no device memory: null pointers come first
    assert lib.sg_png_encode_frames(1, 8, 8, 1, 5, 0, -1, None, None, None, 47, None, 0, None, 100, None, None) == 1
    assert b"null pointer" in lib.sg_last_error()
    # the python side
    assert P._check_geometry(896, 512, None) == (896, 512, 6) and P._check_geometry(10922, 3, None)[2] == 1
    for W, H, rps in ((0, 1, None), (10923, 1, None), (1, 65536, None), (8, 8, 0), (5000, 8, 3)):
        with pytest.raises(ValueError):
            P._check_geometry(W, H, rps)
    with pytest.raises(RuntimeError, match="MI355X only"):
        P.PngEncoder(8, 8, 1, "cpu")
    with pytest.raises(ValueError, match="K = 17"):
        P.PngEncoder(8, 8, 17, "cpu")
    with pytest.raises(ValueError, match="filter must be one of"):
        P.PngEncoder(8, 8, 1, "cpu", filter="best")
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            P.png_encode_host(bad)
    with pytest.raises(ValueError, match="force"):
        P.png_encode_host(np.zeros((4, 4, 3), np.uint8), force=6)
    with pytest.raises(ValueError, match="filter must be one of"):
        P.png_encode_host(np.zeros((4, 4, 3), np.uint8), filter="best")


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def test_dynamic_tables_are_complete_codes_and_the_literals_are_what_the_tool_generates(repo_root):
    assert len(P.CODE_LENGTHS) == P.TABLES - 1
    for lengths in P.CODE_LENGTHS:
        assert len(lengths) == 286 and min(lengths) >= 1 and max(lengths) <= 15
        assert sum(1 << (15 - n) for n in lengths) == 1 << 15, "a Kraft sum of exactly 1"
    spec = importlib.util.spec_from_file_location("png_tables_tool", os.path.join(repo_root, "tools", "png_tables.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.code_lengths() == tuple(tuple(t) for t in P.CODE_LENGTHS)
    # the model: cheaper near 0 and 255, every next table flatter
    for a, b in zip(P.CODE_LENGTHS, P.CODE_LENGTHS[1:]):
        assert a[0] <= b[0] and a[40] >= b[40] and a[255] <= a[128]
    # the fixed code is RFC 1951's
    assert len(P.FIXED_LENGTHS) == 288 and P.canonical_codes(P.FIXED_LENGTHS)[0] == int("00110000"[::-1], 2)
    assert P.canonical_codes(P.FIXED_LENGTHS)[256] == 0 and P.canonical_codes(P.FIXED_LENGTHS)[144] == int("110010000"[::-1], 2)


def test_every_table_inflates_and_the_device_words_hold_it():
    tabs = P.png_tables()
    words = P.device_tables()
    assert len(tabs) == P.TABLES and words.shape == (P.TABLE_WORDS,) and words.dtype == np.uint32
    for t, tab in enumerate(tabs):
        # prefix + end of block as a final block: a complete deflate stream of nothing
        value, bits = tab["prefix"]
        b = P._Bits()
        b.put(value | 1, bits)
        b.put(*tab["lit"][256])
        d = zlib.decompressobj(-15)
        assert d.decompress(b.bytes()) == b"" and d.eof, t
        # every literal and every match length through the table: zlib gives the bytes back
        b = P._Bits()
        b.put(value | 1, bits)
        want = bytearray()
        for v in range(256):
            b.put(*tab["lit"][v])
            want.append(v)
        for m in range(3, 259):
            b.put(*tab["lit"][m & 255])
            b.put(*tab["match"][m])
            want.extend(bytes([m & 255]) * (m + 1))
        b.put(*tab["lit"][256])
        d = zlib.decompressobj(-15)
        assert d.decompress(b.bytes()) == bytes(want) and d.eof, t
        base = t * P.TABLE_STRIDE
        assert [int(w) for w in words[base:base + 257]] == [v << 8 | n for v, n in tab["lit"]]
        assert [int(w) for w in words[base + 257:base + 513]] == [tab["match"][m][0] << 8 | tab["match"][m][1] for m in range(3, 259)]
        assert max(n for _, n in tab["match"].values()) <= 25 and max(n for _, n in tab["lit"]) <= 15
        at = P.T_PREFIX + t * P.PREFIX_STRIDE
        assert int(words[at]) == bits and sum(int(w) << (32 * i) for i, w in enumerate(words[at + 1:at + P.PREFIX_STRIDE])) == value
    assert tabs[0]["prefix"] == (2, 3) and all(tab["prefix"][1] == 1222 for tab in tabs[1:])
    # the CRC tables: the byte table is zlib's, and x^(8 2^j) appends 2^j zero bytes to a register
    reg = lambda data, r=0: zlib.crc32(data, r ^ 0xFFFFFFFF) ^ 0xFFFFFFFF                 # the raw register after `data`, from r
    for j in range(P.POW_WORDS - 3):                              # (2^16 zero bytes at the most here)
        assert P._crc_mul(0xDEADBEEF, int(words[P.T_POW + j])) == reg(bytes(1 << j), 0xDEADBEEF), j
    assert [int(words[P.T_CRC + i]) for i in range(256)] == [reg(bytes([i])) for i in range(256)]


# ---- the stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in pc.CASES])
def test_twin_stream_is_the_fixed_layout_and_decodes_to_the_frame(name):
    _, frames, filter, rps, bgr = next(c for c in pc.CASES if c[0] == name)
    streams, log = pc.twin(name)
    k, H, W = frames.shape[:3]
    rps = P._check_geometry(W, H, rps)[2]
    nseg = (H + rps - 1) // rps
    assert len(streams) == k and len(log["candidates"]) == k * nseg and len(log["filters"]) == k * H
    for i, data in enumerate(streams):
        assert data[:P.HEADER_BYTES] == P.png_header(W, H)
        chunks = _chunks(data)
        assert [c[0] for c in chunks] == [b"IHDR"] + [b"IDAT"] * (nseg + 2) + [b"IEND"]
        assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0) and chunks[1][1] == b"\x78\x01" and chunks[-1][1] == b""
        lines = log["scanlines"][i]
        assert chunks[-2][1] == b"\x03\x00" + struct.pack(">I", zlib.adler32(lines))
        # zlib inflates the concatenated IDAT data to the twin's scanlines (and checks the Adler-32 itself)
        assert zlib.decompress(b"".join(c[1] for c in chunks[1:-1])) == lines
        # every segment on its own: byte aligned, no match reaches outside it, sizes as the closed form says
        for s in range(nseg):
            seg = lines[s * rps * (1 + 3 * W):(s + 1) * rps * (1 + 3 * W)]
            body, c = chunks[2 + s][1], log["candidates"][i * nseg + s]
            sizes = log["sizes"][i * nseg + s]
            assert len(body) == sizes[c] == min(sizes) and c == sizes.index(min(sizes)) and sizes[P.TABLES] == len(seg) + 5
            d = zlib.decompressobj(-15)
            assert d.decompress(body) == seg and not d.eof
            if c == P.TABLES:
                assert body == b"\x00" + struct.pack("<HH", len(seg), len(seg) ^ 0xFFFF) + seg
            else:
                assert (body[0] & 7) == (2 if c == 0 else 4) and body[-4:] == b"\x00\x00\xff\xff"
        assert len(data) <= P.HEADER_BYTES + sum(min(rps, H - r) * (1 + 3 * W) + 17 for r in range(0, H, rps)) + 30
        assert np.array_equal(_pixels(data), (frames[i, ..., ::-1] if bgr else frames[i]))
        got = np.frombuffer(lines, np.uint8).reshape(H, 1 + 3 * W)[:, 0]
        assert got.tolist() == log["filters"][i * H:(i + 1) * H]
        if filter != "adaptive":
            assert set(got.tolist()) == {P.FILTERS.index(filter)}


def test_filters_are_the_png_filters_by_a_plain_loop():
    frame = pc.body(9, 22, 6, 6)
    H, W = frame.shape[:2]
    raw = frame.reshape(H, 3 * W).astype(int)

    def plain(t, y, i):
        x = raw[y, i]
        a = raw[y, i - 3] if i >= 3 else 0
        b = raw[y - 1, i] if y else 0
        c = raw[y - 1, i - 3] if y and i >= 3 else 0
        if t == 4:
            p = a + b - c
            pa, pb, pc_ = abs(p - a), abs(p - b), abs(p - c)
            pred = a if pa <= pb and pa <= pc_ else b if pb <= pc_ else c
        else:
            pred = (0, a, b, (a + b) // 2)[t]
        return (x - pred) & 255
    every = np.array([[[plain(t, y, i) for i in range(3 * W)] for y in range(H)] for t in range(5)], dtype=np.uint8)
    for t, f in enumerate(P.FILTERS[:5]):
        lines, types = P.filter_scanlines(frame, f)
        assert (types == t).all() and np.array_equal(lines[:, 1:], every[t]) and (lines[:, 0] == t).all()
    lines, types = P.filter_scanlines(frame, "adaptive")
    cost = np.abs(every.view(np.int8).astype(int)).sum(axis=2)
    for y in range(H):
        best = min(range(5), key=lambda t: (cost[t, y], t))      # ties go to the lowest type
        assert types[y] == best and np.array_equal(lines[y, 1:], every[best, y])
    assert len(set(types.tolist())) > 1


def test_run_lengths_become_the_closed_form_tokens():
    def closed_form(v, L):
        m = L - 1
        out = [("lit", v)] + [("match", 258)] * (m // 258)
        m %= 258
        return out + ([("match", m)] if m >= 3 else [("lit", v)] * m)
    _, log = pc.twin("runs")
    want = [("lit", 0)]                                           # the filter byte
    for i, n in enumerate(pc.RUN_LENGTHS):
        want += closed_form(10 + 10 * (i % 2), n)
    assert log["tokens"] == [want]
    assert [t for t in want if t[0] == "match"] == [("match", n) for n in (3, 4, 257, 258, 258, 258, 258, 3, 258, 4, 258, 258, 258, 258)]
    assert closed_form(7, 260) == [("lit", 7), ("match", 258), ("lit", 7)] and closed_form(7, 261) == [("lit", 7), ("match", 258), ("lit", 7), ("lit", 7)]
    # one run that is the whole segment
    _, log = pc.twin("black-85x7")
    n = 7 * 256
    assert log["tokens"] == [closed_form(0, n)] and log["tokens"][0] == [("lit", 0)] + [("match", 258)] * 6 + [("match", (n - 1) % 258)]
    # a run cut by a segment boundary starts again with a literal
    streams, log = pc.twin("200x40")
    seg = 7 * 601
    assert log["tokens"][0] == closed_form(0, seg) and log["tokens"][1][:2] == [("lit", 0), ("match", 258)]
    assert log["scanlines"][0][seg - 1] == log["scanlines"][0][seg] == 0 and 40 % 7 == 5, "a run across the boundary; a short last segment"


def test_every_candidate_is_chosen_somewhere_and_random_bytes_are_stored():
    chosen = set()
    for name in ("1x1", "21x13", "200x40", "200x40-flat", "200x40-random"):
        chosen |= set(pc.twin(name)[1]["candidates"])
    assert chosen == set(range(P.TABLES + 1))
    assert set(pc.twin("200x40-random")[1]["candidates"]) == {P.TABLES}
    per_frame = np.array(pc.twin("200x40")[1]["candidates"]).reshape(len(pc.NOISE), -1)
    assert [np.bincount(row[2:5]).argmax() for row in per_frame] == [1, 1, 2, 3, 4], "more noise, a flatter table"


def test_forced_candidates_all_decode_to_the_same_pixels():
    _, frames, filter, rps, bgr = next(c for c in pc.CASES if c[0] == pc.NOISY)
    sizes = []
    for c in range(P.TABLES + 1):
        streams, log = pc.twin(pc.NOISY, c)
        assert set(log["candidates"]) == {c}
        for i, data in enumerate(streams):
            _chunks(data)
            assert np.array_equal(_pixels(data), frames[i]), (c, i)
        sizes.append([len(s) for s in streams])
    best = [len(s) for s in pc.twin(pc.NOISY)[0]]
    assert all(b <= min(col) for b, col in zip(best, zip(*sizes))) and len({tuple(s) for s in sizes}) == P.TABLES + 1


# ---- what is built on the encoder ------------------------------------------------------------------------------------------------
def test_animate_to_frames_and_device_png_attributes_defaults_and_refusals(tmp_path, monkeypatch):
    from sings_amd import posed, run_outputs, scene_anim
    sig = inspect.signature(P.animate_to_frames).parameters
    assert list(sig)[:7] == ["dirname", "canon", "poses", "joints_rest", "A_t2cano", "cameras", "bg_color"]
    assert (sig["pattern"].default, sig["frames_per_launch"].default) == ("{:05d}.png", 8)
    sig = inspect.signature(P.PngEncoder.__init__).parameters
    assert (sig["filter"].default, sig["rows_per_segment"].default, sig["capacity"].default) == ("adaptive", None, None)
    sig = inspect.signature(P.png_encode_host).parameters
    assert [sig[k].default for k in ("filter", "rows_per_segment", "bgr", "force", "log")] == ["adaptive", None, False, -1, None]
    from sings_amd.frame_out import parse_out
    assert parse_out("png").bgr is False and parse_out("png")[1:] == ("png", None)
    for fn in (posed.FrameAnimator.render_frames_batched, posed.animate_chunk, scene_anim.SceneAnimator.render_frames_batched,
               scene_anim.animate_scene):
        assert list(inspect.signature(fn).parameters)[-2:] == ["out", "return_aux"]
    for pattern in ("frame.png", "sub/{:05d}.png"):
        with pytest.raises(ValueError, match="pattern"):
            P.animate_to_frames(str(tmp_path / "a"), None, None, None, None, None, None, pattern=pattern)
    with pytest.raises(TypeError, match="out is not an argument"):
        P.animate_to_frames(str(tmp_path / "a"), None, None, None, None, None, None, out="rgb8")
    assert not os.path.exists(str(tmp_path / "a"))
    # an exception while the frames come leaves the files written so far, whole, and no partial one
    def frames(*a, **k):
        assert k["out"] == "png" and k["frames_per_launch"] == 3
        yield 0, b"first"
        yield 1, b"second"
        raise RuntimeError("the launch failed")
    monkeypatch.setattr(posed, "animate_chunk", frames)
    with pytest.raises(RuntimeError, match="the launch failed"):
        P.animate_to_frames(str(tmp_path / "b"), None, None, None, None, None, None, frames_per_launch=3)
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["00000.png", "00001.png"] and open(str(tmp_path / "b" / "00001.png"), "rb").read() == b"second"
    # ... and an exception inside a write leaves nothing under the name or beside it
    real = os.replace
    monkeypatch.setattr(os, "replace", lambda a, b: (_ for _ in ()).throw(OSError("disk full")))
    with pytest.raises(OSError, match="disk full"):
        P.write_atomic(str(tmp_path / "c.png"), b"data")
    monkeypatch.setattr(os, "replace", real)
    assert os.listdir(str(tmp_path)) == ["b"]
    P.write_atomic(str(tmp_path / "c.png"), b"data")
    assert open(str(tmp_path / "c.png"), "rb").read() == b"data" and sorted(os.listdir(str(tmp_path))) == ["b", "c.png"]
    # RunOutputs.device_png: an attribute, off by default; the constructor is what it was
    assert list(inspect.signature(run_outputs.RunOutputs.__init__).parameters) == [
        "self", "logdir", "A_static", "bg_color", "viz_interval", "progress_interval", "canon_nframes", "save_ply", "write"]
    ro = run_outputs.RunOutputs("log", None, None, viz_interval=1, write=lambda p, a: None)
    assert ro.device_png is False and ro.progress_video is False
    ro.device_png = True
    with pytest.raises((RuntimeError, AttributeError, TypeError)):   # no device: the encoder refuses a CPU tensor, nothing is written
        import torch
        ro._picture(str(tmp_path / "x" / "p.png"), torch.zeros((4, 4, 3), dtype=torch.uint8))
    assert not os.path.exists(str(tmp_path / "x"))
