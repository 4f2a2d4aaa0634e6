"""The device PNG encoder (include/sings_png.h, ``png.PngEncoder``) and what is built on it (``out="png"`` of the animation paths,
``png.animate_to_frames``, ``RunOutputs.device_png``).

The bar is exact: the device's bytes ARE the numpy twin's bytes (``png.png_encode_host``, which tests/test_png_host.py holds to the
format, to zlib and to PIL), for every case of tests/png_case.py -- every size, every filter, BGR -- chosen per segment and with each
candidate forced; a frame beyond its capacity reports what it needs and touches nothing; the call is legal inside a graph capture; the
animation paths hand out exactly the twin's encoding of their own 8-bit frames; a run with ``device_png`` leaves the files of a run
without it, pixel for pixel."""
import io
import os

import numpy as np
import pytest
import torch

import png_case as pc
from sings_amd import png as P

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _pixels(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- bytes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in pc.CASES])
def test_device_bytes_are_the_twins_bytes(name):
    _, frames, filter, rps, bgr = next(c for c in pc.CASES if c[0] == name)
    k, H, W = frames.shape[:3]
    enc = P.PngEncoder(W, H, k, _dev(), filter=filter, rows_per_segment=rps)
    assert enc.header == P.png_header(W, H) and len(enc.header) == P.HEADER_BYTES and enc.capacity == enc.layout["worst_bytes"]
    x = _t(frames)
    for force in range(-1, P.TABLES + 1):
        want, _ = pc.twin(name, force)
        need = [len(w) for w in want]
        if max(need) > enc.capacity:                              # (a forced table on bytes it does not suit: beyond the worst case)
            big = P.PngEncoder(W, H, k, _dev(), filter=filter, rows_per_segment=rps, capacity=max(need))
            assert enc.encode(x, bgr=bgr, force=force)[1].cpu().tolist() == [n if n <= enc.capacity else -n for n in need]
            assert big.encode_to_host(x, bgr=bgr, force=force) == want, (name, force)
            continue
        enc.buf.fill_(0xA5)
        buf, sizes = enc.encode(x, bgr=bgr, force=force)
        n = sizes.cpu().tolist()
        assert n == need, (name, force, n, need)
        rows = buf.cpu().numpy()
        for i in range(k):
            assert rows[i, :n[i]].tobytes() == want[i], (name, force, i)
            assert (rows[i, n[i]:] == 0xA5).all(), "nothing behind a frame's last byte"
    want, _ = pc.twin(name)
    assert enc.encode_to_host(x, bgr=bgr) == want
    if k > 1:                                                     # one frame of the batch alone: the second
        assert enc.encode_to_host(x[1:2], bgr=bgr) == want[1:2]
    expect = frames[..., ::-1] if bgr else frames
    for i in range(k):
        assert np.array_equal(_pixels(want[i]), expect[i])


def test_fewer_frames_than_K_leave_the_other_rows_untouched():
    _, frames, filter, rps, bgr = next(c for c in pc.CASES if c[0] == "85x7")
    want, _ = pc.twin("85x7")
    enc = P.PngEncoder(85, 7, 3, _dev())
    enc.buf.fill_(0xA5)
    enc.sizes.fill_(12345)
    buf, sizes = enc.encode(_t(frames[:2]))
    assert tuple(buf.shape) == (2, enc.capacity) and sizes.cpu().tolist() == [len(w) for w in want[:2]]
    assert (enc.buf[2].cpu().numpy() == 0xA5).all() and int(enc.sizes[2]) == 12345
    assert [buf[i, :len(want[i])].cpu().numpy().tobytes() for i in range(2)] == want[:2]


def test_a_frame_beyond_its_capacity_reports_what_it_needs_and_writes_nothing():
    _, frames, filter, rps, bgr = next(c for c in pc.CASES if c[0] == "200x40")
    want, _ = pc.twin("200x40")
    need = [len(w) for w in want]
    k = len(need)
    assert need == sorted(need) and need[-1] > need[0] + 64, "more noise, more bytes"
    cap = need[2]                                                 # frames 0..2 fit (the third exactly), 3 and 4 do not
    GUARD = 4096
    enc = P.PngEncoder(200, 40, k, _dev(), rows_per_segment=rps, capacity=cap)
    flat = torch.full((k * cap + GUARD,), 0xA5, dtype=torch.uint8, device=_dev())
    sizes = torch.full((k,), 12345, dtype=torch.int32, device=_dev())
    _, got = enc.encode(_t(frames), out=(flat[:k * cap].view(k, cap), sizes))
    torch.cuda.synchronize()
    assert got.cpu().tolist() == [n if n <= cap else -n for n in need]
    host = flat.cpu().numpy()
    assert (host[k * cap:] == 0xA5).all(), "the guard bytes are unchanged"
    for i in range(k):
        row = host[i * cap:(i + 1) * cap]
        if need[i] <= cap:
            assert row[:need[i]].tobytes() == want[i] and (row[need[i]:] == 0xA5).all()
        else:
            assert (row == 0xA5).all(), "the frame that does not fit wrote nothing"
    # a capacity of exactly the need fits; one byte less does not
    exact = P.PngEncoder(200, 40, 1, _dev(), rows_per_segment=rps, capacity=need[0])
    assert exact.encode(_t(frames[:1]))[1].cpu().tolist() == [need[0]]
    short = P.PngEncoder(200, 40, 1, _dev(), rows_per_segment=rps, capacity=need[0] - 1)
    short.buf.fill_(0xA5)
    assert short.encode(_t(frames[:1]))[1].cpu().tolist() == [-need[0]] and (short.buf.cpu().numpy() == 0xA5).all()
    with pytest.raises(RuntimeError, match=f"needs {need[0]} bytes"):
        short.encode_to_host(_t(frames[:1]))


def test_encode_inside_a_graph_capture_replays_on_new_frames():
    _, frames, filter, rps, bgr = next(c for c in pc.CASES if c[0] == "200x40")
    enc = P.PngEncoder(200, 40, len(frames), _dev(), rows_per_segment=rps)
    static = _t(frames)
    enc.encode(static)                                                # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf, sizes = enc.encode(static)
    other = np.ascontiguousarray(frames[::-1, :, ::-1])               # new contents: the frames in reverse order, mirrored
    static.copy_(_t(other))
    enc.buf.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    want = P.png_encode_host(other, rows_per_segment=rps)
    n = sizes.cpu().tolist()
    assert n == [len(w) for w in want]
    rows = buf.cpu().numpy()
    assert [rows[i, :n[i]].tobytes() for i in range(len(want))] == want and want != pc.twin("200x40")[0]


def test_every_refusal_of_the_header_returns_status_1_with_a_message():
    import ctypes as C
    from sings_amd import _lib
    lib = _lib.load()
    enc = P.PngEncoder(22, 9, 2, _dev())
    x = _t(next(c for c in pc.CASES if c[0] == "22x9")[1])
    out = (C.c_size_t * len(_lib.PNG_LAYOUT))()
    for args, text in (((0, 9, 1, 1, 47), "1..10922 wide"), ((10923, 9, 1, 1, 47), "1..10922 wide"), ((22, 0, 1, 1, 47), "high"),
                       ((22, 65536, 1, 1, 47), "high"), ((22, 9, 0, 1, 47), "K = 0"), ((22, 9, 17, 1, 47), "K = 17"),
                       ((22, 9, 1, 0, 47), "rows_per_segment = 0"), ((5000, 9, 1, 3, 47), "a segment holds"), ((22, 9, 1, 1, 0), "header_bytes"),
                       ((10922, 65535, 1, 1, 47), "2^31")):
        assert lib.sg_png_layout(*args, out) == 1 and text in lib.sg_last_error().decode(), args
    assert lib.sg_png_layout(22, 9, 1, 1, 47, None) == 1 and "null pointer" in lib.sg_last_error().decode()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(K=2, W=22, H=9, rps=enc.rows_per_segment, filter=5, bgr=0, force=-1, frames=p(x), tables=p(enc._tables), header=p(enc._header),
                hb=47, ws=p(enc._ws), wsb=enc._ws.numel(), out=p(enc.buf), cap=enc.capacity, sizes=p(enc.sizes), stream=st)
    call = lambda **kw: lib.sg_png_encode_frames(*{**good, **kw}.values())
    assert call() == 0
    for kw, text in ((dict(frames=None), "null pointer"), (dict(tables=None), "null pointer"), (dict(header=None), "null pointer"),
                     (dict(ws=None), "null pointer"), (dict(out=None), "null pointer"), (dict(sizes=None), "null pointer"),
                     (dict(W=0), "wide"), (dict(H=0), "high"), (dict(K=17), "K = 17"), (dict(rps=0), "a segment holds"),
                     (dict(filter=6), "filter = 6"), (dict(filter=-1), "filter = -1"), (dict(force=6), "force = 6"), (dict(force=-2), "force = -2"),
                     (dict(cap=0), "capacity"), (dict(cap=2 ** 31), "capacity"), (dict(wsb=enc.layout["ws_bytes"] - 1), "workspace"),
                     (dict(ws=C.c_void_p(enc._ws.data_ptr() + 4)), "16-byte aligned")):
        assert call(**kw) == 1 and text in lib.sg_last_error().decode(), kw
    torch.cuda.synchronize()
    for bad in (x.cpu(), x.float(), x[:, :, :8], torch.cat([x, x]), x[0]):
        with pytest.raises(ValueError, match="PngEncoder.encode"):
            enc.encode(bad)
    with pytest.raises(ValueError, match="force = 6"):
        enc.encode(x, force=6)
    with pytest.raises(ValueError, match="K = 17"):
        P.PngEncoder(22, 9, 17, _dev())
    with pytest.raises(ValueError, match="filter must be one of"):
        P.PngEncoder(22, 9, 1, _dev(), filter="best")


# ---- the animation paths ---------------------------------------------------------------------------------------------------------
def test_animate_chunk_hands_out_the_twins_streams_and_files_of_them(tmp_path):
    from test_gpu_video import F_A, H_A, W_A, _one_avatar
    from sings_amd.posed import animate_chunk
    canon, poses, jr, A_cano, data, kw = _one_avatar()
    bg = torch.ones(3, device=_dev())
    rgb8 = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=3, out="rgb8", **kw))
    frames = np.stack([rgb8[f].cpu().numpy() for f in range(F_A)])
    assert frames.shape == (F_A, H_A, W_A, 3) and frames.min() < 250, "the avatar is in view"
    want = P.png_encode_host(frames)
    assert len(set(want)) == F_A, "five different frames"
    for K in (1, 3):                                              # 3: 3 + 2 (a padded last batch)
        got = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=K, out="png", **kw))
        assert sorted(got) == list(range(F_A))
        for f in range(F_A):
            assert isinstance(got[f], bytes) and got[f] == want[f], (K, f)
    assert np.array_equal(_pixels(want[0]), frames[0])
    with pytest.raises(ValueError, match="out must be one of"):
        next(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=3, out=("png", 3), **kw))
    d = str(tmp_path / "frames")
    assert P.animate_to_frames(d, canon, poses, jr, A_cano, data, bg, frames_per_launch=3, **kw) == F_A
    assert sorted(os.listdir(d)) == [f"{f:05d}.png" for f in range(F_A)]
    assert [open(os.path.join(d, f"{f:05d}.png"), "rb").read() for f in range(F_A)] == want


# ---- the run's outputs -----------------------------------------------------------------------------------------------------------
def test_a_run_with_device_png_leaves_the_files_of_a_run_without(tmp_path):
    from sings_amd import canonical as cn
    from sings_amd import frame_feed as ff
    from sings_amd.run_outputs import RunOutputs
    from test_gpu_frame_feed_train import SEED, STILL_LRS, _feed_trainer, _quantised, _reset
    from test_gpu_pose_train import _pose_scene
    dev = _dev()
    sc = _pose_scene()
    try:
        rgb_u8, mask_u8 = _quantised(sc, dev)
        _reset()
        store = ff.FrameStore(rgb_u8, mask_u8, device=dev)
        A = cn.static_A("da_pose", _t(sc["joints"]), torch.inverse(_t(sc["post"])), sc["parents"])
        files = {}
        for flag in (False, True):
            logdir = str(tmp_path / f"run{int(flag)}")
            used = []
            ro = RunOutputs(logdir, A, _t(np.array([1.0, 1.0, 1.0], np.float32)), viz_interval=3, progress_interval=2, canon_nframes=3,
                            save_ply=False, write=(lambda path, array: used.append(path)) if flag else None)
            assert ro.device_png is False
            ro.canon_size, ro.progress_size, ro.frames_per_launch, ro.device_png = (48, 64), (32, 32), 2, flag
            tr = _feed_trainer(sc, dev, "fused", True, ff.FrameFeed(store, seed=SEED), lrs=STILL_LRS)
            tr.set_outputs(ro)
            for t in range(4):
                tr.step_next()
            ro.finish()
            assert not used, "write is used for nothing with device_png"
            files[flag] = {os.path.relpath(os.path.join(d, f), logdir): os.path.join(d, f) for d, _, fs in os.walk(logdir) for f in fs}
            _reset()
            del tr
        want = ({f"train/{t:06d}.png" for t in (0, 3)} | {f"canon/{i:05d}.png" for i in range(3)} | {f"train_progress/{t:06d}.png" for t in (0, 2)})
        assert set(files[False]) == set(files[True]) == want
        for rel in sorted(want):
            a, b = _pixels(open(files[False][rel], "rb").read()), _pixels(open(files[True][rel], "rb").read())
            assert a.shape == b.shape and np.array_equal(a, b), rel
            # the device's file is the twin's encoding of those pixels
            assert open(files[True][rel], "rb").read() == P.png_encode_host(a)[0], rel
        assert _pixels(open(files[True]["canon/00000.png"], "rb").read()).min() < 255, "the avatar is in the turntable's view"
    finally:
        _reset()
