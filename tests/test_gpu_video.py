"""The device JPEG encoder (include/sings_jpeg.h, ``video.JpegEncoder``) and what is built on it (``out="jpeg"`` of the animation paths,
``video.animate_to_video``, ``RunOutputs.progress_video``).

The bar: the device's bytes ARE the numpy twin's bytes (``video.jpeg_encode_host``, which tests/test_video_host.py holds to the format
and to libjpeg), for every frame of the host list, in launches of one frame and of three different frames, RGB and BGR; a frame beyond
its capacity reports what it needs and touches nothing; the call is deterministic and legal inside a graph capture; the animation
paths hand out exactly the twin's encoding of their own 8-bit frames; and the outputs that existed before are what they were."""
import io
import os

import numpy as np
import pytest
import torch

import video_case as vc
from sings_amd import video as V

pytestmark = pytest.mark.gpu

CASES = vc.cases()
_TWIN = {}


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _three(name):
    """Three different frames of case ``name``'s size: the case's own, mirrored, and shifted sideways with the channels rotated."""
    f = CASES[name][0]
    return np.stack([f, f[:, ::-1], np.roll(f, (3, 1), (1, 2))])


def _twin(name):
    """The twin's streams of ``_three(name)``, computed once."""
    if name not in _TWIN:
        _, q, ri = CASES[name]
        _TWIN[name] = V.jpeg_encode_host(_three(name), q, ri)
    return _TWIN[name]


def _decodes(data, W, H):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB" and im.size == (W, H)


# ---- bytes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_device_bytes_are_the_twins_bytes(name):
    frames = _three(name)
    _, q, ri = CASES[name]
    H, W = frames.shape[1:3]
    want = _twin(name)
    if name != "constant":
        assert len(set(want)) == 3, "three different frames"
    # (the default capacity, header + H W 3 / 2, is below what noise at quality 100 needs: ``encode_to_host`` grows it, ``encode`` is
    # given what the largest frame needs plus a few bytes that must stay untouched)
    enc = V.JpegEncoder(W, H, 3, _dev(), quality=q, restart_interval=ri, capacity=max(len(w) for w in want) + 5)
    assert enc.header == V.jpeg_header(W, H, q, ri) and want[0].startswith(enc.header)
    for bgr in (False, True):
        x = _t(frames[..., ::-1] if bgr else frames)
        buf, sizes = enc.encode(x, bgr=bgr)                          # K = 3
        n = sizes.cpu().tolist()
        assert n == [len(w) for w in want], (n, [len(w) for w in want])
        rows = buf.cpu().numpy()
        for k in range(3):
            assert rows[k, :n[k]].tobytes() == want[k], (name, bgr, k)
        buf, sizes = enc.encode(x[1:2], bgr=bgr)                     # K = 1, the second frame
        assert sizes.cpu().tolist() == [len(want[1])] and buf.cpu().numpy()[0, :len(want[1])].tobytes() == want[1], (name, bgr)
        assert enc.encode_to_host(x, bgr=bgr) == want
    one = V.JpegEncoder(W, H, 1, _dev(), quality=q, restart_interval=ri)
    assert one.encode_to_host(_t(frames[:1])) == want[:1]
    vc.check_stream(want[2], W, H, (W + 7) // 8 if ri is None else ri)


def test_a_frame_beyond_its_capacity_reports_what_it_needs_and_writes_nothing():
    name = "96x80_rows"
    frames = _three(name).copy()
    frames[1] = vc._noise(96, 80, 21)                                # the middle frame needs several times the others' bytes
    _, q, ri = CASES[name]
    want = V.jpeg_encode_host(frames, q, ri)
    need = [len(w) for w in want]
    assert need[1] > max(need[0], need[2]) + 64
    cap = max(need[0], need[2]) + 32
    GUARD = 4096
    enc = V.JpegEncoder(96, 80, 3, _dev(), quality=q, restart_interval=ri, capacity=cap)
    flat = torch.full((3 * cap + GUARD,), 0xA5, dtype=torch.uint8, device=_dev())
    sizes = torch.full((3,), 12345, dtype=torch.int32, device=_dev())
    buf, got = enc.encode(_t(frames), out=(flat[:3 * cap].view(3, cap), sizes))
    torch.cuda.synchronize()
    assert got.cpu().tolist() == [need[0], -need[1], need[2]]
    host = flat.cpu().numpy()
    assert (host[3 * cap:] == 0xA5).all(), "the guard bytes are unchanged"
    assert (host[cap:2 * cap] == 0xA5).all(), "the frame that does not fit wrote nothing"
    for k in (0, 2):
        assert host[k * cap:k * cap + need[k]].tobytes() == want[k]
        assert (host[k * cap + need[k]:(k + 1) * cap] == 0xA5).all(), "nothing behind a frame's last byte"
    # a capacity of exactly the need fits; one byte less does not
    exact = V.JpegEncoder(96, 80, 1, _dev(), quality=q, restart_interval=ri, capacity=need[0])
    assert exact.encode(_t(frames[:1]))[1].cpu().tolist() == [need[0]]
    short = V.JpegEncoder(96, 80, 1, _dev(), quality=q, restart_interval=ri, capacity=need[0] - 1)
    assert short.encode(_t(frames[:1]))[1].cpu().tolist() == [-need[0]]
    # encode_to_host grows the buffer and encodes again
    assert enc.capacity == cap
    assert enc.encode_to_host(_t(frames)) == want
    assert enc.capacity == need[1]


def test_encode_to_host_gives_up_after_two_retries(monkeypatch):
    frames = _t(_three("16x8"))
    enc = V.JpegEncoder(16, 8, 3, _dev(), capacity=64)
    monkeypatch.setattr(V.JpegEncoder, "_allocate", lambda self, capacity: None)          # a buffer that never grows
    with pytest.raises(RuntimeError, match="after two retries"):
        enc.encode_to_host(frames)


def test_two_encodes_of_the_same_input_give_identical_buffers():
    name = "noise_q100_ri48"
    frames = _t(_three(name))
    _, q, ri = CASES[name]
    enc = V.JpegEncoder(64, 48, 3, _dev(), quality=q, restart_interval=ri, capacity=20000)
    enc.buf.fill_(0)
    a, na = (x.clone() for x in enc.encode(frames))
    enc.buf.fill_(0)
    other = V.JpegEncoder(64, 48, 3, _dev(), quality=q, restart_interval=ri, capacity=20000)             # (another workspace, other stale bytes in it)
    other.buf.fill_(0)
    b, nb = other.encode(frames)
    assert int(na.min()) > 10000 and torch.equal(na, nb) and torch.equal(a, b)
    c, nc = enc.encode(frames)
    assert torch.equal(na, nc) and torch.equal(a, c)


def test_encode_inside_a_graph_capture_replays_on_new_frames():
    name = "96x80_ri5"
    frames = _three(name)
    _, q, ri = CASES[name]
    enc = V.JpegEncoder(96, 80, 3, _dev(), quality=q, restart_interval=ri)
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
    want = V.jpeg_encode_host(other, q, ri)
    n = sizes.cpu().tolist()
    assert n == [len(w) for w in want]
    rows = buf.cpu().numpy()
    assert [rows[k, :n[k]].tobytes() for k in range(3)] == want and want != _twin(name)


def test_refusals_of_the_encoder():
    enc = V.JpegEncoder(16, 8, 2, _dev())
    ok = _t(_three("16x8")[:2])
    for bad in (ok.cpu(), ok.float(), ok[:, :, :8], _t(_three("16x8")), ok[0]):
        with pytest.raises(ValueError, match="JpegEncoder.encode"):
            enc.encode(bad)
    with pytest.raises(ValueError, match="K = 17"):
        V.JpegEncoder(16, 8, 17, _dev())
    with pytest.raises(ValueError, match="rows of capacity bytes"):
        enc.encode(ok, out=(torch.empty((2, 2 * enc.capacity), dtype=torch.uint8, device=_dev())[:, ::2], enc.sizes))


# ---- the animation paths ---------------------------------------------------------------------------------------------------------
W_A, H_A, F_A = 128, 96, 5


def _one_avatar():
    from sings_amd.body import joint_transforms
    from sings_amd.camera import make_camera
    from sings_amd.scene import avatar_scene
    s = avatar_scene(N=3000, J=24, W=W_A, H=H_A, seed=7)
    cam = make_camera(np.eye(4, dtype=np.float32), 170.0, 170.0, W_A / 2, H_A / 2, W_A, H_A)
    data = dict(fovx=cam["fovx"], fovy=cam["fovy"], image_height=H_A, image_width=W_A, world_view_transform=_t(cam["world_view_transform"]),
                full_proj_transform=_t(cam["full_proj_transform"]), camera_center=_t(cam["camera_center"]))
    rs = np.random.RandomState(3)
    poses = _t(rs.normal(0, 0.2, (F_A, 72)).astype(np.float32))
    transl = _t((s["transl"][None] + rs.normal(0, 0.02, (F_A, 3))).astype(np.float32))
    jr = _t(s["joints_rest"])
    canon = dict(xyz_canon=_t(s["xyz_canon"]), rotmat_canon=None, scales=_t(s["scales"] * np.float32(3.0)), opacity=_t(s["opacities"]),
                 shs=_t(s["shs"]), lbs_weights=_t(s["lbs_weights"]), active_sh_degree=0)
    A_cano = joint_transforms(torch.zeros(72, device=_dev()), jr, tuple(s["parents"]))
    return canon, poses, jr, A_cano, data, dict(transl=transl, parents=tuple(s["parents"]))


def _held_to_the_twin(got, rgb8, quality=90):
    assert sorted(got) == sorted(rgb8) == list(range(F_A))
    frames = np.stack([rgb8[f].cpu().numpy() for f in range(F_A)])
    assert frames.shape == (F_A, H_A, W_A, 3) and frames.min() < 250, "the avatar is in view"
    want = V.jpeg_encode_host(frames, quality)
    for f in range(F_A):
        assert isinstance(got[f], bytes) and got[f] == want[f], f
        _decodes(got[f], W_A, H_A)
    return want


def test_animate_chunk_hands_out_the_twins_streams_and_a_video_of_them(tmp_path):
    from sings_amd.posed import animate_chunk, frames_to_u8
    canon, poses, jr, A_cano, data, kw = _one_avatar()
    bg = torch.ones(3, device=_dev())
    rgb8 = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=2, out="rgb8", **kw))
    got = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=2, out="jpeg", **kw))        # 2 + 2 + 1 (padded)
    want = _held_to_the_twin(got, rgb8)
    assert len(set(want)) == F_A, "five different frames"
    # the per-frame loop hands out the same streams; another quality other ones
    assert dict(animate_chunk(canon, poses, jr, A_cano, data, bg, out="jpeg", **kw)) == got
    q50 = dict(animate_chunk(canon, poses[:2], jr, A_cano, data, bg, frames_per_launch=2, out=("jpeg", 50), **kw))
    assert [q50[f] for f in range(2)] == V.jpeg_encode_host(np.stack([rgb8[f].cpu().numpy() for f in range(2)]), 50)
    # the video: the same five streams inside a RIFF AVI
    path = str(tmp_path / "anim.avi")
    assert V.animate_to_video(path, canon, poses, jr, A_cano, data, bg, fps=20, quality=90, frames_per_launch=2, **kw) == F_A
    r = vc.walk_riff(open(path, "rb").read())
    assert r["frames"] == want and len(r["idx1"]) == F_A
    # what existed before is what it was: bgr8 frames are frames_to_u8 of the float frames, rgb8 their channel swap
    f32 = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=2, **kw))
    bgr8 = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=2, out="bgr8", **kw))
    for f in range(F_A):
        assert bgr8[f].dtype == torch.uint8 and torch.equal(bgr8[f], frames_to_u8(f32[f], bgr=True))
        assert torch.equal(bgr8[f], rgb8[f].flip(-1))
        assert np.array_equal(bgr8[f].cpu().numpy(), (np.clip(f32[f].cpu().numpy(), 0, 1) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)[..., ::-1])


@pytest.mark.parametrize("out", ["bgr8", "jpeg", ("jpeg", 50), "png"], ids=str)
def test_the_pipelined_per_frame_path_hands_out_what_the_batched_path_does(out):
    """``streams=2, frames_per_launch=1``: ``FrameAnimator.render_frames``, the output applied frame by frame behind the hand-out."""
    from sings_amd.posed import animate_chunk
    canon, poses, jr, A_cano, data, kw = _one_avatar()
    bg = torch.ones(3, device=_dev())
    want = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, frames_per_launch=2, out=out, **kw))
    got = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, streams=2, frames_per_launch=1, out=out, **kw))
    assert sorted(got) == sorted(want) == list(range(F_A))
    for f in range(F_A):
        if out == "bgr8":
            assert got[f].dtype == torch.uint8 and tuple(got[f].shape) == (H_A, W_A, 3) and torch.equal(got[f], want[f]), f
        else:
            assert isinstance(got[f], bytes) and got[f] == want[f], f
    assert len({got[f] if isinstance(got[f], bytes) else got[f].cpu().numpy().tobytes() for f in range(F_A)}) == F_A, "five different frames"


def test_animate_scene_hands_out_the_twins_streams(tmp_path):
    from test_gpu_scene import _avatar, _cameras
    from sings_amd.body import joint_transforms
    from sings_amd.scene import avatar_scene
    from sings_amd.scene_anim import animate_scene, animate_scene_to_video
    avatars = [_avatar(600, 52, 6, 41, F_A, ext=None), _avatar(200, 24, None, 42, F_A, smpl_scale=None, ext="frames", offset=(0.05, 0.0, 0.1))]
    cams = _cameras(W_A, H_A, F_A, focal=200.0)
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    rs = np.random.RandomState(9)
    poses, rest, cano, parents = [], [], [], []
    for a, seed in zip(avatars, (41, 42)):
        s = avatar_scene(N=8, J=a["J"], W=W_A, H=H_A, seed=seed)
        jr = _t(s["joints_rest"])
        poses.append(_t(rs.normal(0, 0.2, (F_A, a["J"] * 3)).astype(np.float32)))
        rest.append(jr); parents.append(tuple(s["parents"]))
        cano.append(joint_transforms(_t(rs.normal(0, 0.05, a["J"] * 3).astype(np.float32)), jr, parents[-1]))
    kw = dict(transl=[a["transl"] for a in avatars], smpl_scale=[a["smpl_scale"] for a in avatars], ext_tfs=[a["ext_tfs"] for a in avatars],
              parents=parents, frames_per_launch=2)
    canons = [a["canon"] for a in avatars]
    rgb8 = dict(animate_scene(canons, poses, rest, cano, cams, bg, out="rgb8", **kw))
    got = dict(animate_scene(canons, poses, rest, cano, cams, bg, out="jpeg", **kw))
    want = _held_to_the_twin(got, rgb8)
    path = str(tmp_path / "scene.avi")
    assert animate_scene_to_video(path, canons, poses, rest, cano, cams, bg, fps=10, **kw) == F_A
    assert vc.walk_riff(open(path, "rb").read())["frames"] == want


# ---- the run's outputs -----------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, attrs, lbs_weights):
        self.attrs, self.lbs_weights = attrs, lbs_weights

    def decode(self):
        return self.attrs


class _Trainer:
    """What ``RunOutputs.after_step`` reads of a trainer on an iteration that is due for a progress sheet only."""
    sh_degree, last_render = 0, None

    def __init__(self, model):
        self.m = model


def test_progress_video_holds_the_sheets_and_changes_nothing_without_the_flag(tmp_path):
    from sings_amd import canonical as cn
    from sings_amd.body import joint_transforms
    from sings_amd.run_outputs import RunOutputs
    from sings_amd.scene import avatar_scene
    s = avatar_scene(N=2000, J=24, W=64, H=64, seed=11)
    jr = _t(s["joints_rest"])
    A_cano = joint_transforms(torch.zeros(72, device=_dev()), jr, tuple(s["parents"]))
    A = cn.static_A("da_pose", jr, torch.inverse(A_cano), tuple(s["parents"]))
    attrs = {"xyz_canon": _t(s["xyz_canon"]), "rot6d_canon": None, "scales": _t(s["scales"] * np.float32(3.0)), "opacity": _t(s["opacities"]),
             "shs": _t(s["shs"])}
    tr = _Trainer(_Model(attrs, _t(s["lbs_weights"])))
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    written = {}
    for flag in (False, True):
        logdir = str(tmp_path / f"run{int(flag)}")
        got = written[flag] = {}
        ro = RunOutputs(logdir, A, bg, viz_interval=1000, progress_interval=2, save_ply=False,
                        write=lambda path, array, got=got, logdir=logdir: got.__setitem__(os.path.relpath(path, logdir), array.copy()))
        assert ro.progress_video is False
        ro.progress_size, ro.progress_video = (32, 40), flag
        for t in (1, 2, 3, 4, 6):
            ro.after_step(tr, t)
        assert not os.path.exists(ro.video_path), "the video appears under its name at finish()"
        ro.finish()
        assert os.path.exists(ro.video_path) == flag
        if not flag:
            assert not os.path.exists(logdir) or os.listdir(logdir) == ["train_progress"] or os.listdir(logdir) == []
    assert sorted(written[False]) == sorted(written[True]) == [f"train_progress/{t:06d}.png" for t in (2, 4, 6)]
    for k in written[False]:
        assert np.array_equal(written[False][k], written[True][k]), k
    sheets = [written[True][f"train_progress/{t:06d}.png"] for t in (2, 4, 6)]
    Hs, Ws = sheets[0].shape[:2]
    assert (Hs, Ws) == (32 + 4, 4 * 42 + 2)
    r = vc.walk_riff(open(str(tmp_path / "run1" / "train_progress.avi"), "rb").read())
    assert r["frames"] == V.jpeg_encode_host(np.stack(sheets), 90)
    import struct
    assert struct.unpack("<14I", r["avih"])[0] == 100000 and struct.unpack("<14I", r["avih"])[8:10] == (Ws, Hs)
    for f in r["frames"]:
        _decodes(f, Ws, Hs)
