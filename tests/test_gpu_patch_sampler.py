"""The device patch sampler on the GPU (include/sings_sampler.h, csrc/sg_sampler.hip, sings_amd/patch_sampler.py) against its numpy
twin ``origins_host``: INTEGER EQUALITY of the corners and of (M, branch), no tolerance.  The shapes are the smallest that reach each
path of the two kernels: one chunk of SG_PATCH_CHUNK = 4096 crop positions, a ragged one, two chunks with the valid pixels at and
across the boundary, more chunks than the scan has threads, the largest n, several frames with their own masks and with one.  Then the
counter (it lives on the device and moves with every call), a HIP-graph capture of the draw -- a host read inside would fail the
capture: the structural proof that the round trip is gone -- and ``AvatarTrainer(lpips_sampler=...)`` eager and captured."""
import math

import numpy as np
import pytest
import torch

import lpips_case as lc
import test_gpu_train_loop as tl
from sings_amd import _lib
from sings_amd import patch_sampler as ps
from test_patch_sampler_host import census_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_calls(masks, P, n, ratio, seed, calls=3, shared=False):
    """``calls`` consecutive draws from ``masks`` ([H,W], or [K,H,W]; ``shared``: one [H,W] mask for 3 frames) equal the twin's at
    the sampler's counters.  -> (the sampler, the branches seen)."""
    masks = np.asarray(masks, np.float32)
    s = ps.DevicePatchSampler(num_patch=n, patch_size=P, ratio_mask=ratio, seed=seed, device=DEV)
    m = _dev(masks)
    K = 3 if shared else (1 if masks.ndim == 2 else masks.shape[0])
    seen = set()
    for c in range(calls):
        got = s.origins(m, frames=3) if shared else s.origins(m)
        org, info = got.cpu().numpy().reshape(K, n, 2), s.info.cpu().numpy()
        assert got.dtype == torch.int32 and info.shape == (K, 2)
        for k in range(K):
            mk = masks if masks.ndim == 2 else masks[k]
            ref, branch, M = ps.origins_host(mk, P, n, ratio, seed, c, frame=k)
            assert (int(info[k, 0]), int(info[k, 1])) == (M, branch), (c, k, info[k], M, branch)
            assert np.array_equal(org[k], ref), (c, k, org[k], ref)
            seen.add(branch)
    assert s.counter == calls
    return s, seen


def _positions(H, W, P, qs):
    """A mask [H,W] valid exactly at the crop positions ``qs``."""
    m = np.zeros((H, W), np.float32)
    o, Wc = P // 2, W - P
    for q in qs:
        m[o + q // Wc, o + q % Wc] = 1.0
    return m


# ---- the paths of the kernels ----------------------------------------------------------------------------------------------------
def test_one_chunk_census_full_and_nan_masks():
    assert (48 - 16) * (64 - 16) == 1536 < _lib.PATCH_CHUNK
    odd = census_mask()
    odd[10, 10], odd[11, 11], odd[30, 20], odd[3, 30], odd[20, 60] = np.nan, -1.0, -np.inf, 1.0, 1.0
    for mask in (census_mask(), np.ones((48, 64), np.float32), odd):
        _, seen = _check_calls(mask, 16, 4, 0.9, 1234, calls=8)
        assert seen == {ps.BRANCH_MASKED, ps.BRANCH_UNIFORM}          # (the draw of counter 6 is uniform)
    assert ps.origins_host(odd, 16, 4, 0.9, 0, 0)[2] == 8


def test_a_ragged_chunk_whose_rows_are_no_multiple_of_the_wave():
    rng = np.random.default_rng(3)
    mask = (rng.random((70, 53)) < 0.3).astype(np.float32)
    assert (70 - 16) * (53 - 16) == 1998 and (53 - 16) % 64
    _check_calls(mask, 16, 4, 1.0, 5, calls=16)
    last = _positions(70, 53, 16, [0, 1997, 1996, 36, 37])          # the first and the last cell of the crop, a row's ends
    _check_calls(last, 16, 4, 1.0, 5, calls=8)


@pytest.mark.parametrize("case", ["last_chunk", "straddle", "margin_only"])
def test_two_chunks(case):
    H, W, P, n = 96, 112, 16, 4
    total = (H - P) * (W - P)
    assert total == 7680 and _lib.PATCH_CHUNK < total < 2 * _lib.PATCH_CHUNK
    if case == "last_chunk":                                          # exactly n valid, all in the ragged last chunk
        mask = _positions(H, W, P, [4096, 5000, 7000, total - 1])
        s, seen = _check_calls(mask, P, n, 1.0, 8, calls=6)
        assert seen == {ps.BRANCH_MASKED}                             # M = n: every valid position, each once
        assert sorted(map(tuple, s.last_origins.cpu().tolist())) == sorted(divmod(q, W - P) for q in (4096, 5000, 7000, total - 1))
    elif case == "straddle":
        mask = _positions(H, W, P, [4095, 4096, 4097, 17])
        _, seen = _check_calls(mask, P, n, 1.0, 8, calls=6)
        assert seen == {ps.BRANCH_MASKED}
        _check_calls(_positions(H, W, P, [4094, 4095, 4096, 4097, 17, 7679, 0]), P, n, 1.0, 9, calls=12)
    else:                                                             # valid pixels in the margin outside the crop only
        mask = np.zeros((H, W), np.float32)
        mask[:P // 2], mask[-(P // 2):], mask[:, :P // 2], mask[:, -(P // 2):] = 1.0, 1.0, 1.0, 1.0
        s, seen = _check_calls(mask, P, n, 1.0, 8, calls=3)
        assert seen == {ps.BRANCH_FORCED} and int(s.info[0, 0]) == 0 and s.forced_uniform == 3


def test_more_chunks_than_a_wave_has_lanes():
    H, W, P = 500, 890, 128
    assert -(-(H - P) * (W - P) // _lib.PATCH_CHUNK) == 70            # the search for a rank's chunk walks the prefix sums twice
    rng = np.random.default_rng(11)
    mask = (rng.random((H, W)) < 0.3).astype(np.float32)
    _check_calls(mask, P, 4, 0.9, 21, calls=8)


def test_more_chunks_than_the_scan_has_threads():
    """The scan of the chunk counts takes 256 at a time: 952 x 1122 crop positions are 261 chunks, the smallest 1080-row frame
    that makes it loop."""
    H, W, P = 1080, 1250, 128
    assert -(-(H - P) * (W - P) // _lib.PATCH_CHUNK) == 261
    rng = np.random.default_rng(12)
    mask = (rng.random((H, W)) < 0.3).astype(np.float32)
    mask[H - P // 2 - 1, W - P // 2 - 1] = 1.0                        # the last cell of the crop
    _check_calls(mask, P, 4, 1.0, 22, calls=4)
    tail = np.zeros((H, W), np.float32)                               # everything in the last two chunks: ranks behind 256 empty chunks
    tail[H - P // 2 - 4:H - P // 2, P // 2:W - P // 2] = 1.0
    _check_calls(tail, P, 4, 1.0, 23, calls=4)


def test_the_largest_n():
    assert _lib.PATCH_MAX_N == 16
    _, seen = _check_calls(np.ones((96, 112), np.float32), 16, 16, 0.9, 4, calls=12)
    assert ps.BRANCH_MASKED in seen
    _check_calls(np.ones((96, 112), np.float32), 16, 16, 0.0, 4, calls=2)       # (33 words of the stream: nine Philox blocks)


def test_several_frames_with_their_own_masks_and_with_one():
    H, W, P, n = 96, 112, 16, 4
    masks = np.stack([np.ones((H, W), np.float32), np.zeros((H, W), np.float32), _positions(H, W, P, [3, 4096, 5000, 7679])])
    s, _ = _check_calls(masks, P, n, 1.0, 6, calls=3)
    assert s.info[:, 1].tolist() == [ps.BRANCH_MASKED, ps.BRANCH_FORCED, ps.BRANCH_MASKED] and s.forced_uniform == 3
    assert tuple(s.last_origins.shape) == (3, n, 2)
    s, _ = _check_calls(masks[0], P, n, 0.9, 6, calls=3, shared=True)
    o = s.last_origins.cpu().numpy()
    assert not np.array_equal(o[0], o[1]) and not np.array_equal(o[1], o[2]) and s.forced_uniform == 0


def test_mask_shapes_dtypes_and_the_owned_buffers():
    mask = census_mask()
    s = ps.DevicePatchSampler(num_patch=4, patch_size=16, ratio_mask=1.0, seed=2, device=DEV)
    a = s.origins(_dev(mask))
    assert tuple(a.shape) == (4, 2) and np.array_equal(a.cpu().numpy(), ps.origins_host(mask, 16, 4, 1.0, 2, 0)[0])
    b = s.origins(_dev(mask)[None])                                   # [1,H,W] -> [n,2], the same buffer
    assert tuple(b.shape) == (4, 2) and b.data_ptr() == a.data_ptr()
    assert np.array_equal(b.cpu().numpy(), ps.origins_host(mask, 16, 4, 1.0, 2, 1)[0])
    for c, other in enumerate((_dev(mask).bool(), _dev(mask).double(), _dev(mask).half(), _dev(mask.T.copy()).t()), start=2):
        assert not (other.dtype == torch.float32 and other.is_contiguous())
        got = s.origins(other)                                        # converted on the device
        assert np.array_equal(got.cpu().numpy(), ps.origins_host(mask, 16, 4, 1.0, 2, c)[0]), c
    with pytest.raises(RuntimeError, match="no host round trip"):
        s.origins(torch.from_numpy(mask))
    with pytest.raises(RuntimeError, match="no room for a patch"):
        s.origins(torch.ones(16, 64, device=DEV))
    assert s.counter == 6                                             # (a refused call draws nothing)


# ---- the counter -----------------------------------------------------------------------------------------------------------------
def test_the_counter_lives_on_the_device_and_resumes():
    rng = np.random.default_rng(2)
    mask = (rng.random((70, 53)) < 0.3).astype(np.float32)
    m, P, n = _dev(mask), 16, 4
    a = ps.DevicePatchSampler(n, P, 0.9, seed=(1 << 63) + 12345, device=DEV)      # (a seed with the top bit: both key words in use)
    b = ps.DevicePatchSampler(n, P, 0.9, seed=(1 << 63) + 12345, device=DEV)
    c = ps.DevicePatchSampler(n, P, 0.9, seed=12345, device=DEV)
    a.load_state_dict({"seed": a.seed, "counter": (1 << 32) - 3})                 # the run crosses into the counter's high word
    b.load_state_dict(a.state_dict())
    assert a.seed == (1 << 63) + 12345 and b.counter == (1 << 32) - 3
    seq, differ = [], 0
    for i in range(64):
        oa, ob, oc = a.origins(m).clone(), b.origins(m).clone(), c.origins(m).clone()
        ref, branch, M = ps.origins_host(mask, P, n, 0.9, (1 << 63) + 12345, (1 << 32) - 3 + i)
        assert np.array_equal(oa.cpu().numpy(), ref) and torch.equal(oa, ob), i
        assert a.info.cpu().tolist() == [[M, branch]]
        differ += int(not torch.equal(oa, oc))
        seq.append(oa)
    assert differ >= 60 and a.counter == (1 << 32) + 61               # (another seed: four of ~600 pixels coincide by chance never)
    d = ps.DevicePatchSampler(n, P, 0.9, seed=1, device=DEV)
    d.load_state_dict({"seed": (1 << 63) + 12345, "counter": (1 << 32) - 3 + 40})
    for i in range(40, 44):                                           # a resumed run continues the sequence
        assert torch.equal(d.origins(m), seq[i]), i
    # two runs of the same call: the same bits, info and workspace included
    e = ps.DevicePatchSampler(n, P, 0.9, seed=1, device=DEV)
    runs = []
    for _ in range(2):
        e.load_state_dict({"seed": 1, "counter": 7})
        o = e.origins(m)
        runs.append((o.clone(), e.info.clone(), next(iter(e._bufs.values()))["ws"].clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ---- capture ---------------------------------------------------------------------------------------------------------------------
def test_the_draw_captures_and_every_replay_draws_the_next_patches():
    mask, full = census_mask(), np.ones((48, 64), np.float32)
    m = _dev(mask)
    s = ps.DevicePatchSampler(4, 16, 0.9, seed=99, device=DEV)
    s.origins(m)                                                      # (the buffers of this shape: allocated outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = s.origins(m)                                            # a host read here would fail the capture
    assert s.counter == 1                                             # (a capture runs nothing)
    for c, src in ((1, mask), (2, mask), (3, full), (4, mask)):
        m.copy_(_dev(src))                                            # another mask in the captured input: another draw
        g.replay()
        torch.cuda.synchronize()
        ref, branch, M = ps.origins_host(src, 16, 4, 0.9, 99, c)
        assert np.array_equal(out.cpu().numpy(), ref) and s.info.cpu().tolist() == [[M, branch]], c
    assert s.counter == 5


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
PATCH, NPATCH, SEED, STEPS = 16, 4, 31, 4


def _lpips_trainer(sc, use_graph, sampler):
    from sings_amd.lpips import LPIPS
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    wt = lc.make_weights(0)
    tri, geo, app = tl._modules(DEV)
    kw = {} if sampler is False else dict(lpips=LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"], device=DEV),
                                          lpips_w=1.0, lpips_patch_size=PATCH)
    mod = AvatarStep(_dev(sc["xyz"]), _dev(sc["w"]), tri, geo, app, **kw).to(DEV)
    cam = sc["cam"]
    consts = dict(bg=_dev(sc["bg"]), view=_dev(cam["world_view_transform"]), proj=_dev(cam["full_proj_transform"]),
                  campos=_dev(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=tl.H, image_width=tl.W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5),
            bg=consts["bg"], scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg,
            campos=consts["campos"], prefiltered=False, debug=False)
    extra = {"lpips_sampler": sampler} if sampler not in (None, False) else {}
    return AvatarTrainer(mod, settings, consts["bg"], tl.LRS, smpl_scale=_dev(sc["smpl_scale"]), transl=_dev(sc["transl"]),
                         use_graph=use_graph, sh_degree=0, max_sh_degree=1, **extra)


@pytest.fixture(scope="module")
def scene():
    return tl._scene()


@pytest.mark.parametrize("use_graph", [False, True])
def test_the_trainer_draws_the_twins_patches_eager_and_captured(scene, use_graph):
    from sings_amd.train_loop import AvatarTrainer
    sc = scene
    mask = _dev(sc["mask"])
    bgs = [torch.rand(3, tl.H, tl.W, device=DEV, generator=torch.Generator(DEV).manual_seed(i)) for i in range(STEPS)]
    step = lambda t, i, **kw: t.step(_dev(sc["frames"][i % 8]), _dev(sc["gts"][i % 8]), mask, lpips_bg=bgs[i], **kw)
    sampler = ps.DevicePatchSampler(NPATCH, PATCH, 0.9, seed=SEED, device=DEV)
    sampler.load_state_dict({"seed": SEED, "counter": 5})             # (a run that does not start at zero)
    s0, captures = sampler.counter, []
    A = _lpips_trainer(sc, use_graph, sampler)
    A._capture = lambda: (captures.append(A.iteration), AvatarTrainer._capture(A))
    refs = [ps.origins_host(sc["mask"], PATCH, NPATCH, 0.9, SEED, s0 + i)[0] for i in range(STEPS)]
    first = None
    for i in range(STEPS):
        la = step(A, i)
        torch.cuda.synchronize()
        assert np.array_equal(sampler.last_origins.cpu().numpy().reshape(NPATCH, 2), refs[i]), i
        assert "lpips_patch" in la
        first = la if i == 0 else first
    assert sampler.counter == s0 + STEPS == 9                         # the capture's warm-up runs are not steps
    assert captures == ([2] if use_graph else [])                     # two sizing steps, ONE capture, one replay of it
    with pytest.raises(ValueError, match="lpips_origins= cannot be passed too"):
        step(A, 0, lpips_origins=refs[0])
    # trainer B: the same parameters, fed the twin's corners of the same iteration
    B = _lpips_trainer(sc, use_graph, None)
    lb = step(B, 0, lpips_origins=refs[0])
    assert set(first) == set(lb)
    assert all(torch.equal(first[k], lb[k]) for k in lb), {k: (first[k].item(), lb[k].item()) for k in lb}


def test_the_trainer_refuses_a_sampler_without_the_term_and_is_unchanged_without_a_sampler(scene):
    from sings_amd.train_loop import AvatarTrainer
    sc = scene
    plain = _lpips_trainer(sc, False, False)                          # a module without lpips=
    with pytest.raises(ValueError, match="needs the module's LPIPS term"):
        AvatarTrainer(plain.m, plain.settings_fn, plain.bg, tl.LRS, lpips_sampler=ps.DevicePatchSampler(NPATCH, PATCH, device=DEV))
    with pytest.raises(ValueError, match="crops patches of 16"):
        _lpips_trainer(sc, False, ps.DevicePatchSampler(NPATCH, 32, device=DEV))
    # lpips_sampler=None: the trainer of today, key for key and bit for bit in the first step
    mask = _dev(sc["mask"])
    ref, _, _ = ps.origins_host(sc["mask"], PATCH, NPATCH, 0.9, 1, 0)
    bg = torch.rand(3, tl.H, tl.W, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    runs = []
    for explicit_none in (False, True):
        t = _lpips_trainer(sc, False, None)
        if explicit_none:
            t = AvatarTrainer(t.m, t.settings_fn, t.bg, tl.LRS, smpl_scale=t.smpl_scale, transl=t.transl, sh_degree=0, max_sh_degree=1,
                              lpips_sampler=None)
        assert t.lpips_sampler is None
        runs.append(t.step(_dev(sc["frames"][0]), _dev(sc["gts"][0]), mask, lpips_origins=ref, lpips_bg=bg))
    assert set(runs[0]) == set(runs[1]) and "lpips_patch" in runs[0]
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    without = plain.step(_dev(sc["frames"][0]), _dev(sc["gts"][0]), mask)
    assert "lpips_patch" not in without and set(without) | {"lpips_patch"} == set(runs[0])
