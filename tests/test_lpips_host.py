"""CPU tests of the LPIPS-VGG patch loss: weight packing, the patch sampler and the fp64 oracle against vectors produced by the
reference's own loss.py / sampler.py (tests/golden/gen_lpips_golden.py), and the new entry points' argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_case as lc
from sings_amd import _lib
from sings_amd import lpips as L

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "lpips_golden.npz"))
SEEDS = (3, 11, 21)


def test_from_module_and_from_tensors_pack_identically():
    wt = lc.make_weights(1)
    a = L.LPIPS.from_module(lc.StandInLPIPS(wt)).packed
    b = L.LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"]).packed
    assert a.dtype == torch.float32 and torch.equal(a, b)
    offs, total = L.weights_layout()
    assert a.numel() == total and len(offs) == _lib.LPIPS_NUM_OFFSETS and all(o % 4 == 0 for o in offs)
    assert list(offs) == sorted(offs)
    w0, b0 = wt["convs"][0]
    assert torch.equal(a[offs[0]:offs[0] + w0.numel()], w0.reshape(-1)) and torch.equal(a[offs[1]:offs[1] + 64], b0)
    assert torch.equal(a[offs[44]:offs[44] + 3], wt["shift"].reshape(-1)) and torch.equal(a[offs[45]:offs[45] + 3], wt["scale"].reshape(-1))
    for k in range(5):
        c = L.LIN_CHANNELS[k]
        assert torch.equal(a[offs[39 + k]:offs[39 + k] + c], wt["lins"][k].reshape(-1))


def test_packed_weights_forward_and_backward_layouts():
    wt = lc.make_weights(2)
    p = L.pack_weights(wt["convs"], wt["lins"], wt["shift"], wt["scale"])
    offs, _ = L.weights_layout()
    for l in range(1, 13):
        w, b = wt["convs"][l]
        co, ci = w.shape[:2]
        assert torch.equal(L.unpack_backward_weights(p, l), w.transpose(0, 1).flip(2, 3))
        fwd = p[offs[3 * l]:offs[3 * l] + w.numel()].reshape(co, 3, 3, ci).permute(0, 3, 1, 2)
        assert torch.equal(fwd, w)
        assert torch.equal(p[offs[3 * l + 1]:offs[3 * l + 1] + co], b)


def test_pack_refuses_wrong_shapes():
    wt = lc.make_weights(2)
    convs = list(wt["convs"]); convs[3] = (convs[3][0][:, :64], convs[3][1])
    with pytest.raises(ValueError):
        L.pack_weights(convs, wt["lins"], wt["shift"], wt["scale"])
    with pytest.raises(ValueError):
        L.pack_weights(wt["convs"][:12], wt["lins"], wt["shift"], wt["scale"])


@pytest.mark.parametrize("seed", SEEDS)
def test_patch_sampler_reproduces_reference_origins(seed):
    _, _, mask, _ = lc.golden_inputs(seed)
    np.random.seed(seed)
    o = L.PatchSampler(num_patch=int(G["num_patches"]), patch_size=int(G["patch_size"]), ratio_mask=0.9).origins(torch.from_numpy(mask)[None])
    np.testing.assert_array_equal(o, G[f"s{seed}_origins"])


def test_patch_sampler_random_branch_matches_numpy_calls():
    mask = np.ones((64, 48), np.float32)
    np.random.seed(0)
    s = L.PatchSampler(num_patch=3, patch_size=16, ratio_mask=0.0)              # always the randint branch
    o = s.origins(mask)
    np.random.seed(0)
    np.random.rand()
    x = np.random.randint(0, 64 - 16, size=3); y = np.random.randint(0, 48 - 16, size=3)
    np.testing.assert_array_equal(o, np.stack([x, y], 1))


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_reproduces_reference_loss_and_gradient(seed):
    wt = lc.make_weights(int(G["weights_seed"]))
    raw, gt, mask, bg = lc.golden_inputs(seed)
    t_raw = torch.from_numpy(raw).requires_grad_(True)
    loss = lc.patch_loss_ref(wt, t_raw, torch.from_numpy(gt), torch.from_numpy(mask), torch.from_numpy(bg),
                             torch.from_numpy(G[f"s{seed}_bg_rand"]), torch.from_numpy(G[f"s{seed}_origins"]), int(G["patch_size"]),
                             float(G["lpips_w"]))
    loss.backward()
    ref = float(G[f"s{seed}_lpips_patch"])
    assert abs(loss.item() - ref) <= 1e-12 * abs(ref)
    np.testing.assert_allclose(t_raw.grad.numpy(), G[f"s{seed}_grad"], rtol=1e-6, atol=1e-12)
    assert (G[f"s{seed}_grad"] != 0).any()


def test_oracle_module_attribute_structure():
    m = lc.StandInLPIPS(lc.make_weights(0))
    x = torch.rand(1, 3, 16, 16, dtype=torch.float64)
    y = torch.rand(1, 3, 16, 16, dtype=torch.float64)
    v = m(x, y)
    assert v.shape == (1, 1, 1, 1) and v.item() > 0 and m(x, x).item() == 0


def test_lpips_symbols_exported_and_refuse_bad_sizes():
    lib = _lib.load()
    for name in ("sg_lpips_weights_layout", "sg_lpips_ws_bytes", "sg_lpips_forward", "sg_lpips_backward", "sg_lpips_patch_gather",
                 "sg_lpips_patch_scatter"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    n = C.c_size_t(0)
    assert lib.sg_lpips_ws_bytes(2, 128, 128, C.byref(n)) == 0 and n.value > 2 * 2 * 128 * 128 * 64 * 4
    small = n.value
    assert lib.sg_lpips_ws_bytes(2, 37, 53, C.byref(n)) == 0 and 0 < n.value < small
    for B, H, W in ((0, 128, 128), (1, 15, 128), (1, 128, 15), (-1, 64, 64)):
        n.value = 7
        assert lib.sg_lpips_ws_bytes(B, H, W, C.byref(n)) != 0 and n.value == 7
        assert b"sg_lpips_ws_bytes" in lib.sg_last_error()
    fake = C.c_void_p(0x1000)                                                   # never dereferenced
    assert lib.sg_lpips_forward(0, 64, 64, 0, fake, fake, fake, fake, fake, None) != 0
    assert lib.sg_lpips_forward(1, 15, 64, 0, fake, fake, fake, fake, fake, None) != 0
    assert lib.sg_lpips_backward(1, 64, 8, 0, fake, fake, fake, fake, None) != 0
    assert lib.sg_lpips_forward(1, 64, 64, 0, None, fake, fake, fake, fake, None) != 0
    assert lib.sg_lpips_patch_gather(1, 4, 65, 64, 64, *([fake] * 8), None) != 0                # patch larger than the image
    assert lib.sg_lpips_patch_scatter(1, 0, 16, 64, 64, *([fake] * 6), None) != 0                # no patches


def test_python_surface_refuses_without_gpu_or_bad_use():
    m = L.LPIPS.from_tensors(**{k: v for k, v in lc.make_weights(0).items()})
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(NotImplementedError):
        m(x, x, retPerLayer=True)
    with pytest.raises(NotImplementedError):
        m(x, x, spatial=True)
    with pytest.raises(ValueError):
        m(x, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x)


# ---- the pinned fp64 reference (lpips_case.read_state / check_layers / pinned_backward) and the workspace layout ---------------
def _inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)


@pytest.mark.parametrize("normalize", (False, True))
def test_pinned_reference_is_the_oracle_on_its_own_state(normalize):
    """On the fp64 oracle's own masks, pool choices and features, check_layers passes at round-off and pinned_backward is autograd."""
    wt = lc.make_weights(7)
    x0, x1 = _inputs(2, 37, 53, 7)
    st = lc.oracle_state(wt, x0, x1, normalize)
    res = lc.check_layers(wt, x0, x1, normalize, st)
    assert max(res["conv"]) <= 1e-9 and max(res["head"]) <= 1e-9 and res["out"] <= 1e-9 and res["pool"] == [0] * 4, res
    up = torch.tensor([0.7, 1.3], dtype=torch.float64)
    r0 = x0.double().requires_grad_(True)
    lc.lpips_ref(wt, r0, x1.double(), normalize).backward(up.reshape(-1, 1, 1, 1))
    got = lc.pinned_backward(wt, st, up, normalize)
    assert got.shape == r0.shape and (r0.grad != 0).any()
    assert ((got - r0.grad).abs() <= 1e-10 * r0.grad.abs().max()).all()


def test_pinned_bounds_hold_for_torch_fp32_at_the_training_shape():
    """Calibration: torch's own fp32 CPU forward meets check_layers' bounds, and its fp32 autograd gradient meets the strict
    per-element bound against the fp64 backward pinned to its masks -- at 128^2, where it fails the unpinned comparison."""
    wt = lc.make_weights(0)
    g = torch.Generator().manual_seed(0)
    x0 = torch.rand(1, 3, 128, 128, generator=g); x1 = (x0 + 0.1 * torch.randn(1, 3, 128, 128, generator=g)).clamp(0, 1)
    st = lc.oracle_state(wt, x0, x1, dtype=torch.float32)
    res = lc.check_layers(wt, x0, x1, False, st)
    up = torch.tensor([0.8])
    a = x0.clone().requires_grad_(True)
    lc.lpips_ref(wt, a, x1, dtype=torch.float32).backward(up.reshape(-1, 1, 1, 1))
    ref = lc.pinned_backward(wt, st, up)
    err = (a.grad.double() - ref).abs()
    bound = 2e-4 * ref.abs() + 2e-5 * ref.abs().max()
    print(f"torch fp32 at 128^2: worst conv ratio {max(res['conv']):.3g}, head {max(res['head']):.3g}, out {res['out']:.3g}; "
          f"grad worst ratio {(err / bound).max().item():.3g}")
    assert (err <= bound).all(), (err / bound).max().item()


def test_pinned_checks_reject_a_wrong_layer_pool_or_mask():
    wt = lc.make_weights(7)
    x0, x1 = _inputs(2, 37, 53, 8)
    up = torch.tensor([0.7, 1.3], dtype=torch.float64)
    st = lc.oracle_state(wt, x0, x1)
    base = lc.pinned_backward(wt, st, up)
    # one conv 5 output off by 1e-3 of its magnitude sum
    y = st["y"][5]
    c, i, j = (int(v) for v in (y[1] > 0).nonzero()[100])
    w, b = (t.double() for t in wt["convs"][5])
    mag = b.abs()[c] + F.conv2d(st["y"][4][1:2].abs(), w.abs(), padding=1)[0, c, i, j]
    bad = dict(st, y=list(st["y"]))
    bad["y"][5] = y.clone(); bad["y"][5][1, c, i, j] += 1e-3 * mag
    with pytest.raises(AssertionError, match=f"^conv 5: worst at image 1, channel {c}, row {i}, column {j}"):
        lc.check_layers(wt, x0, x1, False, bad)
    # one pool choice (of a window whose maximum is positive, so its ReLU passes the gradient) moved to another window element
    a = st["arg"][1]
    c, i, j = (int(v) for v in (st["pool"][1][0] > 0).nonzero()[40])
    bad = dict(st, arg=list(st["arg"]))
    bad["arg"][1] = a.clone(); bad["arg"][1][0, c, i, j] = (a[0, c, i, j] + 1) % 4
    with pytest.raises(AssertionError, match=f"^pool 1: 1 elements wrong, first at image 0, channel {c}, pixel \\({i}, {j}\\)"):
        lc.check_layers(wt, x0, x1, False, bad)
    assert not torch.equal(lc.pinned_backward(wt, bad, up), base)
    # one ReLU mask bit flipped (conv 4 is neither a slice output nor a pool input: only its mask reads it)
    on = (st["y"][4][0] > 0).nonzero()[50]
    bad = dict(st, y=list(st["y"]))
    bad["y"][4] = st["y"][4].clone(); bad["y"][4][0, on[0], on[1], on[2]] = 0
    assert not torch.equal(lc.pinned_backward(wt, bad, up), base)


LAYOUT_SIZES = ((1, 16, 16), (2, 37, 53), (16, 128, 128), (1, 512, 896))


@pytest.mark.parametrize("B,H,W", LAYOUT_SIZES)
def test_ws_layout_pieces_tile_the_workspace(B, H, W):
    lay = L.ws_layout(B, H, W)
    assert lay["total"] == L._ws_bytes(B, H, W)
    hs, ws = lc.level_sizes(H, W)
    NI = 2 * B
    pieces = ([(f"y{l}", lay["y"][l], NI * hs[v] * ws[v] * L.CONV_CHANNELS[l][1] * 4) for l, v in enumerate(lc.LEVEL)] +
              [(f"pool{q}", lay["pool"][q], NI * hs[q + 1] * ws[q + 1] * lc.POOL_CH[q] * 4) for q in range(4)] +
              [(f"arg{q}", lay["arg"][q], NI * hs[q + 1] * ws[q + 1] * lc.POOL_CH[q]) for q in range(4)] +
              [(f"dpix{k}", lay["dpix"][k], B * hs[k] * ws[k] * 4) for k in range(5)] +
              [(f"g{i}", lay["g"][i], B * H * W * 64 * 4) for i in range(2)])
    assert len(pieces) == _lib.LPIPS_WS_NUM_PIECES
    for kind in ("y", "pool", "arg", "dpix", "g"):
        assert lay[kind] == sorted(lay[kind]), kind
    assert max(o for _, o, _ in pieces[:-2]) < lay["g"][0]                       # the backward's scratch comes last
    pieces.sort(key=lambda p: p[1])
    assert pieces[0][1] == 0
    for (n0, o0, s0), (n1, o1, _) in zip(pieces, pieces[1:]):
        assert o0 % 256 == 0 and o0 + s0 <= o1, (n0, n1)
    name, o, s = pieces[-1]
    assert o % 256 == 0 and o + s <= lay["total"] < o + s + 256, name


def test_ws_layout_refuses_what_ws_bytes_refuses():
    lib = _lib.load()
    offs = (C.c_size_t * _lib.LPIPS_WS_NUM_PIECES)()
    n, t = C.c_size_t(0), C.c_size_t(0)
    for B, H, W in ((0, 128, 128), (1, 15, 128), (1, 128, 15), (-1, 64, 64), (1, 16, 16), (1, 4096, 4096), (1, 4096, 4095),
                    (2, 2048, 4096), (2, 2048, 4095), (1 << 20, 16, 16), (3, 37, 53)):
        a = lib.sg_lpips_ws_bytes(B, H, W, C.byref(n))
        t.value = 7
        b = lib.sg_lpips_ws_layout(B, H, W, offs, C.byref(t))
        assert (a == 0) == (b == 0), (B, H, W)
        assert t.value == (n.value if a == 0 else 7), (B, H, W)
        if b:
            assert b"sg_lpips_ws_layout" in lib.sg_last_error()
    assert lib.sg_lpips_ws_layout(1, 16, 16, None, C.byref(t)) != 0 and lib.sg_lpips_ws_layout(1, 16, 16, offs, None) != 0
