"""CPU tests of the LPIPS-VGG patch loss: weight packing, the patch sampler and the fp64 oracle against vectors produced by the
reference's own loss.py / sampler.py (tests/golden/gen_lpips_golden.py), and the new entry points' argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

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
