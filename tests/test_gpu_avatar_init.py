"""The avatar initialisation on the GPU (sings_amd/avatar_init.py, csrc/sg_init.hip): ``initial_attributes`` against the fixture of
tests/golden/gen_avatar_init_golden.py, ``sg_attr_mse`` against ``torch.nn.functional.mse_loss`` in fp64, and the device
ReduceLROnPlateau launch against its plain-Python restatement."""
import os

import numpy as np
import pytest
import torch

from plateau_case import sequences

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FLOATS = ("scales", "scales_aux", "normals", "rot6d_canon", "rotq")
ROTATIONS = ("rot6d_canon", "rotq")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avatar_init_golden.npz"))


def _inputs(golden, case):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(golden[f"{case}_{k}"])).to(DEV)
    return t("verts"), t("faces"), t("edges")


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ---- initial values
@pytest.mark.parametrize("case", ["s24", "pole"])
def test_initial_attributes_match_the_fixture(golden, case):
    from sings_amd.avatar_init import initial_attributes
    verts, faces, edges = _inputs(golden, case)
    mult, thickness, opacity = (float(x) for x in golden[f"{case}_params"])
    out = initial_attributes(verts, faces, edges, init_scale_multiplier=mult, thickness_factor=thickness, init_opacity=opacity)
    V = int(verts.shape[0])
    # integers: equal
    for k in ("first", "second"):
        assert out[k].dtype == torch.int32 and np.array_equal(out[k].cpu().numpy(), golden[f"{case}_{k}"]), k
    # floats: within four times the reference's own fp32 error (the fixture records it per array); rotations on 1 + c >= 0.05 only
    mask = golden[f"{case}_rot_mask"].astype(bool)
    for k in FLOATS:
        got, want, bound = out[k].cpu().numpy().astype(np.float64), golden[f"{case}_{k}_f64"], float(golden[f"{case}_bound_{k}"])
        assert out[k].dtype == torch.float32 and got.shape == want.shape, k
        rows = mask if k in ROTATIONS else np.ones(V, bool)
        err = np.abs(got[rows] - want[rows]).max()
        print(f"{case} {k}: max error {err:.3e}, allowed {4 * bound:.3e}")
        assert err <= 4 * bound, (k, err, bound)
    # constants: exact
    assert out["xyz_offsets"].shape == (V, 3) and float(out["xyz_offsets"].abs().max()) == 0.0
    shs = out["shs"].cpu().numpy()
    assert shs.shape == (V, 16, 3) and (shs[:, 0] == 0.5).all() and (shs[:, 1:] == 0.0).all()
    assert out["opacity"].shape == (V, 1) and (out["opacity"].cpu().numpy() == np.float32(opacity)).all()
    # a second call: the same bits
    again = initial_attributes(verts, faces, edges, init_scale_multiplier=mult, thickness_factor=thickness, init_opacity=opacity)
    assert set(again) == set(out)
    for k, v in out.items():
        assert _bits_equal(v, again[k]), k


def test_initial_attributes_special_normals():
    """n = +z gives the identity and n = -z the half-turn about x (the reference: 0 / 0): a flat fan around a centre vertex, wound
    either way."""
    from sings_amd.avatar_init import initial_attributes
    from sings_amd.topology import unique_edges
    ring = [[np.cos(a), np.sin(a), 0.0] for a in np.arange(5) * 2 * np.pi / 5]
    verts = torch.tensor([[0.0, 0.0, 0.0]] + ring, dtype=torch.float32, device=DEV)
    up = torch.tensor([[0, 1 + i, 1 + (i + 1) % 5] for i in range(5)], dtype=torch.int32, device=DEV)
    for faces, want in ((up, [1.0, 1.0, 1.0]), (up[:, [0, 2, 1]].contiguous(), [1.0, -1.0, -1.0])):
        edges, _, _ = unique_edges(faces, 6)
        out = initial_attributes(verts, faces, edges)
        assert out["normals"].cpu().tolist() == [[0.0, 0.0, want[2]]] * 6
        assert out["rot6d_canon"].cpu().tolist() == [[want[0], 0.0, 0.0, 0.0, want[1], 0.0]] * 6
        assert bool(torch.isfinite(out["rotq"]).all())


def test_initial_attributes_refuses(golden):
    from sings_amd.avatar_init import initial_attributes
    verts, faces, edges = _inputs(golden, "pole")
    V = int(verts.shape[0])
    # a vertex with one incident edge: one more vertex, tied to vertex 0 by a single row (kept in lexicographic order)
    v1 = torch.cat([verts, verts[:1] + 0.1])
    rows = edges.cpu().numpy()
    at = int(np.searchsorted(rows[:, 0], 1))
    e1 = torch.from_numpy(np.concatenate([rows[:at], [[0, V]], rows[at:]]).astype(np.int32)).to(DEV)
    with pytest.raises(ValueError, match="fewer than two"):
        initial_attributes(v1, faces, e1)
    # bad edge rows: the kernels range-check every row before they use it and skip it
    for bad in ([5, 5], [7, 3], [3, V + 7], [-1, 4]):
        e2 = edges.clone()
        e2[11] = torch.tensor(bad, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="0 <= a < b"):
            initial_attributes(verts, faces, e2)
    f2 = faces.clone()
    f2[3, 1] = V
    with pytest.raises(IndexError):
        initial_attributes(verts, f2, edges)
    # host tensors: no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        initial_attributes(verts.cpu(), faces, edges)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        initial_attributes(verts, faces.cpu(), edges)
    with pytest.raises(ValueError):
        initial_attributes(verts, faces.long(), edges)
    # and the untouched inputs still pass
    initial_attributes(verts, faces, edges)


# ---- the pre-fit's loss
def _mse_case(N, with_rot, seed):
    from sings_amd.avatar_init import ATTR_KEYS, ATTR_WIDTHS
    g = torch.Generator().manual_seed(seed)
    shape = {"shs": (N, 16, 3)}
    outs, tgts = {}, {}
    for k, w in zip(ATTR_KEYS, ATTR_WIDTHS):
        if k == "rot6d_canon" and not with_rot:
            outs[k] = None
            tgts[k] = torch.randn(N, w, generator=g).to(DEV)       # a target the model has no output for: skipped
            continue
        s = shape.get(k, (N, w))
        outs[k] = (torch.randn(*s, generator=g) * (0.3 + 0.2 * w)).to(DEV).requires_grad_(True)
        tgts[k] = torch.randn(*s, generator=g).to(DEV)
    return outs, tgts


@pytest.mark.parametrize("with_rot", [True, False])
@pytest.mark.parametrize("N", [1, 65, 362, 4099])
def test_attr_mse_against_fp64(N, with_rot):
    from sings_amd.avatar_init import ATTR_KEYS, attribute_mse
    outs, tgts = _mse_case(N, with_rot, 100 + N)
    keys = [k for k in ATTR_KEYS if outs[k] is not None]
    ld = attribute_mse(outs, tgts)
    assert list(ld) == ["loss_" + k for k in keys]
    weights = {k: w for k, w in zip(ATTR_KEYS, (1.0, 3.0, 0.5, 1.25, 0.75, 7.0))}
    for weighted in (False, True):
        for k in keys:
            outs[k].grad = None
        ld = attribute_mse(outs, tgts)
        total = sum(ld["loss_" + k] * (weights[k] if weighted else 1.0) for k in keys)
        total.backward()
        for k in keys:
            o64 = outs[k].detach().double().requires_grad_(True)
            ref = torch.nn.functional.mse_loss(o64, tgts[k].double())
            (ref * (weights[k] if weighted else 1.0)).backward()
            numel = o64.numel()
            # the value: an fp32 sum of numel non-negative terms
            rel = abs(float(ld["loss_" + k].detach()) - float(ref.detach())) / float(ref.detach())
            assert rel <= 4 * 2.0 ** -23 * np.sqrt(numel), (k, rel)
            # the gradient, element by element: two roundings (the difference, the division; a weight that is no power of two is a
            # third: 3 * 2^-24 < 2^-22)
            err = (outs[k].grad.double() - o64.grad).abs()
            assert bool((err <= 2.0 ** -22 * o64.grad.abs() + 1e-12).all()), (k, weighted, float(err.max()))
    # two calls: the same bits, values and gradients
    a, b = attribute_mse(outs, tgts), attribute_mse(outs, tgts)
    ga = torch.autograd.grad(sum(a.values()), [outs[k] for k in keys])
    gb = torch.autograd.grad(sum(b.values()), [outs[k] for k in keys])
    for k in a:
        assert _bits_equal(a[k].detach().reshape(1), b[k].detach().reshape(1))
    for x, y in zip(ga, gb):
        assert _bits_equal(x, y)


def test_attr_mse_engine_and_refusals():
    from sings_amd.avatar_init import ATTR_KEYS, AttrMSEEngine, attribute_mse
    N = 362
    outs, tgts = _mse_case(N, False, 5)
    keys = [k for k in ATTR_KEYS if outs[k] is not None]
    ld = attribute_mse(outs, tgts)
    grads = torch.autograd.grad(sum(ld.values()), [outs[k] for k in keys])
    eng = AttrMSEEngine(N, DEV, keys)
    flat = lambda d: {k: d[k].detach().reshape(N, -1) for k in keys}
    got = eng(flat(outs), flat(tgts))
    for k, g in zip(keys, grads):
        assert _bits_equal(got[k], g.reshape(N, -1)), k
        assert float(eng.terms[ATTR_KEYS.index(k)]) == float(ld["loss_" + k].detach())
    assert float(eng.terms[ATTR_KEYS.index("rot6d_canon")]) == 0.0
    total = np.float32(0)
    for k in keys:
        total = np.float32(total + np.float32(float(ld["loss_" + k].detach())))
    assert float(eng.loss) == float(total)                              # the sum: fp32, in the keys' order
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        attribute_mse({k: (v.detach().cpu() if v is not None else None) for k, v in outs.items()}, tgts)
    with pytest.raises(ValueError):
        attribute_mse({"scales": outs["scales"]}, {"scales": tgts["scales"][:-1]})
    with pytest.raises(ValueError):
        attribute_mse({"scales": None}, tgts)


# ---- ReduceLROnPlateau on the device
def test_device_plateau_follows_the_rule():
    from sings_amd.avatar_init import DevicePlateau, PlateauRule
    from sings_amd.optim import hyper_row
    P = 3
    for name, base, losses in sequences(P):
        n = len(losses)
        assert n <= 40
        rows = np.stack([hyper_row(lr, 0.9, 0.999, 1e-15, 7) for lr in base])
        base_hyper = torch.from_numpy(rows).to(DEV)
        hyper = torch.zeros_like(base_hyper)
        terms = torch.zeros(8, dtype=torch.float32, device=DEV)
        dp = DevicePlateau(base, DEV, patience=P, factor=0.5, log_steps=n, n_terms=7)
        rule = PlateauRule(base, patience=P, factor=0.5)
        want_mult = []
        for i in range(n):
            hyper.copy_(base_hyper)                                    # what FusedAdam.advance() does before every step
            dp.begin_step(hyper, terms[6:7], terms)                    # digests the loss of step i - 1, then scales column 5
            got = hyper.cpu().numpy()
            want = rows.copy()
            want[:, 5] = rows[:, 5] * np.asarray(rule.multipliers, np.float32)
            assert np.array_equal(got, want), (name, i)
            want_mult.append(list(rule.multipliers))
            terms[6] = float(losses[i])                                # the loss of step i, as sg_attr_mse leaves it
            terms[0] = float(i)
            rule.step(losses[i])
        dp.finish(terms[6:7], terms)
        mult, log, mult_steps = dp.read()
        assert list(mult) == list(rule.multipliers), name
        assert np.array_equal(mult_steps, np.asarray(want_mult)), name
        assert np.array_equal(log[:, 6], losses.astype(np.float64), equal_nan=True) and np.array_equal(log[:, 0], np.arange(n)), name
