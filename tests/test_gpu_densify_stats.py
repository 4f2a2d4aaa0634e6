"""``sings_amd.density.densify_stats`` (csrc/sg_density.hip) against its numpy fp64 twin ``densify_stats_host``.

Bounds.  ``denom`` and ``max_radii`` are sums and maxima of small integers: exactly equal.  ``accum``: ``|got - ref| <= (K + 4) *
2**-24 * ref`` -- one rounding each (half an ulp, 2**-24 relative) for the product, the fma, the square root, the K - 1 additions of
the frames' non-negative norms and the addition into the prior value; every rounded quantity is at most the final sum, so the
relative errors add up to at most K + 3 of them.  The test prints the worst ratio it saw.

Inputs: ``|g|`` log-uniform in [1e-6, 1e2] with random signs and exact zeros mixed in, radii in [0, 5000] with about a third zero (a few
negative), non-zero prior contents in all three arrays (``denom`` / ``max_radii`` integer-valued, as counts and radii are)."""
import numpy as np
import pytest
import torch

from sings_amd import density as dn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = [1, 63, 64, 65, 255, 257, 1000]
FRAMES = [1, 3, 16]


def _case(N, K, seed=0, finite=False):
    rs = np.random.RandomState(1000 * K + N + seed)
    mag = 10.0 ** rs.uniform(-6, 2, (K, N, 3))
    g = (mag * rs.choice([-1.0, 1.0], (K, N, 3))).astype(np.float32)
    g[rs.rand(K, N, 3) < 0.1] = 0.0
    if not finite:
        g[..., 2] = np.nan                                       # the third column is never read
    radii = rs.randint(1, 5001, (K, N)).astype(np.int32)
    hide = rs.rand(K, N)
    radii[hide < 1 / 3] = 0
    radii[hide < 0.02] = -1
    accum = rs.uniform(0.5, 50.0, (N, 1)).astype(np.float32)
    denom = rs.randint(1, 40, (N, 1)).astype(np.float32)
    mx = rs.randint(1, 3000, N).astype(np.float32)
    return g, radii, accum, denom, mx


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(g, radii, accum, denom, mx, gate=None):
    out = [_t(accum), _t(denom), _t(mx)]
    dn.densify_stats(_t(g), _t(radii), *out, gate=None if gate is None else torch.tensor([gate], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_accum(got, ref, K, what):
    got, ref = got.astype(np.float64).reshape(-1), ref.reshape(-1)
    ratio = np.abs(got - ref) / ((K + 4) * 2.0 ** -24 * ref)
    print(f"{what}: worst |got - ref| / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0, f"{what}: worst |got - ref| / ((K + 4) 2^-24 ref) = {ratio.max():.3f} at row {int(ratio.argmax())}"


@pytest.mark.parametrize("K", FRAMES)
@pytest.mark.parametrize("N", SIZES)
def test_against_the_fp64_twin(N, K):
    case = _case(N, K)
    want = dn.densify_stats_host(*case)
    got = _run(*case)
    assert np.isfinite(got[0]).all()
    assert np.array_equal(got[1].astype(np.float64), want[1]) and np.array_equal(got[2].astype(np.float64), want[2])
    _check_accum(got[0], want[0], K, f"N={N} K={K}")
    assert got[0].shape == (N, 1) and got[2].shape == (N,)
    again = _run(*case)                                          # two runs: the same bits
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    assert not np.array_equal(got[0], case[2]) or not (case[1] > 0).any()


@pytest.mark.parametrize("K", [1, 3])
def test_an_invisible_row_keeps_its_bits_whatever_its_gradient_holds(K):
    N = 257
    g, radii, accum, denom, mx = _case(N, K)
    rows = np.array([0, 63, 64, 200, 256])
    radii[:, rows] = 0
    radii[0, 64] = -5
    g[:, rows] = np.nan
    g[:, 63, 0], g[:, 200, 1] = np.inf, -np.inf
    got = _run(g, radii, accum, denom, mx)
    for a, b in zip(got, (accum, denom, mx)):
        assert np.array_equal(_bits(a).reshape(N)[rows], _bits(b).reshape(N)[rows])
        assert np.isfinite(a).all()
    want = dn.densify_stats_host(g, radii, accum, denom, mx)
    assert np.array_equal(got[1].astype(np.float64), want[1]) and np.array_equal(got[2].astype(np.float64), want[2])
    _check_accum(got[0], want[0], K, f"invisible rows K={K}")


@pytest.mark.parametrize("N, K", [(65, 1), (1000, 16)])
def test_the_gate(N, K):
    case = _case(N, K)
    closed = _run(*case, gate=0)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(closed, case[2:]))
    opened, ungated = _run(*case, gate=1), _run(*case)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(opened, ungated))
    assert not np.array_equal(opened[1], case[3])


def test_one_frame_without_its_axis():
    g, radii, accum, denom, mx = _case(255, 1)
    flat, framed = _run(g[0], radii[0], accum, denom, mx), _run(g, radii, accum, denom, mx)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(flat, framed))
    assert not np.array_equal(flat[0], accum)


@pytest.mark.parametrize("N, K", [(1, 1), (257, 3), (1000, 16)])
def test_against_the_torch_chain_on_finite_gradients(N, K):
    """``AvatarStep.add_densification_stats`` without a gate -- the masked torch arithmetic -- on the same inputs, every gradient
    finite: the same ``accum`` bound for the fused launch against the twin and against the chain, ``denom`` / ``max_radii`` equal."""
    from sings_amd.train_step import AvatarStep
    case = _case(N, K, seed=5, finite=True)
    g, radii, accum, denom, mx = case
    radii = np.maximum(radii, 0)                                 # (the chain takes max(radii) over the frames: no negative radius)
    holder = AvatarStep.__new__(AvatarStep)
    torch.nn.Module.__init__(holder)
    holder.stats_gate = None
    holder.xyz_gradient_accum, holder.denom, holder.max_radii2D = _t(accum), _t(denom), _t(mx)
    m2d = _t(g).requires_grad_(True)
    m2d.grad = _t(g)
    holder.add_densification_stats({"viewspace_points": m2d, "radii": _t(radii)})
    chain = [holder.xyz_gradient_accum.cpu().numpy(), holder.denom.cpu().numpy(), holder.max_radii2D.cpu().numpy()]
    fused = _run(g, radii, accum, denom, mx)
    want = dn.densify_stats_host(g, radii, accum, denom, mx)
    assert np.array_equal(fused[1], chain[1]) and np.array_equal(fused[2], chain[2])
    _check_accum(fused[0], want[0], K, f"fused N={N} K={K}")
    _check_accum(fused[0], chain[0].astype(np.float64), K, f"fused vs torch chain N={N} K={K}")
    holder.stats_gate = torch.ones(1, dtype=torch.int32, device=DEV)      # the same call through the module's gated path
    holder.xyz_gradient_accum, holder.denom, holder.max_radii2D = _t(accum), _t(denom), _t(mx)
    holder.add_densification_stats({"viewspace_points": m2d, "radii": _t(radii)})
    torch.cuda.synchronize()
    assert np.array_equal(_bits(holder.xyz_gradient_accum.cpu().numpy()), _bits(fused[0]))
    assert np.array_equal(holder.denom.cpu().numpy(), fused[1]) and np.array_equal(holder.max_radii2D.cpu().numpy(), fused[2])


def test_wrong_shapes_and_devices_are_refused():
    g, radii, accum, denom, mx = (_t(a) for a in _case(64, 3))
    with pytest.raises(ValueError, match="radii must be"):
        dn.densify_stats(g, radii[:2], accum, denom, mx)
    with pytest.raises(ValueError, match="accum must hold 64"):
        dn.densify_stats(g, radii, accum[:5], denom, mx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dn.densify_stats(g, radii.cpu(), accum, denom, mx)
    with pytest.raises(RuntimeError, match="gate must be a contiguous"):
        dn.densify_stats(g, radii, accum, denom, mx, gate=torch.ones(1, device=DEV))
    with pytest.raises(ValueError, match="K = 17"):
        dn.densify_stats(torch.zeros(17, 4, 3, device=DEV), torch.zeros(17, 4, dtype=torch.int32, device=DEV), accum[:4], denom[:4], mx[:4])
