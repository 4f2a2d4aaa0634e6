"""CPU tests of the avatar initialisation (sings_amd/avatar_init.py): the committed fixture is self-consistent, and the plain-Python
restatement of the ReduceLROnPlateau state machine -- the one ``sg_plateau_step`` runs on the device -- takes torch's decisions."""
import os

import numpy as np
import pytest

from plateau_case import sequences, torch_rates

FLOATS = ("scales", "scales_aux", "normals", "rotmat", "rot6d_canon", "rotq")
ROTATIONS = ("rotmat", "rot6d_canon", "rotq")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avatar_init_golden.npz"))


@pytest.mark.parametrize("case", ["s24", "pole"])
def test_fixture_is_self_consistent(golden, case):
    V = golden[f"{case}_verts"].shape[0]
    mask = golden[f"{case}_rot_mask"].astype(bool)
    assert mask.shape == (V,) and (~mask).sum() <= 0.1 * V            # the cap on what the rotation outputs leave out
    c = golden[f"{case}_normals_f64"][:, 2]
    assert np.array_equal(mask, 1.0 + c >= 0.05)
    for k in FLOATS:
        a, b, bound = golden[f"{case}_{k}_f32"], golden[f"{case}_{k}_f64"], float(golden[f"{case}_bound_{k}"])
        assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape and a.shape[0] == V
        rows = mask if k in ROTATIONS else np.ones(V, bool)
        assert np.isfinite(a[rows]).all() and np.isfinite(b[rows]).all()
        assert 0.0 < bound < 1e-5 and np.abs(a[rows].astype(np.float64) - b[rows]).max() <= bound
    # the incident rows: first < second, both contain the vertex, and no smaller row does
    edges, first, second = golden[f"{case}_edges"], golden[f"{case}_first"], golden[f"{case}_second"]
    assert (edges[:, 0] < edges[:, 1]).all() and (np.lexsort((edges[:, 1], edges[:, 0])) == np.arange(len(edges))).all()
    for v in range(V):
        rows = np.nonzero((edges == v).any(1))[0]
        assert first[v] == rows[0] and second[v] == rows[1]
    # the scale rule as written, from the stored rows, in fp64
    x = golden[f"{case}_verts"].astype(np.float64)
    mult, thickness, _ = golden[f"{case}_params"]
    e0, e1 = edges[first], edges[second]
    length = np.float64(np.float32(mult)) * np.maximum(np.linalg.norm(x[e0[:, 0]] - x[e1[:, 0]], axis=1),
                                                        np.linalg.norm(x[e0[:, 1]] - x[e1[:, 1]], axis=1))
    log_scale = np.log(length)[:, None] * np.array([1.0, 1.0, np.float64(np.float32(thickness))])
    assert np.allclose(np.exp(log_scale), golden[f"{case}_scales_f64"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("patience", [3, 100])
def test_plateau_rule_takes_torchs_decisions(patience):
    """Per-step rates EQUAL torch's: with factor 0.5 a halving is exact in fp32 and fp64."""
    from sings_amd.avatar_init import PlateauRule
    fired = set()
    for name, base, losses in sequences(patience):
        rule = PlateauRule(base, patience=patience, factor=0.5)
        want = torch_rates(base, losses, patience)
        got = [list(rule.step(x)) for x in losses]
        assert got == want, name
        if want[-1] != list(base):
            fired.add(name)
        if name == "eps_stops":
            assert want[-1][0] == 1.5e-8 and want[-1][1] == 1e-3 * 0.5 ** 3      # the small group stopped after one halving
        if name == "just_in_time":
            assert want[2 * patience + 1] == list(base) and want[2 * patience + 2] == [0.5 * b for b in base]
        if name == "plateau":
            assert want[-1] == [0.25 * b for b in base]
    # ("below_threshold": every third step is better than the best by more than the threshold, the count never passes 2: no reduction)
    assert fired == {"plateau", "never_enough", "just_in_time", "two_in_a_row", "eps_stops"}


def test_plateau_rule_refuses_a_bad_factor():
    from sings_amd.avatar_init import PlateauRule
    with pytest.raises(ValueError):
        PlateauRule([1e-3], factor=1.0)
