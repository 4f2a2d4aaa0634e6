"""CPU tests of the hybrid densifier's decision (sings_amd.topology.subdivide_decision / rescaled_multiplier) against the composite of
sings_hybrid.py:1026-1147 recorded by tests/golden/gen_topology_golden.py around the reference's own ``subdivide_meshes``.  Boolean and
index outputs are compared exactly.  (The header / prototype agreement of the new entry points is tests/test_abi.py's.)"""
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topology_golden.npz"))


def _decision_inputs(g, name):
    t = lambda k: torch.from_numpy(g[f"{name}_{k}"])
    grad_thr, scale_thr, screen, max_n = g[f"{name}_params"]
    return (t("accum"), t("denom"), t("scales_canon"), t("max_radii2D"), t("vertex_label"), t("faces"), float(grad_thr),
            float(scale_thr)), dict(max_screen_size=float(screen), max_n_gs=int(max_n))


@pytest.mark.parametrize("name", ["comp", "comp_cap"])
def test_decision_matches_the_reference_composite(golden, name):
    from sings_amd.topology import subdivide_decision
    args, kw = _decision_inputs(golden, name)
    mask, faces_idx = subdivide_decision(*args, **kw)
    assert mask.dtype == torch.bool and faces_idx.dtype == torch.int64
    assert np.array_equal(mask.numpy(), golden[f"{name}_selected_pts_mask"].astype(bool))
    # (comp_cap: the capped faces come in score order, largest first -- the order matters to nobody, the golden's is kept anyway)
    assert np.array_equal(faces_idx.numpy(), golden[f"{name}_selected_faces_idx"])


def test_the_cap_bites_in_one_case_only(golden):
    sel = lambda n: (golden[f"{n}_accum"], golden[f"{n}_selected_pts_mask"])
    assert np.array_equal(sel("comp")[0], sel("comp_cap")[0]) and np.array_equal(sel("comp")[1], sel("comp_cap")[1])
    n_all, n_cap = len(golden["comp_selected_faces_idx"]), len(golden["comp_cap_selected_faces_idx"])
    N, max_n = len(golden["comp_cap_accum"]), int(golden["comp_cap_params"][3])
    assert n_cap == (max_n - N) // 3 < n_all
    assert len(golden["comp_cap_sub_vertices"]) <= max_n          # (what the cap is for)


def test_decision_quirks(golden):
    """No screen term without ``max_screen_size``; ``exclude`` honoured (None: nobody); a budget of zero or less subdivides anyway."""
    from sings_amd.topology import subdivide_decision
    args, kw = _decision_inputs(golden, "comp")
    accum, denom, scales, radii, lab, faces, gt, st = args
    grads = torch.nan_to_num(accum / denom, nan=0.0, posinf=float("inf"))
    base = (grads[:, 0] > gt) & (scales[:, 0] > st)
    hands = torch.isin(lab, torch.tensor([6, 7], dtype=lab.dtype))
    m0, _ = subdivide_decision(*args, max_screen_size=None, max_n_gs=None)
    assert torch.equal(m0, base & ~hands)
    m1, _ = subdivide_decision(*args, max_screen_size=kw["max_screen_size"], max_n_gs=None, exclude=None)
    assert torch.equal(m1, base | (radii > kw["max_screen_size"])) and (m1 & hands).any()
    N = accum.shape[0]
    _, f_full = subdivide_decision(*args, **kw)
    for budget in (N, N - 5):
        _, f = subdivide_decision(*args, max_screen_size=kw["max_screen_size"], max_n_gs=budget)
        assert torch.equal(f, f_full)
    # denom == 0 with accum == 0 is NaN -> 0: never selected by the gradient term
    z = (denom[:, 0] == 0) & (accum[:, 0] == 0)
    assert not (m0 & z).any()


@pytest.mark.parametrize("name", ["comp", "comp_cap"])
def test_rescaled_multiplier_matches_the_reference_composite(golden, name):
    from sings_amd.topology import rescaled_multiplier
    scales = torch.from_numpy(golden[f"{name}_scales_canon"])
    mask = torch.from_numpy(golden[f"{name}_selected_pts_mask"].astype(bool))
    want = golden[f"{name}_scaling_multiplier_old"]
    for start in (None, 1.0, torch.ones(scales.shape[0], 1)):
        got = rescaled_multiplier(start, scales, mask)
        assert got.shape == (scales.shape[0], 1) and np.array_equal(got.numpy(), want)
    assert (want[~mask.numpy()] == 1).all() and (want[mask.numpy()] != 1).any()


def test_mesh_state_owns_its_checkpoint_keys():
    from sings_amd import export
    from sings_amd.topology import MeshState
    assert set(MeshState.CHECKPOINT_KEYS) <= set(export.checkpoint_keys())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MeshState.from_faces(torch.zeros((1, 3), dtype=torch.int64), torch.zeros(3, dtype=torch.int32))


def test_topology_refuses_cpu_tensors():
    from sings_amd.topology import subdivide_meshes, unique_edges
    faces = torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unique_edges(faces, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        subdivide_meshes(torch.zeros(3, 3), faces)
