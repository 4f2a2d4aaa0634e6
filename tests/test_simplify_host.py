"""CPU tests of the pruning half of the ``hybrid`` strategy: ``topology.simplify_decision`` against the recorded composite of
sings_hybrid.py:1157-1222 (tests/golden/simplify_golden.npz, ``comp_*``), the reference's quirks its docstring names, and the
bookkeeping of ``MeshState.prune`` (sings_hybrid.py:1243-1252) on stand-in tensors."""
import os

import numpy as np
import pytest
import torch

from sings_amd.topology import MeshState, simplify_decision

REASONS = {0: None, 1: "min_n_gs", 2: "no_edges", 3: "too_many_edges"}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simplify_golden.npz"))


def _decide(g, name, **over):
    t = lambda k: torch.from_numpy(g[f"{name}_{k}"])
    opacity_threshold, scale_threshold, dead_grad, large_scale, prune_max, min_n_gs = g[f"{name}_params"].tolist()
    kw = dict(dead_grad=dead_grad, large_scale=large_scale, prune_max_n_gs_once=int(prune_max), min_n_gs=int(min_n_gs))
    kw.update(over)
    return simplify_decision(t("accum"), t("denom"), t("opacity"), t("scales"), t("vertex_label"), t("faces"), opacity_threshold,
                             scale_threshold, **kw)


@pytest.mark.parametrize("name", ["comp_prune", "comp_skip_min", "comp_skip_none", "comp_skip_many"])
def test_decision_equals_the_recorded_composite(golden, name):
    mask, edges, reason = _decide(golden, name)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (len(golden[f"{name}_accum"]),)
    assert edges.dtype == torch.int64 and edges.dim() == 2 and edges.shape[1] == 2
    assert reason == REASONS[int(golden[f"{name}_rule"])]
    assert np.array_equal(mask.numpy(), golden[f"{name}_vert_mask"].astype(bool))
    assert np.array_equal(edges.numpy(), golden[f"{name}_selected_edges"].reshape(-1, 2))
    if reason is None:
        # unique rows a < b in lexicographic order, every endpoint selected, no hand
        e = edges.numpy()
        assert len(e) > 0 and bool((e[:, 0] < e[:, 1]).all()) and np.array_equal(e, np.unique(e, axis=0))
        assert bool(mask.numpy()[e].all()) and not np.isin(golden[f"{name}_vertex_label"][mask.numpy()], (6, 7)).any()


def test_a_nan_gradient_is_not_dead(golden):
    """accum / denom = 0 / 0 compares false with ``dead_grad``: a big Gaussian that was never visible is not selected as dead (NaN is not
    zeroed here, unlike in ``subdivide_decision``); x / 0 = inf is not dead either."""
    g, name = golden, "comp_prune"
    accum, denom, scales = g[f"{name}_accum"], g[f"{name}_denom"], g[f"{name}_scales"]
    nan = (accum[:, 0] == 0) & (denom[:, 0] == 0)
    big = scales[:, 0] > g[f"{name}_params"][3]
    assert (nan & big).any(), "the composite holds a big never-visible Gaussian"
    # opacity_threshold 0: only the dead-and-big term can select
    mask, _, _ = _decide(g, name, min_n_gs=None, exclude=None)
    only_dead, _, _ = simplify_decision(*(torch.from_numpy(g[f"{name}_{k}"]) for k in ("accum", "denom", "opacity", "scales", "vertex_label",
                                                                                     "faces")), 0.0, 0.0, exclude=None)
    assert not only_dead.numpy()[nan].any() and not only_dead.numpy()[denom[:, 0] == 0][accum[denom[:, 0] == 0, 0] > 0].any()
    with np.errstate(divide="ignore", invalid="ignore"):
        want = big & (accum[:, 0] / denom[:, 0] < 0.0005)
    assert np.array_equal(only_dead.numpy(), want) and want.any() and bool((mask.numpy() | ~want).all())


def test_min_n_gs_none_means_no_floor_and_the_floor_is_inclusive(golden):
    N = len(golden["comp_prune_accum"])
    assert _decide(golden, "comp_prune", min_n_gs=None)[2] is None
    assert _decide(golden, "comp_prune", min_n_gs=N - 1)[2] is None
    mask, edges, reason = _decide(golden, "comp_prune", min_n_gs=N)
    assert reason == "min_n_gs" and not bool(mask.any()) and tuple(edges.shape) == (0, 2)


def test_a_custom_exclude_is_honoured(golden):
    lab = golden["comp_prune_vertex_label"]
    default, _, _ = _decide(golden, "comp_prune")
    nobody, _, _ = _decide(golden, "comp_prune", exclude=None)
    other, e_other, _ = _decide(golden, "comp_prune", exclude=(0, 1, 2))
    assert not default.numpy()[np.isin(lab, (6, 7))].any() and nobody.numpy()[np.isin(lab, (6, 7))].any()
    assert np.array_equal(default.numpy(), nobody.numpy() & ~np.isin(lab, (6, 7)))
    assert np.array_equal(other.numpy(), nobody.numpy() & ~np.isin(lab, (0, 1, 2)))
    assert not np.isin(lab[np.unique(e_other.numpy())], (0, 1, 2)).any()


def test_the_edge_cap_is_twice_prune_max_n_gs_once(golden):
    Es = len(golden["comp_prune_selected_edges"])
    assert Es % 2 == 1
    assert _decide(golden, "comp_prune", prune_max_n_gs_once=(Es + 1) // 2)[2] is None         # Es <= 2 * max
    mask, edges, reason = _decide(golden, "comp_prune", prune_max_n_gs_once=Es // 2)           # Es  > 2 * max
    assert reason == "too_many_edges" and len(edges) == Es and bool(mask.any())


def test_mesh_state_prune_bookkeeping():
    """labels masked, level ids TRUNCATED (the reference's ``_level_id[:n_gs]``), the last level mark moved, faces and edges replaced."""
    N = 10
    labels = torch.arange(N, dtype=torch.int32) % 8
    level = torch.tensor([0.0] * 6 + [1.0] * 4)
    mesh = MeshState(torch.zeros((4, 3), dtype=torch.int32), torch.zeros((6, 2), dtype=torch.int32), labels, level, [0, 6, N])
    keep = torch.tensor([1, 1, 0, 1, 1, 1, 0, 1, 0, 1], dtype=torch.bool)
    new_faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int64)
    edges = torch.tensor([[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]], dtype=torch.int32)
    mesh.prune(new_faces, keep, edges=edges)
    assert mesh.num_verts == 7 and torch.equal(mesh.vertex_label, labels[keep]) and mesh.vertex_label.dtype == torch.int32
    assert torch.equal(mesh.level_id, level[:7]) and mesh.gs_level_mark == [0, 6, 7]
    assert mesh.faces.dtype == torch.int32 and torch.equal(mesh.faces.long(), new_faces) and mesh.edges is edges
    assert mesh.checkpoint_entries()["gs_level_mark"] == [0, 6, 7]
    with pytest.raises(ValueError, match="keep_mask"):
        mesh.prune(new_faces, torch.ones(N, dtype=torch.bool), edges=edges)


def test_the_entry_points_refuse_before_anything_is_launched():
    """sizes out of range, more edges than the cap, a bad rate, NULL pointers: status 1 and a message, with pointers that are never
    dereferenced (no GPU needed)."""
    import ctypes as C
    from sings_amd import _lib
    lib = _lib.load()
    cap = lib.sg_mesh_collapse_max_edges()
    assert cap >= 10000                                             # the reference's 2 * prune_max_n_gs_once = 10 000 never hits it
    assert lib.sg_mesh_collapse_ws_bytes(0, 4) == 0 and lib.sg_mesh_collapse_ws_bytes(-1, 4) == 0 and lib.sg_mesh_collapse_ws_bytes(8, -1) == 0
    assert lib.sg_mesh_collapse_ws_bytes(2 ** 30 + 1, 4) == 0 and lib.sg_mesh_collapse_ws_bytes(8, 715827883) == 0
    small, large = lib.sg_mesh_collapse_ws_bytes(100, 200), lib.sg_mesh_collapse_ws_bytes(110000, 220000)
    assert 0 < small < large and small % 256 == 0 and large % 256 == 0
    fake, half = C.c_void_p(0x1000), C.c_double(0.5)
    build = lambda V, F, Es, rate=half, verts=fake: lib.sg_mesh_collapse_build(V, F, Es, verts, fake, fake, C.byref(rate), fake, fake, None)
    for args, message in (((0, 4, 1), b"V must be >= 1"), ((8, -1, 1), b"F"), ((8, 4, -1), b"Es must be >= 0"),
                          ((8, 4, cap + 1), b"more selected edges"), ((8, 4, 1, C.c_double(-0.5)), b"collapse_rate"),
                          ((8, 4, 1, C.c_double(float("nan"))), b"collapse_rate"), ((8, 4, 1, C.c_double(float("inf"))), b"collapse_rate"),
                          ((8, 4, 1, half, None), b"null pointer")):
        assert build(*args) != 0 and message in lib.sg_last_error(), (args, lib.sg_last_error())
    emit = lambda V, F, Fn, Vn, mask=fake: lib.sg_mesh_collapse_emit(V, F, Fn, Vn, fake, fake, fake, mask, fake, None)
    for args, message in (((0, 4, 0, 0), b"V must be >= 1"), ((8, 4, 5, 8), b"Fn"), ((8, 4, 4, 9), b"Vn"), ((8, 4, -1, 8), b"Fn"),
                          ((8, 4, 4, 8, None), b"null pointer")):
        assert emit(*args) != 0 and message in lib.sg_last_error(), (args, lib.sg_last_error())
