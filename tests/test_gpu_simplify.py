"""``topology.collapse_edges`` (csrc/sg_mesh.hip: the whole sequential collapse loop in one launch) against the reference's own
``geometry_ops.collapse_edges`` (tests/golden/simplify_golden.npz, made by tests/golden/gen_simplify_golden.py).

Equality is demanded, not closeness: the generator asserts that in every iteration of every case the two longest live edges differ by
at least 16 * 2^-23 relative, and an fp32 length carries about four roundings, so every correct fp32 implementation collapses the
reference's edges in the reference's order.  The reference's face ROWS come in the order of a host hash; they are compared as a set
of rows with winding (both sides ordered by their sorted-corner triple), and ours must be in the original order of the faces they
come from (``<case>_new_faces_ordered``: the generator's restatement, itself held to the reference's set)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = ["s1_all", "pole", "half", "half_full", "rand60", "big_all", "comp_prune_collapse"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simplify_golden.npz"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(g, name, sel=None, **over):
    from sings_amd.topology import collapse_edges
    kw = dict(verts=_t(g[f"{name}_verts"]), verts_attr=_t(g[f"{name}_attr"]), faces=_t(g[f"{name}_faces"]).long(),
              selected_edges=_t(g[f"{name}_sel"] if sel is None else sel).long(), collapse_rate=float(g[f"{name}_rate"]))
    kw.update(over)
    return collapse_edges(kw["verts"], kw["verts_attr"], kw["selected_edges"], kw["faces"], collapse_rate=kw["collapse_rate"],
                          return_collapses=True)


@pytest.fixture(scope="module")
def results(golden):
    """every case once; shared, never written"""
    return {name: _call(golden, name) for name in CASES}


def _by_vertex_set(faces):
    key = np.sort(faces, axis=1)
    assert len(np.unique(key, axis=0)) == len(key), "two faces on the same three vertices"
    return faces[np.lexsort((key[:, 2], key[:, 1], key[:, 0]))]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


@pytest.mark.parametrize("name", CASES)
def test_equals_the_reference(golden, results, name):
    g = golden
    new_verts, new_faces, new_attr, prune, collapses = results[name]
    assert new_faces.dtype == torch.int64 and prune.dtype == torch.bool and tuple(prune.shape) == (len(g[f"{name}_verts"]),)
    want_prune = g[f"{name}_prune_mask"].astype(bool)
    print(f"{name}: collapses {collapses} (reference {int(g[f'{name}_collapses'])}), pruned {int(prune.sum())} ({int(want_prune.sum())}), "
          f"faces {len(new_faces)} ({len(g[f'{name}_new_faces'])}), reference margin {float(g[f'{name}_margin']):.3g}")
    assert collapses == int(g[f"{name}_collapses"])
    assert np.array_equal(prune.cpu().numpy(), want_prune)
    # the survivors' rows: the INPUT rows, bit for bit
    keep = ~want_prune
    assert np.array_equal(new_verts.cpu().numpy().view(np.uint32), g[f"{name}_verts"][keep].view(np.uint32))
    assert np.array_equal(new_attr.cpu().numpy().view(np.uint32), g[f"{name}_attr"][keep].view(np.uint32))
    # the faces: the reference's set of rows with winding; ours in the original order, the first occurrence kept
    ours = new_faces.cpu().numpy()
    assert np.array_equal(_by_vertex_set(ours), _by_vertex_set(g[f"{name}_new_faces"].astype(np.int64)))
    assert np.array_equal(ours, g[f"{name}_new_faces_ordered"])
    assert int(ours.min()) == 0 and int(ours.max()) == int(keep.sum()) - 1 and len(np.unique(ours)) == int(keep.sum())


def test_the_exhausted_list_ends_the_loop(golden, results):
    """collapse_rate 1.0 on the half sphere asks for 49 collapses; the list is empty after 48 (the reference's "No edge could be
    collapsed" break)."""
    n = len(np.unique(golden["half_full_sel"]))
    assert int(n * float(golden["half_full_rate"])) == 49 and results["half_full"][4] == 48
    assert int(golden["half_full_depth"]) >= 6


def test_duplicated_and_shuffled_rows_give_the_same_bits(golden, results):
    sel = golden["s1_all_sel_shuffled"]
    assert len(sel) == 2 * len(golden["s1_all_sel"]) and not np.array_equal(sel[:len(sel) // 2], golden["s1_all_sel"])
    again = _call(golden, "s1_all", sel=sel)
    for a, b in zip(again[:4], results["s1_all"][:4]):
        assert _same_bits(a, b)
    assert again[4] == results["s1_all"][4]
    # int32 rows and int32 faces are taken as they are
    i32 = _call(golden, "s1_all", selected_edges=_t(golden["s1_all_sel"]), faces=_t(golden["s1_all_faces"]))
    assert all(_same_bits(a, b) for a, b in zip(i32[:4], results["s1_all"][:4]))


@pytest.mark.parametrize("name", ["big_all", "rand60"])
def test_the_same_call_twice_gives_the_same_bits(golden, results, name):
    again = _call(golden, name)
    assert all(_same_bits(a, b) for a, b in zip(again[:4], results[name][:4])) and again[4] == results[name][4]


@pytest.mark.parametrize("name", ["pole", "rand60"])
def test_unique_edges_of_the_result(golden, results, name):
    from sings_amd.topology import unique_edges
    new_verts, new_faces = results[name][0], results[name][1]
    edges, counts, _ = unique_edges(new_faces, new_verts.shape[0])
    f = new_faces.cpu()
    e = torch.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    want, want_counts = torch.unique(e, dim=0, return_counts=True)
    assert torch.equal(edges.cpu().long(), want) and torch.equal(counts.cpu().long(), want_counts)


def test_inputs_are_not_written(golden):
    g, name = golden, "half"
    verts, attr, sel, faces = _t(g[f"{name}_verts"]), _t(g[f"{name}_attr"]), _t(g[f"{name}_sel"]).long(), _t(g[f"{name}_faces"]).long()
    from sings_amd.topology import collapse_edges
    collapse_edges(verts, attr, sel, faces)
    assert np.array_equal(verts.cpu().numpy(), g[f"{name}_verts"]) and np.array_equal(attr.cpu().numpy(), g[f"{name}_attr"])
    assert np.array_equal(sel.cpu().numpy(), g[f"{name}_sel"]) and np.array_equal(faces.cpu().numpy(), g[f"{name}_faces"])


def test_refusals(golden, results):
    from sings_amd.topology import collapse_edges, collapse_max_edges
    g = golden
    cap = collapse_max_edges()
    assert cap >= 10000                                             # the reference's 2 * prune_max_n_gs_once never hits it
    verts, attr, faces, sel = g["half_verts"], g["half_attr"], g["half_faces"], g["half_sel"]
    V = len(verts)
    lower = int(np.nonzero(verts[:, 2] < 0)[0][3])                  # a vertex no selected edge touches
    assert lower not in sel

    def run(**over):
        return _call(g, "half", **over)
    with pytest.raises(ValueError, match="at most"):
        run(sel=np.tile(sel[:1], (cap + 1, 1)))
    for row in ([5, 5], [7, 3], [-1, 4], [3, V], [V, V + 1], [2 ** 31 + 1, 2 ** 31 + 2]):
        bad = sel.astype(np.int64).copy()
        bad[11] = row
        with pytest.raises(ValueError, match="selected edge"):
            run(sel=bad)
    for at, value in ((int(sel[4, 1]), np.inf), (int(sel[9, 0]), np.nan), (lower, np.nan), (lower, -np.inf)):
        v = verts.copy()
        v[at, 1] = value
        with pytest.raises(ValueError, match="not finite"):
            run(verts=_t(v))
    f = faces.astype(np.int64).copy()
    f[17, 2] = V
    with pytest.raises(IndexError):
        run(faces=_t(f))
    for k in ("verts", "verts_attr", "selected_edges", "faces"):
        cpu = dict(verts=torch.from_numpy(verts), verts_attr=torch.from_numpy(attr), selected_edges=torch.from_numpy(sel).long(),
                   faces=torch.from_numpy(faces).long())[k]
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            run(**{k: cpu})
    with pytest.raises(ValueError, match="float32"):
        run(verts=_t(verts.astype(np.float64)))
    # every edge of a closed mesh collapsed: one class, every face degenerate (the reference fails in vstack there)
    with pytest.raises(RuntimeError, match="left no face"):
        _call(g, "s1_all", collapse_rate=1.0)
    # and none of it leaves anything behind: the next call is the clean one
    again = run()
    assert all(_same_bits(a, b) for a, b in zip(again[:4], results["half"][:4]))


def test_nothing_selected_and_rate_zero(golden):
    """no selected edge, or a rate of 0: no collapse; the mesh comes back with only its duplicate faces and isolated vertices removed"""
    g, name = golden, "half"
    faces = g[f"{name}_faces"].astype(np.int64)
    for over in (dict(sel=np.zeros((0, 2), np.int64)), dict(collapse_rate=0.0)):
        new_verts, new_faces, _, prune, collapses = _call(g, name, **over)
        assert collapses == 0 and not bool(prune.any()) and np.array_equal(new_faces.cpu().numpy(), faces)
        assert np.array_equal(new_verts.cpu().numpy().view(np.uint32), g[f"{name}_verts"].view(np.uint32))
