"""The mesh kernels of the hybrid densifier (csrc/sg_mesh.hip through sings_amd.topology) on the GPU against the reference's own
``subdivide_meshes`` as recorded in tests/golden/topology_golden.npz (gen_topology_golden.py).

Every index output is compared EXACTLY.  Float outputs are compared BIT FOR BIT: a midpoint is one addition and one multiplication by
0.5 -- the bits of the reference's ``.mean(axis=1)`` over two rows -- so there is no tolerance to choose."""
import os

import numpy as np
import pytest
import torch

from mesh_case import bumpy_sphere

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = ("s1_all", "s1_five", "s1_one", "s1_dup", "pole", "big", "again", "flip")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topology_golden.npz"))


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _case_inputs(g, name):
    verts = torch.from_numpy(g[f"{name}_verts"]).to(DEV)
    faces = torch.from_numpy(g[f"{name}_faces"]).to(DEV).long()
    idx = torch.from_numpy(g[f"{name}_face_index"]).to(DEV).long() if f"{name}_face_index" in g.files else None
    attrs = {k[len(name) + 6:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith(f"{name}_attr_")}
    return verts, faces, idx, attrs


def _edges_by_torch(faces, mask=None):
    """The definition, with torch on the CPU: unique sorted rows, inverse, counts."""
    f = faces.cpu().long()
    sub = f if mask is None else f[mask.cpu().bool()]
    e = torch.sort(sub[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    if e.shape[0] == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    u, inv, cnt = torch.unique(e, dim=0, return_inverse=True, return_counts=True)
    return u.numpy(), cnt.numpy(), inv.reshape(-1, 3).numpy()


@pytest.mark.parametrize("name", CASES)
def test_subdivide_matches_the_reference(golden, name):
    """Cases 1-4, 6 and 7 of the issue: vertices, faces and every attribute (rows 1, 3, 5, 24 and 55 wide, labels) as recorded."""
    from sings_amd.topology import subdivide_meshes
    verts, faces, idx, attrs = _case_inputs(golden, name)
    nv, nf, na = subdivide_meshes(verts, faces, idx, attrs)
    assert nf.dtype == torch.int64 and nv.dtype == torch.float32
    assert np.array_equal(nf.cpu().numpy(), golden[f"{name}_new_faces"])
    assert np.array_equal(_bits(nv), _bits(golden[f"{name}_new_verts"]))
    assert set(na) == set(attrs)
    for k, v in na.items():
        want = golden[f"{name}_new_attr_{k}"]
        assert v.dtype == attrs[k].dtype and tuple(v.shape) == want.shape, k
        assert np.array_equal(_bits(v), _bits(want)), k
    if name == "s1_all":
        widths = sorted({int(np.prod(v.shape[1:])) for v in attrs.values() if v.dtype == torch.float32} | {3})
        assert widths == [1, 3, 5, 24, 55]
    # int32 labels go through the same kernel and come back int32
    lab32 = attrs["vertex_label"].to(torch.int32)
    _, _, n32 = subdivide_meshes(verts, faces.to(torch.int32), idx, {"vertex_label": lab32})
    assert n32["vertex_label"].dtype == torch.int32
    assert np.array_equal(n32["vertex_label"].cpu().numpy(), golden[f"{name}_new_attr_vertex_label"])


def test_duplicated_indices_are_harmless(golden):
    for k in ("new_faces", "new_verts", "new_attr_lbs_weights"):
        assert np.array_equal(_bits(golden[f"s1_dup_{k}"]), _bits(golden[f"s1_five_{k}"]))


def test_no_face_selected_returns_the_input(golden):
    from sings_amd.topology import subdivide_meshes, unique_edges
    verts, faces, _, attrs = _case_inputs(golden, "s1_all")
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    nv, nf, na = subdivide_meshes(verts, faces, none, attrs)
    assert torch.equal(nv, verts) and torch.equal(nf, faces)
    for k in attrs:
        assert torch.equal(na[k], attrs[k])
    e, c, fe = unique_edges(faces, verts.shape[0], torch.zeros(faces.shape[0], dtype=torch.bool, device=DEV))
    assert e.shape == (0, 2) and c.shape == (0,) and bool((fe == -1).all())
    # F = 0: E = 0 without a launch
    e, c, fe = unique_edges(torch.zeros((0, 3), dtype=torch.int64, device=DEV), 5)
    assert e.shape == (0, 2) and c.shape == (0,) and fe.shape == (0, 3)
    nv, nf, _ = subdivide_meshes(verts, torch.zeros((0, 3), dtype=torch.int64, device=DEV), None, None)
    assert torch.equal(nv, verts) and nf.shape == (0, 3)


@pytest.mark.parametrize("name", CASES)
def test_unique_edges_in_lexicographic_order(golden, name):
    """edges, counts and the per-face positions against torch.unique(sorted rows, dim=0, return_inverse, return_counts)."""
    from sings_amd.topology import unique_edges
    verts, faces, idx, _ = _case_inputs(golden, name)
    mask = None
    if idx is not None:
        mask = torch.zeros(faces.shape[0], dtype=torch.bool, device=DEV)
        mask[idx] = True
    e, c, fe = unique_edges(faces, verts.shape[0], mask)
    assert e.dtype == c.dtype == fe.dtype == torch.int32
    we, wc, wfe = _edges_by_torch(faces, mask)
    assert np.array_equal(e.cpu().numpy(), we) and np.array_equal(c.cpu().numpy(), wc)
    fe = fe.cpu().numpy()
    if mask is None:
        assert np.array_equal(fe, wfe)
    else:
        mk = mask.cpu().numpy()
        assert np.array_equal(fe[mk], wfe) and (fe[~mk] == -1).all()
    if name == "pole":                                            # the long row: vertex 0 is the smaller endpoint of 80 edges, 160 instances
        assert int((e[:, 0] == 0).sum()) == 80 and np.array_equal(e[:80, 1].cpu().numpy(), np.arange(1, 81))
    if name == "big":                                             # past one 1024-entry scan block, rows on both sides of it in use
        assert int(e[:, 0].min()) < 1024 <= int(e[:, 0].max()) and verts.shape[0] == 1106


def test_edge_counts_closed_boundary_and_nonmanifold():
    from sings_amd.topology import unique_edges
    v, f, _ = bumpy_sphere(8, 5)
    V = len(v)
    faces = torch.from_numpy(f).to(DEV)
    e, c, _ = unique_edges(faces, V)
    assert e.shape[0] == 3 * len(f) // 2 and bool((c == 2).all())                 # closed: every edge in two faces
    # a band of faces removed: its rim edges are boundary edges
    keep = np.ones(len(f), bool); keep[16:32] = False
    e2, c2, _ = unique_edges(torch.from_numpy(f[keep]).to(DEV), V)
    we, wc, _ = _edges_by_torch(torch.from_numpy(f[keep]))
    assert np.array_equal(e2.cpu().numpy(), we) and np.array_equal(c2.cpu().numpy(), wc)
    assert set(np.unique(wc)) == {1, 2} and int((c2 == 1).sum()) == int((wc == 1).sum()) > 0
    # one extra face glued onto an existing edge (a new apex vertex): that edge is held by three faces
    a, b = int(f[40, 0]), int(f[40, 1])
    glued = np.concatenate([f, [[b, a, V]]])
    e3, c3, fe3 = unique_edges(torch.from_numpy(glued).to(DEV), V + 1)
    at = int(fe3[-1, 0])
    assert sorted(e3[at].tolist()) == sorted([a, b]) and int(c3[at]) == 3
    assert int((c3 == 3).sum()) == 1 and int((c3 == 1).sum()) == 2 and e3.shape[0] == e.shape[0] + 2


def test_orientation_does_not_change_the_edges(golden):
    """Case 6: per-face cyclic shifts and flips leave the edge list as it was; the children follow the corner pattern."""
    from sings_amd.topology import subdivide_meshes, unique_edges
    verts, f0, idx, _ = _case_inputs(golden, "s1_five")
    _, f1, idx1, _ = _case_inputs(golden, "flip")
    assert torch.equal(idx, idx1) and not torch.equal(f0, f1)
    assert torch.equal(torch.sort(f0, dim=1)[0], torch.sort(f1, dim=1)[0])
    V = verts.shape[0]
    for mask in (None, idx):
        m = None
        if mask is not None:
            m = torch.zeros(f0.shape[0], dtype=torch.bool, device=DEV); m[mask] = True
        (e0, c0, _), (e1, c1, fe1) = unique_edges(f0, V, m), unique_edges(f1, V, m)
        assert torch.equal(e0, e1) and torch.equal(c0, c1)
    _, nf, _ = subdivide_meshes(verts, f1, idx, None)
    kids = nf[f1.shape[0] - len(idx):].reshape(len(idx), 4, 3)
    sel = f1[torch.sort(idx)[0]]
    mid = V + fe1[torch.sort(idx)[0]].long()
    v0, v1, v2 = sel[:, 0], sel[:, 1], sel[:, 2]
    m0, m1, m2 = mid[:, 0], mid[:, 1], mid[:, 2]
    want = torch.stack([torch.stack([v0, m0, m2], 1), torch.stack([m0, v1, m1], 1), torch.stack([m2, m1, v2], 1),
                        torch.stack([m0, m1, m2], 1)], 1)
    assert torch.equal(kids, want)
    # m_k is the midpoint of edge k = (v_k, v_k+1)
    for k, (p, q) in enumerate(((v0, v1), (v1, v2), (v2, v0))):
        ek = e1[fe1[torch.sort(idx)[0]][:, k].long()].long()
        assert torch.equal(ek[:, 0], torch.minimum(p, q)) and torch.equal(ek[:, 1], torch.maximum(p, q))


@pytest.mark.parametrize("width", [1, 3, 24, 55])
def test_midpoint_rows_of_any_width(golden, width):
    """Case 7 on the larger mesh: fp32 rows of 1, 3, 24 (vector path) and 55 floats, and int32 labels, against torch gathers."""
    from sings_amd import _marshal
    from sings_amd.topology import unique_edges
    verts, faces, _, _ = _case_inputs(golden, "big")
    V = verts.shape[0]
    e, _, _ = unique_edges(faces, V)
    torch.manual_seed(width)
    src = torch.randn(V, width, device=DEV)
    got = _marshal.mesh_midpoints(e, src)
    el = e.long()
    want = src[el].mean(dim=1)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got), _bits((src[el[:, 0]] + src[el[:, 1]]) * 0.5))
    lab = torch.randint(-5, 100, (V, width), dtype=torch.int32, device=DEV)
    assert torch.equal(_marshal.mesh_midpoints(e, lab), lab[el[:, 0]])
    # a misaligned base (a view that starts one row in): the scalar path, same values
    if width % 4 == 0:
        off = torch.randn(V * width + 1, device=DEV)[1:].view(V, width)
        assert off.data_ptr() % 16 != 0
        assert np.array_equal(_bits(_marshal.mesh_midpoints(e, off)), _bits((off[el[:, 0]] + off[el[:, 1]]) * 0.5))


def test_the_same_call_twice_gives_the_same_bits(golden):
    """What frame-parallel ranks rely on: no output depends on the order atomics land in."""
    from sings_amd.topology import subdivide_meshes, unique_edges
    for name in ("big", "pole", "again"):
        verts, faces, idx, attrs = _case_inputs(golden, name)
        runs = []
        for _ in range(2):
            nv, nf, na = subdivide_meshes(verts, faces, idx, attrs)
            e, c, fe = unique_edges(nf, nv.shape[0])
            runs.append([nv, nf, e, c, fe] + [na[k] for k in sorted(na)])
        for a, b in zip(*runs):
            assert np.array_equal(_bits(a), _bits(b))


def test_refusals(golden):
    from sings_amd import _lib, _marshal
    from sings_amd.topology import subdivide_meshes, unique_edges
    verts, faces, idx, attrs = _case_inputs(golden, "s1_five")
    V = verts.shape[0]
    for bad_value in (V, V + 7, -1, 2 ** 40 + 3):                 # at, past, below; an int64 that would alias index 3 in 32 bits
        bad = faces.clone(); bad[11, 2] = bad_value
        with pytest.raises(IndexError, match="outside"):
            unique_edges(bad, V)
        with pytest.raises(IndexError, match="outside"):
            subdivide_meshes(verts, bad, idx, None)                # (face 11 is not selected: every face is checked)
    with pytest.raises(IndexError, match="outside"):
        unique_edges(faces, 0)                                      # faces without vertices
    for call in (lambda: unique_edges(faces.cpu(), V), lambda: subdivide_meshes(verts.cpu(), faces, idx, None),
                 lambda: subdivide_meshes(verts, faces, idx.cpu(), None), lambda: subdivide_meshes(verts, faces.cpu(), idx, None),
                 lambda: subdivide_meshes(verts, faces, idx, {"lbs_weights": attrs["lbs_weights"].cpu()}),
                 lambda: unique_edges(faces, V, torch.ones(faces.shape[0], dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        unique_edges(faces[:, :2], V)
    # sizes the launches cannot serve: refused by the library with an error code, before anything is launched
    lib = _lib.load()
    assert lib.sg_mesh_ws_bytes(2 ** 30 + 1, 10) == 0 and lib.sg_mesh_ws_bytes(10, 2 ** 31 // 3 + 1) == 0
    assert lib.sg_mesh_ws_bytes(34, 64) > 0
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    f32 = faces.to(torch.int32)
    ws = torch.empty(int(lib.sg_mesh_ws_bytes(V, f32.shape[0])), dtype=torch.uint8, device=DEV)
    P = _marshal._ptr
    assert lib.sg_mesh_edges_build(2 ** 30 + 1, 64, P(f32), None, P(ws), P(info), None) != 0 and b"2^30" in lib.sg_last_error()
    # V + E >= 2^31: E is the caller's word here, refused before a launch
    assert lib.sg_mesh_edges_emit(2 ** 30, 2 ** 29, 2 ** 30, P(f32), None, P(ws), P(ws), P(ws), P(ws), None) != 0
    assert b"2^31" in lib.sg_last_error()
    assert lib.sg_mesh_subdivide(V, 64, 65, P(f32), None, P(ws), P(ws), P(ws), None) != 0
    assert lib.sg_mesh_midpoints(V, 4, 0, P(f32), P(verts), P(verts), None) != 0
    torch.cuda.synchronize()
