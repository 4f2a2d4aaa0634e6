"""The fused mesh terms (sings_amd/mesh_terms.py, csrc/sg_mesh_terms.hip, include/sings_mesh_terms.h) on the GPU: the device build against the
host build as integers, each term against the reference's golden values (tests/golden/reg_golden.npz), the composition against an fp64
torch statement written here, exact zeros at zero weights, the device weights under graph replay, the stale-holder refusal.

Tolerances are test_gpu_reg.py's: a loss 2e-6 relative, a gradient 1e-5 |ref| + 5e-6 max|ref| (fp32 sums in another order).  The fp64
statement below against its own fp32 form sits at 6e-8 and 2e-7 on the CPU, thirty times inside these."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mesh_case import bumpy_sphere

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reg_golden.npz"))
DEV = torch.device("cuda:0")
F32 = np.float32


def _close(a, b, rtol=1e-5, atol_scale=5e-6):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b)
    assert (err <= rtol * np.abs(b) + atol_scale * scale).all(), (err.max(), scale)


def _loss_close(got, want):
    got = got.detach() if torch.is_tensor(got) else got
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want)), (float(got), float(want))


def _edges_of(faces):
    return np.unique(np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)          # a < b, lexicographic, unique


def _mesh(edges, labels):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    return SimpleNamespace(edges=t(np.asarray(edges).reshape(-1, 2), torch.int32), vertex_label=t(labels, torch.int32), num_verts=len(labels))


def _sphere(nu, nv, relabel=False):
    v, f, lab = bumpy_sphere(nu, nv)
    lab = lab.copy()
    if relabel:
        lab[nu + 3] = 9                                  # a label nobody shares (degree 0); label 8 stays unused
    return v, _edges_of(f), lab


def _module(w_pos, w_col, **kw):
    from sings_amd.mesh_terms import MeshTerms
    return MeshTerms(w_pos, w_col, kw.pop("mesh_edge_w", 1.0), 1000.0, 10.0, 1000, **kw)


def _tables(L, seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, L).astype(F32), rng.uniform(0.5, 2.0, L).astype(F32)


def _host_build(V, edges, lab, tables):
    """What sg_mesh_terms_build must give: ``regularizers._csr`` of the same-label edges, and the fp32 statement of the rest."""
    from sings_amd.regularizers import _csr
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    same = lab[e[:, 0]] == lab[e[:, 1]]
    row_ptr, col = _csr(V, e[same])
    deg = np.diff(row_ptr)
    with np.errstate(divide="ignore"):
        deg_inv = np.where(deg > 0, F32(1.0) / deg.astype(F32), F32(0.0)).astype(F32)
    L = len(tables[0])
    count = np.bincount(lab, minlength=L).astype(np.int32)
    den = count[lab].astype(F32) * F32(3.0)
    vscale = np.stack([t[lab] / den for t in tables], axis=1).astype(F32)
    return row_ptr, col, deg_inv, count, vscale, int(same.sum())


def _hand_table(L):
    h = np.zeros(L, F32)
    h[[6, 7]] = 1000.0
    return h


def _cases():
    yield "golden", G["mesh_verts"], np.asarray(G["mesh_edges"]), G["mesh_labels"], 15
    v, e, lab = _sphere(80, 4)
    yield "sphere", v, e, lab, 8
    v, e, lab = _sphere(80, 4, relabel=True)
    yield "relabelled", v, e, lab, 10
    yield "no_edges", v, np.zeros((0, 2), np.int64), lab, 10


def test_the_sphere_is_the_case_the_build_needs():
    v, e, lab = _sphere(80, 4)
    assert v.shape == (242, 3) and e.shape == (720, 2) and int((lab[e[:, 0]] == lab[e[:, 1]]).sum()) == 540
    assert np.bincount(e.ravel()).max() == 80                                       # the poles: more neighbours than a wave has lanes
    same = e[lab[e[:, 0]] == lab[e[:, 1]]]
    assert (np.bincount(same.ravel(), minlength=242) > 0).all()                     # every vertex has a same-label edge
    ge = np.asarray(G["mesh_edges"])                                                # the golden list is in MeshState.edges' form already
    assert np.array_equal(np.unique(np.sort(ge, axis=1), axis=0), ge)


@pytest.mark.parametrize("case", ["golden", "sphere", "relabelled", "no_edges"])
def test_device_build_equals_the_host_build_as_integers(case):
    name, v, e, lab, L = next(c for c in _cases() if c[0] == case)
    V = len(lab)
    wp, wc = _tables(L)
    mod = _module(wp, wc)
    assert mod.L == L
    verts = torch.from_numpy(v).to(DEV)
    mod.reset(_mesh(e, lab), torch.zeros_like(verts), verts)
    row_ptr, col, deg_inv, count, vscale, n_same = _host_build(V, e, lab, (wp, wc, _hand_table(L)))
    assert mod.V == V and mod.E == len(e) and mod.nnz == 2 * n_same == int(row_ptr[-1])
    got = lambda t: t.cpu().numpy()
    assert np.array_equal(got(mod.row_ptr), row_ptr) and np.array_equal(got(mod.col)[:mod.nnz], col)
    assert mod.col.shape[0] == max(2 * len(e), 1)                                   # the upper bound: no size was read to allocate it
    for a, b in ((mod.deg_inv, deg_inv), (mod.vscale, vscale)):
        assert np.array_equal(got(a).view(np.uint32), b.view(np.uint32))
    assert np.array_equal(got(mod.count), count)
    if case == "relabelled":
        iso = int(np.nonzero(lab == 9)[0][0])
        assert count[8] == 0 and count[9] == 1 and row_ptr[iso] == row_ptr[iso + 1] and float(mod.deg_inv[iso]) == 0.0
    if case == "no_edges":
        assert mod.nnz == 0 and float(mod.deg_inv.abs().max()) == 0.0 and float(mod.mesh_edge) == 0.0
    else:
        from oracle import reg_oracle as ro
        _loss_close(mod.mesh_edge, float(ro.mesh_edge_loss(torch.from_numpy(v).double(), torch.from_numpy(e))))
    first = [got(t).copy() for t in (mod.row_ptr, mod.col[:mod.nnz], mod.deg_inv, mod.count, mod.vscale)]
    mod.reset(_mesh(e, lab), torch.zeros_like(verts), verts)                        # two builds: the same bits
    for a, t in zip(first, (mod.row_ptr, mod.col[:mod.nnz], mod.deg_inv, mod.count, mod.vscale)):
        assert np.array_equal(a.view(np.uint32), got(t).view(np.uint32))


def test_bad_rows_are_flagged_not_dereferenced():
    v, e, lab = _sphere(12, 8)
    verts = torch.from_numpy(v).to(DEV)
    wp, wc = _tables(8)
    mod = _module(wp, wc)
    for row in ((5, 5), (7, 3), (-1, 4), (3, len(lab))):
        with pytest.raises(ValueError, match="edge row"):
            mod.reset(_mesh(np.concatenate([e, np.array([row])]), lab), torch.zeros_like(verts), verts)
    for bad in (8, -1):
        lab2 = lab.copy(); lab2[11] = bad
        with pytest.raises(ValueError, match="label outside"):
            mod.reset(_mesh(e, lab2), torch.zeros_like(verts), verts)
    mod.reset(_mesh(e, lab), torch.zeros_like(verts), verts)                        # and the module is usable afterwards
    assert mod.V == len(lab)


def _golden_module():
    mod = _module(G["lap_pos_w"], G["lap_col_w"])
    verts = torch.from_numpy(G["mesh_verts"]).to(DEV)
    mod.reset(_mesh(G["mesh_edges"], G["mesh_labels"]), torch.zeros_like(verts), verts)
    return mod


@pytest.mark.parametrize("term,w3,key,scale", [("region_mesh_lap", (1.0, 0.0, 0.0), "lap_pos", 1.0),
                                               ("region_mesh_lap_color", (0.0, 1.0, 0.0), "lap_col", 1.0),
                                               ("hand_lap", (0.0, 0.0, 1e-5), "lap_hands", 1e-5)])
def test_each_term_against_the_reference_golden(term, w3, key, scale):
    """normals = 0: the anchor is xyz_canon, and each weight vector leaves one of the reference's three losses (loss_items.py:172-192 run
    by the reference itself).  The colour goes in as column 0 of a [V,16,3] tensor: the row stride of 48 floats is exercised."""
    mod = _golden_module()
    t = lambda k: torch.from_numpy(G[k]).to(DEV)
    V = mod.V
    rng = torch.Generator().manual_seed(3)
    xyz = t("lap_pos_x").requires_grad_(True)
    scales = torch.exp(torch.randn(V, 3, generator=rng) * 0.3 - 4.9).to(DEV).requires_grad_(True)
    shs = torch.randn(V, 16, 3, generator=rng).to(DEV)
    shs[:, 0] = t("lap_col_x")
    shs.requires_grad_(True)
    mod.set_weights(w3)
    out = mod({"xyz_canon": xyz, "scales": scales, "shs": shs})
    assert set(out) == set(mod.KEYS)
    (3.0 * (out["region_mesh_lap"] + out["region_mesh_lap_color"] + out["hand_lap"])).backward()      # upstream through autograd
    _loss_close(out[term], scale * float(G[f"{key}_loss"]))
    for other in set(mod.KEYS[:3]) - {term}:
        assert float(out[other]) == 0.0
    grad = (shs.grad[:, 0] if term == "region_mesh_lap_color" else xyz.grad).cpu().numpy() / 3.0
    _close(grad, scale * G[f"{key}_grad"].astype(np.float64))
    assert float(shs.grad[:, 1:].abs().max()) == 0.0 and float(scales.grad.abs().max()) == 0.0       # (normals = 0: no scale gradient)
    if term != "region_mesh_lap_color":
        assert float(shs.grad.abs().max()) == 0.0
    _close(mod.last_grads["shs_dc" if term == "region_mesh_lap_color" else "xyz_canon"].cpu().numpy(), scale * G[f"{key}_grad"].astype(np.float64))


def _statement(xyz, scales, normals, colour, e, lab, tables, w3):
    """The three terms in fp64 torch: L = D^-1 A - I over the same-label edges (a row without one: -I), term = sum_i w[l_i] / (count[l_i] 3)
    |(L x)_i|^2, the position term on the anchor xyz + mean(scales) n / 2."""
    V = len(lab)
    same = e[lab[e[:, 0]] == lab[e[:, 1]]]
    A = torch.zeros((V, V), dtype=torch.float64)
    A[same[:, 0], same[:, 1]] = 1.0
    A[same[:, 1], same[:, 0]] = 1.0
    deg = A.sum(1)
    Lm = A * torch.where(deg > 0, 1.0 / deg.clamp_min(1.0), torch.zeros_like(deg)).unsqueeze(1) - torch.eye(V, dtype=torch.float64)
    count = np.bincount(lab, minlength=len(tables[0])).astype(np.float64)
    vs = [torch.from_numpy(t.astype(np.float64)[lab] / (count[lab] * 3.0)) for t in tables]
    term = lambda x, s: (s * ((Lm @ x) ** 2).sum(1)).sum()
    anchor = xyz + scales.mean(-1, keepdim=True) * normals / 2.0
    return w3[0] * term(anchor, vs[0]), w3[1] * term(colour, vs[1]), w3[2] * term(xyz, vs[2])


@pytest.fixture(scope="module")
def composition():
    """Per mesh: the inputs, the fp64 statement's values and gradients (computed once), a module that has been reset for the mesh."""
    out = {}
    for name, (v, e, lab), L in (("sphere", _sphere(80, 4), 8), ("small", _sphere(12, 8), 8), ("relabelled", _sphere(80, 4, True), 10)):
        V = len(lab)
        rng = torch.Generator().manual_seed(11)
        n = torch.randn(V, 3, generator=rng, dtype=torch.float64)
        ins = dict(xyz=torch.from_numpy(v) + 0.01 * torch.randn(V, 3, generator=rng), normals=(n / n.norm(dim=1, keepdim=True)).float(),
                   scales=torch.exp(torch.randn(V, 3, generator=rng) * 0.3 - 4.9), shs=torch.rand(V, 16, 3, generator=rng))
        wp, wc = _tables(L)
        w3 = (700.0, 10.0, 1e-5)
        x64, s64, c64 = (ins[k].double().requires_grad_(True) for k in ("xyz", "scales", "shs"))
        vals = _statement(x64, s64, ins["normals"].double(), c64[:, 0], e, lab, (wp, wc, _hand_table(L)), w3)
        sum(vals).backward()
        mod = _module(wp, wc)
        mod.reset(_mesh(e, lab), ins["normals"].to(DEV), torch.from_numpy(v).to(DEV))
        mod.set_weights(w3)
        out[name] = dict(ins=ins, vals=[float(x) for x in vals], grads=(x64.grad.numpy(), s64.grad.numpy(), c64.grad.numpy()), mod=mod,
                         lab=lab, tables=(wp, wc))
    return out


@pytest.mark.parametrize("name", ["sphere", "small", "relabelled"])
def test_composition_against_the_fp64_statement(composition, name):
    c = composition[name]
    mod, ins = c["mod"], c["ins"]
    xyz, scales, shs = (ins[k].to(DEV).requires_grad_(True) for k in ("xyz", "scales", "shs"))
    out = mod({"xyz_canon": xyz, "scales": scales, "shs": shs})
    for k, want in zip(mod.KEYS, c["vals"]):
        print(f"{name} {k}: {float(out[k]):.9g} vs {want:.9g}")
    (out["region_mesh_lap"] + out["region_mesh_lap_color"] + out["hand_lap"] + out["mesh_edge_loss"]).backward()
    for k, want in zip(mod.KEYS, c["vals"]):
        _loss_close(out[k], want)
    gx, gs, gc = c["grads"]
    _close(xyz.grad.cpu().numpy(), gx)
    _close(scales.grad.cpu().numpy(), gs)
    _close(shs.grad.cpu().numpy(), gc)
    bits = scales.grad.contiguous().view(torch.int32)
    assert torch.equal(bits[:, 0], bits[:, 1]) and torch.equal(bits[:, 0], bits[:, 2])
    assert float(scales.grad.abs().max()) > 0
    assert not out["mesh_edge_loss"].requires_grad


def test_an_isolated_vertex_contributes_minus_x(composition):
    """Only label 9 -- one vertex, no same-label edge -- carries weight: the position term is alpha w / (1 * 3) |anchor|^2 of that vertex."""
    c = composition["relabelled"]
    lab, ins = c["lab"], c["ins"]
    iso = int(np.nonzero(lab == 9)[0][0])
    wp = np.zeros(10, F32); wp[9] = 1.5
    v, e, _ = _sphere(80, 4, True)
    mod = _module(wp, np.zeros(10, F32), hands=False)
    mod.reset(_mesh(e, lab), ins["normals"].to(DEV), torch.from_numpy(v).to(DEV))
    mod.set_weights((700.0, 10.0, 0.0))
    xyz = ins["xyz"].to(DEV).requires_grad_(True)
    out = mod({"xyz_canon": xyz, "scales": ins["scales"].to(DEV), "shs": ins["shs"].to(DEV)})
    out["region_mesh_lap"].backward()
    anchor = ins["xyz"][iso].double() + ins["scales"][iso].double().mean() * ins["normals"][iso].double() / 2.0
    _loss_close(out["region_mesh_lap"], 700.0 * 1.5 / 3.0 * float((anchor ** 2).sum()))
    want = np.zeros((len(lab), 3)); want[iso] = (2.0 * 700.0 * 1.5 / 3.0 * anchor).numpy()           # d/dx |-x|^2 = 2 x
    _close(xyz.grad.cpu().numpy(), want)
    assert float(out["region_mesh_lap_color"]) == 0.0 and float(out["hand_lap"]) == 0.0


def test_zero_weights_give_exact_zeros(composition):
    c = composition["sphere"]
    mod, ins = c["mod"], c["ins"]
    mod.set_weights((0.0, 0.0, 0.0))
    try:
        xyz, scales, shs = (ins[k].to(DEV).requires_grad_(True) for k in ("xyz", "scales", "shs"))
        out = mod({"xyz_canon": xyz, "scales": scales, "shs": shs})
        (out["region_mesh_lap"] + out["region_mesh_lap_color"] + out["hand_lap"]).backward()
        for k in mod.KEYS[:3]:
            assert float(out[k]) == 0.0
        for t in (xyz.grad, scales.grad, shs.grad, *mod.last_grads.values()):
            assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0
    finally:
        mod.set_weights((700.0, 10.0, 1e-5))


def test_device_weights_under_replay(composition):
    """One captured call, replayed after ``set_iteration`` at two iterations inside the ramp: the position value follows alpha, the other
    two keep their bits -- the weights are read from device memory at replay time."""
    from sings_amd.mesh_terms import MeshTerms
    from sings_amd.train_step import capture_step
    c = composition["sphere"]
    ins = c["ins"]
    v, e, lab = _sphere(80, 4)
    mod = MeshTerms(c["tables"][0], c["tables"][1], 1.0, 1000.0, 10.0, 1000)
    mod.reset(_mesh(e, lab), ins["normals"].to(DEV), torch.from_numpy(v).to(DEV))
    attrs = {"xyz_canon": ins["xyz"].to(DEV), "scales": ins["scales"].to(DEV), "shs": ins["shs"].to(DEV)}
    mod.set_iteration(1100)

    def call():
        mod(attrs)
        return mod.terms

    graph, terms = capture_step(call, warmup=1)
    got = []
    for t_iter in (1250, 1750):
        mod.set_iteration(t_iter)
        graph.replay()
        got.append(terms.clone().cpu().numpy())
    assert mod.weights_at(1250)[0] == 250.0 and mod.weights_at(1750)[0] == 750.0
    a, b = got
    print(f"replayed position term at alpha 250 / 750: {a[0]:.9g} / {b[0]:.9g}")
    assert a[0] > 0 and abs(float(b[0]) - 3.0 * float(a[0])) <= 2e-6 * abs(float(b[0]))
    assert np.array_equal(a[1:].view(np.uint32), b[1:].view(np.uint32)) and a[1] > 0 and a[2] > 0
    mod.set_iteration(900)                                                          # in front of the ramp: the term is switched off
    graph.replay()
    assert float(terms[0]) == 0.0 and np.array_equal(terms.cpu().numpy()[1:].view(np.uint32), a[1:].view(np.uint32))


def test_a_stale_holder_is_refused(composition):
    c = composition["small"]
    mod, ins = c["mod"], c["ins"]
    V = mod.V
    longer = lambda t: torch.cat([t, t[:1]]).to(DEV)
    good = {"xyz_canon": ins["xyz"].to(DEV), "scales": ins["scales"].to(DEV), "shs": ins["shs"].to(DEV)}
    for k, src in (("xyz_canon", "xyz"), ("scales", "scales"), ("shs", "shs")):
        bad = dict(good, **{k: longer(ins[src])})
        assert bad[k].shape[0] == V + 1
        with pytest.raises(ValueError, match=f"built for {V} vertices"):
            mod(bad)
