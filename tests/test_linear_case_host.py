"""The case list of tests/test_gpu_linear_shapes.py tests what it claims (no GPU): tests/linear_case.CASES reaches every
instantiation the host dispatch of sings_amd/csrc/sg_linear.hip can choose for 1 <= Cin, Cout <= 128, the N edges of every round
size, four rounds per persistent workgroup in the long cases; the fp64 reference is torch.nn.functional's and autograd's, not a
private formula; the guarded buffers are what they say.

If the first test fails after a change to the dispatch in sg_linear.hip: restate the change in linear_case.dispatch_class and
revisit the case list -- the new instantiation has no case yet."""
import torch
import torch.nn.functional as F

import linear_case as lc


def _reachable():
    """Every (direction, class) the dispatch can choose below the size guard, by brute force over all 128 x 128 widths, the four
    activations and the flags the dispatch looks at (N does not move the class below the guard)."""
    full = set()
    N = 100
    for Cin in range(1, 129):
        for Cout in range(1, 129):
            for act in lc.ACTS:
                for ro in ((False, True) if act == lc.ACT_SIGMOID else (False,)):
                    for aux in (False, True):
                        full.add(("fwd", lc.dispatch_class("fwd", N, Cin, Cout, act, ro, aux)))
                    full.add(("bwd", lc.dispatch_class("bwd", N, Cin, Cout, act, ro, False)))
                    full.add(("acc", lc.dispatch_class("acc", N, Cin, Cout, act, ro, False)))
    for Cin in (32, 64, 96, 128):
        for Cout in range(4, 129, 4):
            for c0 in range(17):
                for c1 in range(17 - c0):
                    full.add(("fan", lc.dispatch_class("fan", N, Cin, Cout, 0, False, False, (c0, c1))))
    return {(d, cls) for d, cls in full if cls is not None}


def test_cases_reach_every_dispatch_class():
    full = _reachable()
    got = {(c[0], lc.class_of(c)) for c in lc.CASES}
    assert None not in {cls for _, cls in got}, "a case the C ABI refuses"
    assert got == full, (sorted(full - got), sorted(got - full))
    # 6 NQ x 2 VEC x 4 TO for each of narrow forward / backward, wide forward / backward / accumulate; 6 Cout x 2 L skinny;
    # 4 NQ x 2 EXQ x 4 TO fan
    assert len(full) == 5 * 48 + 12 + 32
    kernels = {(d, cls[0]) for d, cls in got}
    assert kernels == {("fwd", "skinny"), ("fwd", "narrow"), ("fwd", "wide"), ("bwd", "narrow"), ("bwd", "wide"), ("acc", "wide"),
                       ("fan", "fan")}


def test_dispatch_class_geometry():
    """Spot values read off sg_linear.hip by hand: sgl_point_tiles, sgl_wide_cfg::PTCAP, the NQ classes, the refusals."""
    assert [lc.nq_class(c) for c in (1, 8, 9, 32, 33, 48, 49, 64, 65, 96, 97, 128)] == [1, 1, 4, 4, 6, 6, 8, 8, 12, 12, 16, 16]
    assert [lc.narrow_point_tiles(1, 8 * q) for q in (1, 4, 6, 8, 12, 16)] == [4, 2, 2, 2, 1, 1]
    assert [lc.narrow_point_tiles(2, 8 * q) for q in (1, 4, 6, 8, 12, 16)] == [2, 2, 2, 2, 1, 1]
    assert [lc.wide_point_tiles(1, q) for q in (1, 4, 6, 7, 8, 9, 12, 13, 16, 18)] == [4, 4, 4, 2, 2, 2, 2, 1, 1, 1]
    assert lc.dispatch_class("fwd", 100, 128, 128, 1, False, True) == ("wide", 16, 0, True, 4, 1, True)
    assert lc.dispatch_class("fwd", 100, 33, 32, 1, False, True) == ("wide", 6, 0, False, 1, 4, False)
    assert lc.dispatch_class("fwd", 100, 64, 32, 2, True, False) == ("narrow", 8, 0, True, 1, 2, True)
    assert lc.dispatch_class("fwd", 100, 64, 3, 0, False, False) == ("skinny", 8, 0, True, 3, 8, True)
    assert lc.dispatch_class("fwd", 100, 64, 3, 0, False, True)[0] == "narrow"
    assert lc.dispatch_class("bwd", 100, 64, 48, 0, False, False) == ("wide", 6, 0, True, 2, 2, False)
    assert lc.dispatch_class("bwd", 100, 65, 100, 3, False, False) == ("narrow", 16, 0, True, 3, 1, False)
    assert lc.dispatch_class("fan", 100, 128, 128, 1, False, False, (3, 6)) == ("fan", 16, 2, True, 4, 1, False)
    assert lc.dispatch_class("fan", 100, 32, 20, 0, False, False, (1, 0)) == ("fan", 6, 1, True, 1, 2, False)
    for refused in (lc.dispatch_class("acc", 100, 48, 64, 0, False, False), lc.dispatch_class("acc", 100, 64, 64, 2, True, False),
                    lc.dispatch_class("fan", 100, 64, 50, 0, False, False, (1, 0)), lc.dispatch_class("fan", 100, 64, 48, 0, False, False, (9, 8)),
                    lc.dispatch_class("fan", 100, 64, 48, 0, False, False, (0, 0)), lc.dispatch_class("fwd", 100, 129, 4, 0, False, False)):
        assert refused is None
    # the size guard sends a wide shape to the narrow kernel; no case crosses it by accident
    assert lc.dispatch_class("fwd", 5_000_000, 128, 128, 1, False, True)[0] == "narrow"
    for c in lc.CASES:
        assert lc.size_guard(c[1], 144), c


def test_cases_cover_what_the_class_tuple_does_not_hold():
    seen = set()
    for c in lc.CASES:
        d, N, Cin, Cout, act, _ = c
        o, cls = lc.opts_of(c), lc.class_of(c)
        seen.add((d, cls[0], "act", act))
        if act == lc.ACT_SIGMOID:
            seen.add((d, cls[0], "row_offset", o["row_offset"]))
        if d == "fwd":
            seen.add((cls[0], "bias", o["bias"]))
            if cls[0] != "skinny":
                seen.add((cls[0], "aux_out", o["aux_out"], act))
            if cls[0] == "narrow" and Cout % 32 == 0:
                seen.add(("narrow", "Cout", Cout))
            if cls[0] == "wide" and not cls[3] and act == lc.ACT_GELU:
                seen.add("wide element loads with the GELU epilogue")
        elif d in ("bwd", "acc"):
            seen.add((d, cls[0], "dz_out", o["dz_out"], act != 0))
        else:
            (c0, a0), (c1, a1) = o["heads"]
            seen.add(("fan", "slots", c0 > 0, c1 > 0))
            seen.add(("fan", "columns", c0 + c1))
            seen.update(("fan", "head act", a) for cc, a in o["heads"] if cc)
            seen.add(("fan", "main Cout", Cout))
            seen.add(("fan", "Cin", Cin))
    for kernel in ("narrow", "wide"):
        for act in lc.ACTS:
            assert ("fwd", kernel, "act", act) in seen and ("bwd", kernel, "act", act) in seen
            assert (kernel, "aux_out", False, act) in seen and (kernel, "aux_out", True, act) in seen
        assert (kernel, "bias", False) in seen and (kernel, "bias", True) in seen
        assert ("bwd", kernel, "dz_out", False, True) in seen and ("bwd", kernel, "dz_out", True, True) in seen
    assert all(("acc", "wide", "act", act) in seen for act in lc.ACTS) and ("acc", "wide", "dz_out", False, True) in seen
    for ro in (False, True):
        assert ("fwd", "narrow", "row_offset", ro) in seen and ("fwd", "skinny", "row_offset", ro) in seen
        assert ("bwd", "narrow", "row_offset", ro) in seen
    assert all(("narrow", "Cout", c) in seen for c in (32, 64, 96, 128))
    assert "wide element loads with the GELU epilogue" in seen
    assert all(("fwd", "skinny", "act", a) in seen for a in (0, 2)) and all(("skinny", "bias", b) in seen for b in (False, True))
    assert {s[2:] for s in seen if s[:2] == ("fan", "slots")} == {(True, False), (False, True), (True, True)}
    assert {s[2] for s in seen if s[:2] == ("fan", "columns")} == set(range(1, 17))
    assert {s[2] for s in seen if s[:2] == ("fan", "head act")} == {0, 2}
    assert {s[2] for s in seen if s[:2] == ("fan", "Cin")} == {32, 64, 96, 128}
    assert {lc.nq_class(s[2]) for s in seen if s[:2] == ("fan", "main Cout")} >= {1, 6, 8, 12, 16}
    assert ("fan", "fan", "act", 0) in seen and ("fan", "fan", "act", 1) in seen
    # TO = 1..4 in both tile kernels, forward
    for kernel in ("narrow", "wide"):
        assert {lc.class_of(c)[4] for c in lc.CASES if c[0] == "fwd" and lc.class_of(c)[0] == kernel} == {1, 2, 3, 4}


def test_every_round_size_has_its_edges():
    """N = R - 1, R, R + 1 (and 1, 2 R + 1) for every (direction, kernel, R); the skinny kernel: one wave's round."""
    by = {}
    for c in lc.CASES:
        cls = lc.class_of(c)
        by.setdefault((c[0], cls[0], lc.rows_per_round(cls)), set()).add(c[1])
    assert {k[2] for k in by if k[1] in ("narrow", "wide")} == {32, 64, 128} and {k[2] for k in by if k[1] == "fan"} == {32, 64}
    assert {k[2] for k in by if k[1] == "skinny"} == {16, 32}
    for (d, kernel, R), ns in by.items():
        assert {1, R - 1, R, R + 1} <= ns, (d, kernel, R)
        if kernel != "skinny":
            assert 2 * R + 1 in ns, (d, kernel, R)
    # ... and for every single class, not only every round size
    per_class = {}
    for c in lc.CASES:
        per_class.setdefault((c[0], lc.class_of(c)), set()).add(c[1])
    for (d, cls), ns in per_class.items():
        R = lc.rows_per_round(cls)
        assert {R - 1, R, R + 1} <= ns, (d, cls)


def test_long_cases_run_four_rounds_per_workgroup():
    longs = [c for c in lc.CASES if lc.opts_of(c)["long"]]
    seen = set()
    for c in longs:
        cls = lc.class_of(c)
        R, cap = lc.rows_per_round(cls), lc.grid_cap(cls)
        assert c[1] % 2 == 1, c
        if cls[0] == "skinny":
            rows_per_wg = 4 * R                                  # four waves
            assert c[1] > 2048 * 256 and c[1] > cap * rows_per_wg, c     # the grid-stride loop runs more than once
        else:
            assert c[1] >= 4 * cap * R + 1, c
            assert -(-c[1] // R) >= 4 * cap                      # tiles per workgroup
        seen.add((cls[0], R))
    assert seen >= {("wide", 32), ("wide", 64), ("wide", 128), ("narrow", 32), ("narrow", 64), ("narrow", 128), ("fan", 32),
                    ("skinny", 16), ("skinny", 32)}
    assert len(longs) <= 12 and all(c[1] < 600_000 for c in longs)
    assert all(c[1] <= 2 * 128 + 1 for c in lc.CASES if not lc.opts_of(c)["long"])


def test_reference_is_torch_functional_and_autograd():
    torch.manual_seed(0)
    z = torch.randn(500, dtype=torch.float64) * 3
    assert torch.allclose(lc.act_forward(lc.ACT_GELU, z), F.gelu(z), rtol=1e-13, atol=1e-15)
    assert torch.allclose(lc.act_forward(lc.ACT_SOFTPLUS, z), F.softplus(z), rtol=1e-13, atol=1e-15)
    ro = torch.randn(500, dtype=torch.float64)
    assert torch.allclose(lc.act_forward(lc.ACT_SIGMOID, z[:, None], ro)[:, 0], torch.sigmoid(z + ro), rtol=1e-13, atol=1e-15)
    zz = z.clone().requires_grad_(True)
    F.gelu(zz).sum().backward()
    assert torch.allclose(lc.gelu_grad(z), zz.grad, rtol=1e-13, atol=1e-15)
    # three whole cases: forward values, then the backward of the same layer fed the forward's aux, against autograd
    picks = [("fwd", 33, 47, 65, lc.ACT_GELU, dict()), ("fwd", 65, 64, 1, lc.ACT_SIGMOID, dict(row_offset=True)),
             ("fwd", 17, 20, 33, lc.ACT_SOFTPLUS, dict(bias=False))]
    for case in picks:
        _, N, Cin, Cout, act, _ = case
        t = lc.make_tensors(case)
        ref = lc.reference(case, t)
        x = t["x"].double().requires_grad_(True)
        W = t["W"].double().requires_grad_(True)
        zt = F.linear(x, W, None if t["bias"] is None else t["bias"].double())
        if act == lc.ACT_GELU:
            h = F.gelu(zt)
        elif act == lc.ACT_SIGMOID:
            h = torch.sigmoid(zt + t["row_offset"].double()[:, None])
        else:
            h = F.softplus(zt)
        assert torch.allclose(ref["h"], h.detach(), rtol=1e-12, atol=1e-14)
        dh = torch.randn(N, Cout, dtype=torch.float64)
        (h * dh).sum().backward(retain_graph=True)
        aux = ref["h"] if act == lc.ACT_SIGMOID else ref["aux"]
        back = lc.reference_backward(act, dh, aux, t["W"])
        assert torch.allclose(back["dx"], x.grad, rtol=1e-11, atol=1e-13)
        assert torch.allclose(back["dz"].T @ t["x"].double(), W.grad, rtol=1e-11, atol=1e-12)
        # a head beside it (the fan) and an old gradient (accumulate) add what autograd adds
        Wh = torch.randn(3, Cin, dtype=torch.float64)
        hh = torch.sigmoid(F.linear(x, Wh))
        dhh = torch.randn(N, 3, dtype=torch.float64)
        x.grad = None
        ((h * dh).sum() + (hh * dhh).sum()).backward()
        old = torch.randn(N, Cin, dtype=torch.float64)
        fan = lc.reference_backward(act, dh, aux, t["W"], heads=[None, dict(c=3, act=2, dh=dhh, aux=hh.detach(), W=Wh)], old=old)
        assert torch.allclose(fan["dx"], old + x.grad, rtol=1e-11, atol=1e-13)


def test_tensors_are_reproducible_and_fp32():
    case = next(c for c in lc.CASES if c[0] == "fan" and lc.opts_of(c)["heads"][1][0])
    a, b = lc.make_tensors(case), lc.make_tensors(case)
    assert torch.equal(a["dh"], b["dh"]) and torch.equal(a["heads"][1]["W"], b["heads"][1]["W"]) and a["dh"].dtype == torch.float32
    ref = lc.reference(case, a)
    assert ref["dx"].dtype == torch.float64 and ref["dx"].shape == (case[1], case[2])


def test_guarded_and_poisoned_buffers():
    dev = torch.device("cpu")
    for shape in ((1, 1), (33, 7), (257, 128), (5,)):
        view, flat = lc.guarded(shape, dev)
        assert view.data_ptr() % 16 == 0 and view.shape == shape and view.dtype == torch.float32
        assert flat.numel() == lc.GUARD_FRONT + view.numel() + lc.GUARD_ROWS * shape[-1]
        assert torch.isnan(view).all() and lc.guard_intact(view, flat)
        view.copy_(torch.randn(*shape))
        view += 1.0
        assert lc.guard_intact(view, flat) and torch.isfinite(view).all()
        flat[lc.GUARD_FRONT + view.numel()] = 0                  # one word behind the view
        assert not lc.guard_intact(view, flat)
        view, flat = lc.guarded(shape, dev)
        flat[lc.GUARD_FRONT - 1] = 0                             # one word in front of it
        assert not lc.guard_intact(view, flat)
        view, flat = lc.guarded(shape, dev, stale=lc.STALE)
        assert torch.isfinite(view).all() and lc.guard_intact(view, flat)
    a = torch.randn(33, 7)
    p = lc.poisoned(a, dev)
    assert torch.equal(p, a) and p.data_ptr() % 16 == 0
    whole = torch.as_strided(p, (33 + lc.POISON_ROWS, 7), (7, 1))
    assert torch.isnan(whole[33:]).all()
    assert lc.fraction_of_bound(a, a.double(), 2e-5, 2e-6) == 0.0
    assert lc.fraction_of_bound(torch.full((2,), float("nan")), torch.ones(2), 2e-5, 2e-6) == float("inf")
    b = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert abs(lc.fraction_of_bound(b + 2.4e-5, b, 2e-5, 2e-6) - 1.0) < 1e-6
