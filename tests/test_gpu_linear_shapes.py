"""The fused linear kernels of sings_amd/csrc/sg_linear.hip at every width class, pad and tile edge, through the C ABI: the cases
of tests/linear_case.py (tests/test_linear_case_host.py proves on a CPU that they reach every instantiation of the dispatch), each
against the fp64 reference of the same file.  Per case:

  values          every entry of h, aux, dz, dx and the heads' dz within |a - b| <= rtol |b| + atol max|b|, the pairs
                  tests/test_gpu_decode.py uses for these kernels (2e-5 / 2e-6 forward and backward, 5e-5 / 5e-6 accumulate and fan);
  nothing else    outputs live inside a larger allocation of sentinel words (64 floats in front, 256 rows behind): every guard word
  written         unchanged; accumulate starts from seeded values; a missing aux / dz array leaves the other output's bits alone;
  nothing foreign inputs (weights and bias too) are followed by 256 rows of NaN inside their own allocation: no NaN in any output;
  read            and with the LAST input row set to NaN no bit of an earlier output row changes (a padded column filled from the
                  next row meets a zero weight: only a NaN shows it);
  determinism     a second call into buffers holding other stale bytes gives the same bits.

Each test prints the worst entry of its class as a fraction of the bound.  The element-wise kernels beside them (sg_bias_act_*,
sg_scales_head_*: sg_decode.hip) get the same checks at the end of the file.

Note on the two GELU evaluations: sg_linear.hip's narrow AND wide forward epilogues both call sg_gelu_both (sg_act.h: Abramowitz-Stegun
erf, h and gelu'(z) from one evaluation); erff is what sg_bias_act_* uses.  test_the_two_gelu_paths_meet holds the two kernels to each
other anyway, and test_bias_act_* holds the erff ones to fp64.
"""
import ctypes as C

import pytest
import torch

import linear_case as lc

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _lib():
    from sings_amd import _lib as L
    return L, L.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Worst:
    """The worst fraction of the bound over a test's cases; every comparison goes through `take`, and `settle` at the end of the
    test fails it if any comparison was beyond its bound (all of them are listed, not only the first)."""

    def __init__(self):
        self.frac, self.where, self.beyond = 0.0, None, []

    def take(self, got, ref, bound, where, scale=None):
        f = lc.fraction_of_bound(got, ref, bound[0], bound[1], scale)
        if f > self.frac:
            self.frac, self.where = f, where
        if not f <= 1.0:
            self.beyond.append((round(f, 3), where))
        return f

    def settle(self, title):
        print(f"\n{title}: worst entry at {self.frac:.3f} of the bound: {self.where}")
        assert not self.beyond, (title, len(self.beyond), "comparisons beyond the bound", self.beyond[:20])


def _clean(bufs, where):
    """Guards intact and no NaN / sentinel left in any output: bufs = [(name, view, flat)]."""
    for name, view, flat in bufs:
        if view is None:
            continue
        assert lc.guard_intact(view, flat), (where, name, "a guard word was written")
        assert bool(torch.isfinite(view).all()), (where, name, "NaN: a row beyond N or an unwritten entry")


def _on(dev, t):
    return None if t is None else lc.poisoned(t, dev)


# ---- one case ----------------------------------------------------------------------------------------------------------------------
def _forward(L, lib, dev, N, Cin, Cout, act, x, W, b, ro, want_aux, stale=lc.SENTINEL):
    h, hf = lc.guarded((N, Cout), dev, stale)
    aux, af = lc.guarded((N, Cout), dev, stale) if want_aux else (None, None)
    L.check(lib.sg_linear_forward(N, Cin, Cout, act, _p(x), _p(W), _p(b), _p(ro), _p(aux), _p(h), _st(dev)), "linear forward")
    return [("h", h, hf), ("aux", aux, af)]


def _run_forward(L, lib, dev, case, worst):
    _, N, Cin, Cout, act, _ = case
    o = lc.opts_of(case)
    t = lc.make_tensors(case, dev if o["long"] else None)
    ref = lc.reference(case, t)
    x, W, b, ro = _on(dev, t["x"]), _on(dev, t["W"]), _on(dev, t["bias"]), _on(dev, t["row_offset"])
    one = _forward(L, lib, dev, N, Cin, Cout, act, x, W, b, ro, o["aux_out"])
    two = _forward(L, lib, dev, N, Cin, Cout, act, x, W, b, ro, o["aux_out"], stale=lc.STALE)
    _clean(one + two, case)
    worst.take(one[0][1], ref["h"], lc.BOUND["fwd"], (case, "h"))
    if o["aux_out"]:
        worst.take(one[1][1], ref["aux"], lc.BOUND["fwd"], (case, "aux"))
    for (name, a, _), (_, c, _) in zip(one, two):
        assert a is None or lc.same_bits(a, c), (case, name, "a second call gave other bits")
    if not o["aux_out"] and lc.dispatch_class("fwd", N, Cin, Cout, act, o["row_offset"], True) == lc.class_of(case):
        full = _forward(L, lib, dev, N, Cin, Cout, act, x, W, b, ro, True)
        _clean(full, case)
        assert lc.same_bits(full[0][1], one[0][1]), (case, "h depends on whether aux_out is given")
    if N >= 2 and not o["long"]:
        # rows are independent: a last input row of NaN changes no bit of the rows before it (the padded columns of row N - 2
        # must not be filled from row N - 1)
        bad = t["x"].clone()
        bad[N - 1] = float("nan")
        leak = _forward(L, lib, dev, N, Cin, Cout, act, _on(dev, bad), W, b, ro, o["aux_out"])
        for (name, a, _), (_, c, _) in zip(one, leak):
            assert a is None or lc.same_bits(a[:N - 1], c[:N - 1]), (case, name, "the last input row reached an earlier output row")


def _backward(L, lib, dev, d, N, Cin, Cout, act, dh, aux, W, ro, old, want_dz, heads=None, stale=lc.SENTINEL):
    dx, dxf = lc.guarded((N, Cin), dev, stale)
    if old is not None:
        dx.copy_(old)
    dz, dzf = lc.guarded((N, Cout), dev, stale) if (want_dz and act != lc.ACT_NONE) else (None, None)
    out = [("dx", dx, dxf), ("dz", dz, dzf)]
    if d == "fan":
        side = (L.SgLinearSide * 2)()
        for i, hd in enumerate(heads):
            if hd is None:
                out.append((f"head {i} dz", None, None))
                continue
            hz, hzf = lc.guarded((N, hd["c"]), dev, stale) if hd["act"] else (None, None)
            side[i].cout, side[i].act = hd["c"], hd["act"]
            side[i].aux, side[i].dh, side[i].W, side[i].dz_out = (None if hd["aux"] is None else hd["aux"].data_ptr(), hd["dh"].data_ptr(),
                                                                  hd["W"].data_ptr(), None if hz is None else hz.data_ptr())
            out.append((f"head {i} dz", hz, hzf))
        L.check(lib.sg_linear_backward_fan(N, Cin, Cout, act, _p(aux), _p(dh), _p(W), _p(dz), _p(dx), side, _st(dev)), "fan backward")
    else:
        fn = lib.sg_linear_backward_accumulate if d == "acc" else lib.sg_linear_backward
        L.check(fn(N, Cin, Cout, act, _p(aux), _p(ro), _p(dh), _p(W), _p(dz), _p(dx), _st(dev)), "linear backward")
    return out


def _heads_on(dev, heads):
    return [None if hd is None else dict(c=hd["c"], act=hd["act"], dh=_on(dev, hd["dh"]), W=_on(dev, hd["W"]), aux=_on(dev, hd["aux"]))
            for hd in heads]


def _run_backward(L, lib, dev, case, worst):
    d, N, Cin, Cout, act, _ = case
    o = lc.opts_of(case)
    t = lc.make_tensors(case, dev if o["long"] else None)
    ref = lc.reference(case, t)
    dh, aux, W, ro = _on(dev, t["dh"]), _on(dev, t["aux"]), _on(dev, t["W"]), _on(dev, t["row_offset"])
    old = None if d != "acc" else t["old"].to(dev)
    heads = _heads_on(dev, t["heads"]) if d == "fan" else None
    args = (L, lib, dev, d, N, Cin, Cout, act, dh, aux, W, ro, old)
    one = _backward(*args, o["dz_out"], heads)
    two = _backward(*args, o["dz_out"], heads, stale=lc.STALE)
    _clean(one + two, case)
    bound = lc.BOUND[d]
    worst.take(one[0][1], ref["dx"], bound, (case, "dx"))
    if one[1][1] is not None:
        worst.take(one[1][1], ref["dz"], bound, (case, "dz"))
    for (name, view, _), r in zip(one[2:], ref["head_dz"]):
        if view is not None:
            worst.take(view, r, bound, (case, name))
    for (name, a, _), (_, c, _) in zip(one, two):
        assert a is None or lc.same_bits(a, c), (case, name, "a second call gave other bits")
    if not o["dz_out"] and act != lc.ACT_NONE:
        full = _backward(*args, True, heads)
        _clean(full, case)
        assert lc.same_bits(full[0][1], one[0][1]), (case, "dx depends on whether dz_out is given")
        worst.take(full[1][1], ref["dz"], bound, (case, "dz"))
    if N >= 2 and not o["long"]:
        # rows are independent: a last row of NaN in dh changes no bit of the rows before it
        bad = t["dh"].clone()
        bad[N - 1] = float("nan")
        leak = _backward(L, lib, dev, d, N, Cin, Cout, act, _on(dev, bad), aux, W, ro, old, o["dz_out"], heads)
        for (name, a, _), (_, c, _) in zip(one, leak):
            assert a is None or lc.same_bits(a[:N - 1], c[:N - 1]), (case, name, "the last input row reached an earlier output row")
    if d == "fan":
        _fan_equals_its_parts(L, lib, dev, case, one, dh, aux, W, heads, worst)


def _fan_equals_its_parts(L, lib, dev, case, fan, dh, aux, W, heads, worst):
    """The fan against sg_linear_backward followed by one sg_linear_backward_accumulate per head; a head alone in slot 1 against
    the same head alone in slot 0, bit for bit."""
    _, N, Cin, Cout, act, _ = case
    parts = _backward(L, lib, dev, "bwd", N, Cin, Cout, act, dh, aux, W, None, None, True)
    dx = parts[0][1]
    part_dz = []
    for hd in heads:
        if hd is None:
            part_dz.append(None)
            continue
        hz, hzf = lc.guarded((N, hd["c"]), dev) if hd["act"] else (None, None)
        L.check(lib.sg_linear_backward_accumulate(N, Cin, hd["c"], hd["act"], _p(hd["aux"]), None, _p(hd["dh"]), _p(hd["W"]), _p(hz),
                                                  _p(dx), _st(dev)), "head accumulate")
        part_dz.append(hz)
        _clean([("head dz (parts)", hz, hzf)], case)
    _clean(parts, case)
    bound = lc.BOUND["fan"]
    worst.take(fan[0][1], dx.double(), bound, (case, "fan dx against its parts"))
    if fan[1][1] is not None:
        worst.take(fan[1][1], parts[1][1].double(), bound, (case, "fan dz against the plain backward"))
    for (name, view, _), pz in zip(fan[2:], part_dz):
        if view is not None:
            worst.take(view, pz.double(), bound, (case, name + " against the accumulate pass"))
    if heads[0] is None:
        swapped = _backward(L, lib, dev, "fan", N, Cin, Cout, act, dh, aux, W, None, None, True, [heads[1], None])
        _clean(swapped, case)
        assert lc.same_bits(swapped[0][1], fan[0][1]), (case, "a head alone in slot 1 differs from the same head in slot 0")
        if fan[3][1] is not None:
            assert lc.same_bits(swapped[2][1], fan[3][1]), (case, "the head's dz differs between the slots")


@pytest.mark.parametrize("direction,kernel,NQ", lc.GROUPS, ids=["-".join(map(str, g)) for g in lc.GROUPS])
def test_linear_kernels_at_every_class_and_edge(direction, kernel, NQ):
    L, lib = _lib()
    dev = _dev()
    worst = _Worst()
    cases = [c for c in lc.CASES if lc.group_of(c) == (direction, kernel, NQ)]
    assert cases
    for case in cases:
        (_run_forward if direction == "fwd" else _run_backward)(L, lib, dev, case, worst)
    worst.settle(f"{direction} {kernel} NQ={NQ}, {len(cases)} cases")


# ---- tails of the activations ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tc", lc.TAIL_CASES, ids=[t["name"] for t in lc.TAIL_CASES])
def test_activation_tails(tc):
    """A bias (or row-offset) ladder far into the tails: finite outputs within the bound of the whole output's scale, the columns
    (rows) whose ladder value is exactly zero bit-identical to the same layer without the ladder, then the backward of that layer
    fed the forward's own aux, against the fp64 chain rule from the fp64 pre-activation."""
    L, lib = _lib()
    dev = _dev()
    worst = _Worst()
    N, Cin, base, extra, act = tc["N"], tc["Cin"], tc["base"], tc["extra"], tc["act"]
    Cout = base + extra
    g = torch.Generator().manual_seed(1000 + Cout + act)
    x = torch.randn(N, Cin, generator=g)
    W = torch.randn(Cout, Cin, generator=g) * Cin ** -0.5
    dh = torch.randn(N, Cout, generator=g)
    ladder = torch.tensor(tc["ladder"])
    bias = torch.zeros(Cout)
    ro = None
    if tc["via"] == "bias":
        bias[base:] = ladder[torch.arange(extra) % len(ladder)]
    else:
        ro = ladder[torch.arange(N) % len(ladder)]
    want_aux = act != lc.ACT_SIGMOID
    assert lc.dispatch_class("fwd", N, Cin, Cout, act, ro is not None, want_aux)[0] == tc["kernel"]
    ref = lc.reference_forward(act, x, W, bias, ro)
    reach = float((ref["z"] if ro is None else ref["z"] + ro.double()[:, None]).abs().max())
    assert max(tc["ladder"]) < reach < 80.0
    xd, Wd, bd, rod = _on(dev, x), _on(dev, W), _on(dev, bias), _on(dev, ro)
    out = _forward(L, lib, dev, N, Cin, Cout, act, xd, Wd, bd, rod, want_aux)
    _clean(out, tc["name"])
    h, aux = out[0][1], out[1][1]
    worst.take(h, ref["h"], lc.BOUND["fwd"], (tc["name"], "h"))
    if want_aux:
        worst.take(aux, ref["aux"], lc.BOUND["fwd"], (tc["name"], "aux"))
    # the same layer without the ladder
    if tc["via"] == "bias":
        assert lc.dispatch_class("fwd", N, Cin, base, act, False, want_aux)[0] == tc["kernel"]
        plain = _forward(L, lib, dev, N, Cin, base, act, xd, _on(dev, W[:base]), _on(dev, bias[:base]), None, want_aux)
        _clean(plain, tc["name"])
        assert lc.same_bits(h[:, :base], plain[0][1]), (tc["name"], "the ladder columns changed their neighbours' h")
        assert lc.same_bits(aux[:, :base], plain[1][1]), (tc["name"], "the ladder columns changed their neighbours' aux")
    else:
        rows = (ro == 0).nonzero().flatten().to(dev)
        plain = _forward(L, lib, dev, N, Cin, Cout, act, xd, Wd, bd, _on(dev, torch.zeros(N)), want_aux)
        _clean(plain, tc["name"])
        assert lc.same_bits(h[rows], plain[0][1][rows]), (tc["name"], "the ladder rows changed their neighbours' h")
        if Cout % 32:                                            # (no row offset at all: the same kernel only where Cout % 32 != 0)
            none = _forward(L, lib, dev, N, Cin, Cout, act, xd, Wd, bd, None, want_aux)
            assert lc.same_bits(none[0][1], plain[0][1]), (tc["name"], "a zero row offset differs from none")
    # its backward, fed what the forward left behind
    z = ref["z"] if ro is None else ref["z"] + ro.double()[:, None]
    zt = z.clone().requires_grad_(True)
    (lc.act_forward(act, zt) * dh.double()).sum().backward()
    dz_ref = zt.grad
    dx_ref = dz_ref @ W.double()
    back = _backward(L, lib, dev, "bwd", N, Cin, Cout, act, _on(dev, dh), aux if want_aux else h, Wd, None, None, True)
    _clean(back, tc["name"])
    worst.take(back[1][1], dz_ref, lc.BOUND["bwd"], (tc["name"], "dz"))
    worst.take(back[0][1], dx_ref, lc.BOUND["bwd"], (tc["name"], "dx"))
    worst.settle(f"tails {tc['name']}")


@pytest.mark.parametrize("Cin", [33, 47, 100, 127])
def test_the_two_gelu_paths_meet(Cin):
    """A Cin -> 32 GELU layer (wide kernel) and the same weights as a Cin -> 33 layer with one zero row added (narrow kernel) agree
    on the first 32 columns within the forward bound; the narrow backward (Cin % 32 != 0), fed the WIDE forward's aux, gives the
    reference's dx."""
    L, lib = _lib()
    dev = _dev()
    worst = _Worst()
    N = 131
    g = torch.Generator().manual_seed(77 + Cin)
    x = torch.randn(N, Cin, generator=g) * 1.5
    W = torch.randn(32, Cin, generator=g) * Cin ** -0.5
    b = torch.randn(32, generator=g)
    dh = torch.randn(N, 32, generator=g)
    W33, b33 = torch.cat([W, torch.zeros(1, Cin)]), torch.cat([b, torch.zeros(1)])
    assert lc.dispatch_class("fwd", N, Cin, 32, 1, False, True)[0] == "wide"
    assert lc.dispatch_class("fwd", N, Cin, 33, 1, False, True)[0] == "narrow"
    assert lc.dispatch_class("bwd", N, Cin, 32, 1, False, False)[0] == "narrow"
    xd = _on(dev, x)
    wide = _forward(L, lib, dev, N, Cin, 32, 1, xd, _on(dev, W), _on(dev, b), None, True)
    narrow = _forward(L, lib, dev, N, Cin, 33, 1, xd, _on(dev, W33), _on(dev, b33), None, True)
    _clean(wide + narrow, Cin)
    ref = lc.reference_forward(lc.ACT_GELU, x, W, b)
    for i, name in enumerate(("h", "aux")):
        worst.take(wide[i][1], ref[name], lc.BOUND["fwd"], (Cin, "wide " + name))
        worst.take(narrow[i][1][:, :32], ref[name], lc.BOUND["fwd"], (Cin, "narrow " + name))
        worst.take(narrow[i][1][:, :32], wide[i][1].double(), lc.BOUND["fwd"], (Cin, "narrow against wide " + name))
    # the added column: gelu(0) = 0 exactly, gelu'(0) = 1/2 to the erf approximation's 1.5e-7 (halved) plus one rounding
    assert bool((narrow[0][1][:, 32] == 0).all()) and float((narrow[1][1][:, 32] - 0.5).abs().max()) <= 2e-7
    back = _backward(L, lib, dev, "bwd", N, Cin, 32, 1, _on(dev, dh), wide[1][1], _on(dev, W), None, None, True)
    _clean(back, Cin)
    dz_ref = dh.double() * lc.gelu_grad(ref["z"])
    worst.take(back[1][1], dz_ref, lc.BOUND["bwd"], (Cin, "dz"))
    worst.take(back[0][1], dz_ref @ W.double(), lc.BOUND["bwd"], (Cin, "dx"))
    worst.settle(f"the two GELU paths, Cin={Cin}")


# ---- the element-wise kernels of sg_decode.hip ---------------------------------------------------------------------------------------
_EW_N = (1, 63, 64, 65, 257, 4099)
_EW_C = (1, 3, 4, 31, 32, 33, 127, 128)


def _act_grad_from_z(act, z, ro):
    zt = z.clone().requires_grad_(True)
    lc.act_forward(act, zt, ro).sum().backward()
    return zt.grad


@pytest.mark.parametrize("N", _EW_N)
def test_bias_act_forward_backward(N):
    """sg_bias_act_forward / _backward (linear_layers.activation) against fp64: every act, bias and row_offset present and absent,
    z_out present, absent, and h_out aliasing y; dz, and dbias against fp64 column sums (3e-5 / 3e-6, the pair test_gpu_decode.py
    uses for db) and absent (the streaming kernel).  dh has mean 0.5 so that no column sum is a cancellation to ~0."""
    L, lib = _lib()
    dev = _dev()
    worst, worst_db = _Worst(), _Worst()
    for C_ in _EW_C:
        g = torch.Generator().manual_seed(N * 131 + C_)
        y = torch.randn(N, C_, generator=g) * 1.5
        bias_c, ro_c = torch.randn(C_, generator=g), torch.randn(N, generator=g)
        dh = torch.randn(N, C_, generator=g) + 0.5
        yd, dhd = _on(dev, y), _on(dev, dh)
        ws = torch.empty(int(lib.sg_bias_act_ws_bytes(N, C_)), dtype=torch.uint8, device=dev)
        for act in lc.ACTS:
            for bias in (None, bias_c):
                for ro in (None, ro_c):
                    where = (N, C_, act, bias is not None, ro is not None)
                    z = y.double() if bias is None else y.double() + bias.double()
                    h_ref = lc.act_forward(act, z, None if ro is None else ro.double())
                    bd, rod = _on(dev, bias), _on(dev, ro)
                    hs = []
                    for mode in ("z_out", "no z_out", "alias"):
                        h, hf = lc.guarded((N, C_), dev)
                        zo, zf = lc.guarded((N, C_), dev) if mode == "z_out" else (None, None)
                        src = yd
                        if mode == "alias":
                            h.copy_(y)
                            src = h
                        L.check(lib.sg_bias_act_forward(N, C_, act, _p(src), _p(bd), _p(rod), _p(zo), _p(h), _st(dev)), "bias act forward")
                        _clean([("h", h, hf), ("z", zo, zf)], where + (mode,))
                        worst.take(h, h_ref, lc.BOUND["fwd"], where + (mode, "h"))
                        if zo is not None:
                            worst.take(zo, z, lc.BOUND["fwd"], where + (mode, "z"))
                        hs.append(h)
                    assert lc.same_bits(hs[0], hs[1]) and lc.same_bits(hs[0], hs[2]), (where, "h depends on z_out / aliasing")
                    # backward from the fp32 pre-activation
                    z32 = z.float()
                    dz_ref = dh.double() * _act_grad_from_z(act, z32.double(), None if ro is None or act != lc.ACT_SIGMOID else ro.double())
                    zd = _on(dev, z32)
                    got = []
                    for with_db in (True, False):
                        dz, dzf = lc.guarded((N, C_), dev)
                        db, dbf = lc.guarded((C_,), dev) if with_db else (None, None)
                        L.check(lib.sg_bias_act_backward(N, C_, act, _p(zd), _p(rod), _p(dhd), _p(ws), _p(dz), _p(db), _st(dev)),
                                "bias act backward")
                        _clean([("dz", dz, dzf), ("dbias", db, dbf)], where)
                        worst.take(dz, dz_ref, lc.BOUND["bwd"], where + ("dz", with_db))
                        if db is not None:
                            worst_db.take(db, dz_ref.sum(0), lc.BOUND_DBIAS, where + ("dbias",))
                        got.append(dz)
                    assert lc.same_bits(got[0], got[1]), (where, "dz depends on whether dbias is asked for")
    worst_db.settle(f"bias + activation, N={N}, dbias")
    worst.settle(f"bias + activation, N={N}")


@pytest.mark.parametrize("N", _EW_N)
def test_scales_head_forward_backward(N):
    """sg_scales_head_forward / _backward (linear_layers.scales_head) against fp64: scales = log(exp(z) + 1) and aux = z, each row three
    times; dz = (sum dscales) e^z / (e^z + 1) + sum daux with dscales and daux each NULL in turn."""
    L, lib = _lib()
    dev = _dev()
    worst = _Worst()
    g = torch.Generator().manual_seed(900 + N)
    z = torch.randn(N, generator=g) * 3
    ds, da = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    zd, dsd, dad = _on(dev, z), _on(dev, ds), _on(dev, da)
    s, sf = lc.guarded((N, 3), dev)
    a, af = lc.guarded((N, 3), dev)
    L.check(lib.sg_scales_head_forward(N, _p(zd), _p(s), _p(a), _st(dev)), "scales head forward")
    _clean([("scales", s, sf), ("aux", a, af)], N)
    worst.take(s, lc.act_forward(lc.ACT_SOFTPLUS, z.double())[:, None].expand(N, 3), lc.BOUND["fwd"], (N, "scales"))
    assert lc.same_bits(a, zd[:, None].expand(N, 3).contiguous()), (N, "aux is z, three times")
    sig = torch.sigmoid(z.double())
    for name, p_ds, p_da, ref in (("both", dsd, dad, ds.double().sum(1) * sig + da.double().sum(1)),
                                  ("no daux", dsd, None, ds.double().sum(1) * sig), ("no dscales", None, dad, da.double().sum(1))):
        dz, dzf = lc.guarded((N,), dev)
        L.check(lib.sg_scales_head_backward(N, _p(zd), _p(p_ds), _p(p_da), _p(dz), _st(dev)), "scales head backward")
        _clean([("dz", dz, dzf)], (N, name))
        worst.take(dz, ref, lc.BOUND["bwd"], (N, name, "dz"))
    worst.settle(f"scales head, N={N}")
