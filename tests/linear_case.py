"""The cases of the fused linear kernels' shape tests (no GPU): tests/test_linear_case_host.py proves on a CPU that the list
reaches every instantiation the host dispatch of sings_amd/csrc/sg_linear.hip can choose, tests/test_gpu_linear_shapes.py runs
the list on the device.

What the dispatch branches on (sg_launch_linear_fwd / _bwd / _bwd_fan -> sg_linear_launch):
  * the reduction width CK (forward: Cin, backward: Cout) in classes NQ = 1, 4, 6, 8, 12, 16 (CK <= 8, 32, 48, 64, 96, 128, padded
    to 8 NQ), and CK % 4 (16-byte or element loads of the streamed rows);
  * the output width CO (forward: Cout, backward: Cin): CO % 32 == 0 without a sigmoid row offset and below the 32-bit size guard
    -> the wide kernel (buffer loads and stores, two tiles of look-ahead), anything else -> the narrow one; TO = ceil(CO / 32)
    column blocks and PT = 1, 2 or 4 point tiles per round, R = 32 PT rows;
  * Cout <= 6 with Cin 64 | 128, act 0 | 2 and no aux array -> the skinny streaming kernel, 4 (64 / L) rows per wave and round;
  * heads riding in the wide backward (the fan): NQ = 6, 8, 12, 16 of the main layer x EXQ = 1, 2 blocks of eight head columns.

A case is ``(direction, N, Cin, Cout, act, options)``; ``options`` is a dict with the keys ``OPTION_DEFAULTS`` lists.
Everything random is seeded from the case itself.  ``reference`` is fp64 torch and nothing else.
"""
import math

import torch

ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_SOFTPLUS = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_SOFTPLUS)
DIRECTIONS = ("fwd", "bwd", "acc", "fan")
# the edges of every NQ class and of % 4, % 8, % 32
WIDTHS = (1, 3, 4, 7, 8, 9, 12, 20, 31, 32, 33, 36, 47, 48, 49, 60, 63, 64, 65, 68, 95, 96, 97, 100, 127, 128)
MAXC = 128
WIDE_GRID_CAP, NARROW_GRID_CAP, SKINNY_GRID_CAP = 512, 768, 2048
NARROW_TILE, WIDE_TILE = 4352, 6656          # floats of one LDS tile (SGL_TILE; sgl_wide_cfg::FIT)
SENTINEL = 0x7FA5A5A5                        # guard words: a NaN pattern no kernel computes
STALE = 0x4E4E4E4E                           # "other stale bytes" of the determinism call: a finite float (8.6e8)
GUARD_FRONT, GUARD_ROWS = 64, 256            # floats in front of a guarded view, rows of `cols` floats behind it
POISON_ROWS = 256
# |a - b| <= rtol |b| + atol_scale max|b|: the pairs tests/test_gpu_decode.py uses for these kernels
BOUND = {"fwd": (2e-5, 2e-6), "bwd": (2e-5, 2e-6), "acc": (5e-5, 5e-6), "fan": (5e-5, 5e-6)}
BOUND_DBIAS = (3e-5, 3e-6)
OPTION_DEFAULTS = dict(bias=True, row_offset=False, aux_out=True, dz_out=True, heads=((0, 0), (0, 0)), long=False)


# ---- the dispatch, restated ----------------------------------------------------------------------------------------------------
def nq_class(ck):
    nq = (ck + 7) // 8
    for c in (1, 4, 6, 8, 12, 16):
        if nq <= c:
            return c
    raise ValueError(ck)


def narrow_point_tiles(TO, CKP):
    pt = 4 // TO
    while pt > 1 and 32 * pt * (CKP + 4) > NARROW_TILE:
        pt >>= 1
    return pt


def wide_point_tiles(TO, nqt):
    fit = WIDE_TILE // (32 * (8 * nqt + 4))
    cap = 4 if fit >= 4 else (2 if fit >= 2 else 1)
    return min(4 // TO, cap)


def size_guard(N, cmax):
    """The 32-bit byte-offset guard of the wide kernel: rows plus two rounds of look-ahead, times the wider side."""
    return (N + 2 * 512 * 128) * cmax * 4 < 0x7fffffff


def dispatch_class(direction, N, Cin, Cout, act, has_row_offset, has_aux_out, heads=()):
    """-> (kernel, NQ, EXQ, VEC, TO, PT, weights_vectorised), or None where the C ABI refuses the call.

    A restatement, in plain Python, of sg_launch_linear_fwd, sg_launch_linear_bwd, sg_launch_linear_bwd_fan and
    sg_linear_launch (sings_amd/csrc/sg_linear.hip) and of the argument checks in front of them (sg_api_ops.hip).  It
    DESCRIBES the dispatch -- which case reaches which instantiation -- and is not used to compute any expected value.

    kernel: "skinny" | "narrow" | "wide" | "fan".  For the tile kernels NQ, EXQ, VEC are the template arguments (the narrow kernel
    tests CK % 4 at run time: the same split), TO the 32-column blocks, PT the 32-row tiles per round, weights_vectorised whether
    the weight registers are filled by 16-byte loads.  For the skinny kernel the slots hold its own template arguments and
    geometry: NQ = L (lanes per row), TO = CO (the column count is a template argument), PT = rows per wave and round / 4.
    ``heads``: the two head column counts of a fan, (c0, c1)."""
    assert direction in DIRECTIONS
    if N <= 0 or act not in ACTS:
        return None
    if not (1 <= Cin <= MAXC and 1 <= Cout <= MAXC):
        return None
    if direction == "fwd":
        if Cout <= 6 and Cin in (64, 128) and act in (ACT_NONE, ACT_SIGMOID) and not has_aux_out and N * Cin * 4 < 0x7fffffff:
            L = Cin // 8
            return ("skinny", L, 0, True, Cout, 64 // L, True)
        CK, CO, bwd = Cin, Cout, False
    else:
        CK, CO, bwd = Cout, Cin, True
    nq, vec = (CK + 7) // 8, CK % 4 == 0
    if direction == "fan":
        c0, c1 = heads
        exc = c0 + c1
        if not (0 <= c0 <= 16 and 0 <= c1 <= 16 and 1 <= exc <= 16):
            return None
        if CO % 32 or not vec or not (N + 2 * 512 * 128) * 144 * 4 < 0x7fffffff:
            return None
        exq = 1 if exc <= 8 else 2
        NQ = max(6, nq_class(CK))
        TO = CO // 32
        return ("fan", NQ, exq, True, TO, wide_point_tiles(TO, NQ + exq), False)
    if direction == "acc" and Cin % 32:
        return None
    NQ = nq_class(CK)
    if CO % 32 == 0 and not (act == ACT_SIGMOID and has_row_offset) and size_guard(N, max(CK, CO)):
        TO = CO // 32
        return ("wide", NQ, 0, vec, TO, wide_point_tiles(TO, NQ), (not bwd) and vec)
    if direction == "acc":
        return None                                              # only the wide kernel accumulates
    TO = (CO + 31) // 32
    return ("narrow", NQ, 0, vec, TO, narrow_point_tiles(TO, 8 * NQ), (not bwd) and vec)


def rows_per_round(cls):
    """R: the rows one workgroup (tile kernels) or one wave (skinny kernel) handles per round."""
    return 4 * cls[5] if cls[0] == "skinny" else 32 * cls[5]


def grid_cap(cls):
    return {"skinny": SKINNY_GRID_CAP, "narrow": NARROW_GRID_CAP, "wide": WIDE_GRID_CAP, "fan": WIDE_GRID_CAP}[cls[0]]


def opts_of(case):
    o = dict(OPTION_DEFAULTS)
    o.update(case[5])
    return o


def class_of(case):
    d, N, Cin, Cout, act, _ = case
    o = opts_of(case)
    heads = tuple(c for c, _ in o["heads"])
    return dispatch_class(d, N, Cin, Cout, act, o["row_offset"], o["aux_out"] if d == "fwd" else False, heads if d == "fan" else ())


# ---- the case list ---------------------------------------------------------------------------------------------------------------
def _n_edges(R):
    return sorted({1, R - 1, R, R + 1, 2 * R + 1} - {0})


def _build_cases():
    cases = []

    def add(d, Cin, Cout, act, ns=None, **o):
        probe = (d, 100, Cin, Cout, act, o)
        cls = class_of(probe)
        assert cls is not None, probe
        R = rows_per_round(cls)
        for N in (ns or _n_edges(R)):
            cases.append((d, N, Cin, Cout, act, dict(o)))

    # (1) one shape per reachable (direction, class) of the tile kernels, all five N edges each.  The candidates are the width
    # edges x the activations x the flags that move the dispatch; among the candidates of a class the one whose (activation, flags)
    # the list has used least so far is taken, the smaller shape first.
    used, count = {}, 0
    for d in ("fwd", "bwd", "acc"):
        by_class = {}
        for Cin in WIDTHS:
            for Cout in WIDTHS:
                for act in ACTS:
                    for ro in ((False, True) if act == ACT_SIGMOID else (False,)):
                        for aux in ((True, False) if d == "fwd" else (True,)):
                            cls = dispatch_class(d, 100, Cin, Cout, act, ro, aux)
                            if cls is not None and cls[0] != "skinny":
                                by_class.setdefault(cls, []).append((Cin, Cout, act, ro, aux))
        for cls in sorted(by_class):
            kernel = cls[0]
            Cin, Cout, act, ro, aux = min(by_class[cls], key=lambda c: (used.get((d, kernel, c[2], c[3], c[4]), 0), c[0] + c[1], c))
            used[(d, kernel, act, ro, aux)] = used.get((d, kernel, act, ro, aux), 0) + 1
            count += 1
            add(d, Cin, Cout, act, row_offset=ro, aux_out=aux, bias=count % 3 != 0, dz_out=count % 4 != 0)

    # (2) what the class tuple does not hold: every activation in both tile kernels and every direction, the sigmoid with and without
    # a row offset, a sigmoid row offset on Cout % 32 == 0 (narrow kernel), the inference call (no aux array) and a backward
    # without dz, the element-load forward with the GELU epilogue
    for act in ACTS:
        for ro in ((False, True) if act == ACT_SIGMOID else (False,)):
            add("fwd", 36, 40, act, row_offset=ro)                              # narrow
            add("fwd", 36, 40, act, row_offset=ro, aux_out=False, bias=False)
            add("bwd", 40, 36, act, row_offset=ro)                              # narrow (CO = Cin = 40)
            add("bwd", 40, 36, act, row_offset=ro, dz_out=False)
            if not ro:
                add("fwd", 36, 64, act)                                         # wide
                add("fwd", 36, 64, act, aux_out=False, bias=False)
                add("fwd", 33, 32, act)                                         # wide, element loads
                add("bwd", 64, 36, act)                                         # wide (CO = Cin = 64)
                add("bwd", 64, 33, act, dz_out=False)
                add("acc", 64, 36, act)
                add("acc", 96, 7, act, dz_out=False)
    for Cout in (32, 64, 96, 128):
        add("fwd", 20, Cout, ACT_SIGMOID, row_offset=True, aux_out=False)
        add("fwd", 20, Cout, ACT_SIGMOID, aux_out=False)

    # (3) the skinny kernel: every Cout x L, both activations, N at the edges of one wave's round
    for Cin in (64, 128):
        rpr = 4 * (64 // (Cin // 8))
        for Cout in range(1, 7):
            add("fwd", Cin, Cout, ACT_NONE, ns=(1, rpr - 1, rpr, rpr + 1), aux_out=False, bias=Cout % 2 == 1)
            add("fwd", Cin, Cout, ACT_SIGMOID, ns=(1, rpr - 1, rpr, rpr + 1), aux_out=False, row_offset=Cout % 2 == 0)

    # (4) the fan: one shape per class (NQ x EXQ x TO), heads in slot 0, slot 1 and both, head act 0 and 2, main act 0 and 1
    heads1 = ((1, 0), (0, 3), (3, 5), (8, 0), (0, 8), (2, 6), (0, 1), (6, 0))
    heads2 = ((9, 0), (0, 16), (8, 8), (16, 0), (10, 6), (0, 9), (3, 6), (1, 8))
    by_class = {}
    for Cin in (32, 64, 96, 128):
        for Cout in (4, 48, 52, 64, 68, 96, 100, 128):
            for hs in heads1 + heads2:
                cls = dispatch_class("fan", 100, Cin, Cout, 0, False, False, hs)
                by_class.setdefault(cls, []).append((Cin, Cout, hs))
    i = 0
    for cls in sorted(by_class):
        Cin, Cout, hs = min(by_class[cls], key=lambda c: (used.get(("fan", c[1]), 0) + used.get(("fan", c[2]), 0), c))
        used[("fan", Cout)] = used.get(("fan", Cout), 0) + 1
        used[("fan", hs)] = used.get(("fan", hs), 0) + 1
        hacts = ((0, 0), (2, 0), (0, 2), (2, 2))[i % 4]
        add("fan", Cin, Cout, (ACT_NONE, ACT_GELU)[(i // 2) % 2], heads=tuple((c, a if c else 0) for c, a in zip(hs, hacts)))
        i += 1
    for c in range(1, 17):                                       # every head width 1..16, alternately in slot 0 and slot 1
        hs = ((c, 2 * (c % 3 == 0)), (0, 0)) if c % 2 else ((0, 0), (c, 2 * (c % 3 == 0)))
        add("fan", 64, 48, ACT_GELU if c % 4 < 2 else ACT_NONE, ns=(65,), heads=hs)

    # (5) long cases: every persistent workgroup runs at least four rounds (N >= 4 grid_cap R + 1, odd), so the two-tile look-ahead
    # reaches its steady state and its ragged end
    for d, N, Cin, Cout, act, o in (
            ("fwd", 65537, 128, 128, ACT_GELU, {}),                                             # wide, R = 32
            ("bwd", 65539, 128, 128, ACT_GELU, {}),
            ("acc", 65541, 96, 48, ACT_SOFTPLUS, {}),
            ("fan", 65543, 128, 128, ACT_GELU, dict(heads=((3, 0), (6, 0)))),
            ("fwd", 131073, 64, 64, ACT_SOFTPLUS, {}),                                          # wide, R = 64
            ("fwd", 262145, 31, 32, ACT_GELU, {}),                                              # wide, R = 128, element loads
            ("fwd", 98305, 100, 127, ACT_SIGMOID, dict(row_offset=True, aux_out=False)),        # narrow, R = 32
            ("bwd", 98307, 97, 68, ACT_SIGMOID, {}),
            ("fwd", 196609, 20, 40, ACT_GELU, {}),                                              # narrow, R = 64
            ("fwd", 393217, 8, 20, ACT_NONE, dict(aux_out=False))):                             # narrow, R = 128
        cases.append((d, N, Cin, Cout, act, dict(o, long=True)))
    # the skinny kernel's grid-stride loop runs more than once: beyond 2048 workgroups x 256 rows
    cases.append(("fwd", 2048 * 256 + 33, 64, 3, ACT_NONE, dict(aux_out=False, long=True)))
    cases.append(("fwd", 2048 * 256 + 17, 128, 6, ACT_SIGMOID, dict(aux_out=False, row_offset=True, long=True)))
    return cases


CASES = _build_cases()


def group_of(case):
    """The test a case runs in: (direction, kernel, NQ)."""
    cls = class_of(case)
    return (case[0], cls[0], cls[1])


GROUPS = sorted({group_of(c) for c in CASES})

# Tail cases: bias or row-offset ladders far into the activations' tails, apart from CASES so that their scale does not loosen the
# ordinary cases' bounds.  A layer of `base` columns with zero bias followed by the ladder columns (bias = the ladder, cycled); the
# sigmoid's ladder goes down the rows through row_offset.  |z| stays below 80: log(exp(z) + 1) is the reference's own expression.
GELU_LADDER = (-9.0, -6.0, -3.0, 0.0, 3.0, 6.0, 9.0)
WIDE_LADDER = (-20.0, -10.0, 0.0, 10.0, 20.0)
TAIL_CASES = (
    dict(name="gelu_wide", act=ACT_GELU, N=97, Cin=64, base=32, extra=32, ladder=GELU_LADDER, via="bias", kernel="wide"),
    dict(name="gelu_narrow", act=ACT_GELU, N=97, Cin=64, base=33, extra=7, ladder=GELU_LADDER, via="bias", kernel="narrow"),
    dict(name="softplus_wide", act=ACT_SOFTPLUS, N=97, Cin=64, base=32, extra=32, ladder=WIDE_LADDER, via="bias", kernel="wide"),
    dict(name="softplus_narrow", act=ACT_SOFTPLUS, N=97, Cin=64, base=33, extra=5, ladder=WIDE_LADDER, via="bias", kernel="narrow"),
    dict(name="sigmoid_rows", act=ACT_SIGMOID, N=97, Cin=64, base=33, extra=0, ladder=WIDE_LADDER, via="row_offset", kernel="narrow"),
    dict(name="sigmoid_rows_32", act=ACT_SIGMOID, N=97, Cin=64, base=32, extra=0, ladder=WIDE_LADDER, via="row_offset", kernel="narrow"),
)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _seed(case):
    d, N, Cin, Cout, act, _ = case
    o = opts_of(case)
    return (DIRECTIONS.index(d) * 1000003 + N * 7919 + Cin * 131 + Cout * 17 + act * 5 + sum(c for c, _ in o["heads"])) % (2 ** 31)


def aux_of(act, z):
    """What the forward leaves for the backward, from the pre-activation z (fp64): gelu'(z) | sigmoid(z) | z."""
    if act == ACT_GELU:
        return gelu_grad(z)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    return z


def make_tensors(case, dev=None):
    """The fp32 inputs of a case (a dict).  On the CPU unless `dev` is given (the long cases are drawn on the device)."""
    d, N, Cin, Cout, act, _ = case
    o = opts_of(case)
    dev = torch.device("cpu") if dev is None else dev
    g = torch.Generator(device=dev).manual_seed(_seed(case))

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * s

    t = {}
    if d == "fwd":
        t["x"] = rn(N, Cin)
        t["W"] = rn(Cout, Cin, s=Cin ** -0.5)
        t["bias"] = rn(Cout) if o["bias"] else None
        t["row_offset"] = rn(N) if o["row_offset"] else None
        return t
    t["dh"] = rn(N, Cout)
    t["W"] = rn(Cout, Cin, s=Cin ** -0.5)
    t["aux"] = aux_of(act, rn(N, Cout, s=1.5).double()).float() if act != ACT_NONE else None
    t["row_offset"] = rn(N) if o["row_offset"] else None           # (the backward takes one and ignores its values)
    if d == "acc":
        t["old"] = rn(N, Cin, s=2.0)
    if d == "fan":
        t["heads"] = []
        for c, a in o["heads"]:
            t["heads"].append(None if c == 0 else dict(c=c, act=a, dh=rn(N, c), W=rn(c, Cin, s=Cin ** -0.5),
                                                       aux=torch.sigmoid(rn(N, c, s=1.5).double()).float() if a else None))
    return t


# ---- the reference: fp64 torch ---------------------------------------------------------------------------------------------------
def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * (0.5 ** 0.5)))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * (0.5 ** 0.5))) + z * torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi))


def act_forward(act, z, row_offset=None):
    if act == ACT_GELU:
        return gelu(z)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-(z if row_offset is None else z + row_offset[:, None])))
    if act == ACT_SOFTPLUS:
        return torch.log(torch.exp(z) + 1.0)
    return z


def act_grad_from_aux(act, aux):
    """act'(z) from what the backward is handed (include/sings_hip.h): gelu'(z) itself | h (1 - h) | e^z / (e^z + 1)."""
    if act == ACT_GELU:
        return aux
    if act == ACT_SIGMOID:
        return aux * (1.0 - aux)
    if act == ACT_SOFTPLUS:
        e = torch.exp(aux)
        return e / (e + 1.0)
    return torch.ones_like(aux)


def reference_forward(act, x, W, bias=None, row_offset=None):
    z = x.double() @ W.double().T
    if bias is not None:
        z = z + bias.double()
    h = act_forward(act, z, None if row_offset is None else row_offset.double())
    return dict(z=z, h=h, aux=gelu_grad(z) if act == ACT_GELU else z)


def reference_backward(act, dh, aux, W, heads=(), old=None):
    dz = dh.double() if act == ACT_NONE else dh.double() * act_grad_from_aux(act, aux.double())
    dx = dz @ W.double()
    hdz = []
    for hd in heads:
        if hd is None:
            hdz.append(None)
            continue
        d = hd["dh"].double() if not hd["act"] else hd["dh"].double() * act_grad_from_aux(ACT_SIGMOID, hd["aux"].double())
        dx = dx + d @ hd["W"].double()
        hdz.append(d)
    if old is not None:
        dx = old.double() + dx
    return dict(dz=dz, dx=dx, head_dz=hdz)


def reference(case, tensors):
    """fp64, on the device the tensors live on (the CPU, but for the long cases)."""
    d, _, _, _, act, _ = case
    t = tensors
    if d == "fwd":
        return reference_forward(act, t["x"], t["W"], t["bias"], t["row_offset"])
    return reference_backward(act, t["dh"], t["aux"], t["W"], t.get("heads", ()), t.get("old"))


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def guarded(shape, dev, stale=SENTINEL):
    """-> (view, flat): a 16-byte aligned fp32 view of `shape` inside a larger allocation, GUARD_FRONT floats in front and
    GUARD_ROWS rows (of shape[-1] floats) behind, all filled with SENTINEL; the view itself holds `stale`."""
    numel = 1
    for s in shape:
        numel *= int(s)
    flat = torch.full((GUARD_FRONT + numel + GUARD_ROWS * int(shape[-1]),), SENTINEL, dtype=torch.int32, device=dev)
    if stale != SENTINEL:
        flat[GUARD_FRONT:GUARD_FRONT + numel] = stale
    view = flat[GUARD_FRONT:GUARD_FRONT + numel].view(torch.float32).view(*shape)
    assert view.data_ptr() % 16 == 0
    return view, flat


def guard_intact(view, flat):
    n = view.numel()
    return bool((flat[:GUARD_FRONT] == SENTINEL).all()) and bool((flat[GUARD_FRONT + n:] == SENTINEL).all())


def poisoned(array, dev):
    """The fp32 input followed by POISON_ROWS more rows of NaN inside the same allocation: a row beyond N that reaches a result
    shows as NaN, and nothing is read outside an allocation.  (A vector counts as rows of one float.)"""
    a = array.contiguous()
    rows = int(a.shape[0])
    big = torch.full((rows + POISON_ROWS,) + tuple(a.shape[1:]), float("nan"), dtype=torch.float32, device=dev)
    big[:rows] = a.to(dev)
    view = big[:rows]
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return view


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fraction_of_bound(got, ref, rtol, atol_scale, scale=None):
    """max over ALL entries of |got - ref| / (rtol |ref| + atol_scale max|ref|): <= 1 passes.  inf if anything is not finite."""
    ref = ref.double()
    got = got.to(ref.device).double()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return float("inf")
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max()) + 1e-30 if scale is None else scale
    return float(((got - ref).abs() / (rtol * ref.abs() + atol_scale * scale)).max())
