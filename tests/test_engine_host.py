"""CPU tests of the pre-allocated engines of sings_amd/engine.py: every workspace against the library's layout calls, the flat
gradient layout of every engine (offset and shape of each ``d_*`` view), and the C calls each engine makes for a fixed script --
entry points in order, the flag word of each call, ``accumulate`` and which engine buffer every pointer lands in -- recorded by a
stub in place of the library.  The engines are built with ``device="cpu"``: nothing here launches a kernel."""
import ctypes as C
import re

import pytest
import torch

P, W, H, CAP, J = 40, 64, 48, 5000, 5

RASTER = [("d_means3D", 3), ("d_scales", 3), ("d_rots", 4), ("d_opacity", 1)]           # then sh 3M
SKINNED = [("d_xyz", 3), ("d_scales", 3), ("d_opacity", 1)]                             # then sh 3M, [rot w]


def _fields(family, M, with_rot=False, rot_width=9, sh_planar=False):
    """The documented flat gradient layout: (attribute, floats per Gaussian); with ``sh_planar`` the SH block comes last.  Without SH
    coefficients a raster engine has no ``d_sh`` (None), a skinned one an empty view."""
    head = RASTER if family == "raster" else SKINNED
    rot = [("d_rot", rot_width)] if with_rot else []
    sh = [("d_sh", 3 * M)] if M or family == "skinned" else []
    return head + rot + sh if sh_planar else head + sh + rot


def _make(kind, M=16, K=3, with_rot=False, rot_width=9, sh_planar=False, aux=False, grad_flat=None, device="cpu"):
    from sings_amd import engine as E
    if kind == "raster":
        return E.RasterEngine(P, W, H, M, device, CAP, grad_flat=grad_flat)
    if kind == "skinned":
        return E.SkinnedEngine(P, J, W, H, M, device, CAP, with_rot=with_rot, grad_flat=grad_flat, rot_width=rot_width,
                               sh_planar=sh_planar)
    if kind == "raster_frames":
        return E.RasterFramesEngine(P, W, H, M, K, device, CAP, grad_flat=grad_flat, sh_planar=sh_planar)
    return E.SkinnedFramesEngine(P, J, W, H, M, K, device, CAP, with_rot=with_rot, grad_flat=grad_flat, rot_width=rot_width,
                                 sh_planar=sh_planar, aux=aux)


LAYOUT_CASES = (
    [dict(kind="raster", M=M) for M in (0, 16)]
    + [dict(kind="skinned", with_rot=r, rot_width=w, sh_planar=p) for r, w in ((False, 9), (True, 6), (True, 9)) for p in (False, True)]
    + [dict(kind="skinned", M=0, with_rot=True, rot_width=6)]
    + [dict(kind="raster_frames", K=K, M=M, sh_planar=p) for K in (1, 3) for M in (0, 16) for p in (False, True) if M or not p]
    + [dict(kind="skinned_frames", K=K, with_rot=r, rot_width=w, sh_planar=p, aux=a) for K in (1, 3)
       for r, w in ((False, 9), (True, 6)) for p, a in ((False, False), (True, False), (False, True))])


def _case_id(c):
    return "-".join(f"{k}={v}" for k, v in c.items())


def _frames_layout(K):
    from sings_amd import _lib
    one, sizes = _lib.SgLayout(), [C.c_size_t() for _ in range(4)]
    _lib.check(_lib.load().sg_frames_layout(P, W, H, CAP, K, C.byref(one), *[C.byref(s) for s in sizes]), "sg_frames_layout")
    return one, [s.value for s in sizes]


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_case_id)
def test_workspaces_match_the_library_layout(case):
    from sings_amd import _lib
    lib = _lib.load()
    e = _make(**case)
    frames = case["kind"].endswith("_frames")
    K = case["K"] if frames else 1
    L = _lib.layout(P, W, H, CAP)
    one, (geom, binning, img, bwd) = _frames_layout(K)
    for name, _ in _lib.SgLayout._fields_:
        assert getattr(e.L, name) == getattr(L, name) == getattr(one, name), name
    assert (geom, binning, img) == (K * L.geom_bytes, K * L.bin_bytes, K * L.img_bytes)
    if K == 1:
        assert bwd == L.bwd_bytes                                    # (the K-camera record sums exist for K > 1 only)
    for t, n in ((e.geom, geom), (e.binning, binning), (e.img, img), (e.bwd_ws, bwd)):
        assert t.dtype == torch.uint8 and t.numel() == n and t.device.type == "cpu"
    assert not e.binning.view(K, L.bin_bytes)[:, :L.bin_ranges].any()      # the counters, zeroed once
    assert (e.P, e.W, e.H, e.cap) == (P, W, H, CAP)
    lead = (K,) if frames else ()
    assert tuple(e.color.shape) == lead + (3, H, W) and e.color.dtype == torch.float32
    assert tuple(e.radii.shape) == lead + (P,) and e.radii.dtype == torch.int32
    assert tuple(e.d_means2D.shape) == lead + (P, 3)
    if case["kind"].startswith("skinned"):
        assert tuple(e.d_A.shape) == lead + (J, 16) and tuple(e.d_transl.shape) == lead + (3,)
        want = lib.sg_skin_ws_floats_frames(P, K) if frames else lib.sg_skin_ws_floats(P)
        assert e.skin_ws.dtype == torch.float32 and e.skin_ws.numel() == want
    if case.get("aux"):
        assert e.aux_ws.numel() == _lib.frames_aux_layout(P, W, H, CAP, K)
        assert tuple(e.depth.shape) == tuple(e.alpha.shape) == (K, 1, H, W)
    elif case["kind"] == "skinned_frames":
        assert e.aux_ws is None and e.depth is None and e.alpha is None


def _check_views(e, fields, sh_planar):
    n = sum(w for _, w in fields)
    assert e.grad_flat.numel() == P * n and e.grad_flat.dtype == torch.float32 and e.grad_flat.is_contiguous()
    o = 0
    for name, w in fields:
        v = getattr(e, name)
        assert w == 0 or (v.data_ptr() - e.grad_flat.data_ptr()) == 4 * o, name           # (an empty view has no address)
        want = ((e.M, P, 3) if sh_planar else (P, e.M, 3)) if name == "d_sh" else (P, w)
        assert tuple(v.shape) == want and v.is_contiguous(), name
        o += P * w
    present = {name for name, _ in fields}
    for name in ("d_sh", "d_rot"):
        if hasattr(e, name) and name not in present:
            assert getattr(e, name) is None, name


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_case_id)
def test_gradient_views_follow_the_field_table(case):
    e = _make(**case)
    family = "raster" if case["kind"].startswith("raster") else "skinned"
    planar = case.get("sh_planar", False)
    fields = _fields(family, e.M, case.get("with_rot", False), case.get("rot_width", 9), planar)
    _check_views(e, fields, planar)
    # a caller-owned buffer: the views land in it, and nothing is written to it
    own = torch.full((e.grad_flat.numel(),), 7.0)
    e2 = _make(**case, grad_flat=own)
    assert e2.grad_flat.data_ptr() == own.data_ptr() and bool((own == 7.0).all())
    _check_views(e2, fields, planar)


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_case_id)
def test_every_engine_has_k_sh_planar_and_active_floats(case):
    e = _make(**case)
    planar = case.get("sh_planar", False)
    assert e.K == case.get("K", 3) if case["kind"].endswith("_frames") else e.K == 1
    assert e.sh_planar == planar
    # the prefix that carries a step's gradient: everything, unless the SH block is coefficient-major (and last)
    head = e.grad_flat.numel() - (e.d_sh.numel() if e.d_sh is not None else 0)
    for deg in range(4):
        assert e.active_floats(deg) == (head + (deg + 1) ** 2 * P * 3 if planar else e.grad_flat.numel())


@pytest.mark.parametrize("case", [c for c in LAYOUT_CASES if c.get("sh_planar")], ids=_case_id)
def test_an_engine_owned_planar_buffer_starts_with_the_sh_planes_zeroed(case):
    """The planes above the SH degree in use are never written by the kernels and are folded with the rest: zeroed once."""
    assert not _make(**case).d_sh.any()


@pytest.mark.parametrize("case", [dict(kind="raster"), dict(kind="skinned", with_rot=True, rot_width=6),
                                  dict(kind="raster_frames", sh_planar=True), dict(kind="skinned_frames", aux=True)], ids=_case_id)
def test_a_bad_gradient_buffer_is_refused(case):
    n = _make(**case).grad_flat.numel()
    msg = f"grad_flat must be a contiguous fp32 tensor of {n} elements on cpu"
    for bad in (torch.zeros(n + 1), torch.zeros(n - 1), torch.zeros(n, dtype=torch.float64), torch.zeros(2 * n)[::2],
                torch.zeros(n, device="meta")):
        with pytest.raises(ValueError, match=msg):
            _make(**case, grad_flat=bad)


@pytest.mark.parametrize("case", [dict(kind="raster"), dict(kind="skinned", with_rot=True, rot_width=6, sh_planar=True),
                                  dict(kind="raster_frames", sh_planar=True), dict(kind="skinned_frames", with_rot=True)],
                         ids=_case_id)
def test_every_engine_rebinds_its_gradient_views(case):
    e = _make(**case)
    family = "raster" if case["kind"].startswith("raster") else "skinned"
    planar = case.get("sh_planar", False)
    fields = _fields(family, e.M, case.get("with_rot", False), case.get("rot_width", 9), planar)
    other = torch.full((e.grad_flat.numel(),), 3.0)
    e.rebind_gradients(other)
    assert e.grad_flat.data_ptr() == other.data_ptr() and bool((other == 3.0).all())
    _check_views(e, fields, planar)
    for bad in (torch.zeros(other.numel() + 3), torch.zeros(other.numel(), dtype=torch.float16)):
        with pytest.raises(ValueError, match="grad_flat must be a contiguous fp32 tensor"):
            e.rebind_gradients(bad)


@pytest.mark.parametrize("kind", ["raster", "skinned", "raster_frames", "skinned_frames"])
def test_an_engine_builds_on_a_device_named_unlike_its_tensors_report_it(kind):
    """``device="cpu:0"``: the engine's tensors report "cpu", as tensors on "cuda" report "cuda:0"."""
    e = _make(kind, device="cpu:0")
    assert e.grad_flat.device == e.geom.device


@pytest.mark.parametrize("kind", ["raster", "skinned", "raster_frames", "skinned_frames"])
def test_a_gradient_buffer_is_checked_against_the_device_of_the_workspaces(kind):
    n = _make(kind).grad_flat.numel()
    e = _make(kind, device="cpu:0", grad_flat=torch.zeros(n))
    e.rebind_gradients(torch.zeros(n))
    with pytest.raises(ValueError, match=f"grad_flat must be a contiguous fp32 tensor of {n} elements on cpu"):
        e.rebind_gradients(torch.zeros(n, device="meta"))


def test_k_outside_one_to_sixteen_is_refused():
    for K in (0, 17):
        for kind in ("raster_frames", "skinned_frames"):
            with pytest.raises(ValueError, match="K must be 1..16"):
                _make(kind, K=K)


# ---- the C calls: a stub library records every call, its arguments read when the call is made ---------------------------------

_FLAG_NAMES = (("SHORT_LISTS", 1), ("WS_CLEAN", 2), ("THROUGHPUT", 4), ("BINNING", 8), ("COMPOSITE", 16), ("SH_PLANAR", 32),
               ("LONG_ROWS", 64))


class _Recorder:
    """Stands in for the library: every entry point records its call as one string and returns 0.  A tensor pointer is written
    as the names (engine attribute and / or caller input) of the tensors that start at that address; the settings struct as its
    flag word and camera pointers, the frame batch as its fields, the skin inputs as the tensors they point at."""

    def __init__(self, engine, inputs):
        self.e, self.inputs, self.calls = engine, inputs, []

    def _names(self):
        m = {}
        for k, v in list(vars(self.e).items()) + list(self.inputs.items()):
            if torch.is_tensor(v) and v.numel():
                m.setdefault(v.data_ptr(), set()).add(k)
        return {p: "|".join(sorted(n)) for p, n in m.items()}

    def _arg(self, a, names):
        ptr = lambda p: "-" if p is None else names.get(p, "?")
        if a is None:
            return "-"
        if isinstance(a, int):
            return str(a)
        if isinstance(a, C.c_void_p):
            return "null" if a.value is None else ptr(a.value)
        if isinstance(a, C.Array):
            return f"nr[{len(a)}]"
        o = getattr(a, "_obj", None)                                 # C.byref(...)
        from sings_amd import _lib
        if isinstance(o, _lib.SgRasterSettings):
            fl = "|".join(n for n, b in _FLAG_NAMES if o.flags & b) or "0"
            return f"S({fl}; {ptr(o.bg)} {ptr(o.viewmatrix)} {ptr(o.projmatrix)} {ptr(o.campos)})"
        if isinstance(o, _lib.SgFrameBatch):
            return f"FB({o.K},{o.camera_stride},{o.transl_stride})"
        if isinstance(o, _lib.SgSkinInputs):
            return "SK(" + " ".join(ptr(getattr(o, n)) for n, _ in _lib.SgSkinInputs._fields_[2:]) + ")"
        if isinstance(o, C.c_int64):
            return "nr"
        raise TypeError(f"unexpected argument {a!r}")

    def __getattr__(self, name):
        if not name.startswith("sg_"):
            raise AttributeError(name)

        def call(*args):
            names = self._names()
            self.calls.append(" ".join([name] + [self._arg(a, names) for a in args]))
            return 0
        return call


def _inputs(K, per_frame_camera=False, with_rot=False):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    z = lambda *s: torch.rand(*s)
    ins = dict(means3D=z(P, 3), shs=z(P, 16, 3), opacities=z(P, 1), scales=z(P, 3), rotations=z(P, 4), dL=z(K, 3, H, W),
               xyz=z(P, 3), rot=z(P, 6) if with_rot else None, w=z(P, J), A=z(K, J, 16), smpl=z(1), transl=z(K, 3),
               bg=z(3), vm=z(K, 4, 4) if per_frame_camera else z(4, 4), pm=z(K, 4, 4) if per_frame_camera else z(4, 4),
               cp=z(K, 3) if per_frame_camera else z(3), ddepth=z(K, 1, H, W), dalpha=z(K, 1, H, W),
               px=z(K, P, 3), pq=z(K, P, 4), ps=z(K, P, 3))
    cam = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.4, bg=ins["bg"], scale_modifier=1.0,
                                        viewmatrix=ins["vm"], projmatrix=ins["pm"], sh_degree=1, campos=ins["cp"], prefiltered=False,
                                        debug=False)
    return {k: v for k, v in ins.items() if v is not None}, cam


def _ready(kind, per_frame_camera=False, **opts):
    """An engine of ``kind`` on the stub library: (engine, inputs, camera, recorded calls, Gaussian inputs, dL_dcolor)."""
    frames = kind.endswith("_frames")
    e = _make(kind, **opts)
    ins, cam = _inputs(opts.get("K", 3) if frames else 1, per_frame_camera, opts.get("with_rot", False))
    e.lib = _Recorder(e, ins)
    e._stream = lambda: C.c_void_p(0)                                # (no HIP streams on the CPU)
    g = [ins[k] for k in (("means3D", "shs", "opacities", "scales", "rotations") if kind.startswith("raster") else
                          ("shs", "opacities", "scales"))]
    return e, ins, cam, e.lib.calls, g, ins["dL"] if frames else ins["dL"][0]


def script_raster():
    e, ins, cam, calls, g, dL = _ready("raster")
    e.set_camera(cam, short_lists=True)
    e.forward(*g)
    e.forward(*g, sync_num_rendered=True)
    e.backward(*g, dL)
    e.set_camera(cam, long_rows=True)
    e.throughput = True
    e.forward(*g)
    e._chain = lambda: (True, None, None)                          # (a ViewBatch whose row an earlier view wrote)
    e.backward(*g, dL)
    e._chain = None
    e.num_rendered()
    return calls


def script_skinned():
    e, ins, cam, calls, g, dL = _ready("skinned", with_rot=True, rot_width=6, sh_planar=True)
    e.set_camera(cam, long_rows=True)
    e.set_frame(ins["xyz"], ins["rot"], ins["w"], ins["A"][0], ins["smpl"], ins["transl"][0])
    e.forward(*g)
    e.forward(*g, sync_num_rendered=True, posed_out=(ins["px"][0], ins["pq"][0], ins["ps"][0]))
    e.backward(*g, dL)
    e.set_camera(cam)
    e.throughput = True
    e.forward(*g)
    e._chain = lambda: (True, None, None)
    e.backward(*g, dL)
    e._chain = None
    e.num_rendered()
    return calls


def script_raster_frames():
    e, ins, cam, calls, g, dL = _ready("raster_frames", per_frame_camera=True, sh_planar=True)
    e.set_camera(cam, short_lists=True, long_rows=True)
    e.forward(*g)
    e.forward(*g, sync_num_rendered=True)
    e.backward(*g, dL)
    e.backward(*g, dL, accumulate=True)
    e.set_camera(cam)
    e.throughput = False
    e.forward(*g)
    e._chain = lambda: (True, None, None)
    e.backward(*g, dL)
    e._chain = None
    e.num_rendered()
    return calls


def script_skinned_frames():
    e, ins, cam, calls, g, dL = _ready("skinned_frames", sh_planar=True)
    e.set_camera(cam, long_rows=True)
    e.set_frames(ins["xyz"], None, ins["w"], ins["A"], ins["smpl"], ins["transl"])
    e.forward(*g)
    e.forward(*g, sync_num_rendered=True, posed_out=(ins["px"], ins["pq"], ins["ps"]))
    e.forward(*g, phase="binning")
    e.forward(*g, phase="composite")
    e.backward(*g, dL)
    e.backward_records(dL)
    e.backward_gaussians(*g, accumulate=True)
    e._chain = lambda: (True, None, None)
    e.backward(*g, dL)
    e._chain = None
    e.num_rendered()
    a, ins, cam, aux_calls, g, dL = _ready("skinned_frames", aux=True)
    a.set_camera(cam)
    a.set_frames(ins["xyz"], None, ins["w"], ins["A"], ins["smpl"], ins["transl"][0])
    a.forward(*g, sync_num_rendered=True)
    a.backward(*g, dL, dL_ddepth=ins["ddepth"], dL_dalpha=ins["dalpha"])
    return calls + aux_calls


CAM = "bg vm pm cp"
GAUSS = "means3D shs - opacities scales rotations -"
EXPECTED = {
    "raster": [
        f"sg_rasterize_forward S(SHORT_LISTS|WS_CLEAN; {CAM}) {P} {GAUSS} geom binning {CAP} img color radii 0 - null",
        f"sg_rasterize_forward S(SHORT_LISTS|WS_CLEAN; {CAM}) {P} {GAUSS} geom binning {CAP} img color radii 0 nr null",
        f"sg_rasterize_backward_records S(SHORT_LISTS|WS_CLEAN; {CAM}) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_rasterize_backward_gaussians S(SHORT_LISTS|WS_CLEAN; {CAM}) {P} {GAUSS} radii geom binning {CAP} bwd_ws 0 d_means3D|grad_flat d_means2D d_sh - d_opacity d_scales d_rots - null",
        f"sg_rasterize_forward S(WS_CLEAN|THROUGHPUT|LONG_ROWS; {CAM}) {P} {GAUSS} geom binning {CAP} img color radii 0 - null",
        f"sg_rasterize_backward_records S(WS_CLEAN|THROUGHPUT|LONG_ROWS; {CAM}) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_rasterize_backward_gaussians S(WS_CLEAN|THROUGHPUT|LONG_ROWS; {CAM}) {P} {GAUSS} radii geom binning {CAP} bwd_ws 1 d_means3D|grad_flat d_means2D d_sh - d_opacity d_scales d_rots - null",
        "sg_read_num_rendered binning nr null",
    ],
    "skinned": [
        f"sg_skinned_forward S(WS_CLEAN|SH_PLANAR|LONG_ROWS; {CAM}) {P} SK(xyz rot w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii - - - - null",
        f"sg_skinned_forward S(WS_CLEAN|SH_PLANAR|LONG_ROWS; {CAM}) {P} SK(xyz rot w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii px pq ps nr null",
        f"sg_rasterize_backward_records S(WS_CLEAN|SH_PLANAR|LONG_ROWS; {CAM}) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_skinned_backward_gaussians S(WS_CLEAN|SH_PLANAR|LONG_ROWS; {CAM}) {P} SK(xyz rot w A smpl transl - - -) shs opacities scales radii geom binning {CAP} bwd_ws skin_ws 0 - - d_xyz|grad_flat d_rot d_scales d_opacity d_sh d_means2D d_A d_transl null",
        f"sg_skinned_forward S(WS_CLEAN|THROUGHPUT|SH_PLANAR; {CAM}) {P} SK(xyz rot w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii - - - - null",
        f"sg_rasterize_backward_records S(WS_CLEAN|THROUGHPUT|SH_PLANAR; {CAM}) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_skinned_backward_gaussians S(WS_CLEAN|THROUGHPUT|SH_PLANAR; {CAM}) {P} SK(xyz rot w A smpl transl - - -) shs opacities scales radii geom binning {CAP} bwd_ws skin_ws 1 - - d_xyz|grad_flat d_rot d_scales d_opacity d_sh d_means2D d_A d_transl null",
        "sg_read_num_rendered binning nr null",
    ],
    "raster_frames": [
        f"sg_rasterize_forward_frames S(SHORT_LISTS|WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,1,0) {P} {GAUSS} geom binning {CAP} img color radii - null",
        f"sg_rasterize_forward_frames S(SHORT_LISTS|WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,1,0) {P} {GAUSS} geom binning {CAP} img color radii nr[3] null",
        f"sg_rasterize_backward_records_frames S(SHORT_LISTS|WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,1,0) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_rasterize_backward_gaussians_frames S(SHORT_LISTS|WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,1,0) {P} {GAUSS} radii geom binning {CAP} bwd_ws 0 d_means3D|grad_flat d_means2D d_sh - d_opacity d_scales d_rots - null",
        f"sg_rasterize_backward_records_frames S(SHORT_LISTS|WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,1,0) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_rasterize_backward_gaussians_frames S(SHORT_LISTS|WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,1,0) {P} {GAUSS} radii geom binning {CAP} bwd_ws 1 d_means3D|grad_flat d_means2D d_sh - d_opacity d_scales d_rots - null",
        f"sg_rasterize_forward_frames S(WS_CLEAN|SH_PLANAR; {CAM}) FB(3,1,0) {P} {GAUSS} geom binning {CAP} img color radii - null",
        f"sg_rasterize_backward_records_frames S(WS_CLEAN|SH_PLANAR; {CAM}) FB(3,1,0) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_rasterize_backward_gaussians_frames S(WS_CLEAN|SH_PLANAR; {CAM}) FB(3,1,0) {P} {GAUSS} radii geom binning {CAP} bwd_ws 1 d_means3D|grad_flat d_means2D d_sh - d_opacity d_scales d_rots - null",
        f"sg_read_num_rendered_frames binning {P} 64 48 {CAP} 3 nr[3] null",
    ],
    "skinned_frames": [
        f"sg_skinned_forward_frames S(WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} SK(xyz - w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii - - - - null",
        f"sg_skinned_forward_frames S(WS_CLEAN|THROUGHPUT|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} SK(xyz - w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii px pq ps nr[3] null",
        f"sg_skinned_forward_frames S(WS_CLEAN|THROUGHPUT|BINNING|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} SK(xyz - w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii - - - - null",
        f"sg_skinned_forward_frames S(THROUGHPUT|COMPOSITE|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} SK(xyz - w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii - - - - null",
        f"sg_rasterize_backward_records_frames S(THROUGHPUT|COMPOSITE|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_skinned_backward_gaussians_frames S(THROUGHPUT|COMPOSITE|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} SK(xyz - w A smpl transl - - -) shs opacities scales radii geom binning {CAP} bwd_ws skin_ws 0 - - d_xyz|grad_flat - d_scales d_opacity d_sh d_means2D d_A d_transl null",
        f"sg_rasterize_backward_records_frames S(THROUGHPUT|COMPOSITE|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_skinned_backward_gaussians_frames S(THROUGHPUT|COMPOSITE|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} SK(xyz - w A smpl transl - - -) shs opacities scales radii geom binning {CAP} bwd_ws skin_ws 1 - - d_xyz|grad_flat - d_scales d_opacity d_sh d_means2D d_A d_transl null",
        f"sg_rasterize_backward_records_frames S(THROUGHPUT|COMPOSITE|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} geom binning {CAP} img bwd_ws dL null",
        f"sg_skinned_backward_gaussians_frames S(THROUGHPUT|COMPOSITE|SH_PLANAR|LONG_ROWS; {CAM}) FB(3,0,3) {P} SK(xyz - w A smpl transl - - -) shs opacities scales radii geom binning {CAP} bwd_ws skin_ws 1 - - d_xyz|grad_flat - d_scales d_opacity d_sh d_means2D d_A d_transl null",
        f"sg_read_num_rendered_frames binning {P} 64 48 {CAP} 3 nr[3] null",
        f"sg_skinned_forward_frames_aux S(WS_CLEAN|THROUGHPUT; {CAM}) FB(3,0,0) {P} SK(xyz - w A smpl transl - - -) shs opacities scales geom binning {CAP} img color radii - - - nr[3] aux_ws depth alpha null",
        f"sg_rasterize_backward_records_frames_aux S(WS_CLEAN|THROUGHPUT; {CAM}) FB(3,0,0) {P} geom binning {CAP} img bwd_ws dL aux_ws ddepth dalpha null",
        f"sg_skinned_backward_gaussians_frames_aux S(WS_CLEAN|THROUGHPUT; {CAM}) FB(3,0,0) {P} SK(xyz - w A smpl transl - - -) shs opacities scales radii geom binning {CAP} bwd_ws skin_ws 0 - - d_xyz|grad_flat - d_scales d_opacity d_sh d_means2D d_A d_transl aux_ws null",
    ],
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_c_calls_of_a_fixed_script(name):
    assert globals()["script_" + name]() == EXPECTED[name]


@pytest.mark.parametrize("kind", ["raster", "skinned", "raster_frames", "skinned_frames"])
def test_accumulate_reaches_the_per_gaussian_call(kind):
    """``backward(accumulate=True)`` adds to the gradient buffer on every engine, OR-ed with the answer of a ViewBatch chain."""
    for accumulate, chained in ((False, False), (True, False), (False, True), (True, True)):
        e, ins, cam, calls, g, dL = _ready(kind)
        e.set_camera(cam)
        if kind == "skinned":
            e.set_frame(ins["xyz"], None, ins["w"], ins["A"][0], ins["smpl"], ins["transl"][0])
        elif kind == "skinned_frames":
            e.set_frames(ins["xyz"], None, ins["w"], ins["A"], ins["smpl"], ins["transl"])
        e._chain = (lambda: (True, None, None)) if chained else None
        e.backward(*g, dL, accumulate=accumulate)
        assert "backward_gaussians" in calls[-1]
        assert re.search(r"(?:bwd_ws|skin_ws) (\d) ", calls[-1]).group(1) == str(int(accumulate or chained))
