"""Host tests of the mesh-terms boundary (include/sings_mesh_terms.h, ``_lib._PROTOTYPES_MESH_TERMS``) and of ``lap_weights``: the third
header is held to its table the way tests/test_metrics_host.py holds the second, each status-returning entry point is refused once
before any HIP call, and the tables of the render path and of the evaluation path (``EXPORTS``, the ABI number) are what they were."""
import ctypes as C
import os
import re

import pytest

from sings_amd import _lib

# One refused call per status-returning entry point: every argument 0 / NULL, and the text.
REFUSED = {
    "sg_mesh_terms_build": "sg_mesh_terms_build: V must be 1..2^30",
    "sg_mesh_terms": "sg_mesh_terms: V must be 1..2^30",
}


def _header(repo_root):
    hdr = open(os.path.join(repo_root, "include", "sings_mesh_terms.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return re.sub(r"//[^\n]*", "", hdr)


def test_header_is_bound_with_its_types(repo_root):
    """Every ``int | size_t | const char * sg_x(...)`` of include/sings_mesh_terms.h against the argtypes / restype the LOADED library
    carries, and the header's functions are exactly the table's, in order."""
    hdr = _header(repo_root)
    assert re.search(r'#include\s+"sings_hip.h"', open(os.path.join(repo_root, "include", "sings_mesh_terms.h")).read())
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert protos and len({n for _, n, _ in protos}) == len(protos)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_MESH_TERMS)
    assert not set(_lib._PROTOTYPES_MESH_TERMS) & (set(_lib._PROTOTYPES) | set(_lib._PROTOTYPES_EVAL))
    pointer_bases = (C._Pointer, C.c_void_p, C.c_char_p)
    scalars = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    lib = _lib.load()
    bad = []
    for ret, name, params in protos:
        fn = getattr(lib, name)
        want_ret = {"int": C.c_int, "size_t": C.c_size_t}.get(ret, C.c_char_p)
        if fn.restype is not want_ret:
            bad.append(f"{name}: restype {fn.restype}, the header returns {ret}")
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        argtypes = fn.argtypes or ()
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(argtypes)} argtypes, the header has {len(params)} parameters")
            continue
        for i, (p, t) in enumerate(zip(params, argtypes)):
            if "*" in p or "[" in p:
                ok = issubclass(t, pointer_bases)
            else:
                words = [w for w in re.findall(r"\w+", p) if w not in ("const", "unsigned")]
                ok = t is scalars.get(words[0])
            if not ok:
                bad.append(f"{name}: parameter {i} `{p}` is bound as {t}")
    assert not bad, "\n".join(bad)


def test_constants_match_the_header(repo_root):
    hdr = open(os.path.join(repo_root, "include", "sings_mesh_terms.h")).read()
    for name in ("INFO_INTS", "BAD_LABEL", "BAD_EDGE"):
        m = re.search(r"#define SG_MESH_TERMS_%s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, "MESH_TERMS_" + name), name


def test_the_other_tables_are_untouched(repo_root):
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES)
    assert _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    assert list(_lib._PROTOTYPES_EVAL) == ["sg_image_metrics_ws_bytes", "sg_image_metrics_frames"]
    for other in ("sings_hip.h", "sings_eval.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", other)).read(), flags=re.S)
        assert "sg_mesh_terms" not in text, other


def test_the_refusal_table_covers_every_status_returning_entry_point():
    assert set(REFUSED) == {n for n, sig in _lib._PROTOTYPES_MESH_TERMS.items() if sig.startswith("i:")}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusal_status_and_text(name):
    lib = _lib.load()
    _, argtypes = _lib._ctypes_of(_lib._PROTOTYPES_MESH_TERMS[name])
    args = [0.0 if t is C.c_float else 0 if t in (C.c_int, C.c_size_t) else None for t in argtypes]
    assert getattr(lib, name)(*args) == 1
    assert lib.sg_last_error().decode() == REFUSED[name] + ": invalid argument"


def test_refusals_in_order():
    """Each refusal the header lists, before any HIP call (no GPU here): sizes, the colour stride, pointers."""
    lib = _lib.load()
    f = C.c_void_p(0x1000)                                           # never dereferenced
    build = lambda V=4, E=3, L=2, edges=f, label=f, wp=f, wc=f, wh=f, rp=f, col=f, di=f, cnt=f, vs=f, dws=f, info=f: (
        lib.sg_mesh_terms_build(V, E, L, edges, label, wp, wc, wh, rp, col, di, cnt, vs, dws, info, None), lib.sg_last_error().decode())
    for kw, text in (({"V": 0}, "V must be 1..2^30"), ({"V": (1 << 30) + 1}, "V must be 1..2^30"), ({"E": -1}, "E must be 0..2^30 - 1"),
                     ({"E": 1 << 30}, "E must be 0..2^30 - 1"), ({"L": 0}, "L must be >= 1"), ({"edges": None}, "null pointer"),
                     ({"col": None}, "null pointer"), ({"rp": None}, "null pointer"), ({"di": None}, "null pointer"),
                     ({"dws": None}, "null pointer"), ({"info": None}, "null pointer"), ({"wp": None}, "null pointer"),
                     ({"wc": None}, "null pointer"), ({"wh": None}, "null pointer"), ({"cnt": None}, "null pointer"),
                     ({"vs": None}, "null pointer")):
        rc, err = build(**kw)
        assert rc == 1 and err == f"sg_mesh_terms_build: {text}: invalid argument", (kw, err)
    terms = lambda V=4, x=f, s=f, n=f, c=f, stride=48, rp=f, col=f, di=f, vs=f, tw=f, ws=f, g=f, out=f: (
        lib.sg_mesh_terms(V, x, s, n, c, stride, rp, col, di, vs, tw, ws, g, out, None, f, f, f, None), lib.sg_last_error().decode())
    for kw, text in (({"V": 0}, "V must be 1..2^30"), ({"V": (1 << 30) + 1}, "V must be 1..2^30"),
                     ({"stride": 2}, "the colour rows are at least 3 floats apart"),
                     *(({k: None}, "null pointer") for k in ("x", "s", "n", "c", "rp", "col", "di", "vs", "tw", "ws", "g", "out"))):
        rc, err = terms(**kw)
        assert rc == 1 and err == f"sg_mesh_terms: {text}: invalid argument", (kw, err)


@pytest.mark.parametrize("t,alpha", [(0, 0.0), (1000, 0.0), (1001, 1.0), (1500, 500.0), (2000, 1000.0), (8001, 1000.0)])
def test_lap_weights_ramp(t, alpha):
    """gs_trainer.py:376-383 with position_strength 1000 from iteration 1000: nothing up to and INCLUDING the start, linear over the next
    1000 iterations, flat from there; no doubling past 8000 (the reference's ``alpha *= 2`` runs after the terms are formed)."""
    from sings_amd.mesh_terms import lap_weights
    assert lap_weights(t, 1000.0, 10.0, 1000) == (alpha, 10.0, 1e-5)


def test_a_start_of_zero_is_refused():
    from sings_amd.mesh_terms import MeshTerms, lap_weights
    with pytest.raises(ValueError, match="impose_from_iter"):
        lap_weights(5, 1000.0, 10.0, 0)
    with pytest.raises(ValueError, match="impose_from_iter"):
        MeshTerms([1.0] * 8, [1.0] * 8, 1.0, 1000.0, 10.0, 0)
    with pytest.raises(ValueError, match="impose_from_iter"):
        MeshTerms([1.0] * 8, [1.0] * 8, 1.0, 1000.0, 10.0, -3)
