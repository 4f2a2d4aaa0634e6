"""Host tests of the evaluation boundary (include/sings_eval.h, ``_lib._PROTOTYPES_EVAL``), of ``comparison_grid`` and of the metrics
golden: the second header is held to its table the way tests/test_abi.py holds the first, each status-returning entry point is
refused once before any HIP call, and the table of the render path (``EXPORTS``, the ABI number) is what it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sings_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_golden.npz")

# One refused call per status-returning entry point: every argument 0 / NULL, and the text.
REFUSED_EVAL = {
    "sg_image_metrics_frames": "sg_image_metrics_frames: K must be 1..65535",
}


def _header(repo_root):
    hdr = open(os.path.join(repo_root, "include", "sings_eval.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return re.sub(r"//[^\n]*", "", hdr)


def test_eval_header_is_bound_with_its_types(repo_root):
    """Every ``int | size_t | const char * sg_x(...)`` of include/sings_eval.h against the argtypes / restype the LOADED library
    carries (test_abi.py's parser and type classes), and the header's functions are exactly the table's."""
    hdr = _header(repo_root)
    assert re.search(r'#include\s+"sings_hip.h"', open(os.path.join(repo_root, "include", "sings_eval.h")).read())
    protos = re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert protos and len({n for _, n, _ in protos}) == len(protos)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_EVAL)
    assert not set(_lib._PROTOTYPES_EVAL) & set(_lib._PROTOTYPES)
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


def test_eval_constants_match_the_header(repo_root):
    hdr = open(os.path.join(repo_root, "include", "sings_eval.h")).read()
    for name in ("CLAMP", "FLOATS", "STRIP_COLS", "CHUNK_ROWS"):
        m = re.search(r"#define SG_METRICS_%s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, "METRICS_" + name), name
    from sings_amd import metrics
    assert (metrics.STRIP_COLS, metrics.CHUNK_ROWS) == (_lib.METRICS_STRIP_COLS, _lib.METRICS_CHUNK_ROWS)


def test_the_render_path_table_is_untouched(repo_root):
    assert _lib.EXPORTS == tuple(_lib._PROTOTYPES)
    assert _lib.ABI_VERSION == 8 and _lib.load().sg_abi_version() == 8
    main = open(os.path.join(repo_root, "include", "sings_hip.h")).read()
    assert "sg_image_metrics" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)


def test_the_refusal_table_covers_every_status_returning_eval_entry_point():
    assert set(REFUSED_EVAL) == {n for n, sig in _lib._PROTOTYPES_EVAL.items() if sig.startswith("i:")}


@pytest.mark.parametrize("name", sorted(REFUSED_EVAL))
def test_eval_refusal_status_and_text(name):
    lib = _lib.load()
    _, argtypes = _lib._ctypes_of(_lib._PROTOTYPES_EVAL[name])
    args = [0.0 if t is C.c_float else 0 if t in (C.c_int, C.c_size_t) else None for t in argtypes]
    assert getattr(lib, name)(*args) == 1
    assert lib.sg_last_error().decode() == REFUSED_EVAL[name] + ": invalid argument"


def test_image_metrics_refusals_in_order_and_workspace_sizes():
    """Each refusal the header lists, before any HIP call (no GPU here): sizes, flags, pointers, a stride without a mask."""
    lib = _lib.load()
    f = C.c_void_p(0x1000)                                           # never dereferenced
    call = lambda K=1, W=8, H=5, flags=1, pred=f, gt=f, gs=0, mask=None, ms=0, ws=f, out=f: (
        lib.sg_image_metrics_frames(K, W, H, flags, pred, gt, gs, mask, ms, ws, out, None), lib.sg_last_error().decode())
    for kw, text in (({"K": 0}, "K must be 1..65535"), ({"K": 65536}, "K must be 1..65535"),
                     ({"W": 0}, "width and height must be >= 1 (and fewer than 2^30 pixels)"),
                     ({"H": -3}, "width and height must be >= 1 (and fewer than 2^30 pixels)"),
                     ({"W": 1 << 15, "H": 1 << 15}, "width and height must be >= 1 (and fewer than 2^30 pixels)"),
                     ({"flags": 2}, "unknown flag bits 0x2"), ({"flags": -2}, "unknown flag bits 0xfffffffe"),
                     ({"pred": None}, "null pointer"), ({"gt": None}, "null pointer"), ({"ws": None}, "null pointer"),
                     ({"out": None}, "null pointer"), ({"ms": 40}, "mask_stride without a mask")):
        rc, err = call(**kw)
        assert rc == 1 and err == f"sg_image_metrics_frames: {text}: invalid argument", (kw, err)
    ws = lib.sg_image_metrics_ws_bytes
    assert ws(0, 8, 5) == 0 and ws(1, 0, 5) == 0 and ws(65536, 8, 5) == 0 and ws(1, 1 << 15, 1 << 15) == 0
    one = ws(1, 1920, 1080)
    assert one > 0 and one % 256 == 0 and ws(8, 1920, 1080) == 8 * one                # K consecutive single-frame workspaces
    # one 16-byte pair per (channel, strip, chunk): a strip more / a chunk more at the constants' edges
    S, R = _lib.METRICS_STRIP_COLS, _lib.METRICS_CHUNK_ROWS
    assert ws(1, S, R) == 256 and ws(1, S + 1, R) == 256 and ws(1, 6 * S, R) == 512 and ws(1, 6 * S, R + 1) == 768


def test_host_tensors_and_grad_inputs_are_refused():
    from sings_amd.metrics import MetricsEngine, image_metrics
    from sings_amd.validate import Validator
    x = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_metrics(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MetricsEngine(8, 8, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Validator(8, 8, "cpu")
    with pytest.raises(RuntimeError, match="not differentiable"):
        image_metrics(x.clone().requires_grad_(True), x)


def test_comparison_grid_geometry():
    """torchvision.utils.make_grid([gt, image], nrow=2, pad_value=1) with its default padding of 2: [3, H + 4, 2 W + 6]."""
    from sings_amd.validate import comparison_grid
    H, W = 7, 5
    g = torch.Generator().manual_seed(1)
    gt, pred = torch.rand(3, H, W, generator=g) * 0.9, torch.rand(3, H, W, generator=g) * 0.9       # (< 1: distinct from the padding)
    grid = comparison_grid(gt, pred)
    assert grid.shape == (3, H + 4, 2 * W + 6) and grid.dtype == torch.float32 and grid.device == gt.device
    assert torch.equal(grid[:, 2:H + 2, 2:W + 2], gt) and torch.equal(grid[:, 2:H + 2, W + 4:2 * W + 4], pred)
    outside = torch.ones(H + 4, 2 * W + 6, dtype=torch.bool)
    outside[2:H + 2, 2:W + 2] = False
    outside[2:H + 2, W + 4:2 * W + 4] = False
    assert int(outside.sum()) == (H + 4) * (2 * W + 6) - 2 * H * W
    assert bool((grid[:, outside] == 1).all())
    with pytest.raises(ValueError):
        comparison_grid(gt, pred[:, :-1])


def test_golden_is_self_consistent_and_pins_the_per_channel_rule():
    """The stored mean PSNR is the fp32 mean of the stored channel PSNRs (+inf where a channel is exact), the stored PSNRs follow from
    the stored MSEs, and in at least one case the figure is far from the PSNR of the whole-image MSE."""
    G = np.load(GOLDEN)
    cases = [str(c) for c in G["cases"]]
    assert cases == ["a", "b", "c", "zju", "exact"] and list(G["masked"]) == [False, False, False, True, False]
    far = 0
    for tag in cases:
        mse, psnr, mean = G[f"{tag}_mse"], G[f"{tag}_psnr"], G[f"{tag}_psnr_mean"]
        assert mse.dtype == np.float32 and psnr.shape == (3,) and G[f"{tag}_raw"].shape == G[f"{tag}_gt"].shape
        assert (f"{tag}_mask" in G) == (tag == "zju")
        assert 0 <= float(G[f"{tag}_psnr_ref_err"]) < 5e-6
        if tag == "exact":
            assert mse[1] == 0 and np.isposinf(psnr[1]) and np.isposinf(mean) and np.isfinite(psnr[[0, 2]]).all()
            assert np.array_equal(G["exact_raw"][1], G["exact_gt"][1])
            continue
        assert abs(float(mean) - float(psnr.astype(np.float64).mean())) <= 2 * np.spacing(np.float32(mean))
        assert np.abs(psnr - 20 * np.log10(1 / np.sqrt(mse.astype(np.float64)))).max() <= 4 * np.spacing(np.float32(psnr.max()))
        whole = 20 * np.log10(1 / np.sqrt(mse.astype(np.float64).mean()))
        far += abs(float(mean) - whole) > 1.0
    assert far >= 1
    assert G["a_raw"].min() < 0 and G["a_raw"].max() > 1                       # the clamp works on both sides
    assert ((G["zju_mask"] > 0) & (G["zju_mask"] < 1)).any()                   # a soft mask
