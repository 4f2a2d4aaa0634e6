"""Finished 8-bit picture sheets on the device (include/sings_sheet.h, csrc/sg_sheet.hip): planar fp32 frames tiled in torchvision's
published ``make_grid`` layout, quantised and interleaved to HWC bytes in ONE launch.

What a training run writes is all this one operation (sings_amd/run_outputs.py): the training picture ``gt | pred``
(gs_trainer.py:443-449: two tiles, no padding, truncation), the validation grids (:588-591: one pair per sheet, padding 2, border 1),
the turntable frames (:838: one tile per sheet) and the progress sheet (:842: ``nrow=4``, border 0).  The host then copies a quarter of
the fp32 bytes, once per launch.  ``validate.comparison_grid`` and ``posed.frames_to_u8`` state two corners of it in torch ops and
stay as they are; tests/test_gpu_sheets.py ties the kernel to both.
"""
import torch

from . import _lib
from ._marshal import _ptr, _stream

QUANT = {"trunc": _lib.SHEET_TRUNC, "round": _lib.SHEET_ROUND}


def sheet_geometry(T, H, W, nrow=8, padding=2):
    """-> (Hs, Ws, xmaps, ymaps) of a sheet of ``T`` tiles [H,W]: ``xmaps = min(nrow, T)`` tiles per row, ``ymaps = ceil(T / xmaps)``
    rows, ``padding`` pixels around and between the tiles.  Tile t starts at row ``(t // xmaps) * (H + padding) + padding`` and column
    ``(t % xmaps) * (W + padding) + padding``.  Pure host arithmetic."""
    T, H, W, nrow, padding = int(T), int(H), int(W), int(nrow), int(padding)
    if T < 1 or H < 1 or W < 1 or nrow < 1 or padding < 0:
        raise ValueError(f"sheet_geometry: T, H, W, nrow >= 1 and padding >= 0 expected, got {(T, H, W, nrow, padding)}")
    xmaps = min(nrow, T)
    ymaps = -(-T // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, xmaps, ymaps


def image_sheets(a, b=None, tiles_per_sheet=None, nrow=8, padding=2, pad_value=0.0, quant="round", bgr=False, mask=None):
    """``a`` [F,3,H,W] (or [3,H,W]) fp32 frames on the GPU -> uint8 [S,Hs,Ws,3] on the GPU, one launch (``sg_image_sheets``).

    ``b`` None: ``tiles_per_sheet`` = T consecutive frames per sheet (default: all F in one sheet); F must be a multiple of T.
    ``b`` [F,3,H,W]: the pair form -- tile 2i of the run is frame i of ``a``, tile 2i + 1 frame i of ``b`` -- with T even (default
    2 F: one sheet; T = 2: one ``a | b`` sheet per frame).  ``quant``: "round" (``save_image``'s ``x * 255 + 0.5``, clamped) or "trunc"
    (``clamp(x, 0, 1) * 255``); NaN gives 0; ``pad_value`` is quantised by the same rule.  ``mask`` [F,H,W] fp32: frame i of either
    tensor is multiplied by row i before it is quantised.  ``bgr`` swaps the first and the third byte."""
    if not torch.is_tensor(a) or a.device.type != "cuda":
        raise RuntimeError("sings_amd.sheets.image_sheets runs on the MI355X only; there is no CPU fallback")
    if quant not in QUANT:
        raise ValueError(f"image_sheets: quant must be one of {sorted(QUANT)}, got {quant!r}")
    if a.dim() == 3:
        a = a.unsqueeze(0)
        b = b.unsqueeze(0) if torch.is_tensor(b) and b.dim() == 3 else b
        mask = mask.unsqueeze(0) if torch.is_tensor(mask) and mask.dim() == 2 else mask
    if a.dtype != torch.float32 or a.dim() != 4 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"image_sheets: fp32 [F,3,H,W] frames expected, got {a.dtype} {tuple(a.shape)}")
    F, H, W = int(a.shape[0]), int(a.shape[2]), int(a.shape[3])
    for name, t, shape in (("b", b, tuple(a.shape)), ("mask", mask, (F, H, W))):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.device != a.device or t.dtype != torch.float32:
            raise RuntimeError(f"image_sheets: {name} must be an fp32 tensor on {a.device} (no CPU fallback)")
        if tuple(t.shape) != shape:
            raise ValueError(f"image_sheets: {name} must be {list(shape)}, got {list(t.shape)}")
    tiles = F * (2 if b is not None else 1)
    T = tiles if tiles_per_sheet is None else int(tiles_per_sheet)
    if T < 1 or tiles % T or (b is not None and T % 2):
        raise ValueError(f"image_sheets: {tiles} tiles do not fill sheets of {T}" + (" (the pair form needs an even count)" if b is not None else ""))
    S = tiles // T
    Hs, Ws, _, _ = sheet_geometry(T, H, W, nrow, padding)
    a, b, mask = (None if t is None else t.contiguous() for t in (a, b, mask))
    out = torch.empty((S, Hs, Ws, 3), dtype=torch.uint8, device=a.device)
    lib = _lib.load()
    if not _lib.HAS_SHEET:
        raise RuntimeError("image_sheets: the loaded library predates include/sings_sheet.h (no fallback): rebuild it")
    with torch.cuda.device(a.device):
        _lib.check(lib.sg_image_sheets(S, T, W, H, int(nrow), int(padding), float(pad_value), QUANT[quant], int(bool(bgr)),
                                       _ptr(a), _ptr(b), _ptr(mask), _ptr(out), _stream(a.device)), "sg_image_sheets")
    return out
