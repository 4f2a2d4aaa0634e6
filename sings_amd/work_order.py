"""The work order of a K-camera launch (include/sings_order.h): lane i of the per-Gaussian kernels works on Gaussian ``order[i]``.

``build_order`` is the device builder (Morton codes by ``sg_work_order_codes``, one stable ``torch.sort``): a pure function of the
positions, off the hot path -- ``RasterFramesEngine`` builds it once and keeps it.  ``morton_codes_host`` / ``order_host`` are its
numpy twin, the same fp32 arithmetic operation for operation, for tests and for the census below.  ``window_census`` counts, from
tile rectangles alone, what an order does to the preprocess: distinct (workgroup, tile) pairs and the tile windows of the workgroups.
"""
import ctypes as C

import numpy as np

from . import _lib


def morton_codes_host(xyz):
    """The codes ``sg_work_order_codes`` computes ([P] uint32), in the same fp32 steps."""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    if x.shape[0] == 0:
        return np.zeros(0, np.uint32)
    with np.errstate(all="ignore"):
        lo, hi = np.fmin.reduce(x, axis=0), np.fmax.reduce(x, axis=0)
        ext = np.fmax(hi - lo, np.float32(1e-12)).astype(np.float32)
        q = (x - lo).astype(np.float32) * (np.float32(1023.0) / ext).astype(np.float32)
        cell = np.where(q >= np.float32(1023.0), np.float32(1023.0), np.where(q > 0, q, np.float32(0))).astype(np.uint32)
    code = np.zeros(x.shape[0], np.uint32)
    for k in range(3):
        for b in range(_lib.ORDER_CODE_BITS):
            code |= ((cell[:, k] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + k)
    return code


def order_host(xyz):
    """Stable sort of (code, index): the permutation ``build_order`` returns, as int32."""
    return np.argsort(morton_codes_host(xyz), kind="stable").astype(np.int32)


def build_order(means3D):
    """The Morton order of ``means3D`` [P,3] (fp32, on the GPU) as an int32 tensor [P].  Two small launches and one sort; nothing
    synchronises with the host."""
    import torch
    from ._marshal import _ptr, _stream
    if means3D.dtype != torch.float32 or means3D.dim() != 2 or means3D.shape[1] != 3 or not means3D.is_cuda:
        raise ValueError("build_order: means3D must be an fp32 [P,3] tensor on the GPU")
    m = means3D.detach().contiguous()
    P = m.shape[0]
    codes = torch.empty(P, dtype=torch.int32, device=m.device)
    ws = torch.empty(_lib.ORDER_WS_BYTES, dtype=torch.uint8, device=m.device)
    _lib.check(_lib.load().sg_work_order_codes(P, _ptr(m), C.c_void_p(ws.data_ptr()), _ptr(codes), _stream(m.device)),
               "sg_work_order_codes")
    return torch.sort(codes, stable=True)[1].to(torch.int32)         # (codes are 30-bit: the sign bit is clear)


def check_order(order, P, device):
    """A caller's order for an engine of P Gaussians on ``device``: int32 / uint32-as-int32 [P], contiguous."""
    import torch
    if not torch.is_tensor(order) or order.dtype != torch.int32 or order.dim() != 1 or not order.is_contiguous():
        raise ValueError("order must be a contiguous int32 tensor [P]")
    if order.numel() != P:
        raise ValueError(f"order has {order.numel()} entries, the engine {P} Gaussians")
    if order.device != device:
        raise ValueError(f"order is on {order.device}, the engine on {device}")
    return order


def order_applies(W, H, flags):
    """Where an order takes effect (sg_order_applies): a directly binned frame of many tiles."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return bool(flags & _lib.FLAG_SHORT_LISTS) and ((gx + 3) // 4) * ((gy + 3) // 4) * 16 > _lib.HIST_TILES_MAX


def window_census(rect_min, rect_max, order=None):
    """``rect_min`` / ``rect_max`` [P,2] (x, y) tile rectangles, max exclusive (an empty rectangle: no pairs).  Workgroups are
    ``ORDER_BLOCK`` consecutive positions of ``order`` (None: the input order).  Returns ``pairs`` (all (tile, Gaussian) pairs),
    ``group_tiles`` (distinct (workgroup, tile) pairs) and ``windows`` (tiles in the bounding box of each workgroup's rectangles;
    0 for a workgroup without pairs)."""
    mn, mx = np.asarray(rect_min, np.int64), np.asarray(rect_max, np.int64)
    if order is not None:
        o = np.asarray(order, np.int64)
        mn, mx = mn[o], mx[o]
    P, B = mn.shape[0], _lib.ORDER_BLOCK
    w, h = np.maximum(mx[:, 0] - mn[:, 0], 0), np.maximum(mx[:, 1] - mn[:, 1], 0)
    area = w * h
    pairs, group_tiles, windows = int(area.sum()), 0, []
    for b0 in range(0, P, B):
        sel = np.nonzero(area[b0:b0 + B])[0] + b0
        if sel.size == 0:
            windows.append(0)
            continue
        x0, y0, x1, y1 = mn[sel, 0].min(), mn[sel, 1].min(), mx[sel, 0].max(), mx[sel, 1].max()
        windows.append(int((x1 - x0) * (y1 - y0)))
        seen = np.zeros((y1 - y0, x1 - x0), bool)
        for i in sel:
            seen[mn[i, 1] - y0:mx[i, 1] - y0, mn[i, 0] - x0:mx[i, 0] - x0] = True
        group_tiles += int(seen.sum())
    return {"pairs": pairs, "group_tiles": group_tiles, "windows": np.asarray(windows, np.int64)}
