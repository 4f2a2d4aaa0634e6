"""The sheet of include/sings_sheet.h restated in numpy: the geometry as the header writes it and both quantisation rules in
``np.float32`` arithmetic, one operation at a time (a multiply, an add, a clamp, a truncation).  What the GPU tests of
``sings_amd.sheets.image_sheets`` and of everything built on it compare bytes with."""
import numpy as np


def quantise(x, quant):
    """fp32 array -> uint8 by rule ``quant`` ("trunc" / "round"); NaN gives 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if quant == "trunc":
            v = np.minimum(np.maximum(np.where(np.isnan(x), np.float32(0), x), np.float32(0)), np.float32(1))
            v = (v * np.float32(255)).astype(np.float32)
        elif quant == "round":
            v = ((x * np.float32(255)).astype(np.float32) + np.float32(0.5)).astype(np.float32)
            v = np.minimum(np.maximum(np.where(np.isnan(v), np.float32(0), v), np.float32(0)), np.float32(255))
        else:
            raise ValueError(quant)
    return v.astype(np.uint8)                                    # (in 0..255: truncation toward zero)


def geometry(T, H, W, nrow, padding):
    xmaps = min(nrow, T)
    ymaps = (T + xmaps - 1) // xmaps
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, xmaps, ymaps


def sheets(a, b=None, tiles_per_sheet=None, nrow=8, padding=2, pad_value=0.0, quant="round", bgr=False, mask=None):
    """``sings_amd.sheets.image_sheets`` on numpy arrays: a [F,3,H,W], b None or [F,3,H,W], mask None or [F,H,W] -> uint8 [S,Hs,Ws,3]."""
    a = np.asarray(a, np.float32)
    F, _, H, W = a.shape
    tiles = F * (2 if b is not None else 1)
    T = tiles if tiles_per_sheet is None else tiles_per_sheet
    assert tiles % T == 0 and (b is None or T % 2 == 0)
    S = tiles // T
    Hs, Ws, xmaps, _ = geometry(T, H, W, nrow, padding)
    out = np.empty((S, Hs, Ws, 3), np.uint8)
    out[...] = quantise(np.float32(pad_value), quant)
    for s in range(S):
        for t in range(T):
            if b is None:
                f, src = s * T + t, a
            else:
                f, src = s * (T // 2) + t // 2, (a if t % 2 == 0 else np.asarray(b, np.float32))
            tile = src[f]
            if mask is not None:
                with np.errstate(invalid="ignore", over="ignore"):
                    tile = (tile * np.asarray(mask, np.float32)[f][None]).astype(np.float32)
            q = quantise(tile, quant).transpose(1, 2, 0)         # [H,W,3]
            if bgr:
                q = q[..., ::-1]
            y0, x0 = (t // xmaps) * (H + padding) + padding, (t % xmaps) * (W + padding) + padding
            out[s, y0:y0 + H, x0:x0 + W] = q
    return out


def planted(shape, seed):
    """fp32 frames over [-0.5, 1.5] with the values planted where the two rules and the special cases can be told apart: NaN, +-Inf,
    -0.0, exact multiples of 1/255 (where TRUNC steps) and of 1/510 (where ROUND steps)."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-0.5, 1.5, size=shape).astype(np.float32)
    flat = x.reshape(-1)
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0] + [k / 255 for k in (1, 2, 127, 128, 254, 255)] + \
              [k / 510 for k in (1, 3, 255, 257, 509)]
    pos = rs.permutation(flat.size)[:len(special)] if flat.size >= len(special) else np.arange(flat.size)
    for p, v in zip(pos, special):
        flat[p] = np.float32(v)
    return x
