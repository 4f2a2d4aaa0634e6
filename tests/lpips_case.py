"""fp64 oracle of LPIPS-VGG (the `lpips` 0.1 package, net='vgg', version='0.1', eval mode) restated with torch functional ops,
weights drawn from a seeded RandomState at the VGG16 shapes (He-scaled: no 59 MB weight file), a stand-in module with
`lpips.LPIPS`'s attribute structure, and the deterministic inputs of the patch-loss golden (tests/golden/gen_lpips_golden.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from sings_amd.lpips import CONV_CHANNELS, LIN_CHANNELS, SLICE_CONVS

SHIFT = (-.030, -.088, -.188)                                  # lpips.pretrained_networks ScalingLayer
SCALE = (.458, .448, .450)


def make_weights(seed=0, conv5_3_bias=None):
    """-> dict(convs=[(W, b)] * 13 float32 tensors, lins=[[1,C,1,1]] * 5, shift, scale [1,3,1,1])."""
    rs = np.random.RandomState(seed)
    convs = []
    for ci, co in CONV_CHANNELS:
        w = rs.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))
        b = rs.standard_normal(co) * 0.05
        convs.append((torch.from_numpy(w.astype(np.float32)), torch.from_numpy(b.astype(np.float32))))
    if conv5_3_bias is not None:
        w, b = convs[12]
        convs[12] = (w, torch.full_like(b, float(conv5_3_bias)))
    lins = [torch.from_numpy((rs.uniform(0, 1, c) / np.sqrt(c)).astype(np.float32)).reshape(1, c, 1, 1) for c in LIN_CHANNELS]
    return {"convs": convs, "lins": lins, "shift": torch.tensor(SHIFT, dtype=torch.float32).reshape(1, 3, 1, 1),
            "scale": torch.tensor(SCALE, dtype=torch.float32).reshape(1, 3, 1, 1)}


def features(wt, x):
    """The five slice outputs (relu1_2 .. relu5_3) of the scaled input, in the dtype of ``x``."""
    outs, l = [], 0
    for k, n in enumerate(SLICE_CONVS):
        if k > 0:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(n):
            w, b = wt["convs"][l]
            x = F.relu(F.conv2d(x, w.to(x.dtype), b.to(x.dtype), padding=1))
            l += 1
        outs.append(x)
    return outs


def lpips_ref(wt, in0, in1, normalize=False, dtype=torch.float64):
    """lpips.LPIPS.forward (version 0.1, no spatial output) -> [B,1,1,1] in ``dtype``; differentiable w.r.t. in0 / in1."""
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    sh, sc = wt["shift"].to(dtype), wt["scale"].to(dtype)
    f0 = features(wt, (in0.to(dtype) - sh) / sc)
    f1 = features(wt, (in1.to(dtype) - sh) / sc)
    val = 0
    for k in range(5):
        n0 = f0[k] / (torch.sqrt(torch.sum(f0[k] ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = f1[k] / (torch.sqrt(torch.sum(f1[k] ** 2, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((n0 - n1) ** 2, wt["lins"][k].to(dtype))
        val = val + d.mean([2, 3], keepdim=True)
    return val


class _Scaling(torch.nn.Module):
    def __init__(self, shift, scale):
        super().__init__()
        self.register_buffer("shift", shift.clone())
        self.register_buffer("scale", scale.clone())


class _Lin(torch.nn.Module):
    def __init__(self, w):
        super().__init__()
        conv = torch.nn.Conv2d(w.shape[1], 1, 1, bias=False)
        conv.weight.data.copy_(w)
        self.model = torch.nn.Sequential(torch.nn.Dropout(), conv)


class _Vgg(torch.nn.Module):
    def __init__(self, convs):
        super().__init__()
        l = 0
        for k, n in enumerate(SLICE_CONVS):
            layers = [torch.nn.MaxPool2d(2, 2)] if k > 0 else []
            for _ in range(n):
                w, b = convs[l]
                c = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
                c.weight.data.copy_(w); c.bias.data.copy_(b)
                layers += [c, torch.nn.ReLU(inplace=False)]
                l += 1
            setattr(self, f"slice{k + 1}", torch.nn.Sequential(*layers))


class StandInLPIPS(torch.nn.Module):
    """The attribute structure of ``lpips.LPIPS(net='vgg')`` (net.slice1..5, lin0..4.model[-1], scaling_layer.shift / .scale) over
    the oracle's weights; calling it runs the fp64 oracle."""

    def __init__(self, wt):
        super().__init__()
        self.wt = wt
        self.scaling_layer = _Scaling(wt["shift"], wt["scale"])
        self.net = _Vgg(wt["convs"])
        for k in range(5):
            setattr(self, f"lin{k}", _Lin(wt["lins"][k]))

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        return lpips_ref(self.wt, in0, in1, normalize)


def golden_inputs(seed, H=96, W=80):
    """The deterministic inputs of a patch-loss golden case: raw (outside [0,1] on both sides), gt rgb, a soft mask, bg [3]."""
    rs = np.random.RandomState(1000 + seed)
    raw = rs.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
    gt = rs.uniform(0, 1, (3, H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((xx - W / 2) / (W / 2.5)) ** 2 + ((yy - H / 2) / (H / 2.2)) ** 2 < 1).astype(np.float32)
    mask[rs.uniform(size=mask.shape) < 0.1] = 0.5
    bg = rs.uniform(0, 1, 3).astype(np.float32)
    return raw, gt, mask, bg


def patch_loss_ref(wt, raw, gt_rgb, mask, bg, bg_rand, origins, P, lpips_w):
    """loss.py:71-80 with the oracle LPIPS (fp64 inside); raw [3,H,W] float32 requiring grad -> 0-dim loss."""
    m = mask.reshape(1, *mask.shape[-2:])
    pred = torch.clamp(raw, 0.0, 1.0)
    gt_img = gt_rgb * m + bg.reshape(3, 1, 1) * (1. - m)
    image_bg = pred * m + bg_rand * (1. - m)
    gt_bg = gt_img * m + bg_rand * (1. - m)
    pp = torch.stack([image_bg[:, x:x + P, y:y + P] for x, y in origins.tolist()], 0)
    gp = torch.stack([gt_bg[:, x:x + P, y:y + P] for x, y in origins.tolist()], 0)
    return lpips_w * lpips_ref(wt, pp.clip(max=1), gp).mean()


# ---- the kernel's own forward state (sg_lpips_ws_layout) and an fp64 reference pinned to it -------------------------------------
# The forward keeps every conv output, every pool output with its argmax code and the per-pixel head terms in its workspace.
# Given those, each conv can be checked on its own input (no round-off compounds across layers), and the backward is a fixed
# linear map -- the kernel's ReLU masks and pool choices, fp64 arithmetic -- that a correct fp32 kernel must match per element.
LEVEL = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)                # conv l's level (H_v = floor(H / 2^v))
SLICE_LAYER = (1, 3, 6, 9, 12)                                  # relu1_2 .. relu5_3
POOL_CH = (64, 128, 256, 512)
CONV_TOL = 1e-5                                                 # |delta| <= CONV_TOL (|b| + conv(|x|, |W|)) per conv output
HEAD_TOL = 1e-5                                                 # |delta| <= HEAD_TOL sum_c |lin_c| (|n0_c| + |n1_c|)^2 per pixel
OUT_TOL = 1e-5                                                  # out[b] relative to sum_k mean(dpix_k[b])


def level_sizes(H, W):
    hs, ws = [H], [W]
    for _ in range(4):
        hs.append(hs[-1] // 2); ws.append(ws[-1] // 2)
    return hs, ws


def read_state(ws, layout, B, H, W, out=None, device="cpu"):
    """The forward's workspace ``ws`` (a uint8 tensor) read through ``layout`` (sings_amd.lpips.ws_layout) as fp64 tensors on
    ``device`` in NCHW: y [13] [2B,Cout,H_v,W_v], pool [4], arg [4] (int64 codes (dy << 1) | dx), dpix [5] [B,H_k,W_k]; ``out``
    (the forward's [B] values) is kept as well when given."""
    hs, wd = level_sizes(H, W)
    NI = 2 * B

    def piece(off, shape, dtype=torch.float32):
        n = int(np.prod(shape)) * (4 if dtype == torch.float32 else 1)
        return ws[off:off + n].to(device).view(dtype).reshape(shape)

    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    st = {"B": B, "H": H, "W": W,
          "y": [nchw(piece(layout["y"][l], (NI, hs[v], wd[v], CONV_CHANNELS[l][1]))).double() for l, v in enumerate(LEVEL)],
          "pool": [nchw(piece(layout["pool"][q], (NI, hs[q + 1], wd[q + 1], POOL_CH[q]))).double() for q in range(4)],
          "arg": [nchw(piece(layout["arg"][q], (NI, hs[q + 1], wd[q + 1], POOL_CH[q]), torch.uint8)).long() for q in range(4)],
          "dpix": [piece(layout["dpix"][k], (B, hs[k], wd[k])).double() for k in range(5)]}
    if out is not None:
        st["out"] = out.detach().to(device).double().reshape(-1)
    return st


def oracle_state(wt, in0, in1, normalize=False, dtype=torch.float64):
    """The state of the oracle's own forward in ``dtype`` (fp64 CPU: self-consistency; fp32: a correct fp32 implementation), in
    read_state's form and fp64.  Each input goes through the network on its own, as lpips_ref does, so the bits are its bits."""
    sh, sc = wt["shift"].to(dtype), wt["scale"].to(dtype)
    parts = []
    for x in (in0, in1):
        if normalize:
            x = 2 * x - 1
        h = (x.to(dtype) - sh) / sc
        y, pool, arg = [], [], []
        for l, (w, b) in enumerate(wt["convs"]):
            if l and LEVEL[l] != LEVEL[l - 1]:
                Wi = h.shape[3]
                h, idx = F.max_pool2d(h, 2, 2, return_indices=True)
                pool.append(h); arg.append(((idx // Wi) % 2) * 2 + (idx % Wi) % 2)
            h = F.relu(F.conv2d(h, w.to(dtype), b.to(dtype), padding=1))
            y.append(h)
        parts.append((y, pool, arg))
    (y0, p0, a0), (y1, p1, a1) = parts
    dpix, out = [], 0
    for k in range(5):
        f0, f1 = y0[SLICE_LAYER[k]], y1[SLICE_LAYER[k]]
        n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((n0 - n1) ** 2, wt["lins"][k].to(dtype))
        dpix.append(d[:, 0])
        out = out + d.mean([2, 3]).reshape(-1)
    cat = lambda a, b: torch.cat([a, b]).double()
    return {"B": in0.shape[0], "H": in0.shape[2], "W": in0.shape[3], "y": [cat(a, b) for a, b in zip(y0, y1)],
            "pool": [cat(a, b) for a, b in zip(p0, p1)], "arg": [torch.cat([a, b]) for a, b in zip(a0, a1)],
            "dpix": [d.double() for d in dpix], "out": out.double()}


def _worst(what, err, bound, labels):
    """-> (worst ratio |err| / bound, a message naming the worst element by ``labels`` of err's dimensions)."""
    r = torch.where(err == 0, torch.zeros_like(err), err.abs() / bound)
    i = int(torch.argmax(torch.nan_to_num(r, nan=float("inf"))))
    idx = np.unravel_index(i, tuple(r.shape))
    ratio = float(r.reshape(-1)[i])
    where = ", ".join(f"{n} {int(v)}" for n, v in zip(labels, idx))
    return ratio, (f"{what}: worst at {where}: |delta| {float(err.abs().reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e}, "
                   f"ratio {ratio:.3g}")


def _scaled(wt, x, normalize, dev):
    x = x.to(dev, torch.float64)
    if normalize:
        x = 2 * x - 1
    return (x - wt["shift"].to(dev, torch.float64)) / wt["scale"].to(dev, torch.float64)


def check_layers(wt, in0, in1, normalize, state):
    """Every conv against an fp64 conv of the kernel's own input to it, every pool exactly, every head term and ``out`` against fp64
    of the kernel's own slice features.  -> dict of the worst ratios to the bounds (conv [13], pool [4] mismatching elements,
    head [5], out); raises AssertionError listing every check that fails, each naming its worst element."""
    dev = state["y"][0].device
    B = state["B"]
    f64 = lambda t: t.to(dev, torch.float64)
    xs = torch.cat([_scaled(wt, in0, normalize, dev), _scaled(wt, in1, normalize, dev)])
    res, fails = {"conv": [], "pool": [], "head": []}, []
    for l, (w, b) in enumerate(wt["convs"]):
        if l == 0:
            x = xs
        elif LEVEL[l] != LEVEL[l - 1]:
            q = LEVEL[l] - 1
            src, p, a = state["y"][SLICE_LAYER[q]], state["pool"][q], state["arg"][q]
            Ho, Wo = p.shape[2], p.shape[3]
            win = torch.stack([src[:, :, dy:2 * Ho:2, dx:2 * Wo:2] for dy in (0, 1) for dx in (0, 1)])
            best, code = win[0], torch.zeros_like(a)
            for c in (1, 2, 3):                                 # first maximum in row-major window order (torch's rule)
                take = (win[c] > best) | torch.isnan(win[c])
                best = torch.where(take, win[c], best); code = torch.where(take, torch.full_like(code, c), code)
            named = torch.gather(win, 0, a.clamp(0, 3).unsqueeze(0))[0]
            bad = (a != code) | (p != named) | (p != best)
            res["pool"].append(int(bad.sum()))
            if bad.any():
                n, c, yy, xx = (int(v) for v in bad.nonzero()[0])
                fails.append(f"pool {q}: {int(bad.sum())} elements wrong, first at image {n}, channel {c}, pixel ({yy}, {xx}): "
                             f"value {float(p[n, c, yy, xx])!r} code {int(a[n, c, yy, xx])}, expected {float(best[n, c, yy, xx])!r} "
                             f"code {int(code[n, c, yy, xx])}")
            x = p
        else:
            x = state["y"][l - 1]
        w, b = f64(w), f64(b)
        ref = F.relu(F.conv2d(x, w, b, padding=1))
        bound = CONV_TOL * (b.abs().reshape(1, -1, 1, 1) + F.conv2d(x.abs(), w.abs(), padding=1))
        ratio, msg = _worst(f"conv {l}", state["y"][l] - ref, bound, ("image", "channel", "row", "column"))
        res["conv"].append(ratio)
        if not ratio <= 1:
            fails.append(msg)
    total = 0
    for k in range(5):
        f = state["y"][SLICE_LAYER[k]]
        lin = f64(wt["lins"][k]).reshape(1, -1, 1, 1)
        n0 = f[:B] / (torch.sqrt((f[:B] ** 2).sum(1, keepdim=True)) + 1e-10)
        n1 = f[B:] / (torch.sqrt((f[B:] ** 2).sum(1, keepdim=True)) + 1e-10)
        ref = (lin * (n0 - n1) ** 2).sum(1)
        bound = HEAD_TOL * (lin.abs() * (n0.abs() + n1.abs()) ** 2).sum(1)
        ratio, msg = _worst(f"head {k}", state["dpix"][k] - ref, bound, ("image", "row", "column"))
        res["head"].append(ratio)
        if not ratio <= 1:
            fails.append(msg)
        total = total + state["dpix"][k].mean((1, 2))
    if "out" in state:
        ratio, msg = _worst("out", state["out"] - total, OUT_TOL * total.abs(), ("image",))
        res["out"] = ratio
        if not ratio <= 1:
            fails.append(msg)
    assert not fails, "\n".join(fails)
    return res


def head_grad(f0, f1, lin, up):
    """d(sum_p up[b] / HW lin . (n0 - n1)^2) / df0 for slice features f0, f1 [B,C,h,w]; 0 where |f0| = 0 (an all-zero feature
    vector: include/sings_hip.h's rule for the kernel, where torch's sqrt backward forms a NaN that the slice's ReLU then zeroes)."""
    HW = f0.shape[2] * f0.shape[3]
    r0 = torch.sqrt((f0 ** 2).sum(1, keepdim=True))
    d0, d1 = r0 + 1e-10, torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10
    q = (up.reshape(-1, 1, 1, 1) / HW) * 2 * lin.reshape(1, -1, 1, 1) * (f0 / d0 - f1 / d1)
    k2 = (q * f0).sum(1, keepdim=True) / (d0 * d0 * torch.where(r0 > 0, r0, torch.ones_like(r0)))
    return torch.where(r0 > 0, q / d0 - f0 * k2, torch.zeros_like(q))


def pinned_backward(wt, state, up, normalize=False):
    """fp64 dL/din0 [B,3,H,W] of sum_b up[b] out[b] through the kernel's own ReLU masks (y_l > 0), pool choices (arg codes) and
    slice features, with the true weights: the linear map a correct backward computes, up to round-off."""
    dev = state["y"][0].device
    B = state["B"]
    up = up.to(dev, torch.float64).reshape(-1)
    lin = lambda k: wt["lins"][k].to(dev, torch.float64).reshape(-1)
    head = lambda k: head_grad(state["y"][SLICE_LAYER[k]][:B], state["y"][SLICE_LAYER[k]][B:], lin(k), up)
    g = head(4)
    for l in range(12, -1, -1):
        w = wt["convs"][l][0].to(dev, torch.float64)
        g = F.conv_transpose2d(g * (state["y"][l][:B] > 0), w, padding=1)
        if l == 0:
            g = g / wt["scale"].to(dev, torch.float64)
            return 2 * g if normalize else g
        if LEVEL[l] != LEVEL[l - 1]:
            q = LEVEL[l] - 1
            a = state["arg"][q][:B]
            Ho, Wo = a.shape[2], a.shape[3]
            f = state["y"][SLICE_LAYER[q]]
            gin = torch.zeros((B, f.shape[1], f.shape[2], f.shape[3]), dtype=torch.float64, device=dev)
            for c in range(4):
                gin[:, :, c >> 1:2 * Ho:2, c & 1:2 * Wo:2] = torch.where(a == c, g, torch.zeros_like(g))
            g = gin + head(q)
