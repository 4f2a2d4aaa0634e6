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
