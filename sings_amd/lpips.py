"""LPIPS-VGG and the reference's LPIPS patch term through the C ABI (sg_lpips_*, csrc/sg_lpips.hip).

``LPIPS`` is a drop-in for ``lpips.LPIPS(net='vgg', version='0.1')`` in eval mode at the reference's two call sites
(sings/rec/losses/loss.py:79 and the validation metric of gs_trainer.py): ``LPIPS(...)(in0, in1, normalize=False)`` -> [B,1,1,1],
autograd to ``in0``.  The network is frozen: no weight gradients, and ``in1`` must not require grad.

``lpips_patch_loss`` is the whole term of loss.py:71-80 -- clamp, the two compositions over the random background, the patch crop,
``.clip(max=1)``, LPIPS, ``.mean()`` and the weight -- with the patch origins as a device tensor (no host round trip, so the step
can be captured as a graph).  ``PatchSampler`` draws the origins as utils/image/sampler.py does, with the same numpy RNG calls
-- on the host, from a copy of the mask; ``sings_amd.patch_sampler.DevicePatchSampler`` draws them on the device, inside a captured step.
No CPU fallback: the HIP library must be present.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._marshal import _ptr, _stream

CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))           # VGG16 `features` convs up to relu5_3: (Cin, Cout)
SLICE_CONVS = (2, 2, 3, 3, 3)                                   # convs per slice (lpips.pretrained_networks.vgg16 slice1..5)
LIN_CHANNELS = (64, 128, 256, 512, 512)


def weights_layout():
    """-> (offsets tuple of SG_LPIPS_NUM_OFFSETS floats offsets, total floats) of the packed weight buffer (sg_lpips_weights_layout)."""
    offs = (C.c_size_t * _lib.LPIPS_NUM_OFFSETS)()
    total = C.c_size_t(0)
    _lib.check(_lib.load().sg_lpips_weights_layout(offs, C.byref(total)), "sg_lpips_weights_layout")
    return tuple(int(o) for o in offs), int(total.value)


def pack_weights(convs, lins, shift, scale):
    """Host-side packing (torch, CPU, once): ``convs`` 13 (W [Cout,Cin,3,3], b [Cout]); ``lins`` 5 [C] (or [1,C,1,1]);
    ``shift`` / ``scale`` 3 values.  -> a float32 CPU tensor laid out as include/sings_hip.h describes."""
    offs, total = weights_layout()
    out = torch.zeros(total, dtype=torch.float32)
    if len(convs) != 13 or len(lins) != 5:
        raise ValueError("pack_weights: 13 convs and 5 lin layers expected")
    for l, ((w, b), (ci, co)) in enumerate(zip(convs, CONV_CHANNELS)):
        w = torch.as_tensor(w).detach().to("cpu", torch.float32)
        b = torch.as_tensor(b).detach().to("cpu", torch.float32).reshape(-1)
        if tuple(w.shape) != (co, ci, 3, 3) or b.numel() != co:
            raise ValueError(f"pack_weights: conv {l} must be [{co},{ci},3,3] with a [{co}] bias, got {tuple(w.shape)}")
        n = w.numel()
        if l == 0:
            out[offs[0]:offs[0] + n] = w.reshape(-1)
        else:
            out[offs[3 * l]:offs[3 * l] + n] = w.permute(0, 2, 3, 1).reshape(-1)                        # [Cout][ky][kx][Cin]
            out[offs[3 * l + 2]:offs[3 * l + 2] + n] = w.transpose(0, 1).flip(2, 3).permute(0, 2, 3, 1).reshape(-1)
        out[offs[3 * l + 1]:offs[3 * l + 1] + co] = b
    for k, (lw, c) in enumerate(zip(lins, LIN_CHANNELS)):
        lw = torch.as_tensor(lw).detach().to("cpu", torch.float32).reshape(-1)
        if lw.numel() != c:
            raise ValueError(f"pack_weights: lin {k} must have {c} weights")
        out[offs[39 + k]:offs[39 + k] + c] = lw
    out[offs[44]:offs[44] + 3] = torch.as_tensor(shift).detach().to("cpu", torch.float32).reshape(-1)
    out[offs[45]:offs[45] + 3] = torch.as_tensor(scale).detach().to("cpu", torch.float32).reshape(-1)
    return out


def unpack_backward_weights(packed, l):
    """The input-gradient weights of conv ``l`` >= 1 as [Cin, Cout, 3, 3] (= W.transpose(0,1).flip(2,3)): for tests."""
    offs, _ = weights_layout()
    ci, co = CONV_CHANNELS[l]
    return packed[offs[3 * l + 2]:offs[3 * l + 2] + ci * co * 9].reshape(ci, 3, 3, co).permute(0, 3, 1, 2)


def _ws_bytes(B, H, W):
    n = C.c_size_t(0)
    _lib.check(_lib.load().sg_lpips_ws_bytes(B, H, W, C.byref(n)), "sg_lpips_ws_bytes")
    return int(n.value)


def ws_layout(B, H, W):
    """Byte offsets of the forward's workspace pieces (sg_lpips_ws_layout; include/sings_hip.h says what each holds):
    -> dict(y=[13], pool=[4], arg=[4], dpix=[5], g=[2], total=bytes).  For tests and inspection."""
    offs = (C.c_size_t * _lib.LPIPS_WS_NUM_PIECES)()
    total = C.c_size_t(0)
    _lib.check(_lib.load().sg_lpips_ws_layout(B, H, W, offs, C.byref(total)), "sg_lpips_ws_layout")
    o = [int(v) for v in offs]
    return {"y": o[0:13], "pool": o[13:17], "arg": o[17:21], "dpix": o[21:26], "g": o[26:28], "total": int(total.value)}


class _LPIPSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1, packed, normalize):
        lib = _lib.load()
        B, H, W = int(in0.shape[0]), int(in0.shape[2]), int(in0.shape[3])
        dev = in0.device
        ws = torch.empty(_ws_bytes(B, H, W), dtype=torch.uint8, device=dev)
        out = torch.empty(B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sg_lpips_forward(B, H, W, int(normalize), _ptr(packed), _ptr(in0), _ptr(in1), _ptr(ws), _ptr(out),
                                            _stream(dev)), "lpips forward")
        ctx.save_for_backward(packed, ws)
        ctx.args = (B, H, W, int(normalize))
        return out

    @staticmethod
    def backward(ctx, g):
        packed, ws = ctx.saved_tensors
        B, H, W, normalize = ctx.args
        dev = ws.device
        g = g.contiguous().float()
        din0 = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sg_lpips_backward(B, H, W, normalize, _ptr(packed), _ptr(ws), _ptr(g), _ptr(din0), _stream(dev)),
                       "lpips backward")
        return din0, None, None, None


class LPIPS(torch.nn.Module):
    """``LPIPS(packed)`` -- use ``LPIPS.from_module(lpips_module)`` or ``LPIPS.from_tensors(...)``.  Calling it:
    ``(in0, in1, normalize=False) -> [B,1,1,1]`` for [B,3,H,W] (or [3,H,W]: B = 1) fp32 images, H and W >= 16."""

    def __init__(self, packed):
        super().__init__()
        _, total = weights_layout()
        if packed.dim() != 1 or packed.numel() != total:
            raise ValueError(f"LPIPS: packed weights must be a flat tensor of {total} floats (sings_amd.lpips.pack_weights)")
        self.register_buffer("packed", packed.detach().to(torch.float32).contiguous())

    @classmethod
    def from_tensors(cls, convs, lins, shift, scale, device=None):
        """``convs``: 13 (weight [Cout,Cin,3,3], bias [Cout]) pairs in ``features`` order; ``lins``: 5 lin weights ([1,C,1,1] or [C]);
        ``shift`` / ``scale``: the scaling layer's 3 values each."""
        p = pack_weights(convs, lins, shift, scale)
        m = cls(p)
        return m.to(device) if device is not None else m

    @classmethod
    def from_module(cls, m, device=None):
        """From a user's own ``lpips.LPIPS(net='vgg')`` object, read by attribute: the Conv2d's of ``m.net.slice1..5``, the weight
        of ``m.lin0..4.model[-1]``, ``m.scaling_layer.shift`` / ``.scale``."""
        convs = []
        for k in range(1, 6):
            for layer in getattr(m.net, f"slice{k}").children():
                if isinstance(layer, torch.nn.Conv2d):
                    convs.append((layer.weight, layer.bias))
        lins = [getattr(m, f"lin{k}").model[-1].weight for k in range(5)]
        return cls.from_tensors(convs, lins, m.scaling_layer.shift, m.scaling_layer.scale, device=device)

    def forward(self, in0, in1, retPerLayer=False, normalize=False, spatial=False):
        if retPerLayer or spatial:
            raise NotImplementedError("sings_amd.lpips.LPIPS: retPerLayer / spatial are not provided")
        if in1.requires_grad:
            raise ValueError("sings_amd.lpips.LPIPS: gradients flow to in0 only; in1 must not require grad")
        if in0.dim() == 3:
            in0 = in0.unsqueeze(0)
        if in1.dim() == 3:
            in1 = in1.unsqueeze(0)
        if not in0.is_cuda:
            raise RuntimeError("sings_amd.lpips: tensors must live on the GPU (no CPU fallback)")
        if in0.dim() != 4 or in0.shape[1] != 3 or in1.shape != in0.shape or in0.shape[0] < 1:
            raise ValueError("sings_amd.lpips.LPIPS: in0 / in1 must both be [B,3,H,W] (or [3,H,W]) with B >= 1")
        if in0.shape[2] < _lib.LPIPS_MIN_SIZE or in0.shape[3] < _lib.LPIPS_MIN_SIZE:
            raise ValueError(f"sings_amd.lpips.LPIPS: H and W must be at least {_lib.LPIPS_MIN_SIZE}")
        packed = self.packed if self.packed.device == in0.device else self.packed.to(in0.device)
        out = _LPIPSFn.apply(in0.contiguous().float(), in1.detach().contiguous().float(), packed, bool(normalize))
        return out.reshape(-1, 1, 1, 1)


class _PatchGather(torch.autograd.Function):
    """raw [K,3,H,W] -> (pred patches [K n,3,P,P] (differentiable), gt patches (not)); csrc/sg_lpips.hip lp_patch_gather / _scatter."""

    @staticmethod
    def forward(ctx, raw, gt_rgb, mask, bg, bg_rand, origins, P):
        K, H, W = int(raw.shape[0]), int(raw.shape[2]), int(raw.shape[3])
        n = int(origins.shape[1])
        dev = raw.device
        pred = torch.empty((K * n, 3, P, P), dtype=torch.float32, device=dev)
        gt = torch.empty_like(pred)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sg_lpips_patch_gather(K, n, P, H, W, _ptr(raw), _ptr(gt_rgb), _ptr(mask), _ptr(bg), _ptr(bg_rand),
                                                         _ptr(origins), _ptr(pred), _ptr(gt), _stream(dev)), "lpips patch gather")
        ctx.save_for_backward(raw, mask, bg_rand, origins)
        ctx.args = (K, n, P, H, W)
        ctx.mark_non_differentiable(gt)
        ctx.set_materialize_grads(False)
        return pred, gt

    @staticmethod
    def backward(ctx, g_pred, g_gt=None):
        raw, mask, bg_rand, origins = ctx.saved_tensors
        K, n, P, H, W = ctx.args
        out = torch.empty_like(raw)
        if g_pred is None:
            return out.zero_(), None, None, None, None, None, None
        g_pred = g_pred.contiguous().float()
        dev = raw.device
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sg_lpips_patch_scatter(K, n, P, H, W, _ptr(raw), _ptr(mask), _ptr(bg_rand), _ptr(origins),
                                                          _ptr(g_pred), _ptr(out), _stream(dev)), "lpips patch scatter")
        return out, None, None, None, None, None, None


def _patch_values(raw, gt_rgb, mask, bg, bg_rand, origins, patch_size, lpips):
    """-> [K, n] LPIPS values of the K frames' n patches each."""
    if not raw.is_cuda:
        raise RuntimeError("sings_amd.lpips: tensors must live on the GPU (no CPU fallback)")
    K, H, W = int(raw.shape[0]), int(raw.shape[2]), int(raw.shape[3])
    if raw.dim() != 4 or raw.shape[1] != 3:
        raise ValueError("lpips_patch_loss: raw must be [3,H,W] or [K,3,H,W]")
    P = int(patch_size)
    if not _lib.LPIPS_MIN_SIZE <= P <= min(H, W):
        raise ValueError(f"lpips_patch_loss: patch_size must be in {_lib.LPIPS_MIN_SIZE}..min(H, W)")
    if origins.dim() != 3 or origins.shape[0] != K or origins.shape[2] != 2 or origins.shape[1] < 1:
        raise ValueError("lpips_patch_loss: origins must be [n,2] ([K,n,2] for K frames) (row, col) corners")
    hw = H * W
    raw = raw.contiguous().float()
    gt_rgb = gt_rgb.float().expand(K, 3, H, W).contiguous() if gt_rgb.numel() in (3 * hw, K * 3 * hw) else None
    mask = mask.float().reshape(-1, H, W).expand(K, H, W).contiguous() if mask.numel() in (hw, K * hw) else None
    if gt_rgb is None or mask is None:
        raise ValueError("lpips_patch_loss: gt_rgb must be [3,H,W] / [K,3,H,W], mask [H,W] / [1,H,W] / [K,H,W]")
    bg_rand = bg_rand.float().reshape(-1, 3, H, W).expand(K, 3, H, W).contiguous()
    bg = bg.float().reshape(3).contiguous()
    origins = origins.to(device=raw.device, dtype=torch.int32).contiguous()
    pred, gt = _PatchGather.apply(raw, gt_rgb, mask, bg, bg_rand, origins, P)
    return lpips(pred, gt).reshape(K, -1)


def lpips_patch_loss(raw, gt_rgb, mask, bg, bg_rand, origins, patch_size, lpips, lpips_w):
    """``loss_dict['lpips_patch']`` of loss.py:71-80 as a 0-dim tensor with autograd to ``raw``:

        pred = clamp(raw, 0, 1);  gt = gt_rgb * mask + bg * (1 - mask)
        lpips_w * lpips(crop(pred * mask + bg_rand * (1 - mask)).clip(max=1), crop(gt * mask + bg_rand * (1 - mask))).mean()

    ``raw`` [3,H,W] the UNCLAMPED render; ``bg`` [3] the step's background; ``bg_rand`` [3,H,W] the random background
    (``torch.rand_like(pred)``); ``origins`` [n,2] device int (row, col) corners (``PatchSampler``).  K frames: ``raw`` [K,3,H,W],
    ``origins`` [K,n,2], ``gt_rgb`` / ``mask`` / ``bg_rand`` per frame or one for all -> a [K] tensor, one term per frame
    (``sum()`` them for the step's loss, as ``photometric_loss_frames``); each frame's value and gradient are bit-equal to a call
    with that frame alone."""
    frames = raw.dim() == 4
    if not frames:
        raw, origins = raw.unsqueeze(0), origins.unsqueeze(0)
    vals = _patch_values(raw, gt_rgb, mask, bg, bg_rand, origins, patch_size, lpips)
    per_frame = vals.mean(1) * lpips_w
    return per_frame if frames else per_frame.reshape(())


class PatchSampler:
    """utils/image/sampler.py restated for the origins only, with the same global-numpy-RNG calls in the same order
    (``np.random.rand``, then ``np.random.choice`` or two ``np.random.randint``): a seeded run picks the reference's patches.
    ``origins(mask)`` -> int32 numpy [n,2] of (row, col) top-left corners; ``mask`` [1,H,W] / [H,W] (tensor or array)."""

    def __init__(self, num_patch=4, patch_size=20, ratio_mask=0.9, dilate=0):
        if patch_size % 2:
            raise ValueError("patch size has to be even")
        if dilate > 0:
            raise NotImplementedError("PatchSampler: dilate > 0 (cv2.dilate) is not provided; the reference's configs use 0")
        self.n, self.patch_size, self.p, self.dilate = num_patch, patch_size, ratio_mask, dilate

    def origins(self, mask):
        m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
        m = m.reshape(m.shape[-2], m.shape[-1])
        H, W = m.shape
        P = self.patch_size
        if np.random.rand() < self.p:
            o = P // 2
            valid = m[o:-o, o:-o] > 0
            xs, ys = np.where(valid)
            idx = np.random.choice(len(xs), size=self.n, replace=False)
            x, y = xs[idx], ys[idx]
        else:
            x = np.random.randint(0, H - P, size=self.n)
            y = np.random.randint(0, W - P, size=self.n)
        return np.stack([x, y], 1).astype(np.int32)
