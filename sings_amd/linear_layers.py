"""The decoders' layers: ``h = act(x W^T + b)`` and its backward as HIP kernels on the matrix cores (sg_linear_*, sg_weight_grad), the
element-wise heads (sg_scales_head_*, sg_bias_act_*), and the three ways several layers share one input (`linear_act`,
`linear_act_shared`, `linear_fan`).  No CPU fallback.  Where a weight-gradient launch goes is decided by sings_amd/side_launch.py.
"""
import ctypes as C

import torch

from . import _lib
from ._marshal import _ptr, _stream
from .grad_arena import arena_out
from .side_launch import defer_side, flush_deferred, weight_grads_overlapped, wg_stream

ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_SOFTPLUS_REF = 0, 1, 2, 3


def _lin_fwd(x, W, b, act, row_offset):
    """h = act(x W^T + b) in one kernel (sg_linear_forward); returns (h, aux, Wc): aux is what the backward needs besides x --
    gelu'(z) for GELU (so the backward's act' is one multiplication), the output h for the sigmoid, z for the softplus."""
    lib = _lib.load()
    if not x.is_cuda:
        raise RuntimeError("sings_amd.decode: tensors must live on the GPU (no CPU fallback)")
    Wc = W.contiguous().float()
    bc = None if b is None else b.contiguous().float()
    dev, N, Cout, Cin = x.device, int(x.shape[0]), int(W.shape[0]), int(W.shape[1])
    ro = row_offset.contiguous().float().reshape(-1) if row_offset is not None else None
    h = torch.empty((N, Cout), dtype=torch.float32, device=dev)
    aux = torch.empty_like(h) if act in (ACT_GELU, ACT_SOFTPLUS_REF) else None
    with torch.cuda.device(dev):
        _lib.check(lib.sg_linear_forward(N, Cin, Cout, act, _ptr(x), _ptr(Wc), _ptr(bc), _ptr(ro), _ptr(aux), _ptr(h),
                                         _stream(dev)), "linear forward")
    if act == ACT_SIGMOID:
        aux = h
    return h, aux, Wc


def _lin_bwd(x, W, aux, act, has_b, dh, need_dx, need_dw, dx_into=None):
    """dz = dh * act'(z) in the prologue of dx = dz W (sg_linear_backward), then dW = dz^T x, db = column sums (sg_weight_grad).
    ``dx_into``: an existing [N,Cin] gradient this layer ADDS its dx to (sg_linear_backward_accumulate)."""
    lib = _lib.load()
    dev, N, Cout, Cin = x.device, int(x.shape[0]), int(W.shape[0]), int(W.shape[1])
    dh = dh.contiguous().float()
    dz = torch.empty_like(dh) if act != ACT_NONE else dh
    dx = None
    with torch.cuda.device(dev):
        if need_dx:
            acc = dx_into is not None
            dx = dx_into if acc else torch.empty((N, Cin), dtype=torch.float32, device=dev)
            fn = lib.sg_linear_backward_accumulate if acc else lib.sg_linear_backward
            _lib.check(fn(N, Cin, Cout, act, _ptr(aux) if act != ACT_NONE else None, None, _ptr(dh), _ptr(W),
                          _ptr(dz) if act != ACT_NONE else None, _ptr(dx), _stream(dev)), "linear backward")
        elif act == ACT_GELU:                                   # a layer whose input needs no gradient: only dz = dh * gelu'(z)
            torch.mul(dh, aux, out=dz)
        elif act == ACT_SIGMOID:
            torch.mul(dh, aux * (1.0 - aux), out=dz)
        elif act == ACT_SOFTPLUS_REF:
            torch.mul(dh, torch.sigmoid(aux), out=dz)
        dW = db = None
        if need_dw:
            dW, db = _weight_grad(x, W, dz, has_b)
    return dx, dW, db


def _weight_grad(x, W, dz, has_b, flush=True):
    """dW = dz^T x and db = column sums of dz in one pass on the matrix cores (sg_weight_grad); on the side stream, one kernel of the
    main chain late, when ``overlap_weight_grads`` is on.  Call it right AFTER the kernel that produced dz has been issued
    (``flush=False``: a further layer of the same kernel -- the launches deferred so far stay deferred)."""
    lib = _lib.load()
    dev, N, Cout, Cin = x.device, int(x.shape[0]), int(W.shape[0]), int(W.shape[1])
    with torch.cuda.device(dev):
        dW = arena_out(W)
        db = torch.empty(Cout, dtype=torch.float32, device=dev) if has_b else None
        ws2 = torch.empty(int(lib.sg_weight_grad_ws_bytes(N, Cout, Cin)), dtype=torch.uint8, device=dev)
        # (a parameter that already carries a .grad -- gradient accumulation, zero_grad(set_to_none=False) -- makes AccumulateGrad READ dW
        #  on the main stream at once: the deferred launch would write memory autograd has read and may have freed.  Inline there.)
        if weight_grads_overlapped() and getattr(W, "grad", None) is None:
            side, cur = wg_stream(dev), torch.cuda.current_stream(dev)
            fork = torch.cuda.Event()
            fork.record(cur)                                     # dz (and x) are complete on the backward stream
            if flush:
                flush_deferred()                                 # the previous layer's: this layer's dx kernel has been issued

            # (the closure must not hold dW / db: AccumulateGrad adopts a returned gradient without a copy only while nobody else
            #  references it -- and a copy made BEFORE the deferred kernel has written it would be a copy of nothing.  p.grad
            #  keeps them alive until the streams have joined: the end-of-backward join of side_launch)
            p_dW, p_db = _ptr(dW), _ptr(db)

            def launch(dz=dz, x=x, ws2=ws2):
                side.wait_event(fork)
                with torch.cuda.device(dev), torch.cuda.stream(side):
                    _lib.check(lib.sg_weight_grad(N, Cout, Cin, _ptr(dz), _ptr(x), _ptr(ws2), p_dW, p_db,
                                                  C.c_void_p(side.cuda_stream)), "weight gradient")
                for t in (dz, x, ws2):
                    t.record_stream(side)
            defer_side(launch)
        else:
            _lib.check(lib.sg_weight_grad(N, Cout, Cin, _ptr(dz), _ptr(x), _ptr(ws2), _ptr(dW), _ptr(db), _stream(dev)),
                       "weight gradient")
    return dW, db


class _LinearAct(torch.autograd.Function):
    """h = act(x @ W^T + b) as ONE kernel on the matrix cores (sg_linear_forward: bias + activation in the GEMM's epilogue);
    backward: sg_linear_backward (dz = dh * act' in the prologue of dx = dz W, dz stored once) + sg_weight_grad.
    No library GEMM, no separate element-wise pass (round 1: torch.addmm / torch.mm + sg_bias_act_*).

    ``slot`` (a dict, `linear_act_shared`): the layer shares its INPUT with other layers of the same slot (the tri-plane features
    read by both decoders' first layers, sings_hybrid.py:259-262) without tying their backward passes together: whichever layer's
    backward runs first writes the input gradient (and hands it to autograd), the others ADD theirs into that very tensor
    (sg_linear_backward_accumulate) and hand autograd nothing -- one [N,Cin] gradient, no addition kernel, and each layer's backward
    runs as soon as ITS gradient is there.  (`linear_fan` needs all of them at once: in the training step the appearance decoder's
    first layer then waited for the geometry decoder's, i.e. for the k-NN regulariser; here its 80 us run in that wait.)"""

    @staticmethod
    def forward(ctx, x, W, b, act, row_offset, slot):
        x = x.contiguous().float()
        h, aux, Wc = _lin_fwd(x, W, b, act, row_offset)
        ctx.save_for_backward(x, Wc, aux if aux is not None else torch.empty(0, device=x.device))
        ctx.act, ctx.has_b, ctx.slot = act, b is not None, slot
        return h

    @staticmethod
    def backward(ctx, dh):
        x, W, aux = ctx.saved_tensors
        need_dw = ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2])
        need_dx = ctx.needs_input_grad[0]
        # the slot takes part only where the accumulating kernel can add into it; without one this is the plain layer's backward
        slot = ctx.slot if (ctx.slot is not None and need_dx and (int(x.shape[1]) & 31) == 0) else None
        into = slot.get("dx") if slot is not None else None
        dx, dW, db = _lin_bwd(x, W, aux, ctx.act, ctx.has_b, dh, need_dx, need_dw, dx_into=into)
        if into is not None:
            dx = None                                            # (already inside the tensor the first layer handed over)
        elif slot is not None:
            slot["dx"] = dx
            # The shared gradient belongs to THIS backward pass only.  A later pass over the same graph (retain_graph=True, one
            # autograd.grad call per loss term, a pass that reaches only one of the decoders) must start with an empty slot: it
            # would otherwise add into the earlier pass's tensor, hand autograd nothing, and lose its input gradient.
            torch.autograd.Variable._execution_engine.queue_callback(lambda: slot.pop("dx", None))
        return dx, dW, db, None, None, None


def linear_act(x, lin, act=ACT_NONE, row_offset=None):
    return _LinearAct.apply(x, lin.weight, lin.bias, act, row_offset, None)


def linear_act_shared(x, lin, act, slot):
    return _LinearAct.apply(x, lin.weight, lin.bias, act, None, slot)


class _LinearFan(torch.autograd.Function):
    """Several layers reading the SAME activation (the decoder trunk and its heads, decoders.py:41-49, 75-94; the tri-plane
    features and the two decoders, sings_hybrid.py:259-262): forward = one sg_linear_forward per layer; backward: the first
    consumer writes dx, the others ADD theirs into the same array (sg_linear_backward_accumulate) -- one [N,Cin] gradient
    instead of one per consumer plus autograd's element-wise additions (two 77-MB passes per trunk at 150 k points)."""

    @staticmethod
    def forward(ctx, x, acts, row_offsets, *wb):
        x = x.contiguous().float()
        outs, saved = [], [x]
        for i, act in enumerate(acts):
            h, aux, Wc = _lin_fwd(x, wb[2 * i], wb[2 * i + 1], act, row_offsets[i])
            outs.append(h)
            saved += [Wc, aux if aux is not None else torch.empty(0, device=x.device)]
        ctx.save_for_backward(*saved)
        ctx.acts, ctx.has_b = tuple(acts), tuple(wb[2 * i + 1] is not None for i in range(len(acts)))
        return tuple(outs)

    @staticmethod
    def _fan_plan(ctx, dhs, x):
        """Layer 0 wide and every other layer a narrow head (<= 16 columns together, at most two, act none | sigmoid): their input
        gradients in ONE kernel (sg_linear_backward_fan).  None: the per-layer path."""
        n = len(ctx.acts)
        if not (2 <= n <= 3) or any(d is None for d in dhs) or (int(x.shape[1]) & 31) or int(x.shape[0]) > 3_000_000:
            return None                                          # (the kernel's 32-bit byte offsets: N + look-ahead rows < 2^31 / 576)
        couts = [int(ctx.saved_tensors[1 + 2 * i].shape[0]) for i in range(n)]
        if couts[0] & 3 or sum(couts[1:]) > 16 or any(a not in (ACT_NONE, ACT_SIGMOID) for a in ctx.acts[1:]):
            return None
        return couts

    @staticmethod
    def backward(ctx, *dhs):
        x = ctx.saved_tensors[0]
        need_dx = ctx.needs_input_grad[0]
        can_acc = (int(x.shape[1]) & 31) == 0
        couts = _LinearFan._fan_plan(ctx, dhs, x) if (need_dx and _FAN["on"]) else None
        if couts is not None:
            return _LinearFan._backward_fused(ctx, dhs, x, couts)
        dx, grads = None, []
        for i, act in enumerate(ctx.acts):
            W, aux = ctx.saved_tensors[1 + 2 * i], ctx.saved_tensors[2 + 2 * i]
            need_dw = ctx.needs_input_grad[3 + 2 * i] or (ctx.has_b[i] and ctx.needs_input_grad[4 + 2 * i])
            if dhs[i] is None:
                grads += [None, None]
                continue
            dxi, dW, db = _lin_bwd(x, W, aux, act, ctx.has_b[i], dhs[i], need_dx, need_dw,
                                   dx_into=dx if (can_acc and dx is not None) else None)
            if need_dx:
                dx = dxi if (dx is None or can_acc) else dx + dxi
            grads += [dW, db]
        return (dx, None, None, *grads)

    @staticmethod
    def _backward_fused(ctx, dhs, x, couts):
        lib = _lib.load()
        dev, N, Cin = x.device, int(x.shape[0]), int(x.shape[1])
        n = len(couts)
        W = [ctx.saved_tensors[1 + 2 * i] for i in range(n)]
        aux = [ctx.saved_tensors[2 + 2 * i] for i in range(n)]
        dh = [d.contiguous().float() for d in dhs]
        dz = [torch.empty_like(dh[i]) if ctx.acts[i] != ACT_NONE else dh[i] for i in range(n)]
        dx = torch.empty((N, Cin), dtype=torch.float32, device=dev)
        side = (_lib.SgLinearSide * 2)()
        for j in range(1, n):
            sd = side[j - 1]
            sd.cout, sd.act = couts[j], ctx.acts[j]
            sd.aux = aux[j].data_ptr() if ctx.acts[j] != ACT_NONE else None
            sd.dh, sd.W = dh[j].data_ptr(), W[j].data_ptr()
            sd.dz_out = dz[j].data_ptr() if ctx.acts[j] != ACT_NONE else None
        with torch.cuda.device(dev):
            _lib.check(lib.sg_linear_backward_fan(N, Cin, couts[0], ctx.acts[0], _ptr(aux[0]) if ctx.acts[0] != ACT_NONE else None,
                                                  _ptr(dh[0]), _ptr(W[0]), _ptr(dz[0]) if ctx.acts[0] != ACT_NONE else None, _ptr(dx),
                                                  side, _stream(dev)), "linear backward (fan)")
        grads = []
        for i in range(n):
            need_dw = ctx.needs_input_grad[3 + 2 * i] or (ctx.has_b[i] and ctx.needs_input_grad[4 + 2 * i])
            dW, db = _weight_grad(x, W[i], dz[i], ctx.has_b[i], flush=not grads) if need_dw else (None, None)
            grads += [dW, db]
        return (dx, None, None, *grads)


_FAN = {"on": True}


def fuse_fan_backward(flag=True):
    """The narrow heads' input gradients inside the wide layer's kernel (default on; off: one accumulate pass per head)."""
    _FAN["on"] = bool(flag)


def linear_fan(x, layers):
    """layers: [(nn.Linear, act, row_offset | None), ...] -> tuple of outputs, one per layer, all reading x."""
    wb = []
    for lin, _, _ in layers:
        wb += [lin.weight, lin.bias]
    return _LinearFan.apply(x, tuple(a for _, a, _ in layers), tuple(r for _, _, r in layers), *wb)


class _ScalesHead(torch.autograd.Function):
    """z [N,1] -> (scales [N,3] = softplus(z) three times, scales_aux [N,3] = z three times), decoders.py:88-98."""

    @staticmethod
    def forward(ctx, z):
        lib = _lib.load()
        z = z.contiguous().float()
        dev, N = z.device, int(z.shape[0])
        scales = torch.empty((N, 3), dtype=torch.float32, device=dev)
        aux = torch.empty_like(scales)
        with torch.cuda.device(dev):
            _lib.check(lib.sg_scales_head_forward(N, _ptr(z), _ptr(scales), _ptr(aux), _stream(dev)), "scales head forward")
        ctx.save_for_backward(z)
        ctx.set_materialize_grads(False)                         # (an output nobody differentiates: None, not a zero-filled tensor)
        return scales, aux

    @staticmethod
    def backward(ctx, dscales, daux):
        lib = _lib.load()
        (z,) = ctx.saved_tensors
        dev, N = z.device, int(z.shape[0])
        if dscales is None and daux is None:
            return None
        ds = dscales.contiguous().float() if dscales is not None else None
        da = daux.contiguous().float() if daux is not None else None
        dz = torch.empty_like(z)
        with torch.cuda.device(dev):
            _lib.check(lib.sg_scales_head_backward(N, _ptr(z), _ptr(ds), _ptr(da), _ptr(dz), _stream(dev)), "scales head backward")
        return dz


scales_head = _ScalesHead.apply


class _Act(torch.autograd.Function):
    """element-wise activation through the same kernels (no bias)."""

    @staticmethod
    def forward(ctx, z, act):
        lib = _lib.load()
        z = z.contiguous().float()
        dev, N, Cc = z.device, int(z.shape[0]), int(z.shape[1])
        h = torch.empty_like(z)
        with torch.cuda.device(dev):
            _lib.check(lib.sg_bias_act_forward(N, Cc, act, _ptr(z), None, None, None, _ptr(h), _stream(dev)), "act forward")
        ctx.save_for_backward(z)
        ctx.act = act
        return h

    @staticmethod
    def backward(ctx, dh):
        lib = _lib.load()
        (z,) = ctx.saved_tensors
        dev, N, Cc = z.device, int(z.shape[0]), int(z.shape[1])
        dh = dh.contiguous().float()
        dz = torch.empty_like(dh)
        ws = torch.empty(int(lib.sg_bias_act_ws_bytes(N, Cc)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sg_bias_act_backward(N, Cc, ctx.act, _ptr(z), None, _ptr(dh), _ptr(ws), _ptr(dz), None, _stream(dev)),
                       "act backward")
        return dz, None


activation = _Act.apply                  # activation(z, act)
