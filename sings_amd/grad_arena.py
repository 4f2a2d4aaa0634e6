"""The gradient arena: ONE flat fp32 buffer that holds every parameter's gradient, written in place by the kernels that produce them.

Frame-parallel training reduces the parameter gradients with ONE collective over ONE flat buffer.  Instead of
gathering the .grad tensors into that buffer and scattering them back every step (two extra passes over 35 MB), the kernels that
PRODUCE the large gradients -- the tri-plane scatter (33 of the 35 MB), the decoders' weight gradients, the pose tables' rows -- write
them straight into the caller's buffer: `set_gradient_arena(params, flat)` registers a slot per parameter, the backward functions
hand autograd a fresh view of the slot (`arena_out`; AccumulateGrad adopts it without a copy when .grad is None, the precondition
the training step already guarantees), so `p.grad` IS a piece of `flat`.  Gradients produced elsewhere (biases, anchors) are small;
the caller copies those into their slots (`arena_sync`).

Plain torch: nothing here needs the HIP library, and host tensors register like device tensors.
"""
import weakref

import torch

_ARENA = {}                            # parameter storage address -> [flat, offset, shape, weakref(parameter), weakref(last view handed out)]
_ARENA_REG = {"params": None, "stale": False}       # the registered parameter objects (weak) / dropped by a topology change


def is_feature_minor(p):
    """[1, F, H, W] in channels_last memory format = [H][W][F] in memory (and not ALSO plain-contiguous: H W > 1, F > 1)."""
    return (p.dim() == 4 and p.dtype == torch.float32 and p.is_contiguous(memory_format=torch.channels_last)
            and not p.is_contiguous())


def like_layout(flat_slice, param_like):
    """A view of ``flat_slice`` (param_like.numel() elements) with the SHAPE and the memory layout of ``param_like``: plain for a
    contiguous parameter, [1,H,W,F].permute(0,3,1,2) for a feature-minor one (channels_last)."""
    if is_feature_minor(param_like):
        n, f, h, w = param_like.shape
        return flat_slice.view(n, h, w, f).permute(0, 3, 1, 2)
    return flat_slice.view(param_like.shape)


def invalidate_gradient_arena():
    """The set of parameters changed (AvatarStep.set_topology): the registration describes parameters that no longer exist.  Nothing is
    written into the old buffer any more, and ``arena_sync`` raises until ``set_gradient_arena`` has registered the new set."""
    if _ARENA or _ARENA_REG["params"] is not None:
        _ARENA.clear()
        _ARENA_REG["stale"] = True


def set_gradient_arena(params, flat):
    """Register (or, with ``params=None``, drop) the flat gradient buffer.  Returns the per-parameter views of ``flat``."""
    _ARENA.clear()
    _ARENA_REG["stale"] = False
    _ARENA_REG["params"] = None if params is None else [weakref.ref(p) for p in params]
    if params is None:
        return []
    views, o = [], 0
    for p in params:
        n = p.numel()
        if not (p.is_contiguous() or is_feature_minor(p)):
            raise ValueError("gradient arena: parameters must be contiguous (or feature-minor tri-plane planes)")
        _ARENA[p.data_ptr()] = [flat, o, tuple(p.shape), weakref.ref(p), None]
        views.append(like_layout(flat[o:o + n], p))              # (a feature-minor plane's slot holds its gradient feature-minor too)
        o += n
    if o != flat.numel() or flat.dtype != torch.float32:
        raise ValueError("gradient arena: `flat` must be fp32 with exactly sum(p.numel()) elements")
    return views


def arena_registration():
    """-> (slots, params), read-only: a copy of the registered slots (storage address -> slot record) and the list of weak references
    to the registered parameters.  ``({}, None)`` when nothing is registered."""
    return dict(_ARENA), _ARENA_REG["params"]


def arena_holds_any(params):
    """One of ``params`` has a slot (its producer then writes the slots, not one buffer of its own)."""
    return any(_ARENA.get(p.data_ptr()) is not None for p in params)


def arena_out(param_like):
    """A FRESH view of the arena slot of the parameter `param_like` aliases (autograd adopts a gradient tensor without copying
    only if nobody else holds that tensor object), or a new tensor when there is no arena / no slot."""
    hit = _ARENA.get(param_like.data_ptr())
    if hit is None or hit[2] != tuple(param_like.shape) or hit[0].device != param_like.device:
        return torch.empty_like(param_like, dtype=torch.float32)
    flat, o, shape, pref, last = hit
    # The slot is the memory `p.grad` lives in once autograd has adopted the view.  Writing the NEXT gradient there is only
    # right when nothing accumulates: p.grad must be None (zero_grad(set_to_none=False), micro-batch accumulation: the kernel
    # would overwrite p.grad's own memory and AccumulateGrad would then add the slot to itself -- 2 x the last gradient instead of
    # old + new), and the view of an earlier hand-out must be gone (a weight or plane used twice in ONE graph: the first use's
    # gradient still sits in the slot, waiting to be accumulated).  Otherwise: a fresh tensor, autograd adds, arena_sync copies.
    p = pref()
    if p is None or p.grad is not None or (last is not None and last() is not None):
        return torch.empty_like(param_like, dtype=torch.float32)
    v = like_layout(flat[o:o + param_like.numel()], param_like)
    hit[4] = weakref.ref(v)
    return v


def arena_sync(params, views, to_arena=True):
    """Gradients that did not land in their slot (produced by torch's own backward functions): copy them in (before the
    collective) / back out (after it) with one multi-tensor launch."""
    reg = _ARENA_REG["params"]
    if _ARENA_REG["stale"] or reg is None or len(reg) != len(params) or any(r() is not p for r, p in zip(reg, params)):
        raise RuntimeError("gradient arena: the registration is stale (a densify / prune replaced parameters, or another parameter list "
                           "is passed than the one registered): call set_gradient_arena(params, flat) for the CURRENT parameters first")
    if any(tuple(v.shape) != tuple(p.shape) for p, v in zip(params, views)):
        raise RuntimeError("gradient arena: the views do not match the parameters' shapes (views of an earlier registration)")
    pairs = [(p.grad, v) for p, v in zip(params, views) if p.grad is not None and p.grad.data_ptr() != v.data_ptr()]
    if pairs:
        if to_arena:
            torch._foreach_copy_([v for _, v in pairs], [g for g, _ in pairs])
        else:
            torch._foreach_copy_([g for g, _ in pairs], [v for _, v in pairs])
    return len(pairs)
