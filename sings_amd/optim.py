"""The optimiser of the training loop on the hot path: ``FusedAdam`` -- ``torch.optim.Adam.step()`` (gs_trainer.py:240-262) as ONE HIP
launch over every parameter of every group (``sg_adam_step``, csrc/sg_optim.hip), capturable into the step's HIP graph -- and the
reference's two learning-rate schedules (utils/general.py:76-126) as plain host functions.

What the launch reads:

    the flat fp32 gradient arena           ``grad_arena.set_gradient_arena``: the big gradients are written there by the kernels that produce
                                           them, the small ones are copied in by ``grad_arena.arena_sync``
    two flat moment buffers                ``exp_avg`` / ``exp_avg_sq`` with the arena's layout (a feature-minor plane is walked in
                                           memory order in all four arrays)
    a segment and a chunk table            one record per parameter tensor / per 4 096 consecutive elements of one tensor
    a per-group row [G][8] of fp32         w1 = 1 - beta1, b2 = beta2, w2 = 1 - beta2, c2 = sqrt(1 - beta2^t), eps,
                                           neg_step = -(lr_t / (1 - beta1^t)): computed in double on the host, rounded once

The row lives in device memory, so the learning rate and the bias corrections change under a replayed graph: ``advance()`` is the
host half of a step (counts the step, computes the rows, enqueues their copy), ``apply()`` the device half (what a graph holds).
There is no CPU fallback: host tensors raise.
"""
import math
import weakref

import numpy as np
import torch

from . import _lib
from ._marshal import adam_step as _adam_step
from .grad_arena import arena_sync, is_feature_minor, like_layout

HYPER_COLUMNS = 8                        # floats per group row (six used)
_RING = 64                               # pinned copies of the table in flight before advance() would have to wait for one


# ---- schedules (host, double) ---------------------------------------------------------------------------------------------------
def expon_lr(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """``get_expon_lr_func`` (utils/general.py:76-109): log-linear from ``lr_init`` (step 0) to ``lr_final`` (``max_steps``), times a
    sine ease-in from ``lr_delay_mult`` over the first ``lr_delay_steps`` steps.  -> ``step -> lr``."""
    def lr(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return lr


def cosine_annealing_lr(lr_init, lr_final, lr_delay_steps, T_max):
    """``get_cosine_annealing_lr`` (utils/general.py:112-126): ``lr_init`` until ``lr_delay_steps``, then half a cosine down to
    ``lr_final`` at ``T_max`` (and, like the reference, up again beyond it).  -> ``step -> lr``."""
    def lr(step):
        if step < lr_delay_steps:
            return lr_init
        cosine = math.cos(math.pi * (step - lr_delay_steps) / (T_max - lr_delay_steps))
        return lr_final + 0.5 * (lr_init - lr_final) * (1 + cosine)
    return lr


# ---- host tables ----------------------------------------------------------------------------------------------------------------
def hyper_row(lr, beta1, beta2, eps, step):
    """The group's row of step ``step`` (>= 1): double arithmetic, each entry rounded once to fp32."""
    row = np.zeros(HYPER_COLUMNS, np.float64)
    row[:6] = (1.0 - beta1, beta2, 1.0 - beta2, math.sqrt(1.0 - beta2 ** step), eps, -(lr / (1.0 - beta1 ** step)))
    return row.astype(np.float32)


def build_tables(addresses, numels, groups, chunk=None, active_groups=None):
    """-> (segments [S,4] int64, chunks [C,2] int32) of ``sg_adam_step`` for parameter tensors at ``addresses`` with ``numels``
    elements that lie one behind the other in the arena.  Pure host arithmetic: every element of every segment is in exactly one
    chunk, and a chunk never crosses a segment.
    ``active_groups`` (group indices; None: all): the chunk table lists the segments of these groups only -- the launch never touches
    the others -- while the segment table, and with it every offset into the arena and the moments, keeps the full layout."""
    chunk = int(_lib.load().sg_adam_chunk_elements()) if chunk is None else int(chunk)
    seg = np.zeros((len(numels), 4), np.int64)
    rows, off = [], 0
    for s, (a, n, g) in enumerate(zip(addresses, numels, groups)):
        n = int(n)
        if n < 0 or n >= 2 ** 31:
            raise ValueError(f"FusedAdam: a parameter of {n} elements (must be 0 .. 2^31 - 1)")
        seg[s] = (int(a), off, n, int(g))
        first = np.arange(0, n if active_groups is None or int(g) in active_groups else 0, chunk, dtype=np.int64)
        rows.append(np.stack([np.full_like(first, s), first], 1))
        off += n
    chunks = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
    return seg, np.ascontiguousarray(chunks.astype(np.int32))


# ---- the row map of a change of the set ------------------------------------------------------------------------------------------
def take_rows(t, src):
    """``t`` [n, ...] through the row map ``src`` (int64 [n_new], entries -1 .. n-1) -> a fresh contiguous [n_new, ...] tensor: row i is
    a bit copy of ``t[src[i]]``, or +0.0 where ``src[i] == -1`` (a row that starts its life).  Every change of the set of Gaussians is
    this one operation on whatever is kept per row: clone + prune, rows appended by a subdivision, a plain ``t[keep]``.  CPU or GPU
    tensors; an index outside -1 .. n-1 is a ValueError (a host check: this runs between steps)."""
    n = int(t.shape[0])
    if src.dtype != torch.int64 or src.dim() != 1:
        raise ValueError(f"take_rows: src must be a 1-D int64 tensor (got {src.dtype}, {src.dim()}-D)")
    if src.numel() and (int(src.min()) < -1 or int(src.max()) >= n):
        raise ValueError(f"take_rows: src has entries outside -1 .. {n - 1}")
    out = torch.zeros((int(src.shape[0]),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    kept = torch.nonzero(src >= 0).reshape(-1)
    out.index_copy_(0, kept, t.index_select(0, src[kept]))
    return out


class FusedAdam:
    """``torch.optim.Adam`` (no weight decay, no amsgrad, not maximize) for GPU fp32 parameters whose gradients live in a flat arena.

    ``param_groups``: dicts with ``params``, ``lr`` and ``name`` (as ``AvatarTrainer`` builds them); ``param_groups[i]["lr"]`` may be
    assigned before every step.  ``grad_flat`` / ``grad_views``: the arena and what ``grad_arena.set_gradient_arena`` returned for the same
    parameters in the same order (``None``: bound later with ``bind_arena``).

        advance()    host half, once per step: step counts, the [G][8] table into a pinned buffer, its copy enqueued on the current
                     stream.  Never synchronises (a ring of pinned buffers; the host would have to run 64 steps ahead of the GPU).
        apply()      device half, capturable: ``grad_arena.arena_sync(params, views, True)``, then the one launch
        step()       advance(); apply()
    """

    def __init__(self, param_groups, grad_flat=None, grad_views=None, betas=(0.9, 0.999), eps=1e-15):
        self.param_groups = []
        for i, g in enumerate(param_groups):
            g = dict(g)
            g["params"] = list(g["params"])
            g.setdefault("name", f"group{i}")
            g.setdefault("betas", tuple(betas)); g.setdefault("eps", float(eps))
            if "lr" not in g:
                raise ValueError(f"FusedAdam: group {g['name']} has no lr")
            self.param_groups.append(g)
        params = self._params()
        if not params:
            raise ValueError("FusedAdam: no parameters")
        for name, p in zip(self._names(), params):
            if not torch.is_tensor(p) or not p.is_cuda:
                raise RuntimeError(f"FusedAdam: parameter {name} must live on the GPU (no CPU fallback)")
            if p.dtype != torch.float32:
                raise RuntimeError(f"FusedAdam: parameter {name} must be float32 (got {p.dtype})")
        if len({id(p) for p in params}) != len(params):
            raise ValueError("FusedAdam: a parameter appears twice")
        self.dev = params[0].device
        self.steps = [0] * len(self.param_groups)
        n = sum(p.numel() for p in params)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=self.dev)
        G = len(self.param_groups)
        self.hyper = torch.zeros((G, HYPER_COLUMNS), dtype=torch.float32, device=self.dev)
        self._pinned = torch.zeros((_RING, G, HYPER_COLUMNS), dtype=torch.float32).pin_memory()
        self._events, self._slot = [None] * _RING, 0
        self.grad_flat = self.grad_views = self._reg = None
        self._active = None                                       # group names that take part in a step (None: all)
        if grad_flat is not None:
            self.bind_arena(grad_flat, grad_views)

    # ---- what is registered
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _names(self):
        return [f"{g['name']}[{i}]" for g in self.param_groups for i in range(len(g["params"]))]

    def _offsets(self):
        o, out = 0, []
        for p in self._params():
            out.append(o); o += p.numel()
        return out

    def _moment_views(self, flat):
        """Per-parameter views of a flat moment buffer, in each parameter's own shape and memory layout."""
        return [like_layout(flat[o:o + p.numel()], p) for o, p in zip(self._offsets(), self._params())]

    def _active_groups(self):
        return None if self._active is None else {gi for gi, g in enumerate(self.param_groups) if g["name"] in self._active}

    def _is_active(self, g):
        return self._active is None or g["name"] in self._active

    def set_active(self, names=None):
        """The groups that take part in the following steps (``names``: group names; None: all, the default).  An inactive group is a
        parameter set the reference's Adam skips because it has no gradient (frozen decoders, gs_trainer.py:225-226): its parameters,
        moments and step count are never touched, ``advance()`` does not count a step for it, and ``apply()`` asks no gradient of it.
        The chunk table of the launch lists the active groups only; segment offsets keep the full layout, so nothing is re-indexed."""
        if names is not None:
            names = set(names)
            known = {g["name"] for g in self.param_groups}
            if not names <= known:
                raise ValueError(f"FusedAdam.set_active: unknown groups {sorted(names - known)}")
            if not names:
                raise ValueError("FusedAdam.set_active: no active group")
            if names == known:
                names = None
        if names == self._active:
            return
        self._active = names
        if self._reg is not None:
            self._build_tables(self._params())
        self._grads_checked = False

    def _build_tables(self, params):
        group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        seg, chunks = build_tables([p.data_ptr() for p in params], [p.numel() for p in params], group_of,
                                   active_groups=self._active_groups())
        self.segments = torch.from_numpy(seg).to(self.dev)
        self.chunks = torch.from_numpy(chunks).to(self.dev)

    def bind_arena(self, grad_flat, grad_views):
        """(Re)bind the gradient arena of the CURRENT parameters and rebuild the device tables."""
        params = self._params()
        n = sum(p.numel() for p in params)
        if not grad_flat.is_cuda or grad_flat.dtype != torch.float32 or grad_flat.numel() != n or not grad_flat.is_contiguous():
            raise ValueError(f"FusedAdam: grad_flat must be a contiguous fp32 GPU buffer of {n} elements (no CPU fallback)")
        if len(grad_views) != len(params) or any(tuple(v.shape) != tuple(p.shape) for v, p in zip(grad_views, params)):
            raise ValueError("FusedAdam: grad_views do not match the parameters")
        for name, p in zip(self._names(), params):
            if not (p.is_contiguous() or is_feature_minor(p)):
                raise ValueError(f"FusedAdam: parameter {name} must be contiguous (or a feature-minor tri-plane plane)")
        if self.exp_avg.numel() != n:
            raise RuntimeError("FusedAdam: the moments were not re-indexed for the new sizes (remap_rows)")
        self._build_tables(params)
        self.grad_flat, self.grad_views = grad_flat, list(grad_views)
        self._reg = [(weakref.ref(p), p.data_ptr()) for p in params]
        self._grads_checked = False

    def _check_current(self, params):
        reg = self._reg
        if reg is None or len(reg) != len(params) or any(r() is not p or a != p.data_ptr() for (r, a), p in zip(reg, params)):
            raise RuntimeError("FusedAdam: the registration is stale (a registered parameter was replaced or moved: densify / prune): "
                               "remap_rows(...) and bind_arena(grad_flat, grad_views) for the CURRENT parameters first")

    # ---- the step
    def advance(self):
        """Host half of a step: every ACTIVE group's step count + 1, its row from ITS ``lr`` / ``betas`` / ``eps``, H2D copy enqueued.
        (An inactive group's count stays; its row, which no chunk of the launch refers to, is zero.)"""
        slot = self._slot
        self._slot = (slot + 1) % _RING
        ev = self._events[slot]
        if ev is not None and not ev.query():
            ev.synchronize()                                      # (only if the host is a whole ring ahead of the GPU)
        host = self._pinned[slot]
        for gi, g in enumerate(self.param_groups):
            if not self._is_active(g):
                host[gi].zero_()
                continue
            self.steps[gi] += 1
            b1, b2 = g["betas"]
            host[gi] = torch.from_numpy(hyper_row(float(g["lr"]), float(b1), float(b2), float(g["eps"]), self.steps[gi]))
        self.hyper.copy_(host, non_blocking=True)
        if ev is None:
            ev = self._events[slot] = torch.cuda.Event()
        ev.record()

    def _check(self):
        """Host checks before anything is enqueued: the registration is current, and (once per binding and set of active groups)
        every parameter of an active group has a gradient."""
        params = self._params()
        self._check_current(params)
        if not self._grads_checked:
            active = [self._is_active(g) for g in self.param_groups for _ in g["params"]]
            for name, p, on in zip(self._names(), params, active):
                if on and p.grad is None:
                    raise RuntimeError(f"FusedAdam: parameter {name} has no gradient -- its arena slot would feed the update a stale "
                                       "one; every registered parameter must take part in the backward")
            self._grads_checked = True
        return params

    def apply(self, sync=True):
        """Device half: the gradients that are not in their arena slot yet are copied in (``sync=False``: the caller has done that, and
        the arena holds e.g. all-reduced gradients), then ONE launch updates every parameter and both moments."""
        params = self._check()
        if sync:
            arena_sync(params, self.grad_views, True)
        _adam_step(self.segments, self.chunks, self.hyper, self.grad_flat, self.exp_avg, self.exp_avg_sq)

    def step(self):
        self._check()                                             # (a refused step is not counted)
        self.advance()
        self.apply()

    def live_tensors(self):
        """What ``apply()`` changes: every parameter's data and both moments.  A caller that runs it without the run being a step (a
        capture's warm-up, with the launch in the captured body) clones these before and copies them back after -- and ``steps``, the
        host list, with them."""
        return [p.detach() for p in self._params()] + [self.exp_avg, self.exp_avg_sq]

    def zero_grad(self, set_to_none=True):
        for p in self._params():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    # ---- torch.optim.Adam's state format
    def state_dict(self):
        state, groups, k = {}, [], 0
        ms, vs = self._moment_views(self.exp_avg), self._moment_views(self.exp_avg_sq)
        for gi, g in enumerate(self.param_groups):
            idx = list(range(k, k + len(g["params"])))
            for i in idx:
                state[i] = {"step": torch.tensor(float(self.steps[gi])), "exp_avg": ms[i].clone(), "exp_avg_sq": vs[i].clone()}
            out = {key: val for key, val in g.items() if key != "params"}
            out.update(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                       decoupled_weight_decay=False, params=idx)
            groups.append(out)
            k += len(idx)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("FusedAdam: the state dict's groups do not match this optimiser's")
        for g in groups:
            if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedAdam: weight decay, amsgrad and maximize are not supported")
        ms, vs = self._moment_views(self.exp_avg), self._moment_views(self.exp_avg_sq)
        params, k = self._params(), 0
        for gi, (saved, g) in enumerate(zip(groups, self.param_groups)):
            seen = set()
            for i in saved["params"]:
                st = sd["state"].get(i)
                if st is None:                                    # (torch creates a parameter's state at its first step)
                    ms[k].zero_(); vs[k].zero_()
                else:
                    if tuple(st["exp_avg"].shape) != tuple(params[k].shape):
                        raise ValueError(f"FusedAdam: state of parameter {i} has shape {tuple(st['exp_avg'].shape)}")
                    ms[k].copy_(st["exp_avg"]); vs[k].copy_(st["exp_avg_sq"])
                    seen.add(int(float(st["step"])))
                k += 1
            if len(seen) > 1:
                raise ValueError(f"FusedAdam: the parameters of group {g['name']} are at different steps {sorted(seen)}")
            self.steps[gi] = seen.pop() if seen else 0
            for key in ("lr", "betas", "eps"):
                if key in saved:
                    g[key] = saved[key]

    # ---- a densify / prune of one parameter's rows
    def remap_rows(self, old, new, clone_mask, keep_mask):
        """Parameter ``old`` becomes ``new`` = ``cat([old, old[clone_mask]])[keep_mask]``: its moments become
        ``cat([m, zeros_like(m[clone_mask])])[keep_mask]`` (cat_tensors_to_optimizer / _prune_optimizer), every other parameter's are
        copied, the step counts stay.  The arena is unbound: ``bind_arena`` with the new parameters' arena before the next step.
        (``reindex_rows`` with the masks written as a row map.)"""
        n, n_clones = int(old.shape[0]), int(old.detach()[clone_mask].shape[0])
        src = torch.cat([torch.arange(n, device=self.dev), torch.full((n_clones,), -1, dtype=torch.int64, device=self.dev)])[keep_mask]
        self.reindex_rows(old, new, src)

    def reindex_rows(self, old, new, src):
        """Parameter ``old`` [n, ...] becomes ``new`` [n_new, ...] whose row i is old row ``src[i]`` or, where ``src[i] == -1``, a new
        one: both moments go through ``take_rows`` (kept rows bit for bit, zeros for the new ones), every other parameter's are
        copied, the step counts stay.  The arena is unbound: ``bind_arena`` with the new parameters' arena before the next step."""
        params = self._params()
        at = [i for i, p in enumerate(params) if p is old]
        if len(at) != 1:
            raise ValueError("FusedAdam.reindex_rows: `old` is not a registered parameter")
        at = at[0]
        if not new.is_cuda or new.dtype != torch.float32:
            raise RuntimeError("FusedAdam.reindex_rows: `new` must be a float32 GPU tensor (no CPU fallback)")
        with torch.no_grad():
            old_m, old_v = self._moment_views(self.exp_avg), self._moment_views(self.exp_avg_sq)
            new_mv = [take_rows(x[at], src) for x in (old_m, old_v)]
            if tuple(new_mv[0].shape) != tuple(new.shape):
                raise ValueError(f"FusedAdam.reindex_rows: `src` gives {tuple(new_mv[0].shape)}, `new` is {tuple(new.shape)}")
            k = 0
            for g in self.param_groups:
                for i in range(len(g["params"])):
                    if k == at:
                        g["params"][i] = new
                    k += 1
            n = sum(p.numel() for p in self._params())
            flats = [torch.zeros(n, dtype=torch.float32, device=self.dev) for _ in range(2)]
            for flat, olds, mine in zip(flats, (old_m, old_v), new_mv):
                for i, dst in enumerate(self._moment_views(flat)):
                    dst.copy_(mine if i == at else olds[i])
            self.exp_avg, self.exp_avg_sq = flats
        self.grad_flat = self.grad_views = self._reg = None
