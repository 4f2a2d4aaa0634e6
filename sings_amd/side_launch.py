"""The side-launch schedule of the decode's backward pass: WHEN the work that runs beside the critical chain is issued.

Two mechanisms, their switches and their module-level state:

    weight gradients    `overlap_weight_grads`: sg_weight_grad on a side stream, each launch deferred by one kernel of the main chain
                        (`defer_side` / `flush_deferred`), joined when the backward pass ends
    tri-plane sorts     the point-only half of the tri-plane backward: issued by the forward (`prepare_triplane_backward_early`), held back
                        until `flush_triplane_prepare` (`prepare_triplane_backward_late`, `triplane_prepare_held`), or left to the backward

``pending()`` reports what is still waiting; ``reset_deferred()`` drops it after a pass that raised.
"""
import contextlib

import torch

# ---- capture order: the critical chain first ---------------------------------------------------------------------------------
# ROCm 7.2's graph executor gives every kernel node a queue while it walks the captured graph (DEBUG_HIP_GRAPH_DOT_PRINT=1 prints
# the assignment): the FIRST-captured dependent of a node stays on its queue, the k-th one goes to queue (q + k) mod 4 behind a
# signal; lists that share a queue run in list order, not in time order.  A side stream forked BEFORE the next kernel of the main
# chain is captured therefore KEEPS the main chain's queue and sends the main chain to another one: in the round-4 step each of the
# ten input-gradient kernels of the decoders' backward sat on a different queue than its predecessor (a signal hop each) and two of
# them behind a weight-gradient kernel of the side stream that happened to share their queue.  The weight-gradient launches are
# therefore DEFERRED by one kernel of the main chain: kept as a closure whose wait is an event recorded at the fork point (nothing
# starts later on the GPU) and issued right after the next input-gradient kernel (2.18 -> 2.06 ms per step, profiles/r05_graph_queues.log).
_DEFER = []


def defer_side(fn):
    _DEFER.append(fn)


def flush_deferred():
    try:
        while _DEFER:
            _DEFER.pop(0)()
    except BaseException:
        del _DEFER[:]
        raise


# ---- weight gradients beside the backward chain -----------------------------------------------------------------------------
# dW = dz^T x is needed by nobody downstream in the backward pass, and sg_weight_grad is bound by the matrix cores (one workgroup
# per CU) while the input-gradient kernels of the layers in front of it are bound by HBM: run on a second stream it fills the idle
# half of either.  Opt-in (`overlap_weight_grads(True)`): the gradients are complete when backward() RETURNS (the streams join in
# an end-of-backward callback), so parameters must not carry a .grad that autograd would add to DURING the pass -- true for the
# usual `optimizer.zero_grad()` (set_to_none) loop, not for gradient accumulation over several backward() calls.
_WG = {"on": False, "streams": {}, "armed": False}


def overlap_weight_grads(flag=True):
    """Run the decoders' weight-gradient kernels on a side stream, concurrently with the rest of the backward pass."""
    _WG["on"] = bool(flag)


def _wg_join():
    _WG["armed"] = False
    flush_deferred()
    for dev_index, side in _WG["streams"].items():
        torch.cuda.current_stream(torch.device("cuda", dev_index)).wait_stream(side)


def weight_grads_overlapped():
    return _WG["on"]


def wg_stream(dev):
    """The weight gradients' side stream on ``dev``; the first call of a backward pass arms the join at its end."""
    side = _WG["streams"].get(dev.index)
    if side is None:
        side = _WG["streams"][dev.index] = torch.cuda.Stream(dev)
    if not _WG["armed"]:
        del _DEFER[:]                                            # (nothing of an earlier pass may be pending when a new one arms the join)
        torch.autograd.Variable._execution_engine.queue_callback(_wg_join)     # joins when this backward pass ends
        _WG["armed"] = True
    return side


# ---- the point-only half of the tri-plane backward, early -------------------------------------------------------------------
# A quarter of the tri-plane backward (texel-major planes, zeroed gradient planes, three counting sorts of the points: ~120 us at
# 150 k points, all latency) needs neither dL/dfeats nor anything else the backward pass produces: it is launched from the FORWARD on
# a side stream, where the decoders' forward hides it, and the backward only waits for its event.  On by default outside HIP-graph
# capture; inside a capture (where an unjoined side stream is an error if backward() never runs) only after
# `prepare_triplane_backward_early(True)`; `False` turns it off everywhere, `None` restores the default.
_TP = {"mode": None, "streams": {}, "late": False}
_TP_PENDING = []


def prepare_triplane_backward_early(flag=True):
    _TP["mode"] = None if flag is None else bool(flag)


def prepare_triplane_backward_late(flag=True):
    """Hold the early preparation back until `flush_triplane_prepare()` (or the backward pass): beside the first decoder layers its
    counting sorts cost the forward chain more than they save (sings_amd.train_step issues it at the end of the forward)."""
    _TP["late"] = bool(flag)


@contextlib.contextmanager
def triplane_prepare_held(flag=True):
    """`prepare_triplane_backward_late(flag)` for the body, the previous setting afterwards (also when the body raises).  A
    preparation left pending by an earlier forward that raised is dropped first."""
    prev = _TP["late"]
    _TP["late"] = bool(flag)
    del _TP_PENDING[:]
    try:
        yield
    finally:
        _TP["late"] = prev


def triplane_prepare_stream(dev):
    """The side stream a forward on ``dev`` issues its preparation on; None: no early preparation (the backward does everything)."""
    if _TP["mode"] is False or (_TP["mode"] is None and torch.cuda.is_current_stream_capturing()):
        return None
    side = _TP["streams"].get(dev.index)
    if side is None:
        side = _TP["streams"][dev.index] = torch.cuda.Stream(dev)
    return side


def issue_triplane_prepare(launch):
    """Issue ``launch()`` now -- or, held back, by `flush_triplane_prepare()` / the backward."""
    if _TP["late"]:
        _TP_PENDING.append(launch)
    else:
        launch()


def flush_triplane_prepare(stream=None):
    """Issue a tri-plane backward preparation that `prepare_triplane_backward_late(True)` held back (``stream``: on that stream
    instead of the module's own side stream)."""
    while _TP_PENDING:
        fn = _TP_PENDING.pop(0)
        fn() if stream is None else fn(stream)


def pending():
    """-> (deferred launches, held-back preparations, join armed): what a pass has left waiting.  ``(0, 0, False)`` between passes."""
    return len(_DEFER), len(_TP_PENDING), _WG["armed"]


def reset_deferred():
    """Drop what a backward pass that RAISED left behind: deferred side-stream launches (their closures hold raw pointers to gradient
    tensors that no parameter adopted), a held-back tri-plane preparation, the armed end-of-backward join.  The step that raised is
    lost; the next one starts clean (sings_amd.train_step.AvatarStep.backward calls this on any exception)."""
    del _DEFER[:]
    del _TP_PENDING[:]
    _WG["armed"] = False
