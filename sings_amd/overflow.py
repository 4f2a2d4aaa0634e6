"""Pair capacity and list-length hints: of the three autograd rasterizer ops (rasterizer.py, skinned.py) and, in a section of its
own (``EngineCapacity``), of the forward-only animator's pre-allocated engines (posed.py).

The workspaces of a call hold `cap` (tile, Gaussian) pairs; the forward reports the count R it produced.  The mode decides when R is read:
  "sync"     (default; the drop-in guarantee) every forward knows R before it returns and re-runs with a larger workspace if needed:
             NEVER a wrong frame.  The binning kernel publishes R to a pinned, mapped host word the moment it exists
             (SgRasterSettings.count_signal, include/sings_hip.h), so the call returns while the composite kernel still runs.
  "async"    opt-in: the forward copies (R, flag word) to pinned host memory behind its kernels and returns at once; the next forward
             on the device looks at it.  The capacity keeps 2x headroom over the largest R seen and the FIRST call of every (device, P,
             image size) is read synchronously, so an overflow needs a > 2x jump between consecutive frames; THAT frame then rendered
             the background with zero gradients, and the next call raises RuntimeError (``on_overflow="warn"``: a RuntimeWarning).
  "deferred" opt-in: no host read at all (a whole step can be captured into a HIP graph): every forward folds (R, flag word) into a
             per-device accumulator ON THE DEVICE; ``check_deferred_overflow()`` reads and resets it.
A "sync" forward's count word also says whether every tile list held <= 512 entries (SG_COUNT_FLAG_HALF_ROWS) / <= 8192 entries
(SG_COUNT_FLAG_HALF_LONG_ROWS); the next frame of that (device, P, W, H) may then pass SG_FLAG_SHORT_LISTS / SG_FLAG_LONG_ROWS.  A
hinted frame that meets a longer list reports NUM_RENDERED_LONG_LIST and is rendered again without the hint before the call returns;
where R is not read (the fused LBS ops pass the long-rows hint in every mode), that is a background frame reported like an overflow.

The decision layer (``plan`` .. ``EngineCapacity``) works on plain ints and bools; the I/O layer below it feeds it from
the early-count words, the pinned ring of "async" results and the "deferred" accumulator, and ``run_forward`` is the forward loop.
"""
import atexit
import ctypes as C
import threading
import warnings

import torch

from . import _lib

_capacity_hint = {}                    # device index -> pairs (rasterizer._capacity_hint is this object: grown and cleared in place)
_mode = {"mode": "sync", "on_overflow": "raise"}
_seen = {}                             # device index -> set of (P, W, H) signatures already checked synchronously
_short_ok = {}                         # (device index, P, W, H) -> the last frame's lists were all <= 512 entries
_rows_ok = {}                          # (device index, P, W, H) -> ... all <= 8192 entries
_HINT_TABLES = {_lib.FLAG_SHORT_LISTS: _short_ok, _lib.FLAG_LONG_ROWS: _rows_ok}


# ---- decision layer: plain ints and bools ---------------------------------------------------------------------------------------
def plan(dev_index, P, W, H, capturing=False):
    """(capacity, read R synchronously?, signature (P, W, H)) of the next forward on device ``dev_index``."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    mode = _mode["mode"]
    cap = max(_capacity_hint.get(dev_index, 0), 4 * P + T, 1 << 16)
    sig = (P, W, H)
    first = sig not in _seen.setdefault(dev_index, set()) or dev_index not in _capacity_hint
    sync = (mode == "sync" or (mode == "async" and first)) and not capturing
    return cap, sync, sig


def grown(R):
    """The capacity a count of R pairs asks for: 2x headroom."""
    return 2 * R + 1024


def _grow(dev_index, R):
    _capacity_hint[dev_index] = max(_capacity_hint.get(dev_index, 0), grown(R))      # (never shrinks)


def done_sync(dev_index, R, sig):
    """A forward of signature ``sig`` read its count R before returning."""
    _seen[dev_index].add(sig)
    _grow(dev_index, R)


def learn(key, word):
    """The flags of a "sync" forward's early-count word into the hint tables of ``key`` = (device index, P, W, H); bit 63 says the
    word arrived (not after a timed-out wait: that read the header instead)."""
    if word >> 63:
        _short_ok[key] = bool((word >> 32) & _lib.COUNT_FLAG_HALF_ROWS)
        _rows_ok[key] = bool((word >> 32) & _lib.COUNT_FLAG_HALF_LONG_ROWS)


def hint_flags(key, hints, sync, debug, needs_sync):
    """The SG_FLAG_* bits of ``hints`` a forward of ``key`` may pass: those the last frame read of ``key`` held; none in debug mode,
    none without a synchronous read if ``needs_sync``."""
    if debug or (needs_sync and not sync):
        return 0
    return sum(f for f in hints if _HINT_TABLES[f].get(key, False))      # (distinct bits)


def forget(key, hints):
    """A hinted frame of ``key`` met a longer list: the hints it consulted are off until a frame is read again."""
    for f in hints:
        _HINT_TABLES[f][key] = False


def _drop_hints(dev_index=None):
    for tbl in (_short_ok, _rows_ok):
        for k in [k for k in tbl if dev_index is None or k[0] == dev_index]:
            del tbl[k]


def _report(msg, on_overflow):
    if (on_overflow or _mode["on_overflow"]) == "raise":
        raise RuntimeError(msg)
    warnings.warn(msg, RuntimeWarning, stacklevel=4)


def absorb_async(dev_index, results, on_overflow=None):
    """Finished "async" results [(R, header flag word, capacity)] of device ``dev_index``: grow the capacity to the largest R, drop
    the device's hints if a hinted list was too long, then report (``on_overflow``, default the mode's: raise or warn) a violated hint
    and the largest R that exceeded its capacity.  Returns the largest R, or None without results."""
    if not results:
        return None
    Rmax = max(R for R, _, _ in results)
    over = [(R, cap) for R, _, cap in results if R > cap]
    _grow(dev_index, Rmax)
    if any(f & _lib.HDR_FLAG_LONG_LIST for _, f, _ in results):      # a learned hint did not hold for an earlier (fused LBS) forward
        _drop_hints(dev_index)
        _report(f"sings_amd: an earlier forward on cuda:{dev_index} met a tile list longer than the row its learned hint promised: "
                f"that frame rendered the background and received zero gradients; the hints of the device are dropped", on_overflow)
    if over:
        worst, worst_cap = max(over, key=lambda rc: rc[0])
        _report(f"sings_amd: an earlier forward on cuda:{dev_index} produced {worst} (tile, Gaussian) pairs for a capacity of "
                f"{worst_cap}: that frame rendered the background and received zero gradients; the capacity is now "
                f"{_capacity_hint[dev_index]} (set_overflow_check('sync') checks every forward before returning)", on_overflow)
    return Rmax


def absorb_deferred(dev_index, R, flags):
    """The "deferred" accumulator of ``dev_index`` (largest R, OR of the header flag words, each set on the device against the
    capacity THAT forward ran with): grow, drop the device's hints on a long list, raise if any flag is set.  Returns R, or None if
    there was no forward."""
    if R == 0 and flags == 0:
        return None
    _grow(dev_index, R)
    long_list = flags & _lib.HDR_FLAG_LONG_LIST
    if long_list:
        _drop_hints(dev_index)
    if flags:
        raise RuntimeError(f"sings_amd: a deferred forward produced up to {R} (tile, Gaussian) pairs, more than its capacity"
                           f"{' (or met a tile list longer than the row its learned hint promised: the hints are dropped)' if long_list else ''}: "
                           f"it rendered the background and no gradients; the capacity is now {_capacity_hint[dev_index]}")
    return R


def capacity_pairs(device):
    """The pair capacity the policy holds for ``device`` (None before its first forward)."""
    return _capacity_hint.get(torch.device(device).index)


def set_overflow_check(mode="sync", on_overflow=None, capacity_pairs=None, device=None):
    """Select when the pair count of a forward is checked against the capacity: "sync" (default) | "async" | "deferred"."""
    if mode not in ("async", "sync", "deferred"):
        raise ValueError("mode must be 'async', 'sync' or 'deferred'")
    _mode["mode"] = mode
    if on_overflow is not None:
        if on_overflow not in ("warn", "raise"):
            raise ValueError("on_overflow must be 'warn' or 'raise'")
        _mode["on_overflow"] = on_overflow
    if capacity_pairs is not None:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        _capacity_hint[dev.index] = int(capacity_pairs)


def set_deferred_overflow_check(on=True, capacity_pairs=None, device=None):
    """Round-1 name: ``on`` selects "deferred", otherwise back to the default "sync"."""
    set_overflow_check("deferred" if on else "sync", capacity_pairs=capacity_pairs, device=device)


# ---- decision layer: the pre-allocated engines of the forward-only animator (posed.FrameAnimator) ---------------------------------
class EngineCapacity:
    """Pair capacity and long-rows hint of a set of engines that render frames nobody differentiates.  The workspaces are held for a
    whole animation and every count is read before its frame is handed out, so the policy is 8 pairs per Gaussian and 1.25x growth:
    deliberately not the 4 P / 2x of the autograd ops above, whose workspaces live for one call."""

    def __init__(self):
        # SG_FLAG_LONG_ROWS (direct binning of few-tile frames: no tile list beyond 16384 entries) is passed optimistically; a frame
        # that reports a longer list is rendered again without the hint, which then stays off
        self.long_rows = True

    @staticmethod
    def floor(cap, P, W, H):
        """The capacity of a first set of engines: what is held already, 8 pairs per Gaussian + 1 per tile, at least 2^16."""
        return max(cap, 8 * P + ((W + 15) // 16) * ((H + 15) // 16), 1 << 16)

    @staticmethod
    def grown(need):
        """The capacity a count of ``need`` pairs asks for."""
        return need + need // 4 + 1024

    def settle(self, counts, cap, flags=0):
        """Frames rendered with capacity ``cap`` have reported their pair counts (``num_rendered()``, or the header's count and
        flag word of a frame whose count was not read): drops the long-rows hint for good if a list outgrew its row.  Returns None
        if the frames stand, else the capacity to render them again with: ``cap`` after a NUM_RENDERED_LONG_LIST count (it hides
        the frame's R: the plain path counts it), ``grown(R)`` if R exceeded ``cap``."""
        if min(counts) == _lib.NUM_RENDERED_LONG_LIST:           # (also of a frame launched before an earlier one dropped the hint)
            self.long_rows = False
            return cap
        long_list = bool(flags & _lib.HDR_FLAG_LONG_LIST)        # (the header's R is the frame's: it may also have overflowed)
        if long_list:
            self.long_rows = False
        need = max(counts)
        if need > cap:
            return self.grown(need)
        return cap if long_list else None

    def redo(self, cap, render):
        """A unit failed ``settle``, which asked for ``cap``: ``render(cap)`` renders it again with at least that capacity and reads
        its counts -> (result, counts, the capacity it ran with).  Returns the result that stands.  The plain path reports the
        exact R and ``grown(R) >= R``, so two renders are enough (hint dropped, then grown); a third failure is an error."""
        for _ in range(2):
            result, counts, ran_with = render(cap)
            cap = self.settle(counts, ran_with)
            if cap is None:
                return result
        raise RuntimeError(f"sings_amd: a frame reported the pair counts {list(counts)} for a capacity of {ran_with} after two "
                           f"re-renders (hint dropped, capacity grown): the counts of one frame do not repeat")


# ---- I/O layer: early-count words ------------------------------------------------------------------------------------------------
_signal = {}                          # device index -> [host address, device address, next slot] of the early-count words
_SIGNAL_SLOTS = 64
_signal_lock = threading.Lock()


def _signal_slot(dev):
    """(device address, host address) of the next early-count word of ``dev`` (a ring: a "sync" forward consumes its word
    before it returns, so slots are only shared by calls that are 64 forwards apart).  Thread-safe (a forward on the main
    thread and one on an autograd / data-loader thread must not be handed the same word); the ring is released at
    interpreter exit only (``reset_overflow_state`` rewinds its cursor: another thread may hold a slot)."""
    with _signal_lock:
        sg = _signal.get(dev.index)
        if sg is None:
            h, d = C.c_void_p(), C.c_void_p()
            with torch.cuda.device(dev):
                _lib.check(_lib.load().sg_signal_alloc(_SIGNAL_SLOTS, C.byref(h), C.byref(d)), "sg_signal_alloc")
            sg = _signal[dev.index] = [h.value, d.value, 0]
        k = sg[2] % _SIGNAL_SLOTS
        sg[2] += 1
        return sg[1] + 8 * k, sg[0] + 8 * k


def _free_signal_rings_at_exit():
    # kernels of a forward still in flight write their slot: drain the devices before the pinned words go
    try:
        if torch.cuda.is_initialized():
            torch.cuda.synchronize()
    except Exception:
        return                                        # (the process is exiting: leaking 512 pinned bytes is harmless)
    with _signal_lock:
        for sg in _signal.values():
            try:
                _lib.load().sg_signal_free(C.c_void_p(sg[0]))
            except Exception:
                pass
        _signal.clear()


atexit.register(_free_signal_rings_at_exit)


# ---- I/O layer: results that were not read before the forward returned -------------------------------------------------------------
_pending = {}                          # device index -> list of [pinned (R, flag word), event, cap] of async forwards
_accum = {}                            # device index -> int32[2] device tensor: max R, OR of flags (deferred mode)
_ring = {}                             # device index -> [pinned int32[_RING, 2], next slot]
_RING = 16
_flag_bit_cache = {}


def frames_header(binning, K, bin_bytes):
    """int32[2] (largest R, OR of the flag words) of the K binning headers of a K-frame call (a frame's "long list" bit must not hide
    another frame's "overflow" bit).  The OR is the sum over the bits of their per-bit maxima (torch has no bitwise-or reduction)."""
    h = binning.view(K, bin_bytes)[:, :8].view(torch.int32)
    bits = _flag_bit_cache.get(h.device)
    if bits is None:
        bits = _flag_bit_cache[h.device] = (2 ** torch.arange(16, dtype=torch.int32)).to(h.device)
    flags = (h[:, 1:2] & bits).amax(0).sum().to(torch.int32)
    return torch.stack([h[:, 0].amax(), flags]).contiguous()


def _queue_unread(dev, hdr, cap):
    """The header (R, flag word) of a forward that did not read R: into the device accumulator ("deferred" mode, graph capture) or,
    behind the forward's kernels, to the pinned ring that the next forward looks at ("async" mode)."""
    if _mode["mode"] == "deferred" or torch.cuda.is_current_stream_capturing():
        acc = _accum.get(dev.index)
        if acc is None:
            acc = _accum[dev.index] = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.maximum(acc, hdr, out=acc)               # R < 2^31; one tiny launch, capturable into a HIP graph
        return
    ring = _ring.get(dev.index)
    if ring is None:
        ring = _ring[dev.index] = [torch.empty((_RING, 2), dtype=torch.int32).pin_memory(), 0]
    host = ring[0][ring[1] % _RING]                    # (at most two entries are pending at any time: _drain_async)
    ring[1] += 1
    host.copy_(hdr, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    _pending.setdefault(dev.index, []).append([host, ev, cap])


def _drain_async(dev, wait_all=False, on_overflow=None):
    """Absorb the (R, flag word) copies of earlier async forwards on ``dev``.  Entries older than the newest one are waited for
    (their forward was issued at least one call ago); returns the largest R seen, or None."""
    lst = _pending.get(dev.index)
    if not lst:
        return None
    results, keep = [], []
    for k, (host, ev, cap) in enumerate(lst):
        if not wait_all and k == len(lst) - 1 and not ev.query():
            keep.append(lst[k])                        # the newest one may still be in flight: leave it for the next call
            continue
        ev.synchronize()
        results.append((int(host[0]) & 0xffffffff, int(host[1]), cap))
    _pending[dev.index] = keep
    return absorb_async(dev.index, results, on_overflow)


def check_deferred_overflow(device=None):
    """Largest pair count of the forwards since the last poll on ``device`` (one D2H read = one host synchronisation;
    "deferred" mode: the device-side accumulator; "async" mode: the pending copies).  Raises RuntimeError if one of them
    exceeded its capacity, after growing the capacity used by the following calls.  None if there was no forward."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if _mode["mode"] != "deferred" and dev.index not in _accum:
        return _drain_async(dev, wait_all=True, on_overflow="raise")
    acc = _accum.get(dev.index)
    if acc is None:
        return None
    R, flags = (int(v) for v in acc.cpu())
    acc.zero_()
    return absorb_deferred(dev.index, R, flags)


def reset_overflow_state(device=None):
    """Forget capacities, checked signatures, hints and pending results (tests; after a change of scene scale)."""
    idx = None if device is None else torch.device(device).index
    _drop_hints(idx)
    for d in (_capacity_hint, _seen, _pending, _accum):
        if idx is None:
            d.clear()
        else:
            d.pop(idx, None)
    # The pinned early-count ring is NOT freed here: a forward on another thread may already hold a slot address the
    # scan kernel will write and the host will spin on; only its cursor is rewound.  The ring lives until interpreter exit.
    with _signal_lock:
        for k, sg in _signal.items():
            if idx is None or k == idx:
                sg[2] = 0


# ---- the forward loop of the three autograd ops ------------------------------------------------------------------------------------
def run_forward(dev, P, W, H, s, launch, header, *, debug, hints, hints_need_sync, early_count, base_flags=0):
    """The forward of an op with settings ``s``: ``launch(cap, flags, sync)`` sizes its workspaces, sets ``s.flags`` and calls the
    entry point, returning the frame counts if ``sync`` (else None); it runs again without the hints after a too long hinted list and
    with a grown capacity after R > cap.  ``header()``: the int32[2] (R, flag word) device tensor of an unread last launch.  The op
    passes ``base_flags`` and the learned ``hints`` (only when R is read, if ``hints_need_sync``); ``early_count``: a "sync" forward
    reads R from the early-count word and learns the hints from it.  Returns (capacity, counts of the last launch or None)."""
    if _mode["mode"] == "async":
        _drain_async(dev)
    cap, sync, sig = plan(dev.index, P, W, H, torch.cuda.is_current_stream_capturing())
    key = (dev.index,) + sig
    hinted = hint_flags(key, hints, sync, debug, hints_need_sync)
    with torch.cuda.device(dev):
        if early_count and sync and not debug:
            s.count_signal, s.count_signal_host = _signal_slot(dev)
        while True:
            counts = launch(cap, base_flags | hinted, sync)
            if not sync:
                break
            if hinted and min(counts) == _lib.NUM_RENDERED_LONG_LIST:      # the scene changed under the hint: again, without it
                forget(key, hints)
                hinted = 0
                continue
            R = max(counts)
            if R <= cap:
                break
            cap = grown(R)                              # workspace too small: grow and re-run
        if sync:
            done_sync(dev.index, R, sig)
            if early_count and s.count_signal_host:
                learn(key, C.c_uint64.from_address(s.count_signal_host).value)
        else:
            _queue_unread(dev, header(), cap)
    return cap, counts
