"""What a training step reads and what a run that is not a step must put back -- the two pieces of ``AvatarTrainer``'s bookkeeping that
decide whether a captured step is correct, as plain host logic on torch tensors (CPU tensors in tests/test_step_inputs_host.py).

``StepInputs``: a captured graph holds its inputs' addresses, so a step's inputs live in tensors that stay where they are while
their shapes do; ``bind`` says when they could not stay.  ``preserved``: a capture's warm-up runs execute the step's body without being
steps; what they change besides the step's outputs is cloned before and copied back after.
"""
import contextlib

FIELDS = ("A", "idx", "gt", "mask", "lp_origins", "lp_bg")
SOURCES = ("A", "idx", "feed")              # the pose comes from A / from the pose tables' rows at idx / from the rows the feed draws


class StepInputs:
    """The static inputs of a step body: the tensor fields ``FIELDS`` (a tensor or None), ``source`` and ``single`` (K = 1 indices
    mean one frame, not a chunk of one)."""

    def __init__(self):
        self.source = self.single = self._signature = None
        for k in FIELDS:
            setattr(self, k, None)

    def bind(self, source, single=None, adopted=None, **copied):
        """-> True if a NEW set of tensors was bound (a graph captured on the old one is stale), False if the held set took the values.

        ``copied`` tensors are the caller's: the set holds clones, and a later bind copies into them.  ``adopted`` tensors are held as
        the objects themselves (a producer that writes them in place, such as a ``FrameFeed``): nothing is ever copied into them.  The
        held set serves while ``source``, ``single``, which fields are adopted and every field's shape (None: absent) stay, and the
        adopted tensors are the very objects already held."""
        adopted = {k: v for k, v in (adopted or {}).items() if v is not None}
        copied = {k: v for k, v in copied.items() if v is not None}
        if source not in SOURCES:
            raise ValueError(f"StepInputs.bind: source must be one of {SOURCES}, got {source!r}")
        unknown, twice = (set(adopted) | set(copied)) - set(FIELDS), set(adopted) & set(copied)
        if unknown or twice:
            raise ValueError(f"StepInputs.bind: unknown fields {sorted(unknown)}, fields both copied and adopted {sorted(twice)}")
        given = {**adopted, **copied}
        signature = (source, single) + tuple((k in adopted, tuple(given[k].shape) if k in given else None) for k in FIELDS)
        if signature == self._signature and all(getattr(self, k) is v for k, v in adopted.items()):
            for k, v in copied.items():
                getattr(self, k).copy_(v)
            return False
        for k in FIELDS:
            setattr(self, k, adopted[k] if k in adopted else copied[k].clone() if k in copied else None)
        self.source, self.single, self._signature = source, single, signature
        return True


@contextlib.contextmanager
def preserved(tensors, lists=()):
    """Around runs that must not count: ``tensors`` are cloned and ``lists`` copied on entry and put back (``copy_``, ``lst[:] =``) on a
    normal exit.  When the block raises nothing is put back: the state is what the failed runs left, and the error propagates."""
    tensors, lists = list(tensors), list(lists)
    kept, kept_lists = [t.clone() for t in tensors], [list(l) for l in lists]
    yield
    for t, k in zip(tensors, kept):
        t.copy_(k)
    for l, k in zip(lists, kept_lists):
        l[:] = k
