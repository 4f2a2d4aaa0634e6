"""The host side of ``posed.FrameAnimator`` that needs no GPU: the redo sequence and its bound (``overflow.EngineCapacity``) and the
split of a job stream into batches (``posed._batches``)."""
import pytest

from sings_amd import _lib
from sings_amd.overflow import EngineCapacity
from sings_amd.posed import _batches

LONG = _lib.NUM_RENDERED_LONG_LIST


def test_redo_sequence_hint_dropped_then_grown():
    ec = EngineCapacity()
    grown = EngineCapacity.grown(5000)
    assert ec.settle([5000, LONG], 4000) == 4000 and ec.long_rows is False
    assert ec.settle([5000, 4800], 4000) == grown
    assert ec.settle([5000, 4800], grown) is None
    # the same sequence through the redo helper: two renders, the second on the grown capacity
    ec, asked = EngineCapacity(), []
    reports = iter([[5000, 4800], [5000, 4800]])

    def render(cap):
        asked.append(cap)
        return f"image@{cap}", next(reports), cap
    assert ec.redo(ec.settle([5000, LONG], 4000), render) == f"image@{grown}"
    assert asked == [4000, grown] and ec.long_rows is False
    # a render on engines that hold more than was asked for is judged by what it ran with
    assert EngineCapacity().redo(4000, lambda cap: ("image", [5000], 8000)) == "image"


def test_a_hinted_unit_popped_after_the_hint_was_dropped_is_rendered_again():
    """Units in flight were launched with the hint; the first one to report NUM_RENDERED_LONG_LIST drops it, the later ones report
    the same count with the hint already off: they are no frames to hand out either."""
    ec = EngineCapacity()
    assert ec.settle([LONG, LONG], 4000) == 4000 and ec.long_rows is False
    assert ec.settle([LONG], 4000) == 4000


def test_redo_is_bounded_by_two_renders():
    ec, asked = EngineCapacity(), []

    def render(cap):                                                     # counts that always exceed the capacity they are given
        asked.append(cap)
        return None, [cap + 1], cap
    with pytest.raises(RuntimeError, match=r"pair counts \[\d+\] for a capacity of \d+ after two re-renders") as err:
        ec.redo(4000, render)
    g = EngineCapacity.grown(4001)
    assert asked == [4000, g]
    assert str(g + 1) in str(err.value) and f"capacity of {g}" in str(err.value)


def _jobs(kinds):
    """Jobs of ``render_round``'s layout whose (smpl_scale, ext_tfs) slots are set ('b') or None ('a')."""
    return [(f"cam{i}", f"A{i}", None, None if k == "a" else 1.0, None if k == "a" else ("t", "r", "s")) for i, k in enumerate(kinds)]


def test_batches_of_a_job_stream():
    jobs = _jobs("a" * 9)
    got = list(_batches(iter(jobs), 4))
    assert [(i0, len(b)) for i0, b in got] == [(0, 4), (4, 4), (8, 1)]
    assert [j for _, b in got for j in b] == jobs                        # every job once, in order
    got = list(_batches(iter(_jobs("aabbbbba")), 4))
    assert [len(b) for _, b in got] == [2, 4, 1, 1] and [i0 for i0, _ in got] == [0, 2, 6, 7]
    assert list(_batches(iter([]), 4)) == []
    got = list(_batches(iter(_jobs("aab")), 1))
    assert [(i0, len(b)) for i0, b in got] == [(0, 1), (1, 1), (2, 1)]
    # a job with a scale and no placement is a kind of its own
    mixed = [("cam", "A", None, 1.0, None), ("cam", "A", None, 1.0, ("t", "r", "s")), ("cam", "A", None, None, ("t", "r", "s"))]
    assert [i0 for i0, _ in _batches(iter(mixed), 4)] == [0, 1, 2]
