"""``sings_amd.step_inputs`` on CPU tensors: when ``StepInputs.bind`` keeps the held set of static inputs (a captured graph reads their
addresses) and when it binds a new one, what it adopts and never writes, and what ``preserved`` puts back around runs that must not
count.  Host logic only: the trainer's GPU tests run the same code under a captured step."""
import pytest
import torch

from sings_amd.step_inputs import FIELDS, StepInputs, preserved


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _base(seed=0, **over):
    """The arguments of a ``step(A, gt, mask)`` call; ``over`` replaces or adds fields."""
    kw = dict(A=_rand(24, 4, 4, seed=seed), gt=_rand(3, 8, 8, seed=seed + 1), mask=_rand(8, 8, seed=seed + 2))
    kw.update(over)
    return kw


def _bound(**over):
    inp = StepInputs()
    assert inp.bind("A", **_base(**over)) is True
    return inp


def test_the_first_bind_clones():
    inp, kw = StepInputs(), _base()
    assert inp.bind("A", **kw) is True
    assert inp.source == "A" and inp.single is None
    for k, v in kw.items():
        held = getattr(inp, k)
        assert held.data_ptr() != v.data_ptr() and torch.equal(held, v), k
    assert inp.idx is None and inp.lp_origins is None and inp.lp_bg is None


def test_a_second_bind_of_the_same_shapes_copies_into_the_held_tensors():
    inp = _bound()
    ptrs = {k: getattr(inp, k).data_ptr() for k in ("A", "gt", "mask")}
    kw = _base(seed=10)
    assert inp.bind("A", **kw) is False
    for k, v in kw.items():
        assert getattr(inp, k).data_ptr() == ptrs[k] and torch.equal(getattr(inp, k), v), k


@pytest.mark.parametrize("change", ["A_chunk", "single", "lp_origins_appears", "lp_origins_goes", "lp_bg_shape", "mask_shape",
                                    "gt_shape"])
def test_each_change_of_the_signature_alone_binds_a_new_set(change):
    origins, bg = torch.zeros(4, 2, dtype=torch.int32), _rand(3, 8, 8, seed=5)
    first, single = _base(lp_bg=bg), None
    second = dict(first)
    if change == "A_chunk":
        second["A"] = _rand(2, 24, 4, 4)
    elif change == "single":
        first = dict(idx=torch.zeros(1, dtype=torch.int32), gt=first["gt"], mask=first["mask"], lp_bg=bg)
        second, single = dict(first), True
    elif change == "lp_origins_appears":
        second["lp_origins"] = origins
    elif change == "lp_origins_goes":
        first["lp_origins"] = origins
    elif change == "lp_bg_shape":
        second["lp_bg"] = _rand(2, 3, 8, 8)
    elif change == "mask_shape":
        second["mask"] = _rand(2, 8, 8)
    else:
        second["gt"] = _rand(2, 3, 8, 8)
    source = "idx" if "idx" in first else "A"
    inp = StepInputs()
    assert inp.bind(source, single, **first) is True
    assert inp.bind(source, single, **first) is False
    held = {k: getattr(inp, k) for k in FIELDS}
    assert inp.bind(source, None if single is None else not single, **second) is True
    for k in FIELDS:                                             # a new set: every field a new tensor (or None), none written in place
        want = second.get(k)
        assert (getattr(inp, k) is None) == (want is None), k
        assert want is None or (getattr(inp, k) is not held[k] and torch.equal(getattr(inp, k), want)), k
    assert inp.bind(source, None if single is None else not single, **second) is False


def test_the_source_is_part_of_the_signature():
    inp = _bound()
    rest = {k: v for k, v in _base().items() if k != "A"}
    idx = torch.tensor([3], dtype=torch.int32)
    assert inp.bind("idx", True, idx=idx, **rest) is True
    assert inp.A is None and inp.source == "idx" and inp.single is True and torch.equal(inp.idx, idx)
    assert inp.bind("idx", True, idx=idx + 1, **rest) is False and int(inp.idx[0]) == 4
    assert inp.bind("A", **_base()) is True
    assert inp.idx is None and inp.source == "A" and inp.single is None


def test_adoption():
    idx, gt, mask = torch.tensor([1, 2], dtype=torch.int32), _rand(2, 3, 8, 8), _rand(2, 8, 8)
    bg = _rand(3, 8, 8, seed=3)
    inp = StepInputs()
    assert inp.bind("feed", False, adopted=dict(idx=idx, gt=gt, mask=mask), lp_bg=bg) is True
    assert inp.idx is idx and inp.gt is gt and inp.mask is mask and inp.A is None and inp.lp_origins is None
    assert inp.lp_bg.data_ptr() != bg.data_ptr() and torch.equal(inp.lp_bg, bg)
    held_bg, kept = inp.lp_bg, [t.clone() for t in (idx, gt, mask)]
    bg2 = _rand(3, 8, 8, seed=4)
    assert inp.bind("feed", False, adopted=dict(idx=idx, gt=gt, mask=mask), lp_bg=bg2) is False      # the same objects: only lp_bg moves
    assert inp.lp_bg is held_bg and torch.equal(held_bg, bg2) and inp.gt is gt
    assert all(torch.equal(a, b) for a, b in zip(kept, (idx, gt, mask)))
    other = dict(idx=idx.clone(), gt=gt.clone(), mask=mask.clone())                                   # other objects, the same shapes
    assert inp.bind("feed", False, adopted=other, lp_bg=bg2) is True and inp.gt is other["gt"]
    assert inp.bind("feed", False, adopted=dict(idx=idx, gt=gt, mask=mask), lp_bg=bg2) is True
    # a step_frames call beside the feed: tensors of its own, the feed's are never written
    assert inp.bind("idx", False, idx=idx + 5, gt=gt + 1, mask=mask + 1) is True
    assert inp.bind("idx", False, idx=idx + 6, gt=gt + 2, mask=mask + 2) is False
    assert inp.gt is not gt and torch.equal(inp.gt, gt + 2) and inp.lp_bg is None
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(kept, (idx, gt, mask)))


def test_refusals():
    inp = StepInputs()
    with pytest.raises(ValueError, match="unknown fields"):
        inp.bind("A", **_base(depth=torch.zeros(8, 8)))
    with pytest.raises(ValueError, match="unknown fields"):
        inp.bind("A", adopted=dict(depth=torch.zeros(8, 8)), **_base())
    with pytest.raises(ValueError, match="both copied and adopted"):
        inp.bind("A", adopted=dict(gt=torch.zeros(3, 8, 8)), **_base())
    with pytest.raises(ValueError, match="source must be one of"):
        inp.bind("frames", **_base())
    assert inp.source is None and all(getattr(inp, k) is None for k in FIELDS)      # (a refused bind holds nothing)


def test_preserved_puts_tensors_and_lists_back():
    a, b, steps = _rand(5, 3), torch.arange(4), [3, 3, 0]
    kept = (a.clone(), b.clone(), list(steps))
    ptrs = (a.data_ptr(), b.data_ptr())
    with preserved([a, b], lists=[steps]):
        a.add_(1.0); b.mul_(2); steps[0] += 2; steps.append(9)
        assert not torch.equal(a, kept[0]) and steps == [5, 3, 0, 9]
    assert torch.equal(a.view(torch.int32), kept[0].view(torch.int32)) and torch.equal(b, kept[1]) and steps == kept[2]
    assert (a.data_ptr(), b.data_ptr()) == ptrs                  # (in place: a captured graph reads these addresses)
    with preserved(iter([a])):                                   # (any iterable; lists= defaults to none)
        a.zero_()
    assert torch.equal(a, kept[0])


def test_preserved_restores_nothing_when_the_block_raises():
    a, steps = _rand(5, 3), [1, 2]
    changed = a + 1.0
    with pytest.raises(RuntimeError, match="the capture failed"):
        with preserved([a], lists=[steps]):
            a.add_(1.0); steps[0] = 7
            raise RuntimeError("the capture failed")
    assert torch.equal(a, changed) and steps == [7, 2]
