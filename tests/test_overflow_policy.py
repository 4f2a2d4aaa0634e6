"""The decision layer of sings_amd.overflow (pair capacity, overflow modes, learned list-length hints) and the FrameAnimator's own
capacity rules, on plain ints: no GPU."""
import warnings

import pytest
import torch

from sings_amd import _lib, overflow as ov
from sings_amd.overflow import EngineCapacity

SHORT, ROWS = _lib.FLAG_SHORT_LISTS, _lib.FLAG_LONG_ROWS
ARRIVED = 1 << 63


@pytest.fixture(autouse=True)
def _clean_policy():
    ov.set_overflow_check("sync", on_overflow="raise")
    ov.reset_overflow_state()
    yield
    ov.set_overflow_check("sync", on_overflow="raise")
    ov.reset_overflow_state()


def test_plan_capacity_floor():
    assert ov.plan(0, 1000, 64, 64)[0] == 1 << 16                       # 2^16 floor
    T = 120 * 68                                                         # 16x16 tiles of 1920 x 1080
    assert ov.plan(0, 200000, 1920, 1080)[0] == 4 * 200000 + T
    ov._capacity_hint[0] = 5_000_000
    assert ov.plan(0, 200000, 1920, 1080)[0] == 5_000_000
    assert ov.plan(1, 200000, 1920, 1080)[0] == 4 * 200000 + T           # (per device)
    assert ov.plan(0, 7, 16, 16)[2] == (7, 16, 16)


def test_plan_sync_flag_in_each_mode():
    assert ov.plan(0, 1000, 64, 64)[1] is True
    assert ov.plan(0, 1000, 64, 64, capturing=True)[1] is False         # a capture never reads R
    ov.set_overflow_check("deferred")
    assert ov.plan(0, 1000, 64, 64)[1] is False
    ov.set_overflow_check("async")
    cap, sync, sig = ov.plan(0, 1000, 64, 64)
    assert sync is True                                                  # the first signature of the device is read
    ov.done_sync(0, 5000, sig)
    assert ov.plan(0, 1000, 64, 64)[1] is False
    assert ov.plan(0, 1000, 64, 64, capturing=True)[1] is False
    assert ov.plan(0, 1000, 128, 64)[1] is True                          # another image size: read once more
    assert ov.plan(1, 1000, 64, 64)[1] is True                           # another device
    ov.reset_overflow_state(torch.device("cuda", 0))
    assert ov.plan(0, 1000, 64, 64)[1] is True


def test_growth_is_twice_the_count_and_never_shrinks():
    assert ov.grown(0) == 1024 and ov.grown(100000) == 201024
    sig = ov.plan(0, 10, 16, 16)[2]
    ov.done_sync(0, 100000, sig)
    assert ov.capacity_pairs("cuda:0") == 201024
    ov.done_sync(0, 10, sig)
    assert ov.capacity_pairs("cuda:0") == 201024
    assert ov.capacity_pairs("cuda:1") is None
    assert ov.plan(0, 10, 16, 16)[0] == 201024


def test_hints_learned_from_the_count_word():
    key = (0, 1000, 64, 64)
    ov.learn(key, (_lib.COUNT_FLAG_HALF_ROWS | _lib.COUNT_FLAG_HALF_LONG_ROWS) << 32 | 12345)
    assert key not in ov._short_ok and key not in ov._rows_ok            # bit 63 clear: the word never arrived
    ov.learn(key, ARRIVED | (_lib.COUNT_FLAG_HALF_ROWS | _lib.COUNT_FLAG_HALF_LONG_ROWS) << 32 | 12345)
    assert ov._short_ok[key] is True and ov._rows_ok[key] is True
    ov.learn(key, ARRIVED | _lib.COUNT_FLAG_HALF_LONG_ROWS << 32 | 12345)
    assert ov._short_ok[key] is False and ov._rows_ok[key] is True
    ov.learn(key, ARRIVED | 12345)
    assert ov._short_ok[key] is False and ov._rows_ok[key] is False


def test_hint_eligibility_of_the_three_ops():
    key = (0, 1000, 64, 64)
    ov._short_ok[key] = ov._rows_ok[key] = True
    dropin = dict(hints=(SHORT, ROWS), needs_sync=True)
    skinned = dict(hints=(ROWS,), needs_sync=False)                      # (the K-frame op: the same, plus SG_FLAG_THROUGHPUT always)
    assert ov.hint_flags(key, sync=True, debug=False, **dropin) == SHORT | ROWS
    assert ov.hint_flags(key, sync=False, debug=False, **dropin) == 0    # "async" / "deferred" / capture: no hint
    assert ov.hint_flags(key, sync=True, debug=True, **dropin) == 0
    assert ov.hint_flags(key, sync=True, debug=False, **skinned) == ROWS
    assert ov.hint_flags(key, sync=False, debug=False, **skinned) == ROWS     # in every mode and under capture
    assert ov.hint_flags(key, sync=False, debug=True, **skinned) == 0
    ov._short_ok[key] = False
    assert ov.hint_flags(key, sync=True, debug=False, **dropin) == ROWS
    assert ov.hint_flags((0, 1000, 64, 65), sync=True, debug=False, **dropin) == 0     # nothing learned for that shape
    # a violation turns off what the op consulted, and only that
    ov._short_ok[key] = True
    ov.forget(key, skinned["hints"])
    assert ov._short_ok[key] is True and ov._rows_ok[key] is False
    ov.forget(key, dropin["hints"])
    assert ov._short_ok[key] is False and ov._rows_ok[key] is False


def _hints_on_two_devices():
    for d in (0, 1):
        ov._short_ok[(d, 10, 16, 16)] = ov._rows_ok[(d, 10, 16, 16)] = True


def test_absorbed_long_list_drops_only_that_devices_hints():
    _hints_on_two_devices()
    with pytest.raises(RuntimeError, match="longer than the row its learned hint promised"):
        ov.absorb_async(0, [(3000, _lib.HDR_FLAG_LONG_LIST, 100000), (5000, 0, 100000)])
    assert ov.capacity_pairs("cuda:0") == ov.grown(5000)                 # grown before the report
    assert not any(k[0] == 0 for k in ov._short_ok) and not any(k[0] == 0 for k in ov._rows_ok)
    assert ov._short_ok[(1, 10, 16, 16)] and ov._rows_ok[(1, 10, 16, 16)]
    # "warn": the same event as a RuntimeWarning
    _hints_on_two_devices()
    ov.set_overflow_check("async", on_overflow="warn")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert ov.absorb_async(1, [(3000, _lib.HDR_FLAG_LONG_LIST, 100000)]) == 3000
    assert len(rec) == 1 and rec[0].category is RuntimeWarning and "hints of the device are dropped" in str(rec[0].message)
    assert not any(k[0] == 1 for k in ov._rows_ok) and ov._rows_ok[(0, 10, 16, 16)]
    # ... and a caller that asks for "raise" (check_deferred_overflow in "async" mode) still gets the exception
    with pytest.raises(RuntimeError):
        ov.absorb_async(1, [(3000, _lib.HDR_FLAG_LONG_LIST, 100000)], on_overflow="raise")
    # "deferred": always raises
    _hints_on_two_devices()
    with pytest.raises(RuntimeError, match="deferred forward produced up to 7000 .* the hints are dropped"):
        ov.absorb_deferred(0, 7000, _lib.HDR_FLAG_LONG_LIST)
    assert not any(k[0] == 0 for k in ov._rows_ok) and ov._rows_ok[(1, 10, 16, 16)]


def test_absorbed_overflow_grows_and_reports_the_worst_count():
    ov.set_overflow_check("async")
    assert ov.absorb_async(0, []) is None and ov.capacity_pairs("cuda:0") is None
    with pytest.raises(RuntimeError, match="produced 9000 .* capacity of 4000: .* capacity is now 20024"):
        ov.absorb_async(0, [(5000, 1, 4000), (9000, 1, 4000), (9500, 0, 10000)])
    assert ov.capacity_pairs("cuda:0") == ov.grown(9500)
    assert ov.absorb_async(0, [(100, 0, 4000)]) == 100                   # nothing to report
    assert ov.absorb_deferred(0, 0, 0) is None
    assert ov.absorb_deferred(0, 800, 0) == 800
    with pytest.raises(RuntimeError, match="deferred forward produced up to 30000"):
        ov.absorb_deferred(0, 30000, _lib.HDR_FLAG_OVERFLOW)
    assert ov.capacity_pairs("cuda:0") == ov.grown(30000)


def test_k_frame_header_keeps_every_frames_flag_bits():
    K, stride = 3, 64
    binning = torch.zeros(K * stride, dtype=torch.uint8)
    h = binning.view(K, stride)[:, :8].view(torch.int32)
    h[:, 0] = torch.tensor([5000, 9000, 7000], dtype=torch.int32)
    h[:, 1] = torch.tensor([_lib.HDR_FLAG_LONG_LIST, _lib.HDR_FLAG_OVERFLOW, 0], dtype=torch.int32)
    hdr = ov.frames_header(binning, K, stride)
    assert hdr.dtype == torch.int32 and hdr.tolist() == [9000, _lib.HDR_FLAG_OVERFLOW | _lib.HDR_FLAG_LONG_LIST]
    h[:, 1] = 0
    assert ov.frames_header(binning, K, stride).tolist() == [9000, 0]


def test_reset_of_one_device_leaves_the_others():
    for d in (0, 1):
        sig = ov.plan(d, 10, 16, 16)[2]
        ov.done_sync(d, 1000 * (d + 1), sig)
    _hints_on_two_devices()
    ov.reset_overflow_state("cuda:1")
    assert ov.capacity_pairs("cuda:0") == ov.grown(1000) and ov.capacity_pairs("cuda:1") is None
    assert 0 in ov._seen and 1 not in ov._seen
    assert ov._rows_ok == {(0, 10, 16, 16): True} and ov._short_ok == {(0, 10, 16, 16): True}
    ov.reset_overflow_state()
    assert not ov._capacity_hint and not ov._rows_ok


def test_rasterizer_reexports_the_policy():
    from sings_amd import rasterizer as rz
    for name in ("_capacity_hint", "_mode", "_pending", "_rows_ok", "_seen", "_short_ok", "_signal"):
        assert getattr(rz, name) is getattr(ov, name), name              # (the same objects: code written against rasterizer reads them)
    for name in ("set_overflow_check", "set_deferred_overflow_check", "check_deferred_overflow", "reset_overflow_state"):
        assert getattr(rz, name) is getattr(ov, name)
    with pytest.raises(ValueError):
        ov.set_overflow_check("never")
    with pytest.raises(ValueError):
        ov.set_overflow_check("sync", on_overflow="ignore")


def test_frame_animator_capacity_rules():
    floor, grown = EngineCapacity.floor, EngineCapacity.grown
    assert floor(0, 1000, 64, 64) == 1 << 16
    assert floor(0, 100000, 512, 896) == 800000 + 32 * 56
    assert floor(10 ** 7, 100000, 512, 896) == 10 ** 7
    assert grown(400000) == 501024
    fa = EngineCapacity()                                                # (the decisions only: no engines, no streams)
    assert fa.long_rows is True
    assert fa.settle([1000, 3000], 4000) is None
    assert fa.settle([1000, 5000], 4000) == grown(5000) and fa.long_rows
    # a count that hides R: the same capacity, the plain path counts the frame
    assert fa.settle([5000, _lib.NUM_RENDERED_LONG_LIST], 4000) == 4000 and fa.long_rows is False
    assert fa.settle([1000, 3000], 4000) is None
    # an unread header: its R is the frame's, so a long list and an overflow are settled at once
    fa.long_rows = True
    assert fa.settle([3000], 4000, _lib.HDR_FLAG_LONG_LIST) == 4000 and fa.long_rows is False
    fa.long_rows = True
    assert fa.settle([5000], 4000, _lib.HDR_FLAG_LONG_LIST | _lib.HDR_FLAG_OVERFLOW) == grown(5000) and fa.long_rows is False
    assert fa.settle([5000], 4000, _lib.HDR_FLAG_OVERFLOW) == grown(5000)
