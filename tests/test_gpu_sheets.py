"""``sings_amd.sheets.image_sheets`` (csrc/sg_sheet.hip) against the numpy restatement of tests/sheet_case.py: the bytes are EQUAL -- both
sides are one fp32 multiply, one fp32 add, a clamp and a truncation per value, so there is no tolerance to choose.

Frame sizes (W, H): (5, 3) has no 4-pixel source path and an odd row pitch; (8, 4) takes the 16-byte loads wherever a thread's four pixels
fall into one tile row at an aligned address; (6, 2) has H W % 4 == 0 but W % 4 != 0 (aligned planes, rows that are not).  T in {1, 2, 5}
at ``nrow=4`` covers ``xmaps < nrow`` and an incomplete last row; the pair form takes T in {2, 6}.  One case of 64 x 48 frames spans many
workgroups.  The inputs carry NaN, +-Inf, -0.0 and the exact multiples of 1/255 and 1/510 at which the two rules part."""
import itertools

import numpy as np
import pytest
import torch

from sheet_case import planted, quantise, sheets
from sings_amd.sheets import image_sheets, sheet_geometry

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(a, b, mask, **kw):
    got = image_sheets(_t(a), _t(b), mask=_t(mask), **kw)
    want = sheets(a, b, mask=mask, **kw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (tuple(got.shape), want.shape, kw)
    same = np.array_equal(got.cpu().numpy(), want)
    if not same:
        bad = np.argwhere(got.cpu().numpy() != want)
        print(f"{len(bad)} bytes differ, first at {bad[0].tolist()}: got {got.cpu().numpy()[tuple(bad[0])]}, want {want[tuple(bad[0])]}; {kw}")
    return same


@pytest.mark.parametrize("W, H", [(5, 3), (8, 4), (6, 2)])
def test_sheets_equal_the_numpy_restatement(W, H):
    n = 0
    for pair, S in itertools.product((False, True), (1, 3)):
        for T in ((2, 6) if pair else (1, 2, 5)):
            F = S * T // (2 if pair else 1)
            a = planted((F, 3, H, W), 100 + T + 10 * S)
            b = planted((F, 3, H, W), 200 + T + 10 * S) if pair else None
            m = np.random.RandomState(T + S).uniform(0, 1, (F, H, W)).astype(np.float32)
            m[:, 0, 0] = 0.0                                     # (0 times Inf or NaN: NaN, a 0 byte)
            for padding, pad_value, quant, bgr, mask in itertools.product((0, 2), (0.0, 1.0, 0.3), ("trunc", "round"), (False, True),
                                                                          (None, m)):
                assert _check(a, b, mask, tiles_per_sheet=T, nrow=4, padding=padding, pad_value=pad_value, quant=quant, bgr=bgr)
                n += 1
    assert n == 2 * 5 * 48


def test_the_two_rules_part_where_they_should():
    """The planted multiples are in the inputs and make the two quantisations differ: the cases above can tell the rules apart."""
    a = planted((2, 3, 4, 8), 5)
    assert np.isnan(a).any() and np.isinf(a).any() and (quantise(a, "trunc") != quantise(a, "round")).any()
    t, r = (image_sheets(_t(a), tiles_per_sheet=1, padding=0, quant=q).cpu().numpy() for q in ("trunc", "round"))
    assert (t != r).any() and np.array_equal(t, sheets(a, tiles_per_sheet=1, padding=0, quant="trunc"))


@pytest.mark.parametrize("quant", ["trunc", "round"])
def test_many_workgroups_and_the_aligned_path(quant):
    """64 x 48 frames: five tiles in three sheets of 102 x 266 pixels (27 workgroups each; padding 2 puts every tile row at an odd
    offset), and one frame per sheet without padding, where every thread takes the 16-byte loads."""
    W, H = 64, 48
    a = planted((15, 3, H, W), 9)
    m = np.random.RandomState(2).uniform(0, 1, (15, H, W)).astype(np.float32)
    assert sheet_geometry(5, H, W, 4, 2)[:2] == (102, 266)
    assert _check(a, None, m, tiles_per_sheet=5, nrow=4, padding=2, pad_value=0.3, quant=quant, bgr=True)
    assert _check(a, None, None, tiles_per_sheet=1, nrow=8, padding=0, pad_value=0.0, quant=quant, bgr=False)
    assert _check(a, None, m, tiles_per_sheet=1, nrow=8, padding=0, pad_value=0.0, quant=quant, bgr=False)
    b = planted((15, 3, H, W), 10)
    assert _check(a, b, None, tiles_per_sheet=2, nrow=2, padding=0, pad_value=0.0, quant=quant, bgr=False)      # the training picture
    assert _check(a, b, m, tiles_per_sheet=6, nrow=4, padding=2, pad_value=0.0, quant=quant, bgr=False)         # a progress sheet


def test_a_source_offset_by_one_float_declines_the_vector_path():
    W, H, F = 8, 4, 3
    a = planted((F, 3, H, W), 31)
    m = np.random.RandomState(3).uniform(0, 1, (F, H, W)).astype(np.float32)
    for shift_a, shift_m in ((1, 0), (0, 1), (1, 1), (2, 3)):
        buf = torch.zeros(a.size + shift_a, dtype=torch.float32, device=DEV)
        mbuf = torch.zeros(m.size + shift_m, dtype=torch.float32, device=DEV)
        buf[shift_a:].copy_(_t(a).reshape(-1)); mbuf[shift_m:].copy_(_t(m).reshape(-1))
        ta, tm = buf[shift_a:].view(F, 3, H, W), mbuf[shift_m:].view(F, H, W)
        assert ta.is_contiguous() and ta.data_ptr() % 16 == (4 * shift_a) % 16
        for quant, mask in itertools.product(("trunc", "round"), (None, tm)):
            got = image_sheets(ta, tiles_per_sheet=1, padding=0, quant=quant, mask=mask)
            want = sheets(a, tiles_per_sheet=1, padding=0, quant=quant, mask=None if mask is None else m)
            assert np.array_equal(got.cpu().numpy(), want), (shift_a, shift_m, quant, mask is not None)


def test_the_pair_form_is_comparison_grid_in_bytes():
    """``T=2, padding=2, pad_value=1, ROUND`` is ``validate.comparison_grid(gt, pred)`` quantised by the same rule: the kernel and the grid
    the project already ships state the same geometry."""
    from sings_amd.run_outputs import validation_grids
    from sings_amd.validate import comparison_grid
    K, H, W = 3, 6, 10
    gt, pred = planted((K, 3, H, W), 41), planted((K, 3, H, W), 42)
    got = validation_grids(_t(gt), _t(pred))
    assert tuple(got.shape) == (K, H + 4, 2 * W + 6, 3)
    for k in range(K):
        grid = comparison_grid(_t(gt[k]), _t(pred[k])).cpu().numpy()
        assert np.array_equal(got[k].cpu().numpy(), quantise(grid, "round").transpose(1, 2, 0)), k
    m = np.random.RandomState(4).uniform(0, 1, (K, H, W)).astype(np.float32)
    masked = validation_grids(_t(gt), _t(pred), mask=_t(m))
    assert np.array_equal(masked.cpu().numpy(), sheets(gt, pred, tiles_per_sheet=2, nrow=2, padding=2, pad_value=1.0, quant="round", mask=m))


@pytest.mark.parametrize("W, H", [(5, 3), (8, 4), (64, 48)])
def test_one_tile_truncated_is_frames_to_u8(W, H):
    from sings_amd.posed import frames_to_u8
    x = _t(planted((4, 3, H, W), 51))
    for bgr in (False, True):
        assert torch.equal(image_sheets(x, tiles_per_sheet=1, padding=0, quant="trunc", bgr=bgr), frames_to_u8(x, bgr=bgr))
    assert torch.equal(image_sheets(x[0], padding=0, quant="trunc")[0], frames_to_u8(x[0]))


def test_the_fronts_refusals():
    x = torch.zeros(4, 3, 4, 8, device=DEV)
    with pytest.raises(ValueError, match="do not fill sheets"):
        image_sheets(x, tiles_per_sheet=3)
    with pytest.raises(ValueError, match="even count"):
        image_sheets(x, x, tiles_per_sheet=1)
    with pytest.raises(ValueError, match="quant must be"):
        image_sheets(x, quant="nearest")
    with pytest.raises(ValueError, match="fp32 \\[F,3,H,W\\]"):
        image_sheets(x.double())
    with pytest.raises(ValueError, match="mask must be"):
        image_sheets(x, mask=torch.zeros(4, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_sheets(x, x.cpu())
