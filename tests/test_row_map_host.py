"""``sings_amd.optim.take_rows`` -- the row map of every change of the set of Gaussians -- against the three expressions it replaces in
the trainer (clone + prune, rows appended, a plain ``t[keep]``), compared as int32 bit patterns.  Host tensors only."""
import pytest
import torch

from sings_amd.optim import take_rows

N = 37


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(_bits(a), _bits(b))


def _table(cols):
    """[37, cols] fp32 whose rows include -0.0, NaNs with a payload, +-inf and a denormal."""
    t = torch.randn((N, cols), generator=torch.Generator().manual_seed(11 + cols))
    t[1], t[5], t[6], t[20], t[36] = -0.0, float("inf"), float("-inf"), 1e-42, -0.0
    bits = t.view(torch.int32)                                   # (shares t's memory)
    bits[9] = 0x7FC12345                                         # a quiet NaN with a payload: its bits must survive
    bits[30, 0] = 0x7FC12345 - 2 ** 31                           # the same with the sign bit set
    assert bool(torch.isnan(t[9]).all()) and bool(torch.isnan(t[30, 0])) and 0.0 < float(t[20, 0]) < 1.2e-38
    assert int(bits[1, 0]) == -2 ** 31
    return t


TABLES = {cols: _table(cols) for cols in (3, 1)}


def _src(n, n_new_rows, keep=None):
    src = torch.cat([torch.arange(n), torch.full((n_new_rows,), -1, dtype=torch.int64)])
    return src if keep is None else src[keep]


def _masks(seed, p_clone=0.3, p_keep=0.8):
    gen = torch.Generator().manual_seed(seed)
    clone = torch.rand(N, generator=gen) < p_clone
    keep = torch.rand(N + int(clone.sum()), generator=gen) < p_keep
    return clone, keep


@pytest.mark.parametrize("cols", (3, 1))
def test_clone_and_prune(cols):
    t = TABLES[cols]
    none, every = torch.zeros(N, dtype=torch.bool), torch.ones(N, dtype=torch.bool)
    one_left = torch.zeros(N + 4, dtype=torch.bool)
    one_left[9] = True
    four = torch.zeros(N, dtype=torch.bool)
    four[[1, 9, 20, 36]] = True
    cases = [_masks(1), _masks(2, 0.6, 0.5),
             (none, _masks(3)[1][:N]),                           # no clones
             (_masks(4)[0], torch.ones(N + int(_masks(4)[0].sum()), dtype=torch.bool)),          # nothing pruned
             (none, every),                                      # neither
             (four, one_left)]                                   # everything pruned but one row
    for clone, keep in cases:
        want = torch.cat([t, torch.zeros_like(t[clone])])[keep]
        got = take_rows(t, _src(N, int(clone.sum()), keep))
        assert _same_bits(got, want) and got.is_contiguous()
    assert take_rows(t, _src(N, 4, one_left)).shape[0] == 1


@pytest.mark.parametrize("cols", (3, 1))
@pytest.mark.parametrize("k", (0, 5))
def test_rows_appended(cols, k):
    t = TABLES[cols]
    want = torch.cat([t, torch.zeros((k, cols), dtype=t.dtype)])
    assert _same_bits(take_rows(t, _src(N, k)), want)


@pytest.mark.parametrize("cols", (3, 1))
def test_plain_keep(cols):
    t = TABLES[cols]
    one = torch.zeros(N, dtype=torch.bool)
    one[30] = True
    for keep in (_masks(5)[1][:N], torch.ones(N, dtype=torch.bool), one):
        assert _same_bits(take_rows(t, torch.arange(N)[keep]), t[keep])


@pytest.mark.parametrize("cols", (3, 1))
def test_only_new_rows_are_positive_zeros(cols):
    got = take_rows(TABLES[cols], torch.full((6,), -1, dtype=torch.int64))
    assert tuple(got.shape) == (6, cols) and not _bits(got).any()           # (the sign bit is clear)
    assert tuple(take_rows(TABLES[cols], torch.zeros(0, dtype=torch.int64)).shape) == (0, cols)


@pytest.mark.parametrize("bad", (N, -2))
def test_an_index_outside_the_table_is_refused(bad):
    src = torch.arange(N)
    src[3] = bad
    with pytest.raises(ValueError):
        take_rows(TABLES[3], src)


def test_the_result_never_aliases_the_table():
    for cols, t in TABLES.items():
        before = t.clone()
        for src in (torch.arange(N), torch.arange(N)[:1], _src(N, 2)):
            got = take_rows(t, src)
            assert got.untyped_storage().data_ptr() != t.untyped_storage().data_ptr()
            got.fill_(7.0)
            assert _same_bits(t, before)
