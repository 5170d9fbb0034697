"""The value table of the variants report on the CPU (``K.VarTable``, the host twins of
csrc/kernels/variants.hip on the layout of var_table.h) against a dict fold: growth across several
doublings, the side slot of the key that equals the empty marker, the skip set, purge and the fold
after it, winners after a purge, and the arguments."""
import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K
from variants_cases import (U64, check_fold, cols, dict_fold, make_triples, rows_of, side_pair, signed, skip_set,
                            table_rows, want_winners)

CPU = torch.device("cpu")


def test_cell_key_is_the_table_key():
    assert K.CT_MIX == golden._TREND_MIX and golden.var_cell_key(5, 0) == 5
    assert golden.var_cell_key(1, 2) == (1 + 2 * K.CT_MIX) & U64 != golden.var_cell_key(2, 1)
    f, v = side_pair(12345)
    assert golden.var_cell_key(f & U64, v & U64) == K.GT_EMPTY & U64


@pytest.mark.parametrize("n,distinct", [(1, 1), (257, 40), (5000, 3000)])
def test_fold_purge_winners(n, distinct):
    check_fold(CPU, make_triples(n, distinct, seed=n))


def test_growth_across_doublings():
    tab = K.VarTable(CPU, cap=2)
    ref = {}
    for k in range(6):                                          # 40, 80, ... triples a time: cap 2 -> 8192
        part = make_triples(40 << k, 30 << k, seed=k, base=1000 * k)
        tab.fold(*cols(part, CPU))
        dict_fold(part, into=ref)
        assert table_rows(tab) == rows_of(ref) and 2 * tab.used <= tab.cap
    assert tab.cap >= 4096 and tab.used == len(ref) > 1500


def test_side_slot():
    side = side_pair(0x1234567)
    triples = make_triples(300, 50, seed=3) + [side + (o,) for o in (700, 5, 90)]
    tab = check_fold(CPU, triples, cap=2)
    assert tab.cap >= 512
    # alone, first into an empty table, and as the only key of a skipped field
    tab = K.VarTable(CPU)
    tab.fold(*cols([side + (9,), side + (4,)], CPU))
    assert table_rows(tab) == [side + (2, 4, 9)] and tab.used == 1
    assert tab.winners(*cols([side + (9,), side + (4,)], CPU)).tolist() == [1]
    tab = K.VarTable(CPU)
    tab.fold(*cols([side + (9,), (7, 7, 1)], CPU), skip=skip_set([side[0]], CPU))
    assert table_rows(tab) == [(7, 7, 1, 1, 1)]


def test_skip():
    triples = make_triples(2049, 700, seed=5)
    fields = sorted({f for f, _, _ in triples})
    tab = check_fold(CPU, triples, skip_fields=fields[1::2])
    assert not {r[0] for r in table_rows(tab)} & set(fields[1::2])
    # everything skipped: an empty table
    tab = K.VarTable(CPU)
    tab.fold(*cols(triples, CPU), skip=skip_set(fields, CPU))
    assert tab.used == 0 and table_rows(tab) == [] and tab.winners(*cols(triples, CPU)).numel() == 0


def test_first_and_last_are_min_and_max():
    triples = [(1, 2, o) for o in (50, 7, 93, 7, 60)] + [(1, 3, 8)]
    tab = K.VarTable(CPU)
    tab.fold(*cols(triples, CPU))
    assert table_rows(tab) == [(1, 2, 5, 7, 93), (1, 3, 1, 8, 8)]
    assert sorted(tab.winners(*cols(triples, CPU)).tolist()) == [1, 3, 5] == want_winners(dict_fold(triples), triples)
    tab.fold(*cols([(1, 2, 3), (1, 2, 99)], CPU))               # a later call widens both ends
    assert table_rows(tab)[0] == (1, 2, 7, 3, 99)


def test_arguments():
    with pytest.raises(ValueError):
        K.VarTable(CPU, cap=48)
    for tile in (100, 4096, 300):
        with pytest.raises(ValueError):
            K.VarTable(CPU, tile=tile)
    tab = K.VarTable(CPU, tile=256)
    one, two = torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        tab.fold(one, two, one)
    with pytest.raises(ValueError):
        tab.winners(one, one, two)
    none = torch.empty(0, dtype=torch.int64)
    tab.fold(none, none, none)
    assert tab.used == 0 and tab.winners(none, none, none).numel() == 0 and tab.purge(one) == 0
    assert all(c.numel() == 0 and c.dtype == torch.int64 for c in tab.rows()) and len(tab.rows()) == 5
    assert signed(U64) == -1
