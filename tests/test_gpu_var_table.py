"""GPU: the value table of the variants report (csrc/kernels/variants.hip k_var_fold / k_var_rows /
k_var_reinsert / k_var_winners on the layout of var_table.h): GPU table rows == CPU table rows ==
dict fold, at sizes around the block and the tile, with distinct keys per tile on both sides of the
1,024 LDS slots and the probe limit, one hot key, the side-slot key, skip sets that hit the LDS path
and the direct path, purge then fold, winners after a purge, and growth. The scenarios are
variants_cases.check_fold's: the CPU tests run the same ones."""
import pytest
import torch

from log_parser_amd.ops import kernels as K
from variants_cases import (check_fold, cols, dict_fold, make_triples, rows_of, side_pair, skip_set, table_rows,
                            want_winners)

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")


def _both(gpu_device, triples, **kw):
    """The scenario on the GPU and on the CPU (each against the dict fold): the same rows."""
    gpu, cpu = check_fold(gpu_device, triples, **kw), check_fold(CPU, triples, **kw)
    assert table_rows(gpu) == table_rows(cpu) and all(c.is_cuda for c in gpu.rows())
    return gpu


@pytest.mark.parametrize("tile", [256, 2048])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049, 5000])
def test_sizes(gpu_device, n, tile):
    _both(gpu_device, make_triples(n, max(1, n // 7), seed=n), tile=tile)
    _both(gpu_device, make_triples(n, n, seed=n + 1), tile=tile)                 # every triple a key of its own


@pytest.mark.parametrize("distinct", [1, 1023, 1024, 1025, 3000])
def test_distinct_keys_per_tile(gpu_device, distinct):
    """One tile of 2,048 triples holds ``distinct`` keys (its first ``distinct`` triples name each
    once): below, at and above the 1,024 LDS slots -- with the probe limit, some go to the global
    table directly well before that."""
    triples = make_triples(2048, min(distinct, 2048), seed=distinct)
    _both(gpu_device, triples, tile=2048)
    _both(gpu_device, make_triples(5000, distinct, seed=distinct + 7), tile=2048)
    _both(gpu_device, make_triples(5000, distinct, seed=distinct + 7), tile=0)   # the tile the launch picks


def test_hot_key_and_side_slot(gpu_device):
    hot = make_triples(5000, 40, seed=1, hot=True)
    assert max(e[2] for e in dict_fold(hot).values()) > 4000                      # one key holds nine triples in ten
    _both(gpu_device, hot, tile=2048)
    _both(gpu_device, hot, tile=256)
    side = side_pair(0x1234567)
    triples = make_triples(3000, 500, seed=3) + [side + (o,) for o in (700, 5, 90)] * 40
    for tile in (256, 2048):
        _both(gpu_device, triples, tile=tile, cap=2)
    tab = K.VarTable(gpu_device)                                                  # alone, first into an empty table
    tab.fold(*cols([side + (9,), side + (4,)], gpu_device))
    assert table_rows(tab) == [side + (2, 4, 9)] and tab.used == 1
    assert tab.winners(*cols([side + (9,), side + (4,)], gpu_device)).tolist() == [1]


def test_skip_on_both_paths(gpu_device):
    """Every other field is skipped. 300 keys in a tile of 2,048 stay in the LDS table (the skip is
    probed at flush time); 2,048 keys in the tile overflow it, and the side-slot key never enters
    it (the skip is probed per triple on the direct path)."""
    for n, distinct in ((2048, 300), (2048, 2048), (5000, 3000)):
        triples = make_triples(n, distinct, seed=n + distinct)
        fields = sorted({f for f, _, _ in triples})
        tab = _both(gpu_device, triples, tile=2048, skip_fields=fields[1::2])
        assert not {r[0] for r in table_rows(tab)} & set(fields[1::2]) and tab.used > 0
    side = side_pair(99)
    triples = make_triples(600, 100, seed=2) + [side + (o,) for o in range(30)]
    tab = K.VarTable(gpu_device, tile=256)
    tab.fold(*cols(triples, gpu_device), skip=skip_set([side[0]], gpu_device))
    assert table_rows(tab) == rows_of(dict_fold(triples, {side[0]})) and side[0] not in {r[0] for r in table_rows(tab)}
    tab = K.VarTable(gpu_device, tile=2048)                                       # everything skipped: an empty table
    every = make_triples(5000, 3000, seed=9)
    tab.fold(*cols(every, gpu_device), skip=skip_set({f for f, _, _ in every}, gpu_device))
    assert tab.used == 0 and table_rows(tab) == [] and tab.winners(*cols(every, gpu_device)).numel() == 0


def test_growth(gpu_device):
    tab, ref = K.VarTable(gpu_device, cap=2), {}
    for k in range(6):                                          # 40, 80, ... triples a time: cap 2 -> 8192
        part = make_triples(40 << k, 30 << k, seed=k, base=1000 * k)
        f, v, o = cols(part, gpu_device)
        tab.fold(f, v, o)
        dict_fold(part, into=ref)
        assert table_rows(tab) == rows_of(ref) and 2 * tab.used <= tab.cap
        assert sorted(tab.winners(f, v, o).tolist()) == want_winners(ref, part)
    assert tab.cap >= 4096 and tab.used == len(ref) > 1500


def test_first_and_last(gpu_device):
    triples = [(1, 2, o) for o in (50, 7, 93, 7, 60)] + [(1, 3, 8)]
    tab = K.VarTable(gpu_device)
    tab.fold(*cols(triples, gpu_device))
    assert table_rows(tab) == [(1, 2, 5, 7, 93), (1, 3, 1, 8, 8)]
    tab.fold(*cols([(1, 2, 3), (1, 2, 99)], gpu_device))
    assert table_rows(tab)[0] == (1, 2, 7, 3, 99)
