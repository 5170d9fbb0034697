"""GPU: the span table (csrc/kernels/spans.hip k_span_fold / k_span_ends / k_span_rows /
k_span_reinsert on the layout of span_table.h) against the same table on the CPU and against the
dict fold of spans_cases.py: 1, 255, 256, 257 and 5,000 pairs, every pair on one key (one slot,
5,000 atomics on it), every key distinct, the side-slot key, growth, purge, and a key whose first
line comes in one fold and whose last in a later one. Token bytes and lengths are compared."""
import pytest
import torch

from log_parser_amd.ops import kernels as K
from spans_cases import SIDE, ZERO, PairPiece, check_table, dict_fold, id_key, id_token, in_sample, rows_of, table_rows

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def _both(gpu_device, folds, cap: int = 1 << 12):
    """The same folds into a table on the GPU and into one on the CPU: rows equal after every
    fold, to each other and to the dict fold. ``folds``: [(ids, seed, line_base)]."""
    gpu, cpu, ref = K.SpanTable(gpu_device, cap=cap), K.SpanTable(CPU, cap=cap), {}
    for ids, seed, base in folds:
        gpu.fold(*PairPiece(ids, seed, base, gpu_device).args())
        piece = PairPiece(ids, seed, base, CPU)
        cpu.fold(*piece.args())
        dict_fold(piece, into=ref)
        assert table_rows(gpu) == table_rows(cpu) == rows_of(ref)
        assert gpu.used == cpu.used == len(ref) and gpu._used.tolist()[1] == 0 and gpu.cap == cpu.cap
    return gpu, cpu, ref


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_sizes(gpu_device, n):
    tab = check_table(gpu_device, n, max(1, n // 3), seed=n)
    assert tab._key.is_cuda and tab._used.tolist()[1] == 0


def test_every_pair_on_one_key(gpu_device):
    gpu, _, ref = _both(gpu_device, [([7] * 5000, 1, 0), ([7] * 5000, 2, 5000)])
    assert gpu.used == 1 and ref[id_key(7)][:3] == [10000, 0, 9999] and ref[id_key(7)][8] == id_token(7).lower()


def test_every_key_distinct(gpu_device):
    gpu, _, ref = _both(gpu_device, [(list(range(5000)), 3, 0)], cap=2)
    assert gpu.used == 5000 and gpu.cap >= 16384 and all(e[0] == 1 and e[1] == e[2] for e in ref.values())


def test_side_slot_and_key_zero(gpu_device):
    ids = [SIDE, 3, ZERO, SIDE, 4, ZERO, SIDE] * 40
    gpu, _, ref = _both(gpu_device, [(ids, 4, 0), ([SIDE], 5, 500)], cap=2)
    assert ref[K.GT_EMPTY][:3] == [121, 0, 500] and ref[0][0] == 80 and gpu.used == 4
    assert gpu.purge(64) == 3 and [r[0] for r in table_rows(gpu)] == [0]


def test_growth_and_purge(gpu_device):
    folds = [([(7 * i + k) % (30 << k) for i in range(40 << k)], k, 1000 * (1 << k)) for k in range(6)]
    gpu, cpu, ref = _both(gpu_device, folds, cap=2)
    assert gpu.cap >= 2048 and gpu.used > 900
    for shift in (1, 3):
        ref = {k: e for k, e in ref.items() if in_sample(k, shift)}
        assert gpu.purge(shift) == cpu.purge(shift) > 0 and table_rows(gpu) == table_rows(cpu) == rows_of(ref)
    kept = [no for no in range(960) if in_sample(id_key(no), 3)]
    later = PairPiece(kept, 9, 10 ** 6, gpu_device)
    gpu.fold(*later.args())
    dict_fold(PairPiece(kept, 9, 10 ** 6, CPU), into=ref)
    assert table_rows(gpu) == rows_of(ref) and gpu.purge(3) == 0


def test_last_line_in_a_later_fold(gpu_device):
    """The two-fold ``closes`` test on the GPU: the later fold rewrites ``closes`` and leaves
    ``opens`` and the token alone."""
    folds = [([5, 6, 5], 10, 0), ([6, 7], 11, 10), ([7, 8], 12, 20), ([8, 5], 13, 30)]
    gpu, _, ref = _both(gpu_device, folds)
    first, last = PairPiece(*folds[0], CPU), PairPiece(*folds[3], CPU)
    five = ref[id_key(5)]
    assert five[:3] == [3, 0, 31] and five[5] == first.sig[0] and five[6] == last.sig[1] and five[8] == id_token(5).lower()
    row = [r for r in table_rows(gpu) if r[0] == id_key(5)][0]
    assert row[6] == first.sig[0] and row[7] == last.sig[1] and row[9] == id_token(5).lower()
