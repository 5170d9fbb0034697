"""The span table of the spans report on the CPU (``K.SpanTable``, the host twins of
csrc/kernels/spans.hip on the layout of span_table.h) against a dict fold: the key whose bits are
the empty marker and key 0, growth in the middle of a sequence of folds, a key whose first line
comes in one fold and whose last comes three folds later, an untimed line as a span's only line,
purge and the fold of a purged key's sibling, the sample filter of the rows, and the arguments.
``lost`` (pairs that found no slot or named no line) is 0 throughout."""
import pytest
import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K
from spans_cases import (I64_MAX, I64_MIN, SIDE, U64, ZERO, PairPiece, check_table, dict_fold, id_key, id_token, in_sample,
                         rows_of, signed, table_rows)

CPU = torch.device("cpu")


def _lost(tab) -> int:
    return tab._used.tolist()[1]


@pytest.mark.parametrize("n,distinct", [(1, 1), (257, 40), (5000, 3000)])
def test_fold_purge_fold(n, distinct):
    assert _lost(check_table(CPU, n, distinct, seed=n)) == 0


def test_level_is_the_hash_sample():
    assert golden.span_level(0) == 64 == golden.span_level(0 & U64)         # fmix64(0) == 0: in every sample
    for k in (1, 12345, K.GT_EMPTY & U64, U64):
        lv = golden.span_level(k)
        h = golden.fmix64(k)
        assert 0 <= lv < 64 and h >> (64 - lv) == 0 and (h >> (63 - lv)) & 1 == 1      # lv zero bits, then a one
    assert golden.spans_shift([0, 1, 1, 5], 4) == 0 and golden.spans_shift([0, 1, 1, 5], 3) == 1
    assert golden.spans_shift([0, 1, 1, 5], 1) == 2 and golden.spans_shift([], 16) == 0


def test_side_slot_and_key_zero():
    ids = [SIDE, 3, ZERO, SIDE, 4, ZERO, SIDE]
    tab = K.SpanTable(CPU, cap=2)
    a = PairPiece(ids, 1, 0, CPU)
    tab.fold(*a.args())
    ref = dict_fold(a)
    assert table_rows(tab) == rows_of(ref) and tab.used == 4 and _lost(tab) == 0
    side = ref[K.GT_EMPTY]
    assert side[:3] == [3, 0, 6] and side[8] == id_token(SIDE).lower() and side[5] == a.sig[0] and side[6] == a.sig[6]
    assert ref[0][:3] == [2, 2, 5]
    # alone, first into an empty table
    tab = K.SpanTable(CPU)
    b = PairPiece([SIDE], 2, 7, CPU)
    tab.fold(*b.args())
    assert table_rows(tab) == rows_of(dict_fold(b)) and tab.used == 1
    # key 0 is in every sample, the marker is in the samples its hash says
    tab.fold(*PairPiece([ZERO], 3, 8, CPU).args())
    tab.purge(64)
    assert [r[0] for r in table_rows(tab)] == [0]


def test_growth_in_the_middle_of_folds():
    tab = K.SpanTable(CPU, cap=2)
    ref, base = {}, 0
    for k in range(6):                                          # 40, 80, ... pairs a time: cap 2 -> 8192
        n = 40 << k
        ids = [(7 * i + k) % (30 << k) for i in range(n)]       # ids of the earlier folds come again
        piece = PairPiece(ids, k, base, CPU)
        tab.fold(*piece.args())
        dict_fold(piece, into=ref)
        base += n
        assert table_rows(tab) == rows_of(ref) and 2 * tab.used <= tab.cap and _lost(tab) == 0
    assert tab.cap >= 2048 and tab.used == len(ref) > 900


def test_last_line_three_folds_after_the_first():
    """The two-fold ``closes`` test: a later piece raises ``last`` and rewrites ``closes``; it
    never touches ``opens`` or the token."""
    tab = K.SpanTable(CPU)
    ref, pieces = {}, []
    for part, ids in enumerate(([5, 6, 5], [6, 7], [7, 8], [8, 5])):
        pieces.append(PairPiece(ids, 10 + part, 10 * part, CPU))
        tab.fold(*pieces[-1].args())
        dict_fold(pieces[-1], into=ref)
        assert table_rows(tab) == rows_of(ref), part
    five = ref[id_key(5)]
    assert five[:3] == [3, 0, 31] and five[5] == pieces[0].sig[0] and five[6] == pieces[3].sig[1] != pieces[0].sig[2]
    assert five[8] == id_token(5).lower() and _lost(tab) == 0


def test_untimed_line_as_the_only_line():
    tab = K.SpanTable(CPU)
    piece = PairPiece([1, 2, 2], 4, 100, CPU, timed=False)
    tab.fold(*piece.args())
    rows = table_rows(tab)
    assert rows == rows_of(dict_fold(piece)) and all(r[4] == I64_MAX and r[5] == I64_MIN for r in rows)
    # a timed line of the same id in a later fold gives it a time
    later = PairPiece([1], 5, 200, CPU)
    later.eff = [777]
    tab.fold(*later.args())
    one = [r for r in table_rows(tab) if r[0] == id_key(1)][0]
    assert one[1:6] == (2, 100, 200, 777, 777)


def test_purge_then_fold_of_a_sibling():
    ids = list(range(400))
    tab = K.SpanTable(CPU)
    piece = PairPiece(ids, 6, 0, CPU)
    tab.fold(*piece.args())
    ref = dict_fold(piece)
    for shift in (1, 2, 4):
        before = tab.used
        dropped = tab.purge(shift)
        ref = {k: e for k, e in ref.items() if in_sample(k, shift)}
        assert dropped == before - len(ref) > 0 and table_rows(tab) == rows_of(ref) and tab.used == len(ref)
    assert 5 < len(ref) < 60
    gone = next(no for no in ids if not in_sample(id_key(no), 4))
    kept = next(no for no in ids if in_sample(id_key(no), 4))
    # the sibling of a purged key -- a new id that lands in the sample -- and a kept one, in a later fold
    sibling = next(no for no in range(1000, 3000) if in_sample(id_key(no), 4))
    later = PairPiece([sibling, kept, sibling], 7, 400, CPU)
    tab.fold(*later.args())
    dict_fold(later, into=ref)
    assert table_rows(tab) == rows_of(ref) and id_key(gone) not in ref and tab.purge(4) == 0 and _lost(tab) == 0


def test_arguments():
    with pytest.raises(ValueError):
        K.SpanTable(CPU, cap=48)
    tab = K.SpanTable(CPU)
    piece = PairPiece([1, 2], 8, 0, CPU)
    line, key, tok, sig, eff, text, ls, base = piece.args()
    for bad in ((line[:1], key, tok, sig, eff, text, ls, base), (line, key, tok, sig[:1], eff, text, ls, base),
                (line.long(), key, tok, sig, eff, text, ls, base), (line, key, tok, sig, eff, text, ls, -1),
                (line, key, tok, sig, eff, text, ls.int(), base)):
        with pytest.raises(ValueError):
            tab.fold(*bad)
    with pytest.raises(ValueError):
        tab.purge(65)
    assert tab.used == 0 and tab.purge(3) == 0
    none = PairPiece([], 9, 0, CPU)
    tab.fold(*none.args())
    rows = tab.rows()
    assert len(rows) == 10 and all(c.shape[0] == 0 for c in rows) and rows[9].shape == (0, K.SPAN_TOK_BYTES)
    # a pair that names no line of the piece is counted as lost, and the next read says so
    tab.fold(torch.tensor([2], dtype=torch.int32), key[:1], tok[:1], sig, eff, text, ls, base)
    with pytest.raises(RuntimeError, match="found no slot"):
        tab.used
    assert signed(U64) == -1
