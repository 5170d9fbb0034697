"""Cases for the trends tests (test_trends.py, test_gpu_trends.py): folds for the cell table with the
cells a ``collections.Counter`` gives, and the 4000-line log with its parameter sets."""
import random
from collections import Counter

import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K
from values_cases import HAND, random_lines

W = 10_000
NONE = K.TS_NONE
GT_EMPTY = K.GT_EMPTY


def signed(s: int) -> int:
    return s - (1 << 64) if s >> 63 else s


def _random_fold(n: int, seed: int, n_sigs: int = 7, line_base: int = 0):
    rng = random.Random(seed)
    sigs = [signed(rng.getrandbits(64)) for _ in range(n_sigs)]
    t = 1_758_283_200_000
    sig, eff = [], []
    for _ in range(n):
        t += rng.choice((0, 0, 1, 50, 400, 9_000))
        sig.append(rng.choice(sigs))
        eff.append(NONE if rng.random() < 0.05 else t)
    return sig, eff, line_base


def cell_cases():
    """name -> [(sig, eff, line_base), ...]: the folds of one table, in order."""
    cases = {"n=%d" % n: [_random_fold(n, n)] for n in (1, 255, 256, 257, 2049)}
    cases["one hot cell"] = [([42] * 2049, [5 * W + 3] * 2049, 0)]
    # more distinct cells than the block's LDS table has slots: a 2048 tile overflows into the global table
    cases["3000 distinct cells"] = [([signed(golden.fnv1a64(b"%d" % i)) for i in range(3000)], [7 * W] * 3000, 0)]
    cases["3000 cells of one template"] = [([-5] * 3000, [i * W for i in range(3000)], 0)]
    edge = [k * W + d for k in (-3, -1, 0, 1, 2) for d in (-1, 0, 1, W - 1)] + [NONE, -1, -W, -W - 1, NONE]
    cases["bucket edges"] = [([9] * len(edge), edge, 0), ([9, 11] * len(edge), edge + edge, 100)]
    # the signature that equals the empty marker, and the one whose key in bucket 12 (and in the undated
    # bucket) equals it: the side slot
    side = [signed(golden.trend_cell_sig(1 << 63, b)) for b in (12, golden.TREND_UNDATED)]
    assert all(golden.trend_cell_key(s & golden._U64, b) == 1 << 63 for s, b in zip(side, (12, golden.TREND_UNDATED)))
    cases["empty marker as a signature"] = [([GT_EMPTY, 3, GT_EMPTY, GT_EMPTY], [12 * W, 12 * W, NONE, 13 * W + 1], 0)]
    cases["empty marker as a key"] = [([side[0], side[0], 4, side[0]], [12 * W, 12 * W + 5, 12 * W, 11 * W], 5),
                                      ([side[0]] * 300, [12 * W + i for i in range(300)], 1)]
    cases["empty marker as the undated key"] = [([side[1], side[1], side[1]], [NONE, NONE, 3 * W], 0)]
    cases["two folds, the later lines first"] = [_random_fold(700, 1, line_base=5000), _random_fold(700, 1, line_base=10)]
    return cases


def cells_of(folds):
    """{(sig, bucket): (lines, smallest line)} of the folds, as the specification counts them."""
    count, first = Counter(), {}
    for sig, eff, base in folds:
        for i, (s, t) in enumerate(zip(sig, eff)):
            cell = (s, golden.TREND_UNDATED if t == NONE else t // W)
            count[cell] += 1
            first[cell] = min(first.get(cell, base + i), base + i)
    return {c: (count[c], first[c]) for c in count}


def fold_all(table, folds, device):
    for sig, eff, base in folds:
        table.fold(torch.tensor(sig, dtype=torch.int64, device=device), torch.tensor(eff, dtype=torch.int64, device=device),
                   base, W)
        assert table._used.tolist()[1] == 0


def rows_of(table):
    sig, bucket, count, first = (c.cpu().tolist() for c in table.rows())
    assert len(set(zip(sig, bucket))) == len(sig)
    return {(s, b): (c, f) for s, b, c, f in zip(sig, bucket, count, first)}


def check_cells(device, tile: int, folds, cap: int = 1 << 12):
    table = K.CellTable(device, cap=cap, tile=tile)
    fold_all(table, folds, device)
    want = cells_of(folds)
    assert rows_of(table) == want and table.used == len(want)
    return table


def growth_folds():
    """Folds of growing size into a table that starts at cap=2."""
    return [_random_fold(n, 100 + n, n_sigs=40, line_base=b) for n, b in ((1, 0), (3, 1), (40, 4), (600, 44), (5000, 644))]


def late_errors(text: str, calm_lines: int = 1000) -> str:
    """``text`` without error lines among its first ``calm_lines`` lines (their level becomes WARN):
    the timeline's first error line then lies behind the first bucket, where a pivot may be."""
    lines = text.split("\n")
    return "\n".join([l.replace(" ERROR [", " WARN  [") for l in lines[:calm_lines]] + lines[calm_lines:])


def stamp_lines(L: int, seed: int):
    """``L`` lines: random ones and, from 63 lines on, the hand-written lines of values_cases (stamps that
    are valid, invalid, past byte 31, zoned and fractioned; lines cut at 1024) at fixed places."""
    lines = random_lines(L - 1, seed)
    if L >= 63:
        special = [x for x, _ in HAND]
        for k, s in enumerate(special):
            lines[(k * 7) % (L - 1) if k else 0] = s
        lines[L - 1] = special[-1]
    return lines
