"""Signature group table on the CPU: the host twins of csrc/kernels/gap_table.hip (gap_fold_host,
gap_winners_host, gap_rows_host) behind ``ops.kernels.GapTable``, against a Python dict."""
import random

import pytest
import torch

from log_parser_amd.ops import kernels as K

SIZES = (0, 1, 63, 64, 65, 257, 5000)
DOCS = (0, 0, 2)                      # three launches: one document twice, then a later one


def _pool(k: int, seed: int):
    rng = random.Random(seed)
    return [rng.randrange(-(1 << 63), 1 << 63) for _ in range(k)]


def _pairs(pool, n: int, doc: int, rng: random.Random):
    """n pairs with skewed signature frequencies (a few hot signatures take most pairs); the
    ordinals are distinct lines of document ``doc``."""
    sig = [pool[min(len(pool) - 1, int(len(pool) * rng.random() ** 4))] for _ in range(n)]
    lines = rng.sample(range(1 << 20), n)
    return sig, [(doc << 40) | x for x in lines]


def _fold_dict(d: dict, sig, ordinal, doc: int) -> None:
    for s, o in zip(sig, ordinal):
        g = d.setdefault(s, [0, (1 << 63) - 1, set()])
        g[0] += 1
        g[1] = min(g[1], o)
        g[2].add(doc)


def _rows(table) -> dict:
    sig, count, first, docs = table.rows()
    assert sig.dtype == count.dtype == first.dtype == torch.int64
    out = {s: (c, f, d) for s, c, f, d in zip(sig.tolist(), count.tolist(), first.tolist(), docs.tolist())}
    assert len(out) == sig.numel()                    # every signature once
    return out


def _want(d: dict) -> dict:
    return {s: (c, f, len(docs)) for s, (c, f, docs) in d.items()}


@pytest.mark.parametrize("distinct", [1, 7, 3000])
@pytest.mark.parametrize("n", SIZES)
def test_random_pairs_match_dict(distinct, n):
    rng = random.Random(1000 * distinct + n)
    pool = _pool(distinct, seed=distinct)
    table = K.GapTable("cpu")
    d: dict = {}
    for doc in DOCS:
        sig, ordinal = _pairs(pool, n, doc, rng)
        win = table.fold(torch.tensor(sig, dtype=torch.int64), torch.tensor(ordinal, dtype=torch.int64), doc)
        _fold_dict(d, sig, ordinal, doc)
        # winners: exactly the pairs that hold their group's smallest ordinal after this launch
        assert win.dtype == torch.int64
        assert sorted(win.tolist()) == [i for i, (s, o) in enumerate(zip(sig, ordinal)) if d[s][1] == o]
    assert _rows(table) == _want(d)
    assert table.used == len(d)
    assert table.cap & (table.cap - 1) == 0 and table.cap >= 2 * table.used


def test_later_launch_lowers_first():
    table = K.GapTable("cpu")
    t = lambda xs: torch.tensor(xs, dtype=torch.int64)                  # noqa: E731
    assert sorted(table.fold(t([5, 5, 9]), t([40, 30, 7])).tolist()) == [1, 2]
    # 5: a smaller ordinal arrives (pair 0), 9: a larger one (no winner), 11: new
    assert sorted(table.fold(t([5, 9, 11, 5]), t([10, 8, 99, 20])).tolist()) == [0, 2]
    assert table.fold(t([5]), t([10])).tolist() == [0]                   # a tie with the minimum is a winner too
    assert _rows(table) == {5: (5, 10, 1), 9: (2, 7, 1), 11: (1, 99, 1)}
    assert table.fold(t([]), t([])).numel() == 0
    with pytest.raises(ValueError):
        table.fold(t([1, 2]), t([1]))


def test_documents_counted_once_per_document():
    table = K.GapTable("cpu")
    t = lambda xs: torch.tensor(xs, dtype=torch.int64)                  # noqa: E731
    table.fold(t([1, 1, 2]), t([3, 4, 5]), doc=0)
    table.fold(t([1]), t([6]), doc=0)                                    # the same document again
    table.fold(t([2, 2, 3]), t([(3 << 40) | 1, (3 << 40) | 2, (3 << 40) | 3]), doc=3)
    assert _rows(table) == {1: (3, 3, 1), 2: (3, 5, 2), 3: (1, (3 << 40) | 3, 1)}
    with pytest.raises(ValueError):                                      # document numbers never decrease
        table.fold(t([1]), t([1]), doc=2)


def test_growth_from_cap_4():
    table = K.GapTable("cpu", cap=4)
    assert table.cap == 4 and table.used == 0
    sig = _pool(5000, seed=4)
    assert len(set(sig)) == 5000
    rng = random.Random(4)
    d: dict = {}
    for lo, hi in ((0, 1), (1, 3), (3, 700), (700, 5000)):              # growth at several table sizes
        part = sig[lo:hi]
        ordinal = [rng.randrange(1 << 40) for _ in part]
        win = table.fold(torch.tensor(part, dtype=torch.int64), torch.tensor(ordinal, dtype=torch.int64))
        assert sorted(win.tolist()) == list(range(len(part)))            # every new signature is its group's first
        _fold_dict(d, part, ordinal, 0)
    assert table.used == 5000
    assert table.cap & (table.cap - 1) == 0 and table.cap >= 2 * table.used
    assert _rows(table) == _want(d)
    # the groups go on counting after the growth
    win = table.fold(torch.tensor(sig[:10], dtype=torch.int64), torch.full((10,), -5, dtype=torch.int64), doc=1)
    assert sorted(win.tolist()) == list(range(10))
    rows = _rows(table)
    assert all(rows[s] == (2, -5, 2) for s in sig[:10]) and rows[sig[10]] == _want(d)[sig[10]]
    with pytest.raises(ValueError):
        K.GapTable("cpu", cap=12)


def test_empty_marker_signature():
    """The bit pattern of the table's empty marker, and -1, are signatures like any other."""
    marker = K.GT_EMPTY
    assert marker == -(1 << 63)
    table = K.GapTable("cpu", cap=4)
    t = lambda xs: torch.tensor(xs, dtype=torch.int64)                  # noqa: E731
    win = table.fold(t([marker, -1, marker, 0, -1, marker]), t([9, 8, 4, 7, 6, 5]), doc=0)
    assert sorted(win.tolist()) == [2, 3, 4]
    assert _rows(table) == {marker: (3, 4, 1), -1: (2, 6, 1), 0: (1, 7, 1)}
    assert table.used == 3
    win = table.fold(t([marker, 3, 4, 5, 6, 7, 8, 9]), t([1 << 40] * 8), doc=1)      # grows with the marker inside
    assert sorted(win.tolist()) == list(range(1, 8))
    rows = _rows(table)
    assert rows[marker] == (4, 4, 2) and rows[-1] == (2, 6, 1) and len(rows) == 10 and table.used == 10
    assert table.fold(t([marker]), t([2]), doc=1).tolist() == [0]
    assert _rows(table)[marker] == (5, 2, 2)
