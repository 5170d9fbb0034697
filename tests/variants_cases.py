"""Cases for the variants tests (test_variants.py, test_var_table.py and their GPU siblings):
hand-written lines with the fields ``golden.line_fields`` must give, the triples a walk must emit,
and the value table's scenarios against a dict fold -- written once, run on either device."""
import random

import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K

U64 = (1 << 64) - 1
S = b"2025-09-19T12:01:02"          # a valid stamp core: 19 bytes

# (line, [(field, token)]): next to values_cases.HAND, what only this report can get wrong
VAR_HAND = [
    # a token cut at byte 1024 is the value its first part spells; one that starts there is none
    (b"x" * 1019 + b" 123456", [(0, b"1234")]), (b"x" * 1017 + b" ab12cdef", [(0, b"ab12cd")]),
    (b"x" * 1023 + b" 77", []), (b"x" * 1020 + b" abc1", []),
    # a ninth field, and fields without a number's shape
    (b"a1 b2 c3 d4 e5 f6 g7 h8 i9", [(i, b"%c%d" % (97 + i, i + 1)) for i in range(8)]),
    (b"pod web-7f9c4d5b8-x2k9q up", [(0, b"7f9c4d5b8"), (1, b"x2k9q")]),
    # a field that starts inside the stamp is hidden; the next one is field 0
    (b"2025-09-19T12:01:00Z7 up 3", [(0, b"3")]), (b"2025-09-19T12:01:007 up 3x", [(0, b"3x")]),
    (S + b".250Z status 503", [(0, b"503")]), (b"[" + S + b"] exit 137", [(0, b"137")]),
    # case is kept: three values, not one
    (b"0xAB 0xab 0xAb", [(0, b"0xAB"), (1, b"0xab"), (2, b"0xAb")]),
    (b"REQ9 req9", [(0, b"REQ9"), (1, b"req9")]),
    # CR at the end of a line that was split at LF only
    (b"exit code 137\r", [(0, b"137")]), (S + b" shard 3\r", [(0, b"3")]),
    # no field
    (b"", []), (b"no digit here", []), (b"\r", []),
]


def signed(x: int) -> int:
    x &= U64
    return x - (1 << 64) if x >> 63 else x


def want_triples(lines):
    """(signatures, [(line, field key, token hash)] in line and byte order, lines with a field) from
    ``golden.line_fields`` / ``var_hash``, signed as the kernels' int64 columns are."""
    sigs = [golden.line_signature(x) for x in lines]
    per = [golden.line_fields(x) for x in lines]
    return ([signed(s) for s in sigs],
            [(i, signed(golden.val_key(sigs[i], j)), signed(golden.var_hash(t))) for i, fs in enumerate(per) for j, _, t in fs],
            sum(map(bool, per)))


# ---- the value table against a dict fold

def side_pair(value: int):
    """(field, value) whose table key equals the empty marker: field = GT_EMPTY - value * CT_MIX."""
    return signed(K.GT_EMPTY - value * K.CT_MIX), signed(value)


def make_triples(n: int, distinct: int, seed: int, base: int = 0, hot: bool = False):
    """``n`` triples over ``distinct`` (field, value) pairs (every pair occurs when n >= distinct)
    in about ``distinct / 6`` fields; ordinals rise from ``base`` with repeats. ``hot``: nine in
    ten triples hold the first pair."""
    rng = random.Random(seed)
    fields = [signed(rng.getrandbits(64)) for _ in range(max(1, distinct // 6))]
    pairs = [(fields[k % len(fields)], signed(rng.getrandbits(64))) for k in range(distinct)]
    out = []
    for i in range(n):
        k = i if i < distinct else rng.randrange(distinct)
        if hot and i and rng.random() < 0.9:
            k = 0
        out.append(pairs[k % distinct] + (base + i // 3,))
    rng.shuffle(out)
    return out


def dict_fold(triples, skip=(), into=None):
    """{table key: [field, value, count, first, last]}: the specification of ``VarTable.fold``."""
    into = {} if into is None else into
    for f, v, o in triples:
        if f in skip:
            continue
        e = into.setdefault(golden.var_cell_key(f & U64, v & U64), [f, v, 0, o, o])
        e[2] += 1
        e[3] = min(e[3], o)
        e[4] = max(e[4], o)
    return into


def rows_of(ref: dict):
    return sorted(tuple(e) for e in ref.values())


def table_rows(tab):
    return sorted(zip(*(c.tolist() for c in tab.rows())))


def cols(triples, device):
    f, v, o = (torch.tensor(c, dtype=torch.int64, device=device) for c in zip(*triples)) if triples else \
        (torch.empty(0, dtype=torch.int64, device=device),) * 3
    return f, v, o


def skip_set(fields, device):
    tab = K.GapTable(device)
    f = torch.tensor(sorted(set(fields)), dtype=torch.int64, device=device)
    tab.fold(f, torch.zeros_like(f), winners=False)
    return tab


def want_winners(ref: dict, triples):
    return sorted(i for i, (f, v, o) in enumerate(triples)
                  if (e := ref.get(golden.var_cell_key(f & U64, v & U64))) is not None and e[3] == o)


def check_fold(device, triples, tile: int = 0, skip_fields=(), cap: int = 1 << 12):
    """Fold, rows == dict fold; winners; purge of a third of the fields, rows and winners again; the
    same triples folded once more into what is left. Returns the table."""
    tab = K.VarTable(device, cap=cap, tile=tile)
    skip = skip_set(skip_fields, device) if skip_fields else None
    f, v, o = cols(triples, device)
    tab.fold(f, v, o, skip=skip)
    ref = dict_fold(triples, set(skip_fields))
    assert table_rows(tab) == rows_of(ref)
    assert tab.used == len(ref) and 2 * tab.used <= tab.cap
    assert sorted(tab.winners(f, v, o).tolist()) == want_winners(ref, triples)
    # purge: the rows without those fields, through the path of growth
    fields = sorted({e[0] for e in ref.values()})
    gone = set(fields[::3])
    dropped = tab.purge(torch.tensor(sorted(gone), dtype=torch.int64, device=device))
    ref = {k: e for k, e in ref.items() if e[0] not in gone}
    assert dropped == len(rows_of(dict_fold(triples, set(skip_fields)))) - len(ref)
    assert table_rows(tab) == rows_of(ref) and tab.used == len(ref)
    assert sorted(tab.winners(f, v, o).tolist()) == want_winners(ref, triples)         # a purged entry wins nothing
    # ... and the fold goes on: later ordinals, the purged fields now skipped
    later = [(a, b, c + 10 ** 6) for a, b, c in triples]
    f2, v2, o2 = cols(later, device)
    both = skip_set(set(skip_fields) | gone, device) if (gone or skip_fields) else None
    tab.fold(f2, v2, o2, skip=both)
    dict_fold(later, set(skip_fields) | gone, into=ref)
    assert table_rows(tab) == rows_of(ref)
    assert tab.winners(f2, v2, o2).numel() == 0                                        # every first line is an earlier one
    return tab
