"""Cases shared by the spans tests (test_spans.py, test_span_table.py and their GPU siblings): the
hand-written lines of the text kernel with what ``golden`` says of them, and pieces of made-up
pairs with a dict fold as the specification of ``K.SpanTable``."""
import random
import re

import torch

from log_parser_amd import golden
from log_parser_amd.ops import kernels as K
from values_cases import index

U64 = (1 << 64) - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
S = b"2025-09-19T12:01:02"

SPAN_HAND = [
    b"INFO request done rid=abc12345",                                  # a token that ends with the line
    b"x " * 505 + b"abcdefgh12345678ijkl",                              # cut at byte 1,024: 14 bytes of it are left
    b"y " * 509 + b"abcd1234efgh5678",                                  # cut at byte 1,024: 6 bytes are left, no key
    b"0123456 abcdefg12345678 tail",                                    # a token that straddles a 16-byte block
    b" ".join(b"tok%05dxy" % i for i in range(9)),                      # nine tokens: the ninth is ignored
    b"rid=abc12345 again abc12345 and ABC12345",                        # the same id three times: one pair
    b"a1" * 32 + b"z " + b"b2" * 32,                                    # 65 bytes: no key; 64 bytes: a key
    b"abcdefghijkl mnopqrstuvwx",                                       # no digit
    b"REQ12345ab req12345AB Req12345Ab",                                # one id in three cases
    b"",
    S + b".123Z",                                                       # only a stamp
    S + b"Z abc12345",                                                  # (with min_len 4 the stamp's own tokens are keys)
    b"abc12345 " + S + b",5+02:00 next9876543",                         # an id in front of the stamp
    b"rid=abc12345\r",                                                  # CR LF: the CR ends the token
    b"[" + S + b"] 20250919T120102 x",                                  # a digit run that is no stamp
]

_RUN = re.compile(rb"[0-9A-Za-z]+")


def signed(x: int) -> int:
    x &= U64
    return x - (1 << 64) if x >> 63 else x


def key_places(line: bytes, min_len: int):
    """[(key, place)] of a line, written without ``golden.line_key_tokens``: place = offset |
    length << 10 of the token's first occurrence."""
    out, seen = [], set()
    for m in _RUN.finditer(line[:1024]):
        t = m.group()
        if not min_len <= len(t) <= 64 or not re.search(rb"[0-9]", t):
            continue
        k = golden.fnv1a64(t.lower())
        if k in seen:
            continue
        if len(out) == 8:
            break
        seen.add(k)
        out.append((k, m.start() | len(t) << K.KEY_POS_LEN_SHIFT))
    assert [k for k, _ in out] == golden.line_keys(line, min_len)
    return out


def want_span_keys(lines, min_len: int = 8, shift: int = 0):
    """(signatures, stamps, [(line, key, place)] in line and byte order, lines with a triple, the
    65 level counts) of ``K.span_keys`` from ``golden``, signed as the int64 columns are."""
    sigs = [signed(golden.line_signature(x)) for x in lines]
    ts = [K.TS_NONE if (t := golden.line_timestamp(x)) is None else t for x in lines]
    triples, held, levels = [], 0, [0] * K.SPAN_LEVELS
    for i, x in enumerate(lines):
        mine = [(k, p) for k, p in key_places(x, min_len) if golden.span_level(k) >= shift]
        triples += [(i, signed(k), p) for k, p in mine]
        if mine:
            held += 1
            levels[max(golden.span_level(k) for k, _ in mine)] += 1
    return sigs, ts, triples, held, levels


def span_index(lines):
    """(text, ls, ll) on the CPU with the lines as they are -- a CR stays part of its line."""
    data = b"\n".join(lines)
    text = torch.zeros(K.padded_len(len(data)), dtype=torch.uint8)
    if data:
        text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    starts, at = [], 0
    for x in lines:
        starts.append(at)
        at += len(x) + 1
    return (text[:len(data)].clone() if data else torch.zeros(16, dtype=torch.uint8),
            torch.tensor(starts, dtype=torch.int64), torch.tensor([len(x) for x in lines], dtype=torch.int32))


def sorted_triples(line, key, tok):
    return sorted(zip(line.tolist(), key.tolist(), tok.tolist()))


# ---- the span table against a dict fold

SIDE, ZERO = 10 ** 6 + 1, 10 ** 6 + 2       # the ids whose keys are the empty marker and 0


def id_token(no: int) -> bytes:
    return b"Id%07dXy" % no                 # (mixed case: the table keeps it lowered)


def id_key(no: int) -> int:
    return K.GT_EMPTY if no == SIDE else 0 if no == ZERO else signed(golden.fnv1a64(id_token(no).lower()))


class PairPiece:
    """A piece of ``len(ids)`` lines, line i holding the id ``ids[i]`` behind a lead-in of varying
    length, with made-up signatures and effective times (about one line in seven has none; none
    at all with ``timed=False``): the inputs of ``SpanTable.fold`` on ``device`` and, as Python
    lists, of ``dict_fold``."""

    def __init__(self, ids, seed: int, line_base: int, device, timed: bool = True):
        rng = random.Random(seed)
        self.ids, self.line_base, self.device = list(ids), line_base, torch.device(device)
        self.lead = [b"ab " * rng.randrange(0, 6) + rng.choice((b"", b"rid=", b"[")) for _ in self.ids]
        self.lines = [ld + id_token(no) + rng.choice((b"", b" done", b"] x")) for ld, no in zip(self.lead, self.ids)]
        self.sig = [signed(rng.getrandbits(64)) for _ in self.ids]
        self.eff = [K.TS_NONE if not timed or rng.random() < 0.15 else rng.randrange(-10 ** 6, 10 ** 12) for _ in self.ids]
        self.order = list(range(len(self.ids)))
        rng.shuffle(self.order)             # the pairs come in no particular order
        text, ls, ll = index(self.lines, 0) if self.lines else span_index([])
        self.text, self.ls = text.to(self.device), ls.to(self.device)

    def args(self):
        dev = self.device
        line = torch.tensor(self.order, dtype=torch.int32, device=dev)
        key = torch.tensor([id_key(self.ids[i]) for i in self.order], dtype=torch.int64, device=dev)
        tok = torch.tensor([len(self.lead[i]) | len(id_token(self.ids[i])) << K.KEY_POS_LEN_SHIFT for i in self.order],
                           dtype=torch.int32, device=dev)
        return (line, key, tok, torch.tensor(self.sig, dtype=torch.int64, device=dev),
                torch.tensor(self.eff, dtype=torch.int64, device=dev), self.text, self.ls, self.line_base)


def dict_fold(piece: PairPiece, into=None):
    """{key: [count, first, last, tmin, tmax, opens, closes, toklen, token]}: the specification of
    ``SpanTable.fold`` -- count, min and max per key; opens and the token from the line that is the
    key's first, closes from the one that is its last."""
    into = {} if into is None else into
    for i, no in enumerate(piece.ids):
        g, t = piece.line_base + i, piece.eff[i]
        tok = id_token(no).lower()
        e = into.setdefault(id_key(no), [0, I64_MAX, I64_MIN, I64_MAX, I64_MIN, 0, 0, 0, b""])
        e[0] += 1
        if g < e[1]:
            e[1], e[5], e[7], e[8] = g, piece.sig[i], len(tok), tok
        if g > e[2]:
            e[2], e[6] = g, piece.sig[i]
        if t != K.TS_NONE:
            e[3], e[4] = min(e[3], t), max(e[4], t)
    return into


def rows_of(ref: dict):
    return sorted((k,) + tuple(e) for k, e in ref.items())


def table_rows(tab):
    cols = tab.rows()
    toks, lens = cols[9].cpu().numpy(), cols[8].tolist()
    assert all(not toks[j, ln:].any() for j, ln in enumerate(lens))                  # zero padded
    nums = [c.tolist() for c in cols[:9]]
    return sorted(tuple(c[j] for c in nums) + (bytes(toks[j, :lens[j]]),) for j in range(len(lens)))


def in_sample(key: int, shift: int) -> bool:
    return golden.span_level(key & U64) >= shift


def check_table(device, n: int, distinct: int, seed: int, cap: int = 1 << 12):
    """Two folds of ``n`` pairs over ``distinct`` ids (the second continues the log: later lines),
    rows == dict fold after each; a purge to sample 1, rows again; a third fold of the same ids,
    the purged ones filtered out as the text kernel would. Returns the table."""
    rng = random.Random(seed)
    ids = [k if k < distinct else rng.randrange(distinct) for k in range(n)]
    rng.shuffle(ids)
    tab = K.SpanTable(device, cap=cap)
    ref = {}
    for part in range(2):
        piece = PairPiece(ids, seed + part, part * n, device)
        tab.fold(*piece.args())
        dict_fold(piece, into=ref)
        assert table_rows(tab) == rows_of(ref), part
        assert tab.used == len(ref) and 2 * tab.used <= tab.cap and tab._used.tolist()[1] == 0
    dropped = tab.purge(1)
    ref = {k: e for k, e in ref.items() if in_sample(k, 1)}
    assert dropped == len(set(map(id_key, ids))) - len(ref) and table_rows(tab) == rows_of(ref) and tab.used == len(ref)
    kept = [no for no in ids if in_sample(id_key(no), 1)]
    piece = PairPiece(kept, seed + 2, 2 * n, device)
    tab.fold(*piece.args())
    dict_fold(piece, into=ref)
    assert table_rows(tab) == rows_of(ref) and tab._used.tolist()[1] == 0
    return tab
