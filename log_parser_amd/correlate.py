"""Correlation report: the failing line carries a request id, a trace id, a pod hash or an address
-- what else does the log say about that id? (``golden.correlate`` is the specification.)

The lead-up report is positional. In a concurrent service the lines of the failed request are
interleaved with everyone else's, lie thousands of lines away and also after the event; this
report follows the id instead. A *key* is the hash of an id-like token of a line
(csrc/kernels/key_core.h), the *event keys* are the keys of the lines that carry an event.

Two passes over ONE log, one text kernel (k_line_keys, csrc/kernels/correlate.hip) in two forms:

1. the pieces of pieces.py -- the matchers run, because the events say where the failures are.
   The kernel walks only the event lines of a piece (``sel``), and their (key, line) pairs are
   folded into the ``GapTable`` ``on_event``: per event key its event lines and the first of them.
   A log without event keys is done here.
2. the same source again WITHOUT matchers (``pieces.stream_lines``). The kernel walks every line
   and emits only the keys that ``on_event`` holds (``table``); the pairs are folded into ``total``
   (all lines of a key, the first of them) and, with the ordinal negated, into ``last``. The lines
   that become their key's first come to the host as its example.

Memory is bounded by the event keys, not by the ids of the log -- a table of every id of a large
log would be as large as the log. That is why there are two passes, why the source must be
readable twice, and why there is no accumulator fed over time. A document or a resident log stays
where it is between the passes; a stream from the host is uploaded twice. No carry between pieces
is needed: a key is a property of one line, and the tables do the rest, so the report is the
one-document report at every chunk size. Nothing is scored and the frequency window is not touched.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .accumulator import U64, Examples
from .engine import Engine
from .golden import correlate_check_args as check_args
from .golden import correlate_row, line_key_tokens
from .ops import kernels as K
from .pieces import Piece, document_piece, stream_lines, stream_pieces

_I64_MIN = -(1 << 63)


def _require(key: torch.Tensor, table: K.GapTable, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(count, smallest ordinal) that ``table`` holds for every key of ``key``: all must be in it."""
    count, first, found, groups = table.lookup(key)
    if groups == 0:
        raise RuntimeError("correlate: the %s table is empty" % what)
    if not bool(found.all()):
        raise RuntimeError("correlate: an event key is missing from the %s table (did the source change "
                           "between the passes?)" % what)
    return count, first


class _Correlation:
    """The tables of one report: ``add_events`` for every piece of pass 1, ``add_lines`` for every
    piece of pass 2 (its events, if it has any, are not looked at), then ``report``."""

    def __init__(self, engine: Engine, min_len: int):
        self.engine, self.min_len = engine, int(min_len)
        self.on_event = K.GapTable(engine.device)       # (key, event line): event lines, the first of them
        self.total = K.GapTable(engine.device)          # (key, line): lines, the first of them
        self.last = K.GapTable(engine.device)           # (key, -line): minus the last of them
        self.lines = self.events = self.event_lines = 0
        self.walked = self.key_lines = 0
        self._examples = Examples("correlate")          # key -> (global line, raw line)

    def add_events(self, piece: Piece) -> None:
        n, base = piece.ls.numel(), piece.line_base
        self.lines += n
        self.events += piece.ev_line.numel()
        if n == 0 or piece.ev_line.numel() == 0:
            return
        ev = torch.unique(piece.ev_line)                # sorted, distinct
        self.event_lines += ev.numel()
        line, key, _, _ = K.line_keys(piece.text, piece.ls, piece.ll, sel=ev, min_len=self.min_len)
        # (the signed 64-bit minimum of the table is the first event line)
        self.on_event.fold(key, line.long() + base, winners=False)

    def add_lines(self, piece: Piece) -> None:
        self.walked += piece.ls.numel()
        if piece.ls.numel() == 0:
            return
        line, key, _, (m, held) = K.line_keys(piece.text, piece.ls, piece.ll, table=self.on_event, min_len=self.min_len)
        self.key_lines += held
        if m == 0:
            return
        ordinal = line.long() + piece.line_base
        win = self.total.fold(key, ordinal)
        self.last.fold(key, -ordinal, winners=False)    # the table keeps a signed minimum: minus the last line
        if win.numel():
            self._examples.record(key, ordinal, win, piece.raw_lines(line[win]))

    def report(self, top: Optional[int], order: str, min_lines: int, max_share: float) -> dict:
        out = {"totalLines": self.lines, "events": self.events, "eventLines": self.event_lines,
               "minLength": self.min_len, "keys": 0, "keyLines": self.key_lines, "top": []}
        key, n_ev, first_ev, _ = self.on_event.rows()
        out["keys"] = int(key.numel())
        if key.numel() == 0:
            return out
        if self.walked != self.lines:
            raise RuntimeError("correlate: %d lines in the first pass, %d in the second" % (self.lines, self.walked))
        n, first = _require(key, self.total, "line")
        _, neg_last = _require(key, self.last, "last-line")
        # (exact: line counts are far below 2^53, and Python compares the same way)
        keep = (n >= min_lines) & (n.double() <= max_share * self.lines)
        key, n_ev, first_ev, n, first, neg_last = (t[keep] for t in (key, n_ev, first_ev, n, first, neg_last))
        pick = torch.sort(key ^ _I64_MIN, stable=True)[1]           # the key as an unsigned number
        if order == "first":
            by = [(first_ev, False)]
        elif order == "lines":
            by = [(first, False), (n_ev, True), (n, True)]
        else:
            by = [(first, False), (n, True), (n_ev, True)]
        for col, desc in by:                                        # least significant first
            pick = pick[torch.sort(col[pick], descending=desc, stable=True)[1]]
        if top is not None:
            pick = pick[:max(0, int(top))]
        rows = torch.stack([key[pick], n_ev[pick], first_ev[pick], n[pick], first[pick], -neg_last[pick]]).cpu().tolist()
        for k, ne, fe, c, f, last in zip(*rows):
            raw = self._examples.take(k, f)
            if not (0 < ne <= c and f <= fe <= last):
                raise RuntimeError("correlate: %016x has %d event lines of %d, lines %d / %d / %d"
                                   % (k & U64, ne, c, f, fe, last))
            if (k & U64) not in dict(line_key_tokens(raw, self.min_len)):
                raise RuntimeError("correlate: line %d does not hold the key %016x" % (f + 1, k & U64))
            out["top"].append(correlate_row(k & U64, ne, fe, c, f, last, raw, self.min_len))
        return out


def correlate_document(eng: Engine, text, n: int, data: bytes, min_len: int = 8, top: Optional[int] = 20,
                       order: str = "events", min_lines: int = 2, max_share: float = 0.25) -> dict:
    """The report of a staged document (``Engine.correlate_document``): both passes read the staged
    text, and the examples are cut from the host copy."""
    check_args(min_len, order, min_lines, max_share)
    acc = _Correlation(eng, min_len)
    piece = document_piece(eng, text, n, data)
    acc.add_events(piece)
    if acc.on_event.used:
        acc.add_lines(piece)
    return acc.report(top, order, min_lines, max_share)


def correlate_stream(eng: Engine, src, chunk_bytes: Optional[int] = None, min_len: int = 8,
                     top: Optional[int] = 20, order: str = "events", min_lines: int = 2,
                     max_share: float = 0.25) -> dict:
    """The report of ONE log in chunks: a bytes-like source (bytes, mmap, ``RepeatBuffer``) or a
    ``ResidentLog``. The source is walked twice -- a host source is uploaded twice, a resident log
    is read in place twice -- and must not change in between. Exactly the one-document report,
    whatever the chunk size."""
    check_args(min_len, order, min_lines, max_share)
    acc = _Correlation(eng, min_len)
    with stream_pieces(eng, src, chunk_bytes) as pieces:
        for piece in pieces:
            acc.add_events(piece)
    if acc.on_event.used:
        with stream_lines(eng, src, chunk_bytes) as pieces:
            for piece in pieces:
                acc.add_lines(piece)
    return acc.report(top, order, min_lines, max_share)
