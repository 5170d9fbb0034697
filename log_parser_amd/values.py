"""Values report: which numbers do the line templates of a log carry, and where do they peak?
(``golden.values`` is the specification.)

Every other report throws the numbers of a line away: the template turns each digit-holding token
into ``0``. Here those tokens are the *fields* of the line, numbered in byte order behind its
stamp, and a *group* is (template signature, field number) under the 64-bit key ``val_key``. One
text kernel, k_line_vals (csrc/kernels/values.hip, the walk in val_core.h), signs every line and
emits its values as (line, key, value) triples, 0..8 per line.

:class:`ValueAccumulator` walks ONE log in pieces without events -- the walk without the
matchers of ``accumulator.LineAccumulator`` -- and folds the triples of a run, with the
global line ``g``, into five ``GapTable`` s (count and a signed 64-bit minimum per key):

=============== ============================================ =====================================
``by_template`` (signature, g), every line                   lines per template
``lo``          (key, value)                                 count, min
``hi``          (key, -((value << 32) | (0xFFFFFFFF - g)))   max and the first line that holds it
``first``       (key, (g << 30) | value), with winners       first line, its value, the example
``last``        (key, -((g << 30) | value))                  last line and its value
=============== ============================================ =====================================

Values are below 2^30 and lines below 2^32, so every packed ordinal stays below 2^62. The exact
sums are kept in torch: per run ``unique`` + ``index_add_``, merged into a running sorted (key,
sum) pair of tensors -- as many entries as templates x fields, not lines. A field belongs to one
line, so no carry between runs is needed and the report is the one-document report at every chunk
size. Filters and order are exact Python arithmetic on the host over the groups' rows. Nothing is
scored and the frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from .accumulator import U64, Examples, LineAccumulator
from .engine import Engine
from .golden import VAL_MAX_LINES, VAL_PER_LINE, val_key
from .golden import values_check_args as check_args
from .golden import values_order_key, values_row
from .ops import kernels as K
from .pieces import Piece

_LOW32 = 0xFFFFFFFF
_LOW30 = (1 << 30) - 1


class ValueAccumulator(LineAccumulator):
    """The values report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log: their first line follows the lines so far.

    Only the lines that become their group's first line with a value come to the host, as its
    example: one per NEW (template, field) in steady state."""

    def __init__(self, engine: Engine, guard: Optional[Callable] = None, line_base: int = 0):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.value_accumulator``). ``line_base``: the number (0-based) of
        the log's first line -- a log that continues an earlier one, and the tests of the line
        limit."""
        if isinstance(line_base, bool) or not isinstance(line_base, int) or not 0 <= line_base < VAL_MAX_LINES:
            raise ValueError("line_base must be an integer in [0, 2^32)")
        super().__init__(engine, guard)
        dev = engine.device
        self.by_template = K.GapTable(dev)      # (signature, g): lines per template
        self.lo = K.GapTable(dev)               # (key, value): count, min
        self.hi = K.GapTable(dev)               # (key, -((value << 32) | (0xFFFFFFFF - g))): max, its first line
        self.first = K.GapTable(dev)            # (key, (g << 30) | value): first line and its value
        self.last = K.GapTable(dev)             # (key, -((g << 30) | value)): last line and its value
        self._sum_key = torch.empty(0, dtype=torch.int64, device=dev)     # sorted, distinct
        self._sum = torch.empty(0, dtype=torch.int64, device=dev)
        self.line_base = self.next_line = int(line_base)
        self.values = self.value_lines = 0
        self._examples = Examples("ValueAccumulator")             # key -> ((g << 30) | value, (signature, raw line))

    def _add_piece(self, piece: Piece) -> None:
        text, ls, ll = piece.text, piece.ls, piece.ll
        n, base = ls.numel(), self.next_line
        if base + n >= VAL_MAX_LINES:           # before anything is folded: the packed ordinals hold 32 bits of line
            raise ValueError("values: the log reaches line 2^32 (%d lines so far, %d more)" % (base, n))
        if n == 0:
            return
        self.next_line = base + n
        dev = text.device
        sig, line, key, value, (m, held) = K.line_values(text, ls, ll)
        self.by_template.fold(sig, torch.arange(base, base + n, dtype=torch.int64, device=dev), winners=False)
        self.values += m
        self.value_lines += held
        if m == 0:
            return
        g, v = line.long() + base, value.long()
        self.lo.fold(key, v, winners=False)
        # the table keeps a signed minimum: of the negated pack it is the largest value, then the smallest line
        self.hi.fold(key, -((v << 32) | (_LOW32 - g)), winners=False)
        at = (g << 30) | v
        win = self.first.fold(key, at)
        self.last.fold(key, -at, winners=False)
        if win.numel():
            # the lines that became their group's first: their bytes are its example, their signature its template
            rows = torch.stack([key[win], at[win], sig[line[win].long()]]).cpu().tolist()
            self._examples.put_all(rows[0], rows[1], zip(rows[2], piece.raw_lines(line[win])))
        # exact sums: this run's per key, merged into the running sorted pair
        uk, inv = torch.unique(key, return_inverse=True)
        part = torch.zeros(uk.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, v)
        allk, inv = torch.unique(torch.cat([self._sum_key, uk]), return_inverse=True)
        self._sum = torch.zeros(allk.numel(), dtype=torch.int64, device=dev).index_add_(
            0, inv, torch.cat([self._sum, part]))
        self._sum_key = allk

    # ------------------------------------------------------------------ the report
    def report(self, top: Optional[int] = 20, order: str = "peak", min_count: int = 5, min_fill: float = 0.9,
               varying: bool = True) -> dict:
        """The report of everything added so far (more can be added afterwards)."""
        check_args(order, min_count, min_fill)
        with self._guard():
            return self._report(top, order, min_count, min_fill, varying)

    def _report(self, top: Optional[int], order: str, min_count: int, min_fill: float, varying: bool) -> dict:
        out = {"totalLines": self.next_line - self.line_base, "valueLines": self.value_lines, "values": self.values,
               "templates": 0, "fields": 0, "top": []}
        if out["totalLines"] == 0:
            return out
        t_sig, t_lines, _, _ = self.by_template.rows()
        out["templates"] = int(t_sig.numel())
        if self.values == 0:
            return out
        key, count, vmin = self.lo.sorted_rows()
        cols = [key, count, vmin, self._sum]
        for table, what in ((self.hi, "max"), (self.first, "first-line"), (self.last, "last-line")):
            k, c, o = table.sorted_rows()
            if k.numel() != key.numel() or not bool((k == key).all()) or not bool((c == count).all()):
                raise RuntimeError("ValueAccumulator: the %s table does not hold the groups of the count table" % what)
            cols.append(o)
        if self._sum_key.numel() != key.numel() or not bool((self._sum_key == key).all()):
            raise RuntimeError("ValueAccumulator: the sums do not cover the groups of the count table")
        out["fields"] = int(key.numel())
        per_sig = dict(zip(*torch.stack([t_sig, t_lines]).cpu().tolist()))
        groups = []
        rows = torch.stack(cols).cpu().tolist()
        for k, c, lo, total, hi, first, last, (signed, raw) in zip(*rows, self._examples.take_all(rows[0], rows[5])):
            # the key says neither template nor field: the template is the one the kernel gave the example
            # line, the field the one whose key this is (values_row recomputes both from the line's bytes
            # for the rows that are listed)
            sig = signed & U64
            j = next((j for j in range(VAL_PER_LINE) if val_key(sig, j) == k & U64), None)
            if j is None or signed not in per_sig:
                raise RuntimeError("ValueAccumulator: line %d does not hold the field of the key %016x"
                                   % ((first >> 30) + 1, k & U64))
            lines = per_sig[signed]
            vmax, max_line = (-hi) >> 32, _LOW32 - ((-hi) & _LOW32)
            if not (0 < c <= lines and lo <= vmax and lo * c <= total <= vmax * c):
                raise RuntimeError("ValueAccumulator: %016x has %d values on %d lines, min %d, max %d, sum %d"
                                   % (k & U64, c, lines, lo, vmax, total))
            if c >= min_count and c >= min_fill * lines and (not varying or lo < vmax):
                groups.append((values_order_key(order, sig, j, c, total, vmax, first >> 30),
                               (sig, j, c, total, lo, vmax, max_line, first >> 30, first & _LOW30,
                                (-last) >> 30, (-last) & _LOW30, lines, raw)))
        groups.sort(key=lambda g: g[0])
        if top is not None:
            groups = groups[:max(0, int(top))]
        out["top"] = [values_row(*row) for _, row in groups]
        return out


def values_document(eng: Engine, data: bytes, top: Optional[int] = 20, order: str = "peak", min_count: int = 5,
                    min_fill: float = 0.9, varying: bool = True) -> dict:
    """The report of one document (``Engine.values_bytes``)."""
    check_args(order, min_count, min_fill)
    acc = ValueAccumulator(eng)
    acc.add_document(data)
    return acc._report(top, order, min_count, min_fill, varying)


def values_stream(eng: Engine, src, chunk_bytes: Optional[int] = None, top: Optional[int] = 20, order: str = "peak",
                  min_count: int = 5, min_fill: float = 0.9, varying: bool = True) -> dict:
    """The report of ONE log in chunks: a bytes-like source (bytes, mmap, ``RepeatBuffer``) or a
    ``ResidentLog``. Exactly the one-document report, whatever the chunk size."""
    check_args(order, min_count, min_fill)
    acc = ValueAccumulator(eng)
    acc.add_stream(src, chunk_bytes)
    return acc._report(top, order, min_count, min_fill, varying)
