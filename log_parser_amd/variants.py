"""Variants report: which values do the variable tokens of a line template take, how often, and
which value is the odd one out? (``golden.variants`` is the specification.)

The categorical sibling of values.py: the same *fields* (``golden.line_fields``: the digit-holding
tokens of a line behind its stamp, numbered in byte order) under the same group key ``val_key``,
but a field counts whether or not it reads as a number, and its value is the token itself, through
the 64-bit ``var_hash``. One text kernel, k_line_vars (csrc/kernels/variants.hip, the walk in
var_core.h), signs every line and emits its fields as (line, field key, token hash) triples, 0..8
per line; the ``VarTable`` (var_table.h) keeps count, first and last line per (field, value).

A field with at most ``max_distinct`` = D distinct values over the whole log is *enumerable* and is
reported exactly; one with more -- an id, a counter, a duration -- is *unbounded* and only counted.
:class:`VariantAccumulator` walks ONE log in pieces without events and, per piece, in this order:

1. ``K.line_vars``;
2. the signatures into ``by_template`` (lines per template);
3. the triples into the table, the fields of the ``unbounded`` set skipped;
4. the census: distinct values per field, from the table's rows;
5. the fields above D into ``unbounded``, their rows purged;
6. ``VarTable.winners``: the triples that hold their value's first line. Only those lines come to
   the host, as the value's example.

What the order guarantees:

* after a piece the table holds at most (enumerable fields) x D rows;
* within a piece it holds at most that plus the piece's triples;
* a field that is unbounded brings no line to the host: its rows are gone before the winners are
  asked for. (A field brings at most D lines in all, the values it showed in the pieces before
  the one that took it above D -- none when its first piece does.)

Chunk independence: the table is exact for every field that is not in ``unbounded``, and a field
enters ``unbounded`` only when its exact distinct count so far exceeds D. The distinct count of a
prefix never exceeds that of the whole log, and the last piece's census sees the whole log: a field
is unbounded at the end if and only if it has more than D values in the whole log, wherever the
pieces are cut. Nothing of an enumerable field is ever dropped, so its rows are those of the
one-document walk. ``D`` is fixed when the accumulator is made -- a purged field cannot come back.

Known limits: ``golden.variants``'; two (field, value) pairs that share the 64-bit
``var_cell_key`` are one value (the table's key). Filters and order are exact Python arithmetic on
the host over the rows. Nothing is scored and the frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch

from .accumulator import U64, Examples, LineAccumulator
from .engine import Engine
from .golden import VAL_PER_LINE, val_key, var_cell_key
from .golden import variants_check_args as check_args
from .golden import variants_head, variants_listed, variants_order_key, variants_row
from .ops import kernels as K
from .pieces import Piece

_MAX_LINE_BASE = 1 << 62


class VariantAccumulator(LineAccumulator):
    """The variants report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log: their first line follows the lines so far.

    ``example_lines`` counts the lines fetched to the host; ``example_fields`` the field key of
    each of them (tests: an unbounded field fetches none)."""

    def __init__(self, engine: Engine, max_distinct: int = 64, guard: Optional[Callable] = None, line_base: int = 0):
        """``max_distinct``: the most distinct values of an enumerable field (2..4096), fixed here.
        ``guard``: a context manager factory entered around every use of the engine (the parser's
        lock, ``LogParser.variant_accumulator``). ``line_base``: the number (0-based) of the log's
        first line -- a log that continues an earlier one."""
        check_args(max_distinct)
        if isinstance(line_base, bool) or not isinstance(line_base, int) or not 0 <= line_base < _MAX_LINE_BASE:
            raise ValueError("line_base must be an integer in [0, 2^62)")
        super().__init__(engine, guard)
        dev = engine.device
        self.max_distinct = max_distinct
        self.by_template = K.GapTable(dev)      # (signature, g), every line: lines per template
        self.table = K.VarTable(dev)            # (field, value): count, first, last
        self.skip = K.GapTable(dev)             # the unbounded fields, as the fold's skip set
        self.unbounded: set = set()             # ... and on the host (signed keys)
        self.line_base = self.next_line = int(line_base)
        self.tokens = self.field_lines = 0
        self.example_lines = 0
        self.example_fields: List[int] = []
        self._examples = Examples("VariantAccumulator")     # cell key -> (g, (signature, raw line))

    def _add_piece(self, piece: Piece) -> None:
        text, ls, ll = piece.text, piece.ls, piece.ll
        n, base = ls.numel(), self.next_line
        if n == 0:
            return
        self.next_line = base + n
        dev = text.device
        sig, line, field, value, (m, held) = K.line_vars(text, ls, ll)
        self.by_template.fold(sig, torch.arange(base, base + n, dtype=torch.int64, device=dev), winners=False)
        self.tokens += m
        self.field_lines += held
        if m == 0:
            return
        g = line.long() + base
        self.table.fold(field, value, g, skip=self.skip)
        # census: the exact distinct values of every field the table holds; the fields above D leave
        fields, distinct = torch.unique(self.table.rows()[0], return_counts=True)
        over = fields[distinct > self.max_distinct]
        if over.numel():
            self.skip.fold(over, torch.zeros_like(over), winners=False)
            self.unbounded.update(over.cpu().tolist())
            self.table.purge(over)
        win = self.table.winners(field, value, g)
        if win.numel():
            # the lines that became a value's first: their bytes are its example, their signature its template
            f, v, at, s = torch.stack([field[win], value[win], g[win], sig[line[win].long()]]).cpu().tolist()
            self.example_lines += len(f)
            self.example_fields.extend(f)
            keys = [var_cell_key(a & U64, b & U64) for a, b in zip(f, v)]
            self._examples.put_all(keys, at, zip(s, piece.raw_lines(line[win])))

    # ------------------------------------------------------------------ the report
    def report(self, top: Optional[int] = 20, order: str = "odd", min_count: int = 5, min_fill: float = 0.9,
               varying: bool = True, show: int = 5) -> dict:
        """The report of everything added so far (more can be added afterwards)."""
        check_args(self.max_distinct, order, min_count, min_fill, show)
        with self._guard():
            return self._report(top, order, min_count, min_fill, varying, show)

    def _report(self, top: Optional[int], order: str, min_count: int, min_fill: float, varying: bool, show: int) -> dict:
        D = self.max_distinct
        out = variants_head(self.next_line - self.line_base, self.field_lines, self.tokens, 0, len(self.unbounded),
                            len(self.unbounded), D)
        if out["totalLines"] == 0:
            return out
        t_sig, t_lines, _, _ = self.by_template.rows()
        out["templates"] = int(t_sig.numel())
        if self.tokens == 0:
            return out
        per_sig = dict(zip(*torch.stack([t_sig, t_lines]).cpu().tolist()))
        by_field: Dict[int, list] = {}
        for f, v, c, first, last in zip(*torch.stack(self.table.rows()).cpu().tolist()):
            by_field.setdefault(f, []).append((c, first, last, v & U64))
        out["fields"] += len(by_field)
        groups = []
        for f, vals in by_field.items():
            if f in self.unbounded or len(vals) > D:
                raise RuntimeError("VariantAccumulator: the table holds %d values of the field %016x (unbounded: %s)"
                                   % (len(vals), f & U64, f in self.unbounded))
            # the key says neither template nor field: the template is the one the kernel gave the example
            # line of the field's first value, the field the one whose key this is (variants_row recomputes
            # both from the bytes of every line it lists)
            c0, first, _, v0 = min(vals, key=lambda x: x[1])
            signed, _ = self._examples.take(var_cell_key(f & U64, v0), first)
            sig = signed & U64
            j = next((j for j in range(VAL_PER_LINE) if val_key(sig, j) == f & U64), None)
            if j is None or signed not in per_sig:
                raise RuntimeError("VariantAccumulator: line %d does not hold the field of the key %016x"
                                   % (first + 1, f & U64))
            lines, count = per_sig[signed], sum(x[0] for x in vals)
            if not 0 < count <= lines or any(x[0] < 1 or x[1] > x[2] for x in vals):
                raise RuntimeError("VariantAccumulator: %016x has %d tokens on %d lines, or a value that ends "
                                   "before it begins" % (f & U64, count, lines))
            if count >= min_count and count >= min_fill * lines and (not varying or len(vals) > 1):
                odd = count - max(x[0] for x in vals)
                groups.append((variants_order_key(order, sig, j, count, odd, len(vals), first), f, sig, j, lines, vals))
        groups.sort(key=lambda x: x[0])
        if top is not None:
            groups = groups[:max(0, int(top))]
        for _, f, sig, j, lines, vals in groups:
            # only the listed values need their lines; the first value's line is the group's example
            need = variants_listed(vals, show)
            first = min(vals, key=lambda x: x[1])
            if first not in need:
                need = need + [first]
            raws = {x[3]: self._examples.take(var_cell_key(f & U64, x[3]), x[1])[1] for x in need}
            try:
                out["top"].append(variants_row(sig, j, lines, [x + (raws.get(x[3]),) for x in vals], show))
            except ValueError as e:
                raise RuntimeError("VariantAccumulator: %s" % e) from None
        return out


def variants_document(eng: Engine, data: bytes, max_distinct: int = 64, top: Optional[int] = 20, order: str = "odd",
                      min_count: int = 5, min_fill: float = 0.9, varying: bool = True, show: int = 5) -> dict:
    """The report of one document (``Engine.variants_bytes``)."""
    check_args(max_distinct, order, min_count, min_fill, show)
    acc = VariantAccumulator(eng, max_distinct)
    acc.add_document(data)
    return acc._report(top, order, min_count, min_fill, varying, show)


def variants_stream(eng: Engine, src, chunk_bytes: Optional[int] = None, max_distinct: int = 64,
                    top: Optional[int] = 20, order: str = "odd", min_count: int = 5, min_fill: float = 0.9,
                    varying: bool = True, show: int = 5) -> dict:
    """The report of ONE log in chunks: a bytes-like source (bytes, mmap, ``RepeatBuffer``) or a
    ``ResidentLog``. Exactly the one-document report, whatever the chunk size."""
    check_args(max_distinct, order, min_count, min_fill, show)
    acc = VariantAccumulator(eng, max_distinct)
    acc.add_stream(src, chunk_bytes)
    return acc._report(top, order, min_count, min_fill, varying, show)
