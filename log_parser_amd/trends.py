"""Trends report: which line templates of a log started, stopped or surged over its time?
(``golden.trends`` is the specification.)

No baseline and no pattern: the log's own earlier part is the baseline. A *cell* is (template
signature, time bucket) with the number of lines in it; a pivot bucket splits the span of the log,
and a template is judged by its dated lines before and from the pivot on.

:class:`TrendAccumulator` walks ONE log in pieces without events (the walk without the matchers
of ``accumulator.LineAccumulator``). Per run:

* ``K.line_stamps`` (k_line_stamps, csrc/kernels/trends.hip): signature and stamp of every line from
  one visit of the line;
* ``K.timeline_fill``: unstamped lines take the time of the nearest earlier stamped line. The
  effective time of the last line so far is the only carry between runs;
* ``CellTable.fold`` (k_cell_fold): the lines into the device-resident cell table; bucket and key
  are computed in registers;
* a ``GapTable`` fold of (signature, global line) with winners: the lines that became their
  template's first come to the host as its example -- one per NEW template in steady state.

``report`` reduces the cells to per-template rows with torch on the table's device (sort by
(signature, bucket), segment sums, the peak); only those rows reach the host, where kinds, filters
and order are exact Python arithmetic (``golden.trends_kind`` / ``trends_order_key`` /
``trends_row``). The report is the one-document report at every chunk size. Nothing is scored and
the frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from .accumulator import U64, Examples, LineAccumulator
from .engine import Engine
from .golden import TREND_UNDATED, iso_ms, timeline_span_error
from .golden import trends_check_args as check_args
from .golden import (trends_head, trends_kind, trends_lift, trends_listed, trends_named_pivot, trends_order_key,
                     trends_pivot, trends_row)
from .ops import kernels as K
from .pieces import Piece

NAMED_PIVOTS = ("first-event", "first-error")


def _segment_sum(x: torch.Tensor, start: torch.Tensor, end: torch.Tensor) -> torch.Tensor:
    """Sums of x[start[t] : end[t]] (exact: int64 prefix sums)."""
    c = torch.cat([x.new_zeros(1), x.cumsum(0)])
    return c[end] - c[start]


class TrendAccumulator(LineAccumulator):
    """The trends report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log: their first line follows the lines so far. The bucket width is fixed when the
    accumulator is made: the cells are counted as the lines arrive."""

    def __init__(self, engine: Engine, bucket_seconds: int = 60, guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.trend_accumulator``)."""
        self.W = check_args(bucket_seconds)[0]
        self.bucket_seconds = int(bucket_seconds)
        super().__init__(engine, guard)
        dev = engine.device
        self.cells = K.CellTable(dev)
        self.by_template = K.GapTable(dev)      # (signature, g): lines per template, its first line
        self.next_line = 0
        self.carry_eff = K.TS_NONE              # effective time of the last line so far
        self._examples = Examples("TrendAccumulator")         # signature (signed) -> (first line, its bytes)

    def _add_piece(self, piece: Piece) -> None:
        text, ls, ll = piece.text, piece.ls, piece.ll
        n, base = ls.numel(), self.next_line
        if n == 0:
            return
        self.next_line = base + n
        sig, ts = K.line_stamps(text, ls.contiguous(), ll.contiguous())
        eff, _ = K.timeline_fill(ts, self.carry_eff)
        self.cells.fold(sig, eff, base, self.W)
        g = torch.arange(base, base + n, dtype=torch.int64, device=text.device)
        win = self.by_template.fold(sig, g)
        # one read for the carry and the winners' signatures
        tail = torch.cat([eff[-1:], sig[win]]).cpu().tolist()
        self.carry_eff = tail[0]
        if win.numel():
            self._examples.put_all(tail[1:], (win + base).cpu().tolist(), piece.raw_lines(win))

    # ------------------------------------------------------------------ the report
    def report(self, at=None, ratio: int = 4, min_count: int = 5, kind: Optional[str] = None, order: str = "change",
               top: Optional[int] = 20, max_buckets: int = 65536, timeline: Optional[Callable[[], dict]] = None) -> dict:
        """The report of everything added so far (more can be added afterwards). ``at``: None, epoch
        milliseconds, a timestamp, or ``"first-event"`` / ``"first-error"`` -- these two need
        ``timeline``, which returns the timeline report of the same log and bucket width; it is
        called, outside the guard, only when the log has a dated line."""
        _, source, at_ms = check_args(self.bucket_seconds, at, ratio, min_count, kind, order, max_buckets)
        if source in NAMED_PIVOTS:
            if timeline is None:
                raise ValueError("trends: the pivot %r needs the log's timeline: use LogParser.trends, or pass "
                                 "`timeline`" % source)
            if self.carry_eff != K.TS_NONE:     # (the last line has an effective time: some line is dated)
                at_ms = trends_named_pivot(source, timeline())
        with self._guard():
            return self._report(source, at_ms, ratio, min_count, kind, order, top, max_buckets)

    def _report(self, source: str, at_ms: Optional[int], ratio: int, min_count: int, kind: Optional[str], order: str,
                top: Optional[int], max_buckets: int) -> dict:
        W = self.W
        total = self.next_line
        if total == 0:
            return trends_head(0, 0, 0, 0, self.bucket_seconds)
        sig, bucket, count, first = self.cells.rows()
        # by (signature, bucket): two stable sorts; a template's undated cell (the smallest bucket value) leads
        o = torch.sort(bucket, stable=True)[1]
        o = o[torch.sort(sig[o], stable=True)[1]]
        sig, bucket, count, first = sig[o], bucket[o], count[o], first[o]
        dated = bucket != TREND_UNDATED
        dcount = torch.where(dated, count, 0)
        n_dated, b0, b1 = torch.stack([dcount.sum(), torch.where(dated, bucket, K.I64_MAX).min(),
                                       torch.where(dated, bucket, -K.I64_MAX).max()]).tolist()
        t_sig, t_len = torch.unique_consecutive(sig, return_counts=True)
        T = int(t_sig.numel())
        out = trends_head(total, n_dated, T, int(sig.numel()), self.bucket_seconds)
        if T != self.by_template.used:
            raise RuntimeError("TrendAccumulator: the cells hold %d templates, the template table %d"
                               % (T, self.by_template.used))
        if n_dated == 0:
            return out
        if b1 - b0 + 1 > max_buckets:
            raise timeline_span_error(b0 * W, b1 * W, W, max_buckets)
        out.update({"firstBucket": iso_ms(b0 * W), "lastBucket": iso_ms(b1 * W), "buckets": b1 - b0 + 1})
        p = trends_pivot(source, at_ms, b0, b1, W)
        if p is None:
            return out
        nb_before, nb_after = p - b0, b1 - p + 1
        out.update({"pivot": iso_ms(p * W), "pivotSource": source, "bucketsBefore": nb_before, "bucketsAfter": nb_after})
        # per template, on the table's device: the segments of the sorted cells
        end = t_len.cumsum(0)
        start = end - t_len
        seg = torch.repeat_interleave(torch.arange(T, device=sig.device), t_len)
        lines = _segment_sum(count, start, end)
        n = _segment_sum(dcount, start, end)
        before = _segment_sum(torch.where(bucket < p, dcount, 0), start, end)
        lead = start + (~dated[start]).long()                 # the template's first dated cell, if it has one
        peak = torch.zeros(T, dtype=torch.int64, device=sig.device).scatter_reduce_(0, seg, dcount, "amax", include_self=True)
        at_peak = dated & (dcount == peak[seg])
        peak_bucket = torch.full((T,), K.I64_MAX, dtype=torch.int64, device=sig.device).scatter_reduce_(
            0, seg, torch.where(at_peak, bucket, K.I64_MAX), "amin", include_self=True)
        first_line = torch.full((T,), K.I64_MAX, dtype=torch.int64, device=sig.device).scatter_reduce_(
            0, seg, first, "amin", include_self=True)
        cols = torch.stack([t_sig, lines, n, before, bucket[lead.clamp(max=sig.numel() - 1)], bucket[end - 1],
                            end - lead, peak_bucket, peak, first_line])
        keep = n >= min_count                                 # (the kinds count these; the others are not listed either)
        listed = []
        for s, c_lines, c_n, c_before, fb, lb, active, pb, pc, fl in zip(*cols[:, keep].cpu().tolist()):
            k = trends_kind(c_before, c_n - c_before, nb_before, nb_after, ratio)
            out["kinds"][k] += 1
            if not trends_listed(kind, k):
                continue
            lift = trends_lift(c_before, c_n - c_before, nb_before, nb_after)
            listed.append((trends_order_key(order, lift, c_n, fl),
                           (s, c_lines, c_n, c_before, c_n - c_before, fb, lb, active, pb, pc, fl, k, lift)))
        listed.sort(key=lambda kv: kv[0])
        if top is not None:
            listed = listed[:max(0, int(top))]
        for _, (s, c_lines, c_n, c_before, c_after, fb, lb, active, pb, pc, fl, k, lift) in listed:
            raw = self._examples.take(s, fl)
            out["top"].append(trends_row(s & U64, c_lines, c_n, c_before, c_after, fb, lb, active, pb, pc, fl, raw, W,
                                         k, lift))
        return out


def trends_document(eng: Engine, data: bytes, bucket_seconds: int = 60, at=None, ratio: int = 4, min_count: int = 5,
                    kind: Optional[str] = None, order: str = "change", top: Optional[int] = 20,
                    max_buckets: int = 65536) -> dict:
    """The report of one document (``Engine.trends_bytes``); a named pivot comes from the
    document's timeline report, a second walk with the matchers."""
    data = bytes(data)
    check_args(bucket_seconds, at, ratio, min_count, kind, order, max_buckets)
    acc = TrendAccumulator(eng, bucket_seconds)
    acc.add_document(data)
    return acc.report(at, ratio, min_count, kind, order, top, max_buckets,
                      timeline=lambda: eng.timeline_bytes(data, bucket_seconds=bucket_seconds, max_buckets=max_buckets))


def trends_stream(eng: Engine, src, chunk_bytes: Optional[int] = None, bucket_seconds: int = 60, at=None,
                  ratio: int = 4, min_count: int = 5, kind: Optional[str] = None, order: str = "change",
                  top: Optional[int] = 20, max_buckets: int = 65536) -> dict:
    """The report of ONE log in chunks: a bytes-like source (bytes, mmap, ``RepeatBuffer``) or a
    ``ResidentLog``. Exactly the one-document report, whatever the chunk size. A named pivot comes
    from the timeline of the same source: a second walk, with the matchers."""
    from .timeline import TimelineAccumulator
    check_args(bucket_seconds, at, ratio, min_count, kind, order, max_buckets)
    acc = TrendAccumulator(eng, bucket_seconds)
    acc.add_stream(src, chunk_bytes)

    def timeline() -> dict:
        tl = TimelineAccumulator(eng, bucket_seconds, max_buckets)
        tl.add_stream(src, chunk_bytes)
        return tl.report()

    return acc.report(at, ratio, min_count, kind, order, top, max_buckets, timeline=timeline)
