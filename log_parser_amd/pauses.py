"""Pauses report: where did a log go silent, and after which line templates? (``golden.pauses`` is
the specification.)

The stamped lines of a log in line order are ``i_0 < i_1 < ...``; the *step* k is the stamp of
``i_k`` minus the stamp of ``i_{k-1}`` (its from-line and its to-line). A step below 0 runs
backwards and is only counted, a step ``>= min_ms`` is a *pause*.

:class:`PauseAccumulator` walks ONE log in pieces without events (the walk without the matchers
of ``accumulator.LineAccumulator``). Per run:

* ``K.line_stamps``: signature and stamp of every line from one visit of the line;
* ``K.pause_scan`` (k_ps_tiles / k_ps_prefix / k_ps_emit, csrc/kernels/pauses.hip): the pauses as
  rows (to-line, from-line, ms, the two signatures) in line order, the interval histogram and the
  head's statistics added to device tensors. Stamp, line and signature of the last stamped line so
  far are the carry between runs; they and the row count are the run's one small read;
* a ``GapTable`` fold of (signature, global line): the lines per template;
* the rows grouped by the key line's signature with torch on their device (``unique`` +
  ``index_add_`` / ``scatter_reduce_``: count, total, max, the to-line of the max, the first
  to-line), merged into running tensors sorted by signature. Sums are exact int64, nothing is
  packed or clamped;
* the run's largest rows (a stable sort by ms: ties stay in line order), merged into the running
  ``longest`` list on the host.

Of the text only this reaches the host: the two lines of a row that enters ``longest``, the key
line of a template's first pause (its example), and the run's last stamped line -- it may turn out
to be the from-line of a pause in the next run. The report is the one-document report at every
chunk size. Nothing is scored and the frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

from .accumulator import U64, Examples, LineAccumulator
from .engine import Engine
from .golden import pauses_check_args as check_args
from .golden import pauses_head, pauses_longest_row, pauses_order_key, pauses_template_row
from .ops import kernels as K
from .pieces import Piece



def check_top(top, what: str = "top") -> Optional[int]:
    if top is None:
        return None
    if isinstance(top, bool) or not isinstance(top, int):
        raise ValueError("pauses: %s must be None or an integer" % what)
    return max(0, top)


def _group(key, count, total, peak, peak_line, first):
    """Rows (key, count, total ms, max ms, to-line of the max, first to-line) -> one row per
    distinct key, sorted by key: counts and totals added, the largest max with the smallest of its
    lines, the smallest first line."""
    uk, inv = torch.unique(key, return_inverse=True)
    n, dev = uk.numel(), key.device
    zeros = torch.zeros(n, dtype=torch.int64, device=dev)
    g_peak = zeros.clone().scatter_reduce_(0, inv, peak, "amax", include_self=False)
    big = torch.full((n,), K.I64_MAX, dtype=torch.int64, device=dev)
    at_peak = torch.where(peak == g_peak[inv], peak_line, K.I64_MAX)
    return (uk, zeros.clone().index_add_(0, inv, count), zeros.clone().index_add_(0, inv, total), g_peak,
            big.clone().scatter_reduce_(0, inv, at_peak, "amin", include_self=True),
            big.clone().scatter_reduce_(0, inv, first, "amin", include_self=True))


class PauseAccumulator(LineAccumulator):
    """The pauses report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log: their first line follows the lines so far. ``min_ms``, ``by`` and the length
    ``longest`` of the list of longest pauses (None: every pause) are fixed when the accumulator is
    made: the rows are folded as the lines arrive."""

    def __init__(self, engine: Engine, min_ms: int = 1000, by: str = "before", longest: Optional[int] = 20,
                 guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.pause_accumulator``)."""
        check_args(min_ms, by)
        self.min_ms, self.by, self.longest = min_ms, by, check_top(longest, "longest")
        super().__init__(engine, guard)
        dev = engine.device
        self.by_template = K.GapTable(dev)      # (signature, g): lines per template
        self.stats = K.pause_stats(dev)
        self.hist = torch.zeros(K.PS_BUCKETS, dtype=torch.int64, device=dev)
        self._groups = tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(6))   # sorted by signature
        self.next_line = 0
        self.pauses = 0
        self.carry: Optional[Tuple[int, int, int]] = None      # (stamp, line, signature) of the last stamped line
        self._carry_raw = b""                                   # its bytes
        self._longest: List[tuple] = []     # (-ms, to-line, from-line, from-stamp, before, after), sorted
        self._examples = Examples("PauseAccumulator")           # signature (signed) -> (first to-line, the key line)

    def _add_piece(self, piece: Piece) -> None:
        text, ls, ll = piece.text, piece.ls, piece.ll
        n, base = ls.numel(), self.next_line
        if n == 0:
            return
        self.next_line = base + n
        dev = text.device
        sig, ts = K.line_stamps(text, ls.contiguous(), ll.contiguous())
        self.by_template.fold(sig, torch.arange(base, base + n, dtype=torch.int64, device=dev), winners=False)
        old, old_raw = self.carry, self._carry_raw
        rows, _, _, self.carry = K.pause_scan(ts, sig, self.min_ms, base, old, self.stats, self.hist)
        to_line, from_line, ms, from_sig, to_sig = rows
        m = to_line.numel()
        self.pauses += m
        want: List[int] = []                    # global lines whose bytes this run needs
        if self.carry is not None and self.carry[1] >= base:
            want.append(self.carry[1])
        cand: List[tuple] = []
        fresh: List[tuple] = []
        if m:
            key, key_line = (from_sig, from_line) if self.by == "before" else (to_sig, to_line)
            # the run's largest rows: stable, so that equal pauses stay in line order
            k = m if self.longest is None else min(m, self.longest)
            o = torch.sort(ms, descending=True, stable=True)[1][:k]
            # its groups, merged into the running ones; a group that is new brings its example
            ones = torch.ones(m, dtype=torch.int64, device=dev)
            run = _group(key, ones, ms, ms, to_line, to_line)
            known = self._groups[0]
            is_new = torch.ones_like(run[0], dtype=torch.bool)
            if known.numel():
                at = torch.searchsorted(known, run[0]).clamp(max=known.numel() - 1)
                is_new = known[at] != run[0]
            # (rows are in line order: a group's first row of the run is the one with its first to-line)
            first_row = torch.searchsorted(to_line, run[5][is_new])
            self._groups = _group(*(torch.cat([a, b]) for a, b in zip(self._groups, run)))
            # one read: the candidates for `longest`, then the new groups (signature, to-line, key line)
            nk = int(o.numel())
            flat = torch.cat([ms[o], to_line[o], from_line[o], ts[to_line[o] - base], run[0][is_new],
                              to_line[first_row], key_line[first_row]]).cpu().tolist()
            full = self.longest is not None and len(self._longest) >= self.longest
            worst = self._longest[-1][:2] if full and self._longest else None
            for c_ms, c_to, c_from, to_ts in zip(flat[:nk], flat[nk:2 * nk], flat[2 * nk:3 * nk], flat[3 * nk:4 * nk]):
                if worst is None or (-c_ms, c_to) < worst:
                    cand.append((c_ms, c_to, c_from, to_ts - c_ms))
                    want += [c_to, c_from]
            g = (len(flat) - 4 * nk) // 3
            rest = flat[4 * nk:]
            fresh = list(zip(rest[:g], rest[g:2 * g], rest[2 * g:]))
            want += [x for _, _, x in fresh]
        here = sorted({x for x in want if x >= base})
        raw = dict(zip(here, piece.raw_lines(torch.tensor(here, dtype=torch.int64, device=dev) - base))) if here else {}
        if old is not None:
            raw[old[1]] = old_raw
        missing = [x for x in want if x not in raw]
        if missing:
            raise RuntimeError("PauseAccumulator: line %d is neither in this run nor the carried line" % (missing[0] + 1))
        if self.carry is not None and self.carry[1] >= base:
            self._carry_raw = raw[self.carry[1]]
        for s, first, x in fresh:
            self._examples.put(s, first, raw[x])      # (a new group: nothing is held for it yet)
        if cand:
            self._longest += [(-c_ms, c_to, c_from, from_ts, raw[c_from], raw[c_to]) for c_ms, c_to, c_from, from_ts in cand]
            self._longest.sort(key=lambda r: r[:2])
            if self.longest is not None:
                del self._longest[self.longest:]

    # ------------------------------------------------------------------ the report
    def report(self, order: str = "total", min_count: int = 1, top: Optional[int] = 20) -> dict:
        """The report of everything added so far (more can be added afterwards). ``top`` cuts both
        lists and is at most the accumulator's ``longest``."""
        check_args(self.min_ms, self.by, order, min_count)
        top = check_top(top)
        if self.longest is not None and (top is None or top > self.longest):
            raise ValueError("pauses: top=%r exceeds the %d longest pauses this accumulator keeps" % (top, self.longest))
        with self._guard():
            return self._report(order, min_count, top)

    def _report(self, order: str, min_count: int, top: Optional[int]) -> dict:
        stamped, backward, paused_ms, first, last = self.stats.tolist()
        out = pauses_head(self.next_line, stamped, backward, self.min_ms, self.pauses, paused_ms,
                          first if stamped else None, last if stamped else None, self.hist.tolist())
        if sum(c["count"] for c in out["intervals"]) != out["steps"] - backward:
            raise RuntimeError("PauseAccumulator: %d stamped lines, %d backward steps, but %d steps in the intervals"
                               % (stamped, backward, sum(c["count"] for c in out["intervals"])))
        if not self.pauses:
            return out
        cut = (lambda rows: rows) if top is None else (lambda rows: rows[:top])
        out["longest"] = [pauses_longest_row(-neg, c_from, c_to, from_ts, before, after, self.by)
                          for neg, c_to, c_from, from_ts, before, after in cut(self._longest)]
        key, count, total, peak, peak_line, first_line = self._groups
        if int(count.sum()) != self.pauses:
            raise RuntimeError("PauseAccumulator: the groups hold %d pauses of %d" % (int(count.sum()), self.pauses))
        # the lines of the groups' templates, looked up on the device
        t_lines, _, held, _ = self.by_template.lookup(key)
        if not bool(held.all()):
            raise RuntimeError("PauseAccumulator: a group's template is not among the log's templates")
        keep = count >= min_count
        cols = torch.stack([key, count, t_lines, total, peak, peak_line, first_line])[:, keep]
        listed = [(pauses_order_key(order, c, lines, tot, mx, fl), (s, c, lines, tot, mx, ml, fl))
                  for s, c, lines, tot, mx, ml, fl in zip(*cols.cpu().tolist())]
        listed.sort(key=lambda kv: kv[0])
        for _, (s, c, lines, tot, mx, ml, fl) in cut(listed):
            raw = self._examples.take(s, fl)
            out["templates"].append(pauses_template_row(s & U64, c, lines, tot, mx, ml, fl, raw))
        return out


def pauses_document(eng: Engine, data: bytes, min_ms: int = 1000, by: str = "before", order: str = "total",
                    min_count: int = 1, top: Optional[int] = 20) -> dict:
    """The report of one document (``Engine.pauses_bytes``)."""
    check_args(min_ms, by, order, min_count)
    acc = PauseAccumulator(eng, min_ms, by, check_top(top))
    acc.add_document(data)
    return acc.report(order, min_count, top)


def pauses_stream(eng: Engine, src, chunk_bytes: Optional[int] = None, min_ms: int = 1000, by: str = "before",
                  order: str = "total", min_count: int = 1, top: Optional[int] = 20) -> dict:
    """The report of ONE log in chunks: a bytes-like source (bytes, mmap, ``RepeatBuffer``) or a
    ``ResidentLog``. Exactly the one-document report, whatever the chunk size."""
    check_args(min_ms, by, order, min_count)
    acc = PauseAccumulator(eng, min_ms, by, check_top(top))
    acc.add_stream(src, chunk_bytes)
    return acc.report(order, min_count, top)
