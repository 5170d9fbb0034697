"""Trace report: which stack traces does a log hold, how often, where first, with which root cause,
and does any pattern explain them? (``golden.traces`` is the specification.)

The other reports treat a log as independent lines; this one reads its multi-line structure. A
*run* is a maximal sequence of consecutive frame / ``... n more`` / ``Caused by:`` lines, a *trace*
a run with a frame, its *head* the line just before it. :class:`TraceAccumulator` walks ONE log in
pieces (pieces.py; the matchers run, because the report says which traces an event lies on):
``K.trace_runs`` classifies the lines and scans the runs (csrc/kernels/traces.hip) and returns one
row per trace, and the rows are folded into a device-resident ``GapTable`` by signature with the
global start line as the ordinal. The rows with an event go into a second table that is joined at
report time. Only the traces that become a group's first occurrence bring lines to the host: head,
top frame and last cause.

A trace can straddle pieces: the open run's aggregate and whether an event lies on the previous
piece's last line (it may be the next run's head) are carried from piece to piece, so the report of
a stream is the one-document report for every chunk size. The text of a piece is gone when the
next one comes, so the (at most three) lines of an open run that a later first occurrence would
need are read before that. A source (``add_document``, ``add_stream``) ends its open run; the
next source continues the line numbers. Nothing is scored and the frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional

import torch

from .accumulator import U64, Accumulator, Examples
from .engine import Engine
from .golden import _TR_EXC
from .novelty import check_order
from .ops import kernels as K
from .pieces import Piece, document_piece


def _text(raw: Optional[bytes], strip: bool = False) -> Optional[str]:
    if raw is None:
        return None
    return (raw.strip(b" \t") if strip else raw).decode("utf-8", errors="replace")


class TraceAccumulator(Accumulator):
    """The trace report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log's line numbers; a trace does not continue across sources."""

    def __init__(self, engine: Engine, guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.traces_stream``)."""
        super().__init__(engine, guard)
        self.table = K.GapTable(engine.device)          # every trace, by signature
        self.ev_table = K.GapTable(engine.device)       # ... that an event lies on
        self.lines = self.events = 0
        # traces, trace lines (heads included), frame lines, traces with an event: summed on the device
        self._sums = torch.zeros(4, dtype=torch.int64, device=engine.device)
        self._carry = K.TR_CARRY_START
        # the lines of the open run read so far, and the last line of the previous piece (a head?)
        self._open: Dict[str, Optional[bytes]] = {"head": None, "top": None, "cause": None}
        self._prev_last: Optional[bytes] = None
        self._examples = Examples("TraceAccumulator")          # signature -> (global start line, first trace)

    def _add_pieces(self, pieces: Iterable[Piece]) -> None:
        last = True
        for piece in pieces:
            self._add_piece(piece)
            last = piece.last
        if not last:                                    # (a source whose last piece does not say so)
            self._end_source()

    def _end_source(self) -> None:
        cols, _, self._carry = K.trace_runs(torch.empty(0, dtype=torch.uint8, device=self.engine.device),
                                            torch.empty(0, dtype=torch.int64, device=self.engine.device),
                                            torch.empty(0, dtype=torch.int32, device=self.engine.device),
                                            None, self._carry, True)
        self._fold(cols, None, self.lines)
        self._open = {"head": None, "top": None, "cause": None}
        self._prev_last = None

    def _add_piece(self, piece: Piece) -> None:
        n, ne = piece.ls.numel(), piece.ev_line.numel()
        self.events += ne
        if n == 0:
            if piece.last:
                self._end_source()
            return
        ev_mask = None
        if ne:
            ev_mask = torch.zeros(n, dtype=torch.uint8, device=piece.text.device)
            ev_mask[piece.ev_line.long()] = 1
        cols, _, carry = K.trace_runs(piece.text, piece.ls, piece.ll, ev_mask, self._carry, piece.last)
        self._fold(cols, piece, piece.line_base)
        self.lines += n
        self._carry = carry
        self._keep_lines(piece, carry)

    def _fold(self, cols: torch.Tensor, piece: Optional[Piece], line_base: int) -> None:
        if cols.shape[1] == 0:
            return
        start, sig, lines, frames, flags = (cols[c] for c in
                                            (K.TR_START, K.TR_SIG, K.TR_LINES, K.TR_FRAMES, K.TR_FLAGS))
        ev = (flags & K.TR_ROW_EVENT) != 0
        headed = (flags & K.TR_ROW_HEADLESS) == 0
        self._sums += torch.stack([lines.new_tensor(lines.numel()), (lines + headed).sum(), frames.sum(), ev.sum()])
        ordinal = start + line_base
        win = self.table.fold(sig.contiguous(), ordinal)
        if win.numel():
            self._examples.record(sig, ordinal, win, self._first_traces(cols[:, win], piece))
        if self.events:
            self.ev_table.fold(sig[ev], ordinal[ev], winners=False)     # (no pair: nothing is launched)

    def _first_traces(self, cols: torch.Tensor, piece: Optional[Piece]) -> List[tuple]:
        """(lines with the head, frames, causes, headless, head, top frame, last cause line) of the
        rows ``cols``: the lines that lie in ``piece`` are read in one go, those of earlier pieces
        are the ones kept for the open run."""
        rows = cols.t().cpu().tolist()
        want: List[int] = []                            # piece lines to read

        def ask(i: int) -> int:
            want.append(i)
            return len(want) - 1

        plan = []
        for start, _, lines, frames, causes, flags, ff, lc in rows:
            headless = bool(flags & K.TR_ROW_HEADLESS)
            head = (None if headless else ("open", "head") if start < 0 else ("prev",) if start == 0
                    else ("line", ask(start - 1)))
            top = ("open", "top") if ff < 0 else ("line", ask(ff))
            cause = None if lc == K.TR_NO_CAUSE else ("open", "cause") if lc < 0 else ("line", ask(lc))
            plan.append((lines + (not headless), frames, causes, headless, head, top, cause))
        raws = piece.raw_lines(torch.tensor(want, dtype=torch.int64, device=piece.ls.device)) if want else []

        def get(ref) -> Optional[bytes]:
            if ref is None:
                return None
            return raws[ref[1]] if ref[0] == "line" else self._prev_last if ref[0] == "prev" else self._open[ref[1]]

        return [(n, f, c, h, get(head), get(top), get(cause)) for n, f, c, h, head, top, cause in plan]

    def _keep_lines(self, piece: Piece, carry) -> None:
        """Before the piece's text goes away: the head, top frame and last cause line of the run it
        leaves open, or its last line (the head of a run that begins the next piece)."""
        if piece.last:
            self._open = {"head": None, "top": None, "cause": None}
            self._prev_last = None
            return
        L = piece.ls.numel()
        if not carry[K.TRC_OPEN]:
            self._prev_last = piece.raw_lines(torch.tensor([L - 1], dtype=torch.int64, device=piece.ls.device))[0]
            return
        # (line numbers of a carry count from the next piece's first line)
        s, ff, lc = carry[K.TRC_START] + L, carry[K.TRC_FF], carry[K.TRC_LC]
        want: Dict[str, int] = {}
        if s > 0:
            want["head"] = s - 1
        elif s == 0:
            self._open["head"] = None if carry[K.TRC_HEADLESS] else self._prev_last
        if s >= 0:                                      # the run began in this piece: nothing of an earlier one
            self._open["top"] = self._open["cause"] = None
        if carry[K.TRC_FRAMES] > 0 and ff + L >= 0:
            want["top"] = ff + L
        if lc != K.TR_NO_CAUSE and lc + L >= 0:
            want["cause"] = lc + L
        if want:
            raws = piece.raw_lines(torch.tensor(list(want.values()), dtype=torch.int64, device=piece.ls.device))
            self._open.update(zip(want.keys(), raws))
        self._prev_last = None                          # (the last line is a run line: no head)

    # ------------------------------------------------------------------ the report
    def report(self, top: Optional[int] = 20, order: str = "count", unexplained_only: bool = False) -> dict:
        """The report of everything added so far (more can be added afterwards)."""
        check_order(order)
        with self._guard():
            return self._report(top, order, unexplained_only)

    def _report(self, top: Optional[int], order: str, unexplained_only: bool) -> dict:
        n_traces, n_lines, n_frames, n_ev = self._sums.tolist()
        out = {"totalLines": self.lines, "events": self.events, "traces": n_traces, "traceLines": n_lines,
               "frameLines": n_frames, "groups": 0, "unexplainedTraces": n_traces - n_ev, "unexplainedGroups": 0,
               "top": []}
        sig, count, first, _ = self.table.rows()
        out["groups"] = int(sig.numel())
        if sig.numel() == 0:
            return out
        evs, _, _, ev_groups = self.ev_table.lookup(sig)
        out["unexplainedGroups"] = out["groups"] - ev_groups
        if unexplained_only:
            keep = evs == 0
            sig, count, first, evs = sig[keep], count[keep], first[keep], evs[keep]
        pick = torch.sort(first, stable=True)[1]                    # by start line (distinct per trace)
        if order == "count":                                        # by (-count, first line)
            pick = pick[torch.sort(count[pick], descending=True, stable=True)[1]]
        if top is not None:
            pick = pick[:max(0, int(top))]
        rows = torch.stack([count[pick], evs[pick], first[pick], sig[pick]]).cpu().tolist()
        for c, cv, f, s in zip(*rows):
            n, frames, causes, headless, head, top_frame, cause = self._examples.take(s, f)
            exc = _TR_EXC.search(head) if head is not None else None
            out["top"].append({"count": c, "eventTraces": cv, "firstLine": f + 1 if headless else f,
                               "signature": "%016x" % (s & U64), "lines": n, "frames": frames, "causes": causes,
                               "head": _text(head), "exception": _text(exc.group()) if exc else None,
                               "topFrame": _text(top_frame, strip=True), "rootCause": _text(cause, strip=True)})
        return out


def traces_document(eng: Engine, text, n: int, data: bytes, top: Optional[int] = 20, order: str = "count",
                    unexplained_only: bool = False) -> dict:
    """The report of a staged document in one piece (``Engine.traces_document``)."""
    check_order(order)
    acc = TraceAccumulator(eng)
    acc._add_pieces([document_piece(eng, text, n, data)])
    return acc._report(top, order, unexplained_only)
