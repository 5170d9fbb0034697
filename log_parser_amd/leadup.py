"""Lead-up report: what does a log say just before its failures that it does not usually say?
(``golden.leadup`` is the specification.)

A line is *in the lead-up* when an event lies on one of the ``window`` lines after it.
:class:`LeadupAccumulator` walks ONE log in pieces (pieces.py; the matchers run, because the events
say where the failures are) and keeps two ``GapTable`` s: ``total`` groups every line by template
signature, ``before`` groups the lead-up lines. One text kernel, k_lead_sig
(csrc/kernels/leadup.hip), signs every line of a piece, marks the lead-up against the piece's own
event lines and compacts the lead-up lines as (line, signature) pairs.

An event of the NEXT piece puts the tail of this one into its lead-up, so the last ``window``
lines of a piece that no event of the piece itself reaches stay *pending* -- global line,
signature and raw bytes, at most ``window`` entries -- until a later piece either brings an event
near enough (they are folded into ``before``, with their own line as the ordinal) or shows that
none can come any more (they are dropped). A piece can be shorter than the window, so an entry may
stay pending over several pieces. With this carry the report of a stream is the one-document
report for every chunk size. Nothing is scored and the frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional

import torch

from .accumulator import U64, Accumulator, Examples
from .engine import Engine
from .golden import LEAD_MAX_WINDOW, line_template
from .ops import kernels as K
from .pieces import Piece, document_piece


def check_args(window: int, order: str = "share", min_count: int = 2) -> None:
    if order not in ("share", "count", "first"):
        raise ValueError("order must be 'share', 'count' or 'first'")
    if not 1 <= window <= LEAD_MAX_WINDOW:
        raise ValueError("window must be 1..%d" % LEAD_MAX_WINDOW)
    if min_count < 1:
        raise ValueError("min_count must be at least 1")


class LeadupAccumulator(Accumulator):
    """The lead-up report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log: the lines still pending at the end of one source can fall into the lead-up of an
    event of the next, and ``report`` counts only what is settled.

    Only the lines that become their group's first lead-up line come to the host, as its example,
    and the at most ``window`` pending lines of every piece."""

    def __init__(self, engine: Engine, window: int = 50, guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.leadup_accumulator``)."""
        check_args(window)
        super().__init__(engine, guard)
        self.window = int(window)
        self.total = K.GapTable(engine.device)          # every line
        self.before = K.GapTable(engine.device)         # ... of the lead-up
        self.lines = self.events = self.event_lines = self.lead = 0
        self._examples = Examples("LeadupAccumulator")  # signature -> (global line, raw line)
        self._pending: List[tuple] = []                 # (global line, signature, raw), ascending

    def _add_pieces(self, pieces: Iterable[Piece], carry: bool = True) -> None:
        for piece in pieces:
            self._add_piece(piece, carry)

    def _add_piece(self, piece: Piece, carry: bool = True) -> None:
        """``carry=False``: no piece follows this one, ever (``leadup_document``) -- nothing is
        fetched for a pending list nobody will read."""
        n, base, W = piece.ls.numel(), piece.line_base, self.window
        dev = piece.text.device
        self.lines += n
        self.events += piece.ev_line.numel()
        if n == 0:
            return
        ev = torch.unique(piece.ev_line)                # sorted, distinct
        ne = ev.numel()
        self.event_lines += ne
        sig, lead, line, pair_sig, n_lead = K.lead_lines(piece.text, piece.ls, piece.ll, ev if ne else None, W)
        self.total.fold(sig, torch.arange(base, base + n, dtype=torch.int64, device=dev), winners=False)
        # the pending lines of the earlier pieces: in the lead-up of this piece's first event, or not at all
        came: List[tuple] = []
        if self._pending:
            if ne:
                first = base + int(ev[0])
                came = [h for h in self._pending if first - h[0] <= W]
                self._pending = []
            else:
                self._pending = [h for h in self._pending if h[0] + W >= base + n]
        self.lead += n_lead + len(came)
        ordinal = line.long() + base
        if came:
            ordinal = torch.cat([ordinal, torch.tensor([h[0] for h in came], dtype=torch.int64, device=dev)])
            pair_sig = torch.cat([pair_sig, torch.tensor([h[1] for h in came], dtype=torch.int64, device=dev)])
        if ordinal.numel():
            win = self.before.fold(pair_sig, ordinal)
            mine = win[win < n_lead]
            if mine.numel():
                self._examples.record(pair_sig, ordinal, mine, piece.raw_lines(line[mine]))
            for w in (win[win >= n_lead].tolist() if came else ()):     # their carried bytes are the example
                g, s, raw = came[w - n_lead]
                self._examples.put(s, g, raw)
        if not carry:
            return
        # the tail that no event of this piece reaches: a later piece's event may
        lo = max(0, n - W)
        x = torch.nonzero(lead[lo:] == 0).flatten() + lo
        if x.numel():
            sigs = sig[x].tolist()
            self._pending += [(base + a, s, raw) for a, s, raw in zip(x.tolist(), sigs, piece.raw_lines(x))]

    # ------------------------------------------------------------------ the report
    def report(self, top: Optional[int] = 20, order: str = "share", min_count: int = 2) -> dict:
        """The report of everything added so far (more can be added afterwards). Lines still
        pending are in no event's lead-up yet and count as such."""
        check_args(self.window, order, min_count)
        with self._guard():
            return self._report(top, order, min_count)

    def _report(self, top: Optional[int], order: str, min_count: int) -> dict:
        out = {"totalLines": self.lines, "events": self.events, "eventLines": self.event_lines, "window": self.window,
               "leadLines": self.lead, "templates": 0, "top": []}
        sig, count, first, _ = self.before.rows()
        out["templates"] = int(sig.numel())
        if sig.numel() == 0:
            return out
        total = self.total.lookup(sig)[0]
        keep = count >= min_count
        sig, count, first, total = sig[keep], count[keep], first[keep], total[keep]
        pick = torch.sort(first, stable=True)[1]                    # by first line (distinct per group)
        if order != "first":                                        # by (-count, first line)
            pick = pick[torch.sort(count[pick], descending=True, stable=True)[1]]
        if order == "share":                                        # by (-count / total, -count, first line)
            share = count[pick].double() / total[pick].double()
            pick = pick[torch.sort(share, descending=True, stable=True)[1]]
        if top is not None:
            pick = pick[:max(0, int(top))]
        rows = torch.stack([count[pick], total[pick], first[pick], sig[pick]]).cpu().tolist()
        for c, t, f, s in zip(*rows):
            raw = self._examples.take(s, f)
            if not 0 < c <= t:
                raise RuntimeError("LeadupAccumulator: %016x has %d lead-up lines of %d" % (s & U64, c, t))
            out["top"].append({"count": c, "total": t, "share": c / t, "lift": (c * self.lines) / (t * self.lead),
                               "firstLine": f + 1, "signature": "%016x" % (s & U64),
                               "template": line_template(raw).decode("utf-8", errors="replace"),
                               "example": raw.decode("utf-8", errors="replace")})
        return out


def leadup_document(eng: Engine, text, n: int, data: bytes, window: int = 50, top: Optional[int] = 20,
                    order: str = "share", min_count: int = 2) -> dict:
    """The report of a staged document in one piece (``Engine.leadup_document``)."""
    check_args(window, order, min_count)
    acc = LeadupAccumulator(eng, window)
    acc._add_pieces([document_piece(eng, text, n, data)], carry=False)
    return acc._report(top, order, min_count)
