"""Coverage-gap report: which error lines of a log does the library not explain, grouped by
shape? One document, a stream in chunks, a log resident in HBM, a corpus of documents
(``golden.gaps`` / ``golden.gaps_corpus`` are the specification).

A source is walked in pieces (pieces.py). Every line of a piece is classified by the context DFAs,
and the candidate lines outside every event (``cover="events"``) or every event's context window
(``"context"``) get a template signature (csrc/kernels/gaps.hip) -- all on the device.

:func:`gaps_document` (``Engine.gaps_document``) groups one document's (line, signature) pairs
with sorts, which a second piece or document cannot continue. :class:`GapAccumulator` folds the
pairs of every piece into a device-resident ``GapTable`` (csrc/kernels/gap_table.hip) instead: per
signature its count, its smallest *ordinal* ``(document << 40) | line`` and the number of documents
it occurs in. After each fold the kernel names the pairs that hold their group's smallest ordinal;
only those lines' text comes to the host, as the group's example.

A piece carries the events of its own lines only, so an event of a neighbouring piece can cover a
line of this one. Context windows are contiguous and at most ``lib.halo`` lines wide; two carries
make the result exact for every chunk size:

* forward: ``cov_until``, the largest global window end of any event of the earlier pieces -- an
  own candidate with global line ``g < cov_until`` is covered;
* backward: an uncovered candidate within ``max(lines_before)`` lines of its piece's end is held
  back (global line, signature, text). Once a later piece's events are known, held lines at or
  after that piece's smallest window start are dropped as covered; held lines no later event can
  reach (``g + max_before`` < the next piece's first line) are folded; the rest stay held -- a
  piece can be a single line -- and the last piece holds nothing back and folds what remains.

With ``cover="events"`` an event covers its own line only and both carries are empty.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional

import numpy as np
import torch

from .accumulator import Accumulator, Examples
from .engine import Engine
from .golden import line_template
from .ops import kernels as K
from .pieces import Piece, document_piece

ORD_SHIFT = 40                      # ordinal = (document << ORD_SHIFT) | line
ORD_LINE_MASK = (1 << ORD_SHIFT) - 1


def check_cover(cover: str) -> None:
    if cover not in ("events", "context"):
        raise ValueError("cover must be 'events' or 'context'")


def event_windows(tabs: dict, ev_line: torch.Tensor, ev_pat: torch.Tensor, cover: str):
    """(a, b) per event: the lines [a, b) it covers, in ``ev_line``'s numbering and unclamped -- its
    line (``cover="events"``) or its context window (csrc/kernels/post_core.h event_window)."""
    x = ev_line.long()
    if cover != "context":
        return x, x + 1
    p = ev_pat.long()
    before, after = tabs["ctx_before"][p].long(), tabs["ctx_after"][p].long()
    rules = before >= 0                     # -1: a pattern without context rules covers its line only
    return torch.where(rules, x - before, x), torch.where(rules, x + 1 + after, x + 1)


def coverage(a: torch.Tensor, b: torch.Tensor, L: int) -> Optional[torch.Tensor]:
    """uint8[L]: line is inside one of the windows [a, b) (clamped to the ``L`` lines) -- a
    difference array. None without windows."""
    if a.numel() == 0:
        return None
    a, b = a.clamp(min=0), b.clamp(max=L)
    one = torch.ones_like(a, dtype=torch.int32)
    diff = torch.zeros(L + 1, dtype=torch.int32, device=a.device)
    diff.scatter_add_(0, a, one)
    diff.scatter_add_(0, b, -one)
    return (diff[:L].cumsum(0) > 0).to(torch.uint8)


def gaps_document(eng: Engine, text, n: int, data: bytes, top: Optional[int] = 20, cover: str = "context") -> dict:
    """The report of a staged document in one piece (``Engine.gaps_document``): only the ``top``
    groups' numbers come back; the host renders template and example from its copy of the text."""
    check_cover(cover)
    piece = document_piece(eng, text, n, data)
    L = piece.ls.numel()
    out = {"totalLines": L, "events": int(piece.ev_line.numel()), "errorLines": 0, "uncoveredErrorLines": 0,
           "templates": 0, "top": []}
    feat = piece.features()
    cov = coverage(*event_windows(eng.tabs, piece.ev_line, piece.ev_pat, cover), L)
    # (capacity L: 12 bytes per line next to the text's ~100, and never a second run)
    line, sig, n_cand = K.gap_lines(text, piece.ls, piece.ll, feat, cov, L)
    out["errorLines"], out["uncoveredErrorLines"] = int(n_cand), int(line.numel())
    if line.numel() == 0:
        return out
    # groups: stable sort by line, then by signature -> runs of one signature in line order
    line, o = torch.sort(line.long(), stable=True)
    sig, o2 = torch.sort(sig[o], stable=True)
    line = line[o2]
    usig, counts = torch.unique_consecutive(sig, return_counts=True)
    first = line[counts.cumsum(0) - counts]                 # each group's head = its first line
    order = torch.sort(first, stable=True)[1]               # by (-count, first line)
    order = order[torch.sort(counts[order], descending=True, stable=True)[1]]
    out["templates"] = int(usig.numel())
    if top is not None:
        order = order[:max(0, int(top))]
    f = first[order]
    # (the rows and their lines' index in ONE read, so not ``piece.raw_lines``)
    rows = torch.stack([counts[order], f, usig[order], piece.ls[f], piece.ll[f].long()]).cpu().tolist()
    for c, x, s, a, m in zip(*rows):
        raw = data[a:a + m]
        out["top"].append({"count": c, "firstLine": x + 1, "signature": "%016x" % (s & 0xFFFFFFFFFFFFFFFF),
                           "template": line_template(raw).decode("utf-8", errors="replace"),
                           "example": raw.decode("utf-8", errors="replace")})
    return out


class GapAccumulator(Accumulator):
    """Folds documents (``add_document``), streams (``add_stream``) and resident logs
    (``add_resident``) into one report; ``report`` renders it. An accumulator that has seen exactly
    one document reports what ``Engine.gaps_bytes`` reports for it; any other number of documents
    gives the corpus report (``golden.gaps_corpus``). Nothing is scored and the frequency window is
    not touched."""

    def __init__(self, engine: Engine, cover: str = "context", guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.gap_accumulator``)."""
        check_cover(cover)
        super().__init__(engine, guard)
        self.cover = cover
        self.table = K.GapTable(engine.device)
        self.lines = self.events = self.error_lines = self.uncovered = self.documents = 0
        self._examples = Examples("GapAccumulator")     # signature -> (ordinal, raw line)
        before = engine.lib.ctx_before
        self._max_before = max(0, int(np.max(before))) if cover == "context" and len(before) else 0

    # ------------------------------------------------------------------ folding
    def _fold(self, doc: int, line: torch.Tensor, sig: torch.Tensor, fetch: Callable,
              held: Optional[List[tuple]] = None) -> None:
        """Fold the pairs (``line``: lines of document ``doc``, int64) and the released ``held``
        lines [(line, signature, raw)] in one launch; ``fetch(idx)`` returns the raw lines of the
        pairs ``idx``."""
        dev = self.engine.device
        n = line.numel()
        if held:
            line = torch.cat([line.long(), torch.tensor([h[0] for h in held], dtype=torch.int64, device=dev)])
            sig = torch.cat([sig, torch.tensor([h[1] for h in held], dtype=torch.int64, device=dev)])
        if line.numel() == 0:
            return
        self.uncovered += line.numel()
        ordinal = line.long() + (doc << ORD_SHIFT)
        win = self.table.fold(sig, ordinal, doc)
        if win.numel() == 0:
            return
        mine = win[win < n]
        if mine.numel():
            self._examples.record(sig, ordinal, mine, fetch(mine))
        if held:
            for w in win[win >= n].tolist():
                g, s, raw = held[w - n]
                self._examples.put(s, g + (doc << ORD_SHIFT), raw)

    def _new_document(self) -> int:
        doc = self.documents
        if doc >= (1 << 22):
            raise ValueError("GapAccumulator: too many documents for the ordinal")
        self.documents += 1
        return doc

    def _line_base(self) -> int:
        return 0                            # every source is a document of its own

    # ------------------------------------------------------------------ one document, piece by piece
    def _add_pieces(self, pieces: Iterable[Piece]) -> None:
        """Fold one document from its pieces. The ``last`` piece holds nothing back and releases
        everything held."""
        doc = self._new_document()
        cov_until = 0                       # forward carry
        held: List[tuple] = []              # backward carry: (global line, signature, raw), ascending
        for piece in pieces:
            cov_until, held = self._add_doc_piece(doc, piece, cov_until, held)

    def _add_doc_piece(self, doc: int, piece: Piece, cov_until: int, held: List[tuple]):
        """Fold one piece of document ``doc``: takes and returns the two carries."""
        n, base, mb = piece.ls.numel(), piece.line_base, self._max_before
        if base + n > ORD_LINE_MASK:
            raise ValueError("GapAccumulator: too many lines for the ordinal")
        self.lines += n
        self.events += int(piece.ev_line.numel())
        a, b = event_windows(self.engine.tabs, piece.ev_line, piece.ev_pat, self.cover)
        cov = coverage(a, b, n)
        if cov_until > base and n:
            if cov is None:
                cov = torch.zeros(n, dtype=torch.uint8, device=self.engine.device)
            cov[:min(cov_until - base, n)] = 1
        # the carries: its events' global [smallest window start, largest window end), where a neighbour can care
        if self.cover == "context" and a.numel() and (held or not piece.last):
            win_lo, win_hi = (torch.stack([a.min(), b.max()]) + base).tolist()
            held = [h for h in held if h[0] < win_lo]               # the rest: inside a window of this piece
            cov_until = max(cov_until, win_hi)
        # (capacity n: 12 bytes per line next to the text's ~100, and never a second run)
        line, sig, n_cand = K.gap_lines(piece.text, piece.ls, piece.ll, piece.features(), cov, n)
        self.error_lines += int(n_cand)
        line = line.long()
        if mb and not piece.last and line.numel():
            tail = line >= n - mb                                   # a later piece's event may still cover these
            t_line, t_sig = line[tail], sig[tail]
            if t_line.numel():
                o = torch.sort(t_line)[1]
                t_line, t_sig = t_line[o], t_sig[o]
                raws = piece.raw_lines(t_line)
                held += [(base + x, s, raw) for x, s, raw in zip(t_line.tolist(), t_sig.tolist(), raws)]
                line, sig = line[~tail], sig[~tail]
        nxt = float("inf") if piece.last else base + n              # the first line a later event can lie on
        done = [h for h in held if h[0] + mb < nxt]                 # out of every later event's reach
        held = [h for h in held if h[0] + mb >= nxt]
        self._fold(doc, line + base, sig, lambda idx: piece.raw_lines(line[idx]), done)
        return cov_until, held

    # ------------------------------------------------------------------ the report
    def report(self, top: Optional[int] = 20) -> dict:
        """The report of everything added so far (more can be added afterwards)."""
        with self._guard():
            return self._report(top)

    def _report(self, top: Optional[int]) -> dict:
        corpus = self.documents != 1
        out = {"totalLines": self.lines, "events": self.events, "errorLines": self.error_lines,
               "uncoveredErrorLines": self.uncovered, "templates": 0, "top": []}
        if corpus:
            out["documents"] = self.documents
        sig, count, first, docs = self.table.rows()
        out["templates"] = int(sig.numel())
        if sig.numel() == 0:
            return out
        order = torch.sort(first, stable=True)[1]                   # by (-count, first ordinal)
        order = order[torch.sort(count[order], descending=True, stable=True)[1]]
        if top is not None:
            order = order[:max(0, int(top))]
        rows = torch.stack([count[order], first[order], sig[order], docs[order].long()]).cpu().tolist()
        for c, f, s, d in zip(*rows):
            raw = self._examples.take(s, f)
            g = {"count": c, "firstLine": (f & ORD_LINE_MASK) + 1, "signature": "%016x" % (s & 0xFFFFFFFFFFFFFFFF),
                 "template": line_template(raw).decode("utf-8", errors="replace"),
                 "example": raw.decode("utf-8", errors="replace")}
            if corpus:
                g["documents"], g["firstDocument"] = d, f >> ORD_SHIFT
            out["top"].append(g)
        return out
