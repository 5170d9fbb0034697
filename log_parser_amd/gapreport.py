"""Coverage-gap report beyond one document: a stream in chunks, a log resident in HBM, a corpus
of documents (``golden.gaps`` / ``golden.gaps_corpus`` are the specification).

``Engine.gaps_document`` groups one document's (line, signature) pairs with sorts, which a second
chunk or document cannot continue. :class:`GapAccumulator` folds the pairs of every launch into a
device-resident ``GapTable`` (csrc/kernels/gap_table.hip) instead: per signature its count, its
smallest *ordinal* ``(document << 40) | line`` and the number of documents it occurs in. After each
fold the kernel names the pairs that hold their group's smallest ordinal; only those lines' text
comes to the host, as the group's example.

A stream (or a ``ResidentLog``) is ONE document processed in the chunks of ``StreamAnalyzer``
(``_plan`` / ``_producer``: line-aligned, with halos). ``Engine.prepare`` emits the events of a
chunk's own lines only, so an event of a neighbouring chunk can cover a line of this one. Context
windows are contiguous and at most ``lib.halo`` lines wide; two carries make the result exact for
every chunk size:

* forward: ``cov_until``, the largest global window end of any event of the earlier chunks -- an
  own candidate with global line ``g < cov_until`` is covered;
* backward: an uncovered candidate within ``max(lines_before)`` lines of its chunk's end is held
  back (global line, signature, text). Once a later chunk's events are known, held lines at or
  after that chunk's smallest window start are dropped as covered; held lines no later event can
  reach (``g + max_before`` < the next chunk's first line) are folded; the rest stay held -- a
  chunk can be a single line -- and the end of the source folds what remains.

With ``cover="events"`` an event covers its own line only and both carries are empty.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from .engine import Engine, Segments
from .golden import line_template
from .ops import kernels as K
from .parallel.stream import document_chunks

ORD_SHIFT = 40                      # ordinal = (document << ORD_SHIFT) | line
ORD_LINE_MASK = (1 << ORD_SHIFT) - 1


def gather_lines(text: torch.Tensor, starts: torch.Tensor, lens: torch.Tensor) -> List[bytes]:
    """The byte ranges text[starts[i] : starts[i] + lens[i]] as bytes objects: one gather on the
    text's device and one copy to the host, however many ranges."""
    lens = lens.long()
    total = int(lens.sum().item()) if lens.numel() else 0
    ends = lens.cumsum(0)
    if total:
        idx = torch.arange(total, device=text.device) + torch.repeat_interleave(starts.long() - (ends - lens), lens)
        blob = text[idx].cpu().numpy().tobytes()
    else:
        blob = b""
    ends = ends.tolist()
    return [blob[a:b] for a, b in zip([0] + ends[:-1], ends)]


class GapAccumulator:
    """Folds documents (``add_document``), streams (``add_stream``) and resident logs
    (``add_resident``) into one report; ``report`` renders it. An accumulator that has seen exactly
    one document reports what ``Engine.gaps_bytes`` reports for it; any other number of documents
    gives the corpus report (``golden.gaps_corpus``). Nothing is scored and the frequency window is
    not touched."""

    def __init__(self, engine: Engine, cover: str = "context", guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.gap_accumulator``)."""
        if cover not in ("events", "context"):
            raise ValueError("cover must be 'events' or 'context'")
        self.engine = engine
        self._guard = guard or contextlib.nullcontext
        self.cover = cover
        self.table = K.GapTable(engine.device)
        self.lines = self.events = self.error_lines = self.uncovered = self.documents = 0
        self._examples: Dict[int, Tuple[int, bytes]] = {}     # signature -> (ordinal, raw line)
        before = engine.lib.ctx_before
        self._max_before = max(0, int(np.max(before))) if cover == "context" and len(before) else 0

    # ------------------------------------------------------------------ folding
    def _fold(self, doc: int, line: torch.Tensor, sig: torch.Tensor, fetch: Optional[Callable],
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
            raws = fetch(mine)
            sigs, ords = torch.stack([sig[mine], ordinal[mine]]).cpu().tolist()
            ex = self._examples
            for s, o, raw in zip(sigs, ords, raws):         # (inlined _record: one winner per NEW template)
                cur = ex.get(s)
                if cur is None or o < cur[0]:
                    ex[s] = (o, raw)
        if held:
            for w in win[win >= n].tolist():
                g, s, raw = held[w - n]
                self._record(s, g + (doc << ORD_SHIFT), raw)

    def _record(self, sig: int, ordinal: int, raw: bytes) -> None:
        cur = self._examples.get(sig)
        if cur is None or ordinal < cur[0]:
            self._examples[sig] = (ordinal, raw)

    def _new_document(self) -> int:
        doc = self.documents
        if doc >= (1 << 22):
            raise ValueError("GapAccumulator: too many documents for the ordinal")
        self.documents += 1
        return doc

    # ------------------------------------------------------------------ one whole document
    def add_document(self, data) -> None:
        """One document (str or bytes) in one piece: ``Engine.gaps_document``'s steps up to the pairs."""
        if isinstance(data, str):
            data = data.encode("utf-8", errors="surrogateescape")
        with self._guard():
            self._add_document(bytes(data))

    def _add_document(self, data: bytes) -> None:
        eng = self.engine
        doc = self._new_document()
        text, n = eng.stage_text(data)
        ls, ll = K.split_lines(text, n)
        L = ls.numel()
        if L == 0:
            return
        if L > ORD_LINE_MASK:
            raise ValueError("GapAccumulator: too many lines for the ordinal")
        self.lines += L
        segs = Segments.single(L, eng.device)
        prep = eng.prepare(text, n, ls, ll, segs, np.frombuffer(data, np.uint8) if n else None)
        self.events += int(prep.ev_line.numel())
        feat = K.context_features_all(text, ls, ll, eng.tabs["dfa"], eng.lib.ctx_dfa_extent)
        cov = eng._gap_coverage(prep.ev_line, prep.ev_pat, L, self.cover)
        line, sig, n_cand = K.gap_lines(text, ls, ll, feat, cov, L)
        self.error_lines += int(n_cand)

        def fetch(idx):
            x = line[idx].long()
            a, m = torch.stack([ls[x], ll[x].long()]).cpu().tolist()
            return [data[s:s + k] for s, k in zip(a, m)]
        self._fold(doc, line, sig, fetch)

    # ------------------------------------------------------------------ one document in chunks
    def add_stream(self, src, chunk_bytes: Optional[int] = None) -> None:
        """A bytes-like source (bytes, mmap, ``RepeatBuffer``) as ONE document, in chunks."""
        with self._guard():
            self._add_chunked(src, chunk_bytes)

    def add_resident(self, res) -> None:
        """A ``ResidentLog`` as ONE document, read in place chunk by chunk."""
        with self._guard():
            self._add_chunked(res, None)

    def _add_chunked(self, src, chunk_bytes: Optional[int]) -> None:
        eng = self.engine
        dev = eng.device
        tabs = eng.tabs
        doc = self._new_document()
        context = self.cover == "context"
        mb = self._max_before
        line_base = 0                       # global number of the chunk's first own line
        cov_until = 0                       # forward carry
        held: List[tuple] = []              # backward carry: (global line, signature, raw), ascending
        for text, n, lh, rh, host in document_chunks(eng, src, chunk_bytes):
            ls, ll = K.split_chunk_lines(text, n)
            L = ls.numel()
            own_lo, own_hi = lh, L - rh
            n_own = own_hi - own_lo
            if line_base + n_own > ORD_LINE_MASK:
                raise ValueError("GapAccumulator: too many lines for the ordinal")
            segs = Segments.scalar(0, L, own_lo, own_hi, line_base - own_lo, 1 << 62, dev)
            prep = eng.prepare(text, n, ls, ll, segs, host_text=host[:n].numpy() if host is not None else None,
                               split_trim=False)
            ne = int(prep.ev_line.numel())
            self.events += ne
            cov = eng._gap_coverage(prep.ev_line, prep.ev_pat, L, self.cover)
            win_lo = win_hi = None          # global [smallest window start, largest window end) of the chunk's events
            if context and ne:
                g = prep.ev_line.long() + (line_base - own_lo)
                p = prep.ev_pat.long()
                before, after = tabs["ctx_before"][p].long(), tabs["ctx_after"][p].long()
                rules = before >= 0
                lo = torch.where(rules, g - before, g).min()
                hi = torch.where(rules, g + 1 + after, g + 1).max()
                win_lo, win_hi = torch.stack([lo, hi]).tolist()
            if held and win_lo is not None:
                held = [h for h in held if h[0] < win_lo]           # the rest: inside a window of this chunk
            if cov_until > line_base and n_own:
                if cov is None:
                    cov = torch.zeros(L, dtype=torch.uint8, device=dev)
                cov[own_lo:own_lo + min(cov_until - line_base, n_own)] = 1
            o_ls, o_ll = ls[own_lo:own_hi], ll[own_lo:own_hi]
            feat = K.context_features_all(text, o_ls, o_ll, tabs["dfa"], eng.lib.ctx_dfa_extent)
            line, sig, n_cand = K.gap_lines(text, o_ls, o_ll, feat, None if cov is None else cov[own_lo:own_hi], n_own)
            self.error_lines += int(n_cand)
            self.lines += n_own
            line = line.long()
            if mb and line.numel():
                tail = line >= n_own - mb                           # a later chunk's event may still cover these
                t_line, t_sig = line[tail], sig[tail]
                if t_line.numel():
                    o = torch.sort(t_line)[1]
                    t_line, t_sig = t_line[o], t_sig[o]
                    raws = gather_lines(text, o_ls[t_line], o_ll[t_line])
                    held += [(line_base + x, s, raw) for x, s, raw in zip(t_line.tolist(), t_sig.tolist(), raws)]
                    line, sig = line[~tail], sig[~tail]
            nxt = line_base + n_own
            done = [h for h in held if h[0] + mb < nxt]             # out of every later event's reach
            held = [h for h in held if h[0] + mb >= nxt]
            rel = line

            def fetch(idx, text=text, o_ls=o_ls, o_ll=o_ll, rel=rel):
                x = rel[idx]
                return gather_lines(text, o_ls[x], o_ll[x])
            self._fold(doc, line + line_base, sig, fetch, done)
            if win_hi is not None:
                cov_until = max(cov_until, win_hi)
            line_base = nxt
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        self._fold(doc, empty, empty, None, held)

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
            o, raw = self._examples[s]
            if o != f:
                raise RuntimeError("GapAccumulator: the example of %016x is not its first line" % (s & (2 ** 64 - 1)))
            g = {"count": c, "firstLine": (f & ORD_LINE_MASK) + 1, "signature": "%016x" % (s & 0xFFFFFFFFFFFFFFFF),
                 "template": line_template(raw).decode("utf-8", errors="replace"),
                 "example": raw.decode("utf-8", errors="replace")}
            if corpus:
                g["documents"], g["firstDocument"] = d, f >> ORD_SHIFT
            out["top"].append(g)
        return out
