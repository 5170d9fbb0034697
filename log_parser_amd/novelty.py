"""Novelty report: what does a log say that the healthy runs never said? (``golden.novelty`` is
the specification.)

A :class:`Baseline` is the set of template signatures of every line of some healthy logs, kept in
a device-resident ``GapTable`` (csrc/kernels/gap_table.hip). Its walk is lines only -- no matcher
runs, no features are computed. :class:`NoveltyAccumulator` walks ONE failing log in pieces
(pieces.py; the matchers run, because the report says on which novel lines an event lies) and
keeps the lines whose signature the baseline does not hold, grouped by signature.

Both use one text kernel, k_novel_sig (csrc/kernels/novelty.hip): it signs every line, probes the
table and writes only the lines it does not find. Building a baseline is the same pass against
the baseline's own table: the lines it emits are the ones whose template is not in the table yet,
they are folded in, and after the first chunk of a healthy log almost nothing is emitted.

Novelty is a property of a line alone and a group's first line is a minimum, so the report of a
stream needs no carry between chunks: it is the one-document report for every chunk size.
Nothing is scored and the frequency window is not touched.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Optional

import numpy as np
import torch

from .accumulator import U64, Accumulator, Examples
from .engine import Engine
from .golden import line_template
from .ops import kernels as K
from .pieces import Piece, as_bytes, document_piece, stream_lines

FORMAT = 1                  # of a saved baseline
FOLD_SLICE = 1 << 20        # pairs per fold of a baseline: its table follows the templates, not the lines


def check_order(order: str) -> None:
    if order not in ("count", "first"):
        raise ValueError("order must be 'count' or 'first'")


def _same_device(a: torch.device, b: torch.device) -> bool:
    return a.type == b.type and (a.index or 0) == (b.index or 0)


class Baseline:
    """The template signatures of healthy logs: ``add_document`` / ``add_file`` / ``add_stream`` /
    ``add_resident`` (these need an engine: its staging and its chunk plan), ``contains``,
    ``save`` / ``load``. ``lines`` and ``documents`` count what was added, ``templates`` the
    distinct signatures."""

    def __init__(self, engine_or_device, guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.baseline``)."""
        self.engine = engine_or_device if isinstance(engine_or_device, Engine) else None
        self.device = self.engine.device if self.engine is not None else torch.device(engine_or_device)
        self._guard = guard or contextlib.nullcontext
        self.table = K.GapTable(self.device)
        self.lines = self.documents = 0

    @property
    def templates(self) -> int:
        """Distinct signatures (a read of the table's counter)."""
        return self.table.used

    def _engine(self) -> Engine:
        if self.engine is None:
            raise ValueError("Baseline: adding a source needs an engine, this baseline has only a device")
        return self.engine

    # ------------------------------------------------------------------ sources
    def _add_lines(self, text: torch.Tensor, ls: torch.Tensor, ll: torch.Tensor) -> None:
        """The lines (ls, ll) of ``text``: k_novel_sig against the baseline's own table names the
        lines whose template it does not hold yet (with repeats inside one launch), and those are
        folded in -- on the text's stream, the probe before the fold."""
        n = ls.numel()
        self.lines += n
        if n == 0:
            return
        # (an empty table finds nothing: every line comes back, so ask for all of them at once)
        _, sig, _, _ = K.novel_lines(text, ls, ll, self.table, cap=n if self.lines == n else None)
        for a in range(0, sig.numel(), FOLD_SLICE):
            s = sig[a:a + FOLD_SLICE]
            self.table.fold(s, torch.zeros_like(s), winners=False)      # (a set: no first lines, no examples)

    def add_document(self, data) -> None:
        """One document (str or bytes), split by Java's rule (``K.split_lines``)."""
        eng, data = self._engine(), as_bytes(data)
        with self._guard():
            text, n = eng.stage_text(data)
            self._add_lines(text, *K.split_lines(text, n))
            self.documents += 1

    def add_file(self, path) -> None:
        """The file at ``path`` as one document."""
        with open(path, "rb") as f:
            self.add_document(f.read())

    def add_stream(self, src, chunk_bytes: Optional[int] = None) -> None:
        """A bytes-like source (bytes, mmap, ``RepeatBuffer``) or a ``ResidentLog`` as ONE document
        in chunks: only a chunk's own lines count, its halo lines belong to its neighbours."""
        eng = self._engine()
        with self._guard(), stream_lines(eng, src, chunk_bytes) as pieces:
            for piece in pieces:
                self._add_lines(piece.text, piece.ls, piece.ll)
            self.documents += 1

    def add_resident(self, res) -> None:
        self.add_stream(res)

    # ------------------------------------------------------------------ membership, persistence
    def contains(self, signatures) -> torch.Tensor:
        """bool[n] on the baseline's device: the baseline holds the signature. ``signatures``: an
        int64 tensor of bit patterns, or Python ints (``golden.line_signature``'s unsigned values
        or their signed bit patterns)."""
        if not isinstance(signatures, torch.Tensor):
            vals = [int(s) & U64 for s in signatures]
            signatures = torch.tensor([v - (1 << 64) if v >> 63 else v for v in vals], dtype=torch.int64)
        with self._guard():
            return self.table.contains(signatures)

    def signatures(self) -> torch.Tensor:
        """The distinct signatures (int64 bit patterns), sorted."""
        with self._guard():
            return torch.sort(self.table.rows()[0])[0]

    def save(self, path) -> None:
        """One ``.npz`` (no pickle): ``format``, ``sig_max_bytes``, ``lines``, ``documents`` and
        the sorted signatures ``sig int64[templates]``."""
        sig = self.signatures().cpu().numpy()
        with open(path, "wb") as f:             # (a file object: numpy appends no suffix of its own)
            np.savez(f, format=np.int64(FORMAT), sig_max_bytes=np.int64(K.SIG_MAX_BYTES), lines=np.int64(self.lines),
                     documents=np.int64(self.documents), sig=sig)

    @classmethod
    def load(cls, path, engine_or_device, guard: Optional[Callable] = None) -> "Baseline":
        """The baseline saved at ``path``, on ``engine_or_device``; more can be added to it (with an
        engine). ValueError for another format or signature length, for signatures that are not
        int64[n], and for duplicates."""
        with np.load(path, allow_pickle=False) as z:
            missing = {"format", "sig_max_bytes", "lines", "documents", "sig"} - set(z.files)
            if missing:
                raise ValueError("Baseline.load: %s lacks %s" % (path, ", ".join(sorted(missing))))
            fmt, smb, lines, docs, sig = (z[k] for k in ("format", "sig_max_bytes", "lines", "documents", "sig"))
        for name, v in (("format", fmt), ("sig_max_bytes", smb), ("lines", lines), ("documents", docs)):
            if v.shape != () or v.dtype.kind not in "iu":
                raise ValueError("Baseline.load: %s must be one integer" % name)
        if int(fmt) != FORMAT:
            raise ValueError("Baseline.load: format %d, this version reads %d" % (int(fmt), FORMAT))
        if int(smb) != K.SIG_MAX_BYTES:
            raise ValueError("Baseline.load: signatures of the first %d bytes of a line, this version signs %d"
                             % (int(smb), K.SIG_MAX_BYTES))
        if sig.dtype != np.int64 or sig.ndim != 1:
            raise ValueError("Baseline.load: sig must be int64[n], not %s%s" % (sig.dtype, list(sig.shape)))
        if np.unique(sig).size != sig.size:
            raise ValueError("Baseline.load: duplicate signatures")
        b = cls(engine_or_device, guard)
        b.table = K.GapTable.from_signatures(b.device, torch.from_numpy(np.ascontiguousarray(sig)))
        b.lines, b.documents = int(lines), int(docs)
        return b


class NoveltyAccumulator(Accumulator):
    """The novelty report of ONE log against ``baseline``: ``add_document``, ``add_stream`` (a
    bytes-like source in chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further
    sources continue the same log.

    The novel (line, signature) pairs of every piece are folded into a ``GapTable`` with the
    global line as the ordinal: count and first line per group. The pairs on candidate lines and
    the pairs with an event on them are folded into two further tables, whose counts are joined to
    the groups by signature at report time. Only the lines that become a group's first line come
    to the host, as its example."""

    def __init__(self, engine: Engine, baseline: Baseline, guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.novelty_stream``)."""
        if not _same_device(baseline.device, engine.device):
            raise ValueError("novelty: the baseline lives on %s, the engine on %s" % (baseline.device, engine.device))
        super().__init__(engine, guard)
        self.baseline = baseline
        self.table = K.GapTable(engine.device)          # every novel line
        self.err_table = K.GapTable(engine.device)      # ... that is a gap candidate
        self.ev_table = K.GapTable(engine.device)       # ... that an event lies on
        self.lines = self.events = self.error_lines = self.novel = self.novel_errors = 0
        self._examples = Examples("NoveltyAccumulator")       # signature -> (global line, raw line)

    def _add_piece(self, piece: Piece) -> None:
        n, ne = piece.ls.numel(), piece.ev_line.numel()
        self.lines += n
        self.events += ne
        if n == 0:
            return
        ev_mask = None
        if ne:
            ev_mask = torch.zeros(n, dtype=torch.uint8, device=piece.text.device)
            ev_mask[piece.ev_line.long()] = 1
        line, sig, flag, (n_cand, n_novel, n_novel_cand) = K.novel_lines(
            piece.text, piece.ls, piece.ll, self.baseline.table, piece.features(), ev_mask)
        self.error_lines += n_cand
        self.novel += n_novel
        self.novel_errors += n_novel_cand
        if n_novel == 0:
            return
        ordinal = line.long() + piece.line_base
        win = self.table.fold(sig, ordinal)
        if win.numel():
            self._examples.record(sig, ordinal, win, piece.raw_lines(line[win]))
        if n_novel_cand:
            m = (flag & K.NV_CAND) != 0
            self.err_table.fold(sig[m], ordinal[m], winners=False)
        if ne:
            m = (flag & K.NV_EVENT) != 0
            self.ev_table.fold(sig[m], ordinal[m], winners=False)       # (no pair: nothing is launched)

    # ------------------------------------------------------------------ the report
    def report(self, top: Optional[int] = 20, order: str = "count", errors_only: bool = False) -> dict:
        """The report of everything added so far (more can be added afterwards)."""
        check_order(order)
        with self._guard():
            return self._report(top, order, errors_only)

    def _report(self, top: Optional[int], order: str, errors_only: bool) -> dict:
        b = self.baseline
        out = {"totalLines": self.lines, "events": self.events, "errorLines": self.error_lines,
               "novelLines": self.novel, "novelErrorLines": self.novel_errors, "templates": 0, "errorTemplates": 0,
               "baseline": {"documents": b.documents, "lines": b.lines, "templates": b.templates}, "top": []}
        sig, count, first, _ = self.table.rows()
        out["templates"] = int(sig.numel())
        if sig.numel() == 0:
            return out
        errs, _, _, out["errorTemplates"] = self.err_table.lookup(sig)      # (no error line, no event: 0)
        evs = self.ev_table.lookup(sig)[0]
        if errors_only:
            keep = errs > 0
            sig, count, first, errs, evs = sig[keep], count[keep], first[keep], errs[keep], evs[keep]
        pick = torch.sort(first, stable=True)[1]                    # by first line (distinct per group)
        if order == "count":                                        # by (-count, first line)
            pick = pick[torch.sort(count[pick], descending=True, stable=True)[1]]
        if top is not None:
            pick = pick[:max(0, int(top))]
        rows = torch.stack([count[pick], errs[pick], evs[pick], first[pick], sig[pick]]).cpu().tolist()
        for c, ce, cv, f, s in zip(*rows):
            raw = self._examples.take(s, f)
            out["top"].append({"count": c, "errorLines": ce, "eventLines": cv, "firstLine": f + 1,
                               "signature": "%016x" % (s & U64),
                               "template": line_template(raw).decode("utf-8", errors="replace"),
                               "example": raw.decode("utf-8", errors="replace")})
        return out


def novelty_document(eng: Engine, text, n: int, data: bytes, baseline: Baseline, top: Optional[int] = 20,
                     order: str = "count", errors_only: bool = False) -> dict:
    """The report of a staged document in one piece (``Engine.novelty_document``)."""
    check_order(order)
    acc = NoveltyAccumulator(eng, baseline)
    acc._add_pieces([document_piece(eng, text, n, data)])
    return acc._report(top, order, errors_only)
