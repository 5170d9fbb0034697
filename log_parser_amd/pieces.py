"""The source walk of the reports: every report that reads a log without scoring it loops over the
pieces of this module (accumulator.py holds that loop).

A *piece* is a run of consecutive lines of one document, with the events on them. What differs
between the two kinds of source, and between a walk with the matchers and one without, stays in
here:

* :func:`document_piece`: a whole document is split by ``K.split_lines`` (Java's rule: no trailing
  empty lines), is one segment that owns every line, and hands ``prepare`` its host bytes;
* :func:`stream_pieces`: a bytes-like source or a ``ResidentLog`` is ONE document in the chunks of
  ``parallel.stream.document_chunks`` -- line-aligned, with ``lib.halo`` lines of the neighbours on
  either side, split by ``K.split_chunk_lines`` (nothing trimmed). ``prepare`` emits the events of
  a chunk's own lines only, and the piece is cut down to those lines; no halo leaves this module;
* :func:`document_lines` / :func:`stream_lines`: the same lines as pieces WITHOUT the matchers
  (no events), for a report that needs none (values, trends, pauses, a baseline) or walks its
  source a second time (correlate.py).

An event of a neighbouring piece can still concern a line of this one: such carries belong to the
report (``line_base`` and ``last`` are for them). Nothing is scored, no frequency window touched.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Iterator, List, Optional

import numpy as np
import torch

from .engine import Engine, Segments
from .ops import kernels as K
from .parallel.stream import document_chunks

_N_OPEN = 1 << 62       # a stream's line count N is open while it is walked (as in ``StreamAnalyzer.run``)


def as_bytes(data) -> bytes:
    """A document given as str or bytes-like, as bytes."""
    if isinstance(data, str):
        data = data.encode("utf-8", errors="surrogateescape")
    return bytes(data)


def gather_lines(text: torch.Tensor, starts: torch.Tensor, lens: torch.Tensor) -> List[bytes]:
    """The byte ranges text[starts[i] : starts[i] + lens[i]] as bytes objects: one gather on the
    text's device and one copy to the host, however many ranges."""
    lens = lens.long()
    ends = lens.cumsum(0)
    idx = torch.repeat_interleave(starts.long() - (ends - lens), lens)      # per byte: range start - blob offset
    blob = text[idx + torch.arange(idx.numel(), device=text.device)].cpu().numpy().tobytes()
    ends = ends.tolist()
    return [blob[a:b] for a, b in zip([0] + ends[:-1], ends)]


@dataclass
class Piece:
    """``ls`` / ``ll``: the line index of the piece's lines in ``text``; ``ev_line`` counts from its
    first line, whose number in the document is ``line_base``; ``last``: no later piece of this
    document can follow; ``host``: the document's bytes (``text`` is their staged copy), if any."""
    eng: Engine
    text: torch.Tensor
    ls: torch.Tensor
    ll: torch.Tensor
    ev_line: torch.Tensor
    ev_pat: torch.Tensor
    line_base: int
    last: bool
    host: Optional[bytes] = None
    _feat: Optional[torch.Tensor] = None

    def features(self) -> torch.Tensor:
        """The context features of every line of the piece (``K.context_features_all``), computed once."""
        if self._feat is None:
            self._feat = K.context_features_all(self.text, self.ls, self.ll, self.eng.tabs["dfa"],
                                                self.eng.lib.ctx_dfa_extent)
        return self._feat

    def raw_lines(self, idx: torch.Tensor) -> List[bytes]:
        """The bytes of the piece's lines ``idx``: cut from the host copy after one read of their
        index rows, or gathered on the device (``gather_lines``) where there is none."""
        x = idx.long()
        if self.host is None:
            return gather_lines(self.text, self.ls[x], self.ll[x])
        a, m = torch.stack([self.ls[x], self.ll[x].long()]).cpu().tolist()
        return [self.host[s:s + k] for s, k in zip(a, m)]


def _lines_piece(eng: Engine, text, ls, ll, line_base: int, last: bool, host: Optional[bytes] = None) -> Piece:
    none = torch.empty(0, dtype=torch.int32, device=text.device)
    return Piece(eng, text, ls, ll, none, none, line_base, last, host=host)


def document_lines(eng: Engine, text: torch.Tensor, n: int, data: bytes) -> Piece:
    """The one piece of a staged document WITHOUT the matchers: its lines and its host bytes."""
    return _lines_piece(eng, text, *K.split_lines(text, n), 0, True, host=data)


def document_piece(eng: Engine, text: torch.Tensor, n: int, data: bytes) -> Piece:
    """The one piece of a staged document (``text`` = ``stage_text(data)``'s buffer), matched as
    ``analyze_bytes`` matches it. Without lines: a piece without lines, and nothing is launched."""
    ls, ll = K.split_lines(text, n)
    if ls.numel() == 0:
        return _lines_piece(eng, text, ls, ll, 0, True, host=data)
    segs = Segments.single(ls.numel(), eng.device)
    prep = eng.prepare(text, n, ls, ll, segs, np.frombuffer(data, np.uint8) if n else None)
    return Piece(eng, text, ls, ll, prep.ev_line, prep.ev_pat, 0, True, host=data)


@contextlib.contextmanager
def stream_pieces(eng: Engine, src, chunk_bytes: Optional[int] = None, line_base: int = 0) -> Iterator[Iterator[Piece]]:
    """``with stream_pieces(eng, src) as pieces: for piece in pieces: ...`` -- the pieces of a
    bytes-like source (bytes, mmap, ``RepeatBuffer``) or a ``ResidentLog`` as ONE document whose
    first line has the number ``line_base``. A source without lines yields no piece."""
    # closing: a report may leave in the middle of the log (the timeline's span error), and the
    # chunk producer must not outlive that (it holds the source, which the caller may be about to
    # unmap) -- on every exit, not only where CPython happens to finalise an abandoned generator
    with contextlib.closing(document_chunks(eng, src, chunk_bytes)) as chunks:
        yield _chunk_pieces(eng, chunks, line_base)


def _chunk_pieces(eng: Engine, chunks, line_base: int) -> Iterator[Piece]:
    for text, n, lh, rh, host, last in chunks:
        ls, ll = K.split_chunk_lines(text, n)
        L = ls.numel()
        own_lo, own_hi = lh, L - rh         # only a chunk's own lines emit events and are reported
        segs = Segments.scalar(0, L, own_lo, own_hi, line_base - own_lo, _N_OPEN, eng.device)
        prep = eng.prepare(text, n, ls, ll, segs, host_text=host[:n].numpy() if host is not None else None,
                           split_trim=False)
        yield Piece(eng, text, ls[own_lo:own_hi], ll[own_lo:own_hi], prep.ev_line - own_lo, prep.ev_pat, line_base,
                    last)
        line_base += own_hi - own_lo


@contextlib.contextmanager
def stream_lines(eng: Engine, src, chunk_bytes: Optional[int] = None, line_base: int = 0) -> Iterator[Iterator[Piece]]:
    """``with stream_lines(eng, src) as pieces: for piece in pieces: ...`` -- the pieces of
    ``stream_pieces`` WITHOUT the matchers: the same chunks, of every chunk its own lines (the halo
    lines cut off), the same ``line_base`` and ``last``, no events."""
    with contextlib.closing(document_chunks(eng, src, chunk_bytes)) as chunks:
        yield _chunk_lines(eng, chunks, line_base)


def _chunk_lines(eng: Engine, chunks, line_base: int) -> Iterator[Piece]:
    for text, n, lh, rh, _host, last in chunks:
        ls, ll = K.split_chunk_lines(text, n)
        own_lo, own_hi = lh, ls.numel() - rh
        yield _lines_piece(eng, text, ls[own_lo:own_hi], ll[own_lo:own_hi], line_base, last)
        line_base += own_hi - own_lo
