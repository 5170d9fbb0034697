"""The host side that the report accumulators share: how a source becomes pieces, and how the
example line of a group is kept.

:class:`Accumulator` owns ``add_document`` / ``add_stream`` / ``add_resident``: a source is walked
in the pieces of pieces.py under the accumulator's guard, and a subclass says what a piece adds
(``_add_piece``) and, where something happens between or after the pieces, how a source's pieces
are looped over (``_add_pieces``). :class:`LineAccumulator` is the walk without the matchers.

:class:`Examples` owns the rule by which a group's example is kept -- the one with the smallest
ordinal wins, whichever comes first -- and the check at report time that the example kept is the
one the device-side table calls the group's first.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch

from .engine import Engine
from .pieces import Piece, as_bytes, document_lines, document_piece, stream_lines, stream_pieces

U64 = (1 << 64) - 1


class Examples:
    """key -> (ordinal, payload) of the group's smallest ordinal seen so far. The payload is the
    raw line, or whatever else a report shows of its first occurrence."""

    def __init__(self, who: str):
        self.who = who
        self._held: Dict[int, Tuple[int, object]] = {}

    def put_all(self, keys, ordinals, payloads) -> None:
        """Candidates whose numbers are on the host already (the rows of a read the caller makes
        anyway). One loop without a call per candidate: a log can bring 100,000 new groups."""
        held = self._held
        for k, o, payload in zip(keys, ordinals, payloads):
            cur = held.get(k)
            if cur is None or o < cur[0]:
                held[k] = (o, payload)

    def put(self, key: int, ordinal: int, payload) -> None:
        """One candidate (a held or pending line whose bytes were carried)."""
        self.put_all((key,), (ordinal,), (payload,))

    def record(self, key: torch.Tensor, ordinal: torch.Tensor, win: torch.Tensor, payloads: List) -> None:
        """The winners ``win`` of a fold (``GapTable.fold``) of the pairs (key, ordinal), with
        ``payloads[i]`` for the pair ``win[i]``: one read of the winners' keys and ordinals; one
        winner per NEW group in steady state."""
        self.put_all(*torch.stack([key[win], ordinal[win]]).cpu().tolist(), payloads)

    def take_all(self, keys, firsts) -> List:
        """The payloads of ``keys``, whose smallest ordinals the table says are ``firsts``."""
        held, out = self._held, []
        for k, f in zip(keys, firsts):
            ordinal, payload = held[k]
            if ordinal != f:
                raise RuntimeError("%s: the example of %016x is not its first line" % (self.who, k & U64))
            out.append(payload)
        return out

    def take(self, key: int, first: int):
        return self.take_all((key,), (first,))[0]


class Accumulator:
    """``add_document`` / ``add_stream`` / ``add_resident`` of a report that is fed over time.
    Sources continue ONE log: the first line of a source has the number ``self.lines``."""

    document_walk, stream_walk = staticmethod(document_piece), staticmethod(stream_pieces)
    lines = 0

    def __init__(self, engine: Engine, guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock)."""
        self.engine = engine
        self._guard = guard or contextlib.nullcontext

    def _line_base(self) -> int:
        """The number of the next source's first line."""
        return self.lines

    def add_document(self, data) -> None:
        """One document (str or bytes) in one piece."""
        data = as_bytes(data)
        with self._guard():
            piece = self.document_walk(self.engine, *self.engine.stage_text(data), data)
            piece.line_base = self._line_base()
            self._add_pieces([piece])

    def add_stream(self, src, chunk_bytes: Optional[int] = None) -> None:
        """A bytes-like source (bytes, mmap, ``RepeatBuffer``) or a ``ResidentLog``, in chunks."""
        with self._guard(), self.stream_walk(self.engine, src, chunk_bytes, line_base=self._line_base()) as pieces:
            self._add_pieces(pieces)

    def add_resident(self, res) -> None:
        """A ``ResidentLog``, read in place chunk by chunk."""
        self.add_stream(res)

    def _add_pieces(self, pieces: Iterable[Piece]) -> None:
        for piece in pieces:
            self._add_piece(piece)

    def _add_piece(self, piece: Piece) -> None:
        raise NotImplementedError


class LineAccumulator(Accumulator):
    """The walk without the matchers: pieces without events, counted in ``next_line``."""

    document_walk, stream_walk = staticmethod(document_lines), staticmethod(stream_lines)
    next_line = 0

    def _line_base(self) -> int:
        return self.next_line

    def _add_pieces(self, pieces: Iterable[Piece]) -> None:
        for piece in pieces:
            if piece.line_base != self.next_line:
                raise RuntimeError("%s: a chunk starts at line %d, expected %d"
                                   % (type(self).__name__, piece.line_base, self.next_line))
            self._add_piece(piece)
