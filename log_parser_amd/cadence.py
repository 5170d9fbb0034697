"""Cadence report: which line templates come at a steady beat, where did one of them miss beats,
and which never came back before the log ended? (``golden.cadence`` is the specification.)

The stamped lines of ONE template in line order are ``j_0 < j_1 < ...``; the *beat* k is the stamp
of ``j_k`` minus the stamp of ``j_{k-1}``. A beat below 0 runs backwards and is only counted.

:class:`CadenceAccumulator` walks ONE log in pieces without events (the walk without the matchers
of ``accumulator.LineAccumulator``). Per run:

* ``K.line_stamps``: signature and stamp of every line from one visit of the line;
* ``K.beat_scan`` (k_cd_tile / k_cdl_tiles / k_cdl_prefix / k_cdl_emit, csrc/kernels/cadence.hip):
  the beat of every stamped line and its interval bucket, and the running *state* -- one row per
  template, sorted by signature: lines, beats, backward beats, sum, min, max with its two lines,
  first and last stamped line. The state stays on the device; the state after the runs is the
  state of the whole log, wherever the cuts fall;
* a ``CellTable`` fold of (signature, bucket) with the bucket width 1: the interval histogram of
  every template;
* a ``GapTable`` fold of (signature, global line): the templates of all lines, stamped or not.

Of the text only this reaches the host: the first stamped line of a template that is new in the
run (its example). The lines around a hole are reported by number and time. ``report`` reads the
state and the cells once; the judgement is ``golden.cadence_judge`` on exact integers. The report
is the one-document report at every chunk size. Nothing is scored and the frequency window is not
touched.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch

from .accumulator import U64, Examples, LineAccumulator
from .engine import Engine
from .golden import PAUSE_BUCKETS, cadence_head, cadence_judge, cadence_listed, cadence_order_key, cadence_row
from .golden import cadence_check_args as check_args
from .ops import kernels as K
from .pieces import Piece


def check_top(top) -> Optional[int]:
    if top is None:
        return None
    if isinstance(top, bool) or not isinstance(top, int):
        raise ValueError("cadence: top must be None or an integer")
    return max(0, top)


class CadenceAccumulator(LineAccumulator):
    """The cadence report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log: their first line follows the lines so far. Every parameter belongs to ``report``:
    what is kept per template does not depend on them."""

    def __init__(self, engine: Engine, guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.cadence_accumulator``)."""
        super().__init__(engine, guard)
        dev = engine.device
        self.state = K.beat_state(dev)          # one row per template with a stamped line, sorted by signature
        self.cells = K.CellTable(dev)           # (signature, interval bucket): the templates' histograms
        self.by_template = K.GapTable(dev)      # (signature, g): the templates of all lines
        self.next_line = 0
        self._examples = Examples("CadenceAccumulator")       # signature (signed) -> (first stamped line, its bytes)

    def _add_piece(self, piece: Piece) -> None:
        text, ls, ll = piece.text, piece.ls, piece.ll
        n, base = ls.numel(), self.next_line
        if n == 0:
            return
        self.next_line = base + n
        dev = text.device
        sig, ts = K.line_stamps(text, ls.contiguous(), ll.contiguous())
        _, bkt, state = K.beat_scan(ts, sig, base, self.state)
        self.cells.fold(sig, bkt, base, 1)
        self.by_template.fold(sig, torch.arange(base, base + n, dtype=torch.int64, device=dev), winners=False)
        # the templates this run brought: their first stamped line is the example
        known, now = self.state[K.CD_SIG], state[K.CD_SIG]
        self.state = state
        if now.numel() == known.numel():        # (signatures only come, never go)
            return
        fresh = torch.ones_like(now, dtype=torch.bool)
        if known.numel():
            fresh = known[torch.searchsorted(known, now).clamp(max=known.numel() - 1)] != now
        keys, firsts = state[[K.CD_SIG, K.CD_FIRST_LINE]][:, fresh].cpu().tolist()
        if min(firsts) < base:
            raise RuntimeError("CadenceAccumulator: a new template's first line %d lies before this run" % (min(firsts) + 1))
        self._examples.put_all(keys, firsts, piece.raw_lines(torch.tensor(firsts, dtype=torch.int64, device=dev) - base))

    # ------------------------------------------------------------------ the report
    def report(self, min_ms: int = 1000, ratio: int = 4, min_count: int = 5, min_regularity=0.8,
               kind: Optional[str] = None, order: str = "gap", top: Optional[int] = 20) -> dict:
        """The report of everything added so far (more can be added afterwards)."""
        min_reg = check_args(min_ms, ratio, min_count, min_regularity, kind, order)
        top = check_top(top)
        with self._guard():
            return self._report(min_ms, ratio, min_count, min_reg, kind, order, top)

    def _report(self, min_ms: int, ratio: int, min_count: int, min_reg, kind: Optional[str], order: str,
                top: Optional[int]) -> dict:
        state = self.state
        templates = self.by_template.used
        if state.shape[1] == 0:
            return cadence_head(self.next_line, 0, templates, None, None)
        # the templates that can be periodic at all, and their cells; one read
        cols = state[:, state[K.CD_BEATS] >= max(min_count, 2)]
        c_sig, c_bkt, c_cnt, _ = self.cells.rows()
        mine = c_bkt != K.CT_UNDATED
        if cols.shape[1]:
            at = torch.searchsorted(cols[K.CD_SIG], c_sig).clamp(max=cols.shape[1] - 1)
            mine &= cols[K.CD_SIG][at] == c_sig
        else:
            mine &= False
        ends = torch.stack([state[K.CD_LINES].sum(), state[K.CD_FIRST_TS][state[K.CD_FIRST_LINE].argmin()],
                            state[K.CD_LAST_TS][state[K.CD_LAST_LINE].argmax()]])
        nc = int(cols.shape[1])
        flat = torch.cat([ends, cols.reshape(-1), c_sig[mine], c_bkt[mine], c_cnt[mine]]).cpu().tolist()
        stamped, first, end = flat[:3]
        rows = list(zip(*(flat[3 + c * nc: 3 + (c + 1) * nc] for c in range(K.CD_COLS))))
        rest = flat[3 + K.CD_COLS * nc:]
        m = len(rest) // 3
        hists: Dict[int, List[int]] = {}
        for s, b, c in zip(rest[:m], rest[m:2 * m], rest[2 * m:]):
            hists.setdefault(s, [0] * PAUSE_BUCKETS)[b] += c
        out = cadence_head(self.next_line, stamped, templates, first, end)
        listed = []
        for r in rows:
            s, beats = r[K.CD_SIG], r[K.CD_BEATS]
            hist = hists.get(s, [0] * PAUSE_BUCKETS)
            if sum(hist) != beats:
                raise RuntimeError("CadenceAccumulator: %016x has %d forward beats, its intervals hold %d"
                                   % (s & U64, beats, sum(hist)))
            j = cadence_judge(beats, r[K.CD_SUM], r[K.CD_MAX], r[K.CD_LAST_TS], end, hist, min_ms, ratio, min_count, min_reg)
            if j is None:
                continue
            out["periodic"] += 1
            out["missed"] += j["missed"]
            out["stopped"] += j["stopped"]
            if cadence_listed(kind, j["missed"], j["stopped"]):
                listed.append((cadence_order_key(order, j["typicalMs"], r[K.CD_MAX], j["overdueMs"], beats,
                                                 r[K.CD_FIRST_LINE]), r, hist, j))
        listed.sort(key=lambda kv: kv[0])
        if top is not None:
            listed = listed[:top]
        for _, r, hist, j in listed:
            raw = self._examples.take(r[K.CD_SIG], r[K.CD_FIRST_LINE])
            out["top"].append(cadence_row(r[K.CD_SIG] & U64, r[K.CD_LINES], r[K.CD_BEATS], r[K.CD_BACKWARD], r[K.CD_SUM],
                                          r[K.CD_MIN], r[K.CD_MAX], r[K.CD_MAX_FROM], r[K.CD_MAX_TO], r[K.CD_MAX_TO_TS],
                                          r[K.CD_FIRST_LINE], r[K.CD_LAST_LINE], r[K.CD_LAST_TS], hist, j, raw))
        return out


def cadence_document(eng: Engine, data: bytes, min_ms: int = 1000, ratio: int = 4, min_count: int = 5,
                     min_regularity=0.8, kind: Optional[str] = None, order: str = "gap",
                     top: Optional[int] = 20) -> dict:
    """The report of one document (``Engine.cadence_bytes``)."""
    check_args(min_ms, ratio, min_count, min_regularity, kind, order)
    check_top(top)
    acc = CadenceAccumulator(eng)
    acc.add_document(data)
    return acc.report(min_ms, ratio, min_count, min_regularity, kind, order, top)


def cadence_stream(eng: Engine, src, chunk_bytes: Optional[int] = None, min_ms: int = 1000, ratio: int = 4,
                   min_count: int = 5, min_regularity=0.8, kind: Optional[str] = None, order: str = "gap",
                   top: Optional[int] = 20) -> dict:
    """The report of ONE log in chunks: a bytes-like source (bytes, mmap, ``RepeatBuffer``) or a
    ``ResidentLog``. Exactly the one-document report, whatever the chunk size."""
    check_args(min_ms, ratio, min_count, min_regularity, kind, order)
    check_top(top)
    acc = CadenceAccumulator(eng)
    acc.add_stream(src, chunk_bytes)
    return acc.report(min_ms, ratio, min_count, min_regularity, kind, order, top)
