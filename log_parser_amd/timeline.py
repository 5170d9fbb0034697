"""Log timeline: when did the lines, the error lines and the events of a log happen?
(``golden.timeline`` is the specification.)

A log is walked in pieces (pieces.py): the whole document (``Engine.timeline_document``) or the
chunks of a stream. :func:`timeline_piece` reads the stamp at the head of every line of a piece
(k_ts_parse), gives unstamped lines the time of the nearest earlier stamped line (k_tl_fill, which
also counts the stamps that run backwards), and counts lines, error lines, events and the events'
severities per time bucket (k_tl_hist) -- all on the text's device; the piece's totals and the
non-empty rows of its histogram come to the host in two small copies.

:class:`TimelineAccumulator` merges the pieces of ONE log. Two carries make the report exactly the
one-piece report for every chunk size: the effective time of the last line so far (the fill of a
chunk's leading unstamped lines) and the largest stamp so far (``outOfOrderLines``). Every piece
builds a dense histogram from its own first bucket; buckets are aligned to multiples of the bucket
width, so merging the non-empty rows by absolute bucket start is exact. Nothing is scored and the
frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from .accumulator import Accumulator
from .engine import Engine
from .golden import iso_ms, timeline_span_error
from .ops import kernels as K
from .pieces import Piece, document_piece


def check_bucket_args(bucket_seconds, max_buckets) -> Tuple[int, int]:
    """(bucket width in milliseconds, max_buckets), or ValueError."""
    if isinstance(bucket_seconds, bool) or not isinstance(bucket_seconds, (int, np.integer)) or bucket_seconds < 1:
        raise ValueError("timeline: bucket_seconds must be an integer >= 1")
    if int(max_buckets) < 1:
        raise ValueError("timeline: max_buckets must be >= 1")
    return 1000 * int(bucket_seconds), int(max_buckets)


class TimelineState:
    """The totals of the pieces seen so far, and the two carries."""

    def __init__(self, W: int, max_buckets: int):
        self.W, self.max_buckets = W, max_buckets
        self.lines = self.stamped = self.undated = self.out_of_order = self.events = self.undated_events = 0
        self.first_ts: Optional[int] = None
        self.last_ts: Optional[int] = None               # (= the largest stamp so far: the out-of-order carry)
        self.carry_eff = K.TS_NONE                       # effective time of the last line so far
        self.first_error: Optional[Tuple[int, int]] = None          # (line, time)
        self.first_event: Optional[Tuple[int, int, int]] = None     # (line, pattern, time)
        self.last_event: Optional[Tuple[int, int, int]] = None
        self.rows: Dict[int, List[int]] = {}             # bucket start -> [lines, errorLines, events, severities...]

    def check_span(self, lo: int, hi: int) -> None:
        W = self.W
        first, last = lo // W * W, hi // W * W
        if (last - first) // W + 1 > self.max_buckets:
            raise timeline_span_error(first, last, W, self.max_buckets)


def timeline_piece(eng: Engine, st: TimelineState, piece: Piece) -> None:
    """Add the lines of ``piece`` and their events (in any order) to ``st``."""
    text, ls, ll, ev_line, ev_pat = piece.text, piece.ls, piece.ll, piece.ev_line, piece.ev_pat
    n = ls.numel()
    ne = ev_line.numel()
    st.lines += n
    st.events += ne
    if n == 0:
        return
    dev = text.device
    P = max(1, len(eng.lib.patterns))
    NONE = K.TS_NONE
    ts = K.line_timestamps(text, ls, ll)
    ar = torch.arange(n, device=dev)
    stamped = ts != NONE
    # fill: the stamp of the nearest earlier stamped line (not the largest), else the carry; out of
    # order: below the largest stamp of any earlier line -- two scans in line order, one pass
    eff, n_ooo = K.timeline_fill(ts, st.carry_eff, NONE if st.last_ts is None else st.last_ts)
    dated = eff != NONE
    feat = piece.features()
    cand = ((feat & 9) != 0) & ((feat & 4) == 0) & dated            # golden.gap_candidate on a dated line
    first_cand = torch.where(cand, ar, n).min()
    nums = [stamped.sum(), dated.sum(), n_ooo[0],
            torch.where(stamped, ts, K.I64_MAX).min(), ts.max(), torch.where(dated, eff, K.I64_MAX).min(), eff.max(),
            eff[-1], first_cand, eff[first_cand.clamp(max=n - 1)]]
    ev = ev_line.long()
    if ne:
        # event order is (line, pattern): the smallest and the largest key among the dated events
        key = ev * P + ev_pat.long()
        ev_dated = eff[ev] != NONE
        k_lo, k_hi = torch.where(ev_dated, key, K.I64_MAX).min(), torch.where(ev_dated, key, -1).max()
        nums += [ev_dated.sum(), k_lo, k_hi, eff[(k_lo // P).clamp(max=n - 1)], eff[(k_hi // P).clamp(min=0)]]
    nums = torch.stack(nums).tolist()
    n_stamped, n_dated, n_ooo, ts_lo, ts_hi, eff_lo, eff_hi, eff_last, c_first, c_time = nums[:10]
    st.stamped += n_stamped
    st.undated += n - n_dated
    st.out_of_order += n_ooo
    st.carry_eff = eff_last
    if n_stamped:
        st.first_ts = ts_lo if st.first_ts is None else min(st.first_ts, ts_lo)
        st.last_ts = ts_hi if st.last_ts is None else max(st.last_ts, ts_hi)
        st.check_span(st.first_ts, st.last_ts)
    if ne:
        n_ev_dated, k_lo, k_hi, t_lo, t_hi = nums[10:]
        st.undated_events += ne - n_ev_dated
        if n_ev_dated:
            if st.first_event is None:
                st.first_event = (piece.line_base + k_lo // P, k_lo % P, t_lo)
            st.last_event = (piece.line_base + k_hi // P, k_hi % P, t_hi)
    if c_first < n and st.first_error is None:
        st.first_error = (piece.line_base + c_first, c_time)
    if not n_dated:
        return
    W = st.W
    # (every effective time is a stamp of this or an earlier piece, so nb <= max_buckets: checked above)
    t0 = eff_lo // W * W
    nb = (eff_hi // W * W - t0) // W + 1
    S = len(eng.lib.sev_names)
    hist = K.timeline_hist(eff, feat, ev_line, ev_pat, eng.tabs["sev_index"], t0, W, nb, S)
    used = hist[:, 0].nonzero().flatten()   # an event lies on a line: a bucket without lines is empty
    for b, *cols in torch.cat([used[:, None], hist[used]], 1).tolist():
        row = st.rows.get(t0 + b * W)
        if row is None:
            st.rows[t0 + b * W] = cols
        else:
            for j, c in enumerate(cols):
                row[j] += c


def render(eng: Engine, st: TimelineState) -> dict:
    """The report of ``st`` (``golden.timeline``'s format)."""
    names, pats = eng.lib.sev_names, eng.lib.patterns

    def event(e):
        return None if e is None else {"lineNumber": e[0] + 1, "patternId": pats[e[1]].id, "timestamp": iso_ms(e[2])}

    fe = st.first_error
    return {"totalLines": st.lines, "stampedLines": st.stamped, "undatedLines": st.undated,
            "outOfOrderLines": st.out_of_order,
            "firstTimestamp": None if st.first_ts is None else iso_ms(st.first_ts),
            "lastTimestamp": None if st.last_ts is None else iso_ms(st.last_ts),
            "bucketSeconds": st.W // 1000, "events": st.events, "undatedEvents": st.undated_events,
            "firstErrorLine": None if fe is None else {"lineNumber": fe[0] + 1, "timestamp": iso_ms(fe[1])},
            "firstEvent": event(st.first_event), "lastEvent": event(st.last_event),
            "buckets": [{"start": iso_ms(t), "lines": r[0], "errorLines": r[1], "events": r[2],
                         "severity": {names[s]: c for s, c in enumerate(r[3:]) if c}}
                        for t, r in sorted(st.rows.items())]}


def timeline_document(eng: Engine, text, n: int, data: bytes, bucket_seconds: int = 60,
                      max_buckets: int = 65536) -> dict:
    """The report of a staged document in one piece (``Engine.timeline_document``)."""
    st = TimelineState(*check_bucket_args(bucket_seconds, max_buckets))
    timeline_piece(eng, st, document_piece(eng, text, n, data))
    return render(eng, st)


class TimelineAccumulator(Accumulator):
    """The timeline of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in chunks) or
    ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the same log."""

    def __init__(self, engine: Engine, bucket_seconds: int = 60, max_buckets: int = 65536,
                 guard: Optional[Callable] = None):
        """``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.timeline_stream``)."""
        super().__init__(engine, guard)
        self.state = TimelineState(*check_bucket_args(bucket_seconds, max_buckets))

    @property
    def lines(self) -> int:
        return self.state.lines

    def _add_piece(self, piece: Piece) -> None:
        timeline_piece(self.engine, self.state, piece)      # (the span error leaves in the middle of the log)

    def report(self) -> dict:
        with self._guard():
            return render(self.engine, self.state)
