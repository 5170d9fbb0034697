"""Spans report: the lifetimes of the ids of a log -- which request, job, trace or connection took
longest, and which started like all the others and never logged the line the others end on?
(``golden.spans`` is the specification.)

No pattern takes part. One text kernel, k_span_keys (csrc/kernels/spans.hip), visits every line
once for its stamp, its template signature and its keys (``golden.line_keys``) with the places of
their tokens; the ``SpanTable`` (span_table.h) keeps a whole span per key: lines, first and last
line, smallest and largest effective time, the templates of the first and the last line, and the
id's own lowered bytes. :class:`SpanAccumulator` walks ONE log in pieces without events and, per
piece, in this order:

1. ``K.span_keys`` with the current sample shift;
2. the signatures into ``by_template``; its winners -- one line per NEW template -- are the only
   lines that come to the host, as the templates' examples;
3. ``K.timeline_fill`` with the carried last stamp: the effective time of every line;
4. ``SpanTable.fold``: fold, then ends;
5. the sample rule.

Bounded memory -- nested hash samples. A table of every id of a large log is as large as the log,
so the table holds at most ``max_ids`` ids between pieces. A key is in sample ``s`` when the top
``s`` bits of ``fmix64(key)`` are zero; ``s`` starts at 0, and after each piece, while the table
holds more than ``max_ids`` keys, ``s += 1`` and the rows outside sample ``s`` are purged. The text
kernel emits only the keys of the current sample.

Chunk independence: the samples are nested, so an id of the final sample was in every earlier
sample, and nothing of it was ever dropped or left unemitted: its row is the row of the
one-document walk (count, min and max fold in any order; ``opens`` and the token come from its
first line, ``closes`` from its last, wherever the pieces are cut). ``s`` rises only when the
distinct ids of sample ``s`` seen so far exceed ``max_ids``, and the distinct count of a prefix
never exceeds that of the whole log; the check after the last piece sees the whole log. Therefore
the final ``s`` is the smallest ``s`` whose sample of the whole log has at most ``max_ids`` ids,
wherever the pieces are cut. Within a piece the table holds at most ``max_ids`` plus the piece's
new ids. The head's ``idLines`` comes from a histogram, kept by the text kernel, of the lines by the
deepest sample that still holds one of their keys: a line counted under an earlier, smaller ``s``
whose keys all left the sample is in a bucket below the final ``s`` and is not summed. ``max_ids``
and ``min_len`` are fixed when the accumulator is made.

``report`` reads the rows once and filters, groups and orders them with torch on the table's
device, in exact integers (the share of ``max_share`` as in correlate.py: a double compare that is
exact below 2^53). The kinds' closing templates -- one small row per (opens, closes) -- come to the
host, where ``golden.spans_usual_end`` decides the usual ends in exact fractions; of the spans only
the listed rows do. Nothing is scored and the frequency window is not touched.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from .accumulator import U64, Examples, LineAccumulator
from .engine import Engine
from .golden import SPAN_BUCKETS, SPAN_MAX_IDS
from .golden import spans_check_args as check_args
from .golden import spans_durations, spans_head, spans_kind_row, spans_row, spans_usual_end
from .ops import kernels as K
from .pieces import Piece

_I64_MIN = -(1 << 63)


def _by(cols, n: int, device) -> torch.Tensor:
    """The order of n rows by ``cols`` = [(column, descending)], most significant first: stable
    sorts, the least significant first."""
    pick = torch.arange(n, dtype=torch.int64, device=device)
    for col, desc in reversed(cols):
        pick = pick[torch.sort(col[pick], descending=desc, stable=True)[1]]
    return pick


class SpanAccumulator(LineAccumulator):
    """The spans report of ONE log: ``add_document``, ``add_stream`` (a bytes-like source in
    chunks) or ``add_resident`` (a ``ResidentLog``), then ``report``. Further sources continue the
    same log: their first line follows the lines so far."""

    def __init__(self, engine: Engine, min_len: int = 8, max_ids: int = SPAN_MAX_IDS, guard: Optional[Callable] = None):
        """``min_len`` (4..64) and ``max_ids`` (16..2^26) are fixed here: a purged id cannot come
        back. ``guard``: a context manager factory entered around every use of the engine (the
        parser's lock, ``LogParser.span_accumulator``)."""
        check_args(min_len, max_ids)
        super().__init__(engine, guard)
        dev = engine.device
        self.min_len, self.max_ids = min_len, max_ids
        self.by_template = K.GapTable(dev)      # (signature, g), every line: the templates and their first lines
        self.table = K.SpanTable(dev)           # key -> span
        self.levels = torch.zeros(K.SPAN_LEVELS, dtype=torch.int64, device=dev)    # id lines by deepest sample
        self.shift = 0
        self.next_line = 0
        self.carry_last = K.TS_NONE             # the stamp of the last stamped line so far
        self._timed = torch.zeros((), dtype=torch.int64, device=dev)
        self._examples = Examples("SpanAccumulator")        # signature (signed) -> (first line, its bytes)

    def _add_piece(self, piece: Piece) -> None:
        text, ls, ll = piece.text, piece.ls.contiguous(), piece.ll.contiguous()
        n, base = ls.numel(), self.next_line
        if n == 0:
            return
        self.next_line = base + n
        dev = text.device
        sig, ts, line, key, tok, (m, _) = K.span_keys(text, ls, ll, self.min_len, self.shift, levels=self.levels)
        g = torch.arange(base, base + n, dtype=torch.int64, device=dev)
        win = self.by_template.fold(sig, g)
        if win.numel():
            self._examples.record(sig, g, win, piece.raw_lines(win))
        eff, _ = K.timeline_fill(ts, self.carry_last)
        self.carry_last = int(eff[-1].item())
        self._timed += (eff != K.TS_NONE).sum()
        if m == 0:
            return
        self.table.fold(line, key, tok, sig, eff, text, ls, base)
        # the sample rule (the host bound of the occupied slots spares the read while it is small)
        while self.table._bound > self.max_ids and self.table.used > self.max_ids:
            self.shift += 1
            self.table.purge(self.shift)

    # ------------------------------------------------------------------ the report
    def report(self, top: Optional[int] = 20, order: str = "duration", unfinished_only: bool = False,
               min_lines: int = 2, max_share: float = 0.25, min_ms: int = 0, kind_min_spans: int = 5, close_share=0.8,
               kinds: Optional[int] = 10) -> dict:
        """The report of everything added so far (more can be added afterwards)."""
        share = check_args(self.min_len, self.max_ids, order, min_lines, max_share, min_ms, kind_min_spans, close_share,
                           top, kinds)
        with self._guard():
            return self._report(top, order, bool(unfinished_only), min_lines, max_share, min_ms, kind_min_spans, share,
                                kinds)

    def _report(self, top, order, unfinished_only, min_lines, max_share, min_ms, kind_min_spans, share, kinds) -> dict:
        dev = self.table.device
        total = self.next_line
        key, count, first, last, tmin, tmax, opens, closes, toklen, tok = self.table.rows()
        ids = int(key.numel())
        timed_lines, id_lines, pairs = torch.stack([self._timed, self.levels[self.shift:].sum(), count.sum()]).tolist()
        out = spans_head(total, timed_lines, id_lines, pairs, ids, self.min_len, self.max_ids, self.shift)
        if ids == 0:
            return out
        timed = tmin <= tmax
        dur = torch.where(timed, tmax - tmin, torch.zeros_like(tmin))
        # (exact: line counts are far below 2^53, and Python compares the same way)
        keep = (count >= min_lines) & (count.double() <= max_share * total) \
            & ((timed & (dur >= min_ms)) | (~timed & (min_ms == 0)))
        key, count, first, last, tmin, tmax, opens, closes, toklen, tok, timed, dur = (
            t[keep] for t in (key, count, first, last, tmin, tmax, opens, closes, toklen, tok, timed, dur))
        n = int(key.numel())
        out["listed"] = n
        if n == 0:
            return out
        ukey = key ^ _I64_MIN                                       # the key as an unsigned number
        pow2 = torch.tensor([1 << b for b in range(SPAN_BUCKETS - 1)], dtype=torch.int64, device=dev)
        hist = torch.bincount(torch.searchsorted(pow2, dur[timed], right=True), minlength=SPAN_BUCKETS)
        # ---- kinds: the spans by `opens`; one small row per (opens, closes) comes to the host
        k_sig, inv = torch.unique(opens, return_inverse=True)
        nk = int(k_sig.numel())
        pr, pr_n = torch.unique(torch.stack([inv, closes], 1), dim=0, return_counts=True)
        k_spans = torch.bincount(inv, minlength=nk)
        k_timed = torch.bincount(inv[timed], minlength=nk)
        k_sum = torch.zeros(nk, dtype=torch.int64, device=dev).index_add_(0, inv, dur)
        k_first = torch.full((nk,), (1 << 63) - 1, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, first, "amin")
        # the longest span of every kind: the first of its timed spans by (-duration, first line, key)
        t_idx = torch.nonzero(timed).flatten()
        t_inv = inv[t_idx]
        p = _by([(t_inv, False), (dur[t_idx], True), (first[t_idx], False), (ukey[t_idx], False)], int(t_idx.numel()), dev)
        lead = torch.ones_like(p, dtype=torch.bool)
        lead[1:] = t_inv[p][1:] != t_inv[p][:-1]
        best = torch.full((nk,), -1, dtype=torch.int64, device=dev)
        best[t_inv[p][lead]] = t_idx[p][lead]
        flat = torch.cat([hist, k_sig, k_spans, k_timed, k_sum, k_first, pr[:, 0], pr[:, 1], pr_n]).tolist()
        out["durations"] = spans_durations(flat[:SPAN_BUCKETS])
        kc = [flat[SPAN_BUCKETS + c * nk: SPAN_BUCKETS + (c + 1) * nk] for c in range(5)]
        rest = flat[SPAN_BUCKETS + 5 * nk:]
        npr = len(rest) // 3
        k_closes: Dict[int, Dict[int, int]] = {}
        for i, c, cn in zip(rest[:npr], rest[npr:2 * npr], rest[2 * npr:]):
            k_closes.setdefault(i, {})[c & U64] = cn
        usual = [spans_usual_end(k_closes[i], kc[1][i], kind_min_spans, share) for i in range(nk)]
        has_usual = torch.tensor([u is not None for u in usual], dtype=torch.bool, device=dev)
        usual_sig = torch.tensor([0 if u is None else u - (1 << 64) if u >> 63 else u for u in usual], dtype=torch.int64,
                                 device=dev)
        unfinished = has_usual[inv] & (closes != usual_sig[inv])
        k_unf = torch.bincount(inv[unfinished], minlength=nk).tolist()
        # ---- the templates' first lines (the examples' ordinals): one read of the template table
        t_sig, _, t_first, _ = self.by_template.rows()
        first_of = dict(zip(*torch.stack([t_sig, t_first]).tolist()))

        def example(sig_signed: int) -> bytes:
            if sig_signed not in first_of:
                raise RuntimeError("SpanAccumulator: no line has the template %016x" % (sig_signed & U64))
            return self._examples.take(sig_signed, first_of[sig_signed])

        def signed(u: int) -> int:
            return u - (1 << 64) if u >> 63 else u

        # ---- the kinds listed
        k_order = sorted(range(nk), key=lambda i: (-k_unf[i], -kc[1][i], kc[4][i], kc[0][i] & U64))
        if kinds is not None:
            k_order = k_order[:max(0, kinds)]
        b_rows = {}
        if k_order:
            at = best[torch.tensor(k_order, dtype=torch.int64, device=dev)]
            has = at >= 0
            if bool(has.any()):
                at = at[has]
                b_dur, b_first, b_len = torch.stack([dur[at], first[at], toklen[at].long()]).tolist()
                b_tok = tok[at].cpu().numpy()
                which = [i for i, h in zip(k_order, has.tolist()) if h]
                b_rows = {i: (d, bytes(b_tok[j, :ln]).decode("ascii", errors="replace"), f)
                          for j, (i, d, f, ln) in enumerate(zip(which, b_dur, b_first, b_len))}
        try:
            for i in k_order:
                o = kc[0][i] & U64
                d, tk, f = b_rows.get(i, (None, None, None))
                raws = {s: example(signed(s)) for s in [o] + list(k_closes[i])}
                out["kinds"].append(spans_kind_row(o, kc[1][i], kc[2][i], kc[3][i], d, tk, f, kc[4][i], k_closes[i],
                                                   usual[i], k_unf[i], raws))
            # ---- top: order on the device, only the listed rows come to the host
            cand = torch.nonzero(unfinished).flatten() if unfinished_only else torch.arange(n, dtype=torch.int64, device=dev)
            if order == "duration":
                cols = [(~timed, False), (dur, True), (first, False), (ukey, False)]
            elif order == "lines":
                cols = [(count, True), (first, False), (ukey, False)]
            else:
                cols = [(first, False), (ukey, False)]
            pick = cand[_by([(c[cand], d) for c, d in cols], int(cand.numel()), dev)]
            if top is not None:
                pick = pick[:max(0, top)]
            if pick.numel():
                rows = torch.stack([key[pick], count[pick], first[pick], last[pick], tmin[pick], tmax[pick], opens[pick],
                                    closes[pick], toklen[pick].long(), timed[pick].long(), unfinished[pick].long(),
                                    inv[pick]]).tolist()
                toks = tok[pick].cpu().numpy()
                for j, (k, c, f, la, t0, t1, o, cl, ln, tm, un, ki) in enumerate(zip(*rows)):
                    if not 1 <= ln <= K.SPAN_TOK_BYTES:
                        raise RuntimeError("SpanAccumulator: %016x has a token of %d bytes" % (k & U64, ln))
                    out["top"].append(spans_row(k & U64, bytes(toks[j, :ln]), c, f, la, t0 if tm else None,
                                                t1 if tm else None, o & U64, cl & U64, bool(un), usual[ki],
                                                example(o), example(cl)))
        except ValueError as e:
            raise RuntimeError("SpanAccumulator: %s" % e) from None
        return out


def spans_document(eng: Engine, data: bytes, min_len: int = 8, max_ids: int = SPAN_MAX_IDS, **kw) -> dict:
    """The report of one document (``Engine.spans_bytes``); ``kw``: the parameters of ``report``."""
    acc = SpanAccumulator(eng, min_len, max_ids)
    check_args(min_len, max_ids, **{k: v for k, v in kw.items() if k != "unfinished_only"})
    acc.add_document(data)
    return acc.report(**kw)


def spans_stream(eng: Engine, src, chunk_bytes: Optional[int] = None, min_len: int = 8, max_ids: int = SPAN_MAX_IDS,
                 **kw) -> dict:
    """The report of ONE log in chunks: a bytes-like source (bytes, mmap, ``RepeatBuffer``) or a
    ``ResidentLog``. Exactly the one-document report, whatever the chunk size."""
    acc = SpanAccumulator(eng, min_len, max_ids)
    check_args(min_len, max_ids, **{k: v for k, v in kw.items() if k != "unfinished_only"})
    acc.add_stream(src, chunk_bytes)
    return acc.report(**kw)
