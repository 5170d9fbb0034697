"""Pure-Python golden model of the reference analysis pipeline (the test oracle).

A line-by-line re-statement of the reference's *semantics*, kept deliberately naive and
independent of the device engine (SURVEY §4, §7 phase 0). Every quirk is reproduced:

* line split ``logs.split("\\r?\\n")`` with Java trailing-empty removal (``AnalysisService.java:53``)
* event order: line, then pattern-set order, then pattern order (``AnalysisService.java:89-113``)
* context extraction, ``[i,i]`` only when rules are null (``AnalysisService.java:132-156``)
* 7-factor score, left-to-right product (``ScoringService.java:63-112``)
* chronological piecewise-linear factor (``ScoringService.java:123-151``)
* proximity: nearest secondary hit within ``min(maxWindow, proximityWindow)``, self line
  excluded, ``1 + Σ w·exp(-d/decay)`` (``ScoringService.java:161-190,315-347``)
* temporal: last event within ±5 (inclusive of i), earlier events by nearest hit strictly
  before a cursor that starts at i, unbounded backwards (``ScoringService.java:199-305``)
* context factor with ERR/WARN else-if, stack bonus, density penalty, cap
  (``ContextAnalysisService.java:46-117``)
* frequency penalty computed *before* recording the match (``ScoringService.java:84-88``,
  ``FrequencyTrackingService.java:41-93``)
* summary with ``NONE`` on empty and first-wins ties (``AnalysisService.java:188-215``)
"""
from __future__ import annotations

import math
import re
import threading
import time
import uuid
from collections import deque
from datetime import datetime, timedelta, timezone
from fractions import Fraction
from typing import Callable, Dict, List, Optional, Sequence

from .models.schema import Pattern, PatternSet, pattern_to_json
from .regex.javacompat import compile_java
from .utils.config import ScoringParams

SEVERITY_MULTIPLIERS = {"CRITICAL": 5.0, "HIGH": 3.0, "MEDIUM": 2.0, "LOW": 1.5, "INFO": 1.0}
SEVERITY_ORDER = ["INFO", "LOW", "MEDIUM", "HIGH", "CRITICAL"]

ERROR_RE = r"(?i)\b(ERROR|FATAL|CRITICAL|SEVERE)\b"
WARN_RE = r"(?i)\b(WARN|WARNING)\b"
STACK_RE = r"^\s*at\s+[\w\.\$]+\(.*\)\s*$"
EXC_RE = r"\b\w*Exception\b|\b\w*Error\b"
CONTEXT_REGEXES = (ERROR_RE, WARN_RE, STACK_RE, EXC_RE)

_SPLIT = re.compile(r"\r?\n")



def java_blank(pid) -> bool:
    """``id == null || id.trim().isEmpty()`` (FrequencyTrackingService.java:42,65). Java's
    String.trim() strips every char <= U+0020 (controls included) and nothing else: "\x01" is
    blank, a non-breaking space (U+00A0) or "\u2003" is not -- unlike Python's str.strip()."""
    return pid is None or all(ord(c) <= 0x20 for c in pid)

def split_lines(logs: str) -> List[str]:
    """Java ``String.split("\\r?\\n")`` (limit 0)."""
    if _SPLIT.search(logs) is None:
        return [logs]
    parts = _SPLIT.split(logs)
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def severity_key(sev: Optional[str]) -> str:
    return (sev or "").upper()


class FrequencyTracker:
    """Sliding-window match counter per pattern id (``FrequencyTrackingService.java:20-162``).

    ``PatternFrequency`` lives in the unavailable common-lib; semantics follow SURVEY §2.4:
    ``hourlyRate = #matches within the last W hours / W``.
    """

    def __init__(self, params: ScoringParams, clock: Callable[[], float] = time.time):
        self.params = params
        self.clock = clock
        self._ts: Dict[str, deque] = {}
        self._lock = threading.Lock()

    def _prune(self, dq: deque, now: float) -> None:
        horizon = now - self.params.freq_window_hours * 3600.0
        while dq and dq[0] <= horizon:
            dq.popleft()

    def record(self, pid: Optional[str]) -> None:
        if java_blank(pid):
            return
        with self._lock:
            self._ts.setdefault(pid, deque()).append(self.clock())

    def count(self, pid: str) -> int:
        with self._lock:
            dq = self._ts.get(pid)
            if dq is None:
                return 0
            self._prune(dq, self.clock())
            return len(dq)

    def hourly_rate(self, pid: str) -> float:
        return self.count(pid) / float(self.params.freq_window_hours)

    def penalty(self, pid: Optional[str]) -> float:
        if java_blank(pid):
            return 0.0
        with self._lock:
            if pid not in self._ts:
                return 0.0
        rate = self.hourly_rate(pid)
        thr = self.params.freq_threshold
        if rate <= thr:
            return 0.0
        return min(self.params.freq_max_penalty, (rate - thr) / thr)

    def statistics(self) -> Dict[str, int]:
        return {k: self.count(k) for k in list(self._ts)}

    def reset(self, pid: str) -> None:
        with self._lock:
            if pid in self._ts:
                self._ts[pid].clear()

    def reset_all(self) -> None:
        with self._lock:
            self._ts.clear()


def _find(regex: Optional[str], line: str) -> bool:
    if regex is None:
        return False
    return compile_java(regex).search(line) is not None


def chronological_factor(line_index: int, n_lines: int, p: ScoringParams) -> float:
    pos = float(line_index) / n_lines
    e, t = p.early_bonus_threshold, p.penalty_threshold
    if pos <= e:
        return 1.5 + (e - pos) * ((p.max_early_bonus - 1.5) / e)
    if pos <= t:
        return 1.0 + (t - pos) * (0.5 / (t - e))
    return 0.5 + (1.0 - pos)


def proximity_factor(pattern: Pattern, i: int, lines: Sequence[str], p: ScoringParams) -> float:
    secs = pattern.secondary_patterns
    if not secs:
        return 1.0
    total = 0.0
    n = len(lines)
    for s in secs:
        w = min(p.max_window, s.proximity_window)
        start, end = max(0, i - w), min(n, i + w + 1)
        best = -1.0
        for j in range(start, end):
            if j == i:
                continue
            if _find(s.regex, lines[j]):
                d = float(abs(j - i))
                if best < 0 or d < best:
                    best = d
        if best >= 0:
            total += s.weight * math.exp(-best / p.decay_constant)
    return 1.0 + total


def _sequence_matched(seq, i: int, lines: Sequence[str]) -> bool:
    events = seq.events
    if not events:
        return False
    n = len(lines)
    cursor = 0
    for k in range(len(events) - 1, -1, -1):
        rx = events[k].regex
        if k == len(events) - 1:
            start, end = max(0, i - 5), min(n, i + 5 + 1)
            if not any(_find(rx, lines[j]) for j in range(start, end)):
                return False
            cursor = i
        else:
            found = -1
            for j in range(cursor - 1, -1, -1):
                if _find(rx, lines[j]):
                    found = j
                    break
            if found < 0:
                return False
            cursor = found
    return True


def temporal_factor(pattern: Pattern, i: int, lines: Sequence[str]) -> float:
    seqs = pattern.sequence_patterns
    if not seqs:
        return 1.0
    total = 0.0
    for s in seqs:
        if _sequence_matched(s, i, lines):
            total += s.bonus_multiplier
    return 1.0 + total


def context_factor(ctx_lines: Optional[List[str]], p: ScoringParams) -> float:
    if not ctx_lines:
        return 1.0
    score = 0.0
    err = stack = 0
    for line in ctx_lines:
        if _find(ERROR_RE, line):
            err += 1
            score += 0.4
        elif _find(WARN_RE, line):
            score += 0.2
        if _find(STACK_RE, line):
            stack += 1
            score += 0.1
        if _find(EXC_RE, line):
            score += 0.3
    if stack > 0:
        score += min(stack * 0.1, 0.5)
    total = len(ctx_lines)
    if total > 10 and (stack + err) > total * 0.7:
        score *= 0.8
    f = 1.0 + score
    if f > p.max_context_factor:
        f = p.max_context_factor
    return f


def extract_context(lines: Sequence[str], i: int, rules) -> dict:
    ctx = {"matchedLine": lines[i], "linesBefore": None, "linesAfter": None}
    if rules is None:
        return ctx
    before = max(0, rules.lines_before)
    after = max(0, rules.lines_after)
    ctx["linesBefore"] = list(lines[max(0, i - before):i])
    ctx["linesAfter"] = list(lines[i + 1:min(len(lines), i + 1 + after)])
    return ctx


def _ctx_lines(ctx: dict) -> List[str]:
    out: List[str] = []
    if ctx["linesBefore"] is not None:
        out.extend(ctx["linesBefore"])
    if ctx["matchedLine"] is not None:
        out.append(ctx["matchedLine"])
    if ctx["linesAfter"] is not None:
        out.extend(ctx["linesAfter"])
    return out


def score_event(pattern: Pattern, i: int, lines: Sequence[str], ctx: dict,
                p: ScoringParams, freq: FrequencyTracker) -> float:
    conf = pattern.primary_pattern.confidence
    sev = SEVERITY_MULTIPLIERS.get(severity_key(pattern.severity), 1.0)
    chrono = chronological_factor(i, len(lines), p)
    prox = proximity_factor(pattern, i, lines, p)
    temp = temporal_factor(pattern, i, lines)
    ctxf = context_factor(_ctx_lines(ctx), p)
    pen = freq.penalty(pattern.id)
    freq.record(pattern.id)
    return conf * sev * chrono * prox * temp * ctxf * (1.0 - pen)


def build_summary(events: List[dict]) -> dict:
    if not events:
        return {"significantEvents": 0, "highestSeverity": "NONE", "severityDistribution": {}}
    dist: Dict[str, int] = {}
    best = None
    best_idx = -2
    for e in events:
        s = severity_key(e["matchedPattern"].get("severity"))
        dist[s] = dist.get(s, 0) + 1
        idx = SEVERITY_ORDER.index(s) if s in SEVERITY_ORDER else -1
        if idx > best_idx:
            best_idx, best = idx, s
    return {"significantEvents": len(events), "highestSeverity": best, "severityDistribution": dist}


def analyze(logs: str, pattern_sets: List[PatternSet], params: ScoringParams,
            freq: FrequencyTracker) -> dict:
    """``AnalysisService.analyze`` (``AnalysisService.java:50-122``)."""
    t0 = time.time()
    lines = split_lines(logs)
    events: List[dict] = []
    for li, line in enumerate(lines):
        for ps in pattern_sets:
            for pat in (ps.patterns or []):
                if pat.primary_pattern is None or not _find(pat.primary_pattern.regex, line):
                    continue
                ctx = extract_context(lines, li, pat.context_extraction)
                sc = score_event(pat, li, lines, ctx, params, freq)
                events.append({"lineNumber": li + 1, "matchedPattern": pattern_to_json(pat),
                               "context": ctx, "score": sc})
    meta = {
        "processingTimeMs": int((time.time() - t0) * 1000),
        "totalLines": len(lines),
        "analyzedAt": datetime.now(timezone.utc).isoformat().replace("+00:00", "Z"),
        "patternsUsed": [(ps.metadata.library_id if ps.metadata else None) for ps in pattern_sets],
    }
    return {"analysisId": str(uuid.uuid4()), "metadata": meta, "events": events,
            "summary": build_summary(events)}


# ---------------------------------------------------------------------------------------------
# Coverage-gap report (an extra: the reference has nothing like it). Which error lines of a log
# does no pattern explain, grouped by shape? These functions are the specification of
# ``Engine.gaps_bytes`` and of the template-signature kernel (csrc/kernels/gaps_core.h).
#
# Known limits: a hex token without a digit ("deadbeef") is kept as it is, and two different
# templates may share a 64-bit signature (their lines are then reported as one group).

SIG_MAX_BYTES = 1024
_FNV_OFFSET = 0xcbf29ce484222325
_FNV_PRIME = 0x100000001b3
_TOKEN = re.compile(rb"[0-9A-Za-z]+")
_DIGIT = re.compile(rb"[0-9]")
_BLANKS = re.compile(rb"[ \t]+")


def line_template(line: bytes) -> bytes:
    """Shape of a line: of its first ``SIG_MAX_BYTES`` bytes, every maximal ``[0-9A-Za-z]`` run
    (ASCII) holding a digit becomes ``0``, then every run of space / tab one space; every other
    byte (bytes >= 0x80 included) is kept."""
    s = bytes(line[:SIG_MAX_BYTES])
    s = _TOKEN.sub(lambda m: b"0" if _DIGIT.search(m.group()) else m.group(), s)
    return _BLANKS.sub(b" ", s)


def line_signature(line: bytes) -> int:
    """FNV-1a-64 of ``line_template(line)``."""
    h = _FNV_OFFSET
    for c in line_template(line):
        h = ((h ^ c) * _FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h


def gap_candidate(line: str) -> bool:
    """An error keyword or an exception / error class name, and not a stack frame."""
    return (_find(ERROR_RE, line) or _find(EXC_RE, line)) and not _find(STACK_RE, line)


def _gap_groups(logs, pattern_sets: List[PatternSet], params: ScoringParams, cover: str):
    """One document's part of the report: (lines, events, candidates, uncovered candidates,
    {signature: [count, first line (0-based), raw first line]})."""
    if cover not in ("events", "context"):
        raise ValueError("cover must be 'events' or 'context'")
    if isinstance(logs, (bytes, bytearray, memoryview)):
        logs = bytes(logs).decode("utf-8", errors="surrogateescape")
    res = analyze(logs, pattern_sets, params, FrequencyTracker(params))
    lines = split_lines(logs)
    covered = [False] * len(lines)
    for e in res["events"]:
        x = e["lineNumber"] - 1
        a, b = x, x + 1
        if cover == "context":
            a -= len(e["context"]["linesBefore"] or ())
            b += len(e["context"]["linesAfter"] or ())
        for i in range(a, b):
            covered[i] = True
    groups: Dict[int, list] = {}
    n_cand = n_sel = 0
    for i, line in enumerate(lines):
        if not gap_candidate(line):
            continue
        n_cand += 1
        if covered[i]:
            continue
        n_sel += 1
        raw = line.encode("utf-8", errors="surrogateescape")
        g = groups.setdefault(line_signature(raw), [0, i, raw])
        g[0] += 1
    return len(lines), len(res["events"]), n_cand, n_sel, groups


def _gap_group_fields(sig: int, count: int, line: int, raw: bytes) -> dict:
    return {"count": count, "firstLine": line + 1, "signature": "%016x" % sig,
            "template": line_template(raw).decode("utf-8", errors="replace"),
            "example": raw.decode("utf-8", errors="replace")}


def gaps(logs, pattern_sets: List[PatternSet], params: ScoringParams, top: Optional[int] = 20,
         cover: str = "context") -> dict:
    """The gap report from ``analyze``'s events: candidate lines (``gap_candidate``) that no event
    covers -- ``cover="events"``: the events' own lines; ``"context"``: their context windows too
    -- grouped by ``line_signature``, most frequent first (ties: first line)."""
    n_lines, n_events, n_cand, n_sel, groups = _gap_groups(logs, pattern_sets, params, cover)
    order = sorted(groups.items(), key=lambda kv: (-kv[1][0], kv[1][1]))
    if top is not None:
        order = order[:max(0, int(top))]
    return {"totalLines": n_lines, "events": n_events, "errorLines": n_cand,
            "uncoveredErrorLines": n_sel, "templates": len(groups),
            "top": [_gap_group_fields(sig, c, i, raw) for sig, (c, i, raw) in order]}


def gaps_corpus(docs, pattern_sets: List[PatternSet], params: ScoringParams, top: Optional[int] = 20,
                cover: str = "context") -> dict:
    """The gap report of a corpus: every document (str or bytes) is analysed on its own -- no
    context window and no template crosses a document border -- and the groups are merged by
    signature. Exactly one document: ``gaps`` of it. Otherwise the totals are summed, and
    ``documents`` counts the documents; every group also carries ``documents`` (how many
    documents it occurs in) and ``firstDocument`` (0-based; ``firstLine`` is 1-based within it).
    Most frequent first, ties by (first document, first line)."""
    docs = list(docs)
    if len(docs) == 1:
        return gaps(docs[0], pattern_sets, params, top, cover)
    tot = [0, 0, 0, 0]
    merged: Dict[int, list] = {}                # signature -> [count, first document, first line, raw, documents]
    for d, logs in enumerate(docs):
        *nums, groups = _gap_groups(logs, pattern_sets, params, cover)
        tot = [a + b for a, b in zip(tot, nums)]
        for sig, (c, i, raw) in groups.items():
            g = merged.setdefault(sig, [0, d, i, raw, 0])
            g[0] += c
            g[4] += 1
    order = sorted(merged.items(), key=lambda kv: (-kv[1][0], kv[1][1], kv[1][2]))
    if top is not None:
        order = order[:max(0, int(top))]
    return {"totalLines": tot[0], "events": tot[1], "errorLines": tot[2], "uncoveredErrorLines": tot[3],
            "templates": len(merged), "top": [
                {**_gap_group_fields(sig, c, i, raw), "documents": nd, "firstDocument": d}
                for sig, (c, d, i, raw, nd) in order], "documents": len(docs)}


# ---------------------------------------------------------------------------------------------
# Novelty report (an extra, as the gap report): what does a log say that a baseline of healthy
# logs never said? A line is *novel* when its template signature is not among the signatures of
# the baseline's lines. These functions are the specification of ``log_parser_amd/novelty.py`` and
# of the kernel that signs, probes and compacts in one pass (csrc/kernels/novelty.hip).
#
# Known limits are the signatures': two templates may share a 64-bit signature, and only the first
# ``SIG_MAX_BYTES`` bytes of a line count.

def _as_text(logs) -> str:
    if isinstance(logs, (bytes, bytearray, memoryview)):
        return bytes(logs).decode("utf-8", errors="surrogateescape")
    return logs


def baseline_signatures(docs):
    """(set of signatures, lines, documents) of the baseline documents (str or bytes): every line
    of every document (``split_lines``) contributes ``line_signature``; an empty line signs as the
    empty template."""
    sigs, n_lines, n_docs = set(), 0, 0
    for d in docs:
        n_docs += 1
        for line in split_lines(_as_text(d)):
            n_lines += 1
            sigs.add(line_signature(line.encode("utf-8", errors="surrogateescape")))
    return sigs, n_lines, n_docs


def novelty(logs, baseline_docs, pattern_sets: List[PatternSet], params: ScoringParams, top: Optional[int] = 20,
            order: str = "count", errors_only: bool = False) -> dict:
    """The novelty report of ``logs`` against the baseline documents: the lines whose signature
    the baseline does not hold, grouped by signature. Per group: its lines (``count``), those that
    are ``gap_candidate`` (``errorLines``), those an event of ``analyze`` lies on (``eventLines``:
    the event's own line, not its context window) and its first line. ``order="count"``: most
    frequent first (ties: first line); ``"first"``: by first line -- the first new thing that
    happened. ``errors_only`` lists only the groups with error lines; the totals do not change."""
    if order not in ("count", "first"):
        raise ValueError("order must be 'count' or 'first'")
    base, b_lines, b_docs = baseline_signatures(baseline_docs)
    logs = _as_text(logs)
    res = analyze(logs, pattern_sets, params, FrequencyTracker(params))
    lines = split_lines(logs)
    on_event = {e["lineNumber"] - 1 for e in res["events"]}
    groups: Dict[int, list] = {}                # signature -> [count, error lines, event lines, first line, raw]
    n_cand = n_novel = n_novel_cand = 0
    for i, line in enumerate(lines):
        cand = bool(gap_candidate(line))
        n_cand += cand
        raw = line.encode("utf-8", errors="surrogateescape")
        sig = line_signature(raw)
        if sig in base:
            continue
        n_novel += 1
        n_novel_cand += cand
        g = groups.setdefault(sig, [0, 0, 0, i, raw])
        g[0] += 1
        g[1] += cand
        g[2] += i in on_event
    listed = [kv for kv in groups.items() if kv[1][1] or not errors_only]
    listed.sort(key=(lambda kv: (-kv[1][0], kv[1][3])) if order == "count" else (lambda kv: kv[1][3]))
    if top is not None:
        listed = listed[:max(0, int(top))]
    return {"totalLines": len(lines), "events": len(res["events"]), "errorLines": n_cand,
            "novelLines": n_novel, "novelErrorLines": n_novel_cand,
            "templates": len(groups), "errorTemplates": sum(1 for g in groups.values() if g[1]),
            "baseline": {"documents": b_docs, "lines": b_lines, "templates": len(base)},
            "top": [{"count": c, "errorLines": ce, "eventLines": cv, "firstLine": i + 1, "signature": "%016x" % sig,
                     "template": line_template(raw).decode("utf-8", errors="replace"),
                     "example": raw.decode("utf-8", errors="replace")}
                    for sig, (c, ce, cv, i, raw) in listed]}


# ---------------------------------------------------------------------------------------------
# Lead-up report (an extra, as the gap report): what does a log say just before its failures that
# it does not usually say? A line is *in the lead-up* when an event of ``analyze`` lies on one of
# the ``window`` lines after it. The templates of these lines are weighed against all the lines of
# the same template. This function is the specification of ``log_parser_amd/leadup.py`` and of the
# kernel that signs every line and marks the lead-up in one pass (csrc/kernels/leadup.hip).
#
# Known limits are the signatures': two templates may share a 64-bit signature, and only the first
# ``SIG_MAX_BYTES`` bytes of a line count.

LEAD_MAX_WINDOW = 4096


def leadup(logs, pattern_sets: List[PatternSet], params: ScoringParams, window: int = 50, top: Optional[int] = 20,
           order: str = "share", min_count: int = 2) -> dict:
    """The lead-up report of ``logs``. ``E``: the lines that carry at least one event. A line ``x``
    is in the lead-up iff some ``e`` in ``E`` has ``x < e <= x + window`` -- an event line is not in
    its own lead-up, but can be in a later event's. Lines are grouped by ``line_signature``; per
    group ``total`` (its lines in the log), ``count`` (those in the lead-up), ``share`` = count /
    total, ``lift`` = share against the lead-up's share of all lines, and its first lead-up line.
    Listed are the groups with ``count >= min_count``: ``order="share"`` by (-share, -count, first
    line), ``"count"`` by (-count, first line), ``"first"`` by first line."""
    if order not in ("share", "count", "first"):
        raise ValueError("order must be 'share', 'count' or 'first'")
    if not 1 <= window <= LEAD_MAX_WINDOW:
        raise ValueError("window must be 1..%d" % LEAD_MAX_WINDOW)
    if min_count < 1:
        raise ValueError("min_count must be at least 1")
    logs = _as_text(logs)
    res = analyze(logs, pattern_sets, params, FrequencyTracker(params))
    lines = split_lines(logs)
    E = sorted({e["lineNumber"] - 1 for e in res["events"]})
    lead = [False] * len(lines)
    for e in E:
        for x in range(max(0, e - window), e):
            lead[x] = True
    groups: Dict[int, list] = {}                # signature -> [total, count, first lead-up line, raw of it]
    for i, line in enumerate(lines):
        raw = line.encode("utf-8", errors="surrogateescape")
        g = groups.setdefault(line_signature(raw), [0, 0, None, None])
        g[0] += 1
        if lead[i]:
            g[1] += 1
            if g[2] is None:
                g[2], g[3] = i, raw
    n_lead = sum(lead)
    listed = [kv for kv in groups.items() if kv[1][1] >= min_count]
    listed.sort(key={"share": lambda kv: (-(kv[1][1] / kv[1][0]), -kv[1][1], kv[1][2]),
                     "count": lambda kv: (-kv[1][1], kv[1][2]),
                     "first": lambda kv: kv[1][2]}[order])
    if top is not None:
        listed = listed[:max(0, int(top))]
    return {"totalLines": len(lines), "events": len(res["events"]), "eventLines": len(E), "window": window,
            "leadLines": n_lead, "templates": sum(1 for g in groups.values() if g[1]),
            "top": [{"count": c, "total": t, "share": c / t, "lift": (c * len(lines)) / (t * n_lead),
                     "firstLine": i + 1, "signature": "%016x" % sig,
                     "template": line_template(raw).decode("utf-8", errors="replace"),
                     "example": raw.decode("utf-8", errors="replace")}
                    for sig, (t, c, i, raw) in listed]}


# ---------------------------------------------------------------------------------------------
# Correlation report (an extra, as the gap report): the failing line carries a request id, a trace
# id, a pod hash or an address -- what else did the log say about that id? The lead-up is
# positional; in a concurrent service the lines of the failed request are interleaved with
# everyone else's, and this report follows the id instead. These functions are the specification
# of ``log_parser_amd/correlate.py`` and of the key kernel (csrc/kernels/key_core.h, correlate.hip).
#
# Known limits: two tokens may share a 64-bit key; only the first ``SIG_MAX_BYTES`` bytes of a line
# and its first ``KEY_PER_LINE`` distinct keys count; an id with ``-`` or ``_`` inside is several
# tokens (a UUID gives two keys, its 8-byte and its 12-byte group).

KEY_MIN_LEN = 4
KEY_MAX_LEN = 64
KEY_PER_LINE = 8


def line_key_tokens(line: bytes, min_len: int = 8) -> List[tuple]:
    """[(key, lowered token)] of a line: of its first ``SIG_MAX_BYTES`` bytes (a run still open
    there ends there), every maximal ``[0-9A-Za-z]`` run of ``min_len .. KEY_MAX_LEN`` bytes that
    holds a digit is a key token; its key is FNV-1a-64 of the token with ASCII letters lowered.
    The first ``KEY_PER_LINE`` distinct keys in byte order; a further one is ignored."""
    out, seen = [], set()
    for m in _TOKEN.finditer(bytes(line[:SIG_MAX_BYTES])):
        t = m.group()
        if not min_len <= len(t) <= KEY_MAX_LEN or not _DIGIT.search(t):
            continue
        t = t.lower()
        k = fnv1a64(t)
        if k in seen:
            continue
        if len(out) == KEY_PER_LINE:
            break
        seen.add(k)
        out.append((k, t))
    return out


def line_keys(line: bytes, min_len: int = 8) -> List[int]:
    """The keys of a line (``line_key_tokens``) as unsigned 64-bit numbers."""
    return [k for k, _ in line_key_tokens(line, min_len)]


def correlate_check_args(min_len: int = 8, order: str = "events", min_lines: int = 2, max_share: float = 0.25) -> None:
    if order not in ("events", "lines", "first"):
        raise ValueError("order must be 'events', 'lines' or 'first'")
    if not KEY_MIN_LEN <= min_len <= KEY_MAX_LEN:
        raise ValueError("min_len must be %d..%d" % (KEY_MIN_LEN, KEY_MAX_LEN))
    if min_lines < 1:
        raise ValueError("min_lines must be at least 1")
    if not 0.0 < max_share <= 1.0:
        raise ValueError("max_share must be in (0, 1]")


def correlate(logs, pattern_sets: List[PatternSet], params: ScoringParams, min_len: int = 8,
              top: Optional[int] = 20, order: str = "events", min_lines: int = 2, max_share: float = 0.25) -> dict:
    """The correlation report of ``logs``. The *event keys* are the keys (``line_keys``) of the
    lines that carry an event of ``analyze``. Per event key: ``eventLines`` (distinct event lines
    holding it), ``lines`` (all lines holding it, event lines included), ``share`` = eventLines /
    lines, its first and last line, its first event line, the lowered token and the first line as
    the example. Dropped are the keys with ``lines < min_lines`` (an id seen only on its own event
    line correlates nothing) and those with ``lines > max_share * totalLines`` (a host name on
    every line correlates everything). ``order="events"``: by (-eventLines, -lines, first line,
    key); ``"lines"``: (-lines, -eventLines, first line, key); ``"first"``: (first event line,
    key). ``keys`` counts the event keys before the filters, ``keyLines`` the lines that hold at
    least one."""
    correlate_check_args(min_len, order, min_lines, max_share)
    logs = _as_text(logs)
    res = analyze(logs, pattern_sets, params, FrequencyTracker(params))
    raws = [line.encode("utf-8", errors="surrogateescape") for line in split_lines(logs)]
    E = sorted({e["lineNumber"] - 1 for e in res["events"]})
    groups: Dict[int, list] = {}        # key -> [event lines, first event line, lines, first line, last line]
    for e in E:
        for k in line_keys(raws[e], min_len):
            groups.setdefault(k, [0, e, 0, None, None])[0] += 1
    key_lines = 0
    for i, raw in enumerate(raws):
        held = [k for k in line_keys(raw, min_len) if k in groups] if groups else []
        key_lines += bool(held)
        for k in held:
            g = groups[k]
            g[2] += 1
            if g[3] is None:
                g[3] = i
            g[4] = i
    listed = [kv for kv in groups.items() if min_lines <= kv[1][2] <= max_share * len(raws)]
    listed.sort(key={"events": lambda kv: (-kv[1][0], -kv[1][2], kv[1][3], kv[0]),
                     "lines": lambda kv: (-kv[1][2], -kv[1][0], kv[1][3], kv[0]),
                     "first": lambda kv: (kv[1][1], kv[0])}[order])
    if top is not None:
        listed = listed[:max(0, int(top))]
    return {"totalLines": len(raws), "events": len(res["events"]), "eventLines": len(E), "minLength": min_len,
            "keys": len(groups), "keyLines": key_lines,
            "top": [correlate_row(k, ne, fe, n, f, last, raws[f], min_len) for k, (ne, fe, n, f, last) in listed]}


def correlate_row(key: int, event_lines: int, first_event: int, lines: int, first: int, last: int, raw: bytes,
                  min_len: int) -> dict:
    """One row of the report from its numbers (lines 0-based) and the first line holding the key:
    the token is the one of that line whose hash is the key. ValueError if none has it."""
    tok = dict(line_key_tokens(raw, min_len)).get(key)
    if tok is None:
        raise ValueError("correlate: line %d does not hold the key %016x" % (first + 1, key))
    return {"key": tok.decode("ascii"), "eventLines": event_lines, "lines": lines, "share": event_lines / lines,
            "firstLine": first + 1, "lastLine": last + 1, "firstEventLine": first_event + 1,
            "signature": "%016x" % key, "example": raw.decode("utf-8", errors="replace")}


# ---------------------------------------------------------------------------------------------
# Log timeline (an extra: the reference reads no time a log line carries). When did the lines, the
# error lines and the events of a log happen? These functions are the specification of
# ``Engine.timeline_bytes`` and of the timestamp kernel (csrc/kernels/ts_core.h).
#
# Not covered: stamps without a year or with month names (klog ``E0919 12:00:00``, syslog
# ``Sep 19 12:00:00``, Apache ``19/Sep/2025:12:00:00``) and bare epoch numbers.

TS_MAX_START = 32
_STAMP = re.compile(rb"(?<![0-9A-Za-z])(\d{4})[-/](\d\d)[-/](\d\d)[T ](\d\d):(\d\d):(\d\d)"
                    rb"(?:[.,](\d{1,9}))?(Z|[+-]\d\d:?\d\d)?")
_EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)


def line_timestamp(line: bytes) -> Optional[int]:
    """Epoch milliseconds (UTC) of the stamp at the head of ``line``, or None: the leftmost match
    of the grammar, which must start before byte ``TS_MAX_START`` and hold valid fields (year >=
    1970, Gregorian month lengths, zone hour <= 23) -- later positions are not tried. The fraction
    is truncated to milliseconds; no zone and ``Z`` mean UTC, ``+hh:mm`` / ``+hhmm`` is subtracted."""
    m = _STAMP.search(bytes(line))
    if m is None or m.start() >= TS_MAX_START:
        return None
    y, mo, d, h, mi, s = (int(m.group(k)) for k in range(1, 7))
    if y < 1970 or h > 23 or mi > 59 or s > 59:
        return None
    try:
        t = datetime(y, mo, d, h, mi, s, tzinfo=timezone.utc)
    except ValueError:                                      # month 13, February 30, ...
        return None
    ms = (t - _EPOCH) // timedelta(milliseconds=1)
    if m.group(7):
        ms += int(m.group(7)[:3].ljust(3, b"0"))
    z = m.group(8)
    if z and z != b"Z":
        zh, zm = int(z[1:3]), int(z[-2:])
        if zh > 23 or zm > 59:
            return None
        ms -= (-1 if z[:1] == b"-" else 1) * (zh * 60 + zm) * 60000
    return ms


def iso_ms(t: int) -> str:
    """``YYYY-MM-DDTHH:MM:SS.mmmZ`` of epoch milliseconds."""
    d = _EPOCH + timedelta(milliseconds=t)
    return "%04d-%02d-%02dT%02d:%02d:%02d.%03dZ" % (d.year, d.month, d.day, d.hour, d.minute, d.second,
                                                    d.microsecond // 1000)


def timeline_span_error(first: int, last: int, W: int, max_buckets: int) -> ValueError:
    """The error of a document whose first and last bucket (starts ``first`` / ``last``) are more
    than ``max_buckets`` buckets apart."""
    return ValueError("timeline: the log spans %d buckets of %g s (%s .. %s), more than max_buckets=%d; "
                      "use a larger bucket" % ((last - first) // W + 1, W / 1000, iso_ms(first), iso_ms(last),
                                               max_buckets))


def timeline(logs, pattern_sets: List[PatternSet], params: ScoringParams, bucket_seconds: int = 60,
             max_buckets: int = 65536) -> dict:
    """The timeline report of one document. A line's effective time is its own stamp
    (``line_timestamp``), else the stamp of the nearest earlier stamped line; lines before the first
    stamped line are undated. Lines, error lines (``gap_candidate``), events (``analyze``) and the
    events' severities are counted per bucket of ``bucket_seconds``, aligned to multiples of it."""
    if isinstance(bucket_seconds, bool) or not isinstance(bucket_seconds, int) or bucket_seconds < 1:
        raise ValueError("timeline: bucket_seconds must be an integer >= 1")
    if isinstance(logs, (bytes, bytearray, memoryview)):
        logs = bytes(logs).decode("utf-8", errors="surrogateescape")
    res = analyze(logs, pattern_sets, params, FrequencyTracker(params))
    lines = split_lines(logs)
    W = 1000 * bucket_seconds
    own = [line_timestamp(l.encode("utf-8", errors="surrogateescape")) for l in lines]
    eff: List[Optional[int]] = []
    cur = top = None
    out_of_order = 0
    for t in own:
        if t is not None:
            if top is not None and t < top:
                out_of_order += 1
            top = t if top is None else max(top, t)
            cur = t
        eff.append(cur)
    stamps = [t for t in own if t is not None]
    events = res["events"]
    out = {"totalLines": len(lines), "stampedLines": len(stamps), "undatedLines": sum(t is None for t in eff),
           "outOfOrderLines": out_of_order,
           "firstTimestamp": iso_ms(min(stamps)) if stamps else None,
           "lastTimestamp": iso_ms(max(stamps)) if stamps else None,
           "bucketSeconds": bucket_seconds, "events": len(events),
           "undatedEvents": sum(eff[e["lineNumber"] - 1] is None for e in events),
           "firstErrorLine": None, "firstEvent": None, "lastEvent": None, "buckets": []}
    if not stamps:
        return out
    first, last = min(stamps) // W * W, max(stamps) // W * W
    if (last - first) // W + 1 > max_buckets:
        raise timeline_span_error(first, last, W, max_buckets)
    buckets: Dict[int, dict] = {}
    for i, line in enumerate(lines):
        if eff[i] is None:
            continue
        b = buckets.setdefault(eff[i] // W * W, {"lines": 0, "errorLines": 0, "events": 0, "severity": {}})
        b["lines"] += 1
        if gap_candidate(line):
            b["errorLines"] += 1
            if out["firstErrorLine"] is None:
                out["firstErrorLine"] = {"lineNumber": i + 1, "timestamp": iso_ms(eff[i])}
    for e in events:
        t = eff[e["lineNumber"] - 1]
        if t is None:
            continue
        b = buckets[t // W * W]
        b["events"] += 1
        s = severity_key(e["matchedPattern"].get("severity"))
        b["severity"][s] = b["severity"].get(s, 0) + 1
        ref = {"lineNumber": e["lineNumber"], "patternId": e["matchedPattern"].get("id"), "timestamp": iso_ms(t)}
        if out["firstEvent"] is None:
            out["firstEvent"] = ref
        out["lastEvent"] = ref
    out["buckets"] = [{"start": iso_ms(t), **buckets[t]} for t in sorted(buckets)]
    return out


# ---------------------------------------------------------------------------------------------
# Values report (an extra, as the gap report): every other report throws the numbers of a line
# away -- ``line_template`` turns each digit-holding token into ``0``. This one keeps them: per
# template and field, how many values, their sum, smallest and largest, where the largest is, so
# that the ``served in 31874ms`` among ten thousand ``served in 12ms`` comes first. These functions
# are the specification of ``log_parser_amd/values.py`` and of the value kernel
# (csrc/kernels/val_core.h, values.hip).
#
# Known limits: no signs; a decimal (``12.5``) is two fields; only the stamps of ``line_timestamp``
# are skipped; the unit is ignored, so ``2s`` and ``15ms`` in one field mix; a hex value without a
# digit behind its ``x`` (``0xff``) reads as 0 on that line; two (template, field) pairs may share
# a 64-bit key; only the first ``SIG_MAX_BYTES`` bytes of a line and its first ``VAL_PER_LINE``
# fields count.

VAL_PER_LINE = 8
VAL_MAX_LINES = 1 << 32         # a log has fewer lines than this (the packed ordinals of values.py)
_VALUE = re.compile(rb"([0-9]{1,9})[A-Za-z]{0,3}")


def stamp_end(line: bytes) -> int:
    """The end of the ``_STAMP`` match where ``line_timestamp(line)`` is not None, else 0: an
    invalid stamp hides nothing."""
    line = bytes(line)
    return 0 if line_timestamp(line) is None else _STAMP.search(line).end()


def line_fields(line: bytes) -> List[tuple]:
    """[(j, value or None, token)]: the *fields* of a line are the digit-holding tokens (maximal
    ``[0-9A-Za-z]`` runs, as in ``line_template``) of its first ``SIG_MAX_BYTES`` bytes (a token
    still open there ends there) that START at byte ``stamp_end(line)`` or later, in byte order,
    numbered j = 0, 1, ...; only the first ``VAL_PER_LINE`` count. A field has a value iff its
    token is ``[0-9]{1,9}[A-Za-z]{0,3}`` from start to end: the integer of the digit prefix."""
    line = bytes(line)
    q = stamp_end(line)
    out = []
    for m in _TOKEN.finditer(line[:SIG_MAX_BYTES]):
        t = m.group()
        if m.start() < q or not _DIGIT.search(t):
            continue
        if len(out) == VAL_PER_LINE:
            break
        v = _VALUE.fullmatch(t)
        out.append((len(out), int(v.group(1)) if v else None, t))
    return out


def line_values(line: bytes) -> List[tuple]:
    """[(j, value)] of the fields of a line (``line_fields``) that have a value."""
    return [(j, v) for j, v, _ in line_fields(line) if v is not None]


def val_key(sig: int, j: int) -> int:
    """The 64-bit group key of field ``j`` of the template with signature ``sig``."""
    return ((sig ^ (j + 1)) * _FNV_PRIME) & 0xFFFFFFFFFFFFFFFF


def values_check_args(order: str = "peak", min_count: int = 5, min_fill: float = 0.9) -> None:
    if order not in ("peak", "max", "count", "first"):
        raise ValueError("order must be 'peak', 'max', 'count' or 'first'")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
        raise ValueError("min_count must be an integer >= 1")
    if isinstance(min_fill, bool) or not isinstance(min_fill, (int, float)) or not 0.0 <= min_fill <= 1.0:
        raise ValueError("min_fill must be in [0, 1]")


def values_order_key(order: str, sig: int, j: int, count: int, total: int, vmax: int, first: int):
    """The sort key of a group: exact arithmetic (ints and ``Fraction``), ``sig`` unsigned."""
    if order == "peak":
        return ((0, -Fraction(vmax * count, total)) if total else (1, 0), -vmax, first, sig, j)
    if order == "max":
        return (-vmax, first, sig, j)
    if order == "count":
        return (-count, first, sig, j)
    return (first, j)


def values_row(sig: int, j: int, count: int, total: int, vmin: int, vmax: int, max_line: int, first: int,
               first_value: int, last: int, last_value: int, lines: int, raw: bytes) -> dict:
    """One row of the report from its numbers (lines 0-based) and the first line with a value of
    the group: ValueError unless that line has the template ``sig`` and holds ``first_value`` in
    field ``j``."""
    if line_signature(raw) != sig or (j, first_value) not in line_values(raw):
        raise ValueError("values: line %d does not hold field %d of %016x with the value %d"
                         % (first + 1, j, sig, first_value))
    return {"signature": "%016x" % sig, "field": j, "token": line_fields(raw)[j][2].decode("ascii"),
            "count": count, "lines": lines, "fill": count / lines, "sum": total, "min": vmin, "max": vmax,
            "mean": total / count, "peak": (vmax * count / total) if total else 0.0,
            "maxLine": max_line + 1, "firstLine": first + 1, "first": first_value,
            "lastLine": last + 1, "last": last_value,
            "template": line_template(raw).decode("utf-8", errors="replace"),
            "example": raw.decode("utf-8", errors="replace")}


def values(logs, top: Optional[int] = 20, order: str = "peak", min_count: int = 5, min_fill: float = 0.9,
           varying: bool = True) -> dict:
    """The values report of ``logs`` (str or bytes; no pattern takes part). A *group* is (template
    signature of the line, field number j). Per group: ``count`` values, their exact ``sum``,
    ``min``, ``max``, ``maxLine`` (the first line that holds the max), ``firstLine`` / ``first``
    and ``lastLine`` / ``last`` (the first / last line with a value, and that value), ``lines``
    (all lines of the template), ``fill`` = count / lines, ``mean``, ``peak`` = max * count / sum
    (the largest value in units of the mean; 0.0 when the sum is 0), the field's ``token`` on the
    first line and that line as the ``example``. Dropped are the groups with ``count <
    min_count``, those with ``count < min_fill * lines`` (a hex or id field that only now and then
    looks like a number) and, with ``varying``, those with ``min == max``. ``order="peak"``: by
    (-peak, -max, first line, signature, field), a zero sum last; ``"max"``: (-max, first line,
    signature, field); ``"count"``: (-count, ...); ``"first"``: (first line, field). ``values``
    counts all values, ``valueLines`` the lines with at least one, ``templates`` the templates of
    all lines, ``fields`` the groups before the filters."""
    values_check_args(order, min_count, min_fill)
    raws = [line.encode("utf-8", errors="surrogateescape") for line in split_lines(_as_text(logs))]
    if len(raws) >= VAL_MAX_LINES:
        raise ValueError("values: a log of 2^32 lines or more")
    per_sig: Dict[int, int] = {}
    groups: Dict[tuple, dict] = {}
    n_values = value_lines = 0
    for i, raw in enumerate(raws):
        sig = line_signature(raw)
        per_sig[sig] = per_sig.get(sig, 0) + 1
        vals = line_values(raw)
        n_values += len(vals)
        value_lines += bool(vals)
        for j, v in vals:
            g = groups.get((sig, j))
            if g is None:
                g = groups[(sig, j)] = {"count": 0, "sum": 0, "min": v, "max": v, "maxLine": i, "first": i,
                                        "firstValue": v}
            g["count"] += 1
            g["sum"] += v
            g["min"] = min(g["min"], v)
            if v > g["max"]:
                g["max"], g["maxLine"] = v, i
            g["last"], g["lastValue"] = i, v
    listed = [kv for kv in groups.items()
              if kv[1]["count"] >= min_count and kv[1]["count"] >= min_fill * per_sig[kv[0][0]]
              and (not varying or kv[1]["min"] < kv[1]["max"])]
    listed.sort(key=lambda kv: values_order_key(order, kv[0][0], kv[0][1], kv[1]["count"], kv[1]["sum"], kv[1]["max"],
                                                kv[1]["first"]))
    if top is not None:
        listed = listed[:max(0, int(top))]
    return {"totalLines": len(raws), "valueLines": value_lines, "values": n_values, "templates": len(per_sig),
            "fields": len(groups),
            "top": [values_row(sig, j, g["count"], g["sum"], g["min"], g["max"], g["maxLine"], g["first"],
                               g["firstValue"], g["last"], g["lastValue"], per_sig[sig], raws[g["first"]])
                    for (sig, j), g in listed]}


# ---------------------------------------------------------------------------------------------
# Variants report (an extra, as the gap report): the categorical sibling of the values report. Which
# values does a template's variable token take, how often, and which value is the odd one out --
# the one 503 among ten thousand 200s? The fields and their numbering are ``line_fields``', the
# group key is ``val_key``; a field counts whether or not it reads as a number, and its value is the
# token itself, compared through ``var_hash``. These functions are the specification of
# ``log_parser_amd/variants.py`` and of the kernels (csrc/kernels/var_core.h, var_table.h,
# variants.hip).
#
# Known limits: the limits of ``line_fields`` (the first ``SIG_MAX_BYTES`` bytes of a line, its
# first ``VAL_PER_LINE`` fields, only the stamps of ``line_timestamp`` are skipped); a token cut at
# byte ``SIG_MAX_BYTES`` is the value its first part spells; case is kept, so ``0xAB`` and ``0xab``
# are two values; two tokens may share a 64-bit hash, two (template, field) pairs a 64-bit key, and
# two (field, value) pairs that share the 64-bit ``var_cell_key`` are ONE value; a field with more
# than ``max_distinct`` values is only counted, never listed.

VARIANT_ORDERS = ("odd", "count", "distinct", "first")
VAR_MIN_DISTINCT, VAR_MAX_DISTINCT = 2, 4096


def var_hash(token: bytes) -> int:
    """FNV-1a-64 of the token's bytes as they are (case kept)."""
    h = _FNV_OFFSET
    for c in bytes(token):
        h = ((h ^ c) * _FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h


def var_cell_key(field: int, value: int) -> int:
    """The 64-bit table key of (``val_key`` of the field, ``var_hash`` of the token):
    ``trend_cell_key``'s mix."""
    return (field + value * _TREND_MIX) & _U64


def variants_check_args(max_distinct: int = 64, order: str = "odd", min_count: int = 5, min_fill: float = 0.9,
                        show: int = 5) -> None:
    if (isinstance(max_distinct, bool) or not isinstance(max_distinct, int)
            or not VAR_MIN_DISTINCT <= max_distinct <= VAR_MAX_DISTINCT):
        raise ValueError("max_distinct must be an integer in [%d, %d]" % (VAR_MIN_DISTINCT, VAR_MAX_DISTINCT))
    if order not in VARIANT_ORDERS:
        raise ValueError("order must be 'odd', 'count', 'distinct' or 'first'")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
        raise ValueError("min_count must be an integer >= 1")
    if isinstance(min_fill, bool) or not isinstance(min_fill, (int, float)) or not 0.0 <= min_fill <= 1.0:
        raise ValueError("min_fill must be in [0, 1]")
    if isinstance(show, bool) or not isinstance(show, int) or show < 1:
        raise ValueError("show must be an integer >= 1")


def variants_order_key(order: str, sig: int, j: int, count: int, odd: int, distinct: int, first: int):
    """The sort key of a group: exact arithmetic (ints and ``Fraction``), ``sig`` unsigned."""
    if order == "odd":
        return (Fraction(odd, count), -count, first, sig, j)
    if order == "count":
        return (-count, first, sig, j)
    if order == "distinct":
        return (-distinct, first, sig, j)
    return (first, j)


def variants_listed(values: list, show: int) -> list:
    """``values``: (count, first line, ...) tuples of a group. Sorted by (-count, first line); all
    of them when there are at most ``2 * show``, else the ``show`` most and the ``show`` least
    common."""
    values = sorted(values, key=lambda v: (-v[0], v[1]))
    return values if len(values) <= 2 * show else values[:show] + values[-show:]


def variants_value(sig: int, j: int, value: int, count: int, total: int, first: int, last: int, raw: bytes) -> dict:
    """One listed value from its numbers (lines 0-based) and its own first line: ValueError unless
    that line has the template ``sig`` and field ``j`` of it hashes to ``value``."""
    fields = line_fields(raw)
    if line_signature(raw) != sig or j >= len(fields) or var_hash(fields[j][2]) != value or not first <= last:
        raise ValueError("variants: line %d does not hold field %d of %016x with the value %016x"
                         % (first + 1, j, sig, value))
    return {"token": fields[j][2].decode("ascii"), "count": count, "share": count / total,
            "firstLine": first + 1, "lastLine": last + 1}


def variants_row(sig: int, j: int, lines: int, values: list, show: int) -> dict:
    """One row of the report. ``values``: (count, first line, last line, hash, raw first line) of
    every value of the group (lines 0-based)."""
    count = sum(v[0] for v in values)
    ordered = sorted(values, key=lambda v: (-v[0], v[1]))
    odd = count - ordered[0][0]
    first = min(values, key=lambda v: v[1])
    return {"signature": "%016x" % sig, "field": j, "count": count, "lines": lines, "fill": count / lines,
            "distinct": len(values), "odd": odd, "oddShare": odd / count, "firstLine": first[1] + 1,
            "template": line_template(first[4]).decode("utf-8", errors="replace"),
            "example": first[4].decode("utf-8", errors="replace"),
            "values": [variants_value(sig, j, h, c, count, f, l, raw)
                       for c, f, l, h, raw in variants_listed(values, show)]}


def variants_head(total: int, field_lines: int, tokens: int, templates: int, fields: int, unbounded: int,
                  max_distinct: int) -> dict:
    return {"totalLines": total, "fieldLines": field_lines, "tokens": tokens, "templates": templates,
            "fields": fields, "unboundedFields": unbounded, "maxDistinct": max_distinct, "top": []}


def variants(logs, max_distinct: int = 64, top: Optional[int] = 20, order: str = "odd", min_count: int = 5,
             min_fill: float = 0.9, varying: bool = True, show: int = 5) -> dict:
    """The variants report of ``logs`` (str or bytes; no pattern takes part). A *group* is
    (template signature of the line, field number j) of ``line_fields``; a *value* of it is a
    token, by ``var_hash``. Per value: its lines (``count``), the first and the last of them. A
    group with at most ``max_distinct`` distinct values over the whole log is *enumerable* and is
    reported; one with more (an id, a counter, a duration) is *unbounded* and only counted in
    ``unboundedFields``. Per group: ``count`` (the sum over its values), ``lines`` (all lines of
    the template), ``fill`` = count / lines, ``distinct``, ``odd`` = count minus the count of the
    most common value, ``oddShare`` = odd / count, ``firstLine`` (the smallest first line of its
    values) with its ``template`` and ``example``, and ``values``: sorted by (-count, first line),
    all of them when ``distinct <= 2 * show``, else the ``show`` most and the ``show`` least
    common; each with its ``token`` (from its own first line), ``count``, ``share`` = count /
    group count, ``firstLine``, ``lastLine``. Dropped are the groups with ``count < min_count``,
    those with ``count < min_fill * lines`` and, with ``varying``, those with one value.
    ``order="odd"``: by (odd / count, -count, first line, signature, field) -- the field with one
    deviant among ten thousand first; ``"count"``: (-count, first line, signature, field);
    ``"distinct"``: (-distinct, ...); ``"first"``: (first line, field). ``tokens`` counts all
    fields of all lines, ``fieldLines`` the lines with at least one, ``templates`` the templates
    of all lines, ``fields`` the groups (enumerable and unbounded) before the filters."""
    variants_check_args(max_distinct, order, min_count, min_fill, show)
    raws = [line.encode("utf-8", errors="surrogateescape") for line in split_lines(_as_text(logs))]
    per_sig: Dict[int, int] = {}
    groups: Dict[tuple, Dict[int, list]] = {}
    tokens = field_lines = 0
    for i, raw in enumerate(raws):
        sig = line_signature(raw)
        per_sig[sig] = per_sig.get(sig, 0) + 1
        fields = line_fields(raw)
        tokens += len(fields)
        field_lines += bool(fields)
        for j, _, tok in fields:
            h = var_hash(tok)
            v = groups.setdefault((sig, j), {}).setdefault(h, [0, i, i, h, raw])
            v[0] += 1
            v[2] = i
    out = variants_head(len(raws), field_lines, tokens, len(per_sig), len(groups),
                        sum(len(g) > max_distinct for g in groups.values()), max_distinct)
    listed = []
    for (sig, j), g in groups.items():
        if len(g) > max_distinct:
            continue
        count = sum(v[0] for v in g.values())
        if count < min_count or count < min_fill * per_sig[sig] or (varying and len(g) == 1):
            continue
        first = min(v[1] for v in g.values())
        listed.append((variants_order_key(order, sig, j, count, count - max(v[0] for v in g.values()), len(g), first),
                       sig, j, list(g.values())))
    listed.sort(key=lambda g: g[0])
    if top is not None:
        listed = listed[:max(0, int(top))]
    out["top"] = [variants_row(sig, j, per_sig[sig], [tuple(v) for v in vals], show) for _, sig, j, vals in listed]
    return out


# ---------------------------------------------------------------------------------------------
# Trends report (an extra, as the gap report): what changed over the time of this log? The log's
# own earlier part is the baseline: lines are counted per *cell* (template signature, time bucket),
# a *pivot* bucket splits the log's span, and a template started, stopped, surged, faded or stayed
# steady across it. No pattern and no baseline of healthy logs takes part. These functions are the
# specification of ``log_parser_amd/trends.py`` and of the cell table (csrc/kernels/trends.hip,
# cell_table.h).
#
# Known limits: only the stamps of ``line_timestamp`` count; an out-of-order stamp lands in whatever
# bucket it names; the pivot has bucket granularity; two cells may share a 64-bit cell key; a
# template is the first ``SIG_MAX_BYTES`` bytes of a line.

TREND_KINDS = ("started", "stopped", "surged", "faded", "steady")
TREND_UNDATED = -(1 << 63)      # the reserved bucket of a template's undated lines
_TREND_MIX = 0x9E3779B97F4A7C15
_U64 = 0xFFFFFFFFFFFFFFFF


def trend_cell_key(sig: int, bucket: int) -> int:
    """The 64-bit key of the cell (``sig``, ``bucket``): ``sig + bucket * _TREND_MIX`` mod 2^64. For
    a fixed bucket it is a bijection of the signatures (``trend_cell_sig`` inverts it)."""
    return (sig + bucket * _TREND_MIX) & _U64


def trend_cell_sig(key: int, bucket: int) -> int:
    """The signature whose cell in ``bucket`` has the key ``key``."""
    return (key - bucket * _TREND_MIX) & _U64


def trends_check_args(bucket_seconds=60, at=None, ratio: int = 4, min_count: int = 5, kind: Optional[str] = None,
                      order: str = "change", max_buckets: int = 65536):
    """(W in milliseconds, pivot source, pivot time in epoch ms or None), or ValueError. The pivot
    source is ``"middle"`` (``at=None``), ``"given"`` (an int, or a string that ``line_timestamp``
    parses from byte 0) or one of ``"first-event"`` / ``"first-error"`` (no time yet)."""
    if isinstance(bucket_seconds, bool) or not isinstance(bucket_seconds, int) or bucket_seconds < 1:
        raise ValueError("trends: bucket_seconds must be an integer >= 1")
    if isinstance(max_buckets, bool) or not isinstance(max_buckets, int) or max_buckets < 1:
        raise ValueError("trends: max_buckets must be an integer >= 1")
    if isinstance(ratio, bool) or not isinstance(ratio, int) or ratio < 2:
        raise ValueError("trends: ratio must be an integer >= 2")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
        raise ValueError("trends: min_count must be an integer >= 1")
    if kind is not None and kind != "all" and kind not in TREND_KINDS:
        raise ValueError("trends: kind must be None, 'all' or one of %s" % ", ".join(TREND_KINDS))
    if order not in ("change", "count", "first"):
        raise ValueError("trends: order must be 'change', 'count' or 'first'")
    W = 1000 * bucket_seconds
    if at is None:
        return W, "middle", None
    if isinstance(at, bool):
        raise ValueError("trends: at must be None, epoch milliseconds, a timestamp, 'first-event' or 'first-error'")
    if isinstance(at, int):
        return W, "given", at
    if isinstance(at, (bytes, str)):
        raw = at.encode("utf-8", errors="surrogateescape") if isinstance(at, str) else bytes(at)
        if raw in (b"first-event", b"first-error"):
            return W, raw.decode(), None
        m = _STAMP.match(raw)
        t = line_timestamp(raw) if m else None
        if t is None:
            raise ValueError("trends: at=%r is no timestamp" % (at,))
        return W, "given", t
    raise ValueError("trends: at must be None, epoch milliseconds, a timestamp, 'first-event' or 'first-error'")


def trends_named_pivot(source: str, timeline_report: dict) -> int:
    """Epoch milliseconds of the pivot ``"first-event"`` / ``"first-error"`` from the timeline
    report of the same log and bucket width, or ValueError when the timeline has none."""
    ref = timeline_report["firstEvent" if source == "first-event" else "firstErrorLine"]
    if ref is None:
        raise ValueError("trends: the log has no %s to take the pivot from"
                         % ("dated event" if source == "first-event" else "dated error line"))
    return line_timestamp(ref["timestamp"].encode("ascii"))


def trends_pivot(source: str, at: Optional[int], b0: int, b1: int, W: int) -> Optional[int]:
    """The pivot bucket p with ``b0 < p <= b1``: the middle ``b0 + nb // 2`` (None with fewer than
    two buckets), or ``floor(at / W)`` -- ValueError when that lies outside ``(b0, b1]``."""
    nb = b1 - b0 + 1
    if source == "middle":
        return b0 + nb // 2 if nb >= 2 else None
    p = at // W
    if not b0 < p <= b1:
        raise ValueError("trends: the pivot %s (%s) is not behind the first bucket and within the span %s .. %s of the log"
                         % (iso_ms(p * W), source, iso_ms(b0 * W), iso_ms(b1 * W)))
    return p


def trends_kind(before: int, after: int, nb_before: int, nb_after: int, ratio: int) -> str:
    x, y = after * nb_before, before * nb_after
    if before == 0:
        return "started"
    if after == 0:
        return "stopped"
    if x >= ratio * y:
        return "surged"
    if y >= ratio * x:
        return "faded"
    return "steady"


def trends_listed(kind: Optional[str], k: str) -> bool:
    """A template of the kind ``k`` is listed under the filter ``kind`` (None: all but steady)."""
    return k != "steady" if kind is None else kind in ("all", k)


def trends_lift(before: int, after: int, nb_before: int, nb_after: int) -> Fraction:
    return Fraction((after + 1) * nb_before, (before + 1) * nb_after)


def trends_order_key(order: str, lift: Fraction, dated: int, first: int):
    """The sort key of a template: exact arithmetic (ints and ``Fraction``)."""
    if order == "change":
        return (-max(lift, 1 / lift), -dated, first)
    if order == "count":
        return (-dated, first)
    return (first,)


def trends_row(sig: int, lines: int, dated: int, before: int, after: int, first_bucket: int, last_bucket: int,
               active: int, peak_bucket: int, peak_count: int, first: int, raw: bytes, W: int, kind: str,
               lift: Fraction) -> dict:
    """One row of the report from its numbers (``first``: the template's first line, 0-based) and
    that line: ValueError unless the line has the template ``sig``."""
    if line_signature(raw) != sig:
        raise ValueError("trends: line %d does not have the template %016x" % (first + 1, sig))
    return {"signature": "%016x" % sig, "kind": kind, "lift": float(lift), "lines": lines, "datedLines": dated,
            "before": before, "after": after, "firstSeen": iso_ms(first_bucket * W), "lastSeen": iso_ms(last_bucket * W),
            "activeBuckets": active, "peakBucket": iso_ms(peak_bucket * W), "peakCount": peak_count,
            "firstLine": first + 1, "template": line_template(raw).decode("utf-8", errors="replace"),
            "example": raw.decode("utf-8", errors="replace")}


def trends_head(total: int, dated: int, templates: int, cells: int, bucket_seconds: int) -> dict:
    """The report of a log before its span is known: the counts, no pivot, nothing listed."""
    return {"totalLines": total, "datedLines": dated, "undatedLines": total - dated, "templates": templates,
            "cells": cells, "bucketSeconds": bucket_seconds, "firstBucket": None, "lastBucket": None, "buckets": 0,
            "pivot": None, "pivotSource": None, "bucketsBefore": 0, "bucketsAfter": 0,
            "kinds": {k: 0 for k in TREND_KINDS}, "top": []}


def trends(logs, pattern_sets: Optional[List[PatternSet]] = None, params: Optional[ScoringParams] = None,
           bucket_seconds: int = 60, at=None, ratio: int = 4, min_count: int = 5, kind: Optional[str] = None,
           order: str = "change", top: Optional[int] = 20, max_buckets: int = 65536) -> dict:
    """The trends report of ``logs`` (str or bytes). A line's effective time is its own stamp, else
    the stamp of the nearest earlier stamped line (``timeline``'s fill); its bucket is
    ``floor(eff / W)`` with ``W = 1000 * bucket_seconds``. The span ``b0 .. b1`` covers the buckets
    of all dated lines (ValueError beyond ``max_buckets``); the pivot p (``trends_pivot``; the
    named pivots come from ``timeline`` with ``pattern_sets`` / ``params``) splits it into
    ``p - b0`` buckets before and ``b1 - p + 1`` from p on. Per template: ``lines``,
    ``datedLines``, ``before`` / ``after`` (dated lines in buckets ``< p`` / ``>= p``),
    ``firstSeen`` / ``lastSeen`` (start of its first / last dated bucket), ``activeBuckets``,
    ``peakBucket`` / ``peakCount`` (its largest dated cell, the earliest on a tie), ``kind``
    (``trends_kind``), ``lift`` (``trends_lift``), its first line and that line as the example.
    Listed are the templates with ``datedLines >= min_count`` of the kind ``kind`` (None: all but
    steady), in ``order`` (``trends_order_key``). ``cells`` counts the (template, bucket) pairs,
    the undated lines of a template as one more; ``kinds`` the templates with ``datedLines >=
    min_count`` per kind."""
    W, source, at_ms = trends_check_args(bucket_seconds, at, ratio, min_count, kind, order, max_buckets)
    raws = [line.encode("utf-8", errors="surrogateescape") for line in split_lines(_as_text(logs))]
    cells: Dict[tuple, int] = {}
    first: Dict[int, int] = {}
    cur = None
    n_dated = 0
    for i, raw in enumerate(raws):
        t = line_timestamp(raw)
        cur = cur if t is None else t
        sig = line_signature(raw)
        first.setdefault(sig, i)
        b = TREND_UNDATED if cur is None else cur // W
        n_dated += cur is not None
        cells[(sig, b)] = cells.get((sig, b), 0) + 1
    out = trends_head(len(raws), n_dated, len(first), len(cells), bucket_seconds)
    dated = [b for _, b in cells if b != TREND_UNDATED]
    if not dated:
        return out
    b0, b1 = min(dated), max(dated)
    if b1 - b0 + 1 > max_buckets:
        raise timeline_span_error(b0 * W, b1 * W, W, max_buckets)
    out.update({"firstBucket": iso_ms(b0 * W), "lastBucket": iso_ms(b1 * W), "buckets": b1 - b0 + 1})
    if source in ("first-event", "first-error"):
        at_ms = trends_named_pivot(source, timeline(logs, pattern_sets or [], params or ScoringParams(),
                                                    bucket_seconds, max_buckets))
    p = trends_pivot(source, at_ms, b0, b1, W)
    if p is None:
        return out
    nb_before, nb_after = p - b0, b1 - p + 1
    out.update({"pivot": iso_ms(p * W), "pivotSource": source, "bucketsBefore": nb_before, "bucketsAfter": nb_after})
    per: Dict[int, Dict[int, int]] = {}
    for (sig, b), c in cells.items():
        per.setdefault(sig, {})[b] = c
    listed = []
    for sig, row in per.items():
        lines = sum(row.values())
        row = {b: c for b, c in row.items() if b != TREND_UNDATED}
        n = sum(row.values())
        if n < min_count:
            continue
        before = sum(c for b, c in row.items() if b < p)
        k = trends_kind(before, n - before, nb_before, nb_after, ratio)
        out["kinds"][k] += 1
        if not trends_listed(kind, k):
            continue
        lift = trends_lift(before, n - before, nb_before, nb_after)
        peak = max(row.values())
        listed.append((trends_order_key(order, lift, n, first[sig]),
                       (sig, lines, n, before, n - before, min(row), max(row), len(row),
                        min(b for b, c in row.items() if c == peak), peak, first[sig], raws[first[sig]], W, k, lift)))
    listed.sort(key=lambda kv: kv[0])
    if top is not None:
        listed = listed[:max(0, int(top))]
    out["top"] = [trends_row(*row) for _, row in listed]
    return out


# ---------------------------------------------------------------------------------------------
# Pauses report (an extra, as the gap report): where did the log stop talking, and what was the
# program doing when it stopped? A deadlock, a long GC pause, a blocked pool and a retry back-off all
# look the same: seconds or minutes between two stamped lines, usually after the same one or two
# templates. These functions are the specification of ``log_parser_amd/pauses.py`` and of the pause
# scan (csrc/kernels/pauses.hip).
#
# Known limits: only the stamps of ``line_timestamp`` count; a log that interleaves sources with
# skewed clocks shows steps that are no pauses of any one of them; stamps lie within +-2^61 ms, so
# no step overflows 64 bits; a template is the first ``SIG_MAX_BYTES`` bytes of a line.

PAUSE_ORDERS = ("total", "max", "count", "share", "first")
PAUSE_BUCKETS = 64


def pauses_check_args(min_ms=1000, by: str = "before", order: str = "total", min_count: int = 1) -> None:
    if isinstance(min_ms, bool) or not isinstance(min_ms, int) or min_ms < 1:
        raise ValueError("pauses: min_ms must be an integer >= 1")
    if by not in ("before", "after"):
        raise ValueError("pauses: by must be 'before' or 'after'")
    if order not in PAUSE_ORDERS:
        raise ValueError("pauses: order must be %s or '%s'" % (", ".join("'%s'" % o for o in PAUSE_ORDERS[:-1]),
                                                              PAUSE_ORDERS[-1]))
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
        raise ValueError("pauses: min_count must be an integer >= 1")


def pause_bucket(step: int) -> int:
    """The interval bucket of a step >= 0: 0 holds step 0, b holds ``[2^(b-1), 2^b)``."""
    return step.bit_length()


def pauses_head(total: int, stamped: int, backward: int, min_ms: int, pauses_n: int, paused_ms: int,
                first: Optional[int], last: Optional[int], hist: Sequence[int]) -> dict:
    """Head and ``intervals`` of the report from the counts (``first`` / ``last``: smallest and
    largest stamp, None without one; ``hist[b]``: the steps >= 0 in bucket b); the lists empty."""
    span = None if first is None else last - first
    return {"totalLines": total, "stampedLines": stamped, "steps": max(0, stamped - 1), "backwardSteps": backward,
            "minPauseMs": min_ms, "pauses": pauses_n, "pausedMs": paused_ms, "spanMs": span,
            "pausedShare": paused_ms / span if span else None,
            "firstTimestamp": None if first is None else iso_ms(first),
            "lastTimestamp": None if last is None else iso_ms(last),
            "intervals": [{"fromMs": (1 << b) >> 1, "toMs": 1 << b, "count": c} for b, c in enumerate(hist) if c],
            "longest": [], "templates": []}


def pauses_longest_row(ms: int, from_line: int, to_line: int, from_ts: int, before: bytes, after: bytes,
                       by: str) -> dict:
    """One row of ``longest`` (lines 0-based) from the pause and its two lines."""
    return {"ms": ms, "fromLine": from_line + 1, "toLine": to_line + 1, "from": iso_ms(from_ts),
            "to": iso_ms(from_ts + ms), "linesBetween": to_line - from_line - 1,
            "before": before.decode("utf-8", errors="replace"), "after": after.decode("utf-8", errors="replace"),
            "signature": "%016x" % line_signature(before if by == "before" else after)}


def pauses_order_key(order: str, count: int, lines: int, total_ms: int, max_ms: int, first_line: int):
    """The sort key of a template: exact arithmetic (ints and ``Fraction``); ties by ``firstLine``."""
    if order == "total":
        return (-total_ms, first_line)
    if order == "max":
        return (-max_ms, first_line)
    if order == "count":
        return (-count, first_line)
    if order == "share":
        return (-Fraction(count, lines), first_line)
    return (first_line,)


def pauses_template_row(sig: int, count: int, lines: int, total_ms: int, max_ms: int, max_line: int,
                        first_line: int, raw: bytes) -> dict:
    """One row of ``templates`` from its numbers (lines 0-based) and the key line of its first
    pause: ValueError unless that line has the template ``sig``."""
    if line_signature(raw) != sig:
        raise ValueError("pauses: the example of %016x does not have that template" % sig)
    return {"signature": "%016x" % sig, "pauses": count, "lines": lines, "share": count / lines, "totalMs": total_ms,
            "maxMs": max_ms, "maxLine": max_line + 1, "firstLine": first_line + 1,
            "template": line_template(raw).decode("utf-8", errors="replace"),
            "example": raw.decode("utf-8", errors="replace")}


def pauses(logs, min_ms: int = 1000, by: str = "before", order: str = "total", min_count: int = 1,
           top: Optional[int] = 20) -> dict:
    """The pauses report of ``logs`` (str or bytes). The stamped lines in line order are ``i_0 <
    i_1 < ...``; step k is ``own[i_k] - own[i_{k-1}]`` with the from-line ``i_{k-1}`` and the
    to-line ``i_k``. A step below 0 is a backward step: counted, never a pause; a step ``>=
    min_ms`` is a pause. ``intervals`` counts the steps >= 0 by ``pause_bucket``; ``longest`` holds
    the ``top`` pauses by (-ms, toLine); ``templates`` groups the pauses by the signature of their
    key line -- the from-line for ``by="before"``, the to-line for ``by="after"`` -- with
    ``lines`` (all lines of that template), ``share`` (pauses / lines), ``totalMs``, ``maxMs``,
    ``maxLine`` (to-line of the largest pause, the first on a tie), ``firstLine`` (to-line of the
    first pause) and the key line of the first pause as the example; groups below ``min_count``
    pauses are dropped, the rest listed in ``order`` (``pauses_order_key``), ``top`` of them."""
    pauses_check_args(min_ms, by, order, min_count)
    raws = [line.encode("utf-8", errors="surrogateescape") for line in split_lines(_as_text(logs))]
    sigs = [line_signature(raw) for raw in raws]
    own = [line_timestamp(raw) for raw in raws]
    stamped = [i for i, t in enumerate(own) if t is not None]
    hist = [0] * PAUSE_BUCKETS
    backward = 0
    found = []                                  # (ms, from-line, to-line)
    for a, b in zip(stamped, stamped[1:]):
        step = own[b] - own[a]
        if step < 0:
            backward += 1
            continue
        hist[pause_bucket(step)] += 1
        if step >= min_ms:
            found.append((step, a, b))
    stamps = [own[i] for i in stamped]
    out = pauses_head(len(raws), len(stamped), backward, min_ms, len(found), sum(p[0] for p in found),
                      min(stamps) if stamps else None, max(stamps) if stamps else None, hist)
    cut = (lambda rows: rows) if top is None else (lambda rows: rows[:max(0, int(top))])
    out["longest"] = [pauses_longest_row(ms, a, b, own[a], raws[a], raws[b], by)
                      for ms, a, b in cut(sorted(found, key=lambda p: (-p[0], p[2])))]
    lines: Dict[int, int] = {}
    for s in sigs:
        lines[s] = lines.get(s, 0) + 1
    groups: Dict[int, list] = {}                # signature -> [count, total, max, maxLine, firstLine, key line]
    for ms, a, b in found:
        key = a if by == "before" else b
        g = groups.setdefault(sigs[key], [0, 0, -1, b, b, key])
        g[0] += 1
        g[1] += ms
        if ms > g[2]:
            g[2], g[3] = ms, b
    listed = [(pauses_order_key(order, g[0], lines[s], g[1], g[2], g[4]), s, g) for s, g in groups.items()
              if g[0] >= min_count]
    listed.sort(key=lambda kv: kv[0])
    out["templates"] = [pauses_template_row(s, g[0], lines[s], g[1], g[2], g[3], g[4], raws[g[5]])
                        for _, s, g in cut(listed)]
    return out


# ---------------------------------------------------------------------------------------------
# Cadence report (an extra, as the gap report): which line templates come at a steady beat -- a
# heartbeat, a health check, a lease renewal, a poller -- where did one of them miss beats while the
# rest of the log went on, and which never came back before the log ended? ``pauses`` sees only the
# steps of the whole log, ``trends`` only one pivot; here every template has a clock of its own.
# These functions are the specification of ``log_parser_amd/cadence.py`` and of the beat scan
# (csrc/kernels/cadence.hip).
#
# Known limits: only the stamps of ``line_timestamp`` count; stamps lie within +-2^61 ms, so no beat
# overflows 64 bits; a template is the first ``SIG_MAX_BYTES`` bytes of a line; a line that comes in
# bursts of a steady size looks periodic to ``regularity``, which sees a histogram and no order.

CADENCE_ORDERS = ("gap", "overdue", "count", "first")
CADENCE_KINDS = ("missed", "stopped")


def cadence_check_args(min_ms=1000, ratio=4, min_count=5, min_regularity=0.8, kind: Optional[str] = None,
                       order: str = "gap") -> Fraction:
    """``min_regularity`` as an exact fraction, or ValueError."""
    if isinstance(min_ms, bool) or not isinstance(min_ms, int) or min_ms < 1:
        raise ValueError("cadence: min_ms must be an integer >= 1")
    if isinstance(ratio, bool) or not isinstance(ratio, int) or ratio < 1:
        raise ValueError("cadence: ratio must be an integer >= 1")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
        raise ValueError("cadence: min_count must be an integer >= 1")
    if isinstance(min_regularity, bool) or not isinstance(min_regularity, (int, float, Fraction)) \
            or min_regularity != min_regularity or not 0 <= min_regularity <= 1:
        raise ValueError("cadence: min_regularity must be a number in [0, 1]")
    if kind is not None and kind != "all" and kind not in CADENCE_KINDS:
        raise ValueError("cadence: kind must be None, 'all', 'missed' or 'stopped'")
    if order not in CADENCE_ORDERS:
        raise ValueError("cadence: order must be 'gap', 'overdue', 'count' or 'first'")
    return Fraction(min_regularity)


def cadence_regularity(hist: Sequence[int], beats: int) -> Fraction:
    """The share of the forward beats in the best pair of adjacent buckets of ``hist`` (64 counts
    by ``pause_bucket``): a band a factor 4 wide."""
    h = list(hist) + [0]
    return Fraction(max(h[b] + h[b + 1] for b in range(len(h) - 1)), beats)


def cadence_judge(beats: int, sum_ms: int, max_ms: int, last_ts: int, end: int, hist: Sequence[int], min_ms: int,
                  ratio: int, min_count: int, min_regularity: Fraction) -> Optional[dict]:
    """What the numbers of one template say, or None when it is not periodic: ``typicalMs`` (the
    mean of the beats but the largest), ``regularity``, ``overdueMs``, ``missed`` / ``missedBeats``
    and ``stopped``. Exact arithmetic."""
    if beats < min_count or beats < 2:
        return None
    typical = (sum_ms - max_ms) // (beats - 1)
    if typical < 1:
        return None
    reg = cadence_regularity(hist, beats)
    if reg < min_regularity:
        return None
    overdue = max(0, end - last_ts)
    threshold = max(min_ms, ratio * typical)
    missed = max_ms >= threshold
    return {"typicalMs": typical, "regularity": reg, "overdueMs": overdue, "missed": missed,
            "missedBeats": max_ms // typical - 1 if missed else 0, "stopped": overdue >= threshold}


def cadence_listed(kind: Optional[str], missed: bool, stopped: bool) -> bool:
    """A periodic template is listed under the filter ``kind`` (None: it missed beats or stopped)."""
    if kind == "all":
        return True
    if kind is None:
        return missed or stopped
    return missed if kind == "missed" else stopped


def cadence_order_key(order: str, typical: int, max_ms: int, overdue: int, beats: int, first_line: int):
    """The sort key of a template: exact arithmetic (ints and ``Fraction``); ties by ``firstLine``."""
    if order == "gap":
        return (-Fraction(max(max_ms, overdue), typical), first_line)
    if order == "overdue":
        return (-overdue, first_line)
    if order == "count":
        return (-beats, first_line)
    return (first_line,)


def cadence_head(total: int, stamped: int, templates: int, first: Optional[int], last: Optional[int]) -> dict:
    """The head of the report (``first`` / ``last``: the stamps of the first and the last stamped
    line in line order, None without one); nothing judged or listed yet."""
    return {"totalLines": total, "stampedLines": stamped, "templates": templates, "periodic": 0, "missed": 0,
            "stopped": 0, "firstTimestamp": None if first is None else iso_ms(first),
            "lastTimestamp": None if last is None else iso_ms(last), "top": []}


def cadence_row(sig: int, lines: int, beats: int, backward: int, sum_ms: int, min_ms: int, max_ms: int, from_line: int,
                to_line: int, to_ts: int, first_line: int, last_line: int, last_ts: int, hist: Sequence[int],
                judged: dict, raw: bytes) -> dict:
    """One row of the report from its numbers (lines 0-based), what ``cadence_judge`` said of them
    and the template's first stamped line: ValueError unless that line has the template ``sig``."""
    if line_signature(raw) != sig:
        raise ValueError("cadence: line %d does not have the template %016x" % (first_line + 1, sig))
    return {"signature": "%016x" % sig, "missed": judged["missed"], "stopped": judged["stopped"], "lines": lines,
            "beats": beats, "backwardBeats": backward, "typicalMs": judged["typicalMs"],
            "regularity": float(judged["regularity"]), "sumMs": sum_ms, "minMs": min_ms, "maxMs": max_ms,
            "fromLine": from_line + 1, "toLine": to_line + 1, "from": iso_ms(to_ts - max_ms), "to": iso_ms(to_ts),
            "missedBeats": judged["missedBeats"], "overdueMs": judged["overdueMs"], "firstLine": first_line + 1,
            "lastLine": last_line + 1, "lastTimestamp": iso_ms(last_ts),
            "intervals": [{"fromMs": (1 << b) >> 1, "toMs": 1 << b, "count": c} for b, c in enumerate(hist) if c],
            "template": line_template(raw).decode("utf-8", errors="replace"),
            "example": raw.decode("utf-8", errors="replace")}


def cadence(logs, min_ms: int = 1000, ratio: int = 4, min_count: int = 5, min_regularity=0.8,
            kind: Optional[str] = None, order: str = "gap", top: Optional[int] = 20) -> dict:
    """The cadence report of ``logs`` (str or bytes). The stamped lines of ONE template signature
    in line order are ``j_0 < j_1 < ...``; the beat k is ``own[j_k] - own[j_{k-1}]`` with the
    from-line ``j_{k-1}`` and the to-line ``j_k``. A beat below 0 is a backward beat: counted,
    nothing else. Per template: ``lines`` (stamped), ``beats`` (forward), ``backwardBeats``,
    ``sumMs``, ``minMs``, ``maxMs`` with its lines and their stamps (the smallest to-line on a
    tie), ``firstLine`` / ``lastLine`` / ``lastTimestamp`` and ``intervals``, the forward beats by
    ``pause_bucket``. ``cadence_judge`` derives ``typicalMs``, ``regularity`` and ``overdueMs``
    (against the stamp of the log's last stamped line) and says whether the template is periodic,
    missed beats (``maxMs >= max(min_ms, ratio * typicalMs)``) or stopped (``overdueMs`` at least
    that). Listed are the periodic templates of the kind ``kind`` (``cadence_listed``) in
    ``order`` (``cadence_order_key``), ``top`` of them, each with its first stamped line as the
    example. The head counts the periodic templates and those that missed / stopped, listed or not."""
    min_reg = cadence_check_args(min_ms, ratio, min_count, min_regularity, kind, order)
    raws = [line.encode("utf-8", errors="surrogateescape") for line in split_lines(_as_text(logs))]
    per: Dict[int, dict] = {}
    seen = set()
    first_ts = end = None
    stamped = 0
    for i, raw in enumerate(raws):
        sig = line_signature(raw)
        seen.add(sig)
        t = line_timestamp(raw)
        if t is None:
            continue
        stamped += 1
        first_ts = t if first_ts is None else first_ts
        end = t
        g = per.get(sig)
        if g is None:
            per[sig] = {"lines": 1, "beats": 0, "back": 0, "sum": 0, "min": None, "max": -1, "from": -1, "to": -1,
                        "to_ts": 0, "first": i, "last": i, "last_ts": t, "hist": [0] * PAUSE_BUCKETS}
            continue
        beat = t - g["last_ts"]
        g["lines"] += 1
        if beat < 0:
            g["back"] += 1
        else:
            g["beats"] += 1
            g["sum"] += beat
            g["min"] = beat if g["min"] is None else min(g["min"], beat)
            g["hist"][pause_bucket(beat)] += 1
            if beat > g["max"]:
                g["max"], g["from"], g["to"], g["to_ts"] = beat, g["last"], i, t
        g["last"], g["last_ts"] = i, t
    out = cadence_head(len(raws), stamped, len(seen), first_ts, end)
    listed = []
    for sig, g in per.items():
        j = cadence_judge(g["beats"], g["sum"], g["max"], g["last_ts"], end, g["hist"], min_ms, ratio, min_count, min_reg)
        if j is None:
            continue
        out["periodic"] += 1
        out["missed"] += j["missed"]
        out["stopped"] += j["stopped"]
        if cadence_listed(kind, j["missed"], j["stopped"]):
            listed.append((cadence_order_key(order, j["typicalMs"], g["max"], j["overdueMs"], g["beats"], g["first"]),
                           (sig, g["lines"], g["beats"], g["back"], g["sum"], g["min"], g["max"], g["from"], g["to"],
                            g["to_ts"], g["first"], g["last"], g["last_ts"], g["hist"], j, raws[g["first"]])))
    listed.sort(key=lambda kv: kv[0])
    if top is not None:
        listed = listed[:max(0, int(top))]
    out["top"] = [cadence_row(*row) for _, row in listed]
    return out


# ---------------------------------------------------------------------------------------------
# Spans report (an extra, as the gap report): which request, job, trace or connection took longest,
# and which started like all the others and never logged the line the others end on? The *span* of
# an id is the set of lines that hold it; a hung request is invisible to ``pauses`` and ``cadence``
# -- the other requests keep the log and the templates busy -- and to ``correlate`` when no pattern
# matches. No pattern takes part here. These functions are the specification of
# ``log_parser_amd/spans.py`` and of the span kernels (csrc/kernels/spans.hip, span_table.h).
#
# Known limits: those of ``line_keys`` (two tokens may share a 64-bit key; a UUID is two tokens;
# the first ``KEY_PER_LINE`` distinct keys of a line's first ``SIG_MAX_BYTES`` bytes); stamps lie
# within +-2^61 ms, as for ``pauses``, so no duration overflows 64 bits; under sampling
# (``sampleShift > 0``) every count is a count of the sample.

SPAN_ORDERS = ("duration", "lines", "first")
SPAN_MAX_IDS_LO, SPAN_MAX_IDS_HI, SPAN_MAX_IDS = 16, 1 << 26, 1 << 22
SPAN_BUCKETS = 64


def _span_int(name: str, v, lo: int, hi: Optional[int] = None) -> None:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError("spans: %s must be an integer %s" % (name, (">= %d" % lo) if hi is None else "in %d..%d" % (lo, hi)))


def spans_check_args(min_len: int = 8, max_ids: int = SPAN_MAX_IDS, order: str = "duration", min_lines: int = 2,
                     max_share: float = 0.25, min_ms: int = 0, kind_min_spans: int = 5, close_share=0.8,
                     top: Optional[int] = 20, kinds: Optional[int] = 10) -> Fraction:
    """``close_share`` as an exact fraction, or ValueError. A float stands for the decimal it prints
    as -- 0.8 is 4/5, not the binary fraction next to it -- so a share of exactly ``close_share``
    passes."""
    _span_int("min_len", min_len, KEY_MIN_LEN, KEY_MAX_LEN)
    _span_int("max_ids", max_ids, SPAN_MAX_IDS_LO, SPAN_MAX_IDS_HI)
    if order not in SPAN_ORDERS:
        raise ValueError("spans: order must be 'duration', 'lines' or 'first'")
    _span_int("min_lines", min_lines, 1)
    if isinstance(max_share, bool) or not isinstance(max_share, (int, float)) or not 0.0 < max_share <= 1.0:
        raise ValueError("spans: max_share must be in (0, 1]")
    _span_int("min_ms", min_ms, 0)
    _span_int("kind_min_spans", kind_min_spans, 1)
    if isinstance(close_share, bool) or not isinstance(close_share, (int, float, Fraction)) \
            or close_share != close_share or not 0 < close_share <= 1:
        raise ValueError("spans: close_share must be a number in (0, 1]")
    for name, v in (("top", top), ("kinds", kinds)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
            raise ValueError("spans: %s must be None or an integer" % name)
    return Fraction(repr(close_share)) if isinstance(close_share, float) else Fraction(close_share)


def span_level(key: int) -> int:
    """The deepest sample that holds ``key``: the leading zero bits of ``fmix64(key)`` (0..64). A key
    is in sample s -- the top s bits of the hash are zero -- exactly when ``span_level(key) >= s``:
    the samples are nested."""
    return 64 - fmix64(key).bit_length()


def spans_shift(levels: Sequence[int], max_ids: int) -> int:
    """The smallest s whose sample holds at most ``max_ids`` of the ids with these levels."""
    s = 0
    while sum(1 for v in levels if v >= s) > max_ids:
        s += 1
    return s


def spans_head(total: int, timed: int, id_lines: int, pairs: int, ids: int, min_len: int, max_ids: int,
               shift: int) -> dict:
    """The head of the report; nothing listed yet."""
    return {"totalLines": total, "timedLines": timed, "idLines": id_lines, "pairs": pairs, "ids": ids, "listed": 0,
            "minLength": min_len, "maxIds": max_ids, "sampleShift": shift, "durations": [], "kinds": [], "top": []}


def spans_durations(hist: Sequence[int]) -> list:
    """The duration histogram (``hist[b]``: listed timed spans whose duration has bit length b)."""
    return [{"fromMs": (1 << b) >> 1, "toMs": 1 << b, "count": c} for b, c in enumerate(hist) if c]


def spans_usual_end(closes: Dict[int, int], spans_n: int, kind_min_spans: int, close_share: Fraction) -> Optional[int]:
    """The usual end of a kind with ``spans_n`` spans whose closing templates (unsigned signature
    -> spans) are ``closes``: the one with the most spans, the smaller signature on a tie -- if
    the kind has at least ``kind_min_spans`` spans and that one's share reaches ``close_share``."""
    if spans_n < kind_min_spans:
        return None
    sig, c = min(closes.items(), key=lambda kv: (-kv[1], kv[0]))
    return sig if Fraction(c, spans_n) >= close_share else None


def spans_order_key(order: str, duration: Optional[int], lines: int, first: int, key: int):
    if order == "duration":
        return (duration is None, -(duration or 0), first, key)
    if order == "lines":
        return (-lines, first, key)
    return (first, key)


def _span_text(raw: bytes) -> str:
    return raw.decode("utf-8", errors="replace")


def spans_kind_row(opens: int, spans_n: int, timed: int, sum_ms: int, max_ms: Optional[int], max_key: Optional[str],
                   max_line: Optional[int], first_line: int, closes: Dict[int, int], usual: Optional[int],
                   unfinished: int, raws: Dict[int, bytes]) -> dict:
    """One row of ``kinds`` (lines 0-based; ``raws``: unsigned signature -> the first line of the
    log with that template, for ``opens`` and every closing template): ValueError unless every such
    line has its template."""
    for s in [opens] + list(closes):
        if line_signature(raws[s]) != s:
            raise ValueError("spans: the example of %016x does not have that template" % s)
    return {"opens": "%016x" % opens, "template": _span_text(line_template(raws[opens])),
            "example": _span_text(raws[opens]), "firstLine": first_line + 1, "spans": spans_n, "timedSpans": timed,
            "sumMs": sum_ms, "maxMs": max_ms, "maxKey": max_key, "maxLine": None if max_line is None else max_line + 1,
            "closes": [{"signature": "%016x" % s, "spans": c, "template": _span_text(line_template(raws[s]))}
                       for s, c in sorted(closes.items(), key=lambda kv: (-kv[1], kv[0]))],
            "usualEnd": None if usual is None else "%016x" % usual, "unfinished": unfinished}


def spans_row(key: int, token: bytes, lines: int, first: int, last: int, tmin: Optional[int], tmax: Optional[int],
              opens: int, closes: int, unfinished: bool, usual: Optional[int], raw_open: bytes, raw_close: bytes) -> dict:
    """One row of ``top`` from its numbers (lines 0-based; ``tmin`` None: no line of the span has a
    time) and the example lines of its two templates: ValueError unless the token hashes to the
    key, the numbers are those of a span and the examples have their templates."""
    if fnv1a64(token) != key or token != token.lower():
        raise ValueError("spans: the token %r does not hash to the key %016x" % (token, key))
    if not (0 <= first <= last and 0 < lines <= last - first + 1) or (tmin is not None and tmin > tmax):
        raise ValueError("spans: %016x has %d lines in %d..%d, or ends before it starts" % (key, lines, first + 1, last + 1))
    if line_signature(raw_open) != opens or line_signature(raw_close) != closes:
        raise ValueError("spans: an example of %016x does not have its template" % key)
    row = {"key": token.decode("ascii"), "signature": "%016x" % key, "lines": lines, "firstLine": first + 1,
           "lastLine": last + 1, "start": None if tmin is None else iso_ms(tmin),
           "end": None if tmin is None else iso_ms(tmax), "durationMs": None if tmin is None else tmax - tmin,
           "opens": "%016x" % opens, "closes": "%016x" % closes, "opensExample": _span_text(raw_open),
           "closesExample": _span_text(raw_close), "unfinished": unfinished}
    if usual is not None:
        row["usualEnd"] = "%016x" % usual
    return row


def spans(logs, min_len: int = 8, max_ids: int = SPAN_MAX_IDS, top: Optional[int] = 20, order: str = "duration",
          unfinished_only: bool = False, min_lines: int = 2, max_share: float = 0.25, min_ms: int = 0,
          kind_min_spans: int = 5, close_share=0.8, kinds: Optional[int] = 10) -> dict:
    """The spans report of ``logs`` (str or bytes). The keys of a line are ``line_keys(line,
    min_len)``; its *time* is the stamp (``line_timestamp``) of the nearest stamped line at or
    before it, none in front of the first stamp. The *span* of a key is every line that holds it:
    ``lines``, ``firstLine`` / ``lastLine``, ``start`` / ``end`` (the smallest and the largest time
    of its timed lines -- min and max, not the times of its first and last line),
    ``durationMs = end - start`` (None when no line of it has a time), ``opens`` / ``closes`` (the
    template signatures of its first and last line) and ``key``, the lowered token of its first line.

    Sampling bounds the ids: with ``s = sampleShift`` the smallest number for which at most
    ``max_ids`` ids have ``span_level(key) >= s``, only those ids exist for the report -- ``ids``,
    ``pairs`` (their lines, summed) and ``idLines`` (the lines that hold at least one) count them.

    Filters, in this order: ``lines >= min_lines``; ``lines <= max_share * totalLines``;
    ``durationMs >= min_ms`` (None passes only for ``min_ms == 0``). ``listed`` counts the
    survivors, ``durations`` their durations by ``pause_bucket``. They are grouped into *kinds* by
    ``opens``: ``spans``, ``timedSpans``, ``sumMs``, ``maxMs`` with ``maxKey`` / ``maxLine`` (the
    span's first line; the smallest (first line, key) on a tie), ``firstLine`` (the smallest first
    line of its spans), ``closes`` (closing templates with their spans) and ``usualEnd``
    (``spans_usual_end``). A span is *unfinished* when its kind has a usual end and its own
    ``closes`` differs. ``kinds``: by (-unfinished, -spans, first line, signature), ``kinds`` of
    them. ``top``: the spans, or with ``unfinished_only`` the unfinished ones, in ``order``
    (``spans_order_key``), ``top`` of them; each names the example lines -- the first line of the
    log with that template -- of its ``opens`` and ``closes``."""
    share = spans_check_args(min_len, max_ids, order, min_lines, max_share, min_ms, kind_min_spans, close_share, top, kinds)
    raws = [line.encode("utf-8", errors="surrogateescape") for line in split_lines(_as_text(logs))]
    sigs = [line_signature(raw) for raw in raws]
    first_of: Dict[int, int] = {}
    for i, s in enumerate(sigs):
        first_of.setdefault(s, i)
    eff, now = [], None
    for raw in raws:
        t = line_timestamp(raw)
        now = now if t is None else t
        eff.append(now)
    per_line = [line_key_tokens(raw, min_len) for raw in raws]
    level = {k: span_level(k) for toks in per_line for k, _ in toks}
    shift = spans_shift(list(level.values()), max_ids)
    found: Dict[int, list] = {}         # key -> [lines, first, last, tmin, tmax, token]
    id_lines = pairs = 0
    for i, toks in enumerate(per_line):
        held = [(k, t) for k, t in toks if level[k] >= shift]
        id_lines += bool(held)
        pairs += len(held)
        for k, t in held:
            g = found.setdefault(k, [0, i, i, None, None, t])
            g[0] += 1
            g[2] = i
            if eff[i] is not None:
                g[3] = eff[i] if g[3] is None else min(g[3], eff[i])
                g[4] = eff[i] if g[4] is None else max(g[4], eff[i])
    out = spans_head(len(raws), sum(t is not None for t in eff), id_lines, pairs, len(found), min_len, max_ids, shift)
    dur = lambda g: None if g[3] is None else g[4] - g[3]
    listed = {k: g for k, g in found.items()
              if g[0] >= min_lines and g[0] <= max_share * len(raws)
              and ((dur(g) is None and min_ms == 0) or (dur(g) is not None and dur(g) >= min_ms))}
    out["listed"] = len(listed)
    hist = [0] * SPAN_BUCKETS
    by_kind: Dict[int, list] = {}
    for k, g in listed.items():
        if dur(g) is not None:
            hist[pause_bucket(dur(g))] += 1
        by_kind.setdefault(sigs[g[1]], []).append(k)
    out["durations"] = spans_durations(hist)
    usual: Dict[int, Optional[int]] = {}
    kind_rows = []
    for o, keys in by_kind.items():
        closes: Dict[int, int] = {}
        for k in keys:
            c = sigs[listed[k][2]]
            closes[c] = closes.get(c, 0) + 1
        usual[o] = u = spans_usual_end(closes, len(keys), kind_min_spans, share)
        unfinished = 0 if u is None else sum(1 for k in keys if sigs[listed[k][2]] != u)
        timed = [k for k in keys if dur(listed[k]) is not None]
        best = min(timed, key=lambda k: (-dur(listed[k]), listed[k][1], k)) if timed else None
        first_line = min(listed[k][1] for k in keys)
        kind_rows.append(((-unfinished, -len(keys), first_line, o),
                          (o, len(keys), len(timed), sum(dur(listed[k]) for k in timed),
                           None if best is None else dur(listed[best]),
                           None if best is None else listed[best][5].decode("ascii"),
                           None if best is None else listed[best][1], first_line, closes, u, unfinished,
                           {s: raws[first_of[s]] for s in [o] + list(closes)})))
    kind_rows.sort(key=lambda kv: kv[0])
    if kinds is not None:
        kind_rows = kind_rows[:max(0, kinds)]
    out["kinds"] = [spans_kind_row(*row) for _, row in kind_rows]

    def is_unfinished(k):
        u = usual[sigs[listed[k][1]]]
        return u is not None and sigs[listed[k][2]] != u

    rows = [k for k in listed if not unfinished_only or is_unfinished(k)]
    rows.sort(key=lambda k: spans_order_key(order, dur(listed[k]), listed[k][0], listed[k][1], k))
    if top is not None:
        rows = rows[:max(0, top)]
    for k in rows:
        n, first, last, tmin, tmax, tok = listed[k]
        out["top"].append(spans_row(k, tok, n, first, last, tmin, tmax, sigs[first], sigs[last], is_unfinished(k),
                                    usual[sigs[first]], raws[first_of[sigs[first]]], raws[first_of[sigs[last]]]))
    return out


# ---------------------------------------------------------------------------------------------
# Trace report (an extra, as the gap report): which stack traces does a log hold, how often, where
# first, with which root cause, and does any pattern explain them? These functions are the
# specification of ``log_parser_amd/traces.py`` and of the line classifier and the run scan
# (csrc/kernels/trace_core.h, traces.hip).
#
# The shape is the JVM's and Node's: the exception first, then ``at`` frames, ``Caused by:`` /
# ``Suppressed:`` lines and ``... n more``. Not covered: Python tracebacks (the exception comes
# last there), Go panics, and exception messages of several lines before the first frame (only
# the line just before the run is the head). The bounds of the regexes let the device classify a
# line from a bounded prefix.

TR_OTHER, TR_FRAME, TR_MORE, TR_CAUSE = 0, 1, 2, 3
TR_TOKEN_MAX = 256
_TR_FRAME = re.compile(rb"^[ \t]{1,64}at[ \t]")
_TR_MORE = re.compile(rb"^[ \t]{1,64}\.\.\.")
_TR_CAUSE = re.compile(rb"^[ \t]{0,64}(?:Caused by:|Suppressed:)[ \t]{0,8}([^: \t]{0,256})")
_TR_EXC = re.compile(rb"(?:[A-Za-z_$][\w$]*\.)*[A-Za-z_$][\w$]*(?:Exception|Error|Throwable)\b")
_TR_M = 0x9E3779B97F4A7C15
_M64 = 0xFFFFFFFFFFFFFFFF


def fmix64(h: int) -> int:
    """The finaliser of MurmurHash3 (``gt_hash`` of csrc/kernels/gap_table.h)."""
    h &= _M64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & _M64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & _M64
    return h ^ (h >> 33)


def fnv1a64(data: bytes) -> int:
    h = _FNV_OFFSET
    for c in data:
        h = ((h ^ c) * _FNV_PRIME) & _M64
    return h


def trace_class(line: bytes):
    """(class, cause token or None) of a line: the first of FRAME, MORE, CAUSE that matches, else OTHER."""
    if _TR_FRAME.match(line):
        return TR_FRAME, None
    if _TR_MORE.match(line):
        return TR_MORE, None
    m = _TR_CAUSE.match(line)
    if m:
        return TR_CAUSE, m.group(1)
    return TR_OTHER, None


def trace_element(line: bytes) -> Optional[int]:
    """What a run line contributes to its trace's signature: a frame its mixed template signature,
    a cause the mixed complement of its token's hash, anything else nothing."""
    cls, token = trace_class(line)
    if cls == TR_FRAME:
        return fmix64(line_signature(line))
    if cls == TR_CAUSE:
        return fmix64(~fnv1a64(token))
    return None


def trace_signature(run: Sequence[bytes]) -> int:
    """``fmix64(V ^ k)`` with ``V = sum(e_i * M^(k - i))`` (mod 2^64) over the k contributing lines
    of the run, in order. The head does not contribute; digits are normalised by the template, so
    a trace keeps its signature across line-number changes."""
    v = k = 0
    for line in run:
        e = trace_element(line)
        if e is not None:
            v = (v * _TR_M + e) & _M64
            k += 1
    return fmix64(v ^ k)


def traces(logs, pattern_sets: List[PatternSet], params: ScoringParams, top: Optional[int] = 20,
           order: str = "count", unexplained_only: bool = False) -> dict:
    """The trace report of ``logs``. A run is a maximal sequence of consecutive non-OTHER lines; a
    run with at least one FRAME is a trace, the line just before it its head (a run that starts
    the document is headless). Traces are grouped by ``trace_signature``; per group its traces
    (``count``), those with an event of ``analyze`` on the head or a run line (``eventTraces``),
    where it first appears, and the shape of its first trace. ``order="count"``: most frequent
    first (ties: first line); ``"first"``: by first line. ``unexplained_only`` lists only the
    groups without an event; the totals do not change."""
    if order not in ("count", "first"):
        raise ValueError("order must be 'count' or 'first'")
    logs = _as_text(logs)
    res = analyze(logs, pattern_sets, params, FrequencyTracker(params))
    lines = [x.encode("utf-8", errors="surrogateescape") for x in split_lines(logs)]
    on_event = {e["lineNumber"] - 1 for e in res["events"]}
    cls = [trace_class(x)[0] for x in lines]
    groups: Dict[int, dict] = {}
    n_traces = n_trace_lines = n_frames = n_unexplained = 0
    i, n = 0, len(lines)
    while i < n:
        if cls[i] == TR_OTHER:
            i += 1
            continue
        a = i
        while i < n and cls[i] != TR_OTHER:
            i += 1
        run = range(a, i)
        frames = [x for x in run if cls[x] == TR_FRAME]
        if not frames:
            continue
        causes = [x for x in run if cls[x] == TR_CAUSE]
        head = lines[a - 1] if a else None
        event = any(x in on_event for x in range(a - 1 if a else a, i))
        n_traces += 1
        n_trace_lines += len(run) + (a > 0)
        n_frames += len(frames)
        n_unexplained += not event
        g = groups.get(trace_signature(lines[a:i]))
        if g is None:
            exc = _TR_EXC.search(head) if head is not None else None
            g = groups[trace_signature(lines[a:i])] = {
                "count": 0, "eventTraces": 0, "firstLine": a if a else 1,
                "lines": len(run) + (a > 0), "frames": len(frames), "causes": len(causes),
                "head": head.decode("utf-8", errors="replace") if head is not None else None,
                "exception": exc.group().decode("utf-8", errors="replace") if exc else None,
                "topFrame": lines[frames[0]].strip(b" \t").decode("utf-8", errors="replace"),
                "rootCause": lines[causes[-1]].strip(b" \t").decode("utf-8", errors="replace") if causes else None}
        g["count"] += 1
        g["eventTraces"] += event
    listed = [kv for kv in groups.items() if not (unexplained_only and kv[1]["eventTraces"])]
    listed.sort(key=(lambda kv: (-kv[1]["count"], kv[1]["firstLine"])) if order == "count"
                else (lambda kv: kv[1]["firstLine"]))
    if top is not None:
        listed = listed[:max(0, int(top))]
    return {"totalLines": n, "events": len(res["events"]), "traces": n_traces, "traceLines": n_trace_lines,
            "frameLines": n_frames, "groups": len(groups), "unexplainedTraces": n_unexplained,
            "unexplainedGroups": sum(1 for g in groups.values() if not g["eventTraces"]),
            "top": [{"count": g["count"], "eventTraces": g["eventTraces"], "firstLine": g["firstLine"],
                     "signature": "%016x" % sig, "lines": g["lines"], "frames": g["frames"], "causes": g["causes"],
                     "head": g["head"], "exception": g["exception"], "topFrame": g["topFrame"],
                     "rootCause": g["rootCause"]} for sig, g in listed]}


# ------------------------------------------------------------------ literal prefilter oracle
def literal_candidates(lib, data: bytes, line_start):
    """Exact candidates of the literal prefilter (ops.kernels.prefilter) as a multiset of keys
    ``regex << 32 | line``: for every literal of ``lib.literals``, every (overlapping) occurrence in
    the ASCII-lower-cased text and every regex the literal belongs to, one key, where ``line`` is
    the index of the last ``line_start <= position``. Unordered: a ``collections.Counter``."""
    import collections

    import numpy as np
    low = bytes(data).lower()                       # ASCII only: bytes >= 0x80 stay as they are
    ls = np.asarray(line_start.cpu() if hasattr(line_start, "cpu") else line_start, dtype=np.int64)
    pf = lib.pf
    out: collections.Counter = collections.Counter()
    for i, lit in enumerate(lib.literals):
        pos = []
        p = low.find(lit)
        while p >= 0:
            pos.append(p)
            p = low.find(lit, p + 1)
        if not pos:
            continue
        lines = np.maximum(np.searchsorted(ls, np.array(pos, np.int64), side="right") - 1, 0)
        per_line = collections.Counter(lines.tolist())
        for r in pf["lit_reg"][int(pf["lit_reg_off"][i]):int(pf["lit_reg_off"][i + 1])]:
            for line, c in per_line.items():
                out[(int(r) << 32) | int(line)] += c
    return out


# ------------------------------------------------------------------ score oracle on hand-built tables
# The seven factors over HIT SETS instead of text: what proximity_factor, temporal_factor,
# context_factor, chronological_factor and FrequencyTracker.penalty above compute once "the regex
# finds line j" is replaced by "j is in the regex's set of lines" and the context regexes by a
# line's feature bits. Linear scans only; this is the specification of csrc/kernels/lp_core.h's
# score (host loop, k_score, request tail) on tables a test lays out by hand.

def exp_correctly_rounded(num: float, den: float) -> float:
    """The double nearest to exp(num / den), the quotient of the two doubles taken exactly (60
    digits, never rounded to a double first). ``Decimal.exp`` is correctly rounded at context
    precision; ``float()`` of a Decimal is the correctly rounded conversion."""
    import decimal
    with decimal.localcontext() as c:
        c.prec = 60
        return float((decimal.Decimal(num) / decimal.Decimal(den)).exp())


def score_reference(tables: dict, params: ScoringParams, events, carry):
    """Scores of ``events`` on hand-built tables, in plain Python.

    ``tables``:
      ``patterns``  list of dicts: ``conf``, ``sev`` (floats), ``context`` (``None`` = rules null,
                    else ``(lines_before, lines_after)``), ``secondaries`` (list of ``(regex,
                    window, weight)``, regex -1 = none, window already clamped to
                    ``max_window`` as the compiled library does) and ``sequences`` (list of ``(bonus,
                    [regex per event], [carry flag per event])``)
      ``hits``      per regex, the ``set`` of batch-local lines it matches
      ``feat``      per batch-local line, the context bits: 1 ERROR, 2 WARN, 4 stack frame, 8 exception
      ``segments``  list of ``(lo, hi, own_lo, g0, n)``: a document (or shard with its halo) holds the
                    batch-local lines ``[lo, hi)``; line ``lo`` is global line ``g0`` of an ``n``-line log;
                    a sequence chain searches back to ``own_lo`` and an event it misses there counts
                    as found exactly when its carry flag is set (the chain was completed by an
                    earlier shard)
    ``events``: list of ``(line, pattern, segment, rank, key)``; the frequency count before the event is
    ``carry[key] + rank``, and ``key`` -1 is a pattern without an id.

    Returns one dict per event: ``factors`` (confidence, severity, chronological, proximity,
    temporal, context, penalty), ``score`` (their left-to-right product, ScoringService.java:102-109)
    and ``prox_terms`` (the ``(weight, distance)`` of every secondary that counted). The proximity
    factor uses ``exp_correctly_rounded``; everything else is the double arithmetic of the functions
    above."""
    hits = [set(h) for h in tables["hits"]]
    feat = tables["feat"]
    out = []
    for x, p, s, rank, key in events:
        pat = tables["patterns"][p]
        lo, hi, own_lo, g0, n = tables["segments"][s]
        chrono = chronological_factor(g0 + (x - lo), n, params)

        prox, terms = 1.0, []
        if pat["secondaries"]:
            total = 0.0
            for r, w, weight in pat["secondaries"]:
                near = [abs(j - x) for j in range(max(lo, x - w), min(hi, x + w + 1))
                        if j != x and r >= 0 and j in hits[r]]
                if near:
                    d = float(min(near))
                    total += weight * exp_correctly_rounded(-d, params.decay_constant)
                    terms.append((weight, d))
            prox = 1.0 + total

        temp = 1.0
        if pat["sequences"]:
            total = 0.0
            for bonus, regs, flags in pat["sequences"]:
                if not regs:
                    continue
                last = regs[-1]
                if not any(last >= 0 and j in hits[last] for j in range(max(lo, x - 5), min(hi, x + 5 + 1))):
                    continue
                ok, cursor = True, x
                for k in range(len(regs) - 2, -1, -1):
                    found = -1
                    for j in range(cursor - 1, own_lo - 1, -1):
                        if regs[k] >= 0 and j in hits[regs[k]]:
                            found = j
                            break
                    if found < 0:
                        ok = bool(flags[k])
                        break
                    cursor = found
                if ok:
                    total += bonus
            temp = 1.0 + total

        window = [x]
        if pat["context"] is not None:
            before, after = pat["context"]
            window = list(range(max(lo, x - max(0, before)), min(hi, x + 1 + max(0, after))))
        sc, err, stack = 0.0, 0, 0
        for j in window:
            f = feat[j]
            if f & 1:
                err += 1
                sc += 0.4
            elif f & 2:
                sc += 0.2
            if f & 4:
                stack += 1
                sc += 0.1
            if f & 8:
                sc += 0.3
        if stack > 0:
            sc += min(stack * 0.1, 0.5)
        if len(window) > 10 and (stack + err) > len(window) * 0.7:
            sc *= 0.8
        ctx = min(1.0 + sc, params.max_context_factor)

        pen = 0.0
        if key >= 0:
            rate = (carry[key] + rank) / float(params.freq_window_hours)
            if rate > params.freq_threshold:
                pen = min(params.freq_max_penalty, (rate - params.freq_threshold) / params.freq_threshold)

        conf, sev = pat["conf"], pat["sev"]
        out.append({"factors": [conf, sev, chrono, prox, temp, ctx, pen],
                    "score": conf * sev * chrono * prox * temp * ctx * (1.0 - pen),
                    "prox_terms": terms})
    return out
