"""In-process API: the engine embedded in a Python program, without the HTTP front end.

The reference exposes its analysis only through ``POST /parse`` (``Parse.java:41-61`` ->
``AnalysisService.analyze``) and keeps ``FrequencyTrackingService``'s statistics / reset methods
internal (``FrequencyTrackingService.java:101-134``). :class:`LogParser` offers the same analysis
to embedders, with what an in-process user needs beyond one call at a time:

* ``parse`` / ``parse_json``: one document, synchronously (the AnalysisResult dict / JSON bytes);
* ``submit``: thread-safe asynchronous analysis through the same continuous batcher the service
  uses (concurrent callers share device batches; the frequency window sees them in submission
  order) -- ``Future`` of the JSON bytes;
* ``parse_file``: a log file of any size -- whole-document analysis below the stream threshold,
  otherwise an mmap'd chunked stream (summary + top-k, bounded memory);
* ``load_resident`` / ``analyze_resident``: a multi-GB log held in HBM and re-analysed (with this
  or another parser's library) without crossing PCIe again;
* ``validate``: the library's compile report (regex kinds, invalid / host-fallback regexes) that
  the reference would only discover as HTTP 500s, request by request (AnalysisService.java:64);
* ``gaps`` / ``gaps_file``: the error lines of a log that no pattern of the library explains,
  grouped by line template -- what the library does not cover yet; ``gaps_stream`` /
  ``gaps_resident`` for one log too large for one piece, ``gaps_corpus`` / ``gap_accumulator``
  for many documents (which templates are most common across them, and in how many);
* ``timeline`` / ``timeline_file``: when the lines, error lines and events of a log happened --
  the stamps of the lines read on the device, counts per time bucket; ``timeline_stream`` /
  ``timeline_resident`` for one log too large for one piece;
* ``baseline`` / ``novelty`` / ``novelty_file``: the lines of a log whose template a baseline of
  healthy logs never showed, grouped by template; ``novelty_stream`` / ``novelty_resident`` for
  one log too large for one piece;
* ``traces`` / ``traces_file``: the stack traces of a log grouped by their frames and causes --
  how often, where first, the root cause, whether an event explains them; ``traces_stream`` /
  ``traces_resident`` for one log too large for one piece;
* ``leadup`` / ``leadup_file``: the line templates that lie within a window of lines before the
  events of a log more often than elsewhere -- what the log said just before each failure;
  ``leadup_stream`` / ``leadup_resident`` for one log too large for one piece,
  ``leadup_accumulator`` for a log that arrives over time;
* ``correlate`` / ``correlate_file``: the ids (request ids, trace ids, pod hashes, addresses) on
  the event lines of a log, followed through the whole log -- ``golden.correlate``;
  ``correlate_stream`` / ``correlate_resident`` for one log too large for one piece (the source
  is walked twice);
* ``values`` / ``values_file``: the numeric fields of the line templates of a log -- count, sum,
  min, max and where the largest value is -- ``golden.values``; ``values_stream`` /
  ``values_resident`` for one log too large for one piece, ``value_accumulator`` for a log that
  arrives over time;
* ``variants`` / ``variants_file``: the values that the variable tokens of the line templates of
  a log take -- per template and field its distinct tokens with count, first and last line, the
  field with one deviant among thousands first -- ``golden.variants``; ``variants_stream`` /
  ``variants_resident`` for one log too large for one piece, ``variant_accumulator`` for a log
  that arrives over time;
* ``trends`` / ``trends_file``: the line templates of a log that started, stopped, surged or
  faded across a pivot in its own time -- ``golden.trends``; ``trends_stream`` /
  ``trends_resident`` for one log too large for one piece, ``trend_accumulator`` for a log that
  arrives over time;
* ``pauses`` / ``pauses_file``: where a log went silent -- the steps between its stamped lines, the
  long ones with the lines around them and grouped by the template in front of them --
  ``golden.pauses``; ``pauses_stream`` / ``pauses_resident`` for one log too large for one piece,
  ``pause_accumulator`` for a log that arrives over time;
* ``cadence`` / ``cadence_file``: the line templates of a log that come at a steady beat, the
  beats they missed and the ones that stopped before the log ended -- ``golden.cadence``;
  ``cadence_stream`` / ``cadence_resident`` for one log too large for one piece,
  ``cadence_accumulator`` for a log that arrives over time;
* ``spans`` / ``spans_file``: the lifetimes of the ids of a log -- per id its lines, first and last
  line, duration and the templates it opens and closes on; the longest first, and the ones that
  never logged the line their kind usually ends on -- ``golden.spans``; ``spans_stream`` /
  ``spans_resident`` for one log too large for one piece, ``span_accumulator`` for a log that
  arrives over time;
* the frequency-tracking surface: ``pattern_frequency``, ``frequency_statistics``,
  ``reset_pattern_frequency``, ``reset_all_frequencies``.
"""
from __future__ import annotations

import contextlib
import json
import mmap
import os
import threading
from concurrent.futures import Future
from typing import List, Optional, Sequence

from .engine import Engine, resolve_device
from .frequency import FrequencyState
from .models.compiled import KIND_DFA, KIND_FALLBACK, KIND_INVALID, KIND_NFA, CompiledLibrary
from .models.library import load_pattern_directory
from .models.schema import PatternSet
from .utils.config import Config

_KIND_NAMES = {KIND_DFA: "dfa", KIND_NFA: "nfa", KIND_FALLBACK: "host-fallback", KIND_INVALID: "invalid"}


@contextlib.contextmanager
def _source(src_or_path):
    """A bytes-like source as it is; the file at a path as a read-only mmap (``b""`` when it is
    empty: nothing to map), closed on the way out."""
    if not isinstance(src_or_path, (str, os.PathLike)):
        yield src_or_path
    elif not os.path.getsize(src_or_path):
        yield b""
    else:
        with open(src_or_path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            yield mm


class LogParser:
    """``LogParser.from_directory(dir).parse(logs)`` -> AnalysisResult dict."""

    def __init__(self, pattern_sets: List[PatternSet], config: Optional[Config] = None,
                 device: Optional[str] = None, freq: Optional[FrequencyState] = None):
        self.config = config or Config.load()
        dev = resolve_device(device or self.config["engine.device"])
        self.library = CompiledLibrary(pattern_sets, self.config.scoring,
                                       max_dfa_states=int(self.config["engine.dfa-max-states"]),
                                       nfa_engine=str(self.config["engine.nfa-engine"]))
        self.engine = Engine(self.library, self.config, device=dev, freq=freq)
        self._batcher = None
        self._lock = threading.Lock()

    @classmethod
    def from_directory(cls, directory: str, **kw) -> "LogParser":
        return cls(load_pattern_directory(directory), **kw)

    # ---- analysis -----------------------------------------------------------------------------
    def parse(self, logs: str) -> dict:
        return json.loads(self.parse_json(logs))

    def parse_json(self, logs: str) -> bytes:
        if self._batcher is not None:         # the batcher owns the engine now: go through it
            return self._batcher.submit(logs).result()
        with self._lock:                      # the engine's staging buffers serve one batch at a time
            return self.engine.analyze_json(logs)

    def parse_batch(self, logs: Sequence[str]) -> List[dict]:
        """Several documents as ONE device batch (each keeps its own line numbering / N)."""
        with self._lock:
            return [json.loads(x) for x in self.engine.analyze_batch_json(list(logs))]

    def submit(self, logs: str) -> "Future[bytes]":
        """Asynchronous, thread-safe: the request joins the continuous batcher (serve/app.py) --
        concurrent submitters share device batches, in submission order."""
        if self._batcher is None:
            with self._lock:
                if self._batcher is None:
                    from .serve.app import Batcher
                    from .utils.metrics import Metrics
                    c = self.config
                    self._batcher = Batcher(self.engine, int(c["engine.batch.max-requests"]),
                                            int(c["engine.batch.max-bytes"]), float(c["engine.batch.max-wait-ms"]),
                                            Metrics())
        return self._batcher.submit(logs)

    def stream_threshold(self) -> int:
        """File size above which ``parse_file`` streams (StreamResult summary) instead of analysing
        one whole document (full AnalysisResult): ``engine.stream.threshold-bytes``, independent of
        the HBM-sized stream chunk, so the output format and host memory of a file do not depend
        on the GPU it runs on."""
        return int(self.config["engine.stream.threshold-bytes"])

    def parse_stream(self, data, chunk_bytes: Optional[int] = None, topk: int = 100, keep_events: bool = False):
        from .parallel.stream import StreamAnalyzer
        with self._lock:
            return StreamAnalyzer(self.engine, chunk_bytes=chunk_bytes, topk=topk, keep_events=keep_events).run(data)

    def parse_file(self, path: str, stream: Optional[bool] = None, topk: int = 20, raw: bool = False):
        """A log file: the AnalysisResult dict (``raw``: its JSON bytes) when it is below the stream
        threshold (or ``stream=False``), else a ``StreamResult`` of an mmap'd chunked pass."""
        if stream is None:
            stream = os.path.getsize(path) > self.stream_threshold()
        if stream:
            with _source(path) as mm:
                return self.parse_stream(mm, topk=topk)
        with open(path, "rb") as f:
            text = f.read().decode("utf-8", errors="surrogateescape")
        return self.parse_json(text) if raw else self.parse(text)

    def load_resident(self, data, chunk_bytes: Optional[int] = None):
        """Stage ``data`` into HBM once (``parallel.stream.ResidentLog``) for repeated analyses."""
        from .parallel.stream import ResidentLog
        return ResidentLog.load(data, self.engine, chunk_bytes=chunk_bytes)

    def analyze_resident(self, resident, topk: int = 100, keep_events: bool = False):
        from .parallel.stream import StreamAnalyzer
        with self._lock:
            return StreamAnalyzer(self.engine, chunk_bytes=resident.chunk_bytes, topk=topk,
                                  keep_events=keep_events).run(resident)

    # ---- library report -----------------------------------------------------------------------
    def gaps(self, logs, top: Optional[int] = 20, cover: str = "context") -> dict:
        """Coverage-gap report of one document (str or bytes): the error lines no pattern explains
        -- an error keyword or an exception class name, not a stack frame, outside every event
        (``cover="events"``) or every event's context window (``"context"``) -- grouped by line
        template, most frequent first (``top=None``: every group). ``Engine.gaps_bytes``; the
        frequency window is not touched."""
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("gaps"):
            return self.engine.gaps_bytes(logs, top=top, cover=cover)

    def gaps_file(self, path: str, top: Optional[int] = 20, cover: str = "context") -> dict:
        """``gaps`` of a log file, read as ONE document whatever its size (the stream threshold does
        not apply: the report has one format)."""
        with open(path, "rb") as f:
            return self.gaps(f.read(), top=top, cover=cover)

    @contextlib.contextmanager
    def _engine_guard(self, who: str = "gaps"):
        """The batcher guard and the lock of ``gaps``, around one use of the engine."""
        msg = who + ": the batcher owns the engine after submit(); use a parser of its own"
        if self._batcher is not None:
            raise RuntimeError(msg)
        with self._lock:
            if self._batcher is not None:
                raise RuntimeError(msg)
            yield

    def gap_accumulator(self, cover: str = "context"):
        """A ``gapreport.GapAccumulator`` on this parser's engine for callers that feed documents
        over time (``add_document`` / ``add_stream`` / ``add_resident``, then ``report``); each of
        its calls runs under the batcher guard and the lock of ``gaps``."""
        from .gapreport import GapAccumulator
        with self._engine_guard("gap_accumulator"):
            return GapAccumulator(self.engine, cover=cover, guard=self._engine_guard)

    def gaps_stream(self, src_or_path, chunk_bytes: Optional[int] = None, top: Optional[int] = 20,
                    cover: str = "context") -> dict:
        """``gaps`` of ONE large log processed in line-aligned chunks with halos (the chunks of
        ``parse_stream``): a bytes-like source, or the path of a file (mmap'd as ``parse_file``
        does). The report is exactly the one-document report, whatever the chunk size."""
        acc = self.gap_accumulator(cover)
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(top)

    def gaps_resident(self, resident, top: Optional[int] = 20, cover: str = "context") -> dict:
        """``gaps`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.gaps_stream(resident, None, top, cover)       # (``_source`` passes a resident log through)

    def gaps_corpus(self, docs, top: Optional[int] = 20, cover: str = "context") -> dict:
        """Coverage-gap report of many documents (an iterable of str or bytes), each analysed on
        its own: the totals summed, ``documents``, and per group also ``documents`` (how many
        documents it occurs in) and ``firstDocument`` (0-based; ``firstLine`` counts within it).
        Exactly one document gives ``gaps`` of it. ``golden.gaps_corpus`` is the specification."""
        acc = self.gap_accumulator(cover)
        for d in docs:
            acc.add_document(d)
        return acc.report(top)

    # ---- log timeline -------------------------------------------------------------------------
    def timeline(self, logs, bucket_seconds: int = 60, max_buckets: int = 65536) -> dict:
        """When did what happen in one document (str or bytes)? The stamp at the head of every line
        (ISO-8601 / RFC 3339 shapes, UTC unless a zone follows) dates the line; a line without one
        takes the time of the nearest earlier stamped line. The report counts lines, error lines,
        events and the events' severities per bucket of ``bucket_seconds`` and names the first
        error line and the first and last event with their times. ValueError when the log spans
        more than ``max_buckets`` buckets. ``Engine.timeline_bytes``; ``golden.timeline`` is the
        specification; the frequency window is not touched."""
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("timeline"):
            return self.engine.timeline_bytes(logs, bucket_seconds=bucket_seconds, max_buckets=max_buckets)

    def timeline_file(self, path: str, bucket_seconds: int = 60, max_buckets: int = 65536) -> dict:
        """``timeline`` of a log file, read as ONE document whatever its size."""
        with open(path, "rb") as f:
            return self.timeline(f.read(), bucket_seconds=bucket_seconds, max_buckets=max_buckets)

    def _timeline_accumulator(self, bucket_seconds: int, max_buckets: int):
        from .timeline import TimelineAccumulator
        with self._engine_guard("timeline"):
            return TimelineAccumulator(self.engine, bucket_seconds, max_buckets,
                                       guard=lambda: self._engine_guard("timeline"))

    def timeline_stream(self, src_or_path, chunk_bytes: Optional[int] = None, bucket_seconds: int = 60,
                        max_buckets: int = 65536) -> dict:
        """``timeline`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). The report is
        exactly the one-document report, whatever the chunk size."""
        acc = self._timeline_accumulator(bucket_seconds, max_buckets)
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report()

    def timeline_resident(self, resident, bucket_seconds: int = 60, max_buckets: int = 65536) -> dict:
        """``timeline`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.timeline_stream(resident, None, bucket_seconds, max_buckets)

    # ---- novelty report -----------------------------------------------------------------------
    def baseline(self):
        """An empty ``novelty.Baseline`` on this parser's device: the template signatures of healthy
        logs (``add_document`` / ``add_file`` / ``add_stream`` / ``add_resident``, ``save``; each of
        its calls runs under the batcher guard and the lock of ``novelty``)."""
        from .novelty import Baseline
        with self._engine_guard("novelty"):
            return Baseline(self.engine, guard=lambda: self._engine_guard("novelty"))

    def load_baseline(self, path: str):
        """The ``novelty.Baseline`` saved at ``path`` (``Baseline.save``), on this parser's device."""
        from .novelty import Baseline
        with self._engine_guard("novelty"):
            return Baseline.load(path, self.engine, guard=lambda: self._engine_guard("novelty"))

    def novelty(self, logs, baseline, top: Optional[int] = 20, order: str = "count", errors_only: bool = False) -> dict:
        """What does one document (str or bytes) say that the healthy logs of ``baseline`` never
        said? The lines whose template signature the baseline does not hold, grouped by template:
        per group its lines, its error lines, the lines an event lies on, its first line and an
        example. ``order="count"``: most frequent first; ``"first"``: in order of first appearance.
        ``errors_only`` lists only the groups with error lines (the totals do not change);
        ``top=None``: every group. ``Engine.novelty_bytes``; ``golden.novelty`` is the
        specification; the frequency window is not touched."""
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("novelty"):
            return self.engine.novelty_bytes(logs, baseline, top=top, order=order, errors_only=errors_only)

    def novelty_file(self, path: str, baseline, top: Optional[int] = 20, order: str = "count",
                     errors_only: bool = False) -> dict:
        """``novelty`` of a log file, read as ONE document whatever its size."""
        with open(path, "rb") as f:
            return self.novelty(f.read(), baseline, top=top, order=order, errors_only=errors_only)

    def _novelty_accumulator(self, baseline):
        from .novelty import NoveltyAccumulator
        with self._engine_guard("novelty"):
            return NoveltyAccumulator(self.engine, baseline, guard=lambda: self._engine_guard("novelty"))

    def novelty_stream(self, src_or_path, baseline, chunk_bytes: Optional[int] = None, top: Optional[int] = 20,
                       order: str = "count", errors_only: bool = False) -> dict:
        """``novelty`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). The report is
        exactly the one-document report, whatever the chunk size."""
        from .novelty import check_order
        check_order(order)
        acc = self._novelty_accumulator(baseline)
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(top, order, errors_only)

    def novelty_resident(self, resident, baseline, top: Optional[int] = 20, order: str = "count",
                         errors_only: bool = False) -> dict:
        """``novelty`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.novelty_stream(resident, baseline, None, top, order, errors_only)

    # ---- trace report -------------------------------------------------------------------------
    def traces(self, logs, top: Optional[int] = 20, order: str = "count", unexplained_only: bool = False) -> dict:
        """Which stack traces does one document (str or bytes) hold? Runs of ``at`` frames,
        ``Caused by:`` / ``Suppressed:`` lines and ``... n more`` (the JVM's and Node's shape),
        grouped by their frames and cause classes -- line numbers do not matter: per group how many
        traces, how many of them an event lies on, where it first appears, and of its first trace
        the head, the exception named there, the top frame and the root cause. ``order="count"``:
        most frequent first; ``"first"``: in order of first appearance. ``unexplained_only`` lists
        only the groups no event lies on (the totals do not change); ``top=None``: every group.
        ``Engine.traces_bytes``; ``golden.traces`` is the specification; the frequency window is
        not touched."""
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("traces"):
            return self.engine.traces_bytes(logs, top=top, order=order, unexplained_only=unexplained_only)

    def traces_file(self, path: str, top: Optional[int] = 20, order: str = "count",
                    unexplained_only: bool = False) -> dict:
        """``traces`` of a log file, read as ONE document whatever its size."""
        with open(path, "rb") as f:
            return self.traces(f.read(), top=top, order=order, unexplained_only=unexplained_only)

    def _trace_accumulator(self):
        from .traces import TraceAccumulator
        with self._engine_guard("traces"):
            return TraceAccumulator(self.engine, guard=lambda: self._engine_guard("traces"))

    def traces_stream(self, src_or_path, chunk_bytes: Optional[int] = None, top: Optional[int] = 20,
                      order: str = "count", unexplained_only: bool = False) -> dict:
        """``traces`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). A trace may straddle
        any number of chunks; the report is exactly the one-document report, whatever the chunk
        size."""
        from .novelty import check_order
        check_order(order)
        acc = self._trace_accumulator()
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(top, order, unexplained_only)

    def traces_resident(self, resident, top: Optional[int] = 20, order: str = "count",
                        unexplained_only: bool = False) -> dict:
        """``traces`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.traces_stream(resident, None, top, order, unexplained_only)

    # ---- lead-up report -----------------------------------------------------------------------
    def leadup(self, logs, window: int = 50, top: Optional[int] = 20, order: str = "share", min_count: int = 2) -> dict:
        """What does one document (str or bytes) say just before its failures that it does not
        usually say? A line is in the lead-up when an event lies on one of the ``window`` (1..4096)
        lines after it. The lines are grouped by template: per group its lines in the lead-up
        (``count``), all its lines (``total``), ``share`` = count / total, ``lift`` = share against
        the lead-up's share of all lines, its first lead-up line and that line as the example.
        Listed are the groups with ``count >= min_count``: ``order="share"`` by share, then count;
        ``"count"``: most frequent first; ``"first"``: in order of first appearance; ``top=None``:
        every group. ``Engine.leadup_bytes``; ``golden.leadup`` is the specification; the frequency
        window is not touched."""
        from .leadup import check_args
        check_args(window, order, min_count)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("leadup"):
            return self.engine.leadup_bytes(logs, window=window, top=top, order=order, min_count=min_count)

    def leadup_file(self, path: str, window: int = 50, top: Optional[int] = 20, order: str = "share",
                    min_count: int = 2) -> dict:
        """``leadup`` of a log file, read as ONE document whatever its size."""
        from .leadup import check_args
        check_args(window, order, min_count)
        with open(path, "rb") as f:
            return self.leadup(f.read(), window=window, top=top, order=order, min_count=min_count)

    def leadup_accumulator(self, window: int = 50):
        """A ``leadup.LeadupAccumulator`` on this parser's engine for a log that arrives over time
        (``add_document`` / ``add_stream`` / ``add_resident`` continue ONE log, then ``report``);
        each of its calls runs under the batcher guard and the lock of ``leadup``."""
        from .leadup import LeadupAccumulator
        with self._engine_guard("leadup"):
            return LeadupAccumulator(self.engine, window, guard=lambda: self._engine_guard("leadup"))

    def leadup_stream(self, src_or_path, chunk_bytes: Optional[int] = None, window: int = 50, top: Optional[int] = 20,
                      order: str = "share", min_count: int = 2) -> dict:
        """``leadup`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). The tail of a chunk
        can lie in the lead-up of the next chunk's event; the report is exactly the one-document
        report, whatever the chunk size."""
        from .leadup import check_args
        check_args(window, order, min_count)
        acc = self.leadup_accumulator(window)
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(top, order, min_count)

    def leadup_resident(self, resident, window: int = 50, top: Optional[int] = 20, order: str = "share",
                        min_count: int = 2) -> dict:
        """``leadup`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.leadup_stream(resident, None, window, top, order, min_count)

    # ---- values report -----------------------------------------------------------------------
    def values(self, logs, top: Optional[int] = 20, order: str = "peak", min_count: int = 5, min_fill: float = 0.9,
               varying: bool = True) -> dict:
        """Which numbers do the line templates of one document (str or bytes) carry, and where do
        they peak? The digit-holding tokens of a line behind its stamp are its *fields*, numbered
        in byte order (the first 8 count); a field has a value where its token is up to nine digits
        and up to three unit letters (``12``, ``31874ms``, ``512MB``). Per template and field:
        ``count``, ``sum``, ``min``, ``max``, ``mean``, ``peak`` = max / mean, ``maxLine`` (the
        first line that holds the max), first and last line with their values, ``lines`` (all
        lines of the template), ``fill`` = count / lines, and the first line as the example.
        Listed are the fields with ``count >= min_count`` and ``count >= min_fill * lines`` (a hex
        or id field only now and then looks like a number) and, with ``varying``, ``min < max``.
        ``order="peak"``: the largest value in units of the mean first; ``"max"``: largest value
        first; ``"count"``: most values first; ``"first"``: in order of first appearance;
        ``top=None``: every field. No pattern takes part. ``Engine.values_bytes``;
        ``golden.values`` is the specification; the frequency window is not touched."""
        from .values import check_args
        check_args(order, min_count, min_fill)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("values"):
            return self.engine.values_bytes(logs, top=top, order=order, min_count=min_count, min_fill=min_fill,
                                            varying=varying)

    def values_file(self, path: str, top: Optional[int] = 20, order: str = "peak", min_count: int = 5,
                    min_fill: float = 0.9, varying: bool = True) -> dict:
        """``values`` of a log file, read as ONE document whatever its size."""
        from .values import check_args
        check_args(order, min_count, min_fill)
        with open(path, "rb") as f:
            return self.values(f.read(), top=top, order=order, min_count=min_count, min_fill=min_fill, varying=varying)

    def value_accumulator(self, line_base: int = 0):
        """A ``values.ValueAccumulator`` on this parser's engine for a log that arrives over time
        (``add_document`` / ``add_stream`` / ``add_resident`` continue ONE log, then ``report``);
        each of its calls runs under the batcher guard and the lock of ``values``."""
        from .values import ValueAccumulator
        with self._engine_guard("values"):
            return ValueAccumulator(self.engine, guard=lambda: self._engine_guard("values"), line_base=line_base)

    def values_stream(self, src_or_path, chunk_bytes: Optional[int] = None, top: Optional[int] = 20,
                      order: str = "peak", min_count: int = 5, min_fill: float = 0.9, varying: bool = True) -> dict:
        """``values`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). A field belongs to
        one line, so the report is exactly the one-document report, whatever the chunk size."""
        from .values import check_args
        check_args(order, min_count, min_fill)
        acc = self.value_accumulator()
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(top, order, min_count, min_fill, varying)

    def values_resident(self, resident, top: Optional[int] = 20, order: str = "peak", min_count: int = 5,
                        min_fill: float = 0.9, varying: bool = True) -> dict:
        """``values`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.values_stream(resident, None, top, order, min_count, min_fill, varying)

    # ---- variants report ---------------------------------------------------------------------
    def variants(self, logs, max_distinct: int = 64, top: Optional[int] = 20, order: str = "odd", min_count: int = 5,
                 min_fill: float = 0.9, varying: bool = True, show: int = 5) -> dict:
        """Which values do the variable tokens of the line templates of one document (str or
        bytes) take, how often, and which is the odd one out? The fields are those of ``values``
        (the digit-holding tokens of a line behind its stamp, the first 8), counted whether or not
        they read as numbers; a value is the token as it is. A field with at most ``max_distinct``
        (2..4096) values over the whole log is listed with ``count``, ``lines``, ``fill``,
        ``distinct``, ``odd`` (its lines that do not hold the most common value), ``oddShare`` and
        its ``values`` -- all of them up to ``2 * show``, else the ``show`` most and least common
        -- each with ``token``, ``count``, ``share``, ``firstLine``, ``lastLine``; a field with more
        (an id, a counter) is only counted in ``unboundedFields``. Listed are the fields with
        ``count >= min_count``, ``count >= min_fill * lines`` and, with ``varying``, more than one
        value. ``order="odd"``: the smallest ``oddShare`` first; ``"count"``; ``"distinct"``;
        ``"first"``; ``top=None``: every field. No pattern takes part. ``Engine.variants_bytes``;
        ``golden.variants`` is the specification; the frequency window is not touched."""
        from .variants import check_args
        check_args(max_distinct, order, min_count, min_fill, show)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("variants"):
            return self.engine.variants_bytes(logs, max_distinct=max_distinct, top=top, order=order,
                                              min_count=min_count, min_fill=min_fill, varying=varying, show=show)

    def variants_file(self, path: str, max_distinct: int = 64, top: Optional[int] = 20, order: str = "odd",
                      min_count: int = 5, min_fill: float = 0.9, varying: bool = True, show: int = 5) -> dict:
        """``variants`` of a log file, read as ONE document whatever its size."""
        from .variants import check_args
        check_args(max_distinct, order, min_count, min_fill, show)
        with open(path, "rb") as f:
            return self.variants(f.read(), max_distinct, top, order, min_count, min_fill, varying, show)

    def variant_accumulator(self, max_distinct: int = 64, line_base: int = 0):
        """A ``variants.VariantAccumulator`` on this parser's engine for a log that arrives over
        time (``add_document`` / ``add_stream`` / ``add_resident`` continue ONE log, then
        ``report``); each of its calls runs under the batcher guard and the lock of ``variants``.
        ``max_distinct`` is fixed here."""
        from .variants import VariantAccumulator
        with self._engine_guard("variants"):
            return VariantAccumulator(self.engine, max_distinct, guard=lambda: self._engine_guard("variants"),
                                      line_base=line_base)

    def variants_stream(self, src_or_path, chunk_bytes: Optional[int] = None, max_distinct: int = 64,
                        top: Optional[int] = 20, order: str = "odd", min_count: int = 5, min_fill: float = 0.9,
                        varying: bool = True, show: int = 5) -> dict:
        """``variants`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). Exactly the
        one-document report, whatever the chunk size (variants.py says why)."""
        from .variants import check_args
        check_args(max_distinct, order, min_count, min_fill, show)
        acc = self.variant_accumulator(max_distinct)
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(top, order, min_count, min_fill, varying, show)

    def variants_resident(self, resident, max_distinct: int = 64, top: Optional[int] = 20, order: str = "odd",
                          min_count: int = 5, min_fill: float = 0.9, varying: bool = True, show: int = 5) -> dict:
        """``variants`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.variants_stream(resident, None, max_distinct, top, order, min_count, min_fill, varying, show)

    # ---- spans report ------------------------------------------------------------------------
    def spans(self, logs, min_len: int = 8, max_ids: int = 1 << 22, top: Optional[int] = 20, order: str = "duration",
              unfinished_only: bool = False, min_lines: int = 2, max_share: float = 0.25, min_ms: int = 0,
              kind_min_spans: int = 5, close_share=0.8, kinds: Optional[int] = 10) -> dict:
        """The lifetimes of the ids of one document (str or bytes): which request, job, trace or
        connection took longest, and which started like all the others and never logged the line
        the others end on? An id is a key token of ``correlate`` (``min_len``..64 letters and
        digits with a digit, case folded; the first 8 of a line); its *span* is every line that
        holds it: ``lines``, ``firstLine`` / ``lastLine``, ``start`` / ``end`` (the smallest and
        largest time of its lines, a line's time being the stamp of the nearest stamped line at or
        before it), ``durationMs``, and ``opens`` / ``closes``, the templates of its first and last
        line. Listed are the spans with ``lines >= min_lines``, ``lines <= max_share *
        totalLines`` (a host name on every line is no id) and ``durationMs >= min_ms``. Spans
        that open alike are a *kind*; a kind of at least ``kind_min_spans`` spans of which a
        share of ``close_share`` close on one template has that template as its *usual end*, and a
        span of the kind that closes otherwise is *unfinished*. ``kinds``: the kinds, those with
        unfinished spans first; ``top``: the spans (``unfinished_only``: only those) by
        ``order="duration"``, ``"lines"`` or ``"first"``. At most ``max_ids`` (16..2^26) ids are
        kept: above that the report is one of a hash sample of the ids (``sampleShift``). No
        pattern takes part. ``Engine.spans_bytes``; ``golden.spans`` is the specification; the
        frequency window is not touched."""
        from .spans import check_args
        check_args(min_len, max_ids, order, min_lines, max_share, min_ms, kind_min_spans, close_share, top, kinds)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("spans"):
            return self.engine.spans_bytes(logs, min_len=min_len, max_ids=max_ids, top=top, order=order,
                                           unfinished_only=unfinished_only, min_lines=min_lines, max_share=max_share,
                                           min_ms=min_ms, kind_min_spans=kind_min_spans, close_share=close_share,
                                           kinds=kinds)

    def spans_file(self, path: str, min_len: int = 8, max_ids: int = 1 << 22, **report) -> dict:
        """``spans`` of a log file, read as ONE document whatever its size (``report``: the other
        parameters of ``spans``)."""
        from .spans import check_args
        check_args(min_len, max_ids, **{k: v for k, v in report.items() if k != "unfinished_only"})
        with open(path, "rb") as f:
            return self.spans(f.read(), min_len, max_ids, **report)

    def span_accumulator(self, min_len: int = 8, max_ids: int = 1 << 22):
        """A ``spans.SpanAccumulator`` on this parser's engine for a log that arrives over time
        (``add_document`` / ``add_stream`` / ``add_resident`` continue ONE log, then ``report``);
        each of its calls runs under the batcher guard and the lock of ``spans``. ``min_len`` and
        ``max_ids`` are fixed here."""
        from .spans import SpanAccumulator
        with self._engine_guard("spans"):
            return SpanAccumulator(self.engine, min_len, max_ids, guard=lambda: self._engine_guard("spans"))

    def spans_stream(self, src_or_path, chunk_bytes: Optional[int] = None, min_len: int = 8, max_ids: int = 1 << 22,
                     **report) -> dict:
        """``spans`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). Exactly the
        one-document report, whatever the chunk size (spans.py says why)."""
        from .spans import check_args
        check_args(min_len, max_ids, **{k: v for k, v in report.items() if k != "unfinished_only"})
        acc = self.span_accumulator(min_len, max_ids)
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(**report)

    def spans_resident(self, resident, min_len: int = 8, max_ids: int = 1 << 22, **report) -> dict:
        """``spans`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.spans_stream(resident, None, min_len, max_ids, **report)

    # ---- trends report -----------------------------------------------------------------------
    def trends(self, logs, bucket_seconds: int = 60, at=None, ratio: int = 4, min_count: int = 5,
               kind: Optional[str] = None, order: str = "change", top: Optional[int] = 20,
               max_buckets: int = 65536) -> dict:
        """What changed over the time of one document (str or bytes)? Lines are counted per
        template and time bucket of ``bucket_seconds`` (a line without a stamp takes the time of
        the nearest earlier stamped line); a pivot bucket splits the span of the log: the middle
        (``at=None``), the bucket of ``at`` (epoch milliseconds or a timestamp), or that of the
        timeline's ``"first-event"`` / ``"first-error"``. A template with no dated line before the
        pivot ``started``, with none from it on ``stopped``; one whose rate per bucket rose or fell
        by the factor ``ratio`` (an integer >= 2) ``surged`` or ``faded``; the others are
        ``steady``. Listed are the templates with ``datedLines >= min_count`` of the kind ``kind``
        (None: all but steady; ``"all"``), ``order="change"``: largest change of rate first;
        ``"count"``: most dated lines first; ``"first"``: in order of first appearance;
        ``top=None``: every template. No pattern and no baseline takes part, except for the two
        named pivots. ``Engine.trends_bytes``; ``golden.trends`` is the specification; the
        frequency window is not touched."""
        from .trends import check_args
        check_args(bucket_seconds, at, ratio, min_count, kind, order, max_buckets)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("trends"):
            return self.engine.trends_bytes(logs, bucket_seconds=bucket_seconds, at=at, ratio=ratio, min_count=min_count,
                                            kind=kind, order=order, top=top, max_buckets=max_buckets)

    def trends_file(self, path: str, bucket_seconds: int = 60, at=None, ratio: int = 4, min_count: int = 5,
                    kind: Optional[str] = None, order: str = "change", top: Optional[int] = 20,
                    max_buckets: int = 65536) -> dict:
        """``trends`` of a log file, read as ONE document whatever its size."""
        from .trends import check_args
        check_args(bucket_seconds, at, ratio, min_count, kind, order, max_buckets)
        with open(path, "rb") as f:
            return self.trends(f.read(), bucket_seconds=bucket_seconds, at=at, ratio=ratio, min_count=min_count,
                               kind=kind, order=order, top=top, max_buckets=max_buckets)

    def trend_accumulator(self, bucket_seconds: int = 60):
        """A ``trends.TrendAccumulator`` on this parser's engine for a log that arrives over time
        (``add_document`` / ``add_stream`` / ``add_resident`` continue ONE log, then ``report``);
        each of its calls runs under the batcher guard and the lock of ``trends``."""
        from .trends import TrendAccumulator
        with self._engine_guard("trends"):
            return TrendAccumulator(self.engine, bucket_seconds, guard=lambda: self._engine_guard("trends"))

    def trends_stream(self, src_or_path, chunk_bytes: Optional[int] = None, bucket_seconds: int = 60, at=None,
                      ratio: int = 4, min_count: int = 5, kind: Optional[str] = None, order: str = "change",
                      top: Optional[int] = 20, max_buckets: int = 65536) -> dict:
        """``trends`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). The effective time
        of a chunk's last line is carried into the next; the report is exactly the one-document
        report, whatever the chunk size. A named pivot reads the source a second time, for its
        timeline."""
        from .trends import check_args, trends_stream
        check_args(bucket_seconds, at, ratio, min_count, kind, order, max_buckets)
        with _source(src_or_path) as src, self._engine_guard("trends"):
            return trends_stream(self.engine, src, chunk_bytes, bucket_seconds, at, ratio, min_count, kind, order, top,
                                 max_buckets)

    def trends_resident(self, resident, bucket_seconds: int = 60, at=None, ratio: int = 4, min_count: int = 5,
                        kind: Optional[str] = None, order: str = "change", top: Optional[int] = 20,
                        max_buckets: int = 65536) -> dict:
        """``trends`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.trends_stream(resident, None, bucket_seconds, at, ratio, min_count, kind, order, top, max_buckets)

    # ---- pauses report -----------------------------------------------------------------------
    def pauses(self, logs, min_ms: int = 1000, by: str = "before", order: str = "total", min_count: int = 1,
               top: Optional[int] = 20) -> dict:
        """Where did one document (str or bytes) go silent, and after which line templates? The
        step between two neighbouring stamped lines is the later stamp minus the earlier; a step
        below 0 is only counted (``backwardSteps``), a step of at least ``min_ms`` milliseconds is
        a pause. The head holds the counts, the exact sum ``pausedMs`` and its share of the log's
        span; ``intervals`` the steps >= 0 by size (bucket b holds ``[2^(b-1), 2^b)`` ms): the
        log's usual cadence next to its outliers; ``longest`` the ``top`` pauses with the line
        before and the line after; ``templates`` the pauses grouped by the template of the line
        before them (``by="before"``: what was running when it went quiet) or after them
        (``"after"``: what woke up), with ``pauses``, ``lines``, ``share``, ``totalMs``,
        ``maxMs``, ``maxLine``, ``firstLine`` and an example; groups below ``min_count`` pauses
        are dropped. ``order``: ``"total"`` (most paused time first), ``"max"``, ``"count"``,
        ``"share"`` or ``"first"``; ``top=None``: every pause and every template. No pattern
        takes part. ``Engine.pauses_bytes``; ``golden.pauses`` is the specification; the
        frequency window is not touched."""
        from .pauses import check_args, check_top
        check_args(min_ms, by, order, min_count)
        check_top(top)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("pauses"):
            return self.engine.pauses_bytes(logs, min_ms=min_ms, by=by, order=order, min_count=min_count, top=top)

    def pauses_file(self, path: str, min_ms: int = 1000, by: str = "before", order: str = "total", min_count: int = 1,
                    top: Optional[int] = 20) -> dict:
        """``pauses`` of a log file, read as ONE document whatever its size."""
        from .pauses import check_args, check_top
        check_args(min_ms, by, order, min_count)
        check_top(top)
        with open(path, "rb") as f:
            return self.pauses(f.read(), min_ms=min_ms, by=by, order=order, min_count=min_count, top=top)

    def pause_accumulator(self, min_ms: int = 1000, by: str = "before", longest: Optional[int] = 20):
        """A ``pauses.PauseAccumulator`` on this parser's engine for a log that arrives over time
        (``add_document`` / ``add_stream`` / ``add_resident`` continue ONE log, then ``report``);
        each of its calls runs under the batcher guard and the lock of ``pauses``. ``longest``:
        how many of the longest pauses it keeps (None: all), the limit of ``report(top=...)``."""
        from .pauses import PauseAccumulator
        with self._engine_guard("pauses"):
            return PauseAccumulator(self.engine, min_ms, by, longest, guard=lambda: self._engine_guard("pauses"))

    def pauses_stream(self, src_or_path, chunk_bytes: Optional[int] = None, min_ms: int = 1000, by: str = "before",
                      order: str = "total", min_count: int = 1, top: Optional[int] = 20) -> dict:
        """``pauses`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). The last stamped
        line of a chunk is carried into the next; the report is exactly the one-document report,
        whatever the chunk size."""
        from .pauses import check_args, check_top
        check_args(min_ms, by, order, min_count)
        acc = self.pause_accumulator(min_ms, by, check_top(top))
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(order, min_count, top)

    def pauses_resident(self, resident, min_ms: int = 1000, by: str = "before", order: str = "total",
                        min_count: int = 1, top: Optional[int] = 20) -> dict:
        """``pauses`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.pauses_stream(resident, None, min_ms, by, order, min_count, top)

    # ---- cadence report ----------------------------------------------------------------------
    def cadence(self, logs, min_ms: int = 1000, ratio: int = 4, min_count: int = 5, min_regularity=0.8,
                kind: Optional[str] = None, order: str = "gap", top: Optional[int] = 20) -> dict:
        """Which line templates of one document (str or bytes) come at a steady beat -- a
        heartbeat, a health check, a lease renewal -- and where did one go quiet while the rest of
        the log went on? The *beat* of a stamped line is its stamp minus the stamp of the previous
        stamped line of the same template; a beat below 0 is only counted (``backwardBeats``).
        Per template: ``typicalMs``, the mean of its beats but the largest; ``regularity``, the
        share of its beats within the best band a factor 4 wide (a periodic line scores about 1,
        random arrivals below 0.5). A template is periodic with at least ``min_count`` beats,
        ``typicalMs >= 1`` and ``regularity >= min_regularity``. It *missed* beats when its largest
        beat ``maxMs`` (``fromLine`` / ``toLine`` / ``from`` / ``to``) is at least ``max(min_ms,
        ratio * typicalMs)`` -- ``missedBeats`` says how many -- and it *stopped* when the time
        from its last line to the log's last stamped line (``overdueMs``) is. ``kind``: None (the
        templates that missed or stopped), ``"missed"``, ``"stopped"`` or ``"all"`` (the steady
        ones too); ``order``: ``"gap"`` (the largest hole in beats of its template first),
        ``"overdue"``, ``"count"`` or ``"first"``; ``top=None``: every one. The head counts the
        lines, the templates and the periodic / missed / stopped ones. No pattern takes part.
        ``Engine.cadence_bytes``; ``golden.cadence`` is the specification; the frequency window
        is not touched."""
        from .cadence import check_args, check_top
        check_args(min_ms, ratio, min_count, min_regularity, kind, order)
        check_top(top)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("pauses"):
            return self.engine.cadence_bytes(logs, min_ms=min_ms, ratio=ratio, min_count=min_count,
                                             min_regularity=min_regularity, kind=kind, order=order, top=top)

    def cadence_file(self, path: str, min_ms: int = 1000, ratio: int = 4, min_count: int = 5, min_regularity=0.8,
                     kind: Optional[str] = None, order: str = "gap", top: Optional[int] = 20) -> dict:
        """``cadence`` of a log file, read as ONE document whatever its size."""
        from .cadence import check_args, check_top
        check_args(min_ms, ratio, min_count, min_regularity, kind, order)
        check_top(top)
        with open(path, "rb") as f:
            return self.cadence(f.read(), min_ms, ratio, min_count, min_regularity, kind, order, top)

    def cadence_accumulator(self):
        """A ``cadence.CadenceAccumulator`` on this parser's engine for a log that arrives over
        time (``add_document`` / ``add_stream`` / ``add_resident`` continue ONE log, then
        ``report`` with the parameters of ``cadence``); each of its calls runs under the batcher
        guard and the lock of ``pauses``."""
        from .cadence import CadenceAccumulator
        with self._engine_guard("pauses"):
            return CadenceAccumulator(self.engine, guard=lambda: self._engine_guard("pauses"))

    def cadence_stream(self, src_or_path, chunk_bytes: Optional[int] = None, min_ms: int = 1000, ratio: int = 4,
                       min_count: int = 5, min_regularity=0.8, kind: Optional[str] = None, order: str = "gap",
                       top: Optional[int] = 20) -> dict:
        """``cadence`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). The templates' rows
        stay on the device between the chunks; the report is exactly the one-document report,
        whatever the chunk size."""
        from .cadence import check_args, check_top
        check_args(min_ms, ratio, min_count, min_regularity, kind, order)
        check_top(top)
        acc = self.cadence_accumulator()
        with _source(src_or_path) as src:
            acc.add_stream(src, chunk_bytes)
        return acc.report(min_ms, ratio, min_count, min_regularity, kind, order, top)

    def cadence_resident(self, resident, min_ms: int = 1000, ratio: int = 4, min_count: int = 5, min_regularity=0.8,
                         kind: Optional[str] = None, order: str = "gap", top: Optional[int] = 20) -> dict:
        """``cadence`` of a log held in HBM (``load_resident``), read in place chunk by chunk."""
        return self.cadence_stream(resident, None, min_ms, ratio, min_count, min_regularity, kind, order, top)

    # ---- correlation report ------------------------------------------------------------------
    def correlate(self, logs, min_len: int = 8, top: Optional[int] = 20, order: str = "events", min_lines: int = 2,
                  max_share: float = 0.25) -> dict:
        """What else does one document (str or bytes) say about the ids on its failing lines? A
        *key* is an id-like token of a line: a ``[0-9A-Za-z]`` run of ``min_len`` (4..64) to 64
        bytes that holds a digit, letters lowered -- a request id, a trace id, a pod hash, an
        address. Per key of an event line: the event lines holding it (``eventLines``), all lines
        holding it (``lines``), ``share`` = eventLines / lines, its first and last line, its first
        event line, and its first line as the example. Dropped are the keys on fewer than
        ``min_lines`` lines (an id seen only on its own event line) and on more than ``max_share``
        of all lines (a host name on every line). ``order="events"``: most event lines first, then
        most lines; ``"lines"``: most lines first; ``"first"``: in order of the first event line;
        ``top=None``: every key. ``Engine.correlate_bytes``; ``golden.correlate`` is the
        specification; the frequency window is not touched."""
        from .correlate import check_args
        check_args(min_len, order, min_lines, max_share)
        if isinstance(logs, str):
            logs = logs.encode("utf-8", errors="surrogateescape")
        with self._engine_guard("correlate"):
            return self.engine.correlate_bytes(logs, min_len=min_len, top=top, order=order, min_lines=min_lines,
                                               max_share=max_share)

    def correlate_file(self, path: str, min_len: int = 8, top: Optional[int] = 20, order: str = "events",
                       min_lines: int = 2, max_share: float = 0.25) -> dict:
        """``correlate`` of a log file, read as ONE document whatever its size."""
        from .correlate import check_args
        check_args(min_len, order, min_lines, max_share)
        with open(path, "rb") as f:
            return self.correlate(f.read(), min_len=min_len, top=top, order=order, min_lines=min_lines,
                                  max_share=max_share)

    def correlate_stream(self, src_or_path, chunk_bytes: Optional[int] = None, min_len: int = 8,
                         top: Optional[int] = 20, order: str = "events", min_lines: int = 2,
                         max_share: float = 0.25) -> dict:
        """``correlate`` of ONE large log processed in line-aligned chunks (the chunks of
        ``gaps_stream``): a bytes-like source, or the path of a file (mmap'd). The report walks its
        source TWICE -- first with the matchers for the ids of the event lines, then without them
        for every line that holds one of those ids -- so the source is uploaded twice and must not
        change in between; memory is bounded by the ids of the event lines, not by the ids of the
        log. The report is exactly the one-document report, whatever the chunk size."""
        from .correlate import check_args, correlate_stream
        check_args(min_len, order, min_lines, max_share)
        with _source(src_or_path) as src, self._engine_guard("correlate"):
            return correlate_stream(self.engine, src, chunk_bytes, min_len, top, order, min_lines, max_share)

    def correlate_resident(self, resident, min_len: int = 8, top: Optional[int] = 20, order: str = "events",
                           min_lines: int = 2, max_share: float = 0.25) -> dict:
        """``correlate`` of a log held in HBM (``load_resident``), read in place twice."""
        return self.correlate_stream(resident, None, min_len, top, order, min_lines, max_share)

    def validate(self, allow=("nfa",)) -> dict:
        """Compile report: library counts plus every regex that is invalid, routed to the host
        fallback, or of a kind not in ``allow``."""
        problems = []
        for r in self.library.regexes:
            name = _KIND_NAMES.get(r.kind, str(r.kind))
            if r.kind in (KIND_INVALID, KIND_FALLBACK) or (r.kind == KIND_NFA and "nfa" not in allow):
                problems.append({"regex": r.pattern, "kind": name, "error": r.error, "roles": sorted(r.roles)})
        return {"library": self.library.summary(), "problems": problems}

    # ---- frequency tracking (FrequencyTrackingService.java:101-134) ---------------------------
    @property
    def frequency(self) -> FrequencyState:
        return self.engine.freq

    def pattern_frequency(self, pattern_id: str) -> Optional[dict]:
        return self.engine.freq.get_pattern_frequency(pattern_id)

    def frequency_statistics(self) -> dict:
        return self.engine.freq.statistics()

    def reset_pattern_frequency(self, pattern_id: str) -> None:
        self.engine.freq.reset(pattern_id)

    def reset_all_frequencies(self) -> None:
        self.engine.freq.reset_all()

    def close(self) -> None:
        if self._batcher is not None:
            self._batcher.close()
            self._batcher = None
